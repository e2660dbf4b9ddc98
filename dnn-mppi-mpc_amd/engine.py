"""Thin object wrapper over the C ABI handle (one engine = one controller on one GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _dev_ptr(t):
    """Device pointer of a contiguous CUDA tensor (zero-copy hand-off to the C ABI)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("expected a contiguous CUDA tensor")
    return C.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(getattr(stream, "cuda_stream", stream))


class Engine:
    """Owns an ``mppi_handle``.  All arithmetic happens in libmppi_hip.so on the GPU."""

    def __init__(self, **cfg):
        self.lib = capi.load_library()
        c = capi.MppiConfig()
        c.struct_size = capi.config_size(self.lib)
        for k, v in cfg.items():
            if k in ("u_max", "sigma", "stage_cost_weight", "terminal_cost_weight"):
                arr = np.asarray(v, dtype=np.float64).reshape(-1)
                field = getattr(c, k)
                for i in range(len(field)):
                    field[i] = float(arr[i]) if i < arr.size else 0.0
            else:
                setattr(c, k, v)
        abi = self.lib.mppi_abi_version()
        if c.obstacle_motion and abi < 7:
            raise capi.MppiError(capi.ERR_UNSUPPORTED, "obstacle_motion needs a library of ABI version 7 or later")
        if c.fleet_radius != 0 and abi < 8:
            raise capi.MppiError(capi.ERR_UNSUPPORTED, "fleet_radius needs a library of ABI version 8 or later")
        self.cfg = c
        self.K, self.T = int(c.K), int(c.T)
        self.nx = 4 if c.model == capi.MODEL_RACECAR else 3
        # several independent problems in one handle: the state / control / cost accessors then carry a leading
        # [n_agents] axis and run_closed_loop advances all of them in one launch per stage
        self.n_agents = max(1, int(c.n_agents))
        self._lead = (self.n_agents,) if self.n_agents > 1 else ()
        self._h = capi._H()
        rc = self.lib.mppi_create(C.byref(c), C.byref(self._h))
        if rc != capi.OK:
            self._h = None
            capi.check(self.lib, None, rc)
        self.stats = capi.MppiStats()
        # buffers and ctypes arguments of the per-iteration call, built once (every `.ctypes.data_as` costs ~1 us)
        self._x0_buf = np.zeros(self.nx)
        self._u_buf, self._u0_buf = np.empty((self.T, 2)), np.empty(2)
        self._step_args = (_dp(self._x0_buf), _dp(self._u_buf), _dp(self._u0_buf), C.byref(self.stats))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mppi_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        capi.check(self.lib, self._h, rc)

    # -- configuration / state ----------------------------------------------------------------
    def set_ref_path(self, path, agent=None):
        """``agent``: None sets every agent of the handle (the shared scene), an index in [0, n_agents) that agent's own path."""
        p = np.ascontiguousarray(path, dtype=np.float64)
        if p.ndim != 2:
            raise ValueError("ref_path must be 2-D")
        if agent is None:
            self._ck(self.lib.mppi_set_ref_path(self._h, _dp(p), p.shape[0], p.shape[1]))
        else:
            self._ck(self.lib.mppi_set_agent_ref_path(self._h, int(agent), _dp(p), p.shape[0], p.shape[1]))

    def set_obstacles(self, circles, agent=None, velocities=None):
        """``agent``: as in `set_ref_path`; an agent given no circles collides with nothing.  ``velocities``: [m, 2] = vx, vy
        in metres per second, for a handle created with ``obstacle_motion=1`` (the learned model: ``2``) (the circles then stand where given at this
        call and move with the handle's iteration counter, see mppi_config.obstacle_motion); None: they stand still."""
        c = np.ascontiguousarray(circles, dtype=np.float64).reshape(-1, 3)
        if velocities is not None:
            v = np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1, 2)
            if v.shape[0] != c.shape[0]:
                raise ValueError("one velocity per circle")
            if agent is None:
                self._ck(self.lib.mppi_set_obstacles_moving(self._h, _dp(c), _dp(v), c.shape[0]))
            else:
                self._ck(self.lib.mppi_set_agent_obstacles_moving(self._h, int(agent), _dp(c), _dp(v), c.shape[0]))
        elif agent is None:
            self._ck(self.lib.mppi_set_obstacles(self._h, _dp(c), c.shape[0]))
        else:
            self._ck(self.lib.mppi_set_agent_obstacles(self._h, int(agent), _dp(c), c.shape[0]))

    def agent_circles(self, agent=0):
        """(circles[m, 3], velocities[m, 2]) that ``agent``'s next iteration tests: its own set, then -- on a handle created
        with ``fleet_radius > 0`` -- one circle per mate in ascending agent order; centres as of rollout step 0 of the current
        obstacle clock, r the radius (mppi_get_agent_circles)."""
        m = C.c_int32()
        rc = self.lib.mppi_get_agent_circles(self._h, int(agent), None, None, 0, C.byref(m))
        if rc != capi.ERR_SHAPE:  # (cap = 0 holds no circle: MPPI_ERR_SHAPE with m written, or m = 0)
            self._ck(rc)
        c, v = np.empty((m.value, 3)), np.empty((m.value, 2))
        if m.value:
            self._ck(self.lib.mppi_get_agent_circles(self._h, int(agent), _dp(c), _dp(v), m.value, C.byref(m)))
        return c, v

    def set_obstacle_tracks(self, xy, radii, agent=None):
        """Obstacles given as predicted positions: ``xy`` [n, L, 2], point i of a track its centre i control steps after this
        call (it holds the last one afterwards), ``radii`` [n]; for a handle created with ``obstacle_motion=1`` (learned: ``2``).  ``agent``: as
        in `set_ref_path`.  n = 0 removes the set (mppi_set_obstacle_tracks / mppi_set_agent_obstacle_tracks)."""
        r = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
        p = np.ascontiguousarray(xy, dtype=np.float64)
        p = p.reshape(r.shape[0], -1, 2) if r.shape[0] else p.reshape(0, 1, 2)
        if agent is None:
            self._ck(self.lib.mppi_set_obstacle_tracks(self._h, _dp(p), _dp(r), p.shape[0], p.shape[1]))
        else:
            self._ck(self.lib.mppi_set_agent_obstacle_tracks(self._h, int(agent), _dp(p), _dp(r), p.shape[0], p.shape[1]))

    def obstacle_tracks_at(self, step, agent=0):
        """[n, 3] = x, y, r: the centres and radii ``agent`` tests at rollout step ``step`` >= 0 of the current clock
        (mppi_get_obstacle_tracks_at)."""
        n = C.c_int32()
        rc = self.lib.mppi_get_obstacle_tracks_at(self._h, int(agent), int(step), None, 0, C.byref(n))
        if rc != capi.ERR_SHAPE:  # (cap = 0 holds no track: MPPI_ERR_SHAPE with n written, or n = 0)
            self._ck(rc)
        out = np.empty((n.value, 3))
        if n.value:
            self._ck(self.lib.mppi_get_obstacle_tracks_at(self._h, int(agent), int(step), _dp(out), n.value, C.byref(n)))
        return out

    def set_cost_grid(self, cells, origin=(0.0, 0.0), resolution=1.0, weight=1.0, lethal=float("inf"), agent=None):
        """A costmap priced along every rollout: ``cells`` [ny, nx], ``cells[iy, ix]`` the value at ``origin + (ix, iy) *
        resolution``, looked up bilinearly at every state's (x, y); the state's cost gains ``weight * g`` and it counts as
        collided when ``g >= lethal``.  For a handle created with ``obstacle_motion=1`` (the learned model: ``2``).  ``agent``: as in `set_ref_path`.
        ``cells=None`` removes the grid (mppi_set_cost_grid / mppi_set_agent_cost_grid)."""
        if cells is None:
            c, ny, nx = None, 0, 0
        else:
            c = np.ascontiguousarray(cells, dtype=np.float64)
            if c.ndim != 2:
                raise ValueError("cells must be a 2-D array [ny, nx]")
            ny, nx = c.shape
        ox, oy = (float(v) for v in origin)
        tail = (_dp(c) if c is not None else None, nx, ny, ox, oy, float(resolution), float(weight), float(lethal))
        if agent is None:
            self._ck(self.lib.mppi_set_cost_grid(self._h, *tail))
        else:
            self._ck(self.lib.mppi_set_agent_cost_grid(self._h, int(agent), *tail))

    def cost_grid_at(self, xy, agent=0):
        """The raw value of ``agent``'s cost grid at the points ``xy`` [n, 2], computed by the device function the rollout
        prices with (mppi_eval_cost_grid)."""
        p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty(p.shape[0])
        self._ck(self.lib.mppi_eval_cost_grid(self._h, int(agent), _dp(p), p.shape[0], _dp(out)))
        return out

    def set_cost_grid_footprint(self, mode):
        """``"outline"``: wherever a cost grid is priced, the largest value under the vehicle's centre and its eight outline
        points (the ones the collision test uses, turned by the state's yaw) takes the place of the value at the centre -- for
        handles created with ``obstacle_model=OBSTACLE_OUTLINE``.  ``"centre"`` (the default): the state's (x, y) only.  One
        mode for every agent, kept across grid uploads; mppi_set_cost_grid_footprint."""
        modes = {"centre": capi.GRID_FOOTPRINT_CENTRE, "outline": capi.GRID_FOOTPRINT_OUTLINE}
        if mode not in modes:
            raise capi.MppiError(capi.ERR_BAD_ARG, f"cost grid footprint {mode!r} is neither 'centre' nor 'outline'")
        self._ck(self.lib.mppi_set_cost_grid_footprint(self._h, modes[mode]))

    @property
    def cost_grid_footprint(self):
        """``"centre"`` or ``"outline"`` (mppi_get_cost_grid_footprint)."""
        m = C.c_int32(0)
        self._ck(self.lib.mppi_get_cost_grid_footprint(self._h, C.byref(m)))
        return "outline" if m.value == capi.GRID_FOOTPRINT_OUTLINE else "centre"

    def cost_grid_footprint_at(self, poses, agent=0, points=False):
        """The footprint value of ``agent``'s cost grid at the poses ``poses`` [n, 3] = x, y, yaw -- the largest value under
        the centre and the eight outline points -- computed by the device function the rollout prices with, in either mode;
        with ``points=True`` also the nine world points [n, 9, 2] (mppi_eval_cost_grid_footprint)."""
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        out = np.empty(p.shape[0])
        pts = np.empty((p.shape[0], 9, 2)) if points else None
        self._ck(self.lib.mppi_eval_cost_grid_footprint(self._h, int(agent), _dp(p), p.shape[0], _dp(out),
                                                        _dp(pts) if points else None))
        return (out, pts) if points else out

    def fleet_clearance(self, reset=False):
        """(min_dist[n_agents], contact_iters[n_agents]) over the iterations run since the handle was made or the last call
        with ``reset=True``: the smallest centre distance of every agent to any mate at the start of an iteration (inf: none
        ran), and how many iterations started closer than ``2 * fleet_radius`` (mppi_get_fleet_clearance)."""
        d, n = np.empty(self.n_agents), np.zeros(self.n_agents, dtype=np.int64)
        self._ck(self.lib.mppi_get_fleet_clearance(self._h, _dp(d), n.ctypes.data_as(C.POINTER(C.c_int64)), int(bool(reset))))
        return d, n

    def set_fleet_prediction(self, mode):
        """How a fleet handle predicts an agent's mates along the horizon: ``"velocity"`` (the default: constant velocity from
        the mate rows) or ``"plan"`` (along each mate's own nominal rollout, made afresh at the start of every iteration; on a
        learned-dynamics fleet, ``model=MODEL_DIFFDRIVE_MLP, obstacle_motion=3``, through the mate's own network);
        mppi_set_fleet_prediction."""
        modes = {"velocity": capi.FLEET_VELOCITY, "plan": capi.FLEET_PLAN}
        if mode not in modes:
            raise capi.MppiError(capi.ERR_BAD_ARG, f"fleet prediction {mode!r} is neither 'velocity' nor 'plan'")
        self._ck(self.lib.mppi_set_fleet_prediction(self._h, modes[mode]))

    def set_scene_mode(self, mode):
        """``"composed"``: the mates' plans, obstacle tracks and a cost grid may stand together on this handle (the setters'
        cross-refusals are lifted; a handle that holds two or more runs the composed rollout form, one that holds fewer the
        launch it always ran).  ``"exclusive"`` (the default): they exclude each other, as the setters document.  Needs
        ``obstacle_motion=1`` and ``T <= 128``; mppi_set_scene_mode."""
        modes = {"exclusive": capi.SCENE_EXCLUSIVE, "composed": capi.SCENE_COMPOSED}
        if mode not in modes:
            raise capi.MppiError(capi.ERR_BAD_ARG, f"scene mode {mode!r} is neither 'exclusive' nor 'composed'")
        self._ck(self.lib.mppi_set_scene_mode(self._h, modes[mode]))

    @property
    def scene_mode(self):
        """``"exclusive"`` or ``"composed"`` (mppi_get_scene_mode)."""
        m = C.c_int32(0)
        self._ck(self.lib.mppi_get_scene_mode(self._h, C.byref(m)))
        return "composed" if m.value == capi.SCENE_COMPOSED else "exclusive"

    def fleet_plans(self):
        """[n_agents, T + 1, 2]: every agent's plan as of the current states and nominal controls -- point 0 its position, point
        j the position after j steps of its nominal sequence (plan mode only; mppi_get_fleet_plans)."""
        xy = np.empty((self.n_agents, self.T + 1, 2))
        self._ck(self.lib.mppi_get_fleet_plans(self._h, _dp(xy)))
        return xy

    def agent_status(self):
        """(idx[n_agents], path_end[n_agents]): every agent's waypoint index and whether its last x0 call found the end of
        its own path -- which agent stopped a `run_closed_loop` that raised MPPI_ERR_PATH_END."""
        idx, end = np.zeros(self.n_agents, dtype=np.int32), np.zeros(self.n_agents, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._ck(self.lib.mppi_get_agent_status(self._h, idx.ctypes.data_as(ip), end.ctypes.data_as(ip)))
        return idx, end.astype(bool)

    # the residual-model shapes the kernels serve: hidden width H x hidden layers n (512 x 3 and 512 x 2 on
    # k_rollout_mlp_h3, every other one on k_rollout_mlp_w<H, ...>)
    SUPPORTED_MLP = {"hidden": (64, 128, 256, 512), "n_hidden": (1, 2, 3, 4)}

    def set_mlp(self, weights, scalers=None, agent=None):
        """Residual-model weights in the checkpoint's key layout (``state_dict`` of the reference's
        ``MultiLayerPerceptron``, train/train_diff_mlp.py:13-36); tensors or arrays.  Linear(5, H) -> n x [Linear(H, H),
        tanh] -> Linear(H, 3) with H in {64, 128, 256, 512} and n in {1, 2, 3, 4} (`SUPPORTED_MLP`); any other shape is a
        ``ValueError`` that names the set.

        ``scalers``: optional dict with the ``StandardScaler`` statistics the model was trained with
        (train/train_diff_mlp.py:72-86): ``in_mean``/``in_scale`` (5: state then control) and ``out_mean``/``out_scale``
        (3).  The affine maps are folded into the first and last Linear on the host (`mppi_set_mlp_scaled`), so the kernel
        is unchanged: MLP((z - m_in) / s_in) * s_out + m_out.

        A handle of ``n_agents`` > 1 (frozen or per-rollout index, K <= 32768) runs all agents in one launch per stage
        (k_rollout_mlp_h3_agents / k_rollout_mlp_w_agents).  ``agent``: None gives every agent this one model (the shared
        model; a later such call returns the batch to it and releases the agents' own copies), an index in [0, n_agents)
        gives that agent its own model (`mppi_set_agent_mlp[_scaled]`), as in `set_ref_path`; on a single-agent handle
        ``agent=0`` is the plain setter.  A launch is one kernel instantiation, so all agents of a handle hold one shape
        (H, n): a per-agent model whose shape differs from the one any other agent holds is refused (``MppiError``,
        MPPI_ERR_SHAPE; the message names both shapes) -- ``set_mlp(weights)`` changes the shape of the whole batch.  Every
        agent needs a model before a run (MPPI_ERR_STATE names the first one without).  Also refused: an ``agent`` outside
        the handle (MPPI_ERR_BAD_ARG), a handle of another dynamics model (MPPI_ERR_STATE), and on a batched handle a
        model only the f32-input kernel can serve -- weights beyond the f16 range, or MPPI_MLP_F32=1 -- (MPPI_ERR_UNSUPPORTED).
        A refused call leaves the agent on the model it had."""
        def arr(k):
            v = weights[k]
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            return np.ascontiguousarray(v, dtype=np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        n_hidden = sum(1 for k in weights if k.startswith("hidden_layer.") and k.endswith(".weight"))
        w_in, b_in = arr("input_layer.weight"), arr("input_layer.bias")
        wh = [arr(f"hidden_layer.{i}.weight") for i in range(n_hidden)]
        bh = [arr(f"hidden_layer.{i}.bias") for i in range(n_hidden)]
        w_out, b_out = arr("out_layer.weight"), arr("out_layer.bias")
        hidden = w_in.shape[0]
        if w_in.shape != (hidden, 5) or w_out.shape != (3, hidden) or any(w.shape != (hidden, hidden) for w in wh):
            raise ValueError("unexpected MLP shapes (expected Linear(5,H) -> n x Linear(H,H) -> Linear(H,3))")
        if hidden not in self.SUPPORTED_MLP["hidden"] or n_hidden not in self.SUPPORTED_MLP["n_hidden"]:
            raise ValueError(f"MLP of hidden width {hidden} with {n_hidden} hidden layers: the supported set is hidden H in "
                             "{64, 128, 256, 512} x n_hidden in {1, 2, 3, 4}")
        PP = C.POINTER(C.c_float) * max(1, n_hidden)
        model = (hidden, n_hidden, fp(w_in), fp(b_in), PP(*[fp(w) for w in wh]), PP(*[fp(b) for b in bh]), fp(w_out), fp(b_out))
        if scalers is None:
            if agent is None:
                self._ck(self.lib.mppi_set_mlp(self._h, *model))
            else:
                self._ck(self.lib.mppi_set_agent_mlp(self._h, int(agent), *model))
            return
        st = {k: np.ascontiguousarray(scalers[k], dtype=np.float64) for k in ("in_mean", "in_scale", "out_mean", "out_scale")}
        if st["in_mean"].shape != (5,) or st["in_scale"].shape != (5,) or st["out_mean"].shape != (3,) or st["out_scale"].shape != (3,):
            raise ValueError("scalers: in_mean / in_scale have 5 entries (state, control), out_mean / out_scale 3")
        stats = (_dp(st["in_mean"]), _dp(st["in_scale"]), _dp(st["out_mean"]), _dp(st["out_scale"]))
        if agent is None:
            self._ck(self.lib.mppi_set_mlp_scaled(self._h, *model, *stats))
        else:
            self._ck(self.lib.mppi_set_agent_mlp_scaled(self._h, int(agent), *model, *stats))

    def set_u_prev(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != self._lead + (self.T, 2):
            raise ValueError(f"u_prev must be {list(self._lead + (self.T, 2))}")
        self._ck(self.lib.mppi_set_u_prev(self._h, _dp(u)))

    def get_u_prev(self):
        u = np.empty(self._lead + (self.T, 2))
        self._ck(self.lib.mppi_get_u_prev(self._h, _dp(u)))
        return u

    def set_waypoint_idx(self, idx):
        self._ck(self.lib.mppi_set_waypoint_idx(self._h, int(idx)))

    def get_waypoint_idx(self):
        v = C.c_int32()
        self._ck(self.lib.mppi_get_waypoint_idx(self._h, C.byref(v)))
        return v.value

    def set_iteration(self, it):
        self._ck(self.lib.mppi_set_iteration(self._h, int(it)))

    def set_state(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != self._lead + (self.nx,):
            raise ValueError(f"state must be {list(self._lead + (self.nx,))}")
        self._ck(self.lib.mppi_set_state(self._h, _dp(x)))

    def get_state(self):
        x = np.empty(self._lead + (self.nx,))
        self._ck(self.lib.mppi_get_state(self._h, _dp(x)))
        return x

    # -- the iteration ----------------------------------------------------------------------------
    def step(self, x0, eps=None, stream=None):
        """One MPPI iteration.  ``eps``: CUDA float32 tensor [K,T,2] or None (on-device Philox).  ``x0``: host array, or a
        float64 CUDA tensor [nx] handed over zero-copy (mppi_step_device_x0).  Returns (u[T,2] shifted, u0[2], stats)."""
        if hasattr(x0, "is_cuda") and x0.is_cuda:
            import torch
            if x0.dtype != torch.float64 or tuple(x0.shape) != (self.nx,) or not x0.is_contiguous():
                raise ValueError(f"a device x0 must be a contiguous float64 tensor with {self.nx} entries")
            if eps is not None:
                self._check_eps(eps)
            _, up, u0p, stp = self._step_args
            rc = self.lib.mppi_step_device_x0(self._h, C.c_void_p(x0.data_ptr()), _dev_ptr(eps), up, u0p, stp,
                                              _stream_ptr(stream))
            if rc:
                self._ck(rc)
            return self._u_buf.copy(), self._u0_buf.copy(), self.stats
        if np.shape(x0) != (self.nx,):
            raise ValueError(f"observed_x must have {self.nx} entries")
        self._x0_buf[:] = x0
        if eps is not None:
            self._check_eps(eps)
        xp, up, u0p, stp = self._step_args
        rc = self.lib.mppi_step(self._h, xp, _dev_ptr(eps), up, u0p, stp, _stream_ptr(stream))
        if rc:
            self._ck(rc)
        return self._u_buf.copy(), self._u0_buf.copy(), self.stats

    def _check_eps(self, eps):
        if eps is not None:
            import torch
            if eps.dtype != torch.float32 or tuple(eps.shape) != (self.K, self.T, 2):
                raise ValueError(f"eps must be float32 [{self.K}, {self.T}, 2]")

    def partial_len(self):
        n = C.c_int32()
        self._ck(self.lib.mppi_partial_len(self._h, C.byref(n)))
        return n.value

    def step_begin(self, x0, eps, partial, stream=None):
        """x0 None: continue from the state on the device (closed loop)."""
        xp = None
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            xp = _dp(x0)
        self._check_eps(eps)
        self._ck(self.lib.mppi_step_begin(self._h, xp, _dev_ptr(eps), _dev_ptr(partial), _stream_ptr(stream)))

    def step_end_async(self, partials, nranks, stream=None):
        self._ck(self.lib.mppi_step_end_async(self._h, _dev_ptr(partials), int(nranks), _stream_ptr(stream)))

    def sync_result(self, stream=None):
        u, u0 = np.empty((self.T, 2)), np.empty(2)
        self._ck(self.lib.mppi_sync_result(self._h, _dp(u), _dp(u0), C.byref(self.stats), _stream_ptr(stream)))
        return u, u0, self.stats

    # -- peer-to-peer exchange of the per-rank record (include/mppi_hip.h, mppi_comm_*) -------------------
    def comm_export(self, nranks):
        """Creates this rank's exchange buffer; returns its IPC handle (bytes) for the other ranks."""
        buf = C.create_string_buffer(self.lib.mppi_comm_handle_bytes())
        self._ck(self.lib.mppi_comm_export(self._h, int(nranks), buf))
        return buf.raw

    def comm_buffer(self):
        p = C.c_void_p()
        self._ck(self.lib.mppi_comm_buffer(self._h, C.byref(p)))
        return p.value

    def comm_connect(self, rank, handles, local_ptrs=None):
        """``handles``: one IPC handle (bytes) per rank, in rank order (own entry ignored); ``local_ptrs``:
        optional device addresses of peers living in this process (entries that are None use the handle)."""
        n = len(handles)
        blob = C.create_string_buffer(b"".join(bytes(hd) for hd in handles))
        lp = None
        if local_ptrs is not None:
            lp = (C.c_void_p * n)(*[C.c_void_p(p) if p else C.c_void_p(None) for p in local_ptrs])
        self._ck(self.lib.mppi_comm_connect(self._h, int(rank), n, blob, lp))

    def comm_probe(self, stream=None):
        self._ck(self.lib.mppi_comm_probe(self._h, _stream_ptr(stream)))

    def comm_close(self):
        self._ck(self.lib.mppi_comm_close(self._h))

    # -- the same exchange carried by RCCL inside the library (include/mppi_hip.h, mppi_comm_init) ----------
    def comm_unique_id(self):
        """ncclGetUniqueId through the library (loads librccl.so.1 on first use); bytes for the other ranks."""
        buf = C.create_string_buffer(self.lib.mppi_comm_unique_id_bytes())
        rc = self.lib.mppi_comm_unique_id(buf)
        if rc != capi.OK:
            raise capi.MppiError(rc, (self.lib.mppi_last_error(None) or b"").decode() or "mppi_comm_unique_id failed")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        """ncclCommInitRank on the handle's device: collective, every rank calls it with rank 0's id.  From then on
        ``step`` and ``run_closed_loop`` carry ONE ncclAllGather per iteration inside the library."""
        buf = C.create_string_buffer(bytes(unique_id), len(unique_id))
        self._ck(self.lib.mppi_comm_init(self._h, buf, int(rank), int(nranks)))

    def step_end(self, partials, nranks, stream=None):
        u, u0 = np.empty((self.T, 2)), np.empty(2)
        self._ck(self.lib.mppi_step_end(self._h, _dev_ptr(partials), int(nranks), _dp(u), _dp(u0),
                                        C.byref(self.stats), _stream_ptr(stream)))
        return u, u0, self.stats

    def costs(self):
        S = np.empty(self._lead + (self.K,))
        self._ck(self.lib.mppi_get_costs(self._h, _dp(S)))
        return S

    def weights(self):
        w = np.empty(self.K)
        self._ck(self.lib.mppi_get_weights(self._h, _dp(w)))
        return w

    def sample_epsilon(self, iteration, out=None, stream=None):
        """The sampler's noise of `iteration` as a tensor: float32 [K,T,2] ([n_agents,K,T,2] for a batched handle)."""
        import torch
        shape = self._lead + (self.K, self.T, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.cfg.device}")
        elif out.dtype != torch.float32 or tuple(out.shape) != shape:
            raise ValueError(f"out must be float32 {list(shape)}")
        self._ck(self.lib.mppi_sample_epsilon(self._h, int(iteration), _dev_ptr(out), _stream_ptr(stream)))
        return out

    def set_noise_ring(self, ring):
        """`_calc_epsilon` materialised for the closed loop: ``ring`` = CUDA float32 [n_slots, (n_agents,) K, T, 2], n_slots a
        power of two; iteration i reads slot i mod n_slots.  ``None`` returns to the in-kernel sampler.  The engine keeps a
        reference to the tensor."""
        if ring is None:
            self._ck(self.lib.mppi_set_noise_ring(self._h, None, 0))
            self._noise_ring = None
            return
        import torch
        want = self._lead + (self.K, self.T, 2)
        if ring.dtype != torch.float32 or tuple(ring.shape[1:]) != want:
            raise ValueError(f"the noise ring must be float32 [n_slots, {', '.join(map(str, want))}]")
        self._ck(self.lib.mppi_set_noise_ring(self._h, _dev_ptr(ring), int(ring.shape[0])))
        self._noise_ring = ring

    def rollout_viz(self, want_optimal=True, want_sampled=True, stream=None):
        import torch
        dev = f"cuda:{self.cfg.device}"
        opt = torch.empty((self.T, self.nx), dtype=torch.float32, device=dev) if want_optimal else None
        smp = torch.empty((self.K, self.T, self.nx), dtype=torch.float32, device=dev) if want_sampled else None
        self._ck(self.lib.mppi_rollout_viz(self._h, _dev_ptr(opt), _dev_ptr(smp), _stream_ptr(stream)))
        return opt, smp

    # -- batched stage methods (include/mppi_hip.h, mppi_eval_*) -------------------------------------------
    @staticmethod
    def _rows(a, ncol):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != ncol:
            raise ValueError(f"expected an [n, {ncol}] array")
        return a

    def eval_state_transition(self, x, v):
        x, v = self._rows(x, self.nx), self._rows(v, 2)
        if v.shape[0] != x.shape[0]:
            raise ValueError("x and v must have the same number of rows")
        out = np.empty_like(x)
        self._ck(self.lib.mppi_eval_state_transition(self._h, _dp(x), _dp(v), x.shape[0], _dp(out)))
        return out

    def eval_clamp(self, v):
        v = self._rows(v, 2)
        out = np.empty_like(v)
        self._ck(self.lib.mppi_eval_clamp(self._h, _dp(v), v.shape[0], _dp(out)))
        return out

    def eval_is_collided(self, x, steps=None):
        """``steps``: int [n], pose i is tested against the circles ``steps[i]`` rollout steps ahead of the current obstacle
        clock (moving obstacles); None: now."""
        x = self._rows(x, self.nx)
        out = np.empty(x.shape[0])
        if steps is None:
            self._ck(self.lib.mppi_eval_is_collided(self._h, _dp(x), x.shape[0], _dp(out)))
            return out
        st = np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
        if st.shape[0] != x.shape[0]:
            raise ValueError("one step per pose")
        self._ck(self.lib.mppi_eval_is_collided_at(self._h, _dp(x), x.shape[0], st.ctypes.data_as(C.POINTER(C.c_int32)), _dp(out)))
        return out

    def eval_nearest_waypoint(self, x, prev_idx, update_prev_idx=False):
        """Returns (idx[n], prev_idx after the calls)."""
        x = self._rows(x, self.nx)
        p, idx = C.c_int32(int(prev_idx)), np.empty(x.shape[0], dtype=np.int32)
        self._ck(self.lib.mppi_eval_nearest_waypoint(self._h, _dp(x), x.shape[0], C.byref(p), int(bool(update_prev_idx)),
                                                     idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, p.value

    def eval_cost(self, x, prev_idx, terminal=False, update_prev_idx=False):
        """Returns (cost[n], idx[n], prev_idx after the calls)."""
        x = self._rows(x, self.nx)
        p, idx, cost = C.c_int32(int(prev_idx)), np.empty(x.shape[0], dtype=np.int32), np.empty(x.shape[0])
        self._ck(self.lib.mppi_eval_cost(self._h, int(bool(terminal)), _dp(x), x.shape[0], C.byref(p),
                                         int(bool(update_prev_idx)), _dp(cost), idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return cost, idx, p.value

    def eval_moving_average(self, xx):
        xx = np.ascontiguousarray(xx, dtype=np.float64)
        if xx.shape != (self.T, 2):
            raise ValueError(f"the filter input must be [{self.T}, 2]")
        out = np.empty_like(xx)
        self._ck(self.lib.mppi_eval_moving_average(self._h, _dp(xx), _dp(out)))
        return out

    def eval_weights(self, S):
        S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1)
        w = np.empty_like(S)
        self._ck(self.lib.mppi_eval_weights(self._h, _dp(S), S.size, _dp(w)))
        return w

    def run_closed_loop(self, n_iters, trace=False, stream=None):
        tr = np.empty((n_iters, 2)) if trace else None
        self._ck(self.lib.mppi_run_closed_loop(self._h, int(n_iters), _dp(tr) if trace else None,
                                               C.byref(self.stats), _stream_ptr(stream)))
        return tr, self.stats

    def enable_timing(self, on=True):
        self._ck(self.lib.mppi_enable_timing(self._h, int(bool(on))))

    def set_rollout_repeats(self, n):
        self._ck(self.lib.mppi_set_rollout_repeats(self._h, int(n)))

    def counters(self):
        out = (C.c_int64 * 3)()
        self._ck(self.lib.mppi_get_counters(self._h, out))
        layout = C.c_int32(-1)
        if hasattr(self.lib, "mppi_get_rollout_layout"):  # (absent from an older diagnostic build under MPPI_LIB)
            self._ck(self.lib.mppi_get_rollout_layout(self._h, C.byref(layout)))
        return {"iterations": out[0], "rollout_launches": out[1], "finalize_launches": out[2], "rollout_layout": layout.value}

    def rollout_kernel(self):
        """Name of the kernel instantiation the last rollout-class launch took, as rocprofv3 prints it."""
        if not hasattr(self.lib, "mppi_get_rollout_kernel"):  # (an older diagnostic build under MPPI_LIB)
            return ""
        buf = C.create_string_buffer(192)
        self._ck(self.lib.mppi_get_rollout_kernel(self._h, buf, 192))
        return buf.value.decode()

    def host_timing(self):
        """Seconds this handle's closed-loop calls spent enqueueing launches / inside the calls (cumulative)."""
        out = (C.c_double * 2)()
        self._ck(self.lib.mppi_get_host_timing(self._h, out))
        return {"enqueue_s": out[0], "loop_s": out[1]}

    def time_rollout_launch(self, n_slots=500, extra=2, stream=None):
        """GPU-side launch-to-launch duration of the rollout kernel (microseconds) and the in-graph iteration period, from
        graph replays (`mppi_time_rollout_launch`): independent of how fast the host enqueues."""
        out = (C.c_double * 2)()
        self._ck(self.lib.mppi_time_rollout_launch(self._h, int(n_slots), int(extra), _stream_ptr(stream), out))
        return {"rollout_us": out[0], "graph_iteration_us": out[1]}

    def last_kernel_ms(self):
        out = (C.c_float * 4)()
        self._ck(self.lib.mppi_last_kernel_ms(self._h, out))
        return {"rollout": out[0], "reduce": out[1], "finalize": out[2], "event_pair_overhead": out[3]}
