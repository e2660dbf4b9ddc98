"""`pytorch_mppi.MPPI` call surface with BUILT-IN dynamics / running-cost models.

The reference's test/test_mppi.py, test/test_mppi_diff.py, test/test_mppi_diff_dyna.py and
train/bullet_mppi_differential_drive.py drive ``pytorch_mppi.MPPI(dynamics, running_cost, nx, noise_sigma, num_samples=...,
horizon=..., lambda_=..., u_min=..., u_max=...)`` with Python callbacks.  Here ``dynamics`` and ``running_cost`` NAME a
model evaluated on the GPU (libmppi_hip.so, ``mppi_cb_*``):

    from dnn_mppi_mpc_amd.callback_mppi import MPPI, RunningCost
    ctrl = MPPI("unicycle", RunningCost.static_obstacles(), 3, noise_sigma, num_samples=1000, horizon=25, lambda_=1.0,
                u_min=[-2, -2], u_max=[2, 2])
    action = ctrl.command(state)

``command`` / ``U`` / ``cost_total`` / ``perturbed_action`` / ``get_trajectories`` mirror the library's and its callers'.
Models: "unicycle", "skid_steer", "racecar" (test/test_mppi_racecar.py), "racecar_dynamic"
(test/test_torch_mppi_race_car.py) and "double_integrator" (test/test_torch_mppi.py, with ``TerminalCost``).  Options built:
``terminal_state_cost``, ``noise_mu``, ``u_scale``, ``u_per_command``, ``noise_abs_cost``, ``sample_null_action``; refused:
``rollout_samples != 1`` and ``rollout_var_cost != 0`` (the built-in models are deterministic).  The loop follows the
published algorithm; the library is absent here and un-pinned by the reference, so that part is parity-unpinned
(include/mppi_hip.h).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi

DYNAMICS = {"unicycle": (0, 3, 2), "skid_steer": (1, 5, 4), "racecar": (2, 4, 2), "racecar_dynamic": (3, 4, 2),
            "double_integrator": (4, 2, 1)}
DEFAULT_DT = {"unicycle": 0.05, "skid_steer": 0.02, "racecar": 0.05, "racecar_dynamic": 0.05, "double_integrator": 0.1}
# the callers' constants, in the order of mppi_cb_config.model_params
MODEL_PARAMS = {"racecar": (0.3,),                                       # L: test/test_mppi_racecar.py:23
                "racecar_dynamic": (1.5, 1.0, 1000.0, 1000.0, 1000.0)}  # l_r, l_f, m, C_f, C_r: test_torch_mppi_race_car.py:17-22


class MppiCbConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("dynamics", C.c_int32), ("obstacle_kind", C.c_int32),
                ("K", C.c_int32), ("T", C.c_int32), ("n_obs", C.c_int32), ("sample_null_action", C.c_int32),
                ("dt", C.c_double), ("lambda_", C.c_double), ("noise_sigma", C.c_double * 16),
                ("u_min", C.c_double * 4), ("u_max", C.c_double * 4), ("u_init", C.c_double * 4),
                ("goal", C.c_double * 5), ("q_diag", C.c_double * 5), ("r_diag", C.c_double * 4),
                ("obstacles", C.c_double * 64), ("safety_distance", C.c_double), ("obstacle_weight", C.c_double),
                ("skid_params", C.c_double * 5), ("seed", C.c_uint64),
                ("model_params", C.c_double * 8), ("terminal_cost", C.c_int32), ("noise_abs_cost", C.c_int32),
                ("terminal_goal", C.c_double * 5), ("terminal_q", C.c_double * 5), ("noise_mu", C.c_double * 4),
                ("u_scale", C.c_double)]


class RunningCost:
    """(s - goal)^T diag(Q) (s - goal) + u^T diag(R) u + weight * sum over obstacles of the obstacle term."""

    def __init__(self, goal, q_diag, r_diag, obstacles, safety_distance, obstacle_weight, kind):
        self.goal, self.q_diag, self.r_diag = map(lambda a: np.asarray(a, float), (goal, q_diag, r_diag))
        self.obstacles = np.asarray(obstacles, float).reshape(-1, 4)  # x, y, vx, vy (per horizon step)
        self.safety_distance, self.obstacle_weight, self.kind = float(safety_distance), float(obstacle_weight), kind

    @classmethod
    def static_obstacles(cls):
        """test/test_mppi.py:30-50."""
        return cls([6.0, 6.0, 1.57], [20, 5, 9], [0.1, 0.1], [[5.0, 4.0, 0, 0], [3.5, 3.5, 0, 0]], 0.8, 10.0, "inverse")

    @classmethod
    def moving_obstacles(cls):
        """test/test_mppi_diff.py:25-52."""
        return cls([5.0, 4.0, 1.57], [10.0, 5.0, 9.0], [1.0, 10.0], [[5.0, 5.0, 0.0, -0.05], [7.0, 3.0, 0.0, 0.05]], 1.0, 1.0,
                   "exponential")

    @classmethod
    def skid_steer(cls):
        """test/test_mppi_diff_dyna.py:44-64."""
        return cls([6.0, 6.0, 1.57, 2.0, 0.0], [200, 200, 20, 10, 20], [0.001] * 4, [[5.0, 4.0, 0, 0], [3.5, 3.5, 0, 0]], 0.8,
                   10.0, "inverse")

    @classmethod
    def racecar(cls):
        """test/test_mppi_racecar.py:33-53."""
        return cls([6.0, 5.0, 0.0, 0.0], [50.0, 35.0, 90.0, 0.1], [0.1, 0.1], [[6.0, 5.0, 0, 0], [7.0, 3.0, 0, 0]], 0.8, 10.0,
                   "inverse")

    @classmethod
    def racecar_dynamic(cls):
        """test/test_torch_mppi_race_car.py:42-61: the obstacle term is exp(-d), the exponential cost with safety 0 and weight 1."""
        return cls([5.0, 5.0, 1.57, 1.0], [10.0, 5.0, 9.0, 1.0], [1.0, 10.0], [[5.0, 5.0, 0, 0], [7.0, 3.0, 0, 0]], 0.0, 1.0,
                   "exponential")

    @classmethod
    def double_integrator(cls):
        """test/test_torch_mppi.py:18-20."""
        return cls([0.0, 0.0], [1.0, 1.0], [1.0], [], 0.0, 0.0, "inverse")


class TerminalCost:
    """(s_T - goal)^T diag(q) (s_T - goal) on the state after the last step, added once to each sample's running costs."""

    def __init__(self, goal, q_diag):
        self.goal, self.q_diag = np.asarray(goal, float).reshape(-1), np.asarray(q_diag, float).reshape(-1)

    @classmethod
    def double_integrator(cls):
        """test/test_torch_mppi.py:23-25: sum of squares."""
        return cls([0.0, 0.0], [1.0, 1.0])


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


class MPPI:
    def __init__(self, dynamics, running_cost, nx, noise_sigma, num_samples=100, horizon=15, device=0,
                 terminal_state_cost=None, lambda_=1.0, noise_mu=None, u_min=None, u_max=None, u_init=None, U_init=None,
                 u_scale=1, u_per_command=1, step_dependent_dynamics=False, rollout_samples=1, rollout_var_cost=0,
                 rollout_var_discount=0.95, sample_null_action=False, noise_abs_cost=False, dt=None, seed=0, model_params=None):
        if dynamics not in DYNAMICS:
            raise ValueError(f"dynamics must name a built-in model: {sorted(DYNAMICS)}")
        if not isinstance(running_cost, RunningCost):
            raise ValueError("running_cost must be a RunningCost (built-in quadratic + obstacle model)")
        if rollout_samples != 1 or rollout_var_cost != 0:
            raise NotImplementedError("rollout_samples != 1 and rollout_var_cost != 0 are not built: the built-in models are "
                                      "deterministic, so M rollouts of one action sequence are M copies of one trajectory")
        if terminal_state_cost is not None and not isinstance(terminal_state_cost, TerminalCost):
            raise ValueError("terminal_state_cost must be a TerminalCost (built-in quadratic) or None")
        dyn, self.nx, self.nu = DYNAMICS[dynamics]
        if int(nx) != self.nx:
            raise ValueError(f"{dynamics} has nx = {self.nx}")
        sigma = _np(noise_sigma).reshape(self.nu, self.nu)
        self.K, self.T = int(num_samples), int(horizon)
        self.u_scale, self.u_per_command = float(u_scale), int(u_per_command)
        if not np.isfinite(self.u_scale) or self.u_scale == 0:
            raise ValueError("u_scale must be finite and not 0")
        if self.u_per_command != u_per_command or not 1 <= self.u_per_command <= self.T:
            raise ValueError(f"u_per_command must be an integer in [1, horizon = {self.T}]")
        self.lib = capi.load_library()
        c = MppiCbConfig()
        c.struct_size = C.sizeof(MppiCbConfig)
        if not hasattr(self.lib, "mppi_cb_top_trajectories"):
            # an older diagnostic build under MPPI_LIB: its struct ends with `seed` (the struct_size handshake), and it has
            # none of what the fields after it configure
            if dyn > 1 or terminal_state_cost is not None or noise_mu is not None or self.u_scale != 1 or noise_abs_cost:
                raise capi.MppiError(capi.ERR_UNSUPPORTED, f"{capi.LIB_PATH} predates this model or option")
            c.struct_size = MppiCbConfig.model_params.offset
        if hasattr(device, "index"):
            device = device.index or 0
        c.device, c.dynamics, c.K, c.T = int(device) if not isinstance(device, str) else 0, dyn, self.K, self.T
        c.obstacle_kind = 0 if running_cost.kind == "inverse" else 1
        c.n_obs, c.sample_null_action = running_cost.obstacles.shape[0], int(bool(sample_null_action))
        c.dt = float(dt) if dt is not None else DEFAULT_DT[dynamics]  # the callers' constants
        c.lambda_ = float(lambda_)
        for i in range(self.nu):
            for j in range(self.nu):
                c.noise_sigma[4 * i + j] = sigma[i, j]
        lo = _np(u_min) if u_min is not None else np.full(self.nu, -1e30)
        hi = _np(u_max) if u_max is not None else np.full(self.nu, 1e30)
        ui = _np(u_init) if u_init is not None else np.zeros(self.nu)
        for i in range(self.nu):
            c.u_min[i], c.u_max[i], c.u_init[i], c.r_diag[i] = lo[i], hi[i], ui[i], running_cost.r_diag[i]
        for i in range(self.nx):
            c.goal[i], c.q_diag[i] = running_cost.goal[i], running_cost.q_diag[i]
        for m, row in enumerate(running_cost.obstacles[:len(c.obstacles) // 4]):  # (more than fit: mppi_cb_create refuses n_obs)
            for q in range(4):
                c.obstacles[4 * m + q] = row[q]
        c.safety_distance, c.obstacle_weight = running_cost.safety_distance, running_cost.obstacle_weight
        for i, v in enumerate((2.0, 0.05, 0.1, 0.4, 0.1)):  # test/test_mppi_diff_dyna.py:15-19, :29-30
            c.skid_params[i] = v
        c.seed = int(seed)
        mp = MODEL_PARAMS.get(dynamics, ()) if model_params is None else tuple(_np(model_params).reshape(-1))
        for i, v in enumerate(mp[:len(c.model_params)]):
            c.model_params[i] = v
        if terminal_state_cost is not None:
            if terminal_state_cost.goal.shape != (self.nx,) or terminal_state_cost.q_diag.shape != (self.nx,):
                raise ValueError(f"the terminal cost of {dynamics} has {self.nx} components")
            c.terminal_cost = 1
            for i in range(self.nx):
                c.terminal_goal[i], c.terminal_q[i] = terminal_state_cost.goal[i], terminal_state_cost.q_diag[i]
        c.noise_abs_cost, c.u_scale = int(bool(noise_abs_cost)), self.u_scale
        if noise_mu is not None:
            for i, v in enumerate(_np(noise_mu).reshape(self.nu)):
                c.noise_mu[i] = v
        self._h = C.c_void_p()
        rc = self.lib.mppi_cb_create(C.byref(c), C.byref(self._h))
        if rc:
            msg = self.lib.mppi_cb_last_error(None)
            self._h = None
            raise capi.MppiError(rc, msg.decode() if msg else "mppi_cb_create failed")
        self.cfg = c
        if U_init is not None:
            self.U = U_init

    def _ck(self, rc):
        if rc:
            msg = self.lib.mppi_cb_last_error(self._h)
            raise capi.MppiError(rc, msg.decode() if msg else "unknown error")

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.mppi_cb_destroy(self._h)
            self._h = None

    @property
    def U(self):
        u = np.empty((self.T, self.nu))
        self._ck(self.lib.mppi_cb_get_nominal(self._h, u.ctypes.data_as(C.POINTER(C.c_double))))
        return u

    @U.setter
    def U(self, value):
        u = np.ascontiguousarray(_np(value).reshape(self.T, self.nu))
        self._ck(self.lib.mppi_cb_set_nominal(self._h, u.ctypes.data_as(C.POINTER(C.c_double))))

    def _eps(self, noise):
        if noise is None:
            return None
        if not noise.is_cuda or not noise.is_contiguous() or tuple(noise.shape) != (self.K, self.T, self.nu) or \
                str(noise.dtype) != "torch.float32":  # (the kernels read the buffer as float whatever it holds)
            raise ValueError(f"noise must be a contiguous CUDA float32 tensor [{self.K}, {self.T}, {self.nu}]")
        return C.c_void_p(noise.data_ptr())

    def command(self, state, shift_nominal_trajectory=True, noise=None):
        """`MPPI.command(state)` -> the first action of the updated nominal sequence ([nu]), or with ``u_per_command = n > 1``
        its first n rows ([n, nu]).  ``noise``: optional CUDA float32 tensor [K, T, nu] in place of the in-kernel Philox
        draw (the whole draw: ``noise_mu`` is not added to it)."""
        s = np.ascontiguousarray(_np(state).reshape(self.nx))
        eps = self._eps(noise)
        a = np.empty(self.nu)
        self._ck(self.lib.mppi_cb_command(self._h, s.ctypes.data_as(C.POINTER(C.c_double)), eps, int(bool(shift_nominal_trajectory)),
                                          a.ctypes.data_as(C.POINTER(C.c_double)), None))
        return a if self.u_per_command == 1 else self.U[:self.u_per_command]

    def _costs(self, which):
        out = np.empty(self.K)
        p = out.ctypes.data_as(C.POINTER(C.c_double))
        self._ck(self.lib.mppi_cb_get_costs(self._h, p if which == 0 else None, p if which == 1 else None))
        return out

    @property
    def cost_total(self):
        return self._costs(0)

    @property
    def omega(self):
        return self._costs(1)

    def _eval(self, what, states, actions, t):
        s = np.ascontiguousarray(_np(states).reshape(-1, self.nx))
        a = np.ascontiguousarray(_np(actions).reshape(-1, self.nu))
        out = np.empty((s.shape[0], self.nx) if what == 0 else s.shape[0])
        D = C.POINTER(C.c_double)
        self._ck(self.lib.mppi_cb_eval(self._h, what, s.ctypes.data_as(D), a.ctypes.data_as(D), int(t), s.shape[0],
                                       out.ctypes.data_as(D)))
        return out

    def _dynamics(self, state, u, t=0):
        return self._eval(0, state, u, t)

    def _running_cost(self, state, u, t=0):
        return self._eval(1, state, u, t)

    def _terminal_cost(self, state):
        return self._eval(2, state, np.zeros((np.asarray(_np(state)).reshape(-1, self.nx).shape[0], self.nu)), 0)

    def get_perturbed_action(self, noise=None):
        """The clamped, unscaled actions [K, T, nu] of the last command; ``noise``: the tensor that command was given, if any."""
        out = np.empty((self.K, self.T, self.nu))
        self._ck(self.lib.mppi_cb_get_perturbed_actions(self._h, self._eps(noise), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    @property
    def perturbed_action(self):
        return self.get_perturbed_action()

    def get_sampled_trajectories(self, state, n=None, noise=None):
        """(trajectories [n, T, nx], indices [n]): the n cheapest samples of the last command, cheapest first, rolled out from
        ``state``.  n defaults to the callers' max(10, K // 10), capped at K (test/test_mppi_racecar.py:77)."""
        n = min(self.K, max(10, self.K // 10)) if n is None else int(n)
        s = np.ascontiguousarray(_np(state).reshape(self.nx))
        tr, idx = np.empty((max(n, 0), self.T, self.nx)), np.empty(max(n, 0), np.int32)
        D = C.POINTER(C.c_double)
        self._ck(self.lib.mppi_cb_top_trajectories(self._h, s.ctypes.data_as(D), self._eps(noise), n, tr.ctypes.data_as(D),
                                                   idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return tr, idx

    def get_trajectories(self, state, noise=None):
        """The callers' wrapper (test/test_mppi_racecar.py:66-86): command(state), then (optimal_traj, sampled_traj_list)."""
        self.command(state, noise=noise)
        return self.get_optimal_trajectory(state), self.get_sampled_trajectories(state, noise=noise)[0]

    def get_optimal_trajectory(self, state):
        """The states the nominal sequence drives through (the `optimal_traj` of the callers' get_trajectories)."""
        s = np.ascontiguousarray(_np(state).reshape(self.nx))
        tr = np.empty((self.T, self.nx))
        D = C.POINTER(C.c_double)
        self._ck(self.lib.mppi_cb_nominal_trajectory(self._h, s.ctypes.data_as(D), tr.ctypes.data_as(D)))
        return tr
