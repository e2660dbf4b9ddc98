"""Moving obstacles (mppi_config.obstacle_motion): the f64 reference and the scenes of test_moving_obstacle_cases.py
(CPU) and test_gpu_moving_obstacles.py.  No device import.

The reference is the project's oracle with `collided` overridden: a circle {x, y, r, vx, vy} stands at c + v * (dt * (n + j))
when the state reached after j rollout steps is tested, n control steps after the set was uploaded.  Which j a call means
follows from how the oracle calls `collided`: RaceCarOracle.state_cost with [K, T] states (column t: step t + 1) and with
[K] terminal states (step T), DiffDriveOracle.iteration with the last state (step T).  The same override records, per tested
pose, the decision margin |min d^2 - r^2| / r^2 of tests/test_gpu_primitives.py, so that a comparison can leave out the samples
an f32 handle may legitimately decide the other way."""
import numpy as np

from oracle import mppi_oracle
from oracle.mppi_oracle import F32

MARGIN = 1e-4          # the project's rule (tests/prims_checks.py COLLISION_MARGIN): decisions inside it may flip in f32
MAX_LEFT_OUT = 0.01    # of a case's samples


def centres(circles, vel, dt, n, j):
    """Centres [..., m, 2] of the circles at rollout step(s) j (int or int array [...]) of clock n: c + v * (dt * (n + j))."""
    tau = dt * (n + np.asarray(j, dtype=np.int64)).astype(np.float64)
    c, v = np.asarray(circles, np.float64), np.asarray(vel, np.float64)
    return c[:, :2] + v * tau[..., None, None]


class _Motion:
    """What both oracles share: velocities, the clock, the step a `collided` call means, the margins it saw."""

    def set_motion(self, vel, clock=0, freeze_at=None):
        """freeze_at: None -- the circles move; an int j -- every test sees them where they stand at step j of the clock (the
        static scenes the CPU tests compare against)."""
        self.obstacle_vel = np.zeros((len(self.obstacle_circles), 2)) if vel is None else np.asarray(vel, np.float64).reshape(-1, 2)
        self.clock = int(clock)
        self.freeze_at = freeze_at
        self.margins = []

    def _steps_of(self, shape, steps):
        if steps is not None:
            j = np.broadcast_to(np.asarray(steps, dtype=np.int64), shape)
        elif len(shape) == 2:  # [K, T] stage states: column t is the state after step t + 1
            j = np.broadcast_to(np.arange(1, shape[1] + 1, dtype=np.int64)[None, :], shape)
        else:                  # [K] terminal / last states
            j = np.full(shape, self.T, dtype=np.int64)
        if self.freeze_at is not None:
            j = np.full(shape, int(self.freeze_at), dtype=np.int64)
        return j

    def _test(self, px, py, r2, steps):
        """points px, py [..., P] (f64) against every circle at the pose's step: hit [...], margin [...]"""
        c = centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps)  # [..., m, 2]
        d2 = (px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2  # [..., P, m]
        hit = (d2 < r2).any(axis=(-1, -2))
        margin = (np.abs(d2 - r2) / r2).min(axis=(-1, -2))
        self.margins.append(margin.reshape(margin.shape[0], -1))
        return hit

    def sample_margin(self):
        """Per sample, the smallest margin over the poses tested since the last `set_motion` / `reset_margins`."""
        return np.concatenate(self.margins, axis=1).min(axis=1)

    def reset_margins(self):
        self.margins = []

    def tick(self):
        self.clock += 1


def filter_window(T):
    """The reference's window of 10 where the horizon has room for it (its filter raises on T < window, and so does
    mppi_create); a horizon of 7 steps takes a window of 5."""
    return 10 if T >= 10 else 5


class MovingDiffDriveOracle(_Motion, mppi_oracle.DiffDriveOracle):
    def __init__(self, *a, obstacle_velocities=None, **kw):
        super().__init__(*a, **kw)
        self.set_motion(obstacle_velocities)

    def collided(self, x, y, steps=None):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        r2 = (0.5 * self.safety_margin_rate + self.obstacle_circles[:, 2]) ** 2  # _obs.py:304-311
        return self._test(x[..., None], y[..., None], r2, self._steps_of(x.shape, steps)).astype(np.float64)

    def iteration_general(self, observed_x, epsilon, mode="sequential", accumulate=False):
        """`iteration` for the handle's other switches: the waypoint index frozen at the x0 call's or threaded per rollout
        (mppi_oracle.per_rollout_waypoint_scan), and the accumulating sum `S[k] += ...` over all T stage costs
        (accumulate_stage_cost = 1 as tests/test_gpu_engine.py configures the diff-drive model: every step is priced, and so
        tested against the circles at ITS step).  mode "sequential" without accumulation is `iteration` itself -- the CPU
        tests hold the two to each other."""
        K, T = self.K, self.T
        x0, eps = np.asarray(observed_x, np.float64), np.asarray(epsilon, np.float64)
        u = self.u_prev.copy()
        p0 = self.nearest_waypoint(x0[0], x0[1], self.prev_way_point_idx)
        out = {"idx_start": p0, "path_end": bool(p0 >= self.ref_path.shape[0] - 1)}
        exploit = (np.arange(K) < mppi_oracle.exploit_threshold(self.param_exploration, K))[:, None, None]
        v = self.clamp(np.where(exploit, u[None] + eps, eps))
        X = self.rollout(x0, v)
        Xc = np.concatenate([X, X[:, -1:]], axis=1)  # the T stage calls and the terminal call, which sees the last state again
        R, W = self.ref_path, self.SEARCH_IDX_LEN
        p_after = p0
        if mode == "frozen":
            win = R[p0:p0 + W, :2]
            idx = p0 + np.argmin((Xc[..., 0:1] - win[:, 0]) ** 2 + (Xc[..., 1:2] - win[:, 1]) ** 2, axis=-1)
        elif mode == "per_rollout":
            idx = mppi_oracle.per_rollout_waypoint_scan(X, R[:, :2], p0, W)
        else:
            idx, p_after = mppi_oracle.sequential_waypoint_scan(Xc[..., 0].reshape(-1), Xc[..., 1].reshape(-1), R[:, :2], p0, W)
            idx = idx.reshape(K, T + 1)
        w, wt = self.stage_cost_weight, self.terminal_cost_weight

        def track(wgt, S_, i):
            return (wgt[0] * (S_[..., 0] - R[i, 0]) ** 2 + wgt[1] * (S_[..., 1] - R[i, 1]) ** 2 + wgt[2] * (S_[..., 2] - R[i, 2]) ** 2)
        q = u @ np.linalg.inv(self.Sigma)  # row t: u_t^T Sigma^-1 (:124)
        ctrl = self.param_gamma * (q[None, :, 0] * v[..., 0] + q[None, :, 1] * v[..., 1])
        if accumulate:
            stage = track(w, X, idx[:, :T]) + self.collided(X[..., 0], X[..., 1]) * 1.0e10 + ctrl  # [K, T]: step t + 1
            term = track(wt, X[:, -1], idx[:, T]) + self.collided(X[:, -1, 0], X[:, -1, 1]) * 1.0e10
            S = stage.sum(axis=1) + term
        else:
            coll = self.collided(X[:, -1, 0], X[:, -1, 1]) * 1.0e10
            S = (track(w, X[:, -1], idx[:, T - 1]) + coll + ctrl[:, T - 1]) + (track(wt, X[:, -1], idx[:, T]) + coll)
        out["S"], out["idx_after"] = S, p_after
        self.prev_way_point_idx = p_after
        wgt = self.compute_weight(S)
        w_eps = mppi_oracle.moving_average_diffdrive(mppi_oracle.sequential_sum(wgt[:, None, None] * eps, axis=0), filter_window(T))
        u = u + w_eps
        if self.visualze_sampled_trajs:
            u = self.clamp(u)
        self.u_prev[:-1] = u[1:]
        self.u_prev[-1] = u[-1]
        out["u_returned"], out["u0_returned"], out["X"] = self.u_prev.copy(), self.u_prev[0].copy(), X
        return out


class MovingRaceCarOracle(_Motion, mppi_oracle.RaceCarOracle):
    def __init__(self, *a, obstacle_velocities=None, **kw):
        super().__init__(*a, **kw)
        self.set_motion(obstacle_velocities)

    def collided(self, x, y, yaw, steps=None):
        """mppi_race_car_obstacle.py:241-274 as the oracle restates it (outline points in f32, circle test in f64), the circles
        at the pose's step"""
        vw, vl = self.vehicle_w * self.collision_safety_margin_rate, self.vehicle_l * self.collision_safety_margin_rate
        sx = [-0.5 * vl, -0.5 * vl, 0.0, +0.5 * vl, +0.5 * vl, +0.5 * vl, 0.0, -0.5 * vl, -0.5 * vl]
        sy = [0.0, +0.5 * vw, +0.5 * vw, +0.5 * vw, 0.0, -0.5 * vw, -0.5 * vw, -0.5 * vw, 0.0]
        c, s = np.cos(yaw), np.sin(yaw)
        qx = np.stack([(F32(a) * c - F32(b) * s + x).astype(np.float64) for a, b in zip(sx, sy)], axis=-1)
        qy = np.stack([(F32(a) * s + F32(b) * c + y).astype(np.float64) for a, b in zip(sx, sy)], axis=-1)
        return self._test(qx, qy, self.obstacle_circles[:, 2] ** 2, self._steps_of(np.shape(x), steps)).astype(F32)


# ------------------------------------------------------------------------------------------ scenes
DIFF_KW = dict(delta_t=0.1, max_speed=5.0, max_omega=3.14, param_exploration=0.05, param_lambda=1.0, param_alpha=0.2,
               sigma=np.array([[0.1, 0.0], [0.0, 0.01]]), stage_cost_weight=np.array([5.0, 5.0, 10.0]),
               terminal_cost_weight=np.array([5.0, 5.0, 10.0]), safety_margin_rate=0.8, visualize_optimal_traj=False,
               visualze_sampled_trajs=False)
TRAVEL, SWEEP = 3.0, 6.0  # metres the nominal rollout covers over the horizon / a moving circle covers meanwhile


def diff_scene(T, accumulate, seed=0):
    """Diff-drive beside the start of a straight path, nominal controls that cover TRAVEL metres over the horizon whatever T,
    and three circles of threshold radius 0.8 (0.5 * 0.8 + 0.4):
      crosser -- comes down the path against the robot, 0.8 m to its left, and meets it at `meet` of the horizon: mid-horizon
                 when every step is priced, at step T when `S[k] =` prices the last state only.  Where it stands at step 0 it
                 is SWEEP * meet beyond the meeting point, where it stands at step T (accumulating) as far behind it.
      leaver  -- sits ON the nominal path at the meeting point at step 0 and leaves sideways: 0.75 * SWEEP away when the robot
                 gets there.
      static  -- 0.9 m to the right of the meeting point: catches the samples that stray 0.1 m that way.
    Returns dict(ref, x0, u, circles [3, 3], vel [3, 2])."""
    rng = np.random.default_rng(100 + seed)
    dt = DIFF_KW["delta_t"]
    ref = mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100)
    yaw = ref[0, 2]
    x0 = np.array([0.1, -0.05, yaw + 0.02])
    speed = TRAVEL / (T * dt)
    u = np.stack([np.full(T, speed), np.zeros(T)], axis=1) + rng.normal(0, 0.01, (T, 2))
    h = np.array([np.cos(x0[2]), np.sin(x0[2])])
    nrm = np.array([-h[1], h[0]])
    meet = round(0.5 * T) / T if accumulate else 1.0  # (a whole step: at T = 7 the two close 1.3 m per step)
    M = x0[:2] + meet * TRAVEL * h  # where the nominal rollout is at `meet` of the horizon
    horizon = T * dt
    crosser_v = -h * (SWEEP / horizon)
    crosser_c = M + 0.8 * nrm - crosser_v * (meet * horizon)
    leaver_v = nrm * (SWEEP / horizon)
    circles = np.array([[*crosser_c, 0.4], [*M, 0.4], [*(M - 0.9 * nrm), 0.4]])
    vel = np.array([crosser_v, leaver_v, [0.0, 0.0]])
    return dict(ref=ref, x0=x0, u=u, circles=circles, vel=vel)


def diff_oracle(sc, K, T, **kw):
    o = MovingDiffDriveOracle(ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T, obstacle_circles=sc["circles"],
                              obstacle_velocities=sc["vel"], **dict(DIFF_KW, **kw))
    o.u_prev[:] = sc["u"]
    return o


RACE_T = 40


def race_scene(seed=0):
    """Race car (outline model, `S[k] +=`: every step is tested) on a lemniscate, T = 40 steps of 0.05 s at ~5 m/s: 10 m of
    road.  crosser: a circle of radius 1 that comes down the road against the car, 3.7 m to its left (the outline's side
    points reach 2.25 m: it takes a car that steers its way), and passes it at mid-horizon -- at step 0 it stands 17 m ahead, at step T 7 m behind the start;
    leaver: sits on the road 7 m ahead and pulls out to the right before the car arrives; static: 4.0 m to the right of the
    road 3 m ahead."""
    path = mppi_oracle.generate_lemniscate_racecar(100, 10.0).astype(np.float64)
    s = path[2].copy()
    s[3] = 5.0
    h = np.array([np.cos(s[2]), np.sin(s[2])])
    nrm = np.array([-h[1], h[0]])
    horizon = RACE_T * 0.05
    cross_v = -h * (24.0 / horizon)
    cross_c = s[:2] + 5.0 * h + 3.7 * nrm - cross_v * (0.5 * horizon)
    leave_v = -nrm * (16.0 / horizon)
    circles = np.array([[*cross_c, 1.0], [*(s[:2] + 7.0 * h), 1.0], [*(s[:2] + 3.0 * h - 4.0 * nrm), 1.0]])
    vel = np.array([cross_v, leave_v, [0.0, 0.0]])
    u = np.random.default_rng(200 + seed).normal(0, 0.05, (RACE_T, 2))
    return dict(ref=path, x0=s, u=u, circles=circles, vel=vel)


RACE_KW = dict(delta_t=0.05, wheel_base=2.5, max_steer_abs=0.523, max_accel_abs=2.0, horizon_step_T=RACE_T, param_exploration=0.1,
               param_lambda=50.0, param_alpha=0.9, collision_safety_margin_rat=1.5, raise_at_path_end=False)


def race_oracle(sc, K):
    o = MovingRaceCarOracle(ref_path=sc["ref"], number_of_samples_K=K, obstacle_circles=sc["circles"],
                            obstacle_velocities=sc["vel"], **RACE_KW)
    o.u_prev[:] = sc["u"].astype(F32)
    return o


def penalised(S):
    return np.asarray(S) > 1e9


def kept(o, f64):
    """The samples an S comparison keeps: all of them for an f64 handle, those whose every tested pose lies outside the margin
    for an f32 one."""
    m = o.sample_margin()
    return np.ones(m.shape, bool) if f64 else m > MARGIN


def table(circles, vel, m):
    """m circles and velocities: the given ones first and LAST (a set of 65 or 70 keeps one beyond the 64 lanes of the table:
    it and its velocity come from memory), far ones that drift slowly in between."""
    circles, vel = np.asarray(circles, np.float64).reshape(-1, 3), np.asarray(vel, np.float64).reshape(-1, 2)
    n = len(circles)
    assert m >= 1
    if m <= n:
        return circles[:m].copy(), vel[:m].copy()
    c = np.stack([[1.0e3 + 3.0 * i, 1.0e3, 0.5] for i in range(m)])
    v = np.stack([[0.01 * (i % 7), -0.02] for i in range(m)])
    half = (n + 1) // 2
    c[:half], v[:half] = circles[:half], vel[:half]
    c[m - (n - half):], v[m - (n - half):] = circles[half:], vel[half:]
    return c, v


# ------------------------------------------------------------------------------------------ cases
K_CASE = 256
HORIZONS = (7, 50, 64, 65, 100, 128, 130)  # one chunk, the chunk seam, a full second chunk; 130: the unfused path


def diff_cases():
    """(T, accumulate, mode): every horizon with the frozen index, both sums; the threaded indices at one horizon of each kind"""
    out = [(T, acc, "frozen") for T in HORIZONS for acc in (False, True)]
    out += [(T, False, mode) for T in (50, 65, 130) for mode in ("per_rollout", "sequential")]
    out += [(100, True, mode) for mode in ("per_rollout", "sequential")]
    return out


# noise seeds: for each case the first seed at which the f64 reference itself leaves out at most MAX_LEFT_OUT of the samples
# (test_moving_obstacle_cases.py asserts it); cases not listed take seed 0
EPS_SEED = {(50, False, "frozen"): 1, (50, False, "per_rollout"): 1, (50, False, "sequential"): 1, (100, True, "frozen"): 1,
            (100, True, "per_rollout"): 1, (100, True, "sequential"): 1, (128, True, "frozen"): 1, (130, True, "frozen"): 3}


def eps_seed(T, accumulate, mode):
    return EPS_SEED.get((T, accumulate, mode), 0)


def diff_case(T, accumulate, mode, K=K_CASE, clock=0, freeze_at=None):
    """-> (scene, eps [K, T, 2] float32, oracle after one iteration at `clock`, its result)"""
    from oracle import philox
    sc = diff_scene(T, accumulate)
    eps = philox.sample_epsilon(DIFF_KW["sigma"], eps_seed(T, accumulate, mode), 0, K, T)
    o = diff_oracle(sc, K, T)
    o.set_motion(sc["vel"], clock, freeze_at)
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    return sc, eps, o, res


def race_case(K=K_CASE, clock=0, freeze_at=None, seed=0):
    from oracle import philox
    sc = race_scene()
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), seed, 0, K, RACE_T)
    o = race_oracle(sc, K)
    o.set_motion(sc["vel"], clock, freeze_at)
    res = o.iteration(sc["x0"], eps)
    return sc, eps, o, res


# the closed loop weighs the tracking error lightly, so that the softmin average over the samples that stay clear -- and with
# it the control trace -- follows where the circles are (under the default weights one best sample carries the update)
LOOP_KW = dict(stage_cost_weight=np.array([0.25, 0.25, 0.5]), terminal_cost_weight=np.array([0.25, 0.25, 0.5]))


def diff_closed_loop(T, n_iters, K=K_CASE, mode="frozen", accumulate=False, seed=31, tick=True, eps_of=None):
    """The closed loop of mppi_run_closed_loop against the diff-drive plant: one iteration, the plant step with the returned
    u0, one tick of the obstacle clock -- n_iters times, noise of iteration i from the sampler (philox.sample_epsilon with
    that iteration counter).  -> dict(u0 [n, 2], x [3], idx, n_hit [n], kept [n] fractions for f32 handles)"""
    from oracle import philox
    sc = diff_scene(T, accumulate)
    o = diff_oracle(sc, K, T, **LOOP_KW)
    x = sc["x0"].copy()
    u0, hits, keep = [], [], []
    for i in range(n_iters):
        o.reset_margins()
        eps = philox.sample_epsilon(DIFF_KW["sigma"], seed, i, K, T) if eps_of is None else eps_of(i)
        res = o.iteration_general(x, eps.astype(np.float64), mode, accumulate)
        u0.append(res["u0_returned"].copy())
        hits.append(int(penalised(res["S"]).sum()))
        keep.append(float((o.sample_margin() > MARGIN).mean()))
        x = mppi_oracle.diffdrive_plant_step(x, res["u0_returned"], DIFF_KW["delta_t"])
        if tick:
            o.tick()
    return dict(scene=sc, u0=np.array(u0), x=x, idx=o.prev_way_point_idx, n_hit=hits, kept=keep, oracle=o)
