"""Fleet plans (mppi_set_fleet_prediction, MPPI_FLEET_PLAN): the f64 definition of a plan, the error model of a plan
point, per-agent oracles whose mates stand where their plans put them, and the scenes of test_fleet_plan_cases.py (CPU) and
test_gpu_fleet_plan.py.  No device import.

The reference: `plans` restates the header's definition -- sequential Euler steps of the nominal controls in f64.  An agent's
oracle is the moving-obstacle oracle of tests/moving_obstacle_checks.py whose `_test` takes, beside the agent's own circles at
the step of the call, one centre per mate from a table indexed by that same step."""
import numpy as np

import fleet_checks as fc
import moving_obstacle_checks as mc
from oracle import mppi_oracle

EPS = fc.EPS


# ------------------------------------------------------------------------------------------ the definition
def plan_cfg(model, clamp=True):
    if model == "race":
        return dict(dt=0.05, u_max=(0.523, 2.0), wheel_base=2.5, clamp=clamp)
    return dict(dt=mc.DIFF_KW["delta_t"], u_max=(mc.DIFF_KW["max_speed"], mc.DIFF_KW["max_omega"]), wheel_base=0.0, clamp=clamp)


def clamped(u, cfg):
    u = np.asarray(u, np.float64)
    return np.clip(u, [-cfg["u_max"][0], -cfg["u_max"][1]], [cfg["u_max"][0], cfg["u_max"][1]]) if cfg["clamp"] else u


def plans(states, u, model, cfg):
    """states [B, nx], u [B, T, 2] (the nominal sequences), model "diff" | "race" -> [B, T + 1, 2] in f64: point 0 the state's
    (x, y), point j the position after the model's Euler steps with rows 0 .. j - 1, clamped where the rollout clamps."""
    x, v = np.asarray(states, np.float64), clamped(u, cfg)
    B, T = v.shape[:2]
    dt = float(cfg["dt"])
    out = np.empty((B, T + 1, 2))
    for a in range(B):
        px, py, yaw = x[a, 0], x[a, 1], x[a, 2]
        vel = x[a, 3] if model == "race" else 0.0
        out[a, 0] = px, py
        for j in range(T):
            if model == "race":  # controls = [steer, accel]
                px, py, yaw, vel = (px + vel * np.cos(yaw) * dt, py + vel * np.sin(yaw) * dt,
                                    yaw + vel / cfg["wheel_base"] * np.tan(v[a, j, 0]) * dt, vel + v[a, j, 1] * dt)
            else:
                px, py, yaw = px + v[a, j, 0] * np.cos(yaw) * dt, py + v[a, j, 0] * np.sin(yaw) * dt, yaw + v[a, j, 1] * dt
            out[a, j + 1] = px, py
    return out


# ------------------------------------------------------------------------------------------ the error model
def _point_bounds(x, v, model, cfg, eps):
    """Bound [T + 1] on |device point - exact point| per coordinate for one agent, eps the spacing of the arithmetic at 1 (a
    rounding errs by h = eps / 2 relative).  One term per rounding, in the order the kernel makes them:
      the state to R                         h |p0|, h |yaw0|, h |v0|
      the clamp limits to R                  h |control| on a clamped row (taken for every row)
      dt to R                                h on every increment
      the increments' products               h each (v1 dt: one; v0 cs dt: two; vel / L tan dt: three and the division)
      the prefix sums                        step i is reached through at most i + 1 additions (the wave scan associates
                                             differently and needs fewer), each h of the running magnitude, and one more for
                                             the carried state
      sincos in R (mathfn.h: <= 2 ulp)       2 eps absolute on cos and sin
      race car: tan (<= 2 ulp)               2 eps relative; the wheel base to R and the division h each; the speed is a
                                             prefix sum of its own, whose error enters the yaw increments and the positions
    A yaw error d turns the step's increment by d: |v| dt d on the position."""
    T = v.shape[0]
    dt, h = float(cfg["dt"]), 0.5 * eps
    sc_err, tan_err = 2.0 * eps, 2.0 * eps
    p0 = float(np.abs(x[:2]).max())
    if model == "race":
        acc = np.abs(v[:, 1]) * dt
        vel = x[3] + np.concatenate([[0.0], np.cumsum(v[:, 1] * dt)])          # exact speeds before step i (i = 0 .. T)
        a_abs = np.concatenate([[0.0], np.cumsum(acc)])
        v_run = abs(x[3]) + a_abs
        e_vel = h * abs(x[3]) + 3.0 * h * a_abs + (np.arange(T + 1) + 1) * h * v_run
        tn = np.abs(np.tan(v[:, 0]))
        dyaw = np.abs(vel[:T]) / cfg["wheel_base"] * tn * dt
        e_dyaw = e_vel[:T] / cfg["wheel_base"] * tn * dt + dyaw * (6.0 * h + tan_err)
        inc = np.abs(vel[:T]) * dt
        e_extra = e_vel[:T] * dt
    else:
        dyaw = np.abs(v[:, 1]) * dt
        e_dyaw = dyaw * 3.0 * h
        inc = np.abs(v[:, 0]) * dt
        e_extra = np.zeros(T)
    y_run = abs(x[2]) + np.concatenate([[0.0], np.cumsum(dyaw)])
    e_yaw = h * abs(x[2]) + np.concatenate([[0.0], np.cumsum(e_dyaw)]) + (np.arange(T + 1) + 1) * h * y_run  # before step i
    e_inc = inc * (e_yaw[:T] + sc_err + 4.0 * h) + e_extra
    p_run = p0 + np.concatenate([[0.0], np.cumsum(inc)])
    return h * p0 + np.concatenate([[0.0], np.cumsum(e_inc)]) + (np.arange(T + 1) + 1) * h * p_run * (np.arange(T + 1) > 0)


def plan_bounds(states, u, model, cfg, precision):
    """[B, T + 1]: what a point read back from a handle of `precision` may differ by from `plans`, per coordinate -- the model
    at the handle's eps, plus the same model at the f64 eps for the reference's own arithmetic."""
    x, v = np.asarray(states, np.float64), clamped(u, cfg)
    return np.stack([_point_bounds(x[a], v[a], model, cfg, EPS[precision]) + _point_bounds(x[a], v[a], model, cfg, EPS["f64"])
                     for a in range(len(x))])


def check_plans(got, states, u, model, cfg, precision):
    """Plans read back against the definition, every point held to the model; -> the largest error / bound."""
    want, bound = plans(states, u, model, cfg), plan_bounds(states, u, model, cfg, precision)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max(axis=2)
    ratio = err / bound
    a, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[a, j] <= 1.0, (model, precision, int(a), int(j), float(err[a, j]), float(bound[a, j]), got[a, j], want[a, j])
    return float(ratio[a, j])


# ------------------------------------------------------------------------------------------ per-agent oracles
class _Plans:
    """Mates from a table: mate_plans [m, T + 1, 2], tested with the squared threshold plan_thr2 at the step of the call."""
    mate_plans = None
    plan_thr2 = None

    def _test(self, px, py, r2, steps):
        c = mc.centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps)
        r2 = np.broadcast_to(r2, (c.shape[-2],))
        if self.mate_plans is not None and len(self.mate_plans):
            j = np.asarray(steps)  # (_steps_of has applied freeze_at already)
            c = np.concatenate([c, np.moveaxis(self.mate_plans[:, j, :], 0, -2)], axis=-2)
            r2 = np.concatenate([r2, np.full(len(self.mate_plans), self.plan_thr2)])
        d2 = (px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2
        hit = (d2 < r2).any(axis=(-1, -2))
        margin = (np.abs(d2 - r2) / r2).min(axis=(-1, -2))
        self.margins.append(margin.reshape(margin.shape[0], -1))
        return hit


class PlanDiffDriveOracle(_Plans, mc.MovingDiffDriveOracle):
    pass


class PlanRaceCarOracle(_Plans, mc.MovingRaceCarOracle):
    pass


def threshold2(model):
    return fc.thr_of(model)(fc.rows_cfg(model)["fleet_radius"]) ** 2


def agent_oracle(sc, a, K, T, **kw):
    if sc["model"] == "race":
        o = PlanRaceCarOracle(ref_path=sc["refs"][a], number_of_samples_K=K, obstacle_circles=np.zeros((0, 3)), **mc.RACE_KW)
        o.u_prev[:] = sc["u"][a].astype(np.float32)
    else:
        o = PlanDiffDriveOracle(ref_path=sc["refs"][a], num_samples_K=K, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)),
                                **dict(mc.DIFF_KW, **kw))
        o.u_prev[:] = sc["u"][a]
    return o


def aim(o, own, mate_plans, thr2, n, freeze_at=None):
    """Point oracle o at its own circles (uploaded at clock 0, now at clock n) and its mates' plans."""
    c, v = np.asarray(own[0], np.float64).reshape(-1, 3), np.asarray(own[1], np.float64).reshape(-1, 2)
    if len(c) == 0:  # (the oracles' margin bookkeeping wants a circle: one that nothing reaches)
        c, v = np.array([[1.0e6, 1.0e6, 0.1]]), np.zeros((1, 2))
    o.obstacle_circles = c
    o.set_motion(v, n, freeze_at)
    o.mate_plans, o.plan_thr2 = np.asarray(mate_plans, np.float64), thr2


def mates_of(P, b):
    return P[[a for a in range(len(P)) if a != b]]


def one_iteration(sc, eps, K, T, mode="frozen", accumulate=False, own=None, what="plan", n=0, **kw):
    """One iteration of every agent at clock n: eps [B, K, T, 2].  what: "plan" the mates' plans, "frozen0" the mates where they
    stand at point 0, "cv" the constant-velocity rows of fleet_checks, "none" nobody sees anybody.
    -> list of (oracle, result) per agent"""
    if what in ("cv", "none"):
        return fc.one_iteration(sc, eps, K, T, mode, accumulate, own=own, mates=what == "cv", n=n, **kw)
    B, model = len(sc["refs"]), sc["model"]
    P = plans(sc["x0"], sc["u"], model, plan_cfg(model))
    if what == "frozen0":
        P = np.repeat(P[:, :1], P.shape[1], axis=1)
    out = []
    for a in range(B):
        o = agent_oracle(sc, a, K, T, **kw)
        aim(o, fc.NO_OWN if own is None else own[a], mates_of(P, a), threshold2(model), n)
        if model == "race":
            res = o.iteration(sc["x0"][a], eps[a])
        else:
            res = o.iteration_general(sc["x0"][a], np.asarray(eps[a], np.float64), mode, accumulate)
        out.append((o, res))
    return out


def closed_loop(sc, eps_of, n_iters, K, T, own=None, what="plan", mode="frozen", accumulate=False, **kw):
    """The batched closed loop in plan mode: per iteration the plans from the states and nominal controls as they stand, one
    iteration per agent, the plant, one tick.  what "cv": fleet_checks.closed_loop (the constant-velocity rows).
    -> as fleet_checks.closed_loop"""
    if what == "cv":
        return fc.closed_loop(sc, eps_of, n_iters, K, T, own=own, mode=mode, accumulate=accumulate, **kw)
    B, model = len(sc["refs"]), sc["model"]
    dt = fc.dt_of(model)
    os_ = [agent_oracle(sc, a, K, T, **kw) for a in range(B)]
    x = sc["x0"].copy()
    xs, hits, keep, Ss, us = [x.copy()], [], [], [], []
    for i in range(n_iters):
        u_now = np.stack([o.u_prev.copy() for o in os_])
        P = plans(x, u_now, model, plan_cfg(model))
        eps = eps_of(i)
        us.append(u_now)
        nx, row_h, row_k, row_S = [], [], [], []
        for a, o in enumerate(os_):
            aim(o, fc.NO_OWN if own is None else own[a], mates_of(P, a), threshold2(model), i)
            res = o.iteration_general(x[a], np.asarray(eps[a], np.float64), mode, accumulate)
            row_h.append(int((np.asarray(res["S"]) >= 1.0e10).sum()))
            row_k.append(o.sample_margin() > mc.MARGIN)
            row_S.append(np.asarray(res["S"], np.float64))
            nx.append(mppi_oracle.diffdrive_plant_step(x[a], res["u0_returned"], dt))
        x = np.stack(nx)
        xs.append(x.copy())
        hits.append(row_h)
        keep.append(row_k)
        Ss.append(row_S)
    return dict(x=np.array(xs), u=np.stack([o.u_prev.copy() for o in os_]), u_start=np.array(us), n_hit=np.array(hits),
                kept=np.array(keep), S=np.array(Ss))


# ------------------------------------------------------------------------------------------ scenes
def arc_scene(T, accumulate, seed=0):
    """Three diff-drive robots on the frame of fleet_checks.crossing_scene, nominal controls that cover mc.TRAVEL metres over
    the horizon:
      0  along +x from the origin;
      1  starts with 0's heading at 1.5 x its speed and turns right by pi / 2 over the horizon, placed so that its nominal
         rollout stands 0.8 m -- the threshold radius -- ahead-left of 0's nominal rollout at the meeting step: step T where
         `S[k] =` prices the last state only, mid-horizon where every step is priced.  Extrapolated at constant velocity from
         its start it never comes near 0;
      2  parallel to 0, 6 m to its left."""
    rng = np.random.default_rng(700 + seed)
    dt = mc.DIFF_KW["delta_t"]
    H = T * dt
    s0 = mc.TRAVEL / H
    jm = int(round(0.5 * T)) if accumulate else T
    u1 = np.stack([np.full(T, 1.5 * s0), np.full(T, -(0.5 * np.pi) / H)], axis=1) + rng.normal(0, 0.01, (T, 2))
    u0 = np.stack([np.full(T, s0), np.zeros(T)], axis=1) + rng.normal(0, 0.01, (T, 2))
    cfg = plan_cfg("diff")
    rel = plans([[0.0, 0.0, 0.0]], u1[None], "diff", cfg)[0]
    p0 = plans([[0.05, -0.03, 0.01]], u0[None], "diff", cfg)[0]
    target = p0[jm] + np.array([0.8, 0.8]) / np.sqrt(2.0) * 0.999
    s1 = target - rel[jm]
    x0 = np.array([[0.05, -0.03, 0.01], [s1[0], s1[1], 0.0], [0.0, 6.0, 0.0]])
    refs = [fc.line((0.0, 0.0), (10.0, 0.0)), fc.line((s1[0], s1[1]), (s1[0] + 10.0, s1[1])), fc.line((0.0, 6.0), (10.0, 6.0))]
    return dict(refs=refs, x0=x0, u=np.stack([u0, u1, u0.copy()]), model="diff")


def arc_own(sc):
    """Own moving sets for the arc scene (those of test_gpu_fleet.py's loop): one circle drifting beside agent 0's path, none
    for agent 1, two for agent 2"""
    return [(np.array([[2.0, -1.0, 0.4]]), np.array([[0.0, 0.25]])), fc.NO_OWN,
            (np.array([[2.5, 6.9, 0.4], [1.0, 5.0, 0.3]]), np.array([[-0.3, 0.0], [0.2, 0.1]]))]


def race_curve_scene(seed=0):
    """fleet_checks.race_pair_scene with a mate that follows the road: car 1 comes against car 0 on the outer side of the
    lemniscate's bend and steers with it (0.1 rad on top of the pair scene's nominal steering, over the whole horizon), so that
    its planned trajectory bends towards car 0's lane where the constant-velocity prediction drives straight on: 0.70 of car
    0's samples are penalised under the plan, a third of them otherwise under either other prediction."""
    sc = fc.race_pair_scene(seed)
    u = sc["u"].copy()
    u[1, :, 0] += 0.1
    return dict(sc, u=u)


def scatter_scene(model, B, T, seed=0):
    """B agents scattered around one shared path, nominal controls partly beyond the clamp (plan read-back)"""
    rng = np.random.default_rng(800 + 7 * B + T + seed)
    if model == "race":
        ref = mppi_oracle.generate_lemniscate_racecar(100, 10.0).astype(np.float64)
        x0 = np.stack([rng.uniform(-12, 12, B), rng.uniform(-6, 6, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(2.0, 6.0, B)], axis=1)
        u = np.stack([rng.uniform(-0.7, 0.7, (B, T)), rng.uniform(-2.5, 2.5, (B, T))], axis=2)
    else:
        ref = fc.line((0.0, 0.0), (10.0, -5.0))
        x0 = np.stack([rng.uniform(-5, 15, B), rng.uniform(-10, 5, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
        u = np.stack([rng.uniform(-1.0, 6.0, (B, T)), rng.uniform(-4.0, 4.0, (B, T))], axis=2)
    return dict(refs=[ref] * B, x0=x0, u=u, model=model)


# one-iteration cases: (T, accumulate, mode)
def arc_cases():
    out = [(T, acc, "frozen") for T in (7, 50, 65, 128) for acc in (False, True)]
    return out + [(50, acc, "per_rollout") for acc in (False, True)]


# noise seeds (mppi_config.seed; the handles of tests/test_gpu_fleet.py take 99): for each case the first seed from 99 on at
# which the f64 reference itself leaves out at most mc.MAX_LEFT_OUT of every agent's samples, with and without the own sets of
# arc_own (test_fleet_plan_cases.py asserts it); cases not listed take 99.  What seed 99 gave for the two listed cases: agent 0
# (the agent the scene is built for) leaves out 0.000, but agent 1 -- the turning mate, which the GPU tests compare as well --
# leaves out 0.0195 (5 of 256 samples within the margin of agent 0's plan) and agent 2 with its own circles 0.0156; under seed
# 100 every agent leaves out at most 0.0078.
EPS_SEED = {(50, True, "frozen"): 100, (50, True, "per_rollout"): 100}


def eps_seed(T, accumulate, mode):
    return EPS_SEED.get((T, accumulate, mode), 99)


def penalised_of(runs, a=0):
    return mc.penalised(np.asarray(runs[a][1]["S"], np.float64))
