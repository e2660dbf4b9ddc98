"""Learned-dynamics fleets (mppi_config.obstacle_motion = 3): the f64 reference, the margin rule and the scenes of
test_mlp_fleet_cases.py (CPU) and test_gpu_mlp_fleet.py.  No device import.

Nothing new is priced here: the reference is composed from what exists.
  the per-agent oracle   mlp_scene_checks._Learned (the learned transition) over fleet_plan_checks._Plans (mates from a plan table)
                         over moving_obstacle_checks.MovingDiffDriveOracle (own moving circles; in velocity mode the mates' rows of
                         fleet_checks.mate_rows behind them);
  `learned_plans`        point 0 the state's (x, y), then the first two columns of DiffDriveMlpOracle.rollout of the clamped nominal
                         rows through the agent's own weights;
  the weights            mlp_scene_checks.scene_weights(H, n, x0_a, u_a, seed=100 + a).

THE MARGIN.  A sample is left out of the S / hit comparisons when any pose it tests lies within 2 DELTA of a mate's threshold
circle, DELTA = mlp_scene_checks.delta(): the sample's own state error plus the plan point's, both the learned transition's error
against f64 as the project measured it on code the fleet forms do not change (profiles/mlp_scene_measured.json).  Own circles keep
mlp_scene_checks' rule (DELTA).  Under the outline model (MPPI_OBSTACLE_OUTLINE: the eight outline points are tested, the
thresholds are the radii themselves) the sample's own error is delta(outline=True) -- its position error plus its yaw error times
the outline's reach --, so a mate's margin is delta(outline=True) + delta() and an own circle's delta(outline=True).
MAX_LEFT_OUT is a condition on the scenes, not a measurement."""
import functools

import numpy as np

import fleet_checks as fc
import fleet_plan_checks as fp
import grid_footprint_checks as gf
import mlp_scene_checks as ms
import moving_obstacle_checks as mc
from oracle import mppi_oracle

K = ms.K
MAX_LEFT_OUT = ms.MAX_LEFT_OUT
KW = {k: v for k, v in mc.DIFF_KW.items() if k != "safety_margin_rate"}
DT = mc.DIFF_KW["delta_t"]
THR = float(np.sqrt(fp.threshold2("diff")))  # 0.5 * 0.8 + 0.4


# ------------------------------------------------------------------------------------------ the plans
def learned_plans(states, u, weights_per_agent):
    """states [B, 3], u [B, T, 2], one weight dict per agent -> [B, T + 1, 2] in f64"""
    x, cfg = np.asarray(states, np.float64), fp.plan_cfg("diff")
    out = []
    for a, w in enumerate(weights_per_agent):
        v = fp.clamped(u[a], cfg)
        o = mppi_oracle.DiffDriveMlpOracle(ref_path=np.zeros((2, 3)), num_samples_K=1, num_horizons_T=len(v), **KW, mlp_weights=w)
        out.append(np.concatenate([x[a, None, :2], o.rollout(x[a], v[None])[0][:, :2]]))
    return np.stack(out)


def zeroed(w):
    return dict(w, **{"out_layer.weight": w["out_layer.weight"] * 0, "out_layer.bias": w["out_layer.bias"] * 0})


# ------------------------------------------------------------------------------------------ the per-agent oracle
class _MateMargin:
    """per tested pose, the distance to the nearest threshold circle in units of the error allowed there: DELTA for the agent's
    own circles, 2 DELTA for its mates (the last n_mate_rows rows of the table in velocity mode, the plan table in plan mode);
    under the outline model delta(outline) and delta(outline) + delta()"""
    n_mate_rows = 0
    outline = False

    def set_motion(self, *a, **kw):
        super().set_motion(*a, **kw)
        self.unit_margins = []

    def _test(self, px, py, r2, steps):
        K_ = px.shape[0]
        d0, d_mate = ms.delta(self.outline), ms.delta(self.outline) + ms.delta()
        c = mc.centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps)
        unit = np.full(len(self.obstacle_circles), d0)
        if self.n_mate_rows:
            unit[-self.n_mate_rows:] = d_mate
        d = np.sqrt((px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2)
        m = (np.abs(d - np.sqrt(np.broadcast_to(r2, unit.shape))) / unit).min(axis=(-1, -2))
        if self.mate_plans is not None and len(self.mate_plans):
            cm = np.moveaxis(self.mate_plans[:, np.asarray(steps), :], 0, -2)
            d = np.sqrt((px[..., :, None] - cm[..., None, :, 0]) ** 2 + (py[..., :, None] - cm[..., None, :, 1]) ** 2)
            m = np.minimum(m, (np.abs(d - np.sqrt(self.plan_thr2)) / d_mate).min(axis=(-1, -2)))
        self.unit_margins.append(m.reshape(K_, -1))
        return super()._test(px, py, r2, steps)

    def sample_unit_margin(self):
        return np.concatenate(self.unit_margins, axis=1).min(axis=1)


class LearnedFleetOracle(ms._Learned, _MateMargin, fp._Plans, mc.MovingDiffDriveOracle):
    pass


class _Outline:
    """MPPI_OBSTACLE_OUTLINE on the diff-drive box of grid_footprint_checks.DIFF_BOX: the eight outline points of every priced
    state (its yaw from the rollout) against the own circles and the mates, each threshold the radius itself"""
    outline = True

    def half_sides(self):
        return 0.5 * gf.DIFF_BOX["vehicle_l"] * self.safety_margin_rate, 0.5 * gf.DIFF_BOX["vehicle_w"] * self.safety_margin_rate

    def collided(self, x, y, steps=None):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        yaw = self._X[..., 2] if x.ndim == 2 else self._X[:, -1, 2]  # [K, T] stage states / [K] last states
        p = gf.world_points(x, y, np.asarray(yaw, np.float64), *self.half_sides())[..., 1:, :]
        return self._test(p[..., 0], p[..., 1], self.obstacle_circles[:, 2] ** 2, self._steps_of(x.shape, steps)).astype(np.float64)


class LearnedFleetOutlineOracle(_Outline, LearnedFleetOracle):
    pass


def plan_threshold2(outline):
    """the mates' squared threshold as make_fleet packs it: (0.5 safety_margin + fleet_radius)^2 for the disc, fleet_radius^2 for
    the outline"""
    return fc.RADIUS ** 2 if outline else fp.threshold2("diff")


def agent_oracle(sc, a, K_, T, **kw):
    if sc.get("outline"):
        kw = dict(kw, safety_margin_rate=gf.DIFF_BOX["safety_margin"])
    cls = LearnedFleetOutlineOracle if sc.get("outline") else LearnedFleetOracle
    o = cls(ref_path=sc["refs"][a], num_samples_K=K_, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)), **dict(mc.DIFF_KW, **kw))
    o.u_prev[:] = sc["u"][a]
    o.mlp_weights = sc["w"][a]
    return o


def kept(o):
    return o.sample_unit_margin() > 1.0


def aim(o, sc, a, what, own, n, P=None, rows=None):
    """what: "plan" (P: every agent's plan), "velocity" (rows: fleet_checks.mate_rows), "none" nobody sees anybody"""
    own_a = fc.NO_OWN if own is None else own[a]
    o.mate_plans, o.n_mate_rows = None, 0
    if what == "plan":
        fp.aim(o, own_a, fp.mates_of(P, a), plan_threshold2(bool(sc.get("outline"))), n)
    else:
        mates = what == "velocity"
        fc.aim(o, own_a, rows[0][a] if mates else rows[0][a][:0], rows[1][a] if mates else rows[1][a][:0], DT, n)
        o.n_mate_rows = len(sc["refs"]) - 1 if mates else 0


def one_iteration(sc, eps, T, mode="frozen", accumulate=False, what="plan", own=None, n=0, plans=None, K_=K):
    """One iteration of every agent at clock n: eps [B, K, T, 2]; plans: the table the agents see in plan mode (default: the
    learned plans).  -> list of (oracle, result) per agent"""
    B = len(sc["refs"])
    P = (learned_plans(sc["x0"], sc["u"], sc["w"]) if plans is None else plans) if what == "plan" else None
    rows = fc.mate_rows(sc["x0"], sc["u"][:, 0], "diff", fc.rows_cfg("diff"))
    out = []
    for a in range(B):
        o = agent_oracle(sc, a, K_, T)
        aim(o, sc, a, what, own, n, P, rows)
        res = o.iteration_general(sc["x0"][a], np.asarray(eps[a], np.float64), mode, accumulate)
        res["w"] = o.compute_weight(np.asarray(res["S"], np.float64))
        out.append((o, res))
    return out


def closed_loop(sc, eps_of, n_iters, T, what, own=None, mode="frozen", accumulate=False, K_=K):
    """The batched closed loop, re-seeded by the caller per iteration if it wants: per iteration the plans or rows from the
    states and nominal controls as they stand, one iteration per agent, the plant, one tick.  -> as fleet_checks.closed_loop"""
    B = len(sc["refs"])
    os_ = [agent_oracle(sc, a, K_, T) for a in range(B)]
    x = sc["x0"].copy()
    xs, keep, Ss, us = [x.copy()], [], [], []
    for i in range(n_iters):
        u_now = np.stack([o.u_prev.copy() for o in os_])
        P = learned_plans(x, u_now, sc["w"]) if what == "plan" else None
        rows = fc.mate_rows(x, u_now[:, 0], "diff", fc.rows_cfg("diff"))
        eps = eps_of(i)
        us.append(u_now)
        nx, row_k, row_S = [], [], []
        for a, o in enumerate(os_):
            aim(o, sc, a, what, own, i, P, rows)
            res = o.iteration_general(x[a], np.asarray(eps[a], np.float64), mode, accumulate)
            row_k.append(kept(o))
            row_S.append(np.asarray(res["S"], np.float64))
            nx.append(mppi_oracle.diffdrive_plant_step(x[a], res["u0_returned"], DT))
        x = np.stack(nx)
        xs.append(x.copy())
        keep.append(row_k)
        Ss.append(row_S)
    return dict(x=np.array(xs), u=np.stack([o.u_prev.copy() for o in os_]), u_start=np.array(us), kept=np.array(keep), S=np.array(Ss))


# ------------------------------------------------------------------------------------------ scenes
def fleet_weights(H, n, x0, u, per_agent=True):
    """a model per agent (seed 100 + a, scaled for the agent's own nominal rollout), or agent 0's for all"""
    ws = [ms.scene_weights(H, n, x0[a], u[a], seed=100 + a) for a in range(len(x0) if per_agent else 1)]
    return ws if per_agent else ws * len(x0)


@functools.lru_cache(maxsize=None)
def arc_scene(T, H=64, n=1, per_agent=True):
    """fleet_plan_checks.arc_scene for `S[k] =` (the last state is priced) placed around the LEARNED plans: mate 1's start is moved
    by fixed-point steps until its learned plan stands 0.999 x 0.8 m ahead-left of agent 0's learned plan at step T (its weights
    are scaled for its own nominal rollout from the start of the fourth placement, within a millimetre of the last)."""
    sc = fp.arc_scene(T, False)
    x0, u = sc["x0"].copy(), sc["u"]
    for i in range(60):  # (four placements with the weights made afresh, then the placement alone with the last weights)
        if i < 4:
            w = fleet_weights(H, n, x0, u, per_agent)
        P = learned_plans(x0, u, w)
        step = P[0, T] + np.array([0.8, 0.8]) / np.sqrt(2.0) * 0.999 - P[1, T]
        if np.linalg.norm(step) < 1e-9:
            break
        x0[1, :2] += step
    assert np.linalg.norm(step) < 1e-6, step
    refs = [sc["refs"][0], fc.line(tuple(x0[1, :2]), (x0[1, 0] + 10.0, x0[1, 1])), sc["refs"][2]]
    return dict(refs=refs, x0=x0, u=u, w=w, model="diff", shape=(H, n), per_agent=per_agent)


# the side scene's stand-off of the mate's lane from agent 0's, found by a scan on the f64 reference over 0.75 .. 1.1 m: the
# value at which the conditions of test_mlp_fleet_cases.py hold with one model for all and with a model per agent (T = 50, every
# step priced: 0.80 / 0.34 of agent 0's samples penalised under the learned plans, 0.36 under the analytic ones)
SIDE_GAP = {7: 0.85, 50: 0.85}


@functools.lru_cache(maxsize=None)
def side_scene(T, H=64, n=1, per_agent=True, gap=None):
    """Every step priced: agent 0 along +x, mate 1 on a parallel lane `gap` metres to its left at the same speed -- under its
    analytic plan it keeps that distance, under its learned plan its residual drifts it by the 0.3 m scene_weights gives --,
    agent 2 parallel 6 m to the left (out of reach)."""
    rng = np.random.default_rng(900 + T)
    gap = SIDE_GAP.get(T, 0.85) if gap is None else gap
    s0 = mc.TRAVEL / (T * DT)
    u = np.stack([np.stack([np.full(T, s0), np.zeros(T)], axis=1) + rng.normal(0, 0.01, (T, 2)) for _ in range(3)])
    x0 = np.array([[0.05, -0.03, 0.01], [0.0, gap, 0.0], [0.0, 6.0, 0.0]])
    refs = [fc.line((0.0, 0.0), (10.0, 0.0)), fc.line((0.0, gap), (10.0, gap)), fc.line((0.0, 6.0), (10.0, 6.0))]
    return dict(refs=refs, x0=x0, u=u, w=fleet_weights(H, n, x0, u, per_agent), model="diff", shape=(H, n), per_agent=per_agent)


# the outline scene: the side scene with the mate's lane OUTLINE_GAP to agent 0's left -- the box's side points reach 0.25 m and the
# threshold is fleet_radius = 0.4 m --, from a scan on the f64 reference (see test_mlp_fleet_cases.py for the conditions)
OUTLINE_GAP = 0.7


def outline_scene(T, gap=None):
    return dict(side_scene(T, 64, 1, True, OUTLINE_GAP if gap is None else gap), outline=True)


def scene_of(T, accumulate, H=64, n=1, per_agent=True, what="plan"):
    """plan mode: the arc scene where the last state is priced, the side scene where every step is; velocity mode: the side scene
    (extrapolated at constant velocity the arc scene's mate never comes near agent 0)"""
    return side_scene(T, H, n, per_agent) if accumulate or what != "plan" else arc_scene(T, H, n, per_agent)


def far_scene(B, T, H=64, n=1):
    sc = fc.far_scene(B, T)
    return dict(sc, w=fleet_weights(H, n, sc["x0"], sc["u"]), shape=(H, n), per_agent=True)


def scatter_scene(B, T, H, n, per_agent):
    """fleet_plan_checks.scatter_scene (controls partly beyond the clamp) with models: the plan read-back"""
    sc = fp.scatter_scene("diff", B, T)
    ws = [ms.weights(H, n, 100 + a) for a in range(B if per_agent else 1)]
    return dict(sc, w=ws if per_agent else ws * B, shape=(H, n), per_agent=per_agent)


def arc_own(sc):
    """own moving sets: one circle drifting beside agent 0's path, none for agent 1, two for agent 2"""
    return fp.arc_own(sc)


# one-iteration cases: (T, accumulate, mode, H, n, per_agent)
def cases():
    out = [(7, False, "frozen", 64, 1, False), (50, False, "frozen", 64, 1, False), (50, True, "frozen", 64, 1, False),
           (50, False, "per_rollout", 64, 1, False), (50, True, "per_rollout", 64, 1, False),
           (50, False, "frozen", 64, 1, True), (50, True, "frozen", 64, 1, True)]
    return out + [(50, False, "frozen", 128, 2, False), (50, True, "frozen", 256, 3, False), (50, False, "frozen", 512, 3, False)]


def numpy_noise(T, B=3, seed=99, it=0, K_=K):
    return fc.numpy_noise(mc.DIFF_KW["sigma"], seed, it, B, K_, T)


@functools.lru_cache(maxsize=None)
def case(T, accumulate, mode, H=64, n=1, per_agent=False, what="plan", with_own=False):
    """-> (scene, own, eps [B, K, T, 2] float32 as oracle/philox.py draws it for seed 99, runs).  The GPU tests hold
    mppi_sample_epsilon to the same arrays first."""
    sc = scene_of(T, accumulate, H, n, per_agent, what)
    own = arc_own(sc) if with_own else None
    eps = numpy_noise(T)
    return sc, own, eps, one_iteration(sc, eps, T, mode, accumulate, what, own)


def penalised_of(runs, a=0):
    return mc.penalised(np.asarray(runs[a][1]["S"], np.float64))


# ------------------------------------------------------------------------------------------ plans beside tracks and a grid
class _PlanAbsMargin:
    """mlp_scene_checks._AbsMargin's bookkeeping (metres, compared with DELTA) for the mates' plan points: half the distance to
    a mate's threshold circle, so that the comparison with DELTA is the 2 DELTA rule"""

    def _test(self, px, py, r2, steps):
        if self.mate_plans is not None and len(self.mate_plans):
            cm = np.moveaxis(np.asarray(self.mate_plans)[:, np.asarray(steps), :], 0, -2)
            d = np.sqrt((px[..., :, None] - cm[..., None, :, 0]) ** 2 + (py[..., :, None] - cm[..., None, :, 1]) ** 2)
            self.abs_margins.append((0.5 * np.abs(d - np.sqrt(self.plan_thr2)).min(axis=(-1, -2))).reshape(px.shape[0], -1))
        return super()._test(px, py, r2, steps)


class ComposedFleetOracle(ms._Learned, _PlanAbsMargin, ms._AbsMargin, ms.sk.SceneDiffDriveOracle):
    pass


# the mate's lane in the composed scene: 1.3 m to agent 0's RIGHT, from a scan on the f64 reference (to the left the mates hit every
# sample up to 0.75 m and none from 0.8 m on; to the right 0.95 at 0.85 m, 0.62 at 1.2 m, 0.32 at 1.3 m, 0.14 at 1.4 m of agent 0's
# samples, beside the 0.76 its tracks hit and the 0.08 its circles hit)
COMPOSED_GAP = -1.3


@functools.lru_cache(maxsize=None)
def composed_scene(T=50, gap=COMPOSED_GAP):
    """mlp_scene_checks' composed scene (two own circles, tracks and a grid, every step priced) for agent 0, mate 1 on a parallel
    lane `gap` metres to its left (negative: to its right), agent 2 six metres to the left; the mates own nothing"""
    s0 = ms.scene("composed", T, True)
    h, nrm = ms.sk.heading(s0["x0"])
    x0 = np.stack([s0["x0"], s0["x0"] + np.array([*(gap * nrm), 0.0]), s0["x0"] + np.array([*(6.0 * nrm), 0.0])])
    refs = [s0["ref"]] + [s0["ref"] + np.array([*(x0[a, :2] - x0[0, :2]), 0.0]) for a in (1, 2)]
    u = np.stack([s0["u"]] * 3)
    w = [s0["w"]] + [ms.scene_weights(64, 1, x0[a], u[a], seed=100 + a) for a in (1, 2)]
    return dict(refs=refs, x0=x0, u=u, w=w, model="diff", shape=(64, 1), per_agent=True, ingredients=s0)


def composed_iteration(sc, eps, T=50, K_=K):
    """one iteration in plan mode, composed: agent 0 prices its circles, tracks, grid and its mates' plans -> [(oracle, result)];
    kept(o) for agent 0 is mlp_scene_checks.kept"""
    P = learned_plans(sc["x0"], sc["u"], sc["w"])
    o = ComposedFleetOracle(ref_path=sc["refs"][0], num_samples_K=K_, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)), **mc.DIFF_KW)
    o.u_prev[:] = sc["u"][0]
    o.mlp_weights = sc["w"][0]
    ms.sk.aim(o, sc["ingredients"], 0, fp.mates_of(P, 0), fp.threshold2("diff"))
    res = o.iteration_general(sc["x0"][0], np.asarray(eps[0], np.float64), "frozen", True)
    res["w"] = o.compute_weight(np.asarray(res["S"], np.float64))
    rest = one_iteration(sc, eps, T, "frozen", True, "plan", K_=K_)
    return [(o, res)] + rest[1:]
