"""Fleet avoidance (mppi_config.fleet_radius): the f64 reference, the error model of a mate's centre and the scenes
of test_fleet_cases.py (CPU) and test_gpu_fleet.py.  No device import.

The reference: `mate_rows` restates the header's definition of a mate's circle; an agent's oracle is the moving-obstacle oracle
of tests/moving_obstacle_checks.py whose circles are the agent's own followed by its mates' rows.  That oracle tests a pose
reached after j steps against c + v dt (n + j) with ONE clock n per table, so a mate -- defined from "now" -- enters it back-
dated, c = p - v dt n, exactly as the library stores it."""
import numpy as np

import moving_obstacle_checks as mc
from oracle import mppi_oracle

EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
RADIUS = 0.4  # fleet_radius of the scenes: with the diff-drive margin of 0.8 the threshold radius is 0.5 * 0.8 + 0.4 = 0.8


# ------------------------------------------------------------------------------------------ the reference
def mate_rows(states, u_rows, model, cfg):
    """states [B, nx] (f64), u_rows [B, 2] (row 0 of every agent's nominal sequence), model "diff" | "race", cfg: fleet_radius
    and u_max0 -> (circles [B, B - 1, 3] = x, y, r; velocities [B, B - 1, 2]) in f64: agent b's mates a != b, ascending a."""
    x, u = np.asarray(states, np.float64), np.asarray(u_rows, np.float64)
    B = x.shape[0]
    s = x[:, 3] if model == "race" else np.clip(u[:, 0], -cfg["u_max0"], cfg["u_max0"])
    v = s[:, None] * np.stack([np.cos(x[:, 2]), np.sin(x[:, 2])], axis=1)
    c = np.concatenate([x[:, :2], np.full((B, 1), float(cfg["fleet_radius"]))], axis=1)
    mates = [[a for a in range(B) if a != b] for b in range(B)]
    return np.stack([c[m] for m in mates]), np.stack([v[m] for m in mates])


def table_of(own_c, own_v, mate_c, mate_v, dt, n):
    """Agent b's table as an oracle with clock n takes it: own rows (uploaded at clock 0) then the mates back-dated."""
    own_c, own_v = np.asarray(own_c, np.float64).reshape(-1, 3), np.asarray(own_v, np.float64).reshape(-1, 2)
    back = np.asarray(mate_c, np.float64).copy()
    back[:, :2] -= np.asarray(mate_v) * (dt * n)
    return np.concatenate([own_c, back]), np.concatenate([own_v, mate_v])


# ------------------------------------------------------------------------------------------ the error model
def centre_bound(p_abs, travel, eps):
    """Bound on |device centre - (p + v dt j)| of a mate, per coordinate, with p_abs >= |p| (the centre's coordinates), travel =
    |v| dt (n + j) and eps the spacing of the handle's precision R at 1 (a rounding to R errs by at most eps / 2 relative):
      p to R                                 eps/2 |p|
      v to R (delta_v) and dt to R           the stored row and the test use the same rounded v and dt, so both act on the
                                             difference v dt j only: eps/2 |v| dt j each, <= eps travel together
      the two products dt n and dt (n + j)   eps/2 |v| dt n + eps/2 |v| dt (n + j) <= eps travel
      the back-dating fma  c = p - v tau_n   eps/2 |c| <= eps/2 (|p| + travel)
      the test's fma  c + v tau_{n+j}        eps/2 |result| <= eps/2 (|p| + travel)
      f64 sincos on the device vs NumPy      <= 2 ulp of f64 each on cos and sin: 2^-51 travel (and as much on p for the
                                             f64 products that form v before the rounding)
    Sum: eps/2 (3 |p| + 6 travel) + 2^-50 (|p| + travel)."""
    return 0.5 * eps * (3.0 * p_abs + 6.0 * travel) + 2.0 ** -50 * (p_abs + travel)


def velocity_bound(v_abs, eps):
    """|device v - v| per coordinate: the rounding to R and the two f64 library roundings (sincos, the product)."""
    return 0.5 * eps * v_abs + 2.0 ** -50 * v_abs


def radius_bound(thr, eps):
    """The radius as mppi_get_agent_circles unpacks it: threshold^2 rounded to R (eps/2 relative: eps/4 on the root), the f64
    square, root and subtraction of the margin beside it."""
    return 0.25 * eps * thr + 2.0 ** -50 * (1.0 + thr)


def check_rows(got_c, got_v, want_c, want_v, dt, n, thr_of, precision):
    """Rows read back at step 0 of clock n against the reference, each held to the model; -> the largest error / bound."""
    eps = EPS[precision]
    got_c, got_v, want_c, want_v = (np.asarray(a, np.float64) for a in (got_c, got_v, want_c, want_v))
    assert got_c.shape == want_c.shape and got_v.shape == want_v.shape, (got_c.shape, want_c.shape)
    worst = 0.0
    for i in range(len(want_c)):
        speed = float(np.hypot(*want_v[i]))
        p_abs = float(np.abs(want_c[i, :2]).max())
        for err, bound in ((np.abs(got_c[i, :2] - want_c[i, :2]).max(), centre_bound(p_abs, speed * dt * n, eps)),
                           (np.abs(got_v[i] - want_v[i]).max(), velocity_bound(speed, eps)),
                           (abs(got_c[i, 2] - want_c[i, 2]), radius_bound(thr_of(want_c[i, 2]), eps))):
            assert err <= bound, (i, err, bound, got_c[i], want_c[i], got_v[i], want_v[i])
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


# ------------------------------------------------------------------------------------------ scenes
def line(p, q, n=100):
    return mppi_oracle.generate_point_trajectory(p, q, n)


def crossing_scene(T, accumulate, seed=0):
    """Three diff-drive robots on straight paths, nominal controls that cover mc.TRAVEL metres over the horizon:
      0  along +x from the origin;
      1  along +y, crossing 0's path: where 0's nominal rollout is at `meet` of the horizon (mid-horizon when every step is
         priced, step T when `S[k] =` prices the last state only), 1 is `gap` ahead of that point on 0's line -- the closest
         approach of the two nominal rollouts is about the threshold radius 0.8, so the samples fall on both sides of it;
      2  parallel to 0, 6 m to its left: out of reach of 0 over the horizon (1 comes within 3 m of its line at most).
    Own circles: none here (the tests add some).  -> dict(refs, x0 [3, 3], u [3, T, 2])"""
    rng = np.random.default_rng(300 + seed)
    dt = mc.DIFF_KW["delta_t"]
    speed = mc.TRAVEL / (T * dt)
    meet = round(0.5 * T) / T if accumulate else 1.0
    gap = 0.8 * np.sqrt(2.0) if accumulate else 0.8  # (perpendicular equal speeds close to gap / sqrt 2)
    M = np.array([meet * mc.TRAVEL + gap, 0.0])
    starts = [np.array([0.0, 0.0, 0.0]), np.array([M[0], M[1] - meet * mc.TRAVEL, 0.5 * np.pi]), np.array([0.0, 6.0, 0.0])]
    refs = [line((0.0, 0.0), (10.0, 0.0)), line((M[0], starts[1][1]), (M[0], starts[1][1] + 10.0)), line((0.0, 6.0), (10.0, 6.0))]
    x0 = np.stack([s + np.array([0.05, -0.03, 0.01]) * (a + 1) for a, s in enumerate(starts)])
    u = np.stack([np.stack([np.full(T, speed), np.zeros(T)], axis=1) + rng.normal(0, 0.01, (T, 2)) for _ in range(3)])
    return dict(refs=refs, x0=x0, u=u, model="diff")


def race_pair_scene(seed=0):
    """Two race cars meeting on the lemniscate of mc.race_scene: car 0 is that scene's car; car 1 comes down the road against
    it at the same speed, 3.7 m to its left (the outline's side points reach 2.25 m), and passes it at mid-horizon -- where
    the scene's `crosser` circle drives, with the radius RACE_RADIUS."""
    sc = mc.race_scene(seed)
    s = sc["x0"]
    h = np.array([np.cos(s[2]), np.sin(s[2])])
    nrm = np.array([-h[1], h[0]])
    horizon = mc.RACE_T * 0.05
    p1 = s[:2] + (s[3] * horizon) * h + 3.7 * nrm  # closing at 2 v: they pass after horizon / 2
    x0 = np.stack([s, np.array([p1[0], p1[1], s[2] + np.pi, s[3]])])
    u = np.stack([sc["u"], np.random.default_rng(210 + seed).normal(0, 0.05, sc["u"].shape)])
    return dict(refs=[sc["ref"], sc["ref"]], x0=x0, u=u, model="race")


RACE_RADIUS = 1.0


def far_scene(B, T, seed=0):
    """B diff-drive robots on parallel paths 1000 m apart: no mate is ever in reach."""
    rng = np.random.default_rng(400 + seed)
    speed = mc.TRAVEL / (T * mc.DIFF_KW["delta_t"])
    refs = [line((0.0, 1000.0 * a), (10.0, 1000.0 * a - 5.0)) for a in range(B)]
    x0 = np.stack([np.array([0.1, 1000.0 * a - 0.05, r[0, 2] + 0.02]) for a, r in enumerate(refs)])
    u = np.stack([np.stack([np.full(T, speed), np.zeros(T)], axis=1) + rng.normal(0, 0.01, (T, 2)) for _ in range(B)])
    return dict(refs=refs, x0=x0, u=u, model="diff")


def far_own(sc):
    """Own moving sets for the far-apart fleet: a circle whose threshold (0.8) reaches the point where the agent's nominal
    rollout ends when it ends (`S[k] =` prices the last state), drifting along the path meanwhile; every fourth agent none."""
    own = []
    T = sc["u"].shape[1]
    for a, x in enumerate(sc["x0"]):
        h = np.array([np.cos(x[2]), np.sin(x[2])])
        v = 0.3 * h
        end = x[:2] + mc.TRAVEL * h + 0.8 * np.array([-h[1], h[0]])
        own.append(NO_OWN if a % 4 == 3 else (np.array([[*(end - v * (mc.DIFF_KW["delta_t"] * T)), 0.4]]), v[None]))
    return own


def head_on_scene(T):
    """Behaviour: two diff-drive robots drive the same straight line from opposite ends, 4 m apart, at 1 m/s nominal."""
    ref0, ref1 = line((0.0, 0.0), (10.0, 0.0)), line((4.0, 0.0), (-6.0, 0.0))
    x0 = np.array([[0.0, 0.02, 0.0], [4.0, -0.02, np.pi]])
    u = np.tile(np.array([1.0, 0.0]), (2, T, 1))
    return dict(refs=[ref0, ref1], x0=x0, u=u, model="diff")


def contact_scene(T):
    """Clearance: the head-on pair 0.7 m apart -- the run starts in contact (2 r = 0.8) -- and a third robot 50 m away."""
    sc = head_on_scene(T)
    sc["x0"][1, 0] = 0.7
    return dict(refs=sc["refs"] + [line((0.0, 50.0), (10.0, 50.0))], x0=np.concatenate([sc["x0"], [[0.0, 50.0, 0.0]]]),
                u=np.concatenate([sc["u"], sc["u"][:1]]), model="diff")


def rows_cfg(model, radius=None):
    return dict(fleet_radius=(RACE_RADIUS if model == "race" else RADIUS) if radius is None else radius,
                u_max0=0.523 if model == "race" else mc.DIFF_KW["max_speed"])


def dt_of(model):
    return 0.05 if model == "race" else mc.DIFF_KW["delta_t"]


def thr_of(model):
    """radius -> threshold radius as set_circles packs it"""
    return (lambda r: r) if model == "race" else (lambda r: 0.5 * mc.DIFF_KW["safety_margin_rate"] + r)


# ------------------------------------------------------------------------------------------ per-agent oracles
def agent_oracle(sc, a, K, T, **kw):
    """Agent a's oracle, with no circles yet (see `aim`)."""
    if sc["model"] == "race":
        o = mc.MovingRaceCarOracle(ref_path=sc["refs"][a], number_of_samples_K=K, obstacle_circles=np.zeros((0, 3)), **mc.RACE_KW)
        o.u_prev[:] = sc["u"][a].astype(np.float32)
    else:
        o = mc.MovingDiffDriveOracle(ref_path=sc["refs"][a], num_samples_K=K, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)),
                                     **dict(mc.DIFF_KW, **kw))
        o.u_prev[:] = sc["u"][a]
    return o


def aim(o, own, mate_c, mate_v, dt, n, freeze_at=None):
    """Point oracle o at its own circles (c [m, 3], v [m, 2], uploaded at clock 0) and this iteration's mates, at clock n."""
    c, v = table_of(own[0], own[1], mate_c, mate_v, dt, n)
    if len(c) == 0:  # (the oracles' margin bookkeeping wants a circle: one that nothing reaches)
        c, v = np.array([[1.0e6, 1.0e6, 0.1]]), np.zeros((1, 2))
    o.obstacle_circles = c
    o.set_motion(v, n, freeze_at)


NO_OWN = (np.zeros((0, 3)), np.zeros((0, 2)))


def one_iteration(sc, eps, K, T, mode="frozen", accumulate=False, own=None, mates=True, freeze_at=None, n=0, **kw):
    """One iteration of every agent at clock n: eps [B, K, T, 2].  mates False: nobody sees anybody.
    -> list of (oracle, result) per agent"""
    B, model = len(sc["refs"]), sc["model"]
    mc_, mv_ = mate_rows(sc["x0"], sc["u"][:, 0], model, rows_cfg(model))
    out = []
    for a in range(B):
        o = agent_oracle(sc, a, K, T, **kw)
        aim(o, NO_OWN if own is None else own[a], mc_[a] if mates else mc_[a][:0], mv_[a] if mates else mv_[a][:0], dt_of(model), n, freeze_at)
        if model == "race":
            res = o.iteration(sc["x0"][a], eps[a])
        else:
            res = o.iteration_general(sc["x0"][a], np.asarray(eps[a], np.float64), mode, accumulate)
        out.append((o, res))
    return out


def closed_loop(sc, eps_of, n_iters, K, T, own=None, mates=True, mode="frozen", accumulate=False, **kw):
    """The batched closed loop: per iteration the mates' rows from the states and nominal controls as they stand, one
    iteration per agent, the plant, one tick.  eps_of(i) -> [B, K, T, 2].  -> dict(x [n + 1, B, 3] the states every iteration
    starts from and the last one, u_start [n, B, T, 2] the nominal controls it starts from, u [B, T, 2] the last ones, n_hit
    [n, B], kept [n, B, K] the samples an f32 comparison keeps, S [n, B, K])"""
    B = len(sc["refs"])
    dt = dt_of(sc["model"])
    os_ = [agent_oracle(sc, a, K, T, **kw) for a in range(B)]
    x = sc["x0"].copy()
    xs, hits, keep, Ss, us = [x.copy()], [], [], [], []
    for i in range(n_iters):
        mc_, mv_ = mate_rows(x, np.stack([o.u_prev[0] for o in os_]), sc["model"], rows_cfg(sc["model"]))
        eps = eps_of(i)
        us.append(np.stack([o.u_prev.copy() for o in os_]))
        nx, row_h, row_k, row_S = [], [], [], []
        for a, o in enumerate(os_):
            aim(o, NO_OWN if own is None else own[a], mc_[a] if mates else mc_[a][:0], mv_[a] if mates else mv_[a][:0], dt, i)
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


def min_mate_distance(x):
    """x [B, nx] -> [B] smallest centre distance of every agent to any mate"""
    d = np.sqrt((x[:, None, 0] - x[None, :, 0]) ** 2 + (x[:, None, 1] - x[None, :, 1]) ** 2)
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)


# one-iteration cases of test_gpu_fleet.py group 3: (T, accumulate, mode)
def diff_cases():
    out = [(T, acc, "frozen") for T in (7, 50, 65, 128) for acc in (False, True)]
    return out + [(50, acc, "per_rollout") for acc in (False, True)]


def numpy_noise(sigma, seed, it, B, K, T, noise_stream=0):
    """oracle/philox.py with the fourth counter word noise_stream + a: [B, K, T, 2] float32"""
    from oracle import philox
    return np.stack([philox.sample_epsilon(np.asarray(sigma, np.float64).reshape(2, 2), seed, it, K, T, stream=noise_stream + a) for a in range(B)])
