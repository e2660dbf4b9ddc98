"""Composed scenes (mppi_set_scene_mode): the f64 reference and the scenes of test_scene_cases.py (CPU) and
test_gpu_scene.py.  No device import.

Nothing new is computed here.  The reference is the grid oracles of tests/cost_grid_checks.py -- the penalty and weight g
wherever a state is priced -- whose circle test `_test` also takes, at the step of the call, the track centres of
obstacle_track_checks.track_centres and one centre per mate from the plans of fleet_plan_checks.plans (aimed by
fleet_plan_checks.aim, threshold fleet_plan_checks.threshold2): a state is hit when the circles, the tracks, the mates or the
grid say so.  `_test` also keeps, per ingredient, which samples it hit, so that the CPU tests can show that each one decides
samples the others spare.  MARGIN, MAX_LEFT_OUT, K_CASE and f32_tolerance are the project's (moving_obstacle_checks.py,
cost_grid_checks.py)."""
import numpy as np

import cost_grid_checks as gc
import fleet_checks as fc
import fleet_plan_checks as pc
import moving_obstacle_checks as mc
import obstacle_track_checks as ot
from cost_grid_checks import f32_tolerance  # noqa: F401  (the tests' names)
from moving_obstacle_checks import K_CASE, MARGIN, MAX_LEFT_OUT, kept, penalised  # noqa: F401
from oracle.mppi_oracle import F32

INGREDIENTS = ("grid", "tracks", "plans")


# ------------------------------------------------------------------------------------------ the staging function, restated
def scene_lds_bytes(elem, n_plan_agents, n_max, T):
    """mppi_scene_lds_bytes (csrc/mppi_scene_staging.h) by its definition -> (plans, tracks, track offset, total) in bytes"""
    budget = 40000 if elem == 4 else 16384
    pb, tb = n_plan_agents * (T + 1) * 2 * elem, n_max * ((T + 1) * 2 + 1) * elem
    plans = pb if 0 < pb <= budget else 0
    off = (plans + 15) & ~15
    tracks = tb if tb > 0 and off + tb <= budget else 0
    return plans, tracks, off, (off + tracks if tracks else plans)


# ------------------------------------------------------------------------------------------ the reference
class _SceneTest(ot._Tracks):
    """The circle test of the moving oracles with the tracks and the mates beside the circles."""
    tracks, track_radii, track_clock, track_variant = np.zeros((0, 1, 2)), np.zeros(0), 0, "tracks"
    mate_plans, plan_thr2 = None, None

    def reset_parts(self):
        self.part_hits = {"circles": [], "tracks": [], "plans": []}

    def _test(self, px, py, r2, steps):
        hit = np.zeros(px.shape[:-1], bool)
        margin = np.full(px.shape[:-1], np.inf)
        K = px.shape[0]

        def against(name, c, thr2):
            nonlocal hit, margin
            d2 = (px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2
            h = (d2 < thr2).any(axis=(-1, -2))
            hit = hit | h
            margin = np.minimum(margin, (np.abs(d2 - thr2) / thr2).min(axis=(-1, -2)))
            self.part_hits[name].append(h.reshape(K, -1))
        if len(self.obstacle_circles):
            against("circles", mc.centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps),
                    np.broadcast_to(r2, (len(self.obstacle_circles),)))
        if len(self.track_radii):
            against("tracks", ot.track_centres(self.tracks, self.track_clock, steps, self.track_variant), self._track_r2())
        if self.mate_plans is not None and len(self.mate_plans):
            against("plans", np.moveaxis(self.mate_plans[:, np.asarray(steps), :], 0, -2), np.full(len(self.mate_plans), self.plan_thr2))
        self.margins.append(margin.reshape(K, -1))
        return hit

    def sample_hit(self, name):
        """per sample: ingredient `name` ("circles", "tracks", "plans", "grid") hit one of the states priced"""
        if name == "grid":
            return self.sample_grid_lethal() if self.grid is not None else np.zeros(self.K, bool)
        rows = self.part_hits[name]
        return np.concatenate(rows, axis=1).any(axis=1) if rows else np.zeros(self.K, bool)


class SceneDiffDriveOracle(_SceneTest, gc.GridDiffDriveOracle):
    def _track_r2(self):  # (as a circle of that radius: obstacle_track_checks.TrackDiffDriveOracle)
        return (0.5 * self.safety_margin_rate + self.track_radii) ** 2


class SceneRaceCarOracle(_SceneTest, gc.GridRaceCarOracle):
    def _track_r2(self):
        return self.track_radii ** 2


def aim(o, ing, clock=0, mate_plans=None, thr2=None):
    """Point oracle o at one agent's ingredients `ing` = dict(circles, vel, tracks, radii, grid; absent or None: the agent lacks
    it) at `clock` control steps after everything was uploaded, and at its mates' plans [m, T + 1, 2] (None: no plan mode)."""
    own = (ing.get("circles", np.zeros((0, 3))), ing.get("vel", np.zeros((0, 2))))
    pc.aim(o, own, np.zeros((0, 1, 2)) if mate_plans is None else mate_plans, thr2, clock)
    trk, radii = (ing["tracks"], ing["radii"]) if ing.get("tracks") is not None else (None, np.zeros(0))
    o.set_tracks(trk, radii, clock)
    o.set_grid(ing.get("grid"))
    o.reset_parts()
    return o


# ------------------------------------------------------------------------------------------ scenes
def heading(x0):
    h = np.array([np.cos(x0[2]), np.sin(x0[2])])
    return h, np.array([-h[1], h[0]])


def moved(points, frm, to):
    """points [..., 2] given beside a robot at pose `frm`, carried over rigidly to stand the same way beside pose `to`"""
    (h0, n0), (h1, n1) = heading(frm), heading(to)
    d = np.asarray(points, np.float64) - frm[:2]
    return to[:2] + (d @ h0)[..., None] * h1 + (d @ n0)[..., None] * n1


# The tracks of obstacle_track_checks.diff_scene, moved to the open side of the nominal rollout -- the wall of
# cost_grid_checks.diff_scene stands 0.55 m to its right and 0.3 m beyond its end: the turner's bend keeps its side (left), the
# stopper is mirrored to the left, and both are set TRACK_BACK m back along the path and TRACK_OUT m out (negative: in).
# Threshold radius 0.8 as there.  The two figures come from a scan on the CPU reference alone (0, 0.15 back x -0.1 .. 0.2 out)
# for the placement that leaves the grid and the tracks each the most samples of their own over single_cases():
# at (0.15, -0.03) the grid alone decides >= 47 of 256 samples, the tracks alone >= 23, and >= 23 stay unpenalised.
TRACK_BACK, TRACK_OUT = 0.15, -0.03
TRACK_RADIUS = 0.4


def small_grid(x0, radius=0.6, weight=4.0, lethal=0.5):
    """The wall on 33 x 17 nodes of 0.25 m over the end of the nominal rollout, at another weight"""
    h, _ = heading(x0)
    origin = tuple(np.floor(x0[:2] + mc.TRAVEL * h) - (4.0, 2.0))
    cells = gc.wall_cells(*gc.diff_wall(dict(x0=x0)), radius, origin, 0.25, 33, 17)
    return gc.Grid(cells, origin, 0.25, weight, lethal)


def diff_ingredients(x0, T, accumulate, clock=0, extra=0, grid="64x64", circles=2, what=INGREDIENTS, back=None, out_=None, wall_ahead=0.0):
    """One diff-drive agent's grid, tracks and own circles beside its nominal rollout from x0 (TRAVEL metres along its heading):
    cost_grid_checks.diff_scene's wall and circles and obstacle_track_checks.diff_scene's turner and stopper, carried over to x0.
    grid: "64x64" (origin floor(x0) - (2, 5): the case grid), "33x17" (small_grid).  extra < 0: the tracks run out inside the
    horizon (L = clock + T + 1 + extra).  what: the ingredients the agent has."""
    base = mc.diff_scene(T, accumulate)
    b0 = base["x0"]
    h, nrm = heading(x0)
    out = dict(circles=np.zeros((0, 3)), vel=np.zeros((0, 2)), tracks=None, radii=None, grid=None)
    if circles:
        g = gc.diff_scene(T, accumulate, circles=circles)
        (hb, nb) = heading(b0)
        c = g["circles"].copy()
        c[:, :2] = moved(c[:, :2], b0, x0)
        v = (g["vel"] @ hb)[:, None] * h + (g["vel"] @ nb)[:, None] * nrm
        out.update(circles=c, vel=v)
    if "grid" in what:
        xw = np.concatenate([x0[:2] + wall_ahead * h, x0[2:]])  # (the pose the wall stands beside: wall_ahead m further on)
        if grid == "33x17":
            out["grid"] = small_grid(xw)
        else:
            nx, ny, res = gc.DIFF_GRIDS[grid]
            origin = tuple(np.floor(x0[:2]) + gc.DIFF_ORIGIN)
            out["grid"] = gc.Grid(gc.wall_cells(*gc.diff_wall(dict(x0=xw)), gc.DIFF_RADIUS, origin, res, nx, ny), origin, res,
                                  gc.DIFF_WEIGHT, gc.DIFF_LETHAL)
    if "tracks" in what:
        t = ot.diff_scene(T, accumulate, clock, extra)["tracks"][:2].copy()
        hb, nb = heading(b0)
        lat = (t[1] - b0[:2]) @ nb
        t[1] = t[1] - 2.0 * lat[:, None] * nb  # the stopper mirrored to the left of the path
        t = t - (TRACK_BACK if back is None else back) * hb + (TRACK_OUT if out_ is None else out_) * nb
        out.update(tracks=moved(t, b0, x0), radii=np.full(2, TRACK_RADIUS))
    return out


def diff_oracle(ref, u, K, T, **kw):
    o = SceneDiffDriveOracle(ref_path=ref, num_samples_K=K, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)), **dict(mc.DIFF_KW, **kw))
    o.u_prev[:] = u
    return o


def race_oracle(ref, u, K):
    o = SceneRaceCarOracle(ref_path=ref, number_of_samples_K=K, obstacle_circles=np.zeros((0, 3)), **mc.RACE_KW)
    o.u_prev[:] = np.asarray(u).astype(F32)
    return o


# ---- one agent: grid + tracks ----
def diff_scene(T, accumulate, clock=0, extra=0, grid="64x64"):
    """cost_grid_checks.diff_scene (path, state, controls, two circles, the wall) with the two tracks"""
    sc = mc.diff_scene(T, accumulate)
    return dict(ref=sc["ref"], x0=sc["x0"], u=sc["u"], clock=clock, **diff_ingredients(sc["x0"], T, accumulate, clock, extra, grid))


def single_cases():
    """(T, accumulate, mode, clock, extra, grid): every horizon with the frozen index and both sums, the track clocks 0 and 3
    alternating; the threaded indices at T = 50 and 65; tracks that run out inside the horizon at both clocks; the small grid"""
    out = [(T, acc, "frozen", 3 if (i + acc) % 2 else 0, 0, "64x64") for i, T in enumerate(gc.HORIZONS) for acc in (False, True)]
    out += [(T, False, mode, 3, 0, "64x64") for T in (50, 65) for mode in ("per_rollout", "sequential")]
    out += [(50, True, "frozen", 0, -20, "64x64"), (65, True, "frozen", 3, -30, "33x17")]
    return out


# noise seeds: for each case the first seed at which the f64 reference itself leaves out at most MAX_LEFT_OUT of the samples
# (test_scene_cases.py asserts it); cases not listed take seed 0
EPS_SEED = {(65, True, 'frozen', 0, 0, '64x64'): 2, (128, True, 'frozen', 3, 0, '64x64'): 3, (65, True, 'frozen', 3, -30, '33x17'): 2}


def eps_seed(*case):
    return EPS_SEED.get(tuple(case), 0)


def single_case(T, accumulate, mode, clock=0, extra=0, grid="64x64", K=K_CASE):
    """-> (scene, eps [K, T, 2] float32, oracle after one iteration at `clock`, its result)"""
    from oracle import philox
    sc = diff_scene(T, accumulate, clock, extra, grid)
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], eps_seed(T, accumulate, mode, clock, extra, grid), 0, K, T)
    o = aim(diff_oracle(sc["ref"], sc["u"], K, T), sc, clock)
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    return sc, eps, o, res


def race_scene(clock=0):
    """cost_grid_checks.race_scene (two circles, the wall) with one track: obstacle_track_checks.race_scene's crosser"""
    sc = gc.race_scene()
    t = ot.race_scene(clock)
    _, nrm = heading(sc["x0"])
    return dict(sc, clock=clock, tracks=t["tracks"][:1] + RACE_TRACK_OUT * nrm, radii=t["radii"][:1])


def race_case(clock=0, K=K_CASE, seed=0):
    from oracle import philox
    sc = race_scene(clock)
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), seed, 0, K, mc.RACE_T)
    o = aim(race_oracle(sc["ref"], sc["u"], K), sc, clock)
    res = o.iteration(sc["x0"], eps)
    return sc, eps, o, res


# ---- batches: the arc fleet ----
# what every agent has in the batch cases: agent 0 everything the case has, agent 1 lacks the tracks (and takes the small grid),
# agent 2 lacks the grid
FLEET_HAS = (("grid", "tracks"), ("grid",), ("tracks",))
FLEET_GRID = ("64x64", "33x17", "64x64")
# Where the batch cases put things, so that agent 0's samples split three ways by how far they get (their last states differ
# along the path by 0.2 - 0.4 m and hardly across it): agent 0 starts FLEET_AHEAD m further on and FLEET_RIGHT m to the right
# of arc_scene's, so that agent 1 ends beside its nominal end, 0.8 m off, and takes the samples in the middle; the tracks
# stand FLEET_BACK m back and take the short ones; the wall stands FLEET_WALL m further on and takes the long ones.  From a
# scan on the CPU reference alone (0.5 - 0.7 x 0.15, 0.22 x 0.8, 0.95 x 0.2, 0.28): the placement whose smallest share is largest.
FLEET_AHEAD, FLEET_RIGHT, FLEET_BACK, FLEET_OUT, FLEET_WALL = 0.5, 0.22, 0.8, -0.3, 0.28
# the race car's track: obstacle_track_checks.race_scene's crosser where it is for the single car (the grid alone then decides
# 95 of 256 samples, the track alone 21); for car 0 of the pair 0.78 m nearer the road and 5.5 m earlier along it, the placement
# of a scan on the CPU reference (-2 .. 0.5 x -6 .. 4) at which the wall, the track and the mate's plan each decide a sixteenth
# of the samples alone (21, 16 and 49)
RACE_TRACK_OUT = 0.0
RACE_FLEET_TRACK = (-0.78, -5.5)


def fleet_scene(T, accumulate, what=INGREDIENTS, clock=0, extra=0, n_tracks=None):
    """fleet_plan_checks.arc_scene (three robots; the arc of agent 1 meets agent 0's nominal rollout) with, per agent, the
    ingredients of FLEET_HAS that `what` names, beside its own nominal rollout.  n_tracks: agent 0's set padded with
    obstacle_track_checks.far_tracks to that many (the LDS cases)."""
    sc = pc.arc_scene(T, accumulate)
    away = np.array([FLEET_AHEAD, -FLEET_RIGHT])  # (agent 1 meets agent 0's nominal rollout 0.565 m ahead and as far to its left: arc_scene)
    x0 = sc["x0"].copy()
    x0[0, :2] += away
    refs = [sc["refs"][0] + np.concatenate([away, np.zeros(sc["refs"][0].shape[1] - 2)])] + list(sc["refs"][1:])
    sc = dict(sc, x0=x0, refs=refs)
    per = []
    for a in range(3):
        has = tuple(w for w in FLEET_HAS[a] if w in what)
        ing = diff_ingredients(sc["x0"][a], T, accumulate, clock, extra, FLEET_GRID[a], circles=2 if a == 0 else 0, what=has,
                               back=FLEET_BACK, out_=FLEET_OUT, wall_ahead=FLEET_WALL if a == 0 else 0.0)
        if a == 0 and n_tracks and ing["tracks"] is not None:
            L = ing["tracks"].shape[1]
            ing["tracks"] = np.concatenate([ing["tracks"], ot.far_tracks(n_tracks - 2, L)])
            ing["radii"] = np.concatenate([ing["radii"], np.full(n_tracks - 2, 0.3)])
        per.append(ing)
    return dict(sc, per=per, plans="plans" in what, clock=clock)


def fleet_cases():
    """(T, accumulate, mode, what, clock, extra), all with `S[k] =` (the last state is priced): all three at the horizons of
    either chunk count, at clock 3 with tracks that run out, and with the per-rollout index; the pairs a batch can hold with
    the plans, and grid + tracks without them.  (With every step priced the arc of agent 1 crosses agent 0's lane in the second
    half of the horizon and takes 240 of its 256 samples wherever the others stand: no placement leaves the grid and the tracks
    a sixteenth each.  The accumulating sum is covered by single_cases() and the race car.  T = 7: the samples' last states lie
    within 0.1 m of each other, too close to split three ways; single_cases() has it.)"""
    all3 = INGREDIENTS
    out = [(T, False, "frozen", all3, 0, 0) for T in (50, 65, 128)]
    out += [(64, False, "frozen", all3, 3, -20), (50, False, "per_rollout", all3, 0, 0), (65, False, "per_rollout", all3, 3, 0)]
    out += [(50, False, "frozen", pair, 0, 0) for pair in (("grid", "plans"), ("tracks", "plans"), ("grid", "tracks"))]
    out += [(65, False, "frozen", pair, 3, 0) for pair in (("grid", "plans"), ("tracks", "plans"))]
    return out


# noise seeds (mppi_config.seed) as fleet_plan_checks.EPS_SEED: the first seed from 99 on at which the f64 reference leaves out
# at most MAX_LEFT_OUT of every agent's samples (test_scene_cases.py asserts it); cases not listed take 99
FLEET_SEED = {}  # (99 serves every case)
RACE_FLEET_SEED = 99


def fleet_seed(*case):
    return FLEET_SEED.get(tuple(case), 99)


def fleet_iteration(sc, eps, K, T, mode="frozen", accumulate=False, **kw):
    """One iteration of every agent of a fleet_scene at its clock: eps [B, K, T, 2] -> list of (oracle, result) per agent.  The
    mates stand where their plans put them (plan mode) or nowhere (`sc["plans"]` false: a batch without a fleet)."""
    P = pc.plans(sc["x0"], sc["u"], "diff", pc.plan_cfg("diff"))
    out = []
    for a in range(len(sc["refs"])):
        o = diff_oracle(sc["refs"][a], sc["u"][a], K, T, **kw)
        aim(o, sc["per"][a], sc["clock"], pc.mates_of(P, a) if sc["plans"] else None, pc.threshold2("diff"))
        out.append((o, o.iteration_general(sc["x0"][a], np.asarray(eps[a], np.float64), mode, accumulate)))
    return out


def fleet_noise(seed, iteration, K, T, B=3, model="diff"):
    """what the device's sampler draws (fleet_checks.numpy_noise, held to it within 4e-6 by test_gpu_fleet.device_noise)"""
    sigma = np.array([[0.5, 0.0], [0.0, 0.1]]) if model == "race" else mc.DIFF_KW["sigma"]
    return fc.numpy_noise(sigma, seed, iteration, B, K, T, 0)


def race_fleet_scene():
    """fleet_plan_checks.race_curve_scene (two cars) with, for car 0, cost_grid_checks.race_scene's wall carried over to its
    pose and one track of obstacle_track_checks.race_scene; car 1 has neither"""
    sc = pc.race_curve_scene()
    x0 = sc["x0"][0]
    h, nrm = heading(x0)
    corner = x0[:2] + 11.5 * h - 2.5 * nrm
    origin = tuple(np.floor(x0[:2] + 5.0 * h) - 16.0)
    cells = gc.wall_cells(corner, x0[:2] - 4.0 * h - 2.5 * nrm, corner + 8.0 * nrm, gc.RACE_RADIUS, origin, gc.RACE_RES, 64, 64)
    base = ot.race_scene(0)
    trk = moved(base["tracks"][:1], base["x0"], x0) + RACE_FLEET_TRACK[0] * nrm + RACE_FLEET_TRACK[1] * h
    car0 = dict(grid=gc.Grid(cells, origin, gc.RACE_RES, gc.RACE_WEIGHT, gc.RACE_LETHAL), tracks=trk, radii=base["radii"][:1])
    return dict(sc, per=[car0, dict()], plans=True, clock=0)


def race_fleet_iteration(sc, eps, K):
    P = pc.plans(sc["x0"], sc["u"], "race", pc.plan_cfg("race"))
    out = []
    for a in range(2):
        o = aim(race_oracle(sc["refs"][a], sc["u"][a], K), sc["per"][a], 0, pc.mates_of(P, a), pc.threshold2("race"))
        out.append((o, o.iteration(sc["x0"][a], eps[a])))
    return out


# ------------------------------------------------------------------------------------------ what the CPU tests ask of a case
def exclusive_hits(o, names):
    """per ingredient of `names`: the samples it alone penalises -- no other ingredient and no circle hit them"""
    hit = {n: o.sample_hit(n) for n in ("circles",) + INGREDIENTS}
    return {n: hit[n] & ~np.any([hit[m] for m in hit if m != n], axis=0) for n in names}


# ------------------------------------------------------------------------------------------ the closed loop
LOOP_T, LOOP_N, LOOP_SWAP = 20, 6, 3


def loop_scene():
    """all three, the tracks two points short of the loop (L = T + 3: the hold is priced in its last iterations)"""
    return fleet_scene(LOOP_T, True, INGREDIENTS, clock=0, extra=2)


def shifted(grid):
    """the wall shifted by one cell (the same shape: the rolling-costmap re-upload)"""
    return None if grid is None else gc.Grid(np.roll(grid.cells, 1, axis=1), grid.origin, grid.resolution, grid.weight, grid.lethal)


def closed_loop(sc, eps_of, n_iters, K, T, swap_at, accumulate=True, **kw):
    """fleet_plan_checks.closed_loop with every agent's grid and tracks: per iteration the plans from the states and nominal
    controls as they stand, one iteration per agent at clock i, the plant, one tick; from iteration `swap_at` on every grid is
    `shifted`.  -> as fleet_plan_checks.closed_loop, and min_dist [B]: the clearance record as mppi_get_fleet_clearance keeps it"""
    from oracle import mppi_oracle
    B = len(sc["refs"])
    dt = fc.dt_of("diff")
    os_ = [diff_oracle(sc["refs"][a], sc["u"][a], K, T, **kw) for a in range(B)]
    x = sc["x0"].copy()
    xs, hits, keep, Ss, us = [x.copy()], [], [], [], []
    min_dist = np.full(B, np.inf)
    for i in range(n_iters):
        u_now = np.stack([o.u_prev.copy() for o in os_])
        P = pc.plans(x, u_now, "diff", pc.plan_cfg("diff"))
        d = np.linalg.norm(x[:, None, :2] - x[None, :, :2], axis=-1) + np.diag(np.full(B, np.inf))
        min_dist = np.minimum(min_dist, d.min(axis=1))
        eps = eps_of(i)
        us.append(u_now)
        nx, row_h, row_k, row_S = [], [], [], []
        for a, o in enumerate(os_):
            ing = dict(sc["per"][a], grid=shifted(sc["per"][a]["grid"]) if i >= swap_at else sc["per"][a]["grid"])
            aim(o, ing, i, pc.mates_of(P, a), pc.threshold2("diff"))
            res = o.iteration_general(x[a], np.asarray(eps[a], np.float64), "frozen", accumulate)
            row_h.append(int((np.asarray(res["S"]) >= 1.0e10).sum()))
            row_k.append(o.sample_margin() > MARGIN)
            row_S.append(np.asarray(res["S"], np.float64))
            nx.append(mppi_oracle.diffdrive_plant_step(x[a], res["u0_returned"], dt))
        x = np.stack(nx)
        xs.append(x.copy())
        hits.append(row_h)
        keep.append(row_k)
        Ss.append(row_S)
    return dict(x=np.array(xs), u=np.stack([o.u_prev.copy() for o in os_]), u_start=np.array(us), n_hit=np.array(hits),
                kept=np.array(keep), S=np.array(Ss), min_dist=min_dist)
