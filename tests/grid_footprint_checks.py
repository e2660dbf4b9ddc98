"""Cost grids under the vehicle's outline (mppi_set_cost_grid_footprint): the f64 reference and the scenes of
test_grid_footprint_cases.py (CPU) and test_gpu_grid_footprint.py.  No device import.

The reference is the oracles of cost_grid_checks.py with `_grid_at` taking the largest of nine values: the grid at the centre and
at the eight outline points of the pose, formed as MovingRaceCarOracle.collided forms them (F32(a) c - F32(b) s + x in the
arithmetic of the oracle's states: f32 for the race car, f64 for the diff-drive box).  Every scene keeps the half-sides a, b
exactly representable in f32, so one reference serves both precisions.  Beside the margin |g_foot - lethal| / lethal it records
the centre's value per priced state.

The diff-drive reference is the OUTLINE model with a grid and NO circles: the diff-drive oracle has the disc test only, so the
box scenes here carry no circles (the race car's do)."""
import numpy as np

import cost_grid_checks as gc
import moving_obstacle_checks as mc
from cost_grid_checks import MARGIN, MAX_LEFT_OUT, K_CASE, PENALTY, Grid, f32_tolerance, penalised, kept  # noqa: F401
from oracle import mppi_oracle
from oracle.mppi_oracle import F32


def outline(a, b):
    """the nine body-frame points: the centre, then the outline in the order of KParams::shape_x / shape_y[0..7]"""
    return np.array([(0, 0), (-a, 0), (-a, b), (0, b), (a, b), (a, 0), (a, -b), (0, -b), (-a, -b)], np.float64)


def world_points(x, y, yaw, a, b):
    """[..., 9, 2]: the points of the poses in the world, in the dtype of the poses"""
    x, y, yaw = np.asarray(x), np.asarray(y), np.asarray(yaw)
    c, s = np.cos(yaw), np.sin(yaw)
    q = outline(float(np.float32(a)), float(np.float32(b))).astype(x.dtype)
    px = np.stack([qa * c - qb * s + x for qa, qb in q], axis=-1)
    py = np.stack([qa * s + qb * c + y for qa, qb in q], axis=-1)
    px[..., 0], py[..., 0] = x, y  # (the centre is the pose's own position)
    return np.stack([px, py], axis=-1)


def footprint_value(grid, x, y, yaw, a, b):
    """g_foot and the centre's g at the poses, in f64 on the points as world_points forms them"""
    p = world_points(x, y, yaw, a, b).astype(np.float64)
    g = grid.value(p[..., 0], p[..., 1])
    return g.max(axis=-1), g[..., 0]


class _Footprint:
    """What both oracles share: the half-sides, the yaw of the states being priced, the centre's value per priced state, and
    `shift_yaw` -- every rollout yaw moved by that many f32 ulps (`shift` of cost_grid_checks.py moves the positions)."""
    shift_yaw = 0
    _yaw = None

    def set_grid(self, grid):
        super().set_grid(grid)
        self.centre_lethal, self.centre_term = [], []

    def half_sides(self):
        raise NotImplementedError

    def _grid_at(self, x, y):
        K = np.shape(x)[0]
        yaw = np.asarray(self._yaw_of(np.shape(x)))
        a, b = self.half_sides()
        dt = np.float32 if yaw.dtype == np.float32 else np.float64
        g, g0 = footprint_value(self.grid, np.asarray(x, dt), np.asarray(y, dt), yaw.astype(dt), a, b)
        if np.isfinite(self.grid.lethal):
            self.margins.append((np.abs(g - self.grid.lethal) / self.grid.lethal).reshape(K, -1))
        self.grid_lethal.append((g >= self.grid.lethal).reshape(K, -1))
        self.grid_term.append((self.grid.weight * g).reshape(K, -1))
        self.centre_lethal.append((g0 >= self.grid.lethal).reshape(K, -1))
        self.centre_term.append((self.grid.weight * g0).reshape(K, -1))
        return g

    def rollout(self, x0, v):
        X = super().rollout(x0, v)
        if self.shift_yaw:
            X = X.copy()
            X[..., 2] += self.shift_yaw * np.spacing(np.abs(X[..., 2]).astype(np.float32)).astype(X.dtype)
        self._X = X
        return X

    def sample_centre_lethal(self):
        return np.concatenate(self.centre_lethal, axis=1).any(axis=1)

    def sample_extra_term(self):
        """sum over the priced states of weight (g_foot - g_centre), per sample"""
        return self.sample_grid_term() - np.concatenate(self.centre_term, axis=1).sum(axis=1)


class _DiffBox(_Footprint):
    """The diff-drive box: vehicle_l x vehicle_w times the safety margin; the yaw of the states a `collided` call means comes
    from the rollout (the diff-drive oracles hand over positions only), or from `is_hit`'s argument."""
    vehicle_l, vehicle_w = 0.75, 0.5

    def half_sides(self):
        return 0.5 * self.vehicle_l * self.safety_margin_rate, 0.5 * self.vehicle_w * self.safety_margin_rate

    def _yaw_of(self, shape):
        if self._yaw is not None:
            return self._yaw
        return self._X[..., 2] if len(shape) == 2 else self._X[:, -1, 2]  # [K, T] stage states / [K] last states


class _RaceBox(_Footprint):
    def half_sides(self):
        return (0.5 * self.vehicle_l * self.collision_safety_margin_rate, 0.5 * self.vehicle_w * self.collision_safety_margin_rate)

    def _yaw_of(self, shape):
        return self._yaw

    def collided(self, x, y, yaw, steps=None):
        self._yaw = yaw
        return super().collided(x, y, yaw, steps)


class FootDiffDriveOracle(_DiffBox, gc.GridDiffDriveOracle):
    """no circles: the diff-drive oracle has the disc test only"""

    def is_hit(self, x, y, yaw, steps=None):
        self._yaw = np.asarray(yaw, np.float64)
        try:
            return super().is_hit(x, y, steps)
        finally:
            self._yaw = None


class FootRaceCarOracle(_RaceBox, gc.GridRaceCarOracle):
    pass


# ---- composed scenes: the oracles of scene_checks.py -- tracks and the mates' plans beside the circles -- with
# the footprint grid.  The box tests its eight outline points against circles, tracks and mates as the race car does (the
# thresholds of the outline model: the radius itself), which the diff-drive oracles of the other files do not.
def scene_race_oracle(ref, u, K):
    import scene_checks as sk

    class FootSceneRaceCarOracle(_RaceBox, sk.SceneRaceCarOracle):
        pass
    o = FootSceneRaceCarOracle(ref_path=ref, number_of_samples_K=K, obstacle_circles=np.zeros((0, 3)), **mc.RACE_KW)
    o.u_prev[:] = np.asarray(u).astype(F32)
    return o


def scene_diff_oracle(ref, u, K, T, **kw):
    import scene_checks as sk

    class FootSceneDiffDriveOracle(_DiffBox, sk.SceneDiffDriveOracle):
        def _track_r2(self):
            return self.track_radii ** 2

        def collided(self, x, y, steps=None):
            """GridDiffDriveOracle.collided with the outline's eight points in the circle test"""
            x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
            a, b = self.half_sides()
            p = world_points(x, y, np.asarray(self._yaw_of(x.shape), np.float64), a, b)[..., 1:, :]
            hit = self._test(p[..., 0], p[..., 1], self.obstacle_circles[:, 2] ** 2, self._steps_of(x.shape, steps))
            K = x.shape[0]
            self.circle_hit.append(hit.reshape(K, -1))
            if self.grid is None:
                return hit.astype(np.float64)
            g = self._grid_at(x, y)
            return (hit | (g >= self.grid.lethal)).astype(np.float64) + self.grid.weight * g / PENALTY
    o = FootSceneDiffDriveOracle(ref_path=ref, num_samples_K=K, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)),
                                 **dict(mc.DIFF_KW, safety_margin_rate=DIFF_BOX["safety_margin"], **kw))
    o.u_prev[:] = u
    return o


# ------------------------------------------------------------------------------------------ scenes
RACE_WEIGHT, RACE_LETHAL, RACE_RADIUS, RACE_RES = 128.0, 0.5, 3.0, 0.5
RACE_A, RACE_B = 3.0, 2.25  # 0.5 * 4 * 1.5, 0.5 * 3 * 1.5


def race_scene(circles=2):
    """race_scene of cost_grid_checks.py with the wall further out: 5.5 m to the right of the road, turning across it 15 m
    ahead, inflated by 3 m, on the 64 x 64 grid of 0.5 m cells (lethal 0.5, weight 128).  The centre of a car on the road stays
    4 m clear of the lethal contour; its right side, 2.25 m out, and its front, 3 m ahead, do not."""
    sc = mc.race_scene()
    s = sc["x0"]
    h = np.array([np.cos(s[2]), np.sin(s[2])])
    nrm = np.array([-h[1], h[0]])
    corner = s[:2] + 15.0 * h - 5.5 * nrm
    origin = tuple(np.floor(s[:2] + 5.0 * h) - 16.0)
    cells = gc.wall_cells(corner, s[:2] - 8.0 * h - 5.5 * nrm, corner + 12.0 * nrm, RACE_RADIUS, origin, RACE_RES, 64, 64)
    c = sc["circles"][:circles].copy()
    c[:, 2] = gc.RACE_CIRCLE_R
    return dict(sc, circles=c, vel=sc["vel"][:circles], grid=Grid(cells, origin, RACE_RES, RACE_WEIGHT, RACE_LETHAL))


def race_oracle(sc, K):
    o = FootRaceCarOracle(ref_path=sc["ref"], number_of_samples_K=K, obstacle_circles=sc["circles"],
                          obstacle_velocities=sc["vel"], **mc.RACE_KW)
    o.u_prev[:] = sc["u"].astype(F32)
    o.set_grid(sc.get("grid"))
    return o


# the diff-drive box: 0.75 m x 0.5 m at a safety margin of 1 (half-sides 0.375 and 0.25, exact in f32)
DIFF_BOX = dict(vehicle_l=0.75, vehicle_w=0.5, safety_margin=1.0)
DIFF_A, DIFF_B = 0.375, 0.25
DIFF_WEIGHT, DIFF_LETHAL, DIFF_RADIUS = 2.0, 0.5, 0.6
DIFF_WALL_SIDE, DIFF_WALL_AHEAD = 0.75, 0.55


def diff_scene(T, accumulate, grid="64x64"):
    """diff_scene of moving_obstacle_checks.py without circles and an L-shaped wall as in cost_grid_checks.py, further out: leg A
    parallel to the nominal rollout DIFF_WALL_SIDE to its right, leg B across it DIFF_WALL_AHEAD beyond its end.  The lethal
    contour (0.3 m off the wall) lies 0.45 m beside and 0.25 m beyond the nominal line: the box's side points (0.25 m out) and
    its front (0.375 m ahead) reach it where the centre does not."""
    sc = mc.diff_scene(T, accumulate)
    x0 = sc["x0"]
    h = np.array([np.cos(x0[2]), np.sin(x0[2])])
    nrm = np.array([-h[1], h[0]])
    corner = x0[:2] + (mc.TRAVEL + DIFF_WALL_AHEAD) * h - DIFF_WALL_SIDE * nrm
    nx, ny, res = gc.DIFF_GRIDS[grid]
    cells = gc.wall_cells(corner, x0[:2] - 1.0 * h - DIFF_WALL_SIDE * nrm, corner + 1.5 * nrm, DIFF_RADIUS, gc.DIFF_ORIGIN, res, nx, ny)
    return dict(sc, circles=np.zeros((0, 3)), vel=np.zeros((0, 2)), grid=Grid(cells, gc.DIFF_ORIGIN, res, DIFF_WEIGHT, DIFF_LETHAL))


def diff_oracle(sc, K, T, **kw):
    o = FootDiffDriveOracle(ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T, obstacle_circles=sc["circles"],
                            obstacle_velocities=sc["vel"], **dict(mc.DIFF_KW, safety_margin_rate=DIFF_BOX["safety_margin"], **kw))
    o.vehicle_l, o.vehicle_w = DIFF_BOX["vehicle_l"], DIFF_BOX["vehicle_w"]
    o.u_prev[:] = sc["u"]
    o.set_grid(sc.get("grid"))
    return o


# ------------------------------------------------------------------------------------------ cases
HORIZONS = (7, 64, 65, 128)


def diff_cases():
    """(T, accumulate, mode): every horizon with the frozen index, both sums; the threaded indices at T = 65"""
    return [(T, acc, "frozen") for T in HORIZONS for acc in (False, True)] + [(65, False, m) for m in ("per_rollout", "sequential")]


# noise seeds: for each case the first seed at which the f64 reference itself leaves out at most MAX_LEFT_OUT of the samples and
# the case's other conditions hold (test_grid_footprint_cases.py asserts them); cases not listed take seed 0
EPS_SEED = {}
RACE_SEED = 0


def eps_seed(T, accumulate, mode):
    return EPS_SEED.get((T, accumulate, mode), 0)


def diff_case(T, accumulate, mode, K=K_CASE, shift=0, shift_yaw=0, seed=None):
    """-> (scene, eps [K, T, 2] float32, oracle after one iteration, its result)"""
    from oracle import philox
    sc = diff_scene(T, accumulate)
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], eps_seed(T, accumulate, mode) if seed is None else seed, 0, K, T)
    o = diff_oracle(sc, K, T)
    o.shift, o.shift_yaw = shift, shift_yaw
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    return sc, eps, o, res


def race_case(K=K_CASE, circles=2, shift=0, shift_yaw=0, seed=None):
    from oracle import philox
    sc = race_scene(circles)
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), RACE_SEED if seed is None else seed, 0, K, mc.RACE_T)
    o = race_oracle(sc, K)
    o.shift, o.shift_yaw = shift, shift_yaw
    res = o.iteration(sc["x0"], eps)
    return sc, eps, o, res


def diff_closed_loop(T, n_iters, grids, K=K_CASE, mode="frozen", accumulate=False, eps_of=None):
    """cost_grid_checks.diff_closed_loop on the box scene: grids(i) is the Grid in force during iteration i"""
    sc = diff_scene(T, accumulate)
    o = diff_oracle(sc, K, T, **mc.LOOP_KW)
    x = sc["x0"].copy()
    u0, hits, keep, x_at, u_at, counted = [], [], [], [], [], []
    for i in range(n_iters):
        o.set_grid(grids(i))
        o.reset_margins()
        x_at.append(x.copy())
        u_at.append(o.u_prev.copy())
        res = o.iteration_general(x, eps_of(i).astype(np.float64), mode, accumulate)
        u0.append(res["u0_returned"].copy())
        hits.append(int(penalised(res["S"]).sum()))
        counted.append(int((np.asarray(res["S"]) >= PENALTY).sum()))
        keep.append(float((o.sample_margin() > MARGIN).mean()))
        x = mppi_oracle.diffdrive_plant_step(x, res["u0_returned"], mc.DIFF_KW["delta_t"])
        o.tick()
    return dict(scene=sc, u0=np.array(u0), x=x, idx=o.prev_way_point_idx, n_hit=hits, n_counted=counted, kept=keep, x_at=x_at, u_at=u_at)
