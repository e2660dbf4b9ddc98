"""Cost grids (mppi_set_cost_grid): the f64 reference and the scenes of test_cost_grid_cases.py (CPU) and
test_gpu_cost_grid.py.  No device import.

The reference is the oracles of moving_obstacle_checks.py with the grid added where the penalty is: wherever a state is priced
its cost gains weight * g and it counts as hit when g >= lethal or a circle says so, g the bilinear value of the grid at the
state's (x, y) by the formula of include/mppi_hip.h.  It runs on the grid as the handle stores it -- every scene here keeps
cells, origin, 1 / resolution, weight and lethal exactly representable in f32, so one reference serves both precisions.  The
oracles record, per priced state, the decision margin |g - lethal| / lethal beside the circles' margins: the margin rule of
moving_obstacle_checks.py (MARGIN, MAX_LEFT_OUT) then leaves out the samples an f32 handle may decide the other way."""
import numpy as np

import moving_obstacle_checks as mc
from moving_obstacle_checks import MARGIN, MAX_LEFT_OUT, K_CASE, penalised, kept  # noqa: F401  (the tests' names)
from oracle import mppi_oracle
from oracle.mppi_oracle import F32

PENALTY = 1.0e10


class Grid:
    """cells [ny, nx] (rounded to f32, as an f32 handle stores them), origin, resolution, weight, lethal"""

    def __init__(self, cells, origin, resolution, weight=1.0, lethal=np.inf):
        self.cells = np.asarray(cells, np.float32).astype(np.float64)
        self.origin = (float(origin[0]), float(origin[1]))
        self.resolution, self.weight, self.lethal = float(resolution), float(weight), float(lethal)
        for v in (*self.origin, 1.0 / self.resolution, self.weight) + ((self.lethal,) if np.isfinite(self.lethal) else ()):
            assert float(np.float32(v)) == v, v  # one reference for both precisions

    @property
    def kwargs(self):
        return dict(cells=self.cells, origin=self.origin, resolution=self.resolution, weight=self.weight, lethal=self.lethal)

    def value(self, x, y):
        return grid_value(self.cells, self.origin, self.resolution, x, y)


def axis_index(x, o, inv, n, dtype=np.float64):
    """gx = fmin(fmax((x - o) inv, 0), n - 1); i = min((int)gx, n - 2); f = gx - i.  fmax / fmin return the other operand for a
    NaN (np.fmax / np.fmin do too): a NaN lands on node 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.fmin(np.fmax((np.asarray(x, dtype) - dtype(o)) * dtype(inv), dtype(0.0)), dtype(n - 1))
    i = np.minimum(g.astype(np.int64), n - 2)
    return i, g - i.astype(dtype)


def grid_value(cells, origin, resolution, x, y, dtype=np.float64):
    """The bilinear value of include/mppi_hip.h at the points (x, y), in f64 (the fmas written as a product and a sum).  With
    dtype = np.float32 at points whose fractions are 0 or 1 -- nodes -- the products are exact and this is the f32 handle's
    arithmetic bit for bit: at the last node of an axis the formula gives a + (b - a), b to one rounding of the difference."""
    G = np.asarray(cells, dtype)
    ny, nx = G.shape
    inv = 1.0 / resolution
    ix, fx = axis_index(x, origin[0], inv, nx, dtype)
    iy, fy = axis_index(y, origin[1], inv, ny, dtype)
    c0 = fx * (G[iy, ix + 1] - G[iy, ix]) + G[iy, ix]
    c1 = fx * (G[iy + 1, ix + 1] - G[iy + 1, ix]) + G[iy + 1, ix]
    return fy * (c1 - c0) + c0


class _GridCost:
    """What both oracles share: the grid, the margins and flags of the states priced since the last reset, and `shift` --
    every rollout position moved by that many f32 ulps (the sensitivity check of test_cost_grid_cases.py)."""
    grid = None
    shift = 0

    def set_grid(self, grid):
        self.grid = grid
        self.grid_lethal, self.circle_hit, self.grid_term = [], [], []

    def _grid_at(self, x, y):
        """g at the states [K, ...]; records the margin, the lethal flag and weight * g per sample"""
        g = self.grid.value(x, y)
        K = np.shape(x)[0]
        if np.isfinite(self.grid.lethal):
            self.margins.append((np.abs(g - self.grid.lethal) / self.grid.lethal).reshape(K, -1))
        self.grid_lethal.append((g >= self.grid.lethal).reshape(K, -1))
        self.grid_term.append((self.grid.weight * g).reshape(K, -1))
        return g

    def rollout(self, x0, v):
        X = super().rollout(x0, v)
        if self.shift:
            X = X.copy()
            X[..., :2] += self.shift * np.spacing(np.abs(X[..., :2]).astype(np.float32)).astype(X.dtype)
        return X

    def sample_grid_lethal(self):
        return np.concatenate(self.grid_lethal, axis=1).any(axis=1)

    def sample_circle_hit(self):
        return np.concatenate(self.circle_hit, axis=1).any(axis=1)

    def sample_grid_term(self):
        """sum over the priced states of weight * g, per sample"""
        return np.concatenate(self.grid_term, axis=1).sum(axis=1)


class GridDiffDriveOracle(_GridCost, mc.MovingDiffDriveOracle):
    def collided(self, x, y, steps=None):
        """What iteration_general multiplies by the penalty of 1e10: hit + weight g / 1e10, so that the state's cost gains the
        penalty (hit: a circle or g >= lethal) and weight g in the one place the penalty is added.  In f64 the product gives
        weight g back to two roundings."""
        hit = super().collided(x, y, steps) > 0 if len(self.obstacle_circles) else np.zeros(np.shape(x), bool)
        K = np.shape(x)[0]
        self.circle_hit.append(hit.reshape(K, -1))
        if self.grid is None:
            return hit.astype(np.float64)
        g = self._grid_at(np.asarray(x, np.float64), np.asarray(y, np.float64))
        return (hit | (g >= self.grid.lethal)).astype(np.float64) + self.grid.weight * g / PENALTY

    def is_hit(self, x, y, steps=None):
        """the state counts as hit (mppi_eval_is_collided)"""
        return self.collided(x, y, steps) >= 1.0


class GridRaceCarOracle(_GridCost, mc.MovingRaceCarOracle):
    def collided(self, x, y, yaw, steps=None):
        hit = super().collided(x, y, yaw, steps) > 0 if len(self.obstacle_circles) else np.zeros(np.shape(x), bool)
        K = np.shape(x)[0]
        self.circle_hit.append(hit.reshape(K, -1))
        self._g = None
        if self.grid is not None:
            self._g = self._grid_at(np.asarray(x, np.float64), np.asarray(y, np.float64))
            hit = hit | (self._g >= self.grid.lethal)
        return hit.astype(F32)

    def state_cost(self, X, p, weight):
        c = super().state_cost(X, p, weight)  # (tracking + the penalty, through collided above)
        if self.grid is not None:
            c = (c + (self.grid.weight * self._g).astype(F32)).astype(F32)
        return c

    def is_hit(self, x, y, yaw, steps=None):
        return self.collided(np.asarray(x, F32), np.asarray(y, F32), np.asarray(yaw, F32), steps) > 0


# ------------------------------------------------------------------------------------------ scenes
def wall_cells(corner, leg_a, leg_b, radius, origin, resolution, nx, ny):
    """An L-shaped wall -- the segments corner..leg_a and corner..leg_b -- inflated: clip(1 - d / radius, 0, 1), d the distance
    of a node to the wall"""
    xs = origin[0] + resolution * np.arange(nx)
    ys = origin[1] + resolution * np.arange(ny)
    P = np.stack(np.meshgrid(xs, ys), axis=-1)  # [ny, nx, 2]

    def seg(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        t = np.clip(((P - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
        return np.linalg.norm(P - (a + t[..., None] * (b - a)), axis=-1)
    d = np.minimum(seg(corner, leg_a), seg(corner, leg_b))
    return np.clip(1.0 - d / radius, 0.0, 1.0)


# name -> (nx, ny, resolution): 64 x 64, and the same wall on a grid too large for any LDS window
DIFF_GRIDS = {"64x64": (64, 64, 0.125), "300x200": (300, 200, 0.03125)}
DIFF_ORIGIN = (-2.0, -5.0)
DIFF_WEIGHT, DIFF_LETHAL, DIFF_RADIUS = 2.0, 0.5, 0.6
DIFF_CIRCLE_R = 0.34  # (0.4 in diff_scene: the crosser then takes half of the samples, and few stay clear of both)


def diff_wall(sc):
    """Beside the nominal rollout of diff_scene (x0 along h for TRAVEL metres): leg A runs parallel to it 0.55 m to its right
    (g = 0.083 on the nominal line: a soft cost at every step, lethal for the few samples that stray 0.25 m that way), leg B
    crosses it 0.3 m beyond its end (lethal for the samples that get further than the nominal one)."""
    x0 = sc["x0"]
    h = np.array([np.cos(x0[2]), np.sin(x0[2])])
    nrm = np.array([-h[1], h[0]])
    corner = x0[:2] + (mc.TRAVEL + 0.3) * h - 0.55 * nrm
    return corner, x0[:2] - 1.0 * h - 0.55 * nrm, corner + 1.5 * nrm


def diff_scene(T, accumulate, grid="64x64", circles=2):
    """diff_scene of moving_obstacle_checks.py with its first `circles` circles (the crosser, 0.8 m to the LEFT of the meeting
    point, and the leaver: they decide samples the wall on the right and ahead does not) and the wall as a Grid"""
    sc = mc.diff_scene(T, accumulate)
    nx, ny, res = DIFF_GRIDS[grid]
    cells = wall_cells(*diff_wall(sc), DIFF_RADIUS, DIFF_ORIGIN, res, nx, ny)
    c = sc["circles"][:circles].copy()
    c[:, 2] = DIFF_CIRCLE_R
    return dict(sc, circles=c, vel=sc["vel"][:circles], grid=Grid(cells, DIFF_ORIGIN, res, DIFF_WEIGHT, DIFF_LETHAL))


def diff_oracle(sc, K, T, **kw):
    o = GridDiffDriveOracle(ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T, obstacle_circles=sc["circles"],
                            obstacle_velocities=sc["vel"], **dict(mc.DIFF_KW, **kw))
    o.u_prev[:] = sc["u"]
    o.set_grid(sc.get("grid"))
    return o


RACE_WEIGHT, RACE_LETHAL, RACE_RADIUS, RACE_RES = 128.0, 0.5, 3.0, 0.5
RACE_CIRCLE_R = 0.5  # (1.0 in race_scene)


def race_scene(circles=2):
    """race_scene of moving_obstacle_checks.py (10 m of road over the horizon) with its crosser and leaver, and a wall 2.5 m
    to the right of the road that turns across it 11.5 m ahead, inflated by 3 m, on a 64 x 64 grid of 0.5 m cells"""
    sc = mc.race_scene()
    s = sc["x0"]
    h = np.array([np.cos(s[2]), np.sin(s[2])])
    nrm = np.array([-h[1], h[0]])
    corner = s[:2] + 11.5 * h - 2.5 * nrm
    origin = tuple(np.floor(s[:2] + 5.0 * h) - 16.0)
    cells = wall_cells(corner, s[:2] - 4.0 * h - 2.5 * nrm, corner + 8.0 * nrm, RACE_RADIUS, origin, RACE_RES, 64, 64)
    c = sc["circles"][:circles].copy()
    c[:, 2] = RACE_CIRCLE_R
    return dict(sc, circles=c, vel=sc["vel"][:circles], grid=Grid(cells, origin, RACE_RES, RACE_WEIGHT, RACE_LETHAL))


def race_oracle(sc, K):
    o = GridRaceCarOracle(ref_path=sc["ref"], number_of_samples_K=K, obstacle_circles=sc["circles"],
                          obstacle_velocities=sc["vel"], **mc.RACE_KW)
    o.u_prev[:] = sc["u"].astype(F32)
    o.set_grid(sc.get("grid"))
    return o


# ------------------------------------------------------------------------------------------ cases
HORIZONS = (7, 50, 64, 65, 128)  # one chunk, the chunk seam, a full second chunk


def diff_cases():
    """(T, accumulate, mode, grid): every horizon with the frozen index, both sums; the threaded indices at one horizon of each
    kind; the large grid at one horizon of each kind and sum"""
    out = [(T, acc, "frozen", "64x64") for T in HORIZONS for acc in (False, True)]
    out += [(T, False, mode, "64x64") for T in (50, 65) for mode in ("per_rollout", "sequential")]
    out += [(50, False, "frozen", "300x200"), (65, True, "frozen", "300x200")]
    return out


# noise seeds: for each case the first seed at which the f64 reference itself leaves out at most MAX_LEFT_OUT of the samples
# (test_cost_grid_cases.py asserts it); cases not listed take seed 0
EPS_SEED = {}  # (seed 0 serves every case of this scene)


def eps_seed(T, accumulate, mode, grid):
    return EPS_SEED.get((T, accumulate, mode, grid), 0)


def diff_case(T, accumulate, mode, grid="64x64", K=K_CASE, circles=2, shift=0, seed=None):
    """-> (scene, eps [K, T, 2] float32, oracle after one iteration, its result)"""
    from oracle import philox
    sc = diff_scene(T, accumulate, grid, circles)
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], eps_seed(T, accumulate, mode, grid) if seed is None else seed, 0, K, T)
    o = diff_oracle(sc, K, T)
    o.shift = shift
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    return sc, eps, o, res


def race_case(K=K_CASE, circles=2, shift=0, seed=0):
    from oracle import philox
    sc = race_scene(circles)
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), seed, 0, K, mc.RACE_T)
    o = race_oracle(sc, K)
    o.shift = shift
    res = o.iteration(sc["x0"], eps)
    return sc, eps, o, res


def f32_tolerance(S):
    """the f32 handles' bound on |S - S_ref| (test_gpu_moving_obstacles.py: rtol = atol = 2e-4)"""
    return 2e-4 + 2e-4 * np.abs(S)


def diff_closed_loop(T, n_iters, grids, K=K_CASE, mode="frozen", accumulate=False, eps_of=None):
    """moving_obstacle_checks.diff_closed_loop with a grid: grids(i) is the Grid in force during iteration i (the
    rolling-costmap loop re-uploads between two calls)"""
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
        counted.append(int((np.asarray(res["S"]) >= PENALTY).sum()))  # (S >= collision_penalty: the kernels' definition)
        keep.append(float((o.sample_margin() > MARGIN).mean()))
        x = mppi_oracle.diffdrive_plant_step(x, res["u0_returned"], mc.DIFF_KW["delta_t"])
        o.tick()
    return dict(scene=sc, u0=np.array(u0), x=x, idx=o.prev_way_point_idx, n_hit=hits, n_counted=counted, kept=keep, x_at=x_at, u_at=u_at)
