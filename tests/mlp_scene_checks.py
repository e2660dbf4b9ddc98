"""Learned-dynamics scene handles (mppi_config.obstacle_motion = 2): the f64 reference, the weights, the scenes and
the margin rule of test_gpu_mlp_scenes.py.  No device import.

Nothing new is priced here.  The reference is scene_checks.SceneDiffDriveOracle (circles, tracks, grid at the centre) and the
outline oracle of grid_footprint_checks.scene_diff_oracle, each with `rollout` replaced by
mppi_oracle.DiffDriveMlpOracle.rollout -- `iteration_general` calls `self.rollout`, so a subclass of a few lines does it.

THE MARGIN.  A sample is kept out of the S / hit comparisons when any pose the reference tested lies within DELTA of a contour:
a circle's or a track's threshold circle (| |p - c| - r |), or g = lethal measured along the grid's gradient
(|g - lethal| / |grad g|; under the outline: the nearest of the nine points).  DELTA is four times the largest error of the
learned rollout's states against the f64 oracle over the shapes and horizons of these cases, as tools/mlp_scene_report.py
measured it through the sampled-trajectory visualisation (the transition code is the static kernels', unchanged by the scene
forms) and wrote it to profiles/mlp_scene_measured.json; four, because a hit decision adds one rounding of the test itself on top
of the state's error.  For the outline the state's error is its position error plus its yaw error times the outline's reach.
MAX_LEFT_OUT is a condition on the scenes, not a measurement."""
import functools
import json
import os

import numpy as np

import cost_grid_checks as gc
import grid_footprint_checks as gf
import moving_obstacle_checks as mc
import scene_checks as sk
from oracle import mppi_oracle, philox
from test_gpu_mlp_shapes import weights

K = 250  # three full 64-sample tiles and a ragged one
MAX_LEFT_OUT = 0.02
SHAPES = ((64, 1), (128, 2), (256, 3), (512, 3))
KINDS = ("circles", "tracks", "grid", "outline", "composed")
OUTLINE_REACH = float(np.hypot(gf.DIFF_A, gf.DIFF_B))

_MEASURED = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_scene_measured.json")


@functools.lru_cache(maxsize=None)
def measured():
    with open(_MEASURED) as f:
        return json.load(f)


def delta(outline=False):
    """DELTA in metres (see the module's text)"""
    m = measured()
    return 4.0 * (m["max_position_error"] + (OUTLINE_REACH * m["max_yaw_error"] if outline else 0.0))


# ------------------------------------------------------------------------------------------ weights
def nominal_end(w, x0, u, kw):
    o = mppi_oracle.DiffDriveMlpOracle(ref_path=np.zeros((2, 3)), num_samples_K=1, num_horizons_T=len(u), **kw, mlp_weights=w)
    return o.rollout(x0, o.clamp(np.asarray(u, np.float64))[None])[0]


def scene_weights(H, n, x0, u, seed=None, move=0.3):
    """test_gpu_mlp_shapes.weights(H, n, seed) with the output layer scaled so that the residual moves the end of the nominal
    rollout by `move` metres (inside the 0.1 .. 0.5 m that make it another trajectory than the analytic one and keep it inside
    the scenes' geometry): the end's displacement is close to linear in that scale, two secant steps land within a per cent."""
    w = weights(H, n, 10 + H + n if seed is None else seed)
    base = {k: v.copy() for k, v in w.items()}
    kw = {k: v for k, v in mc.DIFF_KW.items() if k != "safety_margin_rate"}
    zero = dict(base, **{"out_layer.weight": base["out_layer.weight"] * 0, "out_layer.bias": base["out_layer.bias"] * 0})
    end0 = nominal_end(zero, x0, u, kw)[-1, :2]
    s = 1.0
    for _ in range(4):
        cur = dict(base, **{"out_layer.weight": (base["out_layer.weight"] * s).astype(np.float32),
                            "out_layer.bias": (base["out_layer.bias"] * s).astype(np.float32)})
        d = float(np.linalg.norm(nominal_end(cur, x0, u, kw)[-1, :2] - end0))
        if abs(d - move) <= 0.02 * move:
            break
        s *= move / max(d, 1e-9)
    assert 0.1 <= d <= 0.5, d
    return cur


# ------------------------------------------------------------------------------------------ the reference
class _Learned:
    """the learned transition in place of the analytic one (what `iteration_general` and the grid oracles call)"""
    mlp_weights = None

    def rollout(self, x0, v):
        X = mppi_oracle.DiffDriveMlpOracle.rollout(self, x0, v)
        self._X = X  # (the outline oracle reads the yaw of the states it prices from here)
        return X


class _AbsMargin:
    """per tested pose, the distance in metres to the nearest contour that could flip its decision"""

    def reset_parts(self):
        super().reset_parts()
        self.abs_margins = []

    def _test(self, px, py, r2, steps):
        K_ = px.shape[0]
        m = np.full(px.shape[:-1], np.inf)

        def against(c, thr2):
            nonlocal m
            d = np.sqrt((px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2)
            m = np.minimum(m, np.abs(d - np.sqrt(thr2)).min(axis=(-1, -2)))
        if len(self.obstacle_circles):
            against(mc.centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps),
                    np.broadcast_to(r2, (len(self.obstacle_circles),)))
        if len(self.track_radii):
            against(sk.ot.track_centres(self.tracks, self.track_clock, steps, self.track_variant), self._track_r2())
        self.abs_margins.append(m.reshape(K_, -1))
        return super()._test(px, py, r2, steps)

    def _grid_points(self, x, y):
        return np.asarray(x, np.float64)[..., None], np.asarray(y, np.float64)[..., None]

    def _grid_at(self, x, y):
        g = super()._grid_at(x, y)
        if np.isfinite(self.grid.lethal):
            px, py = self._grid_points(x, y)
            h = 1e-5
            gp = self.grid.value(px, py)
            gx = (self.grid.value(px + h, py) - self.grid.value(px - h, py)) / (2 * h)
            gy = (self.grid.value(px, py + h) - self.grid.value(px, py - h)) / (2 * h)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(np.hypot(gx, gy) > 0, np.abs(gp - self.grid.lethal) / np.hypot(gx, gy), np.inf)
            # (a point on a cell edge sees two slopes; the central difference averages them, which at most halves one: the
            # factor four of DELTA covers it)
            self.abs_margins.append(d.min(axis=-1).reshape(np.shape(x)[0], -1))
        return g

    def sample_abs_margin(self):
        return np.concatenate(self.abs_margins, axis=1).min(axis=1) if self.abs_margins else np.full(self.K, np.inf)


class MlpSceneOracle(_Learned, _AbsMargin, sk.SceneDiffDriveOracle):
    pass


def scene_oracle(ref, u, K_, T, w, outline=False, **kw):
    if outline:
        o = gf.scene_diff_oracle(ref, u, K_, T, **kw)
        base = o.__class__

        class MlpFootSceneOracle(_Learned, _AbsMargin, base):
            def _grid_points(self, x, y):
                a, b = self.half_sides()
                p = gf.world_points(np.asarray(x, np.float64), np.asarray(y, np.float64),
                                    np.asarray(self._yaw_of(np.shape(x)), np.float64), a, b)
                return p[..., 0], p[..., 1]
        o.__class__ = MlpFootSceneOracle
        o.vehicle_l, o.vehicle_w = gf.DIFF_BOX["vehicle_l"], gf.DIFF_BOX["vehicle_w"]
    else:
        o = MlpSceneOracle(ref_path=ref, num_samples_K=K_, num_horizons_T=T, obstacle_circles=np.zeros((0, 3)), **dict(mc.DIFF_KW, **kw))
        o.u_prev[:] = u
    o.mlp_weights = w
    return o


def kept(o, outline=False):
    return o.sample_abs_margin() > delta(outline)


# ------------------------------------------------------------------------------------------ scenes
def wall_grid(xs, side, ahead, radius, weight, lethal):
    """cost_grid_checks' L-shaped wall on the 64 x 64 case grid beside the pose xs: leg A parallel to the nominal rollout `side`
    metres to its right, leg B across it `ahead` metres beyond its end, inflated over `radius`"""
    nx, ny, res = gc.DIFF_GRIDS["64x64"]
    h, nrm = sk.heading(xs)
    corner = xs[:2] + (mc.TRAVEL + ahead) * h - side * nrm
    cells = gc.wall_cells(corner, xs[:2] - 1.0 * h - side * nrm, corner + 1.5 * nrm, radius, gc.DIFF_ORIGIN, res, nx, ny)
    return gc.Grid(cells, gc.DIFF_ORIGIN, res, weight, lethal)


# What the 7-step cases change in the scenes they inherit, so that the f64 reference alone meets the conditions of
# test_mlp_scene_cases.py (found by scans on the CPU reference; T = 7 ends its samples within 0.1 m of each other and prices
# few states, so the inherited weight of 2 leaves the soft term inside the S tolerance and the inherited walls take nearly all
# samples or nearly none).  (kind, T, accumulate) -> wall = (side, ahead, radius, weight, lethal), circle_r = the circles' radius
TUNE = {
    ("grid", 7, False): dict(wall=(0.55, 0.3, 0.6, 16.0, 0.5)),   # the inherited wall at eight times its weight
    ("grid", 7, True): dict(wall=(0.55, 0.3, 0.6, 16.0, 0.5)),
    ("outline", 7, False): dict(wall=(0.75, 0.7, 0.6, 16.0, 0.5)),  # ... and 0.15 m further ahead: 111 of 250 hit instead of 239
    ("outline", 7, True): dict(wall=(0.75, 0.7, 0.6, 16.0, 0.5)),
    ("composed", 7, False): dict(wall=(0.55, 0.3, 0.6, 16.0, 0.5)),
    # (every step priced: circles of radius 0.34 hit nobody and of 0.44 nearly everybody; the wall 0.05 m nearer: 59 hit, not 20)
    ("composed", 7, True): dict(wall=(0.55, 0.25, 0.6, 16.0, 0.5), circle_r=0.4),
}


def scene(kind, T, accumulate, H=64, n=1, clock=0, extra=0):
    """moving_obstacle_checks.diff_scene's path, state and nominal controls; the learned model; and scene_checks' ingredients
    placed around the LEARNED nominal rollout: they stand beside a pose moved by what the residual moves the nominal rollout
    where it is priced (its end with `S[k] =`, mid-horizon with every step priced)."""
    base = mc.diff_scene(T, accumulate)
    x0, u = base["x0"], base["u"]
    w = scene_weights(H, n, x0, u)
    kw = {k: v for k, v in mc.DIFF_KW.items() if k != "safety_margin_rate"}
    zero = dict(w, **{"out_layer.weight": w["out_layer.weight"] * 0, "out_layer.bias": w["out_layer.bias"] * 0})
    at = T - 1 if not accumulate else round(0.5 * T) - 1
    shift = nominal_end(w, x0, u, kw)[at, :2] - nominal_end(zero, x0, u, kw)[at, :2]
    xs = np.concatenate([x0[:2] + shift, x0[2:]])
    what = {"circles": (), "tracks": ("tracks",), "grid": ("grid",), "outline": ("grid",), "composed": ("grid", "tracks")}[kind]
    ing = sk.diff_ingredients(xs, T, accumulate, clock, extra, circles=0 if kind in ("tracks", "grid", "outline") else 2, what=what)
    if kind == "circles":  # the three moving circles of the moving-obstacle cases, carried over
        c = base["circles"].copy()
        c[:, :2] += shift
        ing.update(circles=c, vel=base["vel"])
    if kind == "outline":  # the wall of the footprint cases: the box's side and front reach the contour where its centre does not
        g = gf.diff_scene(T, accumulate)["grid"]
        ing["grid"] = wall_grid(xs, gf.DIFF_WALL_SIDE, gf.DIFF_WALL_AHEAD, gf.DIFF_RADIUS, g.weight, g.lethal)
    t = TUNE.get((kind, T, accumulate), {})
    if "wall" in t:
        ing["grid"] = wall_grid(xs, *t["wall"])
    if "circle_r" in t:
        ing["circles"] = np.column_stack([ing["circles"][:, :2], np.full(len(ing["circles"]), t["circle_r"])])
    return dict(ref=base["ref"], x0=x0, u=u, w=w, clock=clock, kind=kind, outline=kind == "outline", shape=(H, n), **ing)


def cases():
    """(kind, T, accumulate, mode, H, n): every kind with both sums and the frozen index at both horizons, the threaded indices
    at T = 50 -- all at 64 x 1 --; 128 x 2 and 512 x 3 (the h3 form) once per kind; 256 x 3 once"""
    out = []
    for kind in KINDS:
        out += [(kind, T, acc, "frozen", 64, 1) for T in (7, 50) for acc in (False, True)]
        out += [(kind, 50, False, mode, 64, 1) for mode in ("per_rollout", "sequential")]
        out += [(kind, 50, True, "frozen", 128, 2), (kind, 50, False, "frozen", 512, 3)]
    out.append(("composed", 50, True, "frozen", 256, 3))
    return out


@functools.lru_cache(maxsize=None)
def case(kind, T, accumulate, mode, H=64, n=1, clock=0, extra=0):
    """-> (scene, eps [K, T, 2] float32, the oracle after one iteration at `clock`, its result)"""
    sc = scene(kind, T, accumulate, H, n, clock, extra)
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], 0, 0, K, T)  # (seed 0 serves every case: the scenes were moved, not the noise)
    o = sk.aim(scene_oracle(sc["ref"], sc["u"], K, T, sc["w"], sc["outline"]), sc, clock)
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    res["w"] = o.compute_weight(np.asarray(res["S"], np.float64))
    return sc, eps, o, res
