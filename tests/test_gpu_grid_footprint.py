"""Cost grids under the vehicle's outline on the device (mppi_set_cost_grid_footprint): g_foot and its nine points
against the formula, hit and cost either side of the lethal contour as a side point, a corner and the centre see it, one
iteration against the f64 reference of tests/grid_footprint_checks.py in every CPU case, the bit-for-bit statements, the
composed forms, a closed loop with a shifted wall, the refusals and the Python surface.  K = 250: the last workgroup is ragged.
Every reference is computed once per case and shared by the f32 and the f64 handle."""
import functools

import numpy as np
import pytest

import cost_grid_checks as gc
import grid_footprint_checks as fc
import moving_obstacle_checks as mc
from test_gpu_agent_scenes import compare, diff_cfg, race_cfg
from test_gpu_moving_obstacles import cuda, diff_engine, prec, race_engine

pytestmark = pytest.mark.gpu

K = 250


def box_engine(T, mode, accumulate, precision, K=K, **kw):
    """the diff-drive box: the outline model with the half-sides of grid_footprint_checks.DIFF_BOX"""
    from dnn_mppi_mpc_amd import _capi as capi
    return diff_engine(T, mode, accumulate, precision, K=K, **dict(dict(fc.DIFF_BOX, obstacle_model=capi.OBSTACLE_OUTLINE), **kw))


def car_engine(precision, K=K, **kw):
    return race_engine(precision, K=K, **kw)


def spec_of(e):
    return e.rollout_kernel().split(", ")[4]


def load(e, sc, grid=True, footprint="outline"):
    e.set_ref_path(sc["ref"])
    e.set_obstacles(sc["circles"], velocities=sc["vel"])
    e.set_u_prev(sc["u"])
    if footprint is not None:
        e.set_cost_grid_footprint(footprint)
    if grid:
        e.set_cost_grid(**sc["grid"].kwargs)
    return e


def rounded(a, precision):
    return np.asarray(a, np.float32).astype(np.float64) if precision == "f32" else np.asarray(a, np.float64)


def eps_of(precision):
    return float(np.finfo(np.float32 if precision == "f32" else np.float64).eps)


def formula(cells, origin, res, poses, a, b, precision):
    """the nine points by the header's formula and g_foot from the inputs as the handle stores them, in extended precision
    (np.longdouble: the f64 handle is held to a few f64 roundings, which an f64 restatement would spend itself)"""
    x, y, yaw = (rounded(poses[:, i], precision).astype(np.longdouble) for i in range(3))
    sn, cs = np.sin(yaw), np.cos(yaw)
    q = fc.outline(a, b).astype(np.longdouble)
    px = np.stack([qx * cs - qy * sn + x for qx, qy in q], axis=1)
    py = np.stack([qx * sn + qy * cs + y for qx, qy in q], axis=1)
    px[:, 0], py[:, 0] = x, y
    g = gc.grid_value(cells, origin, res, px, py, dtype=np.longdouble)
    return np.stack([px, py], axis=-1), g.max(axis=1), g


# ------------------------------------------------------------------------------------------ 1. value and points
SHAPES = [(2, 2), (33, 17), (17, 33), (64, 64)]  # (nx, ny)
YAWS = (0.0, np.pi / 2, 0.3, -2.5, 1.0e3)
ORIGIN, RES = (-8.0, -8.0), 0.5  # (exact in f32; the poses inside stand at x, y >= 0: |p| <= |p - origin| for every point)


def value_poses(nx, ny, rng):
    span_x, span_y = RES * (nx - 1), RES * (ny - 1)
    inside = np.stack([rng.uniform(0.0, max(span_x - 8.0, 0.5), 24), rng.uniform(0.0, max(span_y - 8.0, 0.5), 24)], axis=1)
    edge = np.stack([np.full(8, ORIGIN[0] + span_x), rng.uniform(0.0, 4.0, 8)], axis=1)  # the centre on the grid's last column
    far = np.array([[1.0e4, 1.0e4], [-1.0e4, 1.0e4], [1.0e4, -1.0e4], [-1.0e4, -1.0e4], [0.25, -1.0e4], [1.0e4, 0.25]])
    xy = np.concatenate([inside, edge, far])
    return np.concatenate([np.concatenate([xy, np.full((len(xy), 1), yaw)], axis=1) for yaw in YAWS])


def smooth_cells(nx, ny, rng):
    """A costmap-like field, 0.5 <= g <= 2.5 and neighbouring nodes at most 0.0125 <= gmax / 32 apart, other wavelengths along x than along y (a
    swap of axes shows).  The f64 bound below has no position term, so it is a bound only for such fields: a point carries four
    roundings of half an ulp of |p - origin| <= 40, in node units (inv = 2) 4 * eps / 2 * 80; each axis passes that on times
    dmax; three fmas add half an ulp of gmax each: 2 * 160 eps * gmax / 32 + 1.5 eps gmax = 11.5 eps gmax < 16 eps gmax."""
    ix, iy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    kx, ky = rng.uniform(0.015, 0.025, 2)
    return 1.5 + 0.5 * np.sin(kx * ix + rng.uniform(0, 6.28)) + 0.5 * np.sin(ky * iy + rng.uniform(0, 6.28))


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["race", "diff"])
def test_value_and_points_against_the_formula(model, precision):
    """Every shape on one handle, in CENTRE mode (the entry point answers in either) and then in OUTLINE mode.
    g_foot: f64 16 eps gmax; f32 4 eps (pmax inv dmax + gmax) -- four roundings: rotation product, rotation sum, offset,
    scale; pmax the largest |coordinate - origin| among the points, dmax the largest difference between neighbouring nodes.
    The points: 4 eps (|p| + a + b).
    (With cells drawn independently -- dmax = 1.5 gmax -- the f32 bound held with a factor of 12 to spare and the f64 bound was
    missed by up to 1.7 x on the 64 x 64 grid: it has no term for the position's own rounding.  See smooth_cells.)"""
    e = car_engine(precision) if model == "race" else box_engine(50, "frozen", False, precision)
    a, b = (fc.RACE_A, fc.RACE_B) if model == "race" else (fc.DIFF_A, fc.DIFF_B)
    e.set_ref_path(mc.race_scene()["ref"] if model == "race" else mc.diff_scene(50, False)["ref"])
    rng = np.random.default_rng(7)
    eps = eps_of(precision)
    worst_g = worst_p = 0.0
    for i, (nx, ny) in enumerate(SHAPES):
        if i == 2:
            e.set_cost_grid_footprint("outline")
        cells = rounded(smooth_cells(nx, ny, rng), "f32")
        e.set_cost_grid(cells, ORIGIN, RES)
        poses = value_poses(nx, ny, rng)
        got, pts = e.cost_grid_footprint_at(poses, points=True)
        want_p, want_g, g9 = formula(cells, ORIGIN, RES, poses, a, b, precision)
        tol_p = 4.0 * eps * (np.abs(want_p) + a + b)
        err_p = np.abs(pts - want_p)
        np.testing.assert_array_equal(pts[:, 0], want_p[:, 0])  # the centre is the pose's own position
        gmax = np.abs(cells).max()
        dmax = max(np.abs(np.diff(cells, axis=0)).max(), np.abs(np.diff(cells, axis=1)).max())
        assert dmax <= gmax / 32.0
        pmax = np.abs(want_p - np.asarray(ORIGIN)).max(axis=(1, 2))
        tol_g = 16.0 * eps * gmax if precision == "f64" else 4.0 * eps * (pmax / RES * dmax + gmax)
        worst_p, worst_g = max(worst_p, float((err_p / tol_p).max())), max(worst_g, float((np.abs(got - want_g) / tol_g).max()))
        print(model, precision, (nx, ny), "points: worst error / tolerance", float((err_p / tol_p).max()),
              "g_foot: worst error / tolerance", float((np.abs(got - want_g) / tol_g).max()))
        assert np.all(err_p <= tol_p)
        assert np.all(np.abs(got - want_g) <= tol_g)
        if nx > 2:
            assert (g9.argmax(axis=1) != 0).mean() > 0.5  # the outline matters on these grids
        centre = e.cost_grid_at(poses[:, :2])  # mppi_eval_cost_grid stays the raw centre value, in either mode
        assert np.all(got >= centre)
        np.testing.assert_allclose(centre, g9[:, 0], rtol=0, atol=float(np.max(tol_g)))
    print(model, precision, "worst over the shapes: points", worst_p, "g_foot", worst_g)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["race", "diff"])
def test_each_of_the_nine_points_finds_a_lone_peak(model, precision):
    """A grid that is zero except one node; nine poses at yaw 0 and nine at yaw pi each put exactly one of the nine points on that
    node -- the others stand at least a cell away (the cell is smaller than the outline's spacing) -- and each returns the peak:
    a dropped or mis-signed point fails."""
    e = car_engine(precision) if model == "race" else box_engine(50, "frozen", False, precision)
    a, b = (fc.RACE_A, fc.RACE_B) if model == "race" else (fc.DIFF_A, fc.DIFF_B)
    res = 0.125 if model == "diff" else 1.0  # (b = 0.25 / 2.25: two cells apart at least)
    e.set_ref_path(mc.race_scene()["ref"] if model == "race" else mc.diff_scene(50, False)["ref"])
    cells = np.zeros((33, 33))
    cells[16, 20] = 5.0
    origin = (-16.0 * res, -16.0 * res)
    peak = np.array([origin[0] + 20 * res, origin[1] + 16 * res])
    e.set_cost_grid(cells, origin, res)
    q = fc.outline(a, b)
    at0 = np.concatenate([peak - q, np.zeros((9, 1))], axis=1)
    # yaw pi: cos = -1 to the last bit, sin = 1.2e-16 (-8.7e-8 in f32): the point lands within 3e-7 of the node, the value
    # within 5 * 3e-7 / res of the peak
    yaw_pi = float(np.float32(np.pi)) if precision == "f32" else np.pi
    atpi = np.concatenate([peak + q, np.full((9, 1), yaw_pi)], axis=1)
    for mode in ("centre", "outline"):
        e.set_cost_grid_footprint(mode)
        got = e.cost_grid_footprint_at(at0)
        np.testing.assert_array_equal(got, np.full(9, 5.0))
        got = e.cost_grid_footprint_at(atpi)
        np.testing.assert_allclose(got, 5.0, rtol=0, atol=5.0 * 4e-7 * (a + b) / res if precision == "f32" else 1e-13)
    centre = e.cost_grid_at(at0[:, :2])
    assert centre[0] == 5.0 and not centre[1:].any()  # without the outline eight of the nine see nothing


# ------------------------------------------------------------------------------------------ 2. the lethal contour
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_hit_and_cost_either_side_of_the_lethal_contour(model, precision):
    """A ramp g = x - ox makes the contour of a POINT the line x = ox + lethal; the pose's contour lies where its point of
    largest x reaches it: a side point at yaw pi / 2 (the right side, b out), a corner at yaw 0.3 and -2.5.  A ridge
    g = top - |x - xr| is highest under the point nearest the ridge: the centre, for poses within a / 2 of it at yaw 0.
    Poses 1e-3 m either side of each contour; no circles."""
    T = 50 if model == "diff" else mc.RACE_T
    a, b = (fc.DIFF_A, fc.DIFF_B) if model == "diff" else (fc.RACE_A, fc.RACE_B)
    sc = fc.diff_scene(T, True) if model == "diff" else fc.race_scene(circles=0)
    nx, ny, res = 64, 48, 0.5
    origin = (float(np.floor(sc["x0"][0]) - 2.0), float(np.floor(sc["x0"][1]) - 12.0))
    lethal, weight = 8.25, 4.0
    ramp = np.broadcast_to(res * np.arange(nx, dtype=np.float64), (ny, nx)).copy()
    xr = 16.0  # the ridge, relative to the origin; its contour for the centre: |x - xr| = a / 4
    ridge = np.broadcast_to(lethal + 0.25 * a - np.abs(res * np.arange(nx, dtype=np.float64) - xr), (ny, nx)).copy()
    rng = np.random.default_rng(3)
    n = 96
    side = np.where(np.arange(n) % 2 == 0, 1e-3, -1e-3)  # (+: the far side of the contour, hit)
    for name, cells in (("ramp", ramp), ("ridge", ridge)):
        grid = fc.Grid(cells, origin, res, weight, lethal)
        e = load(box_engine(T, "frozen", True, precision) if model == "diff" else car_engine(precision), dict(sc, grid=grid))
        plain = load(box_engine(T, "frozen", True, precision) if model == "diff" else car_engine(precision), sc, grid=False, footprint=None)
        poses = np.zeros((n, e.nx))
        poses[:, 1] = origin[1] + rng.uniform(4.0, res * (ny - 1) - 4.0, n)
        if name == "ramp":
            yaw = np.array([np.pi / 2, 0.3, -2.5])[np.arange(n) % 3]
            reach = np.abs(a * np.cos(yaw)) + np.abs(b * np.sin(yaw))  # how far the outline reaches in +x
            poses[:, 0] = origin[0] + lethal - reach + side
            poses[:, 2] = yaw
            by = np.array(["side", "corner", "corner"])[np.arange(n) % 3]
        else:
            poses[:, 0] = origin[0] + xr + np.where(np.arange(n) % 4 < 2, 1.0, -1.0) * (0.25 * a - side)
            by = np.full(n, "centre")
        g, g0 = fc.footprint_value(grid, rounded(poses[:, 0], precision), rounded(poses[:, 1], precision), rounded(poses[:, 2], precision), a, b)
        want = g >= lethal
        outside = np.abs(g - lethal) / lethal > fc.MARGIN
        got = e.eval_is_collided(poses) > 0
        print(model, precision, name, "hit", want.mean(), "outside the margin", outside.mean(), "centre alone lethal", (g0 >= lethal).mean())
        assert outside.mean() > 0.95 and np.array_equal(want[outside], (side > 0)[outside])
        if name == "ramp":
            assert not (g0 >= lethal).any()  # the centre alone sees none of them
        else:
            assert np.array_equal((g0 >= lethal)[outside], want[outside])  # the centre decides
        for kind in set(by):
            assert want[by == kind].any() and not want[by == kind].all()
        assert np.array_equal(got[outside], want[outside])
        assert np.array_equal(e.eval_is_collided(poses, steps=np.zeros(n, np.int32))[outside] > 0, want[outside])
        assert not (plain.eval_is_collided(poses) > 0).any()
        for terminal in (False, True):
            c_grid, idx, _ = e.eval_cost(poses, terminal=terminal, prev_idx=0)
            c_plain, idx2, _ = plain.eval_cost(poses, terminal=terminal, prev_idx=0)
            expect = c_plain + np.where(got, 1e10, 0.0) + weight * g
            assert np.array_equal(idx, idx2)
            np.testing.assert_allclose(c_grid[outside], expect[outside], rtol=1e-12 if precision == "f64" else 2e-6, atol=0)
        # CENTRE on the same handle: the raw value at the pose's position decides again
        e.set_cost_grid_footprint("centre")
        assert np.array_equal((e.eval_is_collided(poses) > 0)[outside], (g0 >= lethal)[outside])


# ------------------------------------------------------------------------------------------ 3. one iteration
@functools.lru_cache(maxsize=None)
def diff_reference(T, accumulate, mode):
    return fc.diff_case(T, accumulate, mode, K=K)


@functools.lru_cache(maxsize=None)
def race_reference(circles):
    return fc.race_case(K=K, circles=circles)


def check_iteration(e, sc, eps, o, res, precision, sequential=False, f32_reference=False, spec="8", multi="false"):
    """One iteration with injected noise against the reference: S within f32_tolerance (f32) / 1e-9 (f64) on the samples kept,
    the hits equal on the samples kept."""
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = fc.kept(o, precision == "f64" and not f32_reference)
    hit_ref = fc.penalised(S_ref)
    err_u = float(np.sqrt(np.mean((u - res["u_returned"]) ** 2)))
    tol = fc.f32_tolerance(S_ref) if (precision == "f32" or f32_reference) else 1e-9 * np.maximum(np.abs(S_ref), 1.0)
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "worst |dS| / tolerance", float(np.max(np.abs(S - S_ref)[keep] / tol[keep])))
    assert keep.mean() >= 1.0 - fc.MAX_LEFT_OUT
    assert np.array_equal(fc.penalised(S)[keep], hit_ref[keep])  # no flip outside the margin
    assert st.n_collided == int((S >= 1.0e10).sum())
    assert np.all(np.abs(S - S_ref)[keep] <= tol[keep])
    if precision == "f64" and not f32_reference:
        np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == int((S_ref >= 1.0e10).sum())
    else:
        assert err_u <= 1e-4
    if sequential:
        assert st.rounds >= 1 and st.idx_after == res["idx_after"] and res["idx_after"] > res["idx_start"]
    name = e.rollout_kernel()
    assert name.startswith("k_rollout_fused<") and name.endswith(f", {multi}, {spec}, false>"), name
    return st


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode", fc.diff_cases())
def test_diff_iteration_against_the_reference(T, accumulate, mode, precision):
    """the box with a grid and no circles: n_collided counts the grid's hits"""
    sc, eps, o, res = diff_reference(T, accumulate, mode)
    e = load(box_engine(T, mode, accumulate, precision), sc)
    st = check_iteration(e, sc, eps, o, res, precision, sequential=mode == "sequential")
    assert e.rollout_kernel().split(", ")[2] == ("1" if T <= 64 else "2")
    n_ref = int(fc.penalised(res["S"]).sum())
    assert n_ref == int(o.sample_grid_lethal().sum()) and K // 16 <= n_ref <= K - K // 16
    assert abs(st.n_collided - n_ref) <= int((~fc.kept(o, precision == "f64")).sum())
    assert int(o.sample_centre_lethal().sum()) + K // 16 <= n_ref  # sampling the centre only fails here


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("circles", [0, 2])
def test_race_iteration_against_the_reference(circles, precision):
    sc, eps, o, res = race_reference(circles)
    e = load(car_engine(precision), sc)
    st = check_iteration(e, sc, eps, o, res, precision, f32_reference=True)  # (the reference itself is f32)
    if circles == 0:  # a grid and no circles: n_collided counts its hits
        n_ref = int(o.sample_grid_lethal().sum())
        assert n_ref >= K // 16 and abs(st.n_collided - n_ref) <= int((~fc.kept(o, False)).sum())


# ------------------------------------------------------------------------------------------ 4. bit for bit
def state_of(e):
    return e.get_u_prev(), e.get_state(), e.costs(), int(e.stats.n_collided)


def assert_same(a, b):
    for x, y in zip(state_of(a), state_of(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_centre_is_the_handle_of_today(model, precision):
    """never called, CENTRE set, OUTLINE then CENTRE: the same kernel and the same bits; OUTLINE names a new kernel and matters"""
    sc = fc.diff_scene(50, True) if model == "diff" else fc.race_scene()

    def make():
        return box_engine(50, "frozen", True, precision, seed=3) if model == "diff" else car_engine(precision)
    never = load(make(), sc, footprint=None)
    centre = load(make(), sc, footprint="centre")
    back = load(make(), sc, footprint="outline")
    outline = load(make(), sc, footprint="outline")
    assert back.cost_grid_footprint == "outline"
    back.set_cost_grid_footprint("centre")
    assert [h.cost_grid_footprint for h in (never, centre, back, outline)] == ["centre", "centre", "centre", "outline"]
    for h in (never, centre, back, outline):
        h.set_state(sc["x0"])
        h.run_closed_loop(2)
    assert never.rollout_kernel() == centre.rollout_kernel() == back.rollout_kernel() and spec_of(never) == "6"
    assert outline.rollout_kernel() == never.rollout_kernel().replace(", 6, false>", ", 8, false>")
    assert_same(never, centre)
    assert_same(never, back)
    assert not np.array_equal(never.costs(), outline.costs())
    # the mode outlives the grid: removed, the handle runs the moving form; uploaded again, the footprint form
    outline.set_cost_grid(None)
    outline.run_closed_loop(1)  # (the kernel's name is that of the last launch)
    assert spec_of(outline) == "3" and outline.cost_grid_footprint == "outline"
    outline.set_cost_grid(**sc["grid"].kwargs)
    outline.run_closed_loop(1)
    assert spec_of(outline) == "8"


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_replay_equals_eager_across_a_same_shape_upload(monkeypatch, precision):
    T, n_it = 50, 3
    sc = fc.diff_scene(T, True)
    shifted = dict(sc["grid"].kwargs, cells=np.roll(sc["grid"].cells, 1, axis=1))

    def run(e):
        e.set_state(sc["x0"])
        e.run_closed_loop(n_it)
        e.set_cost_grid(**shifted)  # the same shape: buffers, plan and a cached graph stay
        e.run_closed_loop(n_it)
        return e
    eager = load(box_engine(T, "frozen", True, precision, seed=31), sc)
    eager.set_state(sc["x0"])
    for _ in range(n_it):
        eager.run_closed_loop(1)
    eager.set_cost_grid(**shifted)
    for _ in range(n_it):
        eager.run_closed_loop(1)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = run(load(box_engine(T, "frozen", True, precision, seed=31), sc))
    assert_same(eager, graph)
    assert spec_of(graph) == "8" and eager.stats.n_collided > 0
    unshifted = load(box_engine(T, "frozen", True, precision, seed=31), sc)
    unshifted.set_state(sc["x0"])
    unshifted.run_closed_loop(2 * n_it)
    assert not np.array_equal(unshifted.costs(), graph.costs())  # the re-upload was seen


@pytest.mark.parametrize("model,precision", [("diff", "f64"), ("diff", "f32"), ("race", "f32")])
def test_agents_with_own_grids_equal_single_handles(model, precision):
    """Three agents: the shared 64 x 64 grid; an own 33 x 17 grid of other weight and lethal; no grid.  Bit for bit against
    single-agent handles, all in OUTLINE mode."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if model == "diff":
        T, sc = 50, fc.diff_scene(50, True)
        cfg = dict(diff_cfg(capi.WAYPOINT_FROZEN, T, precision=prec(precision)), obstacle_motion=1, accumulate_stage_cost=1,
                   obstacle_model=capi.OBSTACLE_OUTLINE, **fc.DIFF_BOX)
        x0 = sc["x0"]
        end = x0[:2] + mc.TRAVEL * np.array([np.cos(x0[2]), np.sin(x0[2])])
        origin = tuple(np.floor(end) - (4.0, 2.0))
        own = fc.Grid(gc.wall_cells(*gc.diff_wall(sc), 0.9, origin, 0.25, 33, 17), origin, 0.25, 0.5, 0.25)
    else:
        T, sc = mc.RACE_T, fc.race_scene()
        cfg = dict(race_cfg(), precision=prec(precision), obstacle_motion=1)
        g = sc["grid"]
        own = fc.Grid(g.cells[12:29, 16:49] * 0.5, (g.origin[0] + 8.0, g.origin[1] + 6.0), 0.5, 32.0, 0.09375)
    grids = [None, own, None]  # (agent 0: the shared one)
    rng = np.random.default_rng(11)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(3)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(3)])
    batch = pkg.Engine(K=K, n_agents=3, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(3)]
    batch.set_ref_path(sc["ref"])
    batch.set_state(x0)
    batch.set_u_prev(u)
    none = (np.zeros((0, 3)), np.zeros((0, 2)))
    batch.set_obstacles(none[0], velocities=none[1])
    batch.set_cost_grid_footprint("outline")
    batch.set_cost_grid(**sc["grid"].kwargs)
    batch.set_cost_grid(**own.kwargs, agent=1)
    batch.set_cost_grid(None, agent=2)
    for a, one in enumerate(singles):
        one.set_ref_path(sc["ref"])
        one.set_state(x0[a])
        one.set_u_prev(u[a])
        one.set_obstacles(none[0], velocities=none[1])
        one.set_cost_grid_footprint("outline")
        if a < 2:
            one.set_cost_grid(**(sc["grid"] if a == 0 else own).kwargs)
    hits = []
    for n_run in (1, 3):
        batch.run_closed_loop(n_run)
        for one in singles:
            one.run_closed_loop(n_run)
        compare(batch, singles, None)
        hits.append([int(one.stats.n_collided) for one in singles])
    poses = np.stack([np.concatenate([sc["x0"][:2] + [0.3 * i, -0.2 * i], [0.4 * i]]) for i in range(8)])
    for a in range(2):
        np.testing.assert_array_equal(batch.cost_grid_footprint_at(poses, agent=a), singles[a].cost_grid_footprint_at(poses))
    with pytest.raises(pkg.MppiError) as ex:
        batch.cost_grid_footprint_at(poses, agent=2)
    assert ex.value.code == capi.ERR_STATE
    print(model, precision, "n_collided per agent and stretch", hits, batch.rollout_kernel())
    assert hits[0][0] > 0 and hits[0][2] == 0
    assert ", true, 8, " in batch.rollout_kernel() and ", false, 8, " in singles[1].rollout_kernel()
    assert ", false, 3, " in singles[2].rollout_kernel()


# ------------------------------------------------------------------------------------------ 5. composed
@functools.lru_cache(maxsize=None)
def race_track_reference():
    """scene_checks.race_scene's track beside the footprint scene's wall and circles"""
    import scene_checks as sk
    from oracle import philox
    sc = fc.race_scene()
    trk = sk.race_scene(0)
    sc = dict(sc, clock=0, tracks=trk["tracks"], radii=trk["radii"])
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), 0, 0, K, mc.RACE_T)
    o = sk.aim(fc.scene_race_oracle(sc["ref"], sc["u"], K), sc, 0)
    return sc, eps, o, o.iteration(sc["x0"], eps)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_composed_grid_and_tracks_on_one_agent(precision):
    sc, eps, o, res = race_track_reference()
    e = car_engine(precision)
    e.set_scene_mode("composed")
    load(e, sc, grid=False)
    e.set_obstacle_tracks(sc["tracks"], sc["radii"])
    e.set_cost_grid(**sc["grid"].kwargs)
    check_iteration(e, sc, eps, o, res, precision, f32_reference=True, spec="9")
    track_alone = o.sample_hit("tracks") & ~o.sample_grid_lethal() & ~o.sample_hit("circles")
    grid_alone = o.sample_grid_lethal() & ~o.sample_hit("tracks") & ~o.sample_hit("circles")
    print("the track alone decides", int(track_alone.sum()), "the footprint grid alone", int(grid_alone.sum()), "of", K)
    assert track_alone.any() and grid_alone.any()
    e.set_obstacle_tracks(np.zeros((0, 1, 2)), np.zeros(0))  # without the tracks: the footprint grid form again
    e.run_closed_loop(1)
    assert spec_of(e) == "8"
    e.set_cost_grid_footprint("centre")
    e.run_closed_loop(1)
    assert spec_of(e) == "6"


FLEET_T = 50


@functools.lru_cache(maxsize=None)
def fleet_reference():
    """scene_checks.fleet_scene with the grid and the plans (no tracks), every agent the box: the outline against the mates'
    plans (threshold: fleet_radius itself) and under the grid"""
    import fleet_checks
    import fleet_plan_checks as pc
    import scene_checks as sk
    import test_gpu_fleet as tf
    from dnn_mppi_mpc_amd import _capi as capi
    sc = sk.fleet_scene(FLEET_T, False, ("grid", "plans"))
    kw = dict(fc.DIFF_BOX, obstacle_model=capi.OBSTACLE_OUTLINE, seed=99)
    noise = tf.engine("diff", "f32", 3, FLEET_T, K=K, **kw)
    eps = noise.sample_epsilon(0).cpu().numpy()  # (what the kernels draw)
    noise.close()
    P = pc.plans(sc["x0"], sc["u"], "diff", pc.plan_cfg("diff"))
    runs = []
    for a in range(3):
        o = fc.scene_diff_oracle(sc["refs"][a], sc["u"][a], K, FLEET_T)
        # (the outline model's thresholds are the radii themselves: the circles' own, fleet_radius for a mate)
        sk.aim(o, sc["per"][a], 0, pc.mates_of(P, a), fleet_checks.RADIUS ** 2)
        runs.append((o, o.iteration_general(sc["x0"][a], np.asarray(eps[a], np.float64), "frozen", False)))
    return sc, kw, runs


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_composed_grid_and_plans_on_a_fleet_of_three(precision):
    import test_gpu_fleet as tf
    from test_gpu_scene import load_fleet
    sc, kw, runs = fleet_reference()
    e = tf.engine("diff", precision, 3, FLEET_T, K=K, **kw)
    e.set_cost_grid_footprint("outline")
    load_fleet(e, sc)
    e.run_closed_loop(1)
    S = e.costs()
    for a, (o, res) in enumerate(runs):
        S_ref = np.asarray(res["S"], np.float64)
        keep = fc.kept(o, precision == "f64")
        tol = fc.f32_tolerance(S_ref) if precision == "f32" else 1e-9 * np.maximum(np.abs(S_ref), 1.0)
        print("agent", a, precision, "kept", keep.mean(), "penalised", fc.penalised(S_ref).mean(), "by the plans", o.sample_hit("plans").mean(),
              "by the grid", o.sample_hit("grid").mean(), "worst |dS| / tolerance", float(np.max(np.abs(S[a] - S_ref)[keep] / tol[keep])))
        assert keep.mean() >= 1.0 - fc.MAX_LEFT_OUT
        assert np.array_equal(fc.penalised(S[a])[keep], fc.penalised(S_ref)[keep])
        assert np.all(np.abs(S[a] - S_ref)[keep] <= tol[keep])
    o0 = runs[0][0]
    assert o0.sample_hit("plans").any() and o0.sample_hit("grid").any() and not fc.penalised(runs[0][1]["S"]).all()
    assert e.rollout_kernel().endswith(", true, 9, false>"), e.rollout_kernel()
    assert e.stats.n_collided == int((S[0] >= 1.0e10).sum())


# ------------------------------------------------------------------------------------------ 6. the closed loop
LOOP_T, LOOP_N, LOOP_SWAP = 50, 6, 3
LOOP_W = dict(stage_cost_weight=[0.25, 0.25, 0.5, 0], terminal_cost_weight=[0.25, 0.25, 0.5, 0])


def loop_grids():
    g = fc.diff_scene(LOOP_T, True)["grid"]
    return g, fc.Grid(np.roll(g.cells, 1, axis=1), g.origin, g.resolution, g.weight, g.lethal)  # the wall shifted by one cell


@functools.lru_cache(maxsize=None)
def loop_reference():
    """The reference loop on the noise the device's sampler draws (mppi_sample_epsilon: bit for bit what the kernels draw)."""
    e = box_engine(LOOP_T, "frozen", True, "f32", seed=31, **LOOP_W)
    ring = [e.sample_epsilon(i).cpu().numpy() for i in range(LOOP_N)]
    e.close()
    g, moved = loop_grids()
    return fc.diff_closed_loop(LOOP_T, LOOP_N, lambda i: g if i < LOOP_SWAP else moved, K=K, accumulate=True, eps_of=lambda i: ring[i])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_closed_loop_with_the_wall_shifted(precision):
    """Six iterations, the wall shifted by one cell between the third and the fourth, u0 as test_gpu_cost_grid.py holds it:
    f64 end to end; f32 re-seeded with the reference's state and controls before every iteration."""
    ref = loop_reference()
    sc = ref["scene"]
    g, moved = loop_grids()
    # (under the loop's light tracking weights the robot steers clear of the wall within three iterations: the hits fall from 188
    # of 250 to a handful, the soft cost weight * g_foot stays)
    assert min(ref["kept"]) >= 1.0 - fc.MAX_LEFT_OUT and ref["n_hit"][0] > K // 2 and sum(ref["n_hit"][LOOP_SWAP:]) > 0
    e = load(box_engine(LOOP_T, "frozen", True, precision, seed=31, **LOOP_W), sc)
    e.set_state(sc["x0"])
    if precision == "f64":
        t1, _ = e.run_closed_loop(LOOP_SWAP, trace=True)
        e.set_cost_grid(**moved.kwargs)
        t2, st = e.run_closed_loop(LOOP_N - LOOP_SWAP, trace=True)
        print("reference hits per iteration", ref["n_hit"], "last n_collided", st.n_collided)
        np.testing.assert_allclose(np.concatenate([t1, t2]), ref["u0"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(e.get_state(), ref["x"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == ref["n_counted"][-1]
    else:
        for i in range(LOOP_N):
            if i == LOOP_SWAP:
                e.set_cost_grid(**moved.kwargs)
            e.set_state(ref["x_at"][i])
            e.set_u_prev(ref["u_at"][i])
            trace, st = e.run_closed_loop(1, trace=True)
            err = float(np.sqrt(np.mean((trace[0] - ref["u0"][i]) ** 2)))
            print("iteration", i, "u0 error", err, "n_collided", st.n_collided, "reference", ref["n_hit"][i])
            assert err <= 1e-4
    assert st.iteration == LOOP_N and spec_of(e) == "8"


# ------------------------------------------------------------------------------------------ 7. refusals and the Python surface
def test_refusals_name_the_limit_and_change_nothing():
    import ctypes as C
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = fc.diff_scene(T, True)
    e = load(box_engine(T, "frozen", True, "f64", seed=3), sc)
    twin = load(box_engine(T, "frozen", True, "f64", seed=3), sc)

    def refused(call, code, word=None):
        with pytest.raises(pkg.MppiError) as ex:
            call()
        assert ex.value.code == code, str(ex.value)
        assert word is None or word in str(ex.value), str(ex.value)
    refused(lambda: e.set_cost_grid_footprint("disc"), capi.ERR_BAD_ARG)
    for mode in (2, -1):
        assert e.lib.mppi_set_cost_grid_footprint(e._h, mode) == capi.ERR_BAD_ARG
        assert b"MPPI_GRID_FOOTPRINT_OUTLINE" in e.lib.mppi_last_error(e._h)
    assert e.lib.mppi_get_cost_grid_footprint(e._h, None) == capi.ERR_BAD_ARG
    m = C.c_int32(-1)
    assert e.lib.mppi_get_cost_grid_footprint(e._h, C.byref(m)) == capi.OK and m.value == capi.GRID_FOOTPRINT_OUTLINE
    poses = np.stack([np.concatenate([sc["x0"][:2] + [0.3 * i, -0.2 * i], [0.5 * i]]) for i in range(8)])
    refused(lambda: e.cost_grid_footprint_at(poses, agent=1), capi.ERR_BAD_ARG, "agent")
    assert e.lib.mppi_eval_cost_grid_footprint(e._h, 0, None, 8, None, None) == capi.ERR_BAD_ARG
    assert e.cost_grid_footprint == "outline"
    np.testing.assert_array_equal(e.cost_grid_footprint_at(poses), twin.cost_grid_footprint_at(poses))
    for h in (e, twin):
        h.set_state(sc["x0"])
        h.run_closed_loop(2)
    assert_same(e, twin)
    # handles that take no outline footprint
    static = box_engine(T, "frozen", True, "f64", obstacle_motion=0)
    for mode in ("centre", "outline"):
        refused(lambda: static.set_cost_grid_footprint(mode), capi.ERR_STATE, "obstacle_motion")
    disc = diff_engine(T, "frozen", True, "f64")  # (the circle model)
    refused(lambda: disc.set_cost_grid_footprint("outline"), capi.ERR_UNSUPPORTED, "inflating the map by its radius")
    disc.set_cost_grid_footprint("centre")  # CENTRE: any handle with obstacle_motion
    assert disc.cost_grid_footprint == "centre"
    long = box_engine(130, "frozen", True, "f64")
    refused(lambda: long.set_cost_grid_footprint("outline"), capi.ERR_UNSUPPORTED, "T <= 128")
    long.set_cost_grid_footprint("centre")
    assert long.cost_grid_footprint == "centre"
    nogrid = box_engine(T, "frozen", True, "f64")
    nogrid.set_cost_grid_footprint("outline")  # before any grid exists
    refused(lambda: nogrid.cost_grid_footprint_at(poses), capi.ERR_STATE, "no cost grid")
    nogrid.set_ref_path(sc["ref"])
    nogrid.set_cost_grid(**sc["grid"].kwargs)
    nogrid.set_state(sc["x0"])
    nogrid.run_closed_loop(1)
    assert spec_of(nogrid) == "8"


def test_controllers_carry_the_footprint_key():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    rs = fc.race_scene()
    kw = dict(ref_path=rs["ref"], horizon_step_T=mc.RACE_T, number_of_samples_K=64)
    rc = pkg.MPPIRacecarController(**kw, cost_grid=dict(rs["grid"].kwargs, footprint="outline"))
    assert rc._engine.cost_grid_footprint == "outline" and rc.cost_grid["footprint"] == "outline"
    rc._engine.set_state(rs["x0"])
    rc._engine.run_closed_loop(1)
    assert rc._engine.rollout_kernel().endswith(", 8, false>")
    pose = rs["x0"][None, :3]
    want, _ = fc.footprint_value(rs["grid"], pose[:, 0], pose[:, 1], pose[:, 2], fc.RACE_A, fc.RACE_B)
    assert rc._engine.cost_grid_footprint_at(pose)[0] == pytest.approx(want[0], abs=1e-4)
    rc.cost_grid = rs["grid"].kwargs  # no key: the default, "centre"
    assert rc._engine.cost_grid_footprint == "centre" and rc.cost_grid["footprint"] == "centre"
    plain = pkg.MPPIRacecarController(**kw, cost_grid=rs["grid"].kwargs)
    plain._engine.set_state(rs["x0"])
    plain._engine.run_closed_loop(1)
    assert plain._engine.cost_grid_footprint == "centre" and plain._engine.rollout_kernel().endswith(", 6, false>")
    ds = fc.diff_scene(50, False)
    dkw = dict(mc.DIFF_KW, ref_path=ds["ref"], num_samples_K=64, num_horizons_T=50)
    with pytest.raises(pkg.MppiError) as ex:  # the diff-drive controller tests a disc
        pkg.MPPIAlgorithms(**dkw, cost_grid=dict(ds["grid"].kwargs, footprint="outline"))
    assert ex.value.code == capi.ERR_UNSUPPORTED and "radius" in str(ex.value)
    with pytest.raises(pkg.MppiError):
        pkg.MPPIRacecarController(**kw, cost_grid=dict(rs["grid"].kwargs, footprint="box"))
