"""Cost grids on the device (mppi_set_cost_grid): the grid's value against the f64 formula, the hit and the cost of
single states, one iteration against the f64 reference of tests/cost_grid_checks.py in every CPU case, the bit-for-bit
statements (never called / cleared, graph replay, batches, the shared grid), a closed loop with a same-shape re-upload, and the
refusals.  K = 256; every reference is computed once per case and shared by the f32 and the f64 handle."""
import functools

import numpy as np
import pytest

import cost_grid_checks as gc
import moving_obstacle_checks as mc
from test_gpu_agent_scenes import compare, diff_cfg, race_cfg
from test_gpu_moving_obstacles import cuda, diff_engine, prec, race_engine

pytestmark = pytest.mark.gpu

K = gc.K_CASE


def spec_of(e):
    return e.rollout_kernel().split(", ")[4]


def load(e, sc, grid=True):
    e.set_ref_path(sc["ref"])
    e.set_obstacles(sc["circles"], velocities=sc["vel"])
    e.set_u_prev(sc["u"])
    if grid:
        e.set_cost_grid(**sc["grid"].kwargs)
    return e


def rounded(a, precision):
    return np.asarray(a, np.float32).astype(np.float64) if precision == "f32" else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------ 1. the value
SHAPES = [(2, 2), (3, 7), (7, 3), (33, 17), (64, 64), (300, 200)]  # (nx, ny)


def value_points(nx, ny, origin, res, rng):
    """nodes, mid-cell points, points on edges between nodes, random points inside, and points far outside (finite)"""
    ix, iy = rng.integers(0, nx, 64), rng.integers(0, ny, 64)
    nodes = np.stack([origin[0] + res * ix, origin[1] + res * iy], axis=1)
    jx, jy = rng.integers(0, nx - 1, 64), rng.integers(0, ny - 1, 64)
    mid = np.stack([origin[0] + res * (jx + 0.5), origin[1] + res * (jy + 0.5)], axis=1)
    edge = np.stack([origin[0] + res * (jx + 0.5), origin[1] + res * iy], axis=1)
    inside = np.stack([origin[0] + res * rng.uniform(0, nx - 1, 64), origin[1] + res * rng.uniform(0, ny - 1, 64)], axis=1)
    span = res * max(nx, ny)
    far = np.concatenate([np.stack([origin[0] + rng.uniform(-2, 3, 32) * span, origin[1] + rng.uniform(-2, 3, 32) * span], axis=1),
                          [[1e6, 1e6], [-1e6, 1e6], [1e6, -1e6], [-1e6, -1e6], [origin[0] + res, -1e6], [1e6, origin[1] + res]]])
    return nodes, (ix < nx - 1) & (iy < ny - 1), np.concatenate([mid, edge, inside, far])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_value_against_the_formula(precision):
    """Every shape on one handle: a reshape each time, and a same-shape re-upload of other cells in between."""
    e = diff_engine(50, "frozen", False, precision)
    e.set_ref_path(mc.diff_scene(50, False)["ref"])
    rng = np.random.default_rng(5)
    origin, res = (-1.5, 0.75), 0.25  # (exact in f32, and so are the nodes' coordinates)
    for nx, ny in SHAPES:
        for upload in range(2):  # the second: the same shape again
            cells = rounded(rng.uniform(-1.0, 2.0, (ny, nx)), "f32")
            e.set_cost_grid(cells, origin, res)
            nodes, inner, other = value_points(nx, ny, origin, res, rng)
            got = e.cost_grid_at(nodes)
            R = np.float32 if precision == "f32" else np.float64
            want = gc.grid_value(cells, origin, res, nodes[:, 0], nodes[:, 1], dtype=R)
            np.testing.assert_array_equal(got, want)  # the formula in the handle's precision, bit for bit: fractions 0 and 1
            # a node returns its cell exactly (the last node of an axis: a + (b - a), the cell to one rounding of the difference)
            at = gc.grid_value(cells, origin, res, nodes[:, 0], nodes[:, 1])
            np.testing.assert_array_equal(got[inner], at[inner])
            np.testing.assert_allclose(got, at, rtol=0, atol=4e-7 if precision == "f32" else 1e-15)
            got = e.cost_grid_at(other)
            want = gc.grid_value(cells, origin, res, rounded(other[:, 0], precision), rounded(other[:, 1], precision))
            # f32: the fraction carries half an ulp of the node coordinate (<= 2^-24 * 300), each fma half an ulp of a value <= 2,
            # the cell differences reach 3: 3 * 2 * 1.8e-5 + 3 * 1.2e-7 < 1.2e-4.  f64: the same with 2^-53
            np.testing.assert_allclose(got, want, rtol=0, atol=1.2e-4 if precision == "f32" else 1e-12)
            edge_nodes = [cells[-1, -1], cells[-1, 0], cells[0, -1], cells[0, 0], cells[0, 1], cells[1, -1]]  # far outside: the edge continues
            np.testing.assert_allclose(got[-6:], edge_nodes, rtol=0, atol=4e-7 if precision == "f32" else 1e-15)
            assert got[-3] == cells[0, 0]


# ------------------------------------------------------------------------------------------ 2. hit and cost of single states
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("circles", [0, 2])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_hit_and_cost_either_side_of_the_lethal_contour(model, circles, precision):
    """Points 1e-3 m either side of the contour g = lethal along the wall, at clock 2; with 2 circles some points are hit by a
    circle alone.  A ramp grid g = x - ox makes the contour a line: x = ox + lethal."""
    T = 50 if model == "diff" else mc.RACE_T
    sc = gc.diff_scene(T, True, circles=circles) if model == "diff" else gc.race_scene(circles=circles)
    nx, ny, res = 64, 48, 0.5
    origin = (float(np.floor(sc["x0"][0]) - 2.0), float(np.floor(sc["x0"][1]) - 12.0))  # (the contour: 6.25 m right of the start, the
    lethal, weight = 8.25, 4.0                                                          # circles on its clear side)
    cells = np.broadcast_to(res * np.arange(nx, dtype=np.float64), (ny, nx)).copy()
    sc = dict(sc, grid=gc.Grid(cells, origin, res, weight, lethal))
    e = load(diff_engine(T, "frozen", True, precision) if model == "diff" else race_engine(precision), sc)
    e.set_state(sc["x0"])
    e.run_closed_loop(2)
    o = (gc.diff_oracle(sc, 1, T) if model == "diff" else gc.race_oracle(sc, 1))
    o.set_motion(sc["vel"], 2)
    rng = np.random.default_rng(3)
    n = 128
    poses = np.zeros((n, e.nx))
    side = np.where(np.arange(n) % 2 == 0, 1e-3, -1e-3)
    poses[:, 0] = origin[0] + lethal + side
    poses[:, 1] = origin[1] + rng.uniform(-2.0, res * ny + 2.0, n)
    poses[:, 2] = rng.uniform(-np.pi, np.pi, n)
    if circles:  # eight poses on the clear side of the contour that touch circle 0 where it stands at clock 2 (the race car: with
        at = mc.centres(sc["circles"], sc["vel"], float(o.delta_t), 2, 0)[0]  # its front outline point, 3 m ahead at yaw 0)
        poses[:8, :2] = at + rng.normal(0, 0.05, (8, 2)) - ([0.0, 0.0] if model == "diff" else [3.0, 0.0])
        poses[:8, 2] = 0.0
        assert poses[:8, 0].max() < origin[0] + lethal - 0.5
    steps = np.zeros(n, np.int32)
    want = o.is_hit(poses[:, 0], poses[:, 1], steps=steps) if model == "diff" else o.is_hit(poses[:, 0], poses[:, 1], poses[:, 2], steps=steps)
    outside = o.sample_margin() > gc.MARGIN
    got = e.eval_is_collided(poses) > 0
    g = sc["grid"].value(poses[:, 0], poses[:, 1])
    print(model, circles, precision, "hit", want.mean(), "outside the margin", outside.mean(), "by a circle alone", int((want & (g < lethal)).sum()))
    assert 0.3 < want.mean() < 0.7 and outside.mean() > 0.95
    assert np.array_equal(got[outside], want[outside])
    assert np.array_equal(e.eval_is_collided(poses, steps=steps)[outside] > 0, want[outside])
    assert int((want & (g < lethal)).sum()) >= 8 if circles else not (want & (g < lethal)).any()
    # the cost: the handle's cost without the grid + the penalty where the grid alone is lethal + weight g
    plain = load(diff_engine(T, "frozen", True, precision) if model == "diff" else race_engine(precision), sc, grid=False)
    plain.set_state(sc["x0"])
    plain.run_closed_loop(2)
    for terminal in (False, True):
        c_grid, idx, _ = e.eval_cost(poses, terminal=terminal, prev_idx=0)
        c_plain, idx2, _ = plain.eval_cost(poses, terminal=terminal, prev_idx=0)
        hit_plain = plain.eval_is_collided(poses) > 0
        expect = c_plain + np.where(got & ~hit_plain, 1e10, 0.0) + weight * g
        assert np.array_equal(idx, idx2)
        np.testing.assert_allclose(c_grid[outside], expect[outside], rtol=1e-12 if precision == "f64" else 2e-6, atol=0)


# ------------------------------------------------------------------------------------------ 3. one iteration
@functools.lru_cache(maxsize=None)
def diff_reference(T, accumulate, mode, grid, K=K, circles=2):
    return gc.diff_case(T, accumulate, mode, grid, K=K, circles=circles)


@functools.lru_cache(maxsize=None)
def race_reference():
    return gc.race_case()


def check_iteration(e, sc, eps, o, res, precision, sequential=False, f32_reference=False):
    """One iteration with injected noise against the reference: the tolerances and the margin rule of
    test_gpu_moving_obstacles.py (S: rtol = atol = 1e-10 in f64, 2e-4 in f32 on the samples kept; u as there)."""
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = gc.kept(o, precision == "f64" and not f32_reference)
    hit_ref = gc.penalised(S_ref)
    err_u = float(np.sqrt(np.mean((u - res["u_returned"]) ** 2)))
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "max rel S err", float(np.max(np.abs(S[keep] - S_ref[keep]) / np.maximum(np.abs(S_ref[keep]), 1.0))))
    assert keep.mean() >= 1.0 - gc.MAX_LEFT_OUT
    assert np.array_equal(gc.penalised(S)[keep], hit_ref[keep])  # no flip outside the margin
    assert st.n_collided == int((S >= 1.0e10).sum())
    if precision == "f64" and not f32_reference:
        np.testing.assert_allclose(S, S_ref, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == int((S_ref >= 1.0e10).sum())
    else:
        np.testing.assert_allclose(S[keep], S_ref[keep], rtol=2e-4, atol=2e-4)
        assert err_u <= 1e-4
    if sequential:
        assert st.rounds >= 1 and st.idx_after == res["idx_after"] and res["idx_after"] > res["idx_start"]
    name = e.rollout_kernel()
    assert name.startswith("k_rollout_fused<") and name.endswith(", 6, false>"), name
    return st


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode,grid", gc.diff_cases())
def test_diff_iteration_against_the_reference(T, accumulate, mode, grid, precision):
    sc, eps, o, res = diff_reference(T, accumulate, mode, grid)
    e = load(diff_engine(T, mode, accumulate, precision), sc)
    check_iteration(e, sc, eps, o, res, precision, sequential=mode == "sequential")
    assert e.rollout_kernel().split(", ")[2] == ("1" if T <= 64 else "2")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_a_ragged_last_workgroup(precision):
    sc, eps, o, res = diff_reference(50, True, "frozen", "64x64", K=250)
    e = load(diff_engine(50, "frozen", True, precision, K=250), sc)
    check_iteration(e, sc, eps, o, res, precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_iteration_against_the_reference(precision):
    sc, eps, o, res = race_reference()
    e = load(race_engine(precision), sc)
    check_iteration(e, sc, eps, o, res, precision, f32_reference=True)  # (the reference itself is f32)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_a_grid_and_no_circles_counts_its_hits(accumulate, precision):
    sc, eps, o, res = diff_reference(50, accumulate, "frozen", "64x64", circles=0)
    e = load(diff_engine(50, "frozen", accumulate, precision), sc)
    st = check_iteration(e, sc, eps, o, res, precision)
    n_ref = int(gc.penalised(res["S"]).sum())
    assert n_ref == int(o.sample_grid_lethal().sum()) and K // 16 <= n_ref <= K - K // 16
    assert abs(st.n_collided - n_ref) <= int((~gc.kept(o, precision == "f64")).sum())


# ------------------------------------------------------------------------------------------ 4. bit for bit
def state_of(e):
    return e.get_u_prev(), e.get_state(), e.costs(), int(e.stats.n_collided)


def assert_same(a, b):
    for x, y in zip(state_of(a), state_of(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_never_called_and_cleared_are_the_same_handle(precision):
    T = 50
    sc = gc.diff_scene(T, True)
    never = load(diff_engine(T, "frozen", True, precision, seed=3), sc, grid=False)
    cleared = load(diff_engine(T, "frozen", True, precision, seed=3), sc, grid=False)
    late = load(diff_engine(T, "frozen", True, precision, seed=3), sc)
    cleared.set_cost_grid(None)  # (nothing to remove)
    for h in (never, cleared, late):
        h.set_state(sc["x0"])
        h.run_closed_loop(2)
    assert spec_of(never) == "3" and spec_of(cleared) == "3" and spec_of(late) == "6"
    assert_same(never, cleared)
    assert not np.array_equal(never.costs(), late.costs())  # the grid matters on this scene
    late.set_cost_grid(None)  # cleared in mid-run: from here on the same iterations again
    for h in (never, late):
        h.set_u_prev(sc["u"])
        h.set_state(sc["x0"])
        h.set_iteration(7)
        h.run_closed_loop(2)
    assert spec_of(late) == "3"
    assert_same(never, late)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_replay_equals_eager_across_a_same_shape_upload(monkeypatch, precision):
    T, n_it = 50, 3
    sc = gc.diff_scene(T, True)
    shifted = dict(sc["grid"].kwargs, cells=np.roll(sc["grid"].cells, 1, axis=1))

    def run(e):
        e.set_state(sc["x0"])
        e.run_closed_loop(n_it)
        e.set_cost_grid(**shifted)  # the same shape: buffers, plan and a cached graph stay
        e.run_closed_loop(n_it)
        return e
    eager = load(diff_engine(T, "frozen", True, precision, seed=31), sc)
    eager.set_state(sc["x0"])
    for _ in range(n_it):
        eager.run_closed_loop(1)
    eager.set_cost_grid(**shifted)
    for _ in range(n_it):
        eager.run_closed_loop(1)
    once = run(load(diff_engine(T, "frozen", True, precision, seed=31), sc))
    assert_same(eager, once)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = run(load(diff_engine(T, "frozen", True, precision, seed=31), sc))
    assert_same(eager, graph)
    assert spec_of(graph) == "6" and eager.stats.n_collided > 0
    unshifted = load(diff_engine(T, "frozen", True, precision, seed=31), sc)
    unshifted.set_state(sc["x0"])
    unshifted.run_closed_loop(2 * n_it)
    assert not np.array_equal(unshifted.costs(), graph.costs())  # the re-upload was seen


def small_grid(sc):
    """an own grid of another shape, weight and lethal: 33 x 17 nodes of 0.25 m over the end of the nominal rollout"""
    g = sc["grid"]
    x0 = sc["x0"]
    end = x0[:2] + mc.TRAVEL * np.array([np.cos(x0[2]), np.sin(x0[2])])
    origin = tuple(np.floor(end) - (4.0, 2.0))
    cells = gc.wall_cells(*gc.diff_wall(sc), 0.9, origin, 0.25, 33, 17)
    return gc.Grid(cells, origin, 0.25, 0.5, 0.25)


@pytest.mark.parametrize("model,precision", [("diff", "f64"), ("diff", "f32"), ("race", "f32")])
def test_agents_with_own_grids_equal_single_handles(model, precision):
    """Three agents: the case grid (64 x 64) with the own circles; an own 33 x 17 grid of other weight and lethal and no circles;
    no grid.  Bit for bit against single-agent handles."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if model == "diff":
        T, sc = 50, gc.diff_scene(50, True)
        cfg = dict(diff_cfg(capi.WAYPOINT_FROZEN, T, precision=prec(precision)), obstacle_motion=1, accumulate_stage_cost=1)
        own = small_grid(sc)
    else:
        T, sc = mc.RACE_T, gc.race_scene()
        cfg = dict(race_cfg(), precision=prec(precision), obstacle_motion=1)
        g = sc["grid"]
        own = gc.Grid(g.cells[12:29, 16:49] * 0.5, (g.origin[0] + 8.0, g.origin[1] + 6.0), 0.5, 32.0, 0.09375)  # (33 x 17 around the car)
    grids = [sc["grid"], own, None]
    none = (np.zeros((0, 3)), np.zeros((0, 2)))
    circles = [(sc["circles"], sc["vel"]), none, (sc["circles"], sc["vel"])]
    rng = np.random.default_rng(11)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(3)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(3)])
    batch = pkg.Engine(K=K, n_agents=3, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(3)]
    batch.set_ref_path(sc["ref"])
    batch.set_state(x0)
    batch.set_u_prev(u)
    for a, one in enumerate(singles):
        one.set_ref_path(sc["ref"])
        one.set_state(x0[a])
        one.set_u_prev(u[a])
        one.set_obstacles(circles[a][0], velocities=circles[a][1])
        batch.set_obstacles(circles[a][0], agent=a, velocities=circles[a][1])
        if grids[a] is not None:
            one.set_cost_grid(**grids[a].kwargs)
            batch.set_cost_grid(**grids[a].kwargs, agent=a)
    hits = []
    for n_run in (1, 3):
        batch.run_closed_loop(n_run)
        for one in singles:
            one.run_closed_loop(n_run)
        compare(batch, singles, None)
        hits.append([int(one.stats.n_collided) for one in singles])
    pts = np.stack([sc["x0"][:2] + [0.3 * i, -0.2 * i] for i in range(8)])
    for a in range(2):
        np.testing.assert_array_equal(batch.cost_grid_at(pts, agent=a), singles[a].cost_grid_at(pts))
    with pytest.raises(pkg.MppiError) as ex:
        batch.cost_grid_at(pts, agent=2)
    assert ex.value.code == capi.ERR_STATE
    print(model, precision, "n_collided per agent and stretch", hits, batch.rollout_kernel())
    assert hits[0][1] > 0  # (agent 1: a grid and no circles counts its hits)
    assert ", true, 6, " in batch.rollout_kernel() and ", false, 6, " in singles[1].rollout_kernel()
    assert ", false, 3, " in singles[2].rollout_kernel()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_shared_grid_its_replacement_and_the_return_to_it(monkeypatch, graph):
    """The plain setter gives every agent of a batch the same grid; one agent gets its own in between, then none, then the
    shared grid again for both: every stretch equals single handles driven the same way."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if graph == "1":
        monkeypatch.setenv("MPPI_GRAPH", "1")
    T = 50
    sc = gc.diff_scene(T, True)
    cfg = dict(diff_cfg(capi.WAYPOINT_FROZEN, T), obstacle_motion=1, accumulate_stage_cost=1)
    rng = np.random.default_rng(13)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(2)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(2)])
    batch = pkg.Engine(K=K, n_agents=2, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(2)]
    for e, xs, us in [(batch, x0, u)] + [(singles[a], x0[a], u[a]) for a in range(2)]:
        e.set_ref_path(sc["ref"])
        e.set_cost_grid(**sc["grid"].kwargs)
        e.set_state(xs)
        e.set_u_prev(us)

    def run(n):
        for e in [batch] + singles:
            e.run_closed_loop(n)
        compare(batch, singles, None)
        return [int(one.stats.n_collided) for one in singles]
    first = run(3)
    own = small_grid(sc)
    batch.set_cost_grid(**own.kwargs, agent=1)
    singles[1].set_cost_grid(**own.kwargs)
    run(3)
    batch.set_cost_grid(None, agent=1)  # an own "none": agent 1 collides with nothing
    singles[1].set_cost_grid(None)
    assert run(2)[1] == 0 and spec_of(singles[1]) == "3" and spec_of(batch) == "6"
    for e in [batch] + singles:
        e.set_cost_grid(**sc["grid"].kwargs)  # back to the shared grid for both
    last = run(2)
    assert batch.stats.iteration == 10 and min(first) > 0 and max(last) > 0


# ------------------------------------------------------------------------------------------ 5. the closed loop
LOOP_T, LOOP_N, LOOP_SWAP = 50, 6, 3
LOOP_W = dict(stage_cost_weight=[0.25, 0.25, 0.5, 0], terminal_cost_weight=[0.25, 0.25, 0.5, 0])


def loop_grids():
    g = gc.diff_scene(LOOP_T, True)["grid"]
    moved = gc.Grid(np.roll(g.cells, 1, axis=1), g.origin, g.resolution, g.weight, g.lethal)  # the wall shifted by one cell
    return g, moved


@functools.lru_cache(maxsize=None)
def loop_reference():
    """The reference loop on the noise the device's sampler draws (mppi_sample_epsilon: bit for bit what the kernels draw)."""
    e = diff_engine(LOOP_T, "frozen", True, "f32", seed=31, **LOOP_W)
    ring = [e.sample_epsilon(i).cpu().numpy() for i in range(LOOP_N)]
    e.close()
    g, moved = loop_grids()
    return gc.diff_closed_loop(LOOP_T, LOOP_N, lambda i: g if i < LOOP_SWAP else moved, accumulate=True, eps_of=lambda i: ring[i])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_closed_loop_with_a_same_shape_re_upload(precision):
    """Six iterations, the wall shifted by one cell between the third and the fourth.  f64: end to end.  f32: re-seeded with
    the reference's state and controls before every iteration (one-iteration bounds)."""
    ref = loop_reference()
    sc = ref["scene"]
    g, moved = loop_grids()
    assert min(ref["kept"]) >= 1.0 - gc.MAX_LEFT_OUT and min(ref["n_hit"]) > 0
    assert abs(ref["n_hit"][LOOP_SWAP] - ref["n_hit"][LOOP_SWAP - 1]) > K // 32  # the shift shows
    e = load(diff_engine(LOOP_T, "frozen", True, precision, seed=31, **LOOP_W), sc)
    e.set_state(sc["x0"])
    if precision == "f64":
        t1, _ = e.run_closed_loop(LOOP_SWAP, trace=True)
        e.set_cost_grid(**moved.kwargs)
        t2, st = e.run_closed_loop(LOOP_N - LOOP_SWAP, trace=True)
        trace = np.concatenate([t1, t2])
        print("reference hits per iteration", ref["n_hit"], "last n_collided", st.n_collided)
        np.testing.assert_allclose(trace, ref["u0"], rtol=1e-8, atol=1e-10)
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
    assert st.iteration == LOOP_N and spec_of(e) == "6"


# ------------------------------------------------------------------------------------------ 6. interfaces
def test_refusals_name_the_limit_and_change_nothing():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = gc.diff_scene(T, True)
    e = load(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    twin = load(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    good = dict(sc["grid"].kwargs, cells=sc["grid"].cells + 0.25)

    def refused(code, word=None, target=None, **kw):
        with pytest.raises(pkg.MppiError) as ex:
            (target or e).set_cost_grid(**dict(good, **kw))
        assert ex.value.code == code, str(ex.value)
        assert word is None or word in str(ex.value), str(ex.value)
    bad = good["cells"].copy()
    bad[3, 7] = np.nan
    refused(capi.ERR_BAD_ARG, "finite", cells=bad)
    bad[3, 7] = np.inf
    refused(capi.ERR_BAD_ARG, cells=bad)
    refused(capi.ERR_BAD_ARG, "4096", cells=np.zeros((2, 4097)))
    refused(capi.ERR_BAD_ARG, "[2,", cells=np.zeros((1, 8)))
    refused(capi.ERR_BAD_ARG, "origin", origin=(np.nan, 0.0))
    refused(capi.ERR_BAD_ARG, "origin", origin=(0.0, np.inf))
    for r in (0.0, -0.5, np.nan, np.inf):
        refused(capi.ERR_BAD_ARG, "resolution", resolution=r)
    for w in (-1.0, np.nan, np.inf):
        refused(capi.ERR_BAD_ARG, "weight", weight=w)
    for v in (0.0, -1.0, np.nan):
        refused(capi.ERR_BAD_ARG, "lethal", lethal=v)
    refused(capi.ERR_BAD_ARG, "agent", agent=1)
    refused(capi.ERR_BAD_ARG, "agent", agent=-1)
    pts = np.stack([sc["x0"][:2] + [0.3 * i, -0.2 * i] for i in range(8)])
    with pytest.raises(pkg.MppiError) as ex:
        e.cost_grid_at(pts, agent=1)
    assert ex.value.code == capi.ERR_BAD_ARG
    np.testing.assert_array_equal(e.cost_grid_at(pts), twin.cost_grid_at(pts))
    # tracks and a grid exclude each other, both ways
    with pytest.raises(pkg.MppiError) as ex:
        e.set_obstacle_tracks(np.zeros((1, 4, 2)), [0.3])
    assert ex.value.code == capi.ERR_STATE and "cost grid" in str(ex.value)
    for h in (e, twin):
        h.set_state(sc["x0"])
        h.run_closed_loop(3)
    assert e.stats.n_collided > 0 and spec_of(e) == "6"
    assert_same(e, twin)
    tracked = load(diff_engine(T, "frozen", True, "f64"), sc, grid=False)
    tracked.set_obstacle_tracks(np.zeros((1, 4, 2)), [0.3])
    refused(capi.ERR_STATE, "obstacle tracks", target=tracked)
    # lethal = +inf is accepted: soft cost only
    soft = load(diff_engine(T, "frozen", True, "f64", seed=3), dict(sc, circles=np.zeros((0, 3)), vel=np.zeros((0, 2))), grid=False)
    soft.set_cost_grid(**dict(sc["grid"].kwargs, lethal=np.inf))
    soft.set_state(sc["x0"])
    soft.run_closed_loop(1)
    assert soft.stats.n_collided == 0 and spec_of(soft) == "6"
    # handles that take no grid
    static = diff_engine(T, "frozen", True, "f64", obstacle_motion=0)
    refused(capi.ERR_STATE, "obstacle_motion", target=static)
    refused(capi.ERR_STATE, "obstacle_motion", target=static, agent=0)
    fleet = pkg.Engine(K=K, n_agents=2, **dict(diff_cfg(capi.WAYPOINT_FROZEN, T), obstacle_motion=1, fleet_radius=0.3))
    refused(capi.ERR_UNSUPPORTED, "fleet_radius", target=fleet)
    long = diff_engine(130, "frozen", True, "f64")
    refused(capi.ERR_UNSUPPORTED, "T <= 128", target=long)


def test_controller_keyword_switches_motion_on():
    """`cost_grid` on the controllers: last keyword, settable property; a controller built without it refuses."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc, eps, o, res = diff_reference(T, False, "frozen", "64x64", circles=0)
    kw = dict(mc.DIFF_KW, ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T)
    c = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", cost_grid=sc["grid"].kwargs)
    assert c._engine.cfg.obstacle_motion == 1 and c._engine.cfg.obstacle_model == capi.OBSTACLE_CIRCLE
    assert np.array_equal(c.cost_grid["cells"], sc["grid"].cells)
    c.u_prev[:] = sc["u"]
    c._calc_epsilon = lambda *a, **k: cuda(eps)
    _, u, _, _ = c._calc_input_control(sc["x0"])
    np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
    c.cost_grid = None  # settable, like obstacle_circles
    assert c.cost_grid is None
    with pytest.raises(pkg.MppiError):
        c._engine.cost_grid_at(np.zeros((1, 2)))
    plain = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", obstacle_circles=mc.diff_scene(T, False)["circles"])
    assert plain.cost_grid is None
    with pytest.raises(pkg.MppiError) as ex:
        plain.cost_grid = sc["grid"].kwargs
    assert ex.value.code == capi.ERR_STATE and "obstacle_motion" in str(ex.value)
    rs = gc.race_scene()
    rc = pkg.MPPIRacecarController(ref_path=rs["ref"], horizon_step_T=mc.RACE_T, number_of_samples_K=64, cost_grid=rs["grid"].kwargs)
    assert rc._engine.cfg.obstacle_motion == 1 and rc._engine.cfg.obstacle_model == capi.OBSTACLE_OUTLINE
    assert rc._engine.cost_grid_at(rs["x0"][None, :2])[0] == pytest.approx(rs["grid"].value(rs["x0"][0], rs["x0"][1]), abs=1e-5)
