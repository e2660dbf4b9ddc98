"""Obstacle tracks on the device (mppi_set_obstacle_tracks): the readback, the collision test at a step of the
tracks' clock, one iteration against the f64 reference of tests/obstacle_track_checks.py on every track form, what must stay bit
for bit, the clock through a closed loop that runs past the end of the tracks, and the refusals.  K = 256 throughout; every
reference is computed once per case and shared by the f32 and the f64 handle."""
import functools

import numpy as np
import pytest

import moving_obstacle_checks as mc
import obstacle_track_checks as tc
from test_gpu_agent_scenes import compare, diff_cfg, race_cfg
from test_gpu_moving_obstacles import cuda, diff_engine, prec, race_engine

pytestmark = pytest.mark.gpu

K = tc.K_CASE


def rounded(a, precision):
    a = np.asarray(a, np.float64)
    return a if precision == "f64" else a.astype(np.float32).astype(np.float64)


def load(e, sc, clock=0):
    """The scene's path, own circles (moving) and tracks; `clock` iterations later, with state, controls and index as given."""
    e.set_ref_path(sc["ref"])
    if len(sc["circles"]):
        e.set_obstacles(sc["circles"], velocities=sc["vel"])
    e.set_obstacle_tracks(sc["tracks"], sc["radii"])
    if clock:
        e.set_state(sc["x0"])
        e.run_closed_loop(clock)
        e.set_waypoint_idx(0)
        e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    return e


def spec_of(e):
    name = e.rollout_kernel()
    assert name.startswith("k_rollout_fused<"), name
    return name.split(", ")[4]


@functools.lru_cache(maxsize=None)
def diff_reference(T, accumulate, mode):
    return tc.diff_case(T, accumulate, mode)


@functools.lru_cache(maxsize=None)
def race_reference():
    return tc.race_case()


def check_iteration(e, sc, eps, o, res, precision, sequential=False):
    """One iteration with injected noise against the reference: test_gpu_moving_obstacles.check_iteration restated (the
    tolerances of DESIGN section 5, the margin rule of tests/prims_checks.py)."""
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = tc.kept(o, precision == "f64")
    hit_ref = tc.penalised(S_ref)
    err_u = float(np.sqrt(np.mean((u - res["u_returned"]) ** 2)))
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "max rel S err", float(np.max(np.abs(S[keep] - S_ref[keep]) / np.maximum(np.abs(S_ref[keep]), 1.0))))
    assert keep.mean() >= 1.0 - tc.MAX_LEFT_OUT
    assert np.array_equal(tc.penalised(S)[keep], hit_ref[keep])  # no flip outside the margin
    assert int(tc.penalised(S)[keep].sum()) == int(hit_ref[keep].sum())
    sure = S_ref >= 1.0e10 + 1.0e4  # (f32: 1e10 has an ulp of 1024)
    unsure = (np.abs(S_ref - 1.0e10) < 1.0e4) | (~keep & ~sure)
    if precision == "f64" and keep.all():
        assert st.n_collided == int((S_ref >= 1.0e10).sum())
    else:
        assert int((sure & keep).sum()) <= st.n_collided <= int((sure | unsure).sum())
    assert st.n_collided == int((S >= 1.0e10).sum())
    if precision == "f64":
        np.testing.assert_allclose(S, S_ref, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
    else:
        np.testing.assert_allclose(S[keep], S_ref[keep], rtol=2e-4, atol=2e-4)
        assert err_u <= 1e-4
    if sequential:
        assert st.rounds >= 1 and st.idx_after == res["idx_after"] and res["idx_after"] > res["idx_start"]
    return st


# ------------------------------------------------------------------------------------------ 1. readback
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_readback_follows_the_clock(n, precision):
    T = 50
    sc = mc.diff_scene(T, False)
    e = diff_engine(T, "frozen", False, precision)
    e.set_ref_path(sc["ref"])
    e.set_state(sc["x0"])
    rng = np.random.default_rng(n)
    steps = (0, 1, 2, T // 2, T, T + 2, T + 3, T + 9, 70000)
    for L in (1, T + 1, T + 4):
        xy = rng.normal(0, 30.0, (n, L, 2))
        radii = rng.uniform(0.0, 2.0, n)
        want = rounded(xy, precision)

        def check(clock):
            for s in steps:
                got = e.obstacle_tracks_at(s)
                assert got.shape == (n, 3)
                assert np.array_equal(got[:, :2], want[:, min(clock + s, L - 1)]), (L, clock, s)
                assert np.array_equal(got[:, 2], radii)  # bit for bit what was given
        e.set_obstacle_tracks(xy, radii)
        check(0)
        e.run_closed_loop(3)
        check(3)
        e.set_iteration(1000)  # replays noise; the clock does not move
        check(3)
        e.run_closed_loop(1)
        assert e.stats.iteration == 1001
        check(4)
        e.set_obstacle_tracks(xy, radii)  # a fresh upload re-bases it
        check(0)
    e.set_obstacle_tracks(np.zeros((0, 1, 2)), [])
    assert e.obstacle_tracks_at(0).shape == (0, 3)


# ------------------------------------------------------------------------------------------ 2. the collision test at a step
def eval_engine(model, obstacle, precision):
    from dnn_mppi_mpc_amd import _capi as capi
    if model == "diff":
        kw = dict(obstacle_model=capi.OBSTACLE_CIRCLE) if obstacle == "circle" else dict(obstacle_model=capi.OBSTACLE_OUTLINE, vehicle_w=3.0, vehicle_l=4.0, safety_margin=1.5)
        return diff_engine(50, "frozen", True, precision, **kw)
    kw = dict(obstacle_model=capi.OBSTACLE_CIRCLE if obstacle == "circle" else capi.OBSTACLE_OUTLINE)
    return race_engine(precision, **kw)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("own", [0, 2])
@pytest.mark.parametrize("obstacle", ["circle", "outline"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_collision_test_at_a_step_of_the_tracks(model, obstacle, own, precision):
    """Poses 1e-3 inside and outside the threshold of a track's point at steps 0, 1, T / 2, T and beyond the end (the held
    point), at clock 2.  Successive points lie decimetres apart, so a wrong index decides the inside poses wrongly."""
    CLK, DELTA = 2, 1.0e-3
    sc = mc.diff_scene(50, True) if model == "diff" else mc.race_scene()
    e = eval_engine(model, obstacle, precision)
    T = e.T
    L = T + 4
    cfg = e.cfg
    rng = np.random.default_rng(17)
    n = 3
    xy = np.cumsum(rng.normal(0, 0.3, (n, L, 2)), axis=1) + np.array([[40.0 * m, -25.0 * m] for m in range(n)])[:, None, :]
    radii = np.array([0.4, 1.0, 0.7])
    e.set_ref_path(sc["ref"])
    own_c, own_v = sc["circles"][:own] + [200.0, 200.0, 0.0], sc["vel"][:own]
    if own:
        e.set_obstacles(own_c, velocities=own_v)
    e.set_obstacle_tracks(xy, radii)
    e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    e.run_closed_loop(CLK)
    pts = rounded(xy, precision)
    steps_of = (0, 1, T // 2, T, L + 5)
    margin = float(cfg.safety_margin)
    vl, vw = float(cfg.vehicle_l) * margin, float(cfg.vehicle_w) * margin
    poses, steps, want = [], [], []
    for m in range(n):
        for s in steps_of:
            C = pts[m, min(CLK + s, L - 1)]
            for inside in (True, False):
                th = rng.uniform(-np.pi, np.pi)
                if obstacle == "circle":
                    d = (0.5 * margin + radii[m]) + (-DELTA if inside else DELTA)
                    offs = [d * np.array([np.cos(th), np.sin(th)])]
                else:  # the nearest outline point a corner / the middle of the front, the centre straight out from it
                    d = radii[m] + (-DELTA if inside else DELTA)
                    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
                    offs = [rot @ (np.array([0.5 * vl, 0.5 * vw]) + d * np.array([1.0, 1.0]) / np.sqrt(2.0)),
                            rot @ (np.array([0.5 * vl, 0.0]) + d * np.array([1.0, 0.0]))]
                for off in offs:
                    p = np.zeros(e.nx)
                    p[:2], p[2] = C - off, th
                    poses.append(p)
                    steps.append(s)
                    want.append(inside)
    poses, steps, want = np.array(poses), np.array(steps, dtype=np.int32), np.array(want)
    got = e.eval_is_collided(poses, steps=steps) > 0
    print(model, obstacle, own, precision, "poses", len(poses), "flips", int((got != want).sum()))
    assert np.array_equal(got, want)
    now = e.eval_is_collided(poses) > 0  # the existing entry prices step 0 of the current clock
    assert np.array_equal(now[steps == 0], want[steps == 0])
    if own:  # the own moving circles are priced beside the tracks: a pose that touches circle 0 at a step of ITS clock (the
        # outline model: with the middle of its front on the centre, yaw 0)
        at = mc.centres(own_c, own_v, float(cfg.delta_t), CLK, np.array([0, T]))[:, 0]
        q = np.zeros((2, e.nx))
        q[:, :2] = at - ([0.5 * vl, 0.0] if obstacle == "outline" else [0.0, 0.0])
        assert (e.eval_is_collided(q, steps=np.array([0, T], dtype=np.int32)) > 0).all()
        assert not (e.eval_is_collided(q, steps=np.array([T, 0], dtype=np.int32)) > 0).any()


# ------------------------------------------------------------------------------------------ 3. one iteration
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode", tc.diff_cases())
def test_diff_iteration_against_the_reference(T, accumulate, mode, precision):
    """Tracks and no circles, three control steps after the upload.  (check_iteration holds mppi_stats.n_collided of the f64
    handle to the reference's penalised samples.)"""
    sc, eps, o, res = diff_reference(T, accumulate, mode)
    e = load(diff_engine(T, mode, accumulate, precision), sc, tc.CLOCK)
    st = check_iteration(e, sc, eps, o, res, precision, sequential=mode == "sequential")
    if precision == "f64":
        assert st.n_collided == int(tc.penalised(res["S"]).sum()) > 0
    name = e.rollout_kernel()
    assert spec_of(e) == "5" and name.split(", ")[2] == ("1" if T <= 64 else "2") and name.split(", ")[3] == "false", name


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_iteration_against_the_reference(precision):
    sc, eps, o, res = race_reference()
    e = load(race_engine(precision), sc, tc.CLOCK)
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = tc.kept(o, False)  # (the reference itself is f32: the margin applies to both handles)
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", tc.penalised(S_ref).mean(), "n_collided", st.n_collided)
    assert keep.mean() >= 1.0 - tc.MAX_LEFT_OUT
    assert np.array_equal(tc.penalised(S)[keep], tc.penalised(S_ref)[keep])
    np.testing.assert_allclose(S[keep], S_ref[keep], rtol=2e-4, atol=2e-4)
    assert float(np.sqrt(np.mean((u - res["u_returned"]) ** 2))) <= 1e-4
    assert int(tc.penalised(S)[keep].sum()) == int(tc.penalised(S_ref)[keep].sum())
    assert spec_of(e) == "5"


# ------------------------------------------------------------------------------------------ 4. equivalence
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_a_track_sampled_from_a_velocity_equals_the_moving_circle(precision):
    T = 50
    sc, eps, o, res = mc.diff_case(T, True, "frozen")
    moving = diff_engine(T, "frozen", True, precision)
    moving.set_ref_path(sc["ref"])
    moving.set_obstacles(sc["circles"], velocities=sc["vel"])
    moving.set_u_prev(sc["u"])
    tracks = diff_engine(T, "frozen", True, precision)
    tracks.set_ref_path(sc["ref"])
    tracks.set_obstacle_tracks(tc.sample_velocity(sc["circles"], sc["vel"], 0.1, T + 1), sc["circles"][:, 2])
    tracks.set_u_prev(sc["u"])
    out = [h.step(sc["x0"], eps=cuda(eps)) for h in (moving, tracks)]
    Sm, St = moving.costs(), tracks.costs()
    keep = mc.kept(o, precision == "f64")
    assert spec_of(moving) == "3" and spec_of(tracks) == "5"
    assert 0 < tc.penalised(Sm).sum() < K and keep.mean() >= 1.0 - tc.MAX_LEFT_OUT
    assert np.array_equal(tc.penalised(Sm)[keep], tc.penalised(St)[keep])
    if precision == "f64":
        np.testing.assert_allclose(St, Sm, rtol=1e-10, atol=1e-10)
        assert out[0][2].n_collided == out[1][2].n_collided
    else:
        np.testing.assert_allclose(St[keep], Sm[keep], rtol=2e-4, atol=2e-4)
        assert abs(out[0][2].n_collided - out[1][2].n_collided) <= int((~keep).sum())


# ------------------------------------------------------------------------------------------ 5. bit for bit
def loop_scene(T=50):
    return tc.loop_scene(T)


def state_of(e):
    return e.get_u_prev(), e.get_state(), e.costs(), int(e.stats.n_collided)


def assert_same(a, b):
    for x, y in zip(state_of(a), state_of(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_never_called_and_cleared_are_the_same_handle(precision):
    T = 50
    sc = loop_scene(T)
    never = diff_engine(T, "frozen", True, precision, seed=3)
    never.set_ref_path(sc["ref"])
    never.set_obstacles(sc["circles"], velocities=sc["vel"])
    cleared = load(diff_engine(T, "frozen", True, precision, seed=3), sc)
    late = load(diff_engine(T, "frozen", True, precision, seed=3), sc)
    cleared.set_obstacle_tracks(np.zeros((0, 1, 2)), [])
    for h in (never, cleared, late):
        h.set_u_prev(sc["u"])
        h.set_state(sc["x0"])
        h.run_closed_loop(2)
    assert spec_of(never) == "3" and spec_of(cleared) == "3" and spec_of(late) == "5"
    assert_same(never, cleared)
    assert not np.array_equal(never.costs(), late.costs())  # the tracks matter on this scene
    late.set_obstacle_tracks(np.zeros((0, 1, 2)), [])  # cleared in mid-run: from here on the same iterations again
    for h in (never, late):
        h.set_u_prev(sc["u"])
        h.set_state(sc["x0"])
        h.set_iteration(7)
        h.run_closed_loop(2)
    assert spec_of(late) == "3"
    assert_same(never, late)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_replay_and_one_call_equal_single_calls(monkeypatch, precision):
    T, n_it = 50, 6
    sc = loop_scene(T)

    def fresh():
        e = load(diff_engine(T, "frozen", True, precision, seed=31), sc)
        e.set_state(sc["x0"])
        return e
    eager = fresh()
    for _ in range(n_it):
        eager.run_closed_loop(1)
    once = fresh()
    trace, _ = once.run_closed_loop(n_it, trace=True)
    assert_same(eager, once)
    assert len(np.unique(np.round(trace[:, 0], 6))) > 2
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = fresh()
    graph.run_closed_loop(n_it)
    assert_same(eager, graph)
    assert spec_of(graph) == "5" and eager.stats.n_collided > 0


@pytest.mark.parametrize("model,precision", [("diff", "f64"), ("diff", "f32"), ("race", "f32")])
def test_agents_with_own_track_sets_equal_single_handles(model, precision):
    """Four agents: the case tracks with the own circles; two of the tracks, shorter (other n, other L); circles and no
    tracks; nothing.  Bit for bit against single-agent handles, the first set uploaded one iteration late on both sides."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if model == "diff":
        T, sc = 50, loop_scene(50)
        cfg = dict(diff_cfg(capi.WAYPOINT_FROZEN, T, precision=prec(precision)), obstacle_motion=1, accumulate_stage_cost=1)
    else:
        T, sc = mc.RACE_T, tc.race_scene(clock=0, extra=2)
        cfg = dict(race_cfg(), precision=prec(precision), obstacle_motion=1)
    L = sc["tracks"].shape[1]
    none = (np.zeros((0, 1, 2)), np.zeros(0))
    tracks = [(sc["tracks"], sc["radii"]), (sc["tracks"][:2, :L // 2] + [0.05, -0.05], sc["radii"][:2]), none, none]
    circles = [(sc["circles"], sc["vel"]), (np.zeros((0, 3)), np.zeros((0, 2))), (sc["circles"], sc["vel"]), (np.zeros((0, 3)), np.zeros((0, 2)))]
    rng = np.random.default_rng(11)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(4)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(4)])
    batch = pkg.Engine(K=K, n_agents=4, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(4)]
    batch.set_ref_path(sc["ref"])
    batch.set_state(x0)
    batch.set_u_prev(u)
    for a, one in enumerate(singles):
        one.set_ref_path(sc["ref"])
        one.set_state(x0[a])
        one.set_u_prev(u[a])
        one.set_obstacles(*[circles[a][0]], velocities=circles[a][1])
        batch.set_obstacles(circles[a][0], agent=a, velocities=circles[a][1])
        if a != 0:
            one.set_obstacle_tracks(*tracks[a])
            batch.set_obstacle_tracks(*tracks[a], agent=a)
    hits = []
    for n_run in (1, 1, 4):
        batch.run_closed_loop(n_run)
        for one in singles:
            one.run_closed_loop(n_run)
        compare(batch, singles, None)
        hits.append([int(one.stats.n_collided) for one in singles])
        if len(hits) == 1:  # agent 0 gets its tracks now: their clock starts at iteration 1
            singles[0].set_obstacle_tracks(*tracks[0])
            batch.set_obstacle_tracks(*tracks[0], agent=0)
        for a in range(4):
            got = batch.obstacle_tracks_at(1, agent=a)
            np.testing.assert_array_equal(got, singles[a].obstacle_tracks_at(1))
            assert len(got) == len(tracks[a][1])
    print(model, precision, "n_collided per agent and stretch", hits, batch.rollout_kernel())
    assert hits[1][1] > 0 and all(h[3] == 0 for h in hits)  # (agent 1: tracks and no circles; agent 3: nothing)
    assert ", true, 5, " in batch.rollout_kernel() and ", false, 5, " in singles[1].rollout_kernel()
    assert ", false, 3, " in singles[3].rollout_kernel()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_shared_track_set_its_replacement_and_the_return_to_it(monkeypatch, graph):
    """The plain setter gives every agent of a batch the same set; one agent gets its own in between (its clock starts
    there), then an empty one, then the shared set again for both -- and (MPPI_GRAPH=1) graph replay across the setters: every
    stretch equals single handles driven the same way."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if graph == "1":
        monkeypatch.setenv("MPPI_GRAPH", "1")
    T = 50
    sc = loop_scene(T)
    cfg = dict(diff_cfg(capi.WAYPOINT_FROZEN, T), obstacle_motion=1, accumulate_stage_cost=1)
    rng = np.random.default_rng(13)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(2)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(2)])
    batch = pkg.Engine(K=K, n_agents=2, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(2)]
    for e, xs, us in [(batch, x0, u)] + [(singles[a], x0[a], u[a]) for a in range(2)]:
        e.set_ref_path(sc["ref"])
        e.set_obstacle_tracks(sc["tracks"], sc["radii"])
        e.set_state(xs)
        e.set_u_prev(us)

    def run(n):
        for e in [batch] + singles:
            e.run_closed_loop(n)
        compare(batch, singles, None)
        return [int(one.stats.n_collided) for one in singles]
    first = run(3)
    own = (sc["tracks"][1:, :20] + [0.1, 0.05], sc["radii"][1:])
    batch.set_obstacle_tracks(*own, agent=1)
    singles[1].set_obstacle_tracks(*own)
    run(3)
    np.testing.assert_array_equal(batch.obstacle_tracks_at(2, agent=0)[:, :2], sc["tracks"][:, 8])  # (agent 0: the shared clock, 6)
    np.testing.assert_array_equal(batch.obstacle_tracks_at(2, agent=1)[:, :2], own[0][:, 5])        # (agent 1: its own, 3)
    batch.set_obstacle_tracks(np.zeros((0, 1, 2)), [], agent=1)  # an own set of no tracks: agent 1 collides with nothing
    singles[1].set_obstacle_tracks(np.zeros((0, 1, 2)), [])
    assert run(2)[1] == 0 and spec_of(singles[1]) == "3" and spec_of(batch) == "5"
    for e in [batch] + singles:
        e.set_obstacle_tracks(sc["tracks"], sc["radii"])  # back to the shared set for both
    last = run(2)
    assert batch.stats.iteration == 10 and min(first) > 0 and min(last) > 0
    assert len(batch.obstacle_tracks_at(0, agent=1)) == 3


LIMIT_T = 128


@pytest.mark.parametrize("precision,staged,memory", [("f32", 38, 39), ("f64", 7, 8)])
def test_both_sides_of_the_lds_limit(precision, staged, memory):
    """T = 128: 38 tracks (4902 points) are staged in LDS by an f32 handle, 39 (5031) are read from memory -- 7 (903) and 8
    (1032) for f64.  The track beyond the limit is a far one: S is bit for bit the same, and both are held to the reference."""
    sc, eps, o, res = diff_reference(LIMIT_T, False, "frozen")
    L = sc["tracks"].shape[1]
    S = []
    for n in (staged, memory):
        far = tc.far_tracks(n - 3, L)
        half = dict(sc, tracks=np.concatenate([sc["tracks"][:2], far, sc["tracks"][2:]]), radii=np.concatenate([sc["radii"][:2], np.full(n - 3, 0.5), sc["radii"][2:]]))
        assert half["tracks"].shape == (n, L, 2) and n * (LIMIT_T + 1) in (4902, 5031, 903, 1032)
        e = load(diff_engine(LIMIT_T, "frozen", False, precision), half, tc.CLOCK)
        check_iteration(e, sc, eps, o, res, precision)
        assert spec_of(e) == "5"
        S.append(e.costs())
    np.testing.assert_array_equal(S[0], S[1])


# ------------------------------------------------------------------------------------------ 6. the closed loop
LOOP_T, LOOP_N = 50, 6
LOOP_W = dict(stage_cost_weight=[0.25, 0.25, 0.5, 0], terminal_cost_weight=[0.25, 0.25, 0.5, 0])


@functools.lru_cache(maxsize=None)
def loop_reference():
    """The reference loop on the noise the device's sampler draws (mppi_sample_epsilon: bit for bit what the kernels draw)."""
    e = diff_engine(LOOP_T, "frozen", True, "f32", seed=31, **LOOP_W)
    ring = [e.sample_epsilon(i).cpu().numpy() for i in range(LOOP_N)]
    e.close()
    return tc.diff_closed_loop(LOOP_T, LOOP_N, eps_of=lambda i: ring[i])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_closed_loop_runs_past_the_end_of_the_tracks(precision):
    """Six iterations with tracks of L = T + 3 and two own moving circles: iterations 3 .. 5 read the held point.  f64: one
    call, end to end.  f32: re-seeded with the reference's state and controls before every iteration (one-iteration bounds)."""
    ref = loop_reference()
    sc = ref["scene"]
    assert sc["tracks"].shape[1] == LOOP_T + 3 and len(sc["circles"]) == 2
    assert max(ref["n_hit"]) - min(ref["n_hit"]) > K // 16 and min(ref["kept"]) >= 1.0 - tc.MAX_LEFT_OUT
    e = load(diff_engine(LOOP_T, "frozen", True, precision, seed=31, **LOOP_W), sc)
    e.set_state(sc["x0"])
    if precision == "f64":
        trace, st = e.run_closed_loop(LOOP_N, trace=True)
        print("reference hits per iteration", ref["n_hit"], "last n_collided", st.n_collided)
        np.testing.assert_allclose(trace, ref["u0"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(e.get_state(), ref["x"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == ref["n_counted"][-1]  # (S >= collision_penalty: the kernels' definition)
    else:
        for i in range(LOOP_N):
            e.set_state(ref["x_at"][i])
            e.set_u_prev(ref["u_at"][i])
            trace, st = e.run_closed_loop(1, trace=True)
            err = float(np.sqrt(np.mean((trace[0] - ref["u0"][i]) ** 2)))
            print("iteration", i, "u0 error", err, "n_collided", st.n_collided, "reference", ref["n_hit"][i])
            assert err <= 1e-4
    assert st.iteration == LOOP_N and spec_of(e) == "5"
    # (clock 6: step T would read point T + 6, beyond the last one, T + 2)
    np.testing.assert_array_equal(e.obstacle_tracks_at(LOOP_T)[:, :2], rounded(sc["tracks"], precision)[:, -1])


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_limit_and_change_nothing():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = loop_scene(T)
    e = load(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    twin = load(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    xy, r = sc["tracks"] + 5.0, sc["radii"]

    def refused(code, *a, word=None, **kw):
        with pytest.raises(pkg.MppiError) as ex:
            e.set_obstacle_tracks(*a, **kw)
        assert ex.value.code == code, str(ex.value)
        assert word is None or word in str(ex.value)
    bad = xy.copy()
    bad[1, 7, 0] = np.nan
    refused(capi.ERR_BAD_ARG, bad, r, word="finite")
    bad[1, 7, 0] = np.inf
    refused(capi.ERR_BAD_ARG, bad, r)
    refused(capi.ERR_BAD_ARG, xy, [0.4, -0.1, 0.4], word="radius")
    refused(capi.ERR_BAD_ARG, xy, [0.4, np.nan, 0.4])
    refused(capi.ERR_SHAPE, np.zeros((257, 2, 2)), np.full(257, 0.4), word="256")
    refused(capi.ERR_SHAPE, np.zeros((1, 65537, 2)), [0.4], word="65536")
    refused(capi.ERR_BAD_ARG, xy, r, agent=1)
    refused(capi.ERR_BAD_ARG, xy, r, agent=-1)
    assert e.lib.mppi_set_obstacle_tracks(e._h, None, None, 2, 5) == capi.ERR_BAD_ARG
    assert e.lib.mppi_set_obstacle_tracks(e._h, xy.ctypes.data_as(capi._D), r.ctypes.data_as(capi._D), 3, 0) == capi.ERR_SHAPE
    import ctypes as C
    n = C.c_int32(-1)
    assert e.lib.mppi_get_obstacle_tracks_at(e._h, 0, 0, None, 0, C.byref(n)) == capi.ERR_SHAPE and n.value == 3
    assert e.lib.mppi_get_obstacle_tracks_at(e._h, 1, 0, None, 0, C.byref(n)) == capi.ERR_BAD_ARG
    assert e.lib.mppi_get_obstacle_tracks_at(e._h, 0, -1, None, 0, C.byref(n)) == capi.ERR_BAD_ARG
    np.testing.assert_array_equal(e.obstacle_tracks_at(4), twin.obstacle_tracks_at(4))
    for h in (e, twin):
        h.set_state(sc["x0"])
        h.run_closed_loop(3)
    assert e.stats.n_collided > 0 and spec_of(e) == "5"
    assert_same(e, twin)
    # handles that take no tracks
    static = diff_engine(T, "frozen", True, "f64", obstacle_motion=0)
    with pytest.raises(pkg.MppiError) as ex:
        static.set_obstacle_tracks(xy, r)
    assert ex.value.code == capi.ERR_STATE and "obstacle_motion" in str(ex.value)
    with pytest.raises(pkg.MppiError) as ex:
        static.set_obstacle_tracks(xy, r, agent=0)
    assert ex.value.code == capi.ERR_STATE
    fleet = pkg.Engine(K=K, n_agents=2, **dict(diff_cfg(capi.WAYPOINT_FROZEN, T), obstacle_motion=1, fleet_radius=0.3))
    with pytest.raises(pkg.MppiError) as ex:
        fleet.set_obstacle_tracks(xy, r)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "fleet_radius" in str(ex.value)
    long = diff_engine(130, "frozen", True, "f64")
    with pytest.raises(pkg.MppiError) as ex:
        long.set_obstacle_tracks(xy, r)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "T <= 128" in str(ex.value)


def test_controller_keyword_switches_motion_on():
    """`obstacle_tracks` on the controllers: last keyword, settable property; a controller built without it refuses."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc, eps, o, res = tc.diff_case(T, False, "frozen", clock=0)
    kw = dict(mc.DIFF_KW, ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T)
    c = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", obstacle_tracks=(sc["tracks"], sc["radii"]))
    assert c._engine.cfg.obstacle_motion == 1 and c._engine.cfg.obstacle_model == capi.OBSTACLE_CIRCLE
    assert np.array_equal(c.obstacle_tracks[0], sc["tracks"]) and np.array_equal(c.obstacle_tracks[1], sc["radii"])
    c.u_prev[:] = sc["u"]
    c._calc_epsilon = lambda *a, **k: cuda(eps)
    _, u, _, _ = c._calc_input_control(sc["x0"])
    np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
    c.obstacle_tracks = (sc["tracks"][:1], sc["radii"][:1])  # settable, like obstacle_circles
    assert len(c._engine.obstacle_tracks_at(0)) == 1
    c.obstacle_tracks = (np.zeros((0, 1, 2)), [])
    assert c.obstacle_tracks is None and len(c._engine.obstacle_tracks_at(0)) == 0
    plain = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", obstacle_circles=mc.diff_scene(T, False)["circles"])
    assert plain.obstacle_tracks is None
    with pytest.raises(pkg.MppiError) as ex:
        plain.obstacle_tracks = (sc["tracks"], sc["radii"])
    assert ex.value.code == capi.ERR_STATE and "obstacle_motion" in str(ex.value)
    rs = tc.race_scene(clock=0)
    rc = pkg.MPPIRacecarController(ref_path=rs["ref"], horizon_step_T=mc.RACE_T, number_of_samples_K=64, obstacle_tracks=(rs["tracks"], rs["radii"]))
    assert rc._engine.cfg.obstacle_motion == 1 and rc._engine.cfg.obstacle_model == capi.OBSTACLE_OUTLINE
    assert len(rc._engine.obstacle_tracks_at(0)) == 2
