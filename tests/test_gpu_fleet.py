"""Fleet avoidance on the device (mppi_config.fleet_radius): the mates' rows k_fleet_rows writes, against the f64
reference and the error model of tests/fleet_checks.py; what the collision test, one iteration and the closed loop make of
them; the clearance record; cutting, graph replay, behaviour and the refusals.  K = 256 unless stated."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import moving_obstacle_checks as mc
from oracle import mppi_oracle
from test_gpu_agent_scenes import diff_cfg, race_cfg

pytestmark = pytest.mark.gpu

K = mc.K_CASE
MODES = {"frozen": "WAYPOINT_FROZEN", "per_rollout": "WAYPOINT_PER_ROLLOUT"}
RACE_SIGMA = np.array([[0.5, 0.0], [0.0, 0.1]])


def prec(name):
    from dnn_mppi_mpc_amd import _capi as capi
    return capi.PREC_F64 if name == "f64" else capi.PREC_F32


def engine(model, precision, B, T=20, mode="frozen", accumulate=False, K=K, fleet=True, **kw):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    if model == "race":
        cfg = dict(race_cfg(), precision=prec(precision))
        radius = fc.RACE_RADIUS
    else:
        cfg = dict(diff_cfg(getattr(capi, MODES[mode]), T, precision=prec(precision)), accumulate_stage_cost=int(accumulate),
                   filter_window=mc.filter_window(T))
        radius = fc.RADIUS
    cfg.update(obstacle_motion=1, n_agents=B, fleet_radius=radius if fleet else 0.0)
    cfg.update(kw)
    return pkg.Engine(K=K, **cfg)


def load(e, sc, own=None, shared=None):
    for a, ref in enumerate(sc["refs"]):
        e.set_ref_path(ref, agent=a)
    if shared is not None:
        e.set_obstacles(shared[0], velocities=shared[1])
    for a, (c, v) in enumerate(own or []):
        e.set_obstacles(c, agent=a, velocities=v)
    e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    return e


def device_noise(model, B, T, n_iters, K=K, **kw):
    """What the sampler draws for iterations 0 .. n_iters - 1 ([B, K, T, 2] each; the same for f32 and f64 handles), held to
    oracle/philox.py with the counter word noise_stream + a as tests/test_gpu_engine.py holds the single-agent sampler to it."""
    e = engine(model, "f32", B, T, K=K, **kw)
    out = []
    for i in range(n_iters):
        got = e.sample_epsilon(i).cpu().numpy()
        want = fc.numpy_noise(RACE_SIGMA if model == "race" else mc.DIFF_KW["sigma"], int(e.cfg.seed), i, B, K, e.T, int(e.cfg.noise_stream))
        np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)
        out.append(got)
    e.close()
    return out


# ------------------------------------------------------------------------------------------ 1. the rows
def rows_scene(model, B, seed=0):
    """B agents scattered around one shared path, some nominal speeds beyond the clamp"""
    rng = np.random.default_rng(500 + B + seed)
    if model == "race":
        ref = mppi_oracle.generate_lemniscate_racecar(100, 10.0).astype(np.float64)
        x0 = np.stack([rng.uniform(-12, 12, B), rng.uniform(-6, 6, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(2.0, 6.0, B)], axis=1)
        u = rng.normal(0, 0.05, (B, mc.RACE_T, 2))
    else:
        ref = fc.line((0.0, 0.0), (10.0, -5.0))
        x0 = np.stack([rng.uniform(-5, 15, B), rng.uniform(-10, 5, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
        u = np.stack([rng.uniform(-1.0, 6.0, (B, 20)), rng.normal(0, 0.1, (B, 20))], axis=2)
    return dict(refs=[ref] * B, x0=x0, u=u, model=model)


def own_sets(kind, B, seed=0):
    """-> (shared or None, per-agent list or None, what agent b owns)"""
    rng = np.random.default_rng(600 + seed)

    def some(m):
        return (np.concatenate([rng.uniform(-20, 20, (m, 2)), rng.uniform(0.2, 1.0, (m, 1))], axis=1), rng.uniform(-2, 2, (m, 2)))
    if kind == "none":
        return None, None, [fc.NO_OWN] * B
    if kind == "shared":
        s = some(2)
        return s, None, [s] * B
    per = [some((0, 1, 3)[a % 3]) for a in range(B)]
    return None, per, per


def expect_rows(e, model, owned, n, agents):
    x, u = e.get_state(), e.get_u_prev()
    mate_c, mate_v = fc.mate_rows(x, u[:, 0], model, fc.rows_cfg(model))
    out = {}
    for b in agents:
        c = np.asarray(owned[b][0], np.float64).reshape(-1, 3).copy()
        v = np.asarray(owned[b][1], np.float64).reshape(-1, 2)
        c[:, :2] += v * (fc.dt_of(model) * n)
        out[b] = (np.concatenate([c, mate_c[b]]), np.concatenate([v, mate_v[b]]))
    return out


def compare_rows(e, model, owned, n, agents, precision):
    worst = 0.0
    for b, (want_c, want_v) in expect_rows(e, model, owned, n, agents).items():
        got_c, got_v = e.agent_circles(b)
        worst = max(worst, fc.check_rows(got_c, got_v, want_c, want_v, fc.dt_of(model), n, fc.thr_of(model), precision))
    return worst


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
@pytest.mark.parametrize("own", ["none", "shared", "per_agent"])
@pytest.mark.parametrize("B", [2, 3, 5, 66])
def test_rows_against_the_reference(B, own, model, precision):
    sc = rows_scene(model, B)
    shared, per, owned = own_sets(own, B)
    e = load(engine(model, precision, B), sc, per, shared)
    agents = range(B) if B <= 5 else (0, 1, 33, 64, 65)
    worst = compare_rows(e, model, owned, 0, agents, precision)  # clock 0
    before = [e.agent_circles(b) for b in agents]
    e.set_iteration(5)  # replays noise: nothing moves at step 0
    for (c0, v0), b in zip(before, agents):
        c1, v1 = e.agent_circles(b)
        assert np.array_equal(c0, c1) and np.array_equal(v0, v1)
    e.run_closed_loop(3)  # clock 3: the own sets have moved on, the mates are back-dated by three steps
    worst = max(worst, compare_rows(e, model, owned, 3, agents, precision))
    rng = np.random.default_rng(B)
    e.set_state(sc["x0"] + rng.normal(0, 1.0, sc["x0"].shape))
    worst = max(worst, compare_rows(e, model, owned, 3, agents, precision))
    e.set_u_prev(sc["u"][::-1] * 0.5)
    worst = max(worst, compare_rows(e, model, owned, 3, agents, precision))
    for b in agents:
        assert e.agent_circles(b)[0].shape[0] == len(owned[b][0]) + B - 1
    print(f"fleet rows {model} B={B} own={own} {precision} max error / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ 2. the collision test on agent 0
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_eval_is_collided_sees_agent_0s_mates(model, precision):
    T = 20 if model == "diff" else mc.RACE_T
    sc = fc.crossing_scene(T, True) if model == "diff" else fc.race_pair_scene()
    B = len(sc["refs"])
    e = load(engine(model, precision, B, T, accumulate=True), sc)
    e.run_closed_loop(2)  # (the rows a getter refreshes are back-dated by two steps)
    x, u = e.get_state(), e.get_u_prev()
    mate_c, mate_v = fc.mate_rows(x, u[:, 0], model, fc.rows_cfg(model))
    p, v, r = mate_c[0][0][:2], mate_v[0][0], mate_c[0][0][2]  # agent 1 as agent 0 sees it
    thr = fc.thr_of(model)(r)
    poses, steps, want = [], [], []
    for j in (0, 1, T // 2, T):
        centre = p + v * (fc.dt_of(model) * j)
        for k, ang in enumerate(np.linspace(0.0, 2 * np.pi, 7)[:-1] + 0.1 * j):
            h = np.array([np.cos(ang), np.sin(ang)])
            for inside in (True, False):
                d = thr * (1.0 - 1e-3 if inside else 1.0 + 1e-3)
                if model == "diff":  # the robot's disc: its centre at distance d
                    pose = [*(centre + d * h), 0.3 * k]
                else:  # the outline's front-centre point (0.5 * 4.0 * 1.5 ahead of the pose) at distance d, the car facing the centre
                    pose = [*(centre - (3.0 + d) * h), ang, 5.0]
                poses.append(pose)
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    poses, steps, want = np.array(poses), np.array(steps, dtype=np.int32), np.array(want)
    got = e.eval_is_collided(poses, steps=steps)
    assert np.array_equal(got, want), (got, want)
    now = e.eval_is_collided(poses)  # the existing entry: step 0 of the current clock
    assert np.array_equal(now[steps == 0], want[steps == 0])
    e.set_state(x + 50.0)  # the mates move away with their states; agent 0's own pose does not enter
    assert not e.eval_is_collided(poses, steps=steps).any()


# ------------------------------------------------------------------------------------------ 3. one iteration's costs
@functools.lru_cache(maxsize=None)
def cost_reference(model, T, accumulate, mode):
    sc = fc.crossing_scene(T, accumulate) if model == "diff" else fc.race_pair_scene()
    B = len(sc["refs"])
    eps = device_noise(model, B, T, 1, mode=mode, accumulate=accumulate)[0]
    return sc, fc.one_iteration(sc, eps, K, T, mode, accumulate)


def check_costs(e, runs, precision, race=False):
    S, u = e.costs(), e.get_u_prev()
    for a, (o, res) in enumerate(runs):
        S_ref = np.asarray(res["S"], np.float64)
        keep = mc.kept(o, precision == "f64" and not race)  # (the race-car reference is f32 itself: the margin applies to both)
        err_u = float(np.sqrt(np.mean((u[a] - res["u_returned"]) ** 2)))
        print("agent", a, e.rollout_kernel(), "kept", keep.mean(), "penalised", mc.penalised(S_ref).mean(), "u rmse", err_u)
        assert keep.mean() >= 1.0 - mc.MAX_LEFT_OUT
        assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(S_ref)[keep])
        if precision == "f64" and not race:
            np.testing.assert_allclose(S[a], S_ref, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(u[a], res["u_returned"], rtol=1e-8, atol=1e-10)
        else:
            np.testing.assert_allclose(S[a][keep], S_ref[keep], rtol=2e-4, atol=2e-4)
            assert err_u <= 1e-4


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode", fc.diff_cases())
def test_diff_costs_of_every_agent(T, accumulate, mode, precision):
    sc, runs = cost_reference("diff", T, accumulate, mode)
    e = load(engine("diff", precision, 3, T, mode, accumulate), sc)
    e.run_closed_loop(1)
    check_costs(e, runs, precision)
    assert ", true, 3, " in e.rollout_kernel()  # the batched moving instantiation, as without the fleet
    assert mc.penalised(e.costs()[0]).any() and mc.penalised(e.costs()[1]).any()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_costs_of_both_cars(precision):
    sc, runs = cost_reference("race", mc.RACE_T, True, "frozen")
    e = load(engine("race", precision, 2), sc)
    e.run_closed_loop(1)
    check_costs(e, runs, precision, race=True)


# ------------------------------------------------------------------------------------------ 4. closed loop
LOOP_T, LOOP_N = 20, 6
LOOP_W = dict(stage_cost_weight=[0.25, 0.25, 0.5, 0], terminal_cost_weight=[0.25, 0.25, 0.5, 0])


def loop_own(sc):
    """Own moving sets for the crossing scene: one circle drifting beside agent 0's path, none for agent 1, two for agent 2"""
    return [(np.array([[2.0, -1.0, 0.4]]), np.array([[0.0, 0.25]])), fc.NO_OWN,
            (np.array([[2.5, 6.9, 0.4], [1.0, 5.0, 0.3]]), np.array([[-0.3, 0.0], [0.2, 0.1]]))]


@functools.lru_cache(maxsize=None)
def loop_reference():
    sc = fc.crossing_scene(LOOP_T, True)
    ring = device_noise("diff", 3, LOOP_T, LOOP_N, accumulate=True, **LOOP_W)
    return sc, fc.closed_loop(sc, lambda i: ring[i], LOOP_N, K, LOOP_T, own=loop_own(sc), accumulate=True, **mc.LOOP_KW)


def test_closed_loop_f64_end_to_end():
    sc, ref = loop_reference()
    e = load(engine("diff", "f64", 3, LOOP_T, accumulate=True, **LOOP_W), sc, loop_own(sc))
    for i in range(LOOP_N):
        e.run_closed_loop(1)
        S = e.costs()
        np.testing.assert_allclose(S, ref["S"][i], rtol=1e-10, atol=1e-10, err_msg=f"iteration {i}")
        assert [int((S[a] >= 1.0e10).sum()) for a in range(3)] == list(ref["n_hit"][i]), i
        assert e.stats.n_collided == ref["n_hit"][i][0]
        np.testing.assert_allclose(e.get_state(), ref["x"][i + 1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(e.get_u_prev(), ref["u"], rtol=1e-8, atol=1e-10)
    print("reference hits per iteration and agent", ref["n_hit"].tolist())
    assert ref["n_hit"][:, :2].max() > K // 16 and len(set(map(tuple, ref["n_hit"]))) > 1  # the mates matter, the scene changes


def test_closed_loop_f32_iteration_by_iteration():
    """Each iteration re-seeded from the reference: a flipped near-threshold sample of one iteration decides no later one."""
    sc, ref = loop_reference()
    e = load(engine("diff", "f32", 3, LOOP_T, accumulate=True, **LOOP_W), sc, loop_own(sc))
    us = list(ref["u_start"]) + [ref["u"]]
    for i in range(LOOP_N):
        e.set_state(ref["x"][i])
        e.set_u_prev(us[i])
        e.set_iteration(i)  # (where the counter already stands: nothing moves)
        e.run_closed_loop(1)
        S = e.costs()
        for a in range(3):
            keep = ref["kept"][i][a]
            assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(ref["S"][i][a])[keep]), (i, a)
            np.testing.assert_allclose(S[a][keep], ref["S"][i][a][keep], rtol=2e-4, atol=2e-4, err_msg=f"iteration {i}, agent {a}")
        if ref["kept"][i].all():  # (a sample left out may carry the update either way)
            assert float(np.sqrt(np.mean((e.get_u_prev() - us[i + 1]) ** 2))) <= 1e-4
            # (the plant integrates u0 once: |dx| <= dt max|du0| <= 0.1 * sqrt(2 T B) * 1e-4 under the bound above)
            np.testing.assert_allclose(e.get_state(), ref["x"][i + 1], rtol=0, atol=0.1 * np.sqrt(2 * LOOP_T * 3) * 1e-4)
    print("kept per iteration and agent", ref["kept"].mean(axis=2).tolist())
    assert ref["kept"].mean(axis=2).min() >= 1.0 - mc.MAX_LEFT_OUT


# ------------------------------------------------------------------------------------------ 5. own circles untouched
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("B", [3, 66])
def test_far_apart_fleet_equals_the_handle_without(B, precision):
    T = 20
    sc = fc.far_scene(B, T)
    own = fc.far_own(sc)
    on = load(engine("diff", precision, B, T), sc, own)
    off = load(engine("diff", precision, B, T, fleet=False), sc, own)
    hits = 0
    for _ in range(5):
        on.run_closed_loop(1)
        off.run_closed_loop(1)
        assert np.array_equal(on.costs(), off.costs())
        hits += int(mc.penalised(on.costs()).sum())
    assert np.array_equal(on.get_u_prev(), off.get_u_prev()) and np.array_equal(on.get_state(), off.get_state())
    assert on.rollout_kernel() == off.rollout_kernel() and hits > 0
    assert on.agent_circles(0)[0].shape[0] == B and off.agent_circles(0)[0].shape[0] == 1
    d, n = on.fleet_clearance()
    assert d.min() > 900.0 and not n.any()


# ------------------------------------------------------------------------------------------ 6. clearance
def test_clearance_against_the_hosts_recomputation():
    T = 20
    sc = fc.contact_scene(T)
    e = load(engine("diff", "f64", 3, T), sc)
    twin = load(engine("diff", "f64", 3, T), sc)
    d, n = e.fleet_clearance()
    assert np.all(np.isinf(d)) and d.min() > 0 and not n.any()
    e.run_closed_loop(8)
    starts = []
    for _ in range(8):
        starts.append(twin.get_state())
        twin.run_closed_loop(1)
    dist = np.array([fc.min_mate_distance(x) for x in starts])  # [8, B]
    d, n = e.fleet_clearance()
    print("min_dist", d, "host", dist.min(axis=0), "contact_iters", n, "host", (dist < 2 * fc.RADIUS).sum(axis=0))
    assert np.all(np.abs(d - dist.min(axis=0)) <= 4 * np.spacing(dist.min(axis=0)))
    assert np.array_equal(n, (dist < 2 * fc.RADIUS).sum(axis=0)) and n[0] >= 1 and n[1] >= 1 and n[2] == 0
    d2, n2 = twin.fleet_clearance()
    assert np.array_equal(d, d2) and np.array_equal(n, n2)
    # the refreshes in front of the getters and mppi_eval_* do not count
    e.agent_circles(0)
    e.eval_is_collided(np.zeros((4, 3)))
    e.eval_is_collided(np.zeros((4, 3)), steps=[0, 1, 2, 3])
    e.eval_cost(np.zeros((4, 3)), 0)
    d3, n3 = e.fleet_clearance(reset=True)
    assert np.array_equal(d, d3) and np.array_equal(n, n3)
    d4, n4 = e.fleet_clearance()
    assert np.all(np.isinf(d4)) and not n4.any()
    e.run_closed_loop(1)
    d5, n5 = e.fleet_clearance()
    assert np.all(np.isfinite(d5)) and n5.max() <= 1


# ------------------------------------------------------------------------------------------ 7. cutting and replay
def test_one_call_equals_one_iteration_calls():
    T = 20
    sc = fc.crossing_scene(T, True)
    a = load(engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, loop_own(sc))
    b = load(engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, loop_own(sc))
    a.run_closed_loop(9)
    for _ in range(9):
        b.run_closed_loop(1)
    for got, want in ((a.get_state(), b.get_state()), (a.get_u_prev(), b.get_u_prev()), (a.costs(), b.costs()),
                      *zip(a.fleet_clearance(), b.fleet_clearance())):
        assert np.array_equal(got, want)


def test_graph_replay_equals_eager(monkeypatch):
    slots = 4
    n = 2 * slots + 3
    T = 8
    sc = fc.crossing_scene(T, True)
    eager = load(engine("diff", "f32", 3, T, accumulate=True, K=64, **LOOP_W), sc)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    monkeypatch.setenv("MPPI_GRAPH_SLOTS", str(slots))
    graph = load(engine("diff", "f32", 3, T, accumulate=True, K=64, **LOOP_W), sc)
    eager.run_closed_loop(n)
    graph.run_closed_loop(n)
    assert graph.stats.iteration == n
    for got, want in ((graph.get_state(), eager.get_state()), (graph.get_u_prev(), eager.get_u_prev()), (graph.costs(), eager.costs()),
                      *zip(graph.fleet_clearance(), eager.fleet_clearance())):
        assert np.array_equal(got, want)
    for h in (graph, eager):  # (the row launch is in neither launch class)
        cnt = h.counters()
        assert (cnt["iterations"], cnt["rollout_launches"], cnt["finalize_launches"]) == (n, n, n)


# ------------------------------------------------------------------------------------------ 8. behaviour
def test_head_on_robots_keep_more_distance_with_the_switch_on():
    Kb, T, n = 512, 20, 45
    sc = fc.head_on_scene(T)
    smallest = {}
    for fleet in (False, True):
        e = load(engine("diff", "f32", 2, T, K=Kb, fleet=fleet), sc)
        d = [fc.min_mate_distance(e.get_state())[0]]
        for _ in range(n):
            e.run_closed_loop(1)
            d.append(fc.min_mate_distance(e.get_state())[0])
        smallest[fleet] = float(min(d))
        if fleet:
            assert abs(e.fleet_clearance()[0][0] - min(d[:-1])) <= 4 * np.spacing(min(d[:-1]))
    print(f"fleet behaviour head-on smallest distance off {smallest[False]:.4f} on {smallest[True]:.4f} (2 r = {2 * fc.RADIUS})")
    assert smallest[False] < 2 * fc.RADIUS  # (geometry: tests/test_fleet_cases.py asserts it on the reference)
    assert smallest[True] > smallest[False]


# ------------------------------------------------------------------------------------------ 9. refusals on a live handle
def test_refusals_on_a_live_handle():
    import ctypes as C

    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 20
    sc = fc.crossing_scene(T, True)
    plain = load(engine("diff", "f32", 3, T, fleet=False), sc)
    with pytest.raises(pkg.MppiError) as ex:
        plain.fleet_clearance()
    assert ex.value.code == capi.ERR_STATE and "fleet_radius" in str(ex.value)
    assert plain.agent_circles(1)[0].shape == (0, 3)  # any handle with an obstacle model answers
    e = load(engine("diff", "f32", 3, T), sc, loop_own(sc))
    m = C.c_int32(-1)
    c, v = np.empty((2, 3)), np.empty((2, 2))
    dp = C.POINTER(C.c_double)
    rc = e.lib.mppi_get_agent_circles(e._h, 2, c.ctypes.data_as(dp), v.ctypes.data_as(dp), 2, C.byref(m))
    assert rc == capi.ERR_SHAPE and m.value == 4  # two own + two mates: written although cap is too small
    for agent in (-1, 3):
        with pytest.raises(pkg.MppiError) as ex:
            e.agent_circles(agent)
        assert ex.value.code == capi.ERR_BAD_ARG
    none = pkg.Engine(K=64, **dict(diff_cfg(capi.WAYPOINT_FROZEN, T, precision=capi.PREC_F32), obstacle_model=capi.OBSTACLE_NONE))
    with pytest.raises(pkg.MppiError) as ex:
        none.agent_circles(0)
    assert ex.value.code == capi.ERR_STATE
    with pytest.raises(pkg.MppiError) as ex:
        engine("diff", "f32", 1, T)
    assert ex.value.code == capi.ERR_BAD_ARG
