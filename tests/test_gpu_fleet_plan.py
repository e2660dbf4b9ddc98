"""Fleet plans on the device (mppi_set_fleet_prediction, MPPI_FLEET_PLAN): the table k_fleet_plan writes, against the
f64 definition and the error model of tests/fleet_plan_checks.py; what the collision test, one iteration (the SPEC 4 rollout
forms) and the closed loop make of it; cutting, graph replay, the switch back, the clearance record and the refusals.
K = 256 unless stated.  The rollout forms stage the plan table in LDS up to 40000 bytes (f32: 5000 points) / 16384 bytes (f64:
1024 points) and read it from memory beyond (fleet_plan_lds_bytes): the three-agent cases are all on the staged
side, the crowds of group 3 stand on both sides of either threshold."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import fleet_plan_checks as pc
import moving_obstacle_checks as mc
from test_gpu_fleet import K, LOOP_W, check_costs, device_noise, engine, load

pytestmark = pytest.mark.gpu


def plan_engine(*a, **kw):
    e = engine(*a, **kw)
    e.set_fleet_prediction("plan")
    return e


# ------------------------------------------------------------------------------------------ 1. the plans read back
def compare_plans(e, model, precision):
    return pc.check_plans(e.fleet_plans(), e.get_state(), e.get_u_prev(), model, pc.plan_cfg(model), precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model,T", [("diff", 7), ("diff", 64), ("diff", 65), ("diff", 128), ("race", mc.RACE_T)])
@pytest.mark.parametrize("B", [2, 3, 66])
def test_plans_against_the_definition(B, model, T, precision):
    sc = pc.scatter_scene(model, B, T)
    e = load(plan_engine(model, precision, B, T), sc)
    assert e.fleet_plans().shape == (B, T + 1, 2)
    worst = compare_plans(e, model, precision)  # clock 0
    e.run_closed_loop(3)  # the states and the nominal controls have moved on
    worst = max(worst, compare_plans(e, model, precision))
    rng = np.random.default_rng(B + T)
    e.set_state(sc["x0"] + rng.normal(0, 1.0, sc["x0"].shape))
    worst = max(worst, compare_plans(e, model, precision))
    e.set_u_prev(sc["u"][::-1] * 0.5)
    worst = max(worst, compare_plans(e, model, precision))
    print(f"fleet plans {model} B={B} T={T} {precision} max error / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ 2. the collision test on agent 0
FAR_OWN = (np.array([[300.0, 300.0, 0.4], [-300.0, 250.0, 0.6]]), np.array([[0.5, -0.25], [0.0, 1.0]]))


@pytest.mark.parametrize("n_own", [0, 2])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_eval_is_collided_at_a_mates_plan_point(model, precision, n_own):
    """MPPI_OBSTACLE_CIRCLE through the diff-drive handle, MPPI_OBSTACLE_OUTLINE through the race car's; at clock 2"""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 20 if model == "diff" else mc.RACE_T
    sc = pc.arc_scene(T, True) if model == "diff" else pc.race_curve_scene()
    B = len(sc["refs"])
    own = [FAR_OWN if n_own else fc.NO_OWN] + [fc.NO_OWN] * (B - 1)
    e = load(plan_engine(model, precision, B, T, accumulate=True), sc, own)
    e.run_closed_loop(2)
    P = pc.plans(e.get_state(), e.get_u_prev(), model, pc.plan_cfg(model))
    thr = np.sqrt(pc.threshold2(model))
    poses, steps, want = [], [], []
    for j in (0, 1, T // 2, T):
        centre = P[1, j]  # agent 1 as agent 0 sees it
        for k, ang in enumerate(np.linspace(0.0, 2 * np.pi, 7)[:-1] + 0.1 * j):
            h = np.array([np.cos(ang), np.sin(ang)])
            for inside in (True, False):
                d = thr * (1.0 - 1e-3 if inside else 1.0 + 1e-3)
                if model == "diff":
                    pose = [*(centre + d * h), 0.3 * k]
                else:  # the outline's front-centre point (0.5 * 4.0 * 1.5 ahead of the pose) at distance d, the car facing the centre
                    pose = [*(centre - (3.0 + d) * h), ang, 5.0]
                poses.append(pose)
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    n_mate = len(poses)
    if n_own:  # poses that only an own circle decides: 1e-3 inside / outside FAR_OWN's first circle where it stands at clock 2 + j
        c, r, v = FAR_OWN[0][0][:2], FAR_OWN[0][0][2], FAR_OWN[1][0]
        own_thr = fc.thr_of(model)(r)
        for j in (0, 1, T // 2, T):
            centre = c + v * (fc.dt_of(model) * (2 + j))
            for inside in (True, False):
                d = own_thr * (1.0 - 1e-3 if inside else 1.0 + 1e-3)
                poses.append([*(centre + d * np.array([0.6, 0.8])), 0.0] if model == "diff" else [*(centre - (3.0 + d) * np.array([0.6, 0.8])), np.arctan2(0.8, 0.6), 5.0])
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    poses, steps, want = np.array(poses), np.array(steps, dtype=np.int32), np.array(want)
    got = e.eval_is_collided(poses, steps=steps)
    assert np.array_equal(got, want), (got, want, steps)
    now = e.eval_is_collided(poses)  # the existing entry: point 0
    assert np.array_equal(now[steps == 0], want[steps == 0])
    with pytest.raises(pkg.MppiError) as ex:
        e.eval_is_collided(poses[:2], steps=np.array([T, T + 1], dtype=np.int32))
    assert ex.value.code == capi.ERR_BAD_ARG
    assert e.agent_circles(0)[0].shape[0] == n_own  # the own circles only
    e.set_state(e.get_state() + 50.0)  # the plans move away with the states, the own circles stay
    moved = e.eval_is_collided(poses, steps=steps)
    assert not moved[:n_mate].any() and np.array_equal(moved[n_mate:], want[n_mate:])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_eval_is_collided_at_with_a_diff_drive_outline(precision):
    """A diff-drive handle with MPPI_OBSTACLE_OUTLINE: the mates are tested against the folded outline, half extents
    0.5 vehicle_l safety_margin and 0.5 vehicle_w safety_margin, threshold fleet_radius -- front-centre, side-centre and corner
    points of the outline 1e-3 inside / outside a mate's plan point"""
    from dnn_mppi_mpc_amd import _capi as capi
    T, vl, vw, margin = 20, 0.8, 0.5, 0.8
    sc = pc.arc_scene(T, True)
    e = load(plan_engine("diff", precision, 3, T, accumulate=True, obstacle_model=capi.OBSTACLE_OUTLINE, vehicle_l=vl, vehicle_w=vw,
                         safety_margin=margin), sc)
    e.run_closed_loop(2)
    P = pc.plans(e.get_state(), e.get_u_prev(), "diff", pc.plan_cfg("diff"))
    ha, hb, thr = 0.5 * vl * margin, 0.5 * vw * margin, fc.RADIUS
    poses, steps, want = [], [], []
    for j in (0, 1, T // 2, T):
        centre = P[1, j]
        for k, (bx, by) in enumerate([(ha, 0.0), (0.0, hb), (ha, hb), (-ha, 0.0), (0.0, -hb), (-ha, -hb)]):
            yaw = 0.4 * k + 0.1 * j
            cs, sn = np.cos(yaw), np.sin(yaw)
            out = np.array([bx, by]) / np.hypot(bx, by)  # the outline point lies on the body-frame ray from the pose to the mate
            for inside in (True, False):
                d = thr * (1.0 - 1e-3 if inside else 1.0 + 1e-3)
                body = np.array([bx, by]) + d * out          # the mate's centre in the body frame
                world = np.array([body[0] * cs - body[1] * sn, body[0] * sn + body[1] * cs])
                poses.append([*(centre - world), yaw])
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    got = e.eval_is_collided(np.array(poses), steps=np.array(steps, dtype=np.int32))
    assert np.array_equal(got, np.array(want)), (got, want)


# ------------------------------------------------------------------------------------------ 3. one iteration's costs
@functools.lru_cache(maxsize=None)
def cost_reference(model, T, accumulate, mode, with_own=False):
    sc = pc.arc_scene(T, accumulate) if model == "diff" else pc.race_curve_scene()
    B = len(sc["refs"])
    seed = {"seed": pc.eps_seed(T, accumulate, mode)} if model == "diff" else {}  # (the race handle's own seed serves)
    eps = device_noise(model, B, T, 1, mode=mode, accumulate=accumulate, **seed)[0]
    own = pc.arc_own(sc) if with_own else None
    return sc, own, seed, pc.one_iteration(sc, eps, K, T, mode, accumulate, own=own)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode", pc.arc_cases())
def test_arc_costs_of_every_agent(T, accumulate, mode, precision):
    sc, _, seed, runs = cost_reference("diff", T, accumulate, mode)
    e = load(plan_engine("diff", precision, 3, T, mode, accumulate, **seed), sc)
    e.run_closed_loop(1)
    check_costs(e, runs, precision)
    assert ", true, 4, " in e.rollout_kernel()  # the batched plan instantiation
    hit0 = mc.penalised(e.costs()[0])
    assert hit0.any() and not hit0.all()
    assert e.stats.n_collided == int(hit0.sum())  # agent 0 has no circles of its own: its mates alone fill the count


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate", [(50, True), (65, False)])
def test_arc_costs_with_own_moving_circles(T, accumulate, precision):
    sc, own, seed, runs = cost_reference("diff", T, accumulate, "frozen", True)
    e = load(plan_engine("diff", precision, 3, T, "frozen", accumulate, **seed), sc, own)
    e.run_closed_loop(1)
    check_costs(e, runs, precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_costs_of_both_cars(precision):
    sc, _, _, runs = cost_reference("race", mc.RACE_T, True, "frozen")
    e = load(plan_engine("race", precision, 2), sc)
    e.run_closed_loop(1)
    check_costs(e, runs, precision, race=True)
    assert ", true, 4, " in e.rollout_kernel()


def crowd_scene(T, B):
    """The arc scene with B - 3 more robots on parallel lanes 10 m apart, out of everybody's reach (TRAVEL = 3 m): a table of
    B (T + 1) points"""
    sc = pc.arc_scene(T, False)
    lanes = 20.0 + 10.0 * np.arange(B - 3)
    refs = sc["refs"] + [fc.line((0.0, y), (10.0, y)) for y in lanes]
    x0 = np.concatenate([sc["x0"], np.stack([np.array([0.1, y - 0.05, 0.02]) for y in lanes])])
    return dict(refs=refs, x0=x0, u=np.concatenate([sc["u"], np.repeat(sc["u"][:1], B - 3, axis=0)]), model="diff")


# (T + 1 = 129 points per agent.  f32: 38 agents = 4902 points, staged; 39 = 5031 and 66: memory.  f64: 7 agents = 903 points,
# staged; 8 = 1032 and 66: memory)
@pytest.mark.parametrize("precision,B", [("f32", 38), ("f32", 39), ("f32", 66), ("f64", 7), ("f64", 8), ("f64", 66)])
def test_costs_in_a_crowd(precision, B):
    T, Kc = 128, 64
    sc = crowd_scene(T, B)
    eps = device_noise("diff", B, T, 1, K=Kc)[0]
    runs = pc.one_iteration(sc, eps, Kc, T)
    e = load(plan_engine("diff", precision, B, T, K=Kc), sc)
    e.run_closed_loop(1)
    # (f64: every agent's costs; f32: the lanes' coordinates reach 650 m, where a tracking error of centimetres is a few
    # spacings: the lanes are held to the reference's hits)
    check_costs(e, runs if precision == "f64" else runs[:3], precision)
    hits = mc.penalised(e.costs())
    assert hits[0].any() and not hits[3:].any()
    assert np.array_equal(hits[3:], np.stack([mc.penalised(np.asarray(r["S"])) for _, r in runs[3:]]))


# ------------------------------------------------------------------------------------------ 4. closed loop
LOOP_T, LOOP_N = 20, 6


@functools.lru_cache(maxsize=None)
def loop_reference():
    sc = pc.arc_scene(LOOP_T, True)
    ring = device_noise("diff", 3, LOOP_T, LOOP_N, accumulate=True, **LOOP_W)
    return sc, pc.closed_loop(sc, lambda i: ring[i], LOOP_N, K, LOOP_T, own=pc.arc_own(sc), accumulate=True, **mc.LOOP_KW)


def test_closed_loop_f64_end_to_end():
    sc, ref = loop_reference()
    e = load(plan_engine("diff", "f64", 3, LOOP_T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
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
    e = load(plan_engine("diff", "f32", 3, LOOP_T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
    us = list(ref["u_start"]) + [ref["u"]]
    for i in range(LOOP_N):
        e.set_state(ref["x"][i])
        e.set_u_prev(us[i])
        e.set_iteration(i)
        e.run_closed_loop(1)
        S = e.costs()
        for a in range(3):
            keep = ref["kept"][i][a]
            assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(ref["S"][i][a])[keep]), (i, a)
            np.testing.assert_allclose(S[a][keep], ref["S"][i][a][keep], rtol=2e-4, atol=2e-4, err_msg=f"iteration {i}, agent {a}")
        if ref["kept"][i].all():
            assert float(np.sqrt(np.mean((e.get_u_prev() - us[i + 1]) ** 2))) <= 1e-4
            np.testing.assert_allclose(e.get_state(), ref["x"][i + 1], rtol=0, atol=0.1 * np.sqrt(2 * LOOP_T * 3) * 1e-4)
    print("kept per iteration and agent", ref["kept"].mean(axis=2).tolist())
    assert ref["kept"].mean(axis=2).min() >= 1.0 - mc.MAX_LEFT_OUT


# ------------------------------------------------------------------------------------------ 5. bitwise
def same(a, b, clearance=True):
    pairs = [(a.get_state(), b.get_state()), (a.get_u_prev(), b.get_u_prev()), (a.costs(), b.costs())]
    if clearance:
        pairs += list(zip(a.fleet_clearance(), b.fleet_clearance()))
    return all(np.array_equal(x, y) for x, y in pairs)


def test_graph_replay_equals_eager(monkeypatch):
    slots = 4
    n = 2 * slots + 3
    T = 8
    sc = pc.arc_scene(T, True)
    eager = load(plan_engine("diff", "f32", 3, T, accumulate=True, K=64, **LOOP_W), sc)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    monkeypatch.setenv("MPPI_GRAPH_SLOTS", str(slots))
    graph = load(plan_engine("diff", "f32", 3, T, accumulate=True, K=64, **LOOP_W), sc)
    eager.run_closed_loop(n)
    graph.run_closed_loop(n)
    assert graph.stats.iteration == n
    assert same(graph, eager)
    assert np.array_equal(graph.fleet_plans(), eager.fleet_plans())
    for h in (graph, eager):  # (the plan launch is in neither launch class)
        cnt = h.counters()
        assert (cnt["iterations"], cnt["rollout_launches"], cnt["finalize_launches"]) == (n, n, n)


def test_one_call_equals_one_iteration_calls():
    T = 20
    sc = pc.arc_scene(T, True)
    a = load(plan_engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
    b = load(plan_engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
    a.run_closed_loop(9)
    for _ in range(9):
        b.run_closed_loop(1)
    assert same(a, b)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_far_apart_fleet_in_plan_mode_equals_the_handle_without(precision):
    B, T = 5, 20
    sc = fc.far_scene(B, T)
    own = fc.far_own(sc)
    on = load(plan_engine("diff", precision, B, T), sc, own)
    off = load(engine("diff", precision, B, T, fleet=False), sc, own)
    hits = 0
    for _ in range(5):
        on.run_closed_loop(1)
        off.run_closed_loop(1)
        assert np.array_equal(on.costs(), off.costs())
        hits += int(mc.penalised(on.costs()).sum())
    assert same(on, off, clearance=False) and hits > 0
    assert ", true, 4, " in on.rollout_kernel() and ", true, 3, " in off.rollout_kernel()


def test_switching_back_equals_the_handle_that_never_switched():
    T = 20
    sc = pc.arc_scene(T, True)
    a = load(engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
    b = load(engine("diff", "f32", 3, T, accumulate=True, **LOOP_W), sc, pc.arc_own(sc))
    a.run_closed_loop(2)
    b.run_closed_loop(2)
    a.set_fleet_prediction("plan")
    a.fleet_plans()
    a.eval_is_collided(np.zeros((4, 3)))
    a.set_fleet_prediction("velocity")
    a.run_closed_loop(3)
    b.run_closed_loop(3)
    assert same(a, b)
    for agent in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(a.agent_circles(agent), b.agent_circles(agent)))
    assert a.rollout_kernel() == b.rollout_kernel() and ", true, 3, " in a.rollout_kernel()


# ------------------------------------------------------------------------------------------ 6. clearance
def test_clearance_against_the_hosts_recomputation():
    T = 20
    sc = fc.contact_scene(T)
    e = load(plan_engine("diff", "f64", 3, T), sc)
    twin = load(plan_engine("diff", "f64", 3, T), sc)
    e.run_closed_loop(8)
    starts = []
    for _ in range(8):
        starts.append(twin.get_state())
        twin.run_closed_loop(1)
    dist = np.array([fc.min_mate_distance(x) for x in starts])
    d, n = e.fleet_clearance()
    assert np.all(np.abs(d - dist.min(axis=0)) <= 4 * np.spacing(dist.min(axis=0)))
    assert np.array_equal(n, (dist < 2 * fc.RADIUS).sum(axis=0)) and n[0] >= 1 and n[1] >= 1 and n[2] == 0
    # the refreshes in front of the read-back and mppi_eval_* do not count
    e.fleet_plans()
    e.eval_is_collided(np.zeros((4, 3)))
    e.eval_is_collided(np.zeros((4, 3)), steps=[0, 1, 2, 3])
    e.eval_cost(np.zeros((4, 3)), 0)
    d3, n3 = e.fleet_clearance(reset=True)
    assert np.array_equal(d, d3) and np.array_equal(n, n3)
    e.run_closed_loop(1)
    d5, n5 = e.fleet_clearance()
    assert np.all(np.isfinite(d5)) and n5.max() <= 1


# ------------------------------------------------------------------------------------------ 7. refusals on a live handle
def test_refusals_on_a_live_handle():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 20
    sc = pc.arc_scene(T, True)
    e = load(engine("diff", "f32", 3, T), sc)
    assert e.lib.mppi_set_fleet_prediction(e._h, 2) == capi.ERR_BAD_ARG
    assert e.lib.mppi_set_fleet_prediction(e._h, -1) == capi.ERR_BAD_ARG
    with pytest.raises(pkg.MppiError) as ex:
        e.set_fleet_prediction("acceleration")
    assert ex.value.code == capi.ERR_BAD_ARG
    with pytest.raises(pkg.MppiError) as ex:
        e.fleet_plans()  # velocity mode
    assert ex.value.code == capi.ERR_STATE
    plain = load(engine("diff", "f32", 3, T, fleet=False), sc)
    with pytest.raises(pkg.MppiError) as ex:
        plain.set_fleet_prediction("plan")
    assert ex.value.code == capi.ERR_STATE and "fleet_radius" in str(ex.value)


# ------------------------------------------------------------------------------------------ behaviour (figures only)
def test_arc_closed_loop_distances_are_reported():
    """The smallest distance of agent 0 to a mate over a closed loop on the arc scene under plans and under constant velocity.
    The CPU reference loops show no ordering that holds across horizons, so nothing is asserted beyond both
    runs finishing; the figures go to the log."""
    Kb, T, n = 512, 20, 30
    sc = pc.arc_scene(T, True)
    smallest = {}
    for mode in ("velocity", "plan"):
        e = load(engine("diff", "f32", 3, T, accumulate=True, K=Kb, **LOOP_W), sc)
        e.set_fleet_prediction(mode)
        e.run_closed_loop(n)
        smallest[mode] = float(e.fleet_clearance()[0][0])
    print(f"fleet plan behaviour arc smallest distance velocity {smallest['velocity']:.4f} plan {smallest['plan']:.4f}")
    assert all(np.isfinite(v) for v in smallest.values())
