"""Learned-dynamics fleets on the device (mppi_config.obstacle_motion = 3): the mates' rows and the plans the
k_fleet_plan_mlp_* kernels write, against the f64 reference and the margin rule of tests/mlp_fleet_checks.py; what the collision
test, one iteration (the fleet forms of the batched scene kernels) and the closed loop make of them; what must stay bit for bit;
the refusals.  B = 3 and K = 250 (three full 64-sample tiles and a ragged one) unless stated; T = 7 or 50."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import fleet_plan_checks as fp
import mlp_fleet_checks as mf
import mlp_scene_checks as ms
import moving_obstacle_checks as mc
from test_gpu_agent_scenes import diff_cfg
from test_gpu_fleet import MODES, compare_rows, own_sets, rows_scene

pytestmark = pytest.mark.gpu

K = mf.K


def engine(T, mode="frozen", accumulate=False, B=3, K=K, motion=3, **kw):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    cfg = dict(diff_cfg(getattr(capi, MODES[mode]), T, precision=capi.PREC_F32), accumulate_stage_cost=int(accumulate),
               filter_window=mc.filter_window(T), model=capi.MODEL_DIFFDRIVE_MLP, obstacle_motion=motion, n_agents=B,
               fleet_radius=fc.RADIUS if motion == 3 else 0.0)
    cfg.update(kw)
    return pkg.Engine(K=K, **cfg)


def load(e, sc, own=None, shared=None, what="velocity"):
    if sc.get("per_agent", True) and "w" in sc:
        for a, w in enumerate(sc["w"]):
            e.set_mlp(w, agent=a)
    elif "w" in sc:
        e.set_mlp(sc["w"][0])
    for a, ref in enumerate(sc["refs"]):
        e.set_ref_path(ref, agent=a)
    if shared is not None:
        e.set_obstacles(shared[0], velocities=shared[1])
    for a, (c, v) in enumerate(own or []):
        e.set_obstacles(c, agent=a, velocities=v)
    e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    if what == "plan":
        e.set_fleet_prediction("plan")
    return e


def fleet_kernel(H, n):
    return "k_rollout_mlp_h3_fleet_agents" if (H, n) in ((512, 3), (512, 2)) else f"k_rollout_mlp_w_fleet_agents<{H}>"


def device_noise(e, n_iters):
    """What the handle's sampler draws for iterations 0 .. n_iters - 1 ([B, K, T, 2] each), held to oracle/philox.py first"""
    out = []
    for i in range(n_iters):
        got = e.sample_epsilon(i).cpu().numpy()
        want = fc.numpy_noise(mc.DIFF_KW["sigma"], int(e.cfg.seed), i, e.n_agents, e.K, e.T, int(e.cfg.noise_stream))
        np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)
        out.append(got)
    return out


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, float) - np.asarray(b, float)) ** 2)))


# ------------------------------------------------------------------------------------------ 1. the rows (velocity mode)
@pytest.mark.parametrize("own", ["none", "shared", "per_agent"])
@pytest.mark.parametrize("B", [2, 3, 66])
def test_rows_against_the_reference(B, own):
    """k_fleet_rows<float> behind the agents' own rows, held to fleet_checks' f32 error model; B = 66: 65 mate rows, the path
    beyond the lane table"""
    sc = rows_scene("diff", B)
    sc = dict(sc, w=[ms.weights(64, 1, 100)], per_agent=False)
    shared, per, owned = own_sets(own, B)
    e = load(engine(20, B=B, K=64 if B == 66 else K), sc, per, shared)
    agents = range(B) if B <= 5 else (0, 1, 33, 64, 65)
    worst = compare_rows(e, "diff", owned, 0, agents, "f32")  # clock 0
    before = [e.agent_circles(b) for b in agents]
    e.set_iteration(5)  # replays noise: nothing moves at step 0
    for (c0, v0), b in zip(before, agents):
        c1, v1 = e.agent_circles(b)
        assert np.array_equal(c0, c1) and np.array_equal(v0, v1)
    e.run_closed_loop(3)  # clock 3
    assert e.rollout_kernel() == fleet_kernel(64, 1)
    worst = max(worst, compare_rows(e, "diff", owned, 3, agents, "f32"))
    for b in agents:
        assert e.agent_circles(b)[0].shape[0] == len(owned[b][0]) + B - 1
    print(f"learned fleet rows B={B} own={own} max error / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ 2. the plans read back
def plan_scene(B, T, H, n, per_agent):
    """The side scene's agents (the geometry the state error was measured on: 3 m of travel near the origin) with nominal
    controls partly beyond the clamp: four rows ask for 7 m/s and +-4 rad/s"""
    sc = mf.side_scene(T, H, n, per_agent)
    u = sc["u"][:B].copy()
    for a in range(B):
        u[a, 1 % T] = (7.0, 4.0)
        u[a, T // 2] = (-7.0, -4.0)
        u[a, T - 1] = (7.0, -4.0 if a else 4.0)
    return dict(refs=sc["refs"][:B], x0=sc["x0"][:B], u=u, w=sc["w"][:B], per_agent=per_agent, shape=(H, n), model="diff")


def plan_error(e, sc):
    """largest distance of a point read back from learned_plans of the handle's states and controls, in units of DELTA"""
    got, want = e.fleet_plans(), mf.learned_plans(e.get_state(), e.get_u_prev(), sc["w"])
    assert got.shape == want.shape == (len(sc["w"]), e.T + 1, 2)
    return float(np.sqrt(((got - want) ** 2).sum(axis=2)).max() / ms.delta())


PLAN_CASES = [(B, T, H, n, pa) for B in (2, 3) for T in (7, 50) for (H, n) in ((64, 1), (128, 2)) for pa in (False, True)]
PLAN_CASES.append((3, 50, 512, 3, True))


@pytest.mark.parametrize("B,T,H,n,per_agent", PLAN_CASES)
def test_plans_against_the_reference(B, T, H, n, per_agent):
    sc = plan_scene(B, T, H, n, per_agent)
    e = load(engine(T, B=B), sc, what="plan")
    worst = plan_error(e, sc)  # clock 0
    e.run_closed_loop(3)  # the states and the nominal controls have moved on
    worst = max(worst, plan_error(e, sc))
    rng = np.random.default_rng(B + T)
    e.set_state(sc["x0"] + rng.normal(0, 0.2, sc["x0"].shape))
    worst = max(worst, plan_error(e, sc))
    e.set_u_prev(sc["u"][::-1] * 0.5)
    worst = max(worst, plan_error(e, sc))
    print(f"learned fleet plans B={B} T={T} {H}x{n} per_agent={per_agent} max error / DELTA {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------ 3. per-pose evaluation
@pytest.mark.parametrize("what", ["plan", "velocity"])
def test_eval_is_collided_at_a_mates_predicted_centre(what):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 20
    sc = mf.side_scene(T, 64, 1, True)
    e = load(engine(T, accumulate=True), sc, what=what)
    e.run_closed_loop(2)
    x, u = e.get_state(), e.get_u_prev()
    if what == "plan":
        centres = mf.learned_plans(x, u, sc["w"])[1]  # agent 1 as agent 0 sees it
    else:
        mate_c, mate_v = fc.mate_rows(x, u[:, 0], "diff", fc.rows_cfg("diff"))
        centres = mate_c[0][0][:2] + mate_v[0][0] * (mf.DT * np.arange(T + 1))[:, None]
    poses, steps, want = [], [], []
    for j in (0, 1, T // 2, T):
        for k, ang in enumerate(np.linspace(0.0, 2 * np.pi, 7)[:-1] + 0.1 * j):
            for inside in (True, False):
                d = mf.THR * (1.0 - 1e-3 if inside else 1.0 + 1e-3)
                poses.append([*(centres[j] + d * np.array([np.cos(ang), np.sin(ang)])), 0.3 * k])
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    poses, steps, want = np.array(poses), np.array(steps, dtype=np.int32), np.array(want)
    got = e.eval_is_collided(poses, steps=steps)
    assert np.array_equal(got, want), (got, want, steps)
    assert np.array_equal(e.eval_is_collided(poses)[steps == 0], want[steps == 0])
    if what == "plan":
        with pytest.raises(pkg.MppiError) as ex:
            e.eval_is_collided(poses[:2], steps=np.array([T, T + 1], dtype=np.int32))
        assert ex.value.code == capi.ERR_BAD_ARG
        assert e.agent_circles(0)[0].shape[0] == 0
    e.set_state(e.get_state() + 50.0)  # the mates move away with the states
    assert not e.eval_is_collided(poses, steps=steps).any()


@pytest.mark.parametrize("what", ["plan", "velocity"])
def test_eval_is_collided_at_with_the_outline_model(what):
    """MPPI_OBSTACLE_OUTLINE: the mates against the vehicle's outline, half extents 0.5 vehicle_l safety_margin and 0.5 vehicle_w
    safety_margin, threshold fleet_radius -- front-centre, side-centre and corner points of the outline 1e-3 inside / outside a
    mate's predicted centre"""
    from dnn_mppi_mpc_amd import _capi as capi
    T, vl, vw, margin = 20, 0.8, 0.5, 0.8
    sc = mf.side_scene(T, 64, 1, True)
    e = load(engine(T, accumulate=True, obstacle_model=capi.OBSTACLE_OUTLINE, vehicle_l=vl, vehicle_w=vw, safety_margin=margin), sc, what=what)
    e.run_closed_loop(2)
    x, u = e.get_state(), e.get_u_prev()
    if what == "plan":
        centres = mf.learned_plans(x, u, sc["w"])[1]
    else:
        mate_c, mate_v = fc.mate_rows(x, u[:, 0], "diff", fc.rows_cfg("diff"))
        centres = mate_c[0][0][:2] + mate_v[0][0] * (mf.DT * np.arange(T + 1))[:, None]
    ha, hb, thr = 0.5 * vl * margin, 0.5 * vw * margin, fc.RADIUS
    poses, steps, want = [], [], []
    for j in (0, 1, T // 2, T):
        for k, (bx, by) in enumerate([(ha, 0.0), (0.0, hb), (ha, hb), (-ha, 0.0), (0.0, -hb), (-ha, -hb)]):
            yaw = 0.4 * k + 0.1 * j
            cs, sn = np.cos(yaw), np.sin(yaw)
            out = np.array([bx, by]) / np.hypot(bx, by)  # the outline point lies on the body-frame ray from the pose to the mate
            for inside in (True, False):
                body = np.array([bx, by]) + thr * (1.0 - 1e-3 if inside else 1.0 + 1e-3) * out  # the mate's centre in the body frame
                world = np.array([body[0] * cs - body[1] * sn, body[0] * sn + body[1] * cs])
                poses.append([*(centres[j] - world), yaw])
                steps.append(j)
                want.append(1.0 if inside else 0.0)
    got = e.eval_is_collided(np.array(poses), steps=np.array(steps, dtype=np.int32))
    assert np.array_equal(got, np.array(want)), (got, want)


# ------------------------------------------------------------------------------------------ 4. one iteration, every agent's costs
@functools.lru_cache(maxsize=None)
def reference(T, accumulate, mode, H, n, per_agent, what, with_own=False):
    sc = mf.scene_of(T, accumulate, H, n, per_agent, what)
    own = mf.arc_own(sc) if with_own else None
    probe = engine(T, mode, accumulate)
    eps = device_noise(probe, 1)[0]
    probe.close()
    return sc, own, mf.one_iteration(sc, eps, T, mode, accumulate, what, own)


def check_costs(e, sc, runs, own=False):
    S, u = e.costs(), e.get_u_prev()
    assert e.rollout_kernel() == fleet_kernel(*sc["shape"])
    for a, (o, res) in enumerate(runs):
        S_ref, keep = np.asarray(res["S"], np.float64), mf.kept(o)
        hit_ref = mc.penalised(S_ref)
        err_u = rmse(u[a], res["u_returned"])
        print("agent", a, e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u,
              "weight left out", float(res["w"][~keep].max(initial=0.0)))
        assert keep.mean() >= 1.0 - mf.MAX_LEFT_OUT
        assert np.array_equal(mc.penalised(S[a])[keep], hit_ref[keep])  # the hit set, exact outside the margin
        np.testing.assert_allclose(S[a][keep], S_ref[keep], rtol=1e-3, atol=1e-3)
        if res["w"][~keep].max(initial=0.0) <= 1e-6:
            assert err_u <= 1e-4
    assert e.stats.n_collided == int((S[0] >= 1.0e10).sum())  # (without own circles: agent 0's mates alone fill the count)
    return S


# plan mode: every case; velocity mode: the 64 x 1 cases (frozen and per-rollout) and 512 x 3 once
COST_CASES = [(c, "plan") for c in mf.cases()] + [(c, "velocity") for c in mf.cases() if c[3:5] in ((64, 1), (512, 3))]


@pytest.mark.parametrize("case,what", COST_CASES, ids=str)
def test_costs_of_every_agent(case, what):
    T, accumulate, mode, H, n, per_agent = case
    sc, _, runs = reference(T, accumulate, mode, H, n, per_agent, what)
    e = load(engine(T, mode, accumulate), sc, what=what)
    e.run_closed_loop(1)
    S = check_costs(e, sc, runs)
    hits = mc.penalised(S)
    assert hits[:2].any() and not hits[:2].all()


@pytest.mark.parametrize("what", ["plan", "velocity"])
def test_costs_with_own_moving_circles(what):
    sc, own, runs = reference(50, True, "frozen", 64, 1, True, what, True)
    e = load(engine(50, "frozen", True), sc, own, what=what)
    e.run_closed_loop(1)
    check_costs(e, sc, runs)


@functools.lru_cache(maxsize=None)
def outline_reference(accumulate, what):
    sc = mf.outline_scene(50)
    probe = engine(50, "frozen", accumulate)
    eps = device_noise(probe, 1)[0]
    probe.close()
    return sc, mf.one_iteration(sc, eps, 50, "frozen", accumulate, what)


@pytest.mark.parametrize("what", ["plan", "velocity"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_costs_with_the_outline_model(accumulate, what):
    """MPPI_OBSTACLE_OUTLINE in the rollout: the eight outline points of every priced state -- the learned yaw -- against the mates,
    threshold fleet_radius; the margin is delta(outline) + delta() (mlp_fleet_checks)"""
    import grid_footprint_checks as gf
    from dnn_mppi_mpc_amd import _capi as capi
    sc, runs = outline_reference(accumulate, what)
    e = load(engine(50, "frozen", accumulate, obstacle_model=capi.OBSTACLE_OUTLINE, **gf.DIFF_BOX), sc, what=what)
    e.run_closed_loop(1)
    hits = mc.penalised(check_costs(e, sc, runs))
    assert hits[0].any() and not hits[0].all()


def test_costs_with_tracks_and_a_grid_beside_the_plans():
    """composed mode: agent 0 prices its own circles, its tracks, its grid and its mates' plans; agents 1 and 2 their mates alone"""
    T = 50
    sc = mf.composed_scene()
    ing = sc["ingredients"]
    e = engine(T, "frozen", True)
    e.set_scene_mode("composed")
    load(e, sc, [(ing["circles"], ing["vel"])])
    e.set_obstacle_tracks(ing["tracks"], ing["radii"], agent=0)
    e.set_cost_grid(**ing["grid"].kwargs, agent=0)
    e.set_fleet_prediction("plan")
    runs = mf.composed_iteration(sc, device_noise(e, 1)[0])
    e.run_closed_loop(1)
    S, u = e.costs(), e.get_u_prev()
    assert e.rollout_kernel() == fleet_kernel(64, 1)
    for a, (o, res) in enumerate(runs):
        S_ref, keep = np.asarray(res["S"], np.float64), ms.kept(o) if a == 0 else mf.kept(o)
        print("agent", a, "kept", keep.mean(), "penalised", mc.penalised(S_ref).mean(), "u rmse", rmse(u[a], res["u_returned"]))
        assert keep.mean() >= 1.0 - mf.MAX_LEFT_OUT
        assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(S_ref)[keep])
        np.testing.assert_allclose(S[a][keep], S_ref[keep], rtol=1e-3, atol=1e-3)
        if res["w"][~keep].max(initial=0.0) <= 1e-6:
            assert rmse(u[a], res["u_returned"]) <= 1e-4
    assert e.stats.n_collided == int((S[0] >= 1.0e10).sum())
    assert mc.penalised(S[1]).any() and not mc.penalised(S[1]).all()  # agent 1 owns nothing: its mates alone


# ------------------------------------------------------------------------------------------ 5. closed loop
@pytest.mark.parametrize("what", ["plan", "velocity"])
def test_closed_loop_iteration_by_iteration(what):
    """Four iterations of three robots, each re-seeded from the CPU loop (a flipped near-threshold sample of one iteration decides
    no later one); the clearance record against the host's recomputation"""
    T, n_it = 50, 4
    sc = mf.side_scene(T, 64, 1, True)
    own = None  # (the mates alone decide: 0.8 / 0.3 of agent 0's samples in the first iteration)
    e = load(engine(T, "frozen", True), sc, own, what=what)
    ring = device_noise(e, n_it)
    ref = mf.closed_loop(sc, lambda i: ring[i], n_it, T, what, own, accumulate=True)
    us = list(ref["u_start"]) + [ref["u"]]
    for i in range(n_it):
        e.set_state(ref["x"][i])
        e.set_u_prev(us[i])
        e.set_iteration(i)
        e.run_closed_loop(1)
        S = e.costs()
        for a in range(3):
            keep = ref["kept"][i][a]
            assert keep.mean() >= 1.0 - mf.MAX_LEFT_OUT
            assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(ref["S"][i][a])[keep]), (i, a)
            np.testing.assert_allclose(S[a][keep], ref["S"][i][a][keep], rtol=1e-3, atol=1e-3, err_msg=f"iteration {i}, agent {a}")
        if ref["kept"][i].all():
            assert rmse(e.get_u_prev(), us[i + 1]) <= 1e-4
    dist = np.array([fc.min_mate_distance(x) for x in ref["x"][:n_it]])
    d, n = e.fleet_clearance()
    assert np.all(np.abs(d - dist.min(axis=0)) <= 4 * np.spacing(dist.min(axis=0)))
    assert np.array_equal(n, (dist < 2 * fc.RADIUS).sum(axis=0))


# ------------------------------------------------------------------------------------------ 6. bitwise
def same(a, b, clearance=True):
    pairs = [(a.get_state(), b.get_state()), (a.get_u_prev(), b.get_u_prev()), (a.costs(), b.costs())]
    if clearance:
        pairs += list(zip(a.fleet_clearance(), b.fleet_clearance()))
    return all(np.array_equal(x, y) for x, y in pairs)


@pytest.mark.parametrize("what", ["plan", "velocity"])
@pytest.mark.parametrize("H,n", [(64, 1), (512, 3)])
def test_far_apart_fleet_equals_the_value_2_batch(H, n, what):
    B, T = 4, 20
    sc = mf.far_scene(B, T, H, n)
    own = fc.far_own(sc)
    on = load(engine(T, B=B), sc, own, what=what)
    off = load(engine(T, B=B, motion=2), sc, own)
    hits = 0
    for _ in range(3):
        on.run_closed_loop(1)
        off.run_closed_loop(1)
        assert np.array_equal(on.costs(), off.costs())
        hits += int(mc.penalised(on.costs()).sum())
    assert same(on, off, clearance=False) and hits > 0
    assert on.rollout_kernel() == fleet_kernel(H, n) and "_scene_agents" in off.rollout_kernel()


def test_switching_back_equals_the_handle_that_never_switched():
    T = 20
    sc = mf.side_scene(T, 64, 1, True)
    a = load(engine(T, accumulate=True), sc, mf.arc_own(sc))
    b = load(engine(T, accumulate=True), sc, mf.arc_own(sc))
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
    assert a.rollout_kernel() == b.rollout_kernel() == fleet_kernel(64, 1)


@pytest.mark.parametrize("what", ["plan", "velocity"])
def test_graph_replay_equals_eager_and_one_call_equals_n_calls(what, monkeypatch):
    slots, T = 4, 8
    n = 2 * slots + 3
    sc = mf.side_scene(T, 64, 1, True)
    eager = load(engine(T, accumulate=True, K=64), sc, what=what)
    single = load(engine(T, accumulate=True, K=64), sc, what=what)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    monkeypatch.setenv("MPPI_GRAPH_SLOTS", str(slots))
    graph = load(engine(T, accumulate=True, K=64), sc, what=what)
    eager.run_closed_loop(n)
    graph.run_closed_loop(n)
    for _ in range(n):
        single.run_closed_loop(1)
    assert graph.stats.iteration == n
    assert same(graph, eager) and same(single, eager)
    if what == "plan":
        assert np.array_equal(graph.fleet_plans(), eager.fleet_plans())
    for h in (graph, eager):  # (the launch at the front of the slot is in neither launch class)
        cnt = h.counters()
        assert (cnt["iterations"], cnt["rollout_launches"], cnt["finalize_launches"]) == (n, n, n)


# ------------------------------------------------------------------------------------------ 7. refusals on a live handle
def test_refusals_on_a_live_handle():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 20
    sc = mf.far_scene(3, T)
    e = engine(T)
    for a, ref in enumerate(sc["refs"]):
        e.set_ref_path(ref, agent=a)
    e.set_fleet_prediction("plan")
    with pytest.raises(pkg.MppiError) as ex:  # the plans run through the agents' models: none yet
        e.fleet_plans()
    assert ex.value.code == capi.ERR_STATE and "model" in str(ex.value)
    e = load(e, sc)
    e.set_fleet_prediction("velocity")
    with pytest.raises(pkg.MppiError) as ex:
        e.fleet_plans()  # velocity mode
    assert ex.value.code == capi.ERR_STATE
    assert e.lib.mppi_set_fleet_prediction(e._h, 2) == capi.ERR_BAD_ARG
    grid = ms.scene("grid", 50, False)["grid"]
    with pytest.raises(pkg.MppiError) as ex:  # the analytic fleet handles' exclusivity: a grid needs the composed mode
        e.set_cost_grid(**grid.kwargs)
    assert ex.value.code == capi.ERR_UNSUPPORTED
    big = dict(sc["w"][0])
    big["input_layer.weight"] = big["input_layer.weight"].copy()
    big["input_layer.weight"][0, 0] = 1.0e5  # beyond the f16 range: the f32-input kernel has no scene form
    with pytest.raises(pkg.MppiError) as ex:
        e.set_mlp(big)
    assert ex.value.code == capi.ERR_UNSUPPORTED
    plain = load(engine(T, motion=2), sc)
    with pytest.raises(pkg.MppiError) as ex:
        plain.set_fleet_prediction("plan")
    assert ex.value.code == capi.ERR_STATE and "fleet_radius" in str(ex.value)
