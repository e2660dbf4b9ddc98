"""Composed scenes on the device (mppi_set_scene_mode): a cost grid, obstacle tracks and the mates' plans on one
handle -- the SPEC 7 rollout forms and k_eval_pose -- against the f64 reference of tests/scene_checks.py (the oracles of the
three features composed: nothing new is computed there), the LDS layout on either side of its budget, what must stay bit for
bit, a closed loop with a rolling costmap and ticking tracks, and the switch.  K = 256 throughout; the tolerances, the margin
rule and the loop's bars are those of test_gpu_cost_grid.py / test_gpu_fleet.py."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import fleet_plan_checks as pc
import moving_obstacle_checks as mc
import scene_checks as sk
import test_gpu_fleet as tf
from test_gpu_agent_scenes import diff_cfg
from test_gpu_moving_obstacles import cuda, diff_engine, race_engine

pytestmark = pytest.mark.gpu

K = sk.K_CASE


def kernel(e):
    name = e.rollout_kernel()
    assert name.startswith("k_rollout_fused<"), name
    return name


def spec_of(e):
    return kernel(e).split(", ")[4]


def give(e, ing, agent=None):
    """one agent's tracks and grid (absent: not called at all)"""
    if ing.get("tracks") is not None:
        e.set_obstacle_tracks(ing["tracks"], ing["radii"], agent=agent)
    if ing.get("grid") is not None:
        e.set_cost_grid(**ing["grid"].kwargs, agent=agent)


def load_single(e, sc, composed=True):
    """the scene's path, circles, tracks and grid; sc["clock"] iterations later, with state, controls and index as given"""
    if composed:
        e.set_scene_mode("composed")
    e.set_ref_path(sc["ref"])
    e.set_obstacles(sc["circles"], velocities=sc["vel"])
    give(e, sc)
    if sc.get("clock"):
        e.set_state(sc["x0"])
        e.run_closed_loop(sc["clock"])
        e.set_waypoint_idx(0)
        e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    return e


def fleet_engine(sc, precision, T, mode="frozen", accumulate=False, model="diff", **kw):
    B = len(sc["refs"])
    return tf.engine(model, precision, B, T, mode, accumulate, fleet=sc["plans"], **kw)


def load_fleet(e, sc, composed=True):
    if composed:
        e.set_scene_mode("composed")
    tf.load(e, sc, [(p.get("circles", np.zeros((0, 3))), p.get("vel", np.zeros((0, 2)))) for p in sc["per"]])
    if sc["plans"]:
        e.set_fleet_prediction("plan")
    for a, ing in enumerate(sc["per"]):
        give(e, ing, agent=a)
    if sc.get("clock"):
        e.run_closed_loop(sc["clock"])
        e.set_waypoint_idx(0)
        e.set_state(sc["x0"])
        e.set_u_prev(sc["u"])
    return e


# ------------------------------------------------------------------------------------------ 1. one iteration
@functools.lru_cache(maxsize=None)
def single_reference(*case):
    return sk.single_case(*case)


def check_iteration(e, sc, eps, o, res, precision, sequential=False, f32_reference=False, multi="false"):
    """test_gpu_cost_grid.check_iteration for the composed form"""
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = sk.kept(o, precision == "f64" and not f32_reference)
    hit_ref = sk.penalised(S_ref)
    err_u = float(np.sqrt(np.mean((u - res["u_returned"]) ** 2)))
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "max rel S err", float(np.max(np.abs(S[keep] - S_ref[keep]) / np.maximum(np.abs(S_ref[keep]), 1.0))))
    assert keep.mean() >= 1.0 - sk.MAX_LEFT_OUT
    assert np.array_equal(sk.penalised(S)[keep], hit_ref[keep])  # no flip outside the margin
    assert st.n_collided == int((S >= 1.0e10).sum())
    if precision == "f64" and not f32_reference:
        np.testing.assert_allclose(S, S_ref, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == int((S_ref >= 1.0e10).sum())
    else:
        assert np.all(np.abs(S[keep] - S_ref[keep]) <= sk.f32_tolerance(S_ref[keep]))
        assert err_u <= 1e-4
    if sequential:
        assert st.rounds >= 1 and st.idx_after == res["idx_after"] and res["idx_after"] > res["idx_start"]
    assert kernel(e).endswith(f", {multi}, 7, false>"), kernel(e)
    return st


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("case", sk.single_cases(), ids=str)
def test_grid_and_tracks_on_one_agent(case, precision):
    T, accumulate, mode = case[:3]
    sc, eps, o, res = single_reference(*case)
    e = load_single(diff_engine(T, mode, accumulate, precision), sc)
    check_iteration(e, sc, eps, o, res, precision, sequential=mode == "sequential")
    assert kernel(e).split(", ")[2] == ("1" if T <= 64 else "2")


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("clock", [0, 3])
def test_race_car_with_a_grid_and_a_track(clock, precision):
    sc, eps, o, res = sk.race_case(clock)
    e = load_single(race_engine(precision), sc)
    check_iteration(e, sc, eps, o, res, precision, f32_reference=True)  # (the reference itself is f32)


@functools.lru_cache(maxsize=None)
def fleet_reference(*case):
    T, accumulate, mode, what, clock, extra = case
    sc = sk.fleet_scene(T, accumulate, what, clock, extra)
    seed = sk.fleet_seed(*case)
    noise = tf.engine("diff", "f32", 3, T, mode, accumulate, seed=seed)
    eps = noise.sample_epsilon(clock).cpu().numpy()  # (what the kernels draw at iteration `clock`)
    noise.close()
    np.testing.assert_allclose(eps, sk.fleet_noise(seed, clock, K, T), rtol=0, atol=4e-6)
    return sc, seed, sk.fleet_iteration(sc, eps, K, T, mode, accumulate)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("case", sk.fleet_cases(), ids=str)
def test_batches_of_three(case, precision):
    """agent 0 holds everything the case has, agent 1 lacks the tracks, agent 2 lacks the grid"""
    T, accumulate, mode, what, clock, extra = case
    sc, seed, runs = fleet_reference(*case)
    e = load_fleet(fleet_engine(sc, precision, T, mode, accumulate, seed=seed), sc)
    e.run_closed_loop(1)
    tf.check_costs(e, runs, precision)
    assert kernel(e).endswith(", true, 7, false>"), kernel(e)
    S0 = e.costs()[0]
    assert e.stats.n_collided == int((S0 >= 1.0e10).sum())
    if precision == "f64":
        assert e.stats.n_collided == int((np.asarray(runs[0][1]["S"]) >= 1.0e10).sum())


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_pair(precision):
    sc = sk.race_fleet_scene()
    noise = tf.engine("race", "f32", 2, seed=sk.RACE_FLEET_SEED)
    eps = noise.sample_epsilon(0).cpu().numpy()
    noise.close()
    runs = sk.race_fleet_iteration(sc, eps, K)
    e = load_fleet(fleet_engine(sc, precision, mc.RACE_T, model="race", seed=sk.RACE_FLEET_SEED), sc)
    e.run_closed_loop(1)
    tf.check_costs(e, runs, precision, race=True)
    assert kernel(e).endswith(", true, 7, false>"), kernel(e)


# ------------------------------------------------------------------------------------------ 2. the LDS layout
def crowd(sc, B):
    """the batch with B - 3 more robots on far lanes that hold nothing (test_gpu_fleet_plan.crowd_scene): a larger plan table"""
    lanes = 20.0 + 10.0 * np.arange(B - 3)
    refs = list(sc["refs"]) + [fc.line((0.0, y), (10.0, y)) for y in lanes]
    x0 = np.concatenate([sc["x0"], np.stack([np.array([0.1, y - 0.05, 0.02]) for y in lanes])]) if B > 3 else sc["x0"]
    u = np.concatenate([sc["u"], np.repeat(sc["u"][:1], B - 3, axis=0)])
    return dict(sc, refs=refs, x0=x0, u=u, per=list(sc["per"]) + [dict() for _ in lanes])


# (precision, B, tracks of agent 0) -> what scene_lds_bytes stages at T = 128: (plans, tracks)
LDS_CASES = [("f64", 3, 4, (6192, 8288)), ("f64", 3, 5, (6192, 0)), ("f64", 8, 4, (0, 8288)), ("f64", 8, 8, (0, 0)),
             ("f32", 3, 35, (3096, 36260)), ("f32", 3, 36, (3096, 0))]


@functools.lru_cache(maxsize=None)
def lds_run(precision, B, n_tracks):
    T = 128
    sc = crowd(sk.fleet_scene(T, False, sk.INGREDIENTS, 0, 0, n_tracks=n_tracks), B)
    noise = tf.engine("diff", "f32", B, T)
    eps = noise.sample_epsilon(0).cpu().numpy()
    noise.close()
    runs = sk.fleet_iteration(sc, eps, K, T)
    e = load_fleet(fleet_engine(sc, precision, T), sc)
    e.run_closed_loop(1)
    tf.check_costs(e, runs if precision == "f64" else runs[:3], precision)  # (f32: the far lanes as test_gpu_fleet_plan.py holds them)
    assert kernel(e).endswith(", true, 7, false>")
    return e.costs(), e.get_u_prev()


@pytest.mark.parametrize("precision,B,n_tracks,staged", LDS_CASES)
def test_staging_on_either_side_of_the_budget(precision, B, n_tracks, staged):
    assert sk.scene_lds_bytes(4 if precision == "f32" else 8, B, n_tracks, 128)[:2] == staged
    lds_run(precision, B, n_tracks)


@pytest.mark.parametrize("precision,a,b", [("f64", (3, 4), (3, 5)), ("f64", (8, 4), (8, 8)), ("f64", (3, 4), (8, 4)), ("f32", (3, 35), (3, 36))])
def test_staged_and_unstaged_launches_agree_bit_for_bit(precision, a, b):
    """the scenes differ by far tracks / far robots nothing comes near: what differs is where the plans and the tracks are read"""
    (Sa, ua), (Sb, ub) = lds_run(precision, *a), lds_run(precision, *b)
    np.testing.assert_array_equal(Sa[:3], Sb[:3])
    np.testing.assert_array_equal(ua[:3], ub[:3])


# ------------------------------------------------------------------------------------------ 3. bit for bit
def state_of(e):
    return e.get_u_prev(), e.get_state(), e.costs(), int(e.stats.n_collided)


def assert_same(a, b):
    for x, y in zip(state_of(a), state_of(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_ingredient_composed_equals_exclusive_and_the_return(precision):
    T = 50
    sc = sk.diff_scene(T, True)
    parts = {"5": dict(sc, grid=None), "6": dict(sc, tracks=None), "3": dict(sc, tracks=None, grid=None)}
    for spec, part in parts.items():
        excl = load_single(diff_engine(T, "frozen", True, precision, seed=3), part, composed=False)
        comp = load_single(diff_engine(T, "frozen", True, precision, seed=3), part)
        back = load_single(diff_engine(T, "frozen", True, precision, seed=3), sc)  # both, then the other one removed again
        for h in (excl, comp, back):
            h.set_state(sc["x0"])
            h.run_closed_loop(2)
        assert spec_of(excl) == spec and spec_of(comp) == spec and spec_of(back) == "7"
        assert comp.scene_mode == "composed" and excl.scene_mode == "exclusive"
        assert_same(excl, comp)
        if part["tracks"] is None:
            back.set_obstacle_tracks(np.zeros((0, 1, 2)), [])
        if part["grid"] is None:
            back.set_cost_grid(None)
        for h in (excl, back):
            h.set_u_prev(sc["u"])
            h.set_state(sc["x0"])
            h.set_waypoint_idx(0)
            h.set_iteration(7)
            h.run_closed_loop(2)
        assert spec_of(back) == spec
        assert_same(excl, back)


def test_fleet_handle_returns_to_the_plan_form():
    T = 50
    full = sk.fleet_scene(T, False)
    bare = dict(full, per=[dict(circles=p["circles"], vel=p["vel"]) for p in full["per"]])
    excl = load_fleet(fleet_engine(bare, "f64", T), bare, composed=False)
    comp = load_fleet(fleet_engine(bare, "f64", T), bare)
    back = load_fleet(fleet_engine(full, "f64", T), full)
    for h in (excl, comp, back):
        h.run_closed_loop(2)
    assert spec_of(excl) == "4" and spec_of(comp) == "4" and spec_of(back) == "7"
    np.testing.assert_array_equal(excl.costs(), comp.costs())
    assert not np.array_equal(excl.costs(), back.costs())
    back.set_obstacle_tracks(np.zeros((0, 1, 2)), [])
    back.set_cost_grid(None)
    for h in (excl, back):
        h.set_state(full["x0"])
        h.set_u_prev(full["u"])
        h.set_waypoint_idx(0)
        h.set_iteration(7)
        h.run_closed_loop(2)
    assert spec_of(back) == "4"
    np.testing.assert_array_equal(excl.costs(), back.costs())
    np.testing.assert_array_equal(excl.get_u_prev(), back.get_u_prev())


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_replay_across_a_grid_and_a_track_re_upload(monkeypatch, precision):
    T, n_it = 50, 3
    sc = sk.diff_scene(T, True, extra=8)
    g = sc["grid"]
    moved = dict(g.kwargs, cells=np.roll(g.cells, 1, axis=1))
    later = sc["tracks"][:, 2:] + 0.05  # the same predictor two steps on: another L

    def run(e, piecewise):
        e.set_state(sc["x0"])
        for stretch in range(3):
            if stretch == 1:
                e.set_cost_grid(**moved)  # the same shape: buffers, plan and a cached graph stay
            if stretch == 2:
                e.set_obstacle_tracks(later, sc["radii"])
            for _ in range(n_it if piecewise else 1):
                e.run_closed_loop(1 if piecewise else n_it)
        return e
    eager = run(load_single(diff_engine(T, "frozen", True, precision, seed=31), sc), True)
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = run(load_single(diff_engine(T, "frozen", True, precision, seed=31), sc), False)
    assert_same(eager, graph)
    assert spec_of(graph) == "7" and eager.stats.n_collided > 0
    still = load_single(diff_engine(T, "frozen", True, precision, seed=31), sc)
    still.set_state(sc["x0"])
    still.run_closed_loop(3 * n_it)
    assert not np.array_equal(still.costs(), graph.costs())  # the re-uploads were seen


# ------------------------------------------------------------------------------------------ 4. single states
def contour_point(grid, inside, outside):
    """the point of the segment inside -> outside where g = lethal (bisection in f64)"""
    a, b = np.asarray(inside, np.float64), np.asarray(outside, np.float64)
    d = (b - a) / np.linalg.norm(b - a)  # (pointing out of the lethal side)
    assert grid.value(*a) >= grid.lethal > grid.value(*b)
    for _ in range(60):
        m = 0.5 * (a + b)
        a, b = (m, b) if grid.value(*m) >= grid.lethal else (a, m)
    return a, d


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_hit_and_cost_either_side_of_every_boundary(model, precision):
    """Agent 0 of a composed fleet handle at clock 2: poses 1e-3 m either side of a track's threshold circle, of a mate's, and
    of the grid's lethal contour, at several steps ahead -- through k_eval_pose"""
    import dnn_mppi_mpc_amd as pkg
    CLOCK = 2
    if model == "diff":
        T = 20
        sc = sk.fleet_scene(T, False, clock=0, extra=-8)
        thr_t, thr_m, reach = 0.8, float(np.sqrt(pc.threshold2("diff"))), 0.0
    else:
        T = mc.RACE_T
        sc = sk.race_fleet_scene()
        thr_t, thr_m, reach = float(sc["per"][0]["radii"][0]), float(np.sqrt(pc.threshold2("race"))), 3.0  # (the front outline point)
    e = load_fleet(fleet_engine(sc, precision, T, model=model), sc)
    e.run_closed_loop(CLOCK)
    e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    assert spec_of(e) == "7"
    ing = sc["per"][0]
    P = pc.plans(sc["x0"], sc["u"], model, pc.plan_cfg(model))
    o = (sk.diff_oracle(sc["refs"][0], sc["u"][0], 1, T) if model == "diff" else sk.race_oracle(sc["refs"][0], sc["u"][0], 1))
    sk.aim(o, ing, CLOCK, pc.mates_of(P, 0), pc.threshold2(model))
    steps_of = [0, 1, T // 2, T]
    poses, steps = [], []
    L = ing["tracks"].shape[1]
    for s in steps_of:
        for centre, thr in ((ing["tracks"][0, min(CLOCK + s, L - 1)], thr_t), (P[1, s], thr_m)):
            for side in (1e-3, -1e-3):
                p = np.zeros(e.nx)
                p[:2] = centre - np.array([reach + thr + side, 0.0])
                poses.append(p)
                steps.append(s)
    x0 = sc["x0"][0]
    h, nrm = sk.heading(x0)
    far = (mc.TRAVEL + 0.3) if model == "diff" else 11.5
    for t in (0.2, 0.5, 0.8):  # across leg A of the wall, from the wall itself out towards the path
        on_wall = x0[:2] + t * far * h - (0.55 if model == "diff" else 2.5) * nrm
        c, d = contour_point(ing["grid"], on_wall, on_wall + (0.5 if model == "diff" else 2.4) * nrm)
        for side in (1e-3, -1e-3):
            p = np.zeros(e.nx)
            p[:2] = c - side * d  # (+: inside the contour, like the circles' inner side)
            p[2] = x0[2] + np.pi  # (the race car: the outline points away from the mates and the track)
            poses.append(p)
            steps.append(0)
    poses, steps = np.array(poses), np.array(steps, np.int32)
    if model == "diff":
        want = o.is_hit(poses[:, 0], poses[:, 1], steps=steps)
    else:
        want = o.is_hit(poses[:, 0], poses[:, 1], poses[:, 2], steps=steps)
    outside = o.sample_margin() > sk.MARGIN
    got = e.eval_is_collided(poses, steps=steps) > 0
    print(model, precision, "hit", want.mean(), "outside the margin", outside.mean(), len(poses))
    assert outside.mean() > 0.9 and 0.2 < want.mean() < 0.8
    assert np.array_equal(got[outside], want[outside])
    now = steps == 0
    assert np.array_equal((e.eval_is_collided(poses[now]) > 0)[outside[now]], want[now][outside[now]])
    # the cost: agent 0's handle without mates, tracks and grid + the penalty where they alone hit + weight g
    plain = tf.engine(model, precision, 1, T, fleet=False, n_agents=1) if model == "diff" else race_engine(precision)
    plain.set_ref_path(sc["refs"][0])
    plain.set_obstacles(ing.get("circles", np.zeros((0, 3))), velocities=ing.get("vel", np.zeros((0, 2))))
    plain.set_state(sc["x0"][0])
    plain.set_u_prev(sc["u"][0])
    plain.run_closed_loop(CLOCK)
    g = ing["grid"].value(poses[now, 0], poses[now, 1])
    for terminal in (False, True):
        c_scene, idx, _ = e.eval_cost(poses[now], terminal=terminal, prev_idx=0)
        c_plain, idx2, _ = plain.eval_cost(poses[now], terminal=terminal, prev_idx=0)
        hit_plain = plain.eval_is_collided(poses[now]) > 0
        expect = c_plain + np.where(got[now] & ~hit_plain, 1e10, 0.0) + ing["grid"].weight * g
        assert np.array_equal(idx, idx2)
        np.testing.assert_allclose(c_scene[outside[now]], expect[outside[now]], rtol=1e-12 if precision == "f64" else 2e-6, atol=0)
    with pytest.raises(pkg.MppiError):  # the plans are among the ingredients: a step beyond them is refused
        e.eval_is_collided(poses[:1], steps=np.array([T + 1], np.int32))


# ------------------------------------------------------------------------------------------ 5. the closed loop
@functools.lru_cache(maxsize=None)
def loop_reference():
    sc = sk.loop_scene()
    ring = tf.device_noise("diff", 3, sk.LOOP_T, sk.LOOP_N, accumulate=True, **tf.LOOP_W)
    return sc, sk.closed_loop(sc, lambda i: ring[i], sk.LOOP_N, K, sk.LOOP_T, sk.LOOP_SWAP, **mc.LOOP_KW)


def shift_grids(e, sc):
    for a, ing in enumerate(sc["per"]):
        if ing["grid"] is not None:
            e.set_cost_grid(**sk.shifted(ing["grid"]).kwargs, agent=a)  # the same shape


def test_closed_loop_f64_end_to_end():
    sc, ref = loop_reference()
    e = load_fleet(fleet_engine(sc, "f64", sk.LOOP_T, accumulate=True, **tf.LOOP_W), sc)
    for i in range(sk.LOOP_N):
        if i == sk.LOOP_SWAP:
            shift_grids(e, sc)
        e.run_closed_loop(1)
        S = e.costs()
        np.testing.assert_allclose(S, ref["S"][i], rtol=1e-10, atol=1e-10, err_msg=f"iteration {i}")
        assert [int((S[a] >= 1.0e10).sum()) for a in range(3)] == list(ref["n_hit"][i]), i
        assert e.stats.n_collided == ref["n_hit"][i][0]
        np.testing.assert_allclose(e.get_state(), ref["x"][i + 1], rtol=1e-8, atol=1e-10)  # (the plant step of the returned u0)
    np.testing.assert_allclose(e.get_u_prev(), ref["u"], rtol=1e-8, atol=1e-10)
    d, _ = e.fleet_clearance()
    np.testing.assert_allclose(d, ref["min_dist"], rtol=1e-8, atol=1e-10)
    print("reference hits per iteration and agent", ref["n_hit"].tolist())
    assert spec_of(e) == "7" and len(set(map(tuple, ref["n_hit"]))) > 1


def test_closed_loop_f32_iteration_by_iteration():
    """Each iteration re-seeded from the reference (test_gpu_fleet_plan.py): a flipped near-threshold sample decides no later one."""
    sc, ref = loop_reference()
    e = load_fleet(fleet_engine(sc, "f32", sk.LOOP_T, accumulate=True, **tf.LOOP_W), sc)
    us = list(ref["u_start"]) + [ref["u"]]
    for i in range(sk.LOOP_N):
        if i == sk.LOOP_SWAP:
            shift_grids(e, sc)
        e.set_state(ref["x"][i])
        e.set_u_prev(us[i])
        e.run_closed_loop(1)
        S = e.costs()
        for a in range(3):
            keep = ref["kept"][i][a]
            assert np.array_equal(mc.penalised(S[a])[keep], mc.penalised(ref["S"][i][a])[keep]), (i, a)
            assert np.all(np.abs(S[a][keep] - ref["S"][i][a][keep]) <= sk.f32_tolerance(ref["S"][i][a][keep])), (i, a)
        if ref["kept"][i].all():
            assert float(np.sqrt(np.mean((e.get_u_prev() - us[i + 1]) ** 2))) <= 1e-4
    print("kept per iteration and agent", ref["kept"].mean(axis=2).tolist())
    assert ref["kept"].mean(axis=2).min() >= 1.0 - mc.MAX_LEFT_OUT


# ------------------------------------------------------------------------------------------ 6. the switch
def refused(call, code, word=None):
    import dnn_mppi_mpc_amd as pkg
    with pytest.raises(pkg.MppiError) as ex:
        call()
    assert ex.value.code == code, str(ex.value)
    assert word is None or word in str(ex.value), str(ex.value)
    return str(ex.value)


def test_a_handle_that_never_opted_in_refuses_as_before():
    """the cross-refusals of the three setters, codes and texts (what tests/test_gpu_cost_grid.py and
    tests/test_gpu_obstacle_tracks.py pin, here with the whole message)"""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = sk.diff_scene(T, True)
    trk, rad, grid = np.zeros((1, 4, 2)), [0.3], sc["grid"].kwargs
    e = diff_engine(T, "frozen", True, "f64")
    e.set_ref_path(sc["ref"])
    e.set_cost_grid(**grid)
    msg = refused(lambda: e.set_obstacle_tracks(trk, rad), capi.ERR_STATE)
    assert msg == ("libmppi_hip: mppi_set_obstacle_tracks: the handle has a cost grid, which uses the same parameter words (limit: remove "
                   f"it first, mppi_set_cost_grid with cells = NULL) (status {capi.ERR_STATE})")
    e.set_cost_grid(None)
    e.set_obstacle_tracks(trk, rad)
    msg = refused(lambda: e.set_cost_grid(**grid), capi.ERR_STATE)
    assert msg == ("libmppi_hip: mppi_set_cost_grid: the handle has obstacle tracks, which use the same parameter words (limit: remove "
                   f"them first, mppi_set_obstacle_tracks with n = 0) (status {capi.ERR_STATE})")
    fleet = pkg.Engine(K=K, n_agents=2, **dict(diff_cfg(capi.WAYPOINT_FROZEN, T), obstacle_motion=1, fleet_radius=0.3))
    msg = refused(lambda: fleet.set_cost_grid(**grid), capi.ERR_UNSUPPORTED)
    assert msg == ("libmppi_hip: mppi_set_cost_grid: a fleet handle (fleet_radius > 0) takes no cost grid: its plan mode uses the same "
                   f"parameter words (limit: fleet_radius = 0) (status {capi.ERR_UNSUPPORTED})")
    msg = refused(lambda: fleet.set_obstacle_tracks(trk, rad, agent=1), capi.ERR_UNSUPPORTED)
    assert msg == ("libmppi_hip: mppi_set_agent_obstacle_tracks: a fleet handle (fleet_radius > 0) takes no obstacle tracks: its plan mode "
                   f"uses the same parameter words (limit: fleet_radius = 0) (status {capi.ERR_UNSUPPORTED})")
    fleet.set_fleet_prediction("plan")  # (and nothing stands in the way of the plan mode)
    assert getattr(e, "scene_mode", "exclusive") == "exclusive"


def test_the_switch_and_its_refusals():
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = sk.diff_scene(T, True)
    e = load_single(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    twin = load_single(diff_engine(T, "frozen", True, "f64", seed=3), sc)
    assert e.scene_mode == "composed"
    refused(lambda: e.set_scene_mode("both"), capi.ERR_BAD_ARG)
    assert e.lib.mppi_set_scene_mode(e._h, 2) == capi.ERR_BAD_ARG and e.lib.mppi_set_scene_mode(e._h, -1) == capi.ERR_BAD_ARG
    msg = refused(lambda: e.set_scene_mode("exclusive"), capi.ERR_STATE, "obstacle tracks")  # two are held: refused and harmless
    assert "cost grid" in msg and e.scene_mode == "composed"
    for h in (e, twin):
        h.set_state(sc["x0"])
        h.run_closed_loop(2)
    assert spec_of(e) == "7"
    assert_same(e, twin)
    # every other refusal of the setters stays in composed mode
    refused(lambda: e.set_cost_grid(**dict(sc["grid"].kwargs, resolution=0.0)), capi.ERR_BAD_ARG, "resolution")
    refused(lambda: e.set_obstacle_tracks(np.zeros((1, 4, 2)), [-1.0]), capi.ERR_BAD_ARG, "radius")
    refused(lambda: e.set_cost_grid(**sc["grid"].kwargs, agent=1), capi.ERR_BAD_ARG, "agent")
    e.set_cost_grid(None)
    e.set_scene_mode("exclusive")  # one ingredient left: accepted, and the exclusive refusals are back
    refused(lambda: e.set_cost_grid(**sc["grid"].kwargs), capi.ERR_STATE, "obstacle tracks")
    # handles that cannot opt in
    static = diff_engine(T, "frozen", True, "f64", obstacle_motion=0)
    refused(lambda: static.set_scene_mode("composed"), capi.ERR_STATE, "obstacle_motion")
    long = diff_engine(130, "frozen", True, "f64")
    refused(lambda: long.set_scene_mode("composed"), capi.ERR_UNSUPPORTED, "T <= 128")
    # a fleet handle: tracks and a grid in velocity mode, the plans beside them; back only with one left
    full = sk.fleet_scene(T, False)
    fleet = load_fleet(fleet_engine(full, "f64", T), full)
    refused(lambda: fleet.set_scene_mode("exclusive"), capi.ERR_STATE, "MPPI_FLEET_PLAN")
    fleet.set_fleet_prediction("velocity")
    fleet.run_closed_loop(1)
    assert spec_of(fleet) == "7"  # (tracks and a grid: the composed form, the mates in the rows)
    fleet.set_cost_grid(None)
    fleet.run_closed_loop(1)
    assert spec_of(fleet) == "5"
    fleet.set_scene_mode("exclusive")
    refused(lambda: fleet.set_fleet_prediction("plan"), capi.ERR_STATE, "obstacle tracks")
    refused(lambda: fleet.set_cost_grid(**full["per"][0]["grid"].kwargs), capi.ERR_UNSUPPORTED, "fleet_radius")


def test_controller_keyword_composes_the_scene():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    case = (50, False, "frozen", 0, 0, "64x64")
    sc, eps, o, res = single_reference(*case)
    kw = dict(mc.DIFF_KW, ref_path=sc["ref"], num_samples_K=K, num_horizons_T=50, precision="f64", waypoint_mode="frozen",
              obstacle_circles=sc["circles"], obstacle_velocities=sc["vel"], obstacle_tracks=(sc["tracks"], sc["radii"]),
              cost_grid=sc["grid"].kwargs)
    with pytest.raises(pkg.MppiError) as ex:
        pkg.MPPIAlgorithms(**kw)  # the default: exclusive
    assert ex.value.code == capi.ERR_STATE
    c = pkg.MPPIAlgorithms(**kw, compose_scene=True)
    assert c._engine.scene_mode == "composed"
    c.u_prev[:] = sc["u"]
    c._calc_epsilon = lambda *a, **k: cuda(eps)
    _, u, _, _ = c._calc_input_control(sc["x0"])
    np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
    assert spec_of(c._engine) == "7"
