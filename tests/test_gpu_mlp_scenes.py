"""Learned-dynamics scene handles on the device (mppi_config.obstacle_motion = 2): moving circles, obstacle tracks
and a cost grid -- under the centre or under the outline -- priced along the learned rollout by the scene forms of
k_rollout_mlp_w / k_rollout_mlp_h3, against the f64 reference of tests/mlp_scene_checks.py; the clock; what must stay bit for
bit; the refusals and the stage methods.  K = 250 (three full 64-sample tiles and a ragged one), T = 7 or 50."""
import numpy as np
import pytest

import mlp_scene_checks as ms
import moving_obstacle_checks as mc
import grid_footprint_checks as gf
import scene_checks as sk
from test_gpu_moving_obstacles import cuda, diff_engine

pytestmark = pytest.mark.gpu

K = ms.K


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, float) - np.asarray(b, float)) ** 2)))


def scene_kernel(H, n, agents=False):
    tail = "_agents" if agents else ""
    return f"k_rollout_mlp_h3_scene{tail}" if (H, n) in ((512, 3), (512, 2)) else f"k_rollout_mlp_w_scene{tail}<{H}>"


def engine(T, mode, accumulate, outline=False, motion=2, **kw):
    from dnn_mppi_mpc_amd import _capi as capi
    cfg = dict(model=capi.MODEL_DIFFDRIVE_MLP, obstacle_motion=motion)
    if outline:
        cfg.update(gf.DIFF_BOX, obstacle_model=capi.OBSTACLE_OUTLINE)
    cfg.update(kw)
    return diff_engine(T, mode, accumulate, "f32", K=K, **cfg)


def give(e, ing, agent=None):
    if ing.get("tracks") is not None:
        e.set_obstacle_tracks(ing["tracks"], ing["radii"], agent=agent)
    if ing.get("grid") is not None:
        e.set_cost_grid(**ing["grid"].kwargs, agent=agent)


def load(e, sc, moving=True):
    e.set_mlp(sc["w"])
    e.set_ref_path(sc["ref"])
    if sc.get("outline"):
        e.set_cost_grid_footprint("outline")
    if sc.get("tracks") is not None and sc.get("grid") is not None:
        e.set_scene_mode("composed")
    if moving:
        e.set_obstacles(sc["circles"], velocities=sc["vel"])
    else:
        e.set_obstacles(sc["circles"])
    give(e, sc)
    e.set_u_prev(sc["u"])
    return e


# ------------------------------------------------------------------------------------------ 1. one iteration
def check_iteration(e, sc, eps, o, res, mode):
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = ms.kept(o, sc["outline"])
    hit_ref = mc.penalised(S_ref)
    err_u = rmse(u, res["u_returned"])
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "max rel S err", float(np.max(np.abs(S[keep] - S_ref[keep]) / np.maximum(np.abs(S_ref[keep]), 1.0))),
          "weight left out", float(res["w"][~keep].max(initial=0.0)))
    assert e.rollout_kernel() == scene_kernel(*sc["shape"])
    assert keep.mean() >= 1.0 - ms.MAX_LEFT_OUT
    assert np.array_equal(mc.penalised(S)[keep], hit_ref[keep])  # the hit set, exact outside the margin
    np.testing.assert_allclose(S[keep], S_ref[keep], rtol=1e-3, atol=1e-3)
    if res["w"][~keep].max(initial=0.0) <= 1e-6:
        assert err_u <= 1e-4
    assert st.n_collided == int((S >= 1.0e10).sum())
    # ... and against the reference's own count: equal over the kept samples, so the two differ by kept-out samples at most
    assert int((S[keep] >= 1.0e10).sum()) == int(hit_ref[keep].sum())
    assert abs(st.n_collided - int(hit_ref.sum())) <= int((~keep).sum())
    if mode == "sequential":
        assert st.idx_after == res["idx_after"]
    return st, S, keep


@pytest.mark.parametrize("case", ms.cases(), ids=str)
def test_one_iteration_against_the_reference(case):
    kind, T, accumulate, mode = case[:4]
    sc, eps, o, res = ms.case(*case)
    e = load(engine(T, mode, accumulate, sc["outline"]), sc)
    st, S, keep = check_iteration(e, sc, eps, o, res, mode)
    if kind == "grid":  # a grid and no circles: the count comes from the grid alone
        assert len(sc["circles"]) == 0 and st.n_collided > 0
        if keep.all():
            assert st.n_collided == int(mc.penalised(res["S"]).sum())


# ------------------------------------------------------------------------------------------ 2. the clock
def test_the_clock_moves_circles_tracks_and_a_reuploaded_grid():
    """Five iterations, the handle's state set back from the reference before each (nothing drifts): the circles move, the tracks
    advance and then hold their last point (L = T + 2: the hold is priced from the third iteration on), the grid is uploaded
    again, shifted by one cell, after the third; then mppi_set_iteration, which must not move the obstacles."""
    T = 50
    sc = ms.scene("composed", T, True, extra=1)
    eps = ms.philox.sample_epsilon(mc.DIFF_KW["sigma"], 5, 0, K, T)
    e = load(engine(T, "frozen", True), sc)
    o = ms.scene_oracle(sc["ref"], sc["u"], K, T, sc["w"])
    S_seen = []
    for i in range(5):
        ing = dict(sc, grid=sk.shifted(sc["grid"]) if i >= 3 else sc["grid"])
        if i == 3:
            e.set_cost_grid(**ing["grid"].kwargs)
        o.u_prev[:] = sc["u"]
        o.prev_way_point_idx = 0
        sk.aim(o, ing, i)
        res = o.iteration_general(sc["x0"], eps.astype(np.float64), "frozen", True)
        e.set_u_prev(sc["u"])
        e.set_waypoint_idx(0)
        u, _, st = e.step(sc["x0"], eps=cuda(eps))
        S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
        keep = ms.kept(o)
        print("iteration", i, "kept", keep.mean(), "penalised", mc.penalised(S_ref).mean())
        assert keep.mean() >= 1.0 - ms.MAX_LEFT_OUT
        assert np.array_equal(mc.penalised(S)[keep], mc.penalised(S_ref)[keep])
        np.testing.assert_allclose(S[keep], S_ref[keep], rtol=1e-3, atol=1e-3)
        S_seen.append(S_ref)
    assert not np.array_equal(mc.penalised(S_seen[0]), mc.penalised(S_seen[2]))  # the scene moved
    # the counter replays noise and does not move obstacles: the sixth iteration at another counter value prices clock 5
    e.set_iteration(40)
    o.u_prev[:] = sc["u"]
    o.prev_way_point_idx = 0
    sk.aim(o, dict(sc, grid=sk.shifted(sc["grid"])), 5)
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), "frozen", True)
    e.set_u_prev(sc["u"])
    e.set_waypoint_idx(0)
    e.step(sc["x0"], eps=cuda(eps))
    S, S_ref, keep = e.costs(), np.asarray(res["S"], np.float64), ms.kept(o)
    assert np.array_equal(mc.penalised(S)[keep], mc.penalised(S_ref)[keep])
    np.testing.assert_allclose(S[keep], S_ref[keep], rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------ 3. bit for bit
@pytest.mark.parametrize("H,n", [(64, 1), (512, 3)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_zero_velocities_equal_the_static_handle(H, n, accumulate):
    T = 50
    sc = ms.scene("circles", T, accumulate, H, n)
    sc = dict(sc, vel=np.zeros_like(sc["vel"]))
    eps = cuda(ms.philox.sample_epsilon(mc.DIFF_KW["sigma"], 3, 0, K, T))
    out = []
    for motion in (2, 0):
        e = load(engine(T, "frozen", accumulate, motion=motion), sc, moving=motion == 2)
        u, _, st = e.step(sc["x0"], eps=eps)
        out.append((u.copy(), e.costs(), st.n_collided, e.rollout_kernel()))
    assert out[0][3] == scene_kernel(H, n) and "scene" not in out[1][3]
    assert out[0][2] == out[1][2] > 0
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])


def test_graph_replay_equals_eager_across_a_same_shape_upload(monkeypatch):
    T, n_it = 50, 3
    sc = ms.scene("grid", T, True)
    shifted = sk.shifted(sc["grid"]).kwargs

    def run(e):
        e.set_state(sc["x0"])
        e.run_closed_loop(n_it)
        e.set_cost_grid(**shifted)  # the same shape: buffers, plan and a cached graph stay
        e.run_closed_loop(n_it)
        return e
    eager = run(load(engine(T, "frozen", True, seed=31), sc))
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = run(load(engine(T, "frozen", True, seed=31), sc))
    assert np.array_equal(eager.costs(), graph.costs()) and np.array_equal(eager.get_u_prev(), graph.get_u_prev())
    assert np.array_equal(eager.get_state(), graph.get_state()) and eager.stats.n_collided > 0
    unshifted = load(engine(T, "frozen", True, seed=31), sc)
    unshifted.set_state(sc["x0"])
    unshifted.run_closed_loop(2 * n_it)
    assert not np.array_equal(unshifted.costs(), graph.costs())  # the re-upload was seen


@pytest.mark.parametrize("H,n", [(64, 1), (512, 3)])
def test_three_agents_equal_three_single_handles(H, n):
    """own models for all three; a composed scene for agent 0, an own grid alone for agent 1, nothing for agent 2"""
    T = 50
    full = ms.scene("composed", T, True, H, n)
    per = [full, dict(ms.scene("grid", T, True, H, n)), dict(full, circles=np.zeros((0, 3)), vel=np.zeros((0, 2)), tracks=None, radii=None, grid=None)]
    models = [ms.scene_weights(H, n, full["x0"], full["u"], seed=70 + a, move=0.2 + 0.1 * a) for a in range(3)]
    x0 = np.stack([full["x0"] + 0.01 * a for a in range(3)])
    batch = engine(T, "frozen", True, n_agents=3, seed=77)
    batch.set_scene_mode("composed")
    for a in range(3):
        batch.set_mlp(models[a], agent=a)
        batch.set_ref_path(per[a]["ref"], agent=a)
        batch.set_obstacles(per[a]["circles"], agent=a, velocities=per[a]["vel"])
        give(batch, per[a], agent=a)
    batch.set_state(x0)
    batch.set_u_prev(np.stack([full["u"]] * 3))
    batch.run_closed_loop(2)
    assert batch.rollout_kernel() == scene_kernel(H, n, agents=True)
    S, u = batch.costs(), batch.get_u_prev()
    for a in range(3):
        e = engine(T, "frozen", True, seed=77, noise_stream=a)
        e.set_scene_mode("composed")
        e.set_mlp(models[a])
        e.set_ref_path(per[a]["ref"])
        e.set_obstacles(per[a]["circles"], velocities=per[a]["vel"])
        give(e, per[a])
        e.set_state(x0[a])
        e.set_u_prev(full["u"])
        e.run_closed_loop(2)
        assert e.rollout_kernel() == scene_kernel(H, n)
        assert np.array_equal(S[a], e.costs()) and np.array_equal(u[a], e.get_u_prev()), a
    assert (S[0] >= 1e10).any() and (S[1] >= 1e10).any() and not (S[2] >= 1e10).any()


# ------------------------------------------------------------------------------------------ 4. refusals and stage methods
def test_refusals():
    from dnn_mppi_mpc_amd import _capi as capi
    with pytest.raises(capi.MppiError) as ex:  # value 1 with the learned model stays refused, and says where to go
        engine(50, "frozen", False, motion=1)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "MPPI_MODEL_DIFFDRIVE_MLP" in str(ex.value) and "obstacle_motion = 2" in str(ex.value)
    with pytest.raises(capi.MppiError) as ex:
        diff_engine(50, "frozen", False, "f32", obstacle_motion=2)  # an analytic model
    assert ex.value.code == capi.ERR_BAD_ARG
    with pytest.raises(capi.MppiError) as ex:
        engine(50, "frozen", False, n_agents=2, fleet_radius=0.4)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "fleet" in str(ex.value)
    with pytest.raises(capi.MppiError) as ex:
        engine(50, "frozen", False, K_global=2 * K)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "shard" in str(ex.value)
    with pytest.raises(capi.MppiError) as ex:
        diff_engine(50, "frozen", False, "f64", K=K, model=capi.MODEL_DIFFDRIVE_MLP, obstacle_motion=2)
    assert ex.value.code == capi.ERR_UNSUPPORTED
    sc = ms.scene("composed", 50, False)
    e = engine(130, "frozen", False)  # T > 128: the setters' limit
    for call in (lambda: e.set_obstacle_tracks(sc["tracks"], sc["radii"]), lambda: e.set_cost_grid(**sc["grid"].kwargs)):
        with pytest.raises(capi.MppiError) as ex:
            call()
        assert ex.value.code == capi.ERR_UNSUPPORTED and "T <= 128" in str(ex.value)
    static = engine(50, "frozen", False, motion=0)  # a learned handle without the switch: the setters name the value IT needs
    for call in (lambda: static.set_obstacle_tracks(sc["tracks"], sc["radii"]), lambda: static.set_cost_grid(**sc["grid"].kwargs),
                 lambda: static.set_obstacles(sc["circles"], velocities=sc["vel"]), lambda: static.set_scene_mode("composed")):
        with pytest.raises(capi.MppiError) as ex:
            call()
        assert ex.value.code == capi.ERR_STATE and "obstacle_motion = 2" in str(ex.value)
    e = engine(50, "frozen", False)
    e.set_obstacle_tracks(sc["tracks"], sc["radii"])
    with pytest.raises(capi.MppiError) as ex:  # the setters' exclusivity is what it was
        e.set_cost_grid(**sc["grid"].kwargs)
    assert ex.value.code == capi.ERR_STATE
    big = dict(ms.scene_weights(512, 3, sc["x0"], sc["u"]))
    big["input_layer.weight"] = big["input_layer.weight"].copy()
    big["input_layer.weight"][0, 0] = 1.0e5  # beyond the f16 range: the f32-input kernel has no scene form
    with pytest.raises(capi.MppiError) as ex:
        e.set_mlp(big)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "scene" in str(ex.value)


def test_mlp_f32_switch_is_refused_on_a_scene_handle(monkeypatch):
    from dnn_mppi_mpc_amd import _capi as capi
    sc = ms.scene("circles", 50, False, 512, 3)
    e = engine(50, "frozen", False)
    monkeypatch.setenv("MPPI_MLP_F32", "1")
    with pytest.raises(capi.MppiError) as ex:
        e.set_mlp(sc["w"])
    assert ex.value.code == capi.ERR_UNSUPPORTED and "MPPI_MLP_F32" in str(ex.value)


def test_controller_picks_the_scene_handle():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc, eps, o, res = ms.case("composed", T, False, "frozen")
    kw = dict({k: v for k, v in mc.DIFF_KW.items() if k != "safety_margin_rate"}, ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T)
    c = pkg.MPPIAlgorithms(**kw, obstacle_circles=sc["circles"], safety_margin_rate=0.8, learned_dynamics=sc["w"], waypoint_mode="frozen",
                           obstacle_velocities=sc["vel"], obstacle_tracks=(sc["tracks"], sc["radii"]), cost_grid=sc["grid"].kwargs,
                           compose_scene=True)
    assert c._engine.cfg.obstacle_motion == capi.OBSTACLE_MOTION_LEARNED
    c.u_prev[:] = sc["u"]
    c._calc_epsilon = lambda *a, **k: eps
    c._calc_input_control(sc["x0"])
    assert c._engine.rollout_kernel() == scene_kernel(64, 1)
    S, keep = c.sample_costs(), ms.kept(o)
    assert np.array_equal(mc.penalised(S)[keep], mc.penalised(res["S"])[keep])


@pytest.mark.parametrize("kind", ["composed", "outline"])
def test_stage_methods_equal_the_analytic_handle(kind):
    """mppi_eval_cost, mppi_eval_is_collided[_at] and mppi_eval_cost_grid answer for agent 0 as an analytic handle with the same
    scene does, bit for bit (the same k_eval_pose behind another carrier)."""
    T = 50
    sc = ms.scene(kind, T, True)
    learned = load(engine(T, "frozen", True, sc["outline"]), sc)
    from dnn_mppi_mpc_amd import _capi as capi
    kw = dict(gf.DIFF_BOX, obstacle_model=capi.OBSTACLE_OUTLINE) if sc["outline"] else {}
    analytic = diff_engine(T, "frozen", True, "f32", K=K, **kw)
    analytic.set_ref_path(sc["ref"])
    if sc["outline"]:
        analytic.set_cost_grid_footprint("outline")
    else:
        analytic.set_scene_mode("composed")
    analytic.set_obstacles(sc["circles"], velocities=sc["vel"])
    give(analytic, sc)
    rng = np.random.default_rng(4)
    h, nrm = sk.heading(sc["x0"])
    x = np.column_stack([sc["x0"][:2] + rng.uniform(0, 3.5, (300, 1)) * h + rng.uniform(-1.2, 1.2, (300, 1)) * nrm, rng.uniform(-3, 3, 300)])
    steps = rng.integers(0, T + 1, 300).astype(np.int32)
    for e in (learned, analytic):
        e.set_state(sc["x0"])
    a, b = learned.eval_is_collided(x), analytic.eval_is_collided(x)
    assert np.array_equal(a, b)
    a, b = learned.eval_is_collided(x, steps), analytic.eval_is_collided(x, steps)
    assert np.array_equal(a, b) and 0 < a.sum() < len(a)
    for terminal in (False, True):
        ca, ia, _ = learned.eval_cost(x, 0, terminal=terminal)
        cb, ib, _ = analytic.eval_cost(x, 0, terminal=terminal)
        assert np.array_equal(ca, cb) and np.array_equal(ia, ib)
    assert np.array_equal(learned.cost_grid_at(x[:, :2]), analytic.cost_grid_at(x[:, :2]))
