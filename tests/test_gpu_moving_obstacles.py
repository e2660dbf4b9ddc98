"""Moving obstacles on the device (mppi_config.obstacle_motion): the collision test at a step of the obstacle
clock, one iteration against the f64 reference of tests/moving_obstacle_checks.py on every rollout form, the clock through
closed loops, graph replay and mppi_set_iteration, batched agents with their own moving sets, sharding, and the refusals.
K = 256 throughout; every reference is computed once per case and shared by the f32 and the f64 handle."""
import functools

import numpy as np
import pytest

import moving_obstacle_checks as mc
from test_gpu_agent_scenes import compare, diff_cfg, race_cfg

pytestmark = pytest.mark.gpu

K = mc.K_CASE
MODES = {"frozen": "WAYPOINT_FROZEN", "per_rollout": "WAYPOINT_PER_ROLLOUT", "sequential": "WAYPOINT_SEQUENTIAL"}


def prec(name):
    from dnn_mppi_mpc_amd import _capi as capi
    return capi.PREC_F64 if name == "f64" else capi.PREC_F32


def diff_engine(T, mode, accumulate, precision, K=K, **kw):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    cfg = dict(diff_cfg(getattr(capi, MODES[mode]), T, precision=prec(precision)), accumulate_stage_cost=int(accumulate),
               filter_window=mc.filter_window(T), obstacle_motion=1)
    cfg.update(kw)
    return pkg.Engine(K=K, **cfg)


def race_engine(precision, K=K, **kw):
    import dnn_mppi_mpc_amd as pkg
    cfg = dict(race_cfg(), precision=prec(precision), obstacle_motion=1)
    cfg.update(kw)
    return pkg.Engine(K=K, **cfg)


def load(e, sc, moving=True):
    e.set_ref_path(sc["ref"])
    e.set_obstacles(sc["circles"], velocities=sc["vel"] if moving else None)
    e.set_u_prev(sc["u"])
    return e


def cuda(eps):
    import torch
    return torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def diff_reference(T, accumulate, mode):
    return mc.diff_case(T, accumulate, mode)


@functools.lru_cache(maxsize=None)
def race_reference():
    return mc.race_case()


def check_iteration(e, sc, eps, o, res, precision, sequential=False):
    """One iteration with injected noise against the reference (tolerances: DESIGN section 5)."""
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = mc.kept(o, precision == "f64")
    hit_ref = mc.penalised(S_ref)
    err_u = float(np.sqrt(np.mean((u - res["u_returned"]) ** 2)))
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", hit_ref.mean(), "u rmse", err_u, "n_collided", st.n_collided,
          "max rel S err", float(np.max(np.abs(S[keep] - S_ref[keep]) / np.maximum(np.abs(S_ref[keep]), 1.0))))
    assert keep.mean() >= 1.0 - mc.MAX_LEFT_OUT
    assert np.array_equal(mc.penalised(S)[keep], hit_ref[keep])  # no flip outside the margin
    assert int(mc.penalised(S)[keep].sum()) == int(hit_ref[keep].sum())  # the count on the samples kept, from the costs
    # mppi_stats.n_collided is the kernels' count of S >= collision_penalty over ALL samples (every rollout kernel's
    # definition): a penalised sample whose tracking + control terms sum below zero is not in it, and in f32 such a sum rounds
    # either way.  So: exactly the reference's count by that definition for an f64 handle with nothing left out, else within
    # the samples that may fall either way.
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


# ------------------------------------------------------------------------------------------ 1. the collision test at a step
def eval_scene(model, m):
    """The case scene with the crosser first and the leaver LAST (circle m - 1: beyond the 64 lanes for m = 65 and 70, it and
    its velocity come from memory), poses scattered around where the circles stand over the steps asked for."""
    sc = mc.diff_scene(50, True) if model == "diff" else mc.race_scene()
    order = [0, 2, 1]
    circles, vel = mc.table(sc["circles"][order], sc["vel"][order], m)
    return dict(sc, circles=circles, vel=vel)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 2, 64, 65, 70])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_collision_test_at_a_step(model, m, precision):
    T = 50 if model == "diff" else mc.RACE_T
    sc = eval_scene(model, m)
    e = load(diff_engine(T, "frozen", True, precision) if model == "diff" else race_engine(precision), sc)
    o = (mc.diff_oracle if model == "diff" else mc.race_oracle)(sc, 1, *([T] if model == "diff" else []))
    dt = float(o.delta_t)
    rng = np.random.default_rng(7 + m)
    movers = [i for i in (0, m - 1) if i < m]
    n_loop = 3
    for clock in (0, n_loop):  # n > 0: reached by a short closed loop
        if clock:
            e.set_state(sc["x0"])
            e.run_closed_loop(n_loop)
        steps = np.repeat(np.array([0, 1, T, T // 2], dtype=np.int32), 96)
        at = mc.centres(sc["circles"], sc["vel"], dt, clock, steps)[np.arange(len(steps)), rng.choice(movers, len(steps))]
        spread = 0.6 if model == "diff" else 2.5
        poses = np.zeros((len(steps), e.nx))
        poses[:, :2] = at + rng.normal(0, spread, at.shape)
        poses[:, 2] = rng.uniform(-np.pi, np.pi, len(steps))
        o.set_motion(sc["vel"], clock)
        want = (o.collided(poses[:, 0], poses[:, 1], steps=steps) if model == "diff"
                else o.collided(poses[:, 0].astype(np.float32), poses[:, 1].astype(np.float32), poses[:, 2].astype(np.float32), steps=steps)) > 0
        outside = o.sample_margin() > mc.MARGIN
        got = e.eval_is_collided(poses, steps=steps) > 0
        print(model, m, precision, "clock", clock, "hit", want.mean(), "outside the margin", outside.mean(), "flips", int((got != want).sum()))
        assert 0.1 < want.mean() < 0.9 and outside.mean() > 0.98
        assert np.array_equal(got[outside], want[outside])
        for j in (0, 1, T):  # every step asked for sees both outcomes
            assert 0 < want[steps == j].sum() < (steps == j).sum()
        now = e.eval_is_collided(poses) > 0  # the existing entry prices step 0 of the current clock
        assert np.array_equal(now[outside & (steps == 0)], want[outside & (steps == 0)])
    # zero velocities: exactly the static test, at any step
    e.set_obstacles(sc["circles"], velocities=np.zeros_like(sc["vel"]))
    static = diff_engine(T, "frozen", True, precision, obstacle_motion=0) if model == "diff" else race_engine(precision, obstacle_motion=0)
    load(static, sc, moving=False)
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), static.eval_is_collided(poses))
    assert np.array_equal(e.eval_is_collided(poses), static.eval_is_collided(poses))
    e.set_obstacles(sc["circles"])  # the static setter on a moving handle: velocity 0
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), static.eval_is_collided(poses))


# ------------------------------------------------------------------------------------------ 2. one iteration
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("T,accumulate,mode", mc.diff_cases())
def test_diff_iteration_against_the_reference(T, accumulate, mode, precision):
    sc, eps, o, res = diff_reference(T, accumulate, mode)
    e = load(diff_engine(T, mode, accumulate, precision), sc)
    check_iteration(e, sc, eps, o, res, precision, sequential=mode == "sequential")
    name = e.rollout_kernel()
    if T <= 128:  # k_rollout_fused<R, MODEL, NCH, MULTI, SPEC = 3, HYPK>
        assert name.startswith("k_rollout_fused<") and name.split(", ")[4] == "3" and name.split(", ")[2] == ("1" if T <= 64 else "2"), name
    else:
        assert name.startswith("k_rollout_moving<"), name


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_race_iteration_against_the_reference(precision):
    sc, eps, o, res = race_reference()
    e = load(race_engine(precision), sc)
    u, _, st = e.step(sc["x0"], eps=cuda(eps))
    S, S_ref = e.costs(), np.asarray(res["S"], np.float64)
    keep = mc.kept(o, False)  # (the reference itself is f32: the margin applies to both handles)
    print(e.rollout_kernel(), "kept", keep.mean(), "penalised", mc.penalised(S_ref).mean(), "n_collided", st.n_collided)
    assert keep.mean() >= 1.0 - mc.MAX_LEFT_OUT
    assert np.array_equal(mc.penalised(S)[keep], mc.penalised(S_ref)[keep])
    np.testing.assert_allclose(S[keep], S_ref[keep], rtol=2e-4, atol=2e-4)
    assert float(np.sqrt(np.mean((u - res["u_returned"]) ** 2))) <= 1e-4
    assert int(mc.penalised(S)[keep].sum()) == int(mc.penalised(S_ref)[keep].sum())
    assert e.rollout_kernel().split(", ")[4] == "3"


# ------------------------------------------------------------------------------------------ 3. the clock
LOOP_T, LOOP_N = 50, 12


def loop_engine(precision, **kw):
    e = diff_engine(LOOP_T, "frozen", False, precision, seed=31, stage_cost_weight=[0.25, 0.25, 0.5, 0], terminal_cost_weight=[0.25, 0.25, 0.5, 0], **kw)
    return e


@functools.lru_cache(maxsize=None)
def loop_reference():
    """The reference loop on the noise the device's sampler draws (mppi_sample_epsilon: bit for bit what the kernels draw
    for that iteration; the NumPy sampler agrees with it to f32 rounding of sin / cos / log only)."""
    e = loop_engine("f32")
    ring = [e.sample_epsilon(i).cpu().numpy() for i in range(LOOP_N)]
    e.close()
    return mc.diff_closed_loop(LOOP_T, LOOP_N, eps_of=lambda i: ring[i])


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_closed_loop_advances_the_obstacles(monkeypatch, precision, graph):
    """mppi_run_closed_loop(12) with the plant against the reference that ticks the circles once per iteration; under
    MPPI_GRAPH=1 the replayed graph reads the clock afresh."""
    if graph == "1":
        monkeypatch.setenv("MPPI_GRAPH", "1")
    ref = loop_reference()
    sc = ref["scene"]
    e = load(loop_engine(precision), sc)
    e.set_state(sc["x0"])
    trace, st = e.run_closed_loop(LOOP_N, trace=True)
    err = float(np.sqrt(np.mean((trace - ref["u0"]) ** 2)))
    print(precision, graph, "u0 rmse", err, "reference hits per iteration", ref["n_hit"], "kept", min(ref["kept"]), "last n_collided", st.n_collided)
    assert max(ref["n_hit"]) - min(ref["n_hit"]) > K // 16  # the scene changes under the loop
    if precision == "f64":
        np.testing.assert_allclose(trace, ref["u0"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(e.get_state(), ref["x"], rtol=1e-8, atol=1e-10)
        assert st.n_collided == ref["n_hit"][-1]
    else:
        assert err <= 1e-4
        # (the state integrates u0: |dx| <= n dt max|du0| <= 12 * 0.1 * sqrt(24) * 1e-4 = 5.9e-4 under the bound above)
        np.testing.assert_allclose(e.get_state(), ref["x"], rtol=0, atol=1e-3)
    assert e.get_waypoint_idx() == ref["idx"] and st.iteration == LOOP_N


def test_set_iteration_does_not_move_obstacles_and_an_upload_rebases():
    sc = mc.diff_scene(LOOP_T, False)
    e = load(loop_engine("f64"), sc)
    e.set_state(sc["x0"])
    o = mc.diff_oracle(sc, 1, LOOP_T)
    rng = np.random.default_rng(5)
    steps = rng.integers(0, LOOP_T + 1, 256).astype(np.int32)
    poses = np.zeros((256, 3))  # fixed poses around where the two movers stand a few control steps in
    poses[:, :2] = mc.centres(sc["circles"], sc["vel"], 0.1, 3, steps)[np.arange(256), rng.integers(0, 2, 256)] + rng.normal(0, 0.8, (256, 2))

    def want(clock):
        o.set_motion(sc["vel"], clock)
        return o.collided(poses[:, 0], poses[:, 1], steps=steps)
    w0, w3, w4, w6 = want(0), want(3), want(4), want(6)
    assert 0 < w4.sum() < 256 and (w4 != w6).sum() > 8 and (w0 != w3).sum() > 8
    e.run_closed_loop(4)
    before = e.eval_is_collided(poses, steps=steps)
    assert np.array_equal(before, w4)
    e.set_iteration(1000)  # replays noise; the circles stay
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), before)
    e.run_closed_loop(2)   # and go on from where they were: clock 6
    assert e.stats.iteration == 1002
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), w6)
    e.set_obstacles(sc["circles"], velocities=sc["vel"])  # a fresh upload: the circles stand where given NOW
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), w0)
    e.run_closed_loop(3)
    assert np.array_equal(e.eval_is_collided(poses, steps=steps), w3)


# ------------------------------------------------------------------------------------------ 4. batches
def agent_scenes(model, T):
    """Four agents: the case scene; its two movers a little displaced; a static set (the circles where they stand when the
    robot meets them: step T for `S[k] =`, mid-horizon for the race car); no circles at all."""
    sc = mc.diff_scene(T, False) if model == "diff" else mc.race_scene()
    dt = 0.1 if model == "diff" else 0.05
    met = sc["circles"].copy()
    met[:, :2] = mc.centres(sc["circles"], sc["vel"], dt, 0, T if model == "diff" else T // 2)
    sets = [(sc["circles"], sc["vel"]), (sc["circles"][:2] + [0.05, -0.05, 0.0], sc["vel"][:2]), (met, None),
            (np.zeros((0, 3)), np.zeros((0, 2)))]
    rng = np.random.default_rng(11)
    x0 = np.stack([sc["x0"] + 0.02 * a for a in range(4)])
    u = np.stack([sc["u"] + rng.normal(0, 0.01, sc["u"].shape) for _ in range(4)])
    return sc, sets, x0, u


def batch_cfg(model, T, precision):
    from dnn_mppi_mpc_amd import _capi as capi
    base = diff_cfg(capi.WAYPOINT_FROZEN, T, precision=prec(precision)) if model == "diff" else dict(race_cfg(), precision=prec(precision))
    return dict(base, obstacle_motion=1)


def set_agent(e, a, circles, vel):
    e.set_obstacles(circles, agent=a, velocities=vel)


@pytest.mark.parametrize("model,precision", [("diff", "f64"), ("diff", "f32"), ("race", "f32")])
def test_agents_with_own_moving_sets_equal_single_handles(model, precision):
    """Bit for bit: batch and single handles run the same one-sample-per-wave instantiation family (MULTI or not)."""
    import dnn_mppi_mpc_amd as pkg
    T, n_it = (50, 6) if model == "diff" else (mc.RACE_T, 6)
    sc, sets, x0, u = agent_scenes(model, T)
    cfg = batch_cfg(model, T, precision)
    batch = pkg.Engine(K=K, n_agents=4, **cfg)
    batch.set_ref_path(sc["ref"])
    for a, (c, v) in enumerate(sets):
        set_agent(batch, a, c, v)
    batch.set_state(x0)
    batch.set_u_prev(u)
    singles = []
    for a, (c, v) in enumerate(sets):
        one = pkg.Engine(K=K, noise_stream=a, **cfg)
        one.set_ref_path(sc["ref"])
        one.set_obstacles(c, velocities=v)
        one.set_state(x0[a])
        one.set_u_prev(u[a])
        singles.append(one)
    hits = []
    for n in (1, n_it - 1):  # (the first iteration apart: its collision counts say that every set with circles matters)
        batch.run_closed_loop(n)
        for one in singles:
            one.run_closed_loop(n)
        hits.append([int(one.stats.n_collided) for one in singles])
        compare(batch, singles, None)
    print(model, precision, "n_collided per agent, first and last iteration", hits, batch.rollout_kernel())
    assert all(h > 0 for h in hits[0][:3]) and hits[0][3] == hits[1][3] == 0 and hits[0][:3] != hits[1][:3]
    assert ", true, 3, " in batch.rollout_kernel() and ", false, 3, " in singles[0].rollout_kernel()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_shared_moving_set_its_replacement_and_the_return_to_it(monkeypatch, graph):
    """The shared moving set for every agent, an own set for one agent in between, the shared one again, and (MPPI_GRAPH=1)
    graph replay across the replaced set: every stretch equals single handles driven the same way."""
    import dnn_mppi_mpc_amd as pkg
    if graph == "1":
        monkeypatch.setenv("MPPI_GRAPH", "1")
    T = 50
    sc, sets, x0, u = agent_scenes("diff", T)
    cfg = batch_cfg("diff", T, "f64")
    batch = pkg.Engine(K=K, n_agents=2, **cfg)
    singles = [pkg.Engine(K=K, noise_stream=a, **cfg) for a in range(2)]
    for e, xs, us in [(batch, x0[:2], u[:2])] + [(singles[a], x0[a], u[a]) for a in range(2)]:
        e.set_ref_path(sc["ref"])
        e.set_obstacles(*[sets[0][0]], velocities=sets[0][1])
        e.set_state(xs)
        e.set_u_prev(us)

    def run(n):
        for e in [batch] + singles:
            e.run_closed_loop(n)
        compare(batch, singles, None)
    run(4)
    set_agent(batch, 1, *sets[1])  # agent 1 gets its own moving set (uploaded at iteration 4: its clock starts there)
    singles[1].set_obstacles(sets[1][0], velocities=sets[1][1])
    run(4)
    batch.set_obstacles(sets[0][0], velocities=sets[0][1])  # back to a shared set for both
    for one in singles:
        one.set_obstacles(sets[0][0], velocities=sets[0][1])
    run(4)
    assert batch.stats.iteration == 12


# ------------------------------------------------------------------------------------------ 5. sharding
def test_sharded_pair_through_the_split_step_equals_the_whole():
    import torch
    T = 50
    sc = mc.diff_scene(T, False)
    whole = load(diff_engine(T, "frozen", False, "f64", seed=5), sc)
    parts = [load(diff_engine(T, "frozen", False, "f64", K=k, K_global=K, k_offset=o, seed=5), sc) for k, o in ((96, 0), (K - 96, 96))]
    n = whole.partial_len()
    x = sc["x0"].copy()
    hits = []
    for it in range(4):
        u_ref, u0_ref, st = whole.step(x)
        hits.append(st.n_collided)
        gathered = torch.empty(2 * n, dtype=torch.float64, device="cuda")
        for r, e in enumerate(parts):
            e.step_begin(x, None, gathered[r * n:(r + 1) * n])
        for u, u0, _ in [e.step_end(gathered, 2) for e in parts]:
            np.testing.assert_allclose(u, u_ref, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(u0, u0_ref, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(np.concatenate([e.costs() for e in parts]), whole.costs(), rtol=1e-12)
        x = x + 0.1 * np.array([u0_ref[0] * np.cos(x[2]), u0_ref[0] * np.sin(x[2]), u0_ref[1]])
    print("n_collided per iteration", hits)
    assert max(hits) > 0 and len(set(hits)) > 1


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_limit_and_change_nothing():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc = mc.diff_scene(T, False)
    with pytest.raises(pkg.MppiError) as ex:
        diff_engine(T, "frozen", False, "f32", obstacle_model=capi.OBSTACLE_NONE)
    assert ex.value.code == capi.ERR_BAD_ARG and "MPPI_OBSTACLE_NONE" in str(ex.value)
    with pytest.raises(pkg.MppiError) as ex:
        diff_engine(T, "frozen", False, "f32", model=capi.MODEL_DIFFDRIVE_MLP)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "MPPI_MODEL_DIFFDRIVE_MLP" in str(ex.value)
    with pytest.raises(pkg.MppiError) as ex:  # a batch beyond the one-sample-per-wave limit
        diff_engine(T, "frozen", False, "f32", K=16384, n_agents=2)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "K <= 8192" in str(ex.value)
    static = load(diff_engine(T, "frozen", False, "f64", obstacle_motion=0), sc, moving=False)
    with pytest.raises(pkg.MppiError) as ex:
        static.set_obstacles(sc["circles"], velocities=sc["vel"])
    assert ex.value.code == capi.ERR_STATE and "obstacle_motion" in str(ex.value)
    with pytest.raises(pkg.MppiError) as ex:
        static.set_obstacles(sc["circles"], agent=0, velocities=sc["vel"])
    assert ex.value.code == capi.ERR_STATE
    # a refused setter leaves the scene and the results as they were
    e = load(diff_engine(T, "frozen", False, "f64", seed=3), sc)
    twin = load(diff_engine(T, "frozen", False, "f64", seed=3), sc)
    bad = sc["vel"].copy()
    bad[1, 0] = np.nan
    with pytest.raises(pkg.MppiError) as ex:
        e.set_obstacles(sc["circles"] + 5.0, velocities=bad)
    assert ex.value.code == capi.ERR_BAD_ARG and "finite" in str(ex.value)
    bad[1, 0] = np.inf
    with pytest.raises(pkg.MppiError):
        e.set_obstacles(sc["circles"] + 5.0, velocities=bad)
    with pytest.raises(pkg.MppiError) as ex:
        e.eval_is_collided(np.zeros((2, 3)), steps=[0, -1])
    assert ex.value.code == capi.ERR_BAD_ARG
    for h in (e, twin):
        h.set_state(sc["x0"])
        h.run_closed_loop(3)
    assert e.stats.n_collided > 0
    np.testing.assert_array_equal(e.get_u_prev(), twin.get_u_prev())
    np.testing.assert_array_equal(e.costs(), twin.costs())


def test_controller_keyword_switches_motion_on():
    """`obstacle_velocities` on the controllers: last keyword, settable property; a controller built without it refuses."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 50
    sc, eps, o, res = diff_reference(T, False, "frozen")
    kw = dict(mc.DIFF_KW, ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T, obstacle_circles=sc["circles"])
    c = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", obstacle_velocities=sc["vel"])
    assert np.array_equal(c.obstacle_velocities, sc["vel"])
    c.u_prev[:] = sc["u"]
    c._calc_epsilon = lambda *a, **k: cuda(eps)
    _, u, _, _ = c._calc_input_control(sc["x0"])
    np.testing.assert_allclose(u, res["u_returned"], rtol=1e-8, atol=1e-10)
    c.obstacle_velocities = 0.5 * sc["vel"]  # settable, like obstacle_circles
    assert np.array_equal(c.obstacle_velocities, 0.5 * sc["vel"])
    plain = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen")
    assert plain.obstacle_velocities is None
    with pytest.raises(pkg.MppiError) as ex:
        plain.obstacle_velocities = sc["vel"]
    assert ex.value.code == capi.ERR_STATE and "obstacle_motion" in str(ex.value)
    rc = pkg.MPPIRacecarController(ref_path=mc.race_scene()["ref"], horizon_step_T=mc.RACE_T, number_of_samples_K=64,
                                   obstacle_circles=mc.race_scene()["circles"], obstacle_velocities=mc.race_scene()["vel"])
    assert rc._engine.cfg.obstacle_motion == 1
