"""Batched handles (mppi_config.n_agents > 1) whose agents each follow their own reference path and see their own obstacles
(mppi_set_agent_ref_path / mppi_set_agent_obstacles / mppi_get_agent_status).  The yardstick throughout is the
same problem in separate single-agent handles: agent a of the batch against a handle with noise_stream = a, agent a's path and
circles and the same x0 / u_prev, closed loop, with the tolerances test_gpu_engine.py and test_gpu_mlp_agents.py use for that
comparison (bit for bit / 1e-12 where batch and single take the same layout, the f64 re-association bound where they do not)."""
import numpy as np
import pytest

from oracle import mppi_oracle
from test_gpu_mlp_agents import agent_inputs, base_cfg
from test_gpu_mlp_shapes import frozen_reference, rmse, weights

pytestmark = pytest.mark.gpu

FAR = 1.0e3  # circles out there are never hit: they fill a table up to its size


def line(p, q, n):
    return mppi_oracle.generate_point_trajectory(p, q, n)


def table(near, m):
    """m circles: the `near` ones first and last (a set of 70 keeps some beyond the 64 lanes of ObsLanes), far ones between."""
    near = np.asarray(near, dtype=np.float64).reshape(-1, 3)
    if m == 0:
        return np.zeros((0, 3))
    out = np.stack([[FAR + 3.0 * i, FAR, 0.5] for i in range(m)])
    half = (len(near) + 1) // 2
    out[:half] = near[:half]
    if len(near) > half:
        out[m - (len(near) - half):] = near[half:]
    return out


def diff_cfg(waypoint_mode, T, precision=None):
    from dnn_mppi_mpc_amd import _capi as capi
    return dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
                param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
                search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=waypoint_mode,
                obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10, seed=99,
                precision=capi.PREC_F64 if precision is None else precision)


def diff_scenes(T, lengths=(100, 12, 600), counts=(70, 0, 2)):
    """Three diff-drive agents: paths of `lengths` waypoints, `counts` circles, x0 beside the start of the own path, constant
    nominal controls.  `S[k] =` prices the LAST state only (mppi_differential_drive.py:124), so the circles sit where the
    nominal rollout ends: one whose threshold circle (0.5 * 0.8 + 0.4 = 0.8) passes through that point, one a little further
    off on the other side -- the samples end within ~0.2 m of it (sigma_v 0.32 per step over T steps of 0.1 s)."""
    ends = [((0.0, 0.0), (10.0, -5.0)), ((0.0, 1.0), (6.0, 4.0)), ((1.0, -1.0), (31.0, -16.0))]
    paths, x0, u, circles = [], [], [], []
    rng = np.random.default_rng(3)
    for a, ((p, q), n, m) in enumerate(zip(ends, lengths, counts)):
        path = line(p, q, n)
        yaw = path[0, 2]
        s = np.array([p[0] + 0.1, p[1] - 0.05 * a, yaw + 0.05 * (a - 1)])
        v = 0.6 + 0.1 * a
        end = s[:2] + T * 0.1 * v * np.array([np.cos(s[2]), np.sin(s[2])])
        nrm = np.array([-np.sin(s[2]), np.cos(s[2])])
        near = [[*(end + 0.8 * nrm), 0.4], [*(end - 1.0 * nrm), 0.4], [*(end + 0.9 * nrm + 0.3), 0.4], [*(end - 1.1 * nrm - 0.2), 0.4]]
        paths.append(path)
        x0.append(s)
        u.append(np.stack([np.full(T, v), np.zeros(T)], axis=1) + rng.normal(0, 0.02, (T, 2)))
        circles.append(table(near[:m] if m < 4 else near, m))
    return paths, np.stack(x0), np.stack(u), circles


def race_cfg():
    from dnn_mppi_mpc_amd import _capi as capi
    return dict(model=capi.MODEL_RACECAR, T=40, delta_t=0.05, u_max=[0.523, 2.0], wheel_base=2.5, param_exploration=0.1,
                param_lambda=50.0, param_alpha=0.9, sigma=[0.5, 0.0, 0.0, 0.1], stage_cost_weight=[50.0, 50.0, 1.0, 20.0],
                terminal_cost_weight=[50.0, 50.0, 1.0, 20.0], beta_mode=capi.BETA_INV_LAMBDA, accumulate_stage_cost=1,
                waypoint_mode=capi.WAYPOINT_FROZEN, search_window=200, wrap_yaw_stage=1, wrap_yaw_terminal=1,
                clamp_rollout=1, clamp_u_after_update=1, filter_mode=capi.FILTER_RACECAR, filter_window=10,
                obstacle_model=capi.OBSTACLE_OUTLINE, safety_margin=1.5, vehicle_w=3.0, vehicle_l=4.0,
                collision_penalty=1e10, seed=7, precision=capi.PREC_F32)


def race_scenes(lengths=(12, 600, 100), counts=(0, 2, 70)):
    """Three race cars on lemniscates of different radius and resolution, each starting on its own path; circles of radius 1
    three metres beside the path ahead (`S[k] +=`: every step is tested; the outline's side points pass within a metre of
    them when the car drives straight on, and the steering noise takes many samples clear)."""
    paths, x0, circles = [], [], []
    for a, (n, m) in enumerate(zip(lengths, counts)):
        path = mppi_oracle.generate_lemniscate_racecar(n, 10.0 + 2.0 * a).astype(np.float64)
        i0 = max(1, n // 50)
        s = path[i0].copy()
        h = np.array([np.cos(s[2]), np.sin(s[2])])
        nrm = np.array([-h[1], h[0]])
        near = [[*(s[:2] + 5.0 * h + 3.0 * nrm), 1.0], [*(s[:2] + 8.0 * h - 3.0 * nrm), 1.0],
                [*(s[:2] + 3.0 * h - 3.2 * nrm), 1.0], [*(s[:2] + 7.0 * h + 3.3 * nrm), 1.0]]
        paths.append(path)
        x0.append(s)
        circles.append(table(near[:m] if m < 4 else near, m))
    u = np.random.default_rng(3).normal(0, 0.1, (len(lengths), 40, 2))
    return paths, np.stack(x0), u, circles


def make_batch(cfg, K, paths, x0, u, circles):
    """A batched handle with every agent's own path and circles (circles None: the handle has no obstacles at all)."""
    import dnn_mppi_mpc_amd as pkg
    e = pkg.Engine(K=K, n_agents=len(paths), **cfg)
    for a, path in enumerate(paths):
        e.set_ref_path(path, agent=a)
        if circles is not None:
            e.set_obstacles(circles[a], agent=a)
    e.set_state(x0)
    e.set_u_prev(u)
    return e


def make_single(cfg, K, path, x0, u, circles, a):
    import dnn_mppi_mpc_amd as pkg
    e = pkg.Engine(K=K, noise_stream=a, **cfg)
    e.set_ref_path(path)
    if circles is not None:
        e.set_obstacles(circles)
    e.set_state(x0)
    e.set_u_prev(u)
    return e


def compare(batch, singles, tol):
    """u_prev, state, costs and waypoint index of every agent against its single-agent handle (tol None: bit for bit)."""
    ub, xb, Sb = batch.get_u_prev(), batch.get_state(), batch.costs()
    idx, _ = batch.agent_status()
    for a, one in enumerate(singles):
        for got, ref in ((ub[a], one.get_u_prev()), (xb[a], one.get_state()), (Sb[a], one.costs())):
            if tol is None:
                np.testing.assert_array_equal(got, ref)
            else:
                np.testing.assert_allclose(got, ref, **tol)
        assert idx[a] == one.get_waypoint_idx()
    for a in range(len(singles)):  # the agents are different problems
        for b in range(a):
            assert not np.array_equal(ub[a], ub[b])


def assert_scenes_matter(singles, circles):
    """The last iteration of the single-agent handles: some samples of an agent with circles carry a collision penalty, none of
    an agent without -- the scene cannot silently have become irrelevant."""
    hits = [int(one.stats.n_collided) for one in singles]
    print("n_collided per agent:", hits)
    assert any(h > 0 for h, c in zip(hits, circles) if len(c) > 0)
    assert all(h == 0 for h, c in zip(hits, circles) if len(c) == 0)


@pytest.mark.parametrize("dual", ["0", "1"])
@pytest.mark.parametrize("model", ["diff", "race"])
def test_own_scenes_equal_separate_handles(monkeypatch, dual, model):
    """B = 3, K = 300, 6 iterations: paths of 12 (shorter than the search window), 100 and 600 waypoints, 0, 2 and 70 circles
    (beyond the 64 lanes of the obstacle table) -- diff-drive f64 with circles, race car f32 with the outline model, one and
    two samples per wave."""
    from dnn_mppi_mpc_amd import _capi as capi
    monkeypatch.setenv("MPPI_DUAL", dual)
    K, n_it = 300, 6
    if model == "diff":
        cfg = diff_cfg(capi.WAYPOINT_FROZEN, 50)
        paths, x0, u, circles = diff_scenes(50)
        tol = dict(rtol=1e-12, atol=1e-14)
    else:
        cfg = race_cfg()
        paths, x0, u, circles = race_scenes()
        tol = dict(rtol=1e-6, atol=1e-7)
    assert sorted(len(p) for p in paths) == [12, 100, 600] and sorted(len(c) for c in circles) == [0, 2, 70]
    batch = make_batch(cfg, K, paths, x0, u, circles)
    batch.run_closed_loop(n_it)
    singles = [make_single(cfg, K, paths[a], x0[a], u[a], circles[a], a) for a in range(3)]
    for one in singles:
        one.run_closed_loop(n_it)
    assert_scenes_matter(singles, circles)
    compare(batch, singles, tol)
    assert batch.counters()["rollout_launches"] == n_it and batch.counters()["finalize_launches"] == n_it


def test_own_scenes_per_rollout_index():
    """MPPI_WAYPOINT_PER_ROLLOUT, diff-drive: the same three paths -- 600 waypoints exceed the 512 the threading kernel keeps
    in LDS, so one launch mixes the LDS copy and the cached path."""
    from dnn_mppi_mpc_amd import _capi as capi
    K, T, n_it = 300, 40, 5
    cfg = diff_cfg(capi.WAYPOINT_PER_ROLLOUT, T)
    paths, x0, u, circles = diff_scenes(T)
    batch = make_batch(cfg, K, paths, x0, u, circles)
    batch.run_closed_loop(n_it)
    singles = [make_single(cfg, K, paths[a], x0[a], u[a], circles[a], a) for a in range(3)]
    for one in singles:
        one.run_closed_loop(n_it)
    assert_scenes_matter(singles, circles)
    compare(batch, singles, dict(rtol=1e-12, atol=1e-14))


def test_own_scenes_streaming_layout():
    """B = 4 agents of K = 2048, f64, frozen index: 8192 samples per launch take the two-samples-per-wave layout and the
    streaming kernel, a single agent of K = 2048 the one-sample layout -- equal to the re-association of the prefix sums."""
    from dnn_mppi_mpc_amd import _capi as capi
    K, T, n_it = 2048, 50, 3
    cfg = diff_cfg(capi.WAYPOINT_FROZEN, T)
    paths, x0, u, circles = diff_scenes(T)
    paths.append(line((-1.0, 2.0), (7.0, 9.0), 40))  # a fourth agent, sharing no path with the others
    x0 = np.vstack([x0, [-0.9, 2.0, paths[3][0, 2] + 0.1]])
    u = np.concatenate([u, u[1:2] * 0.9])
    end = x0[3, :2] + T * 0.1 * u[3, 0, 0] * np.array([np.cos(x0[3, 2]), np.sin(x0[3, 2])])  # where its nominal rollout ends
    circles.append(table([[*(end + 0.8 * np.array([-np.sin(x0[3, 2]), np.cos(x0[3, 2])])), 0.4]], 1))
    batch = make_batch(cfg, K, paths, x0, u, circles)
    batch.run_closed_loop(n_it)
    assert batch.counters()["rollout_layout"] & capi.LAYOUT_KIND == capi.LAYOUT_DUAL
    assert batch.rollout_kernel().startswith("k_rollout_stream<double, true, true")
    singles = [make_single(cfg, K, paths[a], x0[a], u[a], circles[a], a) for a in range(4)]
    for one in singles:
        one.run_closed_loop(n_it)
        assert one.counters()["rollout_layout"] & capi.LAYOUT_KIND == capi.LAYOUT_FUSED
    assert_scenes_matter(singles, circles)
    compare(batch, singles, dict(rtol=1e-9, atol=1e-11))


MLP_PATHS = [line((0.0, 0.0), (10.0, -5.0), 100), line((-0.5, 0.5), (12.0, -4.0), 200), line((0.2, 0.3), (9.0, -6.0), 100)]


def mlp_circles(x0, u, counts=(2, 3, 0)):
    """Circles of radius 0.6 (the handle's margin is 0: the threshold is the radius) either side of where each agent's nominal
    controls take the unicycle (`S[k] =` prices the last state; the learned residual moves it by centimetres): one whose edge
    lies 0.1 m beyond that point, one 0.1 m short of it."""
    out = []
    for a, m in enumerate(counts):
        x, y, yaw = x0[a]
        for v, w in u[a]:
            x, y, yaw = x + 0.1 * v * np.cos(yaw), y + 0.1 * v * np.sin(yaw), yaw + 0.1 * w
        nrm = np.array([-np.sin(yaw), np.cos(yaw)])
        out.append(table([[x + 0.5 * nrm[0], y + 0.5 * nrm[1], 0.6], [x - 0.7 * nrm[0], y - 0.7 * nrm[1], 0.6]], m))
    return out


def make_mlp(cfg, K, w, paths, x0, u, circles, n_agents=1, noise_stream=0):
    import dnn_mppi_mpc_amd as pkg
    e = pkg.Engine(K=K, n_agents=n_agents, noise_stream=noise_stream, **cfg)
    if n_agents > 1:
        for a in range(n_agents):
            e.set_ref_path(paths[a], agent=a)
            e.set_obstacles(circles[a], agent=a)
    else:
        e.set_ref_path(paths)
        e.set_obstacles(circles)
    e.set_mlp(w)
    e.set_state(x0)
    e.set_u_prev(u)
    return e


@pytest.mark.parametrize("waypoint_mode", ["frozen", "per_rollout"])
@pytest.mark.parametrize("H,n", [(64, 1), (256, 3)])
def test_learned_dynamics_own_scenes_equal_separate_handles(H, n, waypoint_mode):
    """B = 3, K = 256: paths of 100 and 200 waypoints -- at 256 x 3 the path's room in LDS is 128 waypoints, so one agent
    stages its path and its neighbour reads memory -- bit for bit against single-agent handles."""
    B, K, T, n_it = 3, 256, 30, 5
    cfg = base_cfg(waypoint_mode, T)
    w = weights(H, n, 11 + H + n)
    x0, u = agent_inputs(B, T)
    circles = mlp_circles(x0, u)
    batch = make_mlp(cfg, K, w, MLP_PATHS, x0, u, circles, n_agents=B)
    batch.run_closed_loop(n_it)
    assert batch.rollout_kernel() == f"k_rollout_mlp_w_agents<{H}>"
    singles = [make_mlp(cfg, K, w, MLP_PATHS[a], x0[a], u[a], circles[a], noise_stream=a) for a in range(B)]
    for one in singles:
        one.run_closed_loop(n_it)
    assert_scenes_matter(singles, circles)
    compare(batch, singles, None)


@pytest.mark.parametrize("H,n", [(64, 1), (256, 3)])
def test_learned_dynamics_own_scene_against_the_oracle(H, n):
    """Agent 2 of the batch -- its own path, no circles beside neighbours that have some -- equals the f64 oracle on the
    injected noise of one iteration: u within 1e-4 RMSE, S within 1e-3 (the bounds of test_gpu_mlp_agents.py)."""
    B, K, T, ag = 3, 512, 30, 2
    cfg = base_cfg("frozen", T)
    w = weights(H, n, 31 + H)
    x0, u = agent_inputs(B, T)
    e = make_mlp(cfg, K, w, MLP_PATHS, x0, u, mlp_circles(x0, u), n_agents=B)
    eps = e.sample_epsilon(0)
    e.set_noise_ring(eps[None].contiguous())
    e.run_closed_loop(1)
    kw = dict(delta_t=0.1, ref_path=MLP_PATHS[ag], max_speed=5.0, max_omega=3.14, num_samples_K=K, num_horizons_T=T,
              param_exploration=0.05, param_lambda=1.0, param_alpha=0.99, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              stage_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]), terminal_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
    S_ref, _, u_ref = frozen_reference(o, x0[ag], u[ag], eps[ag].cpu().numpy(), K)
    np.testing.assert_allclose(e.costs()[ag], S_ref, rtol=1e-3, atol=1e-3)
    assert rmse(e.get_u_prev()[ag], u_ref) <= 1e-4


def test_shared_setters_return_the_batch_to_the_shared_scene():
    """After per-agent setters (and a run with them), set_ref_path / set_obstacles without an agent give the outputs of a fresh
    batch that only ever had the shared scene; so does a batch whose agents were each handed that scene one by one."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    K, T, n_it = 300, 50, 4
    cfg = diff_cfg(capi.WAYPOINT_FROZEN, T)
    paths, x0, u, circles = diff_scenes(T)
    shared_path, shared_circles = paths[0], circles[2]

    def outputs(e):
        e.set_iteration(0)
        e.set_waypoint_idx(0)
        e.set_state(x0)
        e.set_u_prev(u)
        e.run_closed_loop(n_it)
        return e.get_u_prev(), e.get_state(), e.costs(), e.agent_status()[0]

    fresh = pkg.Engine(K=K, n_agents=3, **cfg)
    fresh.set_ref_path(shared_path)
    fresh.set_obstacles(shared_circles)
    ref = outputs(fresh)

    back = make_batch(cfg, K, paths, x0, u, circles)
    back.run_closed_loop(2)
    back.set_ref_path(shared_path)
    back.set_obstacles(shared_circles)
    one_by_one = pkg.Engine(K=K, n_agents=3, **cfg)
    for a in range(3):
        one_by_one.set_ref_path(shared_path, agent=a)
        one_by_one.set_obstacles(shared_circles, agent=a)
    for e in (back, one_by_one):
        for got, want in zip(outputs(e), ref):
            np.testing.assert_array_equal(got, want)
    assert not np.array_equal(ref[0][0], ref[0][1])


def test_path_end_names_the_agent():
    """Race car, raise_at_path_end: agent 1 starts two waypoints before the end of a short path and reaches it within the call;
    the call raises MPPI_ERR_PATH_END, agent_status() says it was agent 1, and every agent's index is its single handle's."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    K, n_it = 300, 12
    cfg = dict(race_cfg(), raise_at_path_end=1, obstacle_model=capi.OBSTACLE_NONE)
    full = mppi_oracle.generate_lemniscate_racecar(100, 10.0).astype(np.float64)
    paths = [full, full[:30].copy(), mppi_oracle.generate_lemniscate_racecar(150, 12.0).astype(np.float64)]
    x0 = np.stack([paths[0][2], paths[1][27], paths[2][5]])
    u = np.random.default_rng(5).normal(0, 0.1, (3, 40, 2))
    singles = [make_single(cfg, K, paths[a], x0[a], u[a], None, a) for a in range(3)]
    ended = []
    for one in singles:
        try:
            one.run_closed_loop(n_it)
            ended.append(False)
        except pkg.MppiError as ex:
            assert ex.code == capi.ERR_PATH_END
            ended.append(True)
    assert ended == [False, True, False]  # the start was chosen so: only agent 1's own handle reaches the end within the call
    batch = make_batch(cfg, K, paths, x0, u, None)
    with pytest.raises(pkg.MppiError) as ex:
        batch.run_closed_loop(n_it)
    assert ex.value.code == capi.ERR_PATH_END
    idx, path_end = batch.agent_status()
    assert list(path_end) == [False, True, False]
    for a, one in enumerate(singles):
        i1, e1 = one.agent_status()
        assert idx[a] == i1[0] and bool(path_end[a]) == bool(e1[0])
    assert idx[1] == len(paths[1]) - 1
    for a in (0, 2):  # the others went on to the end of the call
        np.testing.assert_allclose(batch.get_u_prev()[a], singles[a].get_u_prev(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(batch.get_state()[a], singles[a].get_state(), rtol=1e-6, atol=1e-7)


def test_refusals():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    K, T = 300, 50
    cfg = diff_cfg(capi.WAYPOINT_FROZEN, T)
    paths, x0, u, circles = diff_scenes(T)

    def refused(code, fn):
        with pytest.raises(pkg.MppiError) as ex:
            fn()
        assert ex.value.code == code, ex.value

    e = pkg.Engine(K=K, n_agents=3, **cfg)
    for agent in (-1, 3):
        refused(capi.ERR_BAD_ARG, lambda: e.set_ref_path(paths[0], agent=agent))
        refused(capi.ERR_BAD_ARG, lambda: e.set_obstacles(circles[0], agent=agent))
    e.set_ref_path(paths[0], agent=0)
    e.set_ref_path(paths[1], agent=1)
    e.set_state(x0)
    refused(capi.ERR_STATE, lambda: e.run_closed_loop(1))  # agent 2 has no path yet
    refused(capi.ERR_SHAPE, lambda: e.set_ref_path(paths[2][:, :2], agent=2))
    race = pkg.Engine(K=K, n_agents=2, **race_cfg())
    refused(capi.ERR_SHAPE, lambda: race.set_ref_path(paths[0], agent=1))  # the race car's path has four columns
    e.set_ref_path(paths[2], agent=2)
    refused(capi.ERR_BAD_ARG, lambda: e.set_waypoint_idx(12))  # beyond agent 1's 12 waypoints
    e.set_waypoint_idx(11)
    e.set_waypoint_idx(0)
    e.run_closed_loop(1)

    def single(agent):
        one = pkg.Engine(K=K, **cfg)
        if agent is None:
            one.set_ref_path(paths[0])
            one.set_obstacles(circles[0])
        else:
            one.set_ref_path(paths[0], agent=agent)
            one.set_obstacles(circles[0], agent=agent)
        one.set_state(x0[0])
        one.set_u_prev(u[0])
        one.run_closed_loop(3)
        return one.get_u_prev(), one.get_state(), one.costs()

    for got, want in zip(single(0), single(None)):
        np.testing.assert_array_equal(got, want)
    one = pkg.Engine(K=K, **cfg)
    refused(capi.ERR_BAD_ARG, lambda: one.set_ref_path(paths[0], agent=1))


def test_replacing_a_path_drops_the_stale_graph(monkeypatch):
    """MPPI_GRAPH=1: 150 iterations, agent 2's path replaced by one of another length, 150 more -- bit for bit the same
    sequence launched eagerly (modelled on test_reloading_a_model_drops_the_cached_graph)."""
    from dnn_mppi_mpc_amd import _capi as capi
    K, T = 256, 30
    cfg = diff_cfg(capi.WAYPOINT_FROZEN, T, precision=capi.PREC_F32)
    paths, x0, u, circles = diff_scenes(T, lengths=(100, 60, 300), counts=(2, 0, 70))
    paths.append(line((-1.0, 2.0), (7.0, 9.0), 80))
    x0 = np.vstack([x0, [-0.9, 2.0, paths[3][0, 2]]])
    u = np.concatenate([u, u[:1]])
    circles.append(np.zeros((0, 3)))
    other = line((1.0, -1.0), (25.0, -10.0), 450)

    def run():
        e = make_batch(cfg, K, paths, x0, u, circles)
        out = []
        e.run_closed_loop(150)
        out.append((e.get_u_prev(), e.get_state(), e.costs(), e.agent_status()[0]))
        e.set_ref_path(other, agent=2)
        e.run_closed_loop(150)
        out.append((e.get_u_prev(), e.get_state(), e.costs(), e.agent_status()[0]))
        return out, e.counters()

    monkeypatch.delenv("MPPI_GRAPH", raising=False)
    eager, c_eager = run()
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph, c_graph = run()
    for ref, got in zip(eager, graph):
        for r, g in zip(ref, got):
            np.testing.assert_array_equal(g, r)
    assert c_graph["iterations"] == c_eager["iterations"] == 300
    assert c_graph["rollout_launches"] == c_eager["rollout_launches"] == 300
    assert not np.array_equal(eager[0][0][2], eager[1][0][2])
