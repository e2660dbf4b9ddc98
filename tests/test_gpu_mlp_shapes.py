"""Learned dynamics with residual MLPs of hidden width H in {64, 128, 256, 512} and depth n in {1, 2, 3, 4}: every shape but
512 x 3 and 512 x 2 runs k_rollout_mlp_w<H, ...>, against the f64 NumPy restatement (oracle/mppi_oracle.py)."""
import numpy as np
import pytest

from oracle import mppi_oracle, philox

pytestmark = pytest.mark.gpu

NEW_SHAPES = [(h, n) for h in (64, 128, 256) for n in (1, 2, 3, 4)] + [(512, 1), (512, 4)]


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, float) - np.asarray(b, float)) ** 2)))


def weights(H, n, seed):
    """The oracle's random weights with the hidden layers rescaled by sqrt(512 / H): the tanh layers stay nonlinear at
    small H (the same pre-activation spread as at 512)."""
    w = mppi_oracle.random_mlp_weights(seed, hidden=H, n_hidden=n)
    for i in range(n):
        w[f"hidden_layer.{i}.weight"] = (w[f"hidden_layer.{i}.weight"] * np.sqrt(512.0 / H)).astype(np.float32)
    return w


def kwargs(K, T, **over):
    """A softmin that is not one-hot (rate 1 / param_exploration = 20; ESS 40 .. 900 at K = 1500): the stage and terminal
    cost weights scaled by 0.01, and param_alpha = 0.99, so that the control cost gamma u' Sigma^-1 v (gamma =
    lambda (1 - alpha)) does not spread S by several units on its own."""
    kw = dict(delta_t=0.1, ref_path=mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100),
              max_speed=5.0, max_omega=3.14, num_samples_K=K, num_horizons_T=T, param_exploration=0.05,
              param_lambda=1.0, param_alpha=0.99, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              stage_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]), terminal_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    kw.update(over)
    return kw


def u_nominal(T):
    tt = np.arange(T)
    return np.stack([1.2 + 0.3 * np.sin(0.2 * tt), 0.05 * np.cos(0.1 * tt)], axis=1)


def frozen_reference(o, x0, u_in, eps, K_exploit):
    """S of the frozen waypoint index (every call searches from the x0 index), softmin weights and the returned controls."""
    K, T = eps.shape[:2]
    p0 = o.nearest_waypoint(x0[0], x0[1], 0)
    v = o.clamp(np.where((np.arange(K) < mppi_oracle.exploit_threshold(o.param_exploration, K_exploit))[:, None, None],
                         u_in[None] + eps, eps.astype(np.float64)))
    X = o.rollout(x0, v)
    R, win = o.ref_path, o.ref_path[p0:p0 + 20]
    xT, yT, yawT = X[:, -1, 0], X[:, -1, 1], X[:, -1, 2]
    i = p0 + np.argmin((xT[:, None] - win[:, 0]) ** 2 + (yT[:, None] - win[:, 1]) ** 2, axis=1)
    ws, wt = o.stage_cost_weight, o.terminal_cost_weight
    q = u_in[T - 1] @ np.linalg.inv(o.Sigma)
    S = ((ws[0] + wt[0]) * (xT - R[i, 0]) ** 2 + (ws[1] + wt[1]) * (yT - R[i, 1]) ** 2
         + (ws[2] + wt[2]) * (yawT - R[i, 2]) ** 2 + o.param_gamma * (q[0] * v[:, -1, 0] + q[1] * v[:, -1, 1]))
    w = o.compute_weight(S)
    un = u_in + mppi_oracle.moving_average_diffdrive(np.einsum("k,ktd->td", w, eps.astype(np.float64)), 10)
    return S, w, np.vstack([un[1:], un[-1:]])


@pytest.mark.parametrize("waypoint_mode", ["sequential", "frozen"])
@pytest.mark.parametrize("H,n", NEW_SHAPES)
def test_new_shapes_against_oracle(H, n, waypoint_mode):
    """Every new shape, K = 1500, T = 30, injected noise: u within 1e-4 RMSE, S to 1e-3, the softmin weights, the index."""
    import dnn_mppi_mpc_amd as pkg
    K, T = 1500, 30
    kw = kwargs(K, T)
    w = weights(H, n, 10 + H + n)
    eps = philox.sample_epsilon(kw["sigma"], 40 + n, 0, K, T)
    x0 = np.array([0.4, -0.1, -0.35])
    u_in = u_nominal(T)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
    o.u_prev[:] = u_in
    if waypoint_mode == "frozen":
        S_ref, w_ref, u_ref = frozen_reference(o, x0, u_in, eps, K)
        idx_ref = None
    else:
        ref = o.iteration(x0, eps.astype(np.float64))
        S_ref, w_ref, u_ref, idx_ref = ref["S"], ref["w"], ref["u_returned"], ref["idx_after"]
    c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, waypoint_mode=waypoint_mode)
    assert c._engine.rollout_kernel() == f"k_rollout_mlp_w<{H}, false>"
    c.u_prev[:] = u_in
    c._calc_epsilon = lambda *a, **k: eps
    u = c._calc_input_control(x0)[1]
    assert c.last_stats.ess >= 20
    np.testing.assert_allclose(c.sample_costs(), S_ref, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(c._engine.weights(), w_ref, rtol=1e-2, atol=1e-5)
    assert rmse(u, u_ref) <= 1e-4
    if idx_ref is not None:
        assert c.prev_way_point_idx == idx_ref


def test_per_rollout_index_new_shape():
    """MPPI_WAYPOINT_PER_ROLLOUT through k_rollout_mlp_w (128 x 3) against the NumPy per-rollout scan: S, the softmin
    weights, the returned controls and the index.  param_alpha = 0.998 here: with the faster nominal controls the control
    cost alone would otherwise make the softmin nearly one-hot (ESS ~ 300 of 512 this way)."""
    import torch

    import dnn_mppi_mpc_amd as pkg
    K, T = 512, 30
    w = weights(128, 3, 3)
    kw = kwargs(K, T, param_alpha=0.998)
    tt = np.arange(T)
    u_in = np.stack([2.0 + 0.3 * np.sin(0.2 * tt), -0.1 + 0.05 * np.cos(0.1 * tt)], axis=1)
    x0 = np.array([0.4, -0.1, -0.35])
    eps = philox.sample_epsilon(kw["sigma"], 92, 0, K, T)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
    v = o.clamp(np.where((np.arange(K) < mppi_oracle.exploit_threshold(kw["param_exploration"], K))[:, None, None],
                         u_in[None] + eps, eps.astype(np.float64)))
    X = o.rollout(x0, v)
    p0 = o.nearest_waypoint(x0[0], x0[1], 0)
    idx = mppi_oracle.per_rollout_waypoint_scan(X, o.ref_path[:, :2], p0, 20)
    R, ws, wt = o.ref_path, o.stage_cost_weight, o.terminal_cost_weight
    i_s, i_t = idx[:, T - 1], idx[:, T]
    xT, yT, yawT = X[:, -1, 0], X[:, -1, 1], X[:, -1, 2]
    q = u_in[T - 1] @ np.linalg.inv(o.Sigma)
    S_ref = (ws[0] * (xT - R[i_s, 0]) ** 2 + ws[1] * (yT - R[i_s, 1]) ** 2 + ws[2] * (yawT - R[i_s, 2]) ** 2
             + o.param_gamma * (q[0] * v[:, -1, 0] + q[1] * v[:, -1, 1])
             + wt[0] * (xT - R[i_t, 0]) ** 2 + wt[1] * (yT - R[i_t, 1]) ** 2 + wt[2] * (yawT - R[i_t, 2]) ** 2)
    assert (idx[:, -1] > p0).any()
    w_ref = o.compute_weight(S_ref)
    un = u_in + mppi_oracle.moving_average_diffdrive(np.einsum("k,ktd->td", w_ref, eps.astype(np.float64)), 10)
    u_ref = np.vstack([un[1:], un[-1:]])
    c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, waypoint_mode="per_rollout", seed=1)
    c.u_prev[:] = u_in
    c._calc_epsilon = lambda *a, **k: torch.from_numpy(eps).cuda()
    u = c._calc_input_control(x0)[1]
    assert c.last_stats.ess >= 20
    np.testing.assert_allclose(c.sample_costs(), S_ref, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(c._engine.weights(), w_ref, rtol=1e-2, atol=1e-5)
    assert rmse(u, u_ref) <= 1e-4
    assert c.prev_way_point_idx == p0


@pytest.mark.parametrize("H,n", [(64, 1), (128, 4)])
def test_visualisation_and_state_transition_new_shapes(H, n):
    """The visualisation rollouts (the reference's loop with the transition swapped) and the batched `_state_transition`
    through k_rollout_mlp_w<H, true>, against the f64 restatement: 1e-3 on the trajectories, 1e-5 on one step."""
    import dnn_mppi_mpc_amd as pkg
    K, T = 200, 20
    kw = kwargs(K, T, visualize_optimal_traj=True, visualze_sampled_trajs=True, max_speed=1.5)
    w = weights(H, n, 2)
    eps = philox.sample_epsilon(kw["sigma"], 33, 0, K, T)
    x0 = np.array([0.2, 0.1, -0.2])
    tt = np.arange(T)
    u_in = np.stack([1.3 + 0.4 * np.sin(0.3 * tt), 0.1 * np.cos(0.2 * tt)], axis=1)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
    o.u_prev[:] = u_in
    ref = o.iteration(x0, eps.astype(np.float64))
    opt_ref, smp_ref = o.viz_trajectories(x0, ref["u_pre_shift"], ref["v"])
    c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w)
    c.u_prev[:] = u_in
    c._calc_epsilon = lambda *a, **k: eps
    u0, u, opt, smp = c._calc_input_control(x0)
    assert rmse(u, ref["u_returned"]) <= 1e-4
    np.testing.assert_allclose(opt, opt_ref, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(smp, smp_ref, rtol=1e-3, atol=1e-3)
    opt_only, none = c._engine.rollout_viz(True, False)
    assert none is None
    np.testing.assert_allclose(opt_only.cpu().numpy(), opt_ref, rtol=1e-3, atol=1e-3)
    rng = np.random.default_rng(8)
    for m in (1, 5, 64, 131):
        x = rng.normal(0, 1.0, (m, 3))
        v = np.column_stack([rng.uniform(-2, 2, m), rng.uniform(-1, 1, m)])
        r = mppi_oracle.mlp_forward(w, np.concatenate([x, v], axis=1))
        f = np.stack([v[:, 0] * np.cos(x[:, 2]), v[:, 0] * np.sin(x[:, 2]), v[:, 1]], axis=1)
        np.testing.assert_allclose(c._state_transition(x, v), x + kw["delta_t"] * (f + r), rtol=1e-5, atol=1e-5)


def test_standard_scalers_new_shape():
    """The StandardScaler statistics (SURVEY.md App. C values) folded into the first and last Linear at 256 x 2."""
    import dnn_mppi_mpc_amd as pkg
    K, T = 512, 20
    kw = kwargs(K, T)
    w = weights(256, 2, 4)
    eps = philox.sample_epsilon(kw["sigma"], 35, 0, K, T)
    sc = dict(in_mean=np.array([4.390025834218122, -0.1261226463393075, -0.08013703690080425, 0.3585598113405002, -0.03134529264047761]),
              in_scale=np.array([5.586594593004116, 3.6412154342302943, 1.0597377625187672, 1.0238108433208775, 1.8363768322750769]),
              out_mean=np.array([-0.5611190600527631, 0.02943515716319776, -0.0151000663932475]) * 0.05,
              out_scale=np.array([5.701096415279686, 3.590083579774014, 0.9961674472612329]) * 0.05)

    class ScaledOracle(mppi_oracle.DiffDriveMlpOracle):
        def rollout(self, x0, v):
            K, T = v.shape[:2]
            X = np.empty((K, T, 3))
            s = np.tile(np.asarray(x0, np.float64), (K, 1))
            for t in range(T):
                z = (np.concatenate([s, v[:, t]], axis=1) - sc["in_mean"]) / sc["in_scale"]
                r = mppi_oracle.mlp_forward(self.mlp_weights, z) * sc["out_scale"] + sc["out_mean"]
                f = np.stack([v[:, t, 0] * np.cos(s[:, 2]), v[:, t, 0] * np.sin(s[:, 2]), v[:, t, 1]], axis=1)
                s = s + self.delta_t * (f + r)
                X[:, t] = s
            return X

    x0 = np.array([0.3, 0.2, 0.1])
    ref = ScaledOracle(**kw, mlp_weights=w).iteration(x0, eps.astype(np.float64))
    c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, learned_scalers=sc)
    c._calc_epsilon = lambda *a, **k: eps
    u = c._calc_input_control(x0)[1]
    np.testing.assert_allclose(c.sample_costs(), ref["S"], rtol=1e-3, atol=1e-3)
    assert rmse(u, ref["u_returned"]) <= 1e-4


@pytest.mark.parametrize("obstacles", [0, 5])
def test_zero_residual_new_shape_equals_analytic_kernel(obstacles):
    """out_layer = 0 at 64 x 3: the rollout reproduces the analytic kernel, with and without circular obstacles."""
    import dnn_mppi_mpc_amd as pkg
    K, T = 1024, 40
    kw = kwargs(K, T)
    w = weights(64, 3, 2)
    eps = philox.sample_epsilon(kw["sigma"], 37, 0, K, T)
    x0 = np.array([0.2, 0.1, -0.5])
    tt = np.arange(T)
    u_in = np.stack([1.0 + 0.2 * np.sin(0.2 * tt), 0.03 * np.cos(0.1 * tt)], axis=1)
    if obstacles:
        xe = x0.copy()
        for t in range(T):
            xe = mppi_oracle.diffdrive_plant_step(xe, u_in[t], kw["delta_t"])
        rng = np.random.default_rng(3)
        kw.update(obstacle_circles=np.column_stack([xe[0] + rng.uniform(-0.6, 0.6, obstacles), xe[1] + rng.uniform(-0.6, 0.6, obstacles),
                                                    rng.uniform(0.05, 0.2, obstacles)]), safety_margin_rate=0.8)
    w["out_layer.weight"][:] = 0
    w["out_layer.bias"][:] = 0
    a = pkg.MPPIAlgorithms(**kw)
    b = pkg.MPPIAlgorithms(**kw, learned_dynamics=w)
    assert b._engine.rollout_kernel() == "k_rollout_mlp_w<64, false>"
    for c in (a, b):
        c.u_prev[:] = u_in
        c._calc_epsilon = lambda *aa, **k: eps
    ua = a._calc_input_control(x0)[1].copy()
    ub = b._calc_input_control(x0)[1].copy()
    hit = a.sample_costs() > 1e9
    if obstacles:
        assert 0 < hit.sum() < K
    assert np.count_nonzero((b.sample_costs() > 1e9) != hit) <= 2
    same = (b.sample_costs() > 1e9) == hit
    np.testing.assert_allclose(b.sample_costs()[same & ~hit], a.sample_costs()[same & ~hit], rtol=2e-4, atol=2e-4)
    if np.array_equal(b.sample_costs() > 1e9, hit):
        assert rmse(ua, ub) <= 1e-4
    assert a.prev_way_point_idx == b.prev_way_point_idx


def test_noise_ring_new_shape():
    """128 x 3: a closed loop reading the sampler's tensors from the noise ring equals the in-kernel Philox closed loop."""
    import torch

    import dnn_mppi_mpc_amd as pkg
    w = weights(128, 3, 5)
    kw = kwargs(256, 20)
    a = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, waypoint_mode="frozen", seed=8)
    b = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, waypoint_mode="frozen", seed=8)
    for c in (a, b):
        c._engine.set_state(np.array([0.1, -0.05, 0.2]))
    ring = torch.stack([b._engine.sample_epsilon(i) for i in range(4)])
    b._engine.set_noise_ring(ring)
    a._engine.run_closed_loop(4)
    b._engine.run_closed_loop(4)
    np.testing.assert_allclose(b._engine.get_u_prev(), a._engine.get_u_prev(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(b._engine.get_state(), a._engine.get_state(), rtol=0, atol=1e-6)


def _mlp_engine(pkg, capi, K, w, **over):
    cfg = dict(model=capi.MODEL_DIFFDRIVE_MLP, K=K, T=30, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
               param_lambda=1.0, param_alpha=0.99, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[0.05, 0.05, 0.1, 0],
               terminal_cost_weight=[0.05, 0.05, 0.1, 0], search_window=20, filter_window=10, clamp_rollout=1,
               waypoint_mode=capi.WAYPOINT_FROZEN, precision=capi.PREC_F32)
    cfg.update(over)
    e = pkg.Engine(**cfg)
    e.set_ref_path(mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100))
    e.set_mlp(w)
    return e


def test_two_shards_in_one_process_new_shape():
    """K_global = 2K over two 128 x 3 handles (k_offset 0 and K, frozen index), merged by the split step: S bit-identical
    to one whole-K handle on the same noise, u within 1e-7 RMSE."""
    import torch

    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    K, T = 800, 30
    w = weights(128, 3, 6)
    eps = torch.from_numpy(philox.sample_epsilon(np.array([[0.1, 0.0], [0.0, 0.01]]), 44, 0, 2 * K, T)).cuda()
    x0 = np.array([0.4, -0.1, -0.35])
    u_in = u_nominal(T)
    parts = [_mlp_engine(pkg, capi, K, w, K_global=2 * K, k_offset=0), _mlp_engine(pkg, capi, K, w, K_global=2 * K, k_offset=K)]
    whole = _mlp_engine(pkg, capi, 2 * K, w)
    recs = torch.empty((2, parts[0].partial_len()), dtype=torch.float64, device="cuda")
    for e in parts + [whole]:
        e.set_u_prev(u_in)
    for r, e in enumerate(parts):
        e.step_begin(x0, eps[r * K:(r + 1) * K].contiguous(), recs[r])
    u_split = parts[0].step_end(recs.reshape(-1), 2)[0]
    S_split = np.concatenate([e.costs() for e in parts])
    u_whole = whole.step(x0, eps)[0]
    np.testing.assert_array_equal(S_split, whole.costs())
    assert rmse(u_split, u_whole) <= 1e-7


def test_reloading_a_model_drops_the_cached_graph(monkeypatch):
    """MPPI_GRAPH=1 replays long frozen-index closed loops from a captured graph, whose launches carry the model's
    weights and shape.  Loading another model on the same handle (256 x 3 -> 128 x 3, then the same shape with another
    output bias) must not replay the old one: the closed loop equals the eagerly launched one bit for bit.  (The widths only
    shrink here, so a stale replay would read repacked but allocated weights.)"""
    import dnn_mppi_mpc_amd as pkg
    models = [weights(256, 3, 21), weights(128, 3, 22), weights(128, 3, 22)]
    models[2]["out_layer.bias"] = (models[2]["out_layer.bias"] + np.float32(0.05)).astype(np.float32)

    def run():
        c = pkg.MPPIAlgorithms(**kwargs(512, 30), learned_dynamics=models[0], waypoint_mode="frozen", seed=4)
        e = c._engine
        out = []
        for m in models:
            e.set_mlp(m)
            e.set_state(np.array([0.1, -0.05, 0.2]))
            e.set_u_prev(u_nominal(30))
            e.run_closed_loop(150)  # long enough for graph replays (64 iterations per graph)
            out.append((e.get_u_prev().copy(), e.get_state().copy()))
        return out

    monkeypatch.delenv("MPPI_GRAPH", raising=False)
    eager = run()
    monkeypatch.setenv("MPPI_GRAPH", "1")
    graph = run()
    for (ue, xe), (ug, xg) in zip(eager, graph):
        np.testing.assert_array_equal(ug, ue)
        np.testing.assert_array_equal(xg, xe)
    assert not np.array_equal(eager[1][0], eager[2][0])  # (the bias change matters)


def test_full_size_k32768_subset_new_shape():
    """K = 32768, T = 50, 128 x 3, frozen index, in-kernel Philox: a strided 1024-sample subset of the costs against the
    f64 restatement; the softmin weights sum to one."""
    import dnn_mppi_mpc_amd as pkg
    K, T, seed = 32768, 50, 555
    w = weights(128, 3, 7)
    kw = kwargs(K, T)
    u_in = u_nominal(T)
    x0 = np.array([0.4, -0.1, -0.35])
    c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w, waypoint_mode="frozen", seed=seed)
    c.u_prev[:] = u_in
    u = c._calc_input_control(x0)[1].copy()
    S = c.sample_costs()
    assert S.shape == (K,) and np.isfinite(S).all()
    eps = philox.sample_epsilon(kw["sigma"], seed, 0, K, T)
    sub = np.arange(0, K, 32)
    o = mppi_oracle.DiffDriveMlpOracle(**dict(kw, num_samples_K=sub.size), mlp_weights=w)
    p0 = o.nearest_waypoint(x0[0], x0[1], 0)
    exploit = (sub < mppi_oracle.exploit_threshold(kw["param_exploration"], K))[:, None, None]
    v = o.clamp(np.where(exploit, u_in[None] + eps[sub], eps[sub].astype(np.float64)))
    X = o.rollout(x0, v)
    R, win = o.ref_path, o.ref_path[p0:p0 + 20]
    xT, yT, yawT = X[:, -1, 0], X[:, -1, 1], X[:, -1, 2]
    i = p0 + np.argmin((xT[:, None] - win[:, 0]) ** 2 + (yT[:, None] - win[:, 1]) ** 2, axis=1)
    ws, wt = o.stage_cost_weight, o.terminal_cost_weight
    q = u_in[T - 1] @ np.linalg.inv(o.Sigma)
    S_ref = ((ws[0] + wt[0]) * (xT - R[i, 0]) ** 2 + (ws[1] + wt[1]) * (yT - R[i, 1]) ** 2
             + (ws[2] + wt[2]) * (yawT - R[i, 2]) ** 2 + o.param_gamma * (q[0] * v[:, -1, 0] + q[1] * v[:, -1, 1]))
    np.testing.assert_allclose(S[sub], S_ref, rtol=1e-3, atol=1e-3)
    e = np.exp(-(S - S.min()) / kw["param_exploration"])  # (the diff-drive softmin's rate: 1 / param_exploration)
    wk = e / e.sum()
    np.testing.assert_allclose(c._compute_weight(), wk, rtol=1e-5, atol=1e-12)
    un = u_in + mppi_oracle.moving_average_diffdrive(np.einsum("k,ktd->td", wk, eps.astype(np.float64)), 10)
    assert rmse(u, np.vstack([un[1:], un[-1:]])) <= 1e-4


def plan_name(H, n, agents, scene):
    """The kernel plan_mlp selects for a rollout: shape x one agent or a batch x a static or a scene handle."""
    tail = ("_scene" if scene else "") + ("_agents" if agents > 1 else "")
    if H == 512 and n in (2, 3):  # the default form of the 512 x 3 / 512 x 2 kernel
        return f"k_rollout_mlp_h3{tail}" + ("" if scene else "<8, 2, 3>" if agents > 1 else "<false, 8, 2, 3>")
    return f"k_rollout_mlp_w{tail}<{H}>" if tail else f"k_rollout_mlp_w<{H}, false>"


PLAN_SHAPES = [(h, n) for h in (64, 128, 256, 512) for n in (1, 3)] + [(512, 2), (512, 4)]


@pytest.mark.parametrize("H,n", PLAN_SHAPES)
def test_plan_table(H, n):
    """The host dispatch over shape x {one agent, two agents} x obstacle_motion {0, 2}: the exact kernel name, and that the
    launch ran (finite controls and costs).  K = 65: one full 64-sample tile and a ragged one; T = 7; in-kernel Philox; an
    empty scene.  Pinned elsewhere by an exact rollout_kernel() assertion: every static single-agent shape
    (test_new_shapes_against_oracle, test_gpu_mlp_agents), the static batches of 512 x 3, 128 x 3, 64 x 1 and 256 x 2
    (test_gpu_mlp_agents), the scene handles of 64 x 1, 128 x 2, 256 x 3 and 512 x 3 and the scene batches of 64 x 1 and 512 x 3
    (test_gpu_mlp_scenes), MPPI_MLP_FORM / _TERMS / _F32 (test_gpu_engine).  New here, of this table's ten shapes: the static batches of
    seven (all but 64 x 1, 128 x 3, 512 x 3), the scene handles and the scene batches of eight each (all but 64 x 1, 512 x 3)."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    K, T = 65, 7
    w = weights(H, n, 50 + H + n)
    x0 = np.array([[0.4, -0.1, -0.35], [0.3, 0.1, -0.2]])
    for motion in (0, 2):
        for agents in (1, 2):
            e = _mlp_engine(pkg, capi, K, w, T=T, filter_window=5, seed=3, obstacle_model=capi.OBSTACLE_CIRCLE,
                            obstacle_motion=motion, n_agents=agents)
            e.set_u_prev(u_nominal(T) if agents == 1 else np.stack([u_nominal(T)] * agents))
            if agents == 1:
                u = e.step(x0[0])[0]
            else:
                e.set_state(x0)
                e.run_closed_loop(1)
                u = e.get_u_prev()
            assert e.rollout_kernel() == plan_name(H, n, agents, motion == 2), (motion, agents)
            S = e.costs()
            assert S.shape == ((K,) if agents == 1 else (agents, K)) and np.isfinite(S).all() and np.isfinite(u).all()
            e.close()


def test_dispatch_and_refusals():
    """rollout_kernel() names the kernel that serves the shape; shapes outside the set are refused naming the set, by the
    Python layer (ValueError) and by the C ABI (MPPI_ERR_SHAPE); a weight beyond the f16 range on a new shape is refused
    with MPPI_ERR_UNSUPPORTED (no f32-input kernel serves it), as is MPPI_MLP_F32=1."""
    import ctypes as C
    import os

    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    kw = kwargs(256, 20)
    assert pkg.MPPIAlgorithms(**kw, learned_dynamics=weights(128, 2, 1))._engine.rollout_kernel() == "k_rollout_mlp_w<128, false>"
    assert pkg.MPPIAlgorithms(**kw, learned_dynamics=mppi_oracle.random_mlp_weights(1))._engine.rollout_kernel() == \
        "k_rollout_mlp_h3<false, 8, 2, 3>"
    for H, n in ((32, 3), (96, 3), (1024, 1), (128, 0), (128, 5)):
        w = mppi_oracle.random_mlp_weights(1, hidden=H, n_hidden=n)
        with pytest.raises(ValueError, match=r"\{64, 128, 256, 512\} x n_hidden in \{1, 2, 3, 4\}"):
            pkg.MPPIAlgorithms(**kw, learned_dynamics=w)
        # the same refusal one layer down
        cfg = dict(model=capi.MODEL_DIFFDRIVE_MLP, K=256, T=20, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                   param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0],
                   terminal_cost_weight=[5, 5, 10, 0], search_window=20, filter_window=10, precision=capi.PREC_F32)
        e = pkg.Engine(**cfg)
        f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        keep = [np.zeros((H, 5), np.float32), np.zeros(H, np.float32), np.zeros((3, H), np.float32), np.zeros(3, np.float32),
                np.zeros((H, H), np.float32), np.zeros(H, np.float32)]
        wh = (C.POINTER(C.c_float) * 1)(f(keep[4]))
        bh = (C.POINTER(C.c_float) * 1)(f(keep[5]))
        rc = e.lib.mppi_set_mlp(e._h, H, n, f(keep[0]), f(keep[1]), wh, bh, f(keep[2]), f(keep[3]))
        assert rc == capi.ERR_SHAPE
        assert "{64, 128, 256, 512} x n_hidden in {1, 2, 3, 4}" in e.lib.mppi_last_error(e._h).decode()
    # a hidden weight beyond 65504 at H = 128: no f32-input kernel for this shape
    w = weights(128, 3, 1)
    w["hidden_layer.1.weight"][3, 7] = 1e5
    with pytest.raises(pkg.MppiError) as ex:
        pkg.MPPIAlgorithms(**kw, learned_dynamics=w)
    assert ex.value.code == capi.ERR_UNSUPPORTED and "f16 range" in str(ex.value)
    os.environ["MPPI_MLP_F32"] = "1"
    try:
        with pytest.raises(pkg.MppiError) as ex:
            pkg.MPPIAlgorithms(**kw, learned_dynamics=weights(64, 2, 1))
        assert ex.value.code == capi.ERR_UNSUPPORTED and "MPPI_MLP_F32" in str(ex.value)
    finally:
        os.environ.pop("MPPI_MLP_F32", None)
