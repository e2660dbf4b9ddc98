"""A residual model per agent of a batched learned-dynamics handle (mppi_set_agent_mlp, Engine.set_mlp(..., agent=a); DESIGN
3.6.2): the batched kernels read agent blockIdx.y's entry of a device table of MlpParams.  Checked against the same problems
in separate single-agent handles (noise_stream = the agent) bit for bit, against the f64 oracle, under graph replay, with
scalers and own scenes, and for the refusals."""
import numpy as np
import pytest

from oracle import mppi_oracle
from test_gpu_mlp_agents import OBSTACLES, REF, agent_inputs, base_cfg, batched_name, make
from test_gpu_mlp_shapes import frozen_reference, rmse, weights

pytestmark = pytest.mark.gpu


def results(e):
    return e.get_u_prev(), e.get_state(), e.costs()


def assert_agent_equals(batch_out, a, one):
    for got, ref in zip(batch_out, results(one)):
        np.testing.assert_array_equal(got[a], ref)


def make_own(cfg, K, ws, x0, u, obstacles=True):
    """A batched handle, agent a on its own model ws[a]."""
    import dnn_mppi_mpc_amd as pkg
    e = pkg.Engine(K=K, n_agents=len(ws), **cfg)
    e.set_ref_path(REF)
    if obstacles:
        e.set_obstacles(OBSTACLES)
    for a, w in enumerate(ws):
        e.set_mlp(w, agent=a)
    e.set_state(x0)
    e.set_u_prev(u)
    return e


@pytest.mark.parametrize("waypoint_mode", ["frozen", "per_rollout"])
@pytest.mark.parametrize("H,n", [(512, 3), (128, 3), (64, 1), (256, 2)])
def test_batch_of_different_models_equals_separate_handles(H, n, waypoint_mode):
    """B = 5 agents with five models, 6 closed-loop iterations, obstacles some samples hit: every agent's nominal controls,
    state and costs equal those of a single-agent handle holding its model, bit for bit -- and differ from what the agent
    gets in a batch where everybody shares model 0."""
    B, K, T, n_it = 5, 300, 30, 6
    cfg = base_cfg(waypoint_mode, T)
    ws = [weights(H, n, 7 + H + n + a) for a in range(B)]
    x0, u = agent_inputs(B, T)
    batch = make_own(cfg, K, ws, x0, u)
    batch.run_closed_loop(n_it)
    assert batch.rollout_kernel() == batched_name(H, n)
    out = results(batch)
    assert out[0].shape == (B, T, 2) and out[1].shape == (B, 3) and out[2].shape == (B, K)
    assert batch.counters()["rollout_launches"] == n_it and batch.counters()["finalize_launches"] == n_it
    assert (out[2] >= 1e10).any() and (out[2] < 1e10).any()  # some samples collide, some do not
    for a in range(B):
        one = make(cfg, K, ws[a], x0[a], u[a], noise_stream=a)
        one.run_closed_loop(n_it)
        assert_agent_equals(out, a, one)
    shared = make(cfg, K, ws[0], x0, u, n_agents=B)
    shared.run_closed_loop(n_it)
    sh = results(shared)
    for got, ref in zip(out, sh):
        np.testing.assert_array_equal(got[0], ref[0])  # (agent 0 has model 0 in both)
    for a in range(1, B):  # a build that ignored the per-agent model would give these
        for got, ref in zip(out, sh):
            assert not np.array_equal(got[a], ref[a])


def test_mixed_models_and_back_to_the_shared_one():
    """Agents 1 and 3 on their own models beside 0, 2 and 4 on the shared one; then set_mlp without an agent returns the
    batch to one model (a fresh shared-model batch, bit for bit)."""
    B, K, T, n_it, H, n = 5, 300, 30, 6, 128, 3
    cfg = base_cfg("frozen", T)
    w = weights(H, n, 50)
    own = {1: weights(H, n, 51), 3: weights(H, n, 53)}
    x0, u = agent_inputs(B, T)
    batch = make(cfg, K, w, x0, u, n_agents=B)
    for a, wa in own.items():
        batch.set_mlp(wa, agent=a)
    batch.run_closed_loop(n_it)
    out = results(batch)
    for a in range(B):
        one = make(cfg, K, own.get(a, w), x0[a], u[a], noise_stream=a)
        one.run_closed_loop(n_it)
        assert_agent_equals(out, a, one)
    batch.set_mlp(w)
    batch.set_state(x0)
    batch.set_u_prev(u)
    batch.set_waypoint_idx(0)
    batch.set_iteration(0)  # (the sampler is keyed by the iteration counter)
    batch.run_closed_loop(n_it)
    fresh = make(cfg, K, w, x0, u, n_agents=B)
    fresh.run_closed_loop(n_it)
    for got, ref in zip(results(batch), results(fresh)):
        np.testing.assert_array_equal(got, ref)
    assert not np.array_equal(out[0][1], results(batch)[0][1])


@pytest.mark.parametrize("H,n", [(512, 3), (128, 3)])
def test_own_model_against_the_oracle(H, n):
    """Agent 2 of a batch of three models equals the f64 oracle holding ITS model on the injected noise of one iteration: S
    within 1e-3, u within 1e-4 RMSE (the bars of test_gpu_mlp_agents.py; another agent's model misses both)."""
    B, K, T, ag = 3, 512, 30, 2
    cfg = base_cfg("frozen", T, obstacles=False)
    ws = [weights(H, n, 31 + H + a) for a in range(B)]
    x0, u = agent_inputs(B, T)
    e = make_own(cfg, K, ws, x0, u, obstacles=False)
    eps = e.sample_epsilon(0)
    e.set_noise_ring(eps[None].contiguous())
    e.run_closed_loop(1)
    assert e.rollout_kernel() == batched_name(H, n)
    kw = dict(delta_t=0.1, ref_path=REF, max_speed=5.0, max_omega=3.14, num_samples_K=K, num_horizons_T=T,
              param_exploration=0.05, param_lambda=1.0, param_alpha=0.99, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              stage_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]), terminal_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=ws[ag])
    S_ref, _, u_ref = frozen_reference(o, x0[ag], u[ag], eps[ag].cpu().numpy(), K)
    S, un = e.costs()[ag], e.get_u_prev()[ag]
    print(f"{H} x {n}: max |S - S_ref| / (1e-3 + 1e-3 |S_ref|) = {np.max(np.abs(S - S_ref) / (1e-3 + 1e-3 * np.abs(S_ref))):.3g}, "
          f"u RMSE = {rmse(un, u_ref):.3g}")
    np.testing.assert_allclose(S, S_ref, rtol=1e-3, atol=1e-3)
    assert rmse(un, u_ref) <= 1e-4


def test_scalers_per_agent():
    """set_mlp(w, scalers=s_a, agent=a): the folded statistics are the agent's own (mppi_set_agent_mlp_scaled)."""
    B, K, T, n_it = 2, 300, 30, 4
    cfg = base_cfg("frozen", T)
    w = weights(128, 3, 60)
    sc = [dict(in_mean=np.array([4.39, -0.126, -0.08, 0.359, -0.031]), in_scale=np.array([5.59, 3.64, 1.06, 1.02, 1.84]),
               out_mean=np.array([-0.028, 0.0015, -0.00075]), out_scale=np.array([0.285, 0.18, 0.05])),
          dict(in_mean=np.array([1.0, 0.5, 0.1, 0.2, 0.0]), in_scale=np.array([2.0, 2.5, 0.8, 1.5, 1.2]),
               out_mean=np.array([0.01, -0.02, 0.005]), out_scale=np.array([0.1, 0.25, 0.08]))]
    x0, u = agent_inputs(B, T)
    batch = make(cfg, K, w, x0, u, n_agents=B)
    for a in range(B):
        batch.set_mlp(w, scalers=sc[a], agent=a)
    batch.run_closed_loop(n_it)
    out = results(batch)
    for a in range(B):
        one = make(cfg, K, w, x0[a], u[a], noise_stream=a)
        one.set_mlp(w, scalers=sc[a])
        one.run_closed_loop(n_it)
        assert_agent_equals(out, a, one)
    plain = make(cfg, K, w, x0, u, n_agents=B)
    plain.run_closed_loop(n_it)
    assert not np.array_equal(out[0][0], results(plain)[0][0]) and not np.array_equal(out[0][1], results(plain)[0][1])


def test_own_model_and_own_scene_together():
    """Agent 1 follows its own path (another length) with its own model beside two agents on the shared path and model."""
    import dnn_mppi_mpc_amd as pkg
    B, K, T, n_it, ag = 3, 300, 30, 5, 1
    cfg = base_cfg("frozen", T)
    w, w1 = weights(128, 3, 70), weights(128, 3, 71)
    path1 = mppi_oracle.generate_point_trajectory((-0.5, 0.5), (12.0, -4.0), 160)
    x0, u = agent_inputs(B, T)
    batch = make(cfg, K, w, x0, u, n_agents=B)
    batch.set_ref_path(path1, agent=ag)
    batch.set_mlp(w1, agent=ag)
    batch.run_closed_loop(n_it)
    out = results(batch)
    for a in range(B):
        one = pkg.Engine(K=K, noise_stream=a, **cfg)
        one.set_ref_path(path1 if a == ag else REF)
        one.set_obstacles(OBSTACLES)
        one.set_mlp(w1 if a == ag else w)
        one.set_state(x0[a])
        one.set_u_prev(u[a])
        one.run_closed_loop(n_it)
        assert_agent_equals(out, a, one)


def test_graph_replay_across_a_replaced_model(monkeypatch):
    """MPPI_GRAPH=1: 150 batched iterations, agent 1's model replaced, 150 more -- bit for bit the eagerly launched run (a
    replayed graph reads the model table afresh)."""
    B, K, T = 4, 256, 30
    cfg = base_cfg("frozen", T)
    ws = [weights(128, 3, 80 + a) for a in range(B)]
    w_new = weights(128, 3, 90)
    x0, u = agent_inputs(B, T)

    def run():
        e = make_own(cfg, K, ws, x0, u)
        out = []
        e.run_closed_loop(150)
        out.append(results(e))
        e.set_mlp(w_new, agent=1)
        e.run_closed_loop(150)
        out.append(results(e))
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
    # the replaced model took effect: the same run without the replacement ends elsewhere
    monkeypatch.delenv("MPPI_GRAPH")
    kept = make_own(cfg, K, ws, x0, u)
    kept.run_closed_loop(300)
    assert not np.array_equal(results(kept)[0][1], eager[1][0][1])


def test_refusals():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    B, K, T = 3, 256, 30
    cfg = base_cfg("frozen", T)
    w = weights(128, 3, 1)
    x0, u = agent_inputs(B, T)

    def refused(code, fn):
        with pytest.raises(pkg.MppiError) as ex:
            fn()
        assert ex.value.code == code, ex.value
        return str(ex.value)

    e = make(cfg, K, w, x0, u, n_agents=B)
    e.set_mlp(weights(128, 3, 2), agent=1)
    refused(capi.ERR_BAD_ARG, lambda: e.set_mlp(w, agent=-1))
    refused(capi.ERR_BAD_ARG, lambda: e.set_mlp(w, agent=B))
    msg = refused(capi.ERR_SHAPE, lambda: e.set_mlp(weights(64, 1, 3), agent=2))
    assert "64 x 1" in msg and "128 x 3" in msg
    w_big = weights(128, 3, 4)
    w_big["input_layer.weight"] = (w_big["input_layer.weight"] * 0 + 1e5).astype(np.float32)  # beyond the f16 range
    refused(capi.ERR_UNSUPPORTED, lambda: e.set_mlp(w_big, agent=1))
    e.run_closed_loop(4)
    same = make(cfg, K, w, x0, u, n_agents=B)  # the refused calls changed nothing: agent 1 kept its model
    same.set_mlp(weights(128, 3, 2), agent=1)
    same.run_closed_loop(4)
    for got, ref in zip(results(e), results(same)):
        np.testing.assert_array_equal(got, ref)

    fresh = pkg.Engine(K=K, n_agents=B, **cfg)  # only agent 0 has a model
    fresh.set_ref_path(REF)
    fresh.set_obstacles(OBSTACLES)
    fresh.set_mlp(w, agent=0)
    fresh.set_state(x0)
    assert "agent 1" in refused(capi.ERR_STATE, lambda: fresh.run_closed_loop(1))

    analytic = pkg.Engine(K=K, n_agents=B, **dict(cfg, model=capi.MODEL_DIFFDRIVE))
    refused(capi.ERR_STATE, lambda: analytic.set_mlp(w, agent=0))

    one = make(cfg, K, w, x0[0], u[0])  # a single-agent handle: agent = 0 is the plain setter
    one.run_closed_loop(3)
    two = make(cfg, K, weights(128, 3, 9), x0[0], u[0])
    two.set_mlp(w, agent=0)
    refused(capi.ERR_BAD_ARG, lambda: two.set_mlp(w, agent=1))
    two.run_closed_loop(3)
    assert two.rollout_kernel() == "k_rollout_mlp_w<128, false>"
    for got, ref in zip(results(two), results(one)):
        np.testing.assert_array_equal(got, ref)
