"""Learned dynamics with several agents per handle (mppi_config.n_agents > 1): one residual model shared by
every agent, agents as the second grid dimension of k_rollout_mlp_h3_agents / k_rollout_mlp_w_agents.  Checked against the
same problems in separate single-agent handles (noise_stream = the agent), against the f64 oracle, under graph replay, and
for the combinations that stay refused."""
import numpy as np
import pytest

from oracle import mppi_oracle
from test_gpu_mlp_shapes import frozen_reference, rmse, weights

pytestmark = pytest.mark.gpu

REF = mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100)
# one circle on the path, one beside it: with the nominal speed below some samples of every agent run into one of them
OBSTACLES = np.array([[1.0, -0.5, 0.35], [2.2, -0.6, 0.3]])


def base_cfg(waypoint_mode, T=30, obstacles=True):
    """The reference's diff-drive configuration (accumulate 0, frozen or per-rollout index), the learned model, f32.
    Cost weights scaled by 0.01 and param_alpha = 0.99: a softmin that is not one-hot (see test_gpu_mlp_shapes.kwargs)."""
    from dnn_mppi_mpc_amd import _capi as capi
    return dict(model=capi.MODEL_DIFFDRIVE_MLP, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                param_lambda=1.0, param_alpha=0.99, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[0.05, 0.05, 0.1, 0.0],
                terminal_cost_weight=[0.05, 0.05, 0.1, 0.0], beta_mode=capi.BETA_INV_EXPLORATION, accumulate_stage_cost=0,
                waypoint_mode={"frozen": capi.WAYPOINT_FROZEN, "per_rollout": capi.WAYPOINT_PER_ROLLOUT}[waypoint_mode],
                search_window=20, filter_mode=capi.FILTER_DIFFDRIVE, filter_window=10, clamp_rollout=1,
                obstacle_model=capi.OBSTACLE_CIRCLE if obstacles else capi.OBSTACLE_NONE, safety_margin=0.0,
                collision_penalty=1e10, seed=99, precision=capi.PREC_F32)


def agent_inputs(B, T):
    """Every agent its own x0 and nominal controls."""
    tt = np.arange(T)
    x0 = np.stack([[0.1 * a - 0.2, -0.05 * a + 0.1, 0.1 * a - 0.45] for a in range(B)])
    u = np.stack([np.stack([1.1 + 0.1 * a + 0.3 * np.sin(0.2 * tt + a), -0.1 + 0.05 * a + 0.05 * np.cos(0.1 * tt)], axis=1)
                  for a in range(B)])
    return x0, u


def make(cfg, K, w, x0, u, n_agents=1, noise_stream=0, obstacles=True):
    import dnn_mppi_mpc_amd as pkg
    e = pkg.Engine(K=K, n_agents=n_agents, noise_stream=noise_stream, **cfg)
    e.set_ref_path(REF)
    if obstacles:
        e.set_obstacles(OBSTACLES)
    e.set_mlp(w)
    e.set_state(x0)
    e.set_u_prev(u)
    return e


def batched_name(H, n):
    return "k_rollout_mlp_h3_agents<8, 2, 3>" if H == 512 and n in (2, 3) else f"k_rollout_mlp_w_agents<{H}>"


@pytest.mark.parametrize("waypoint_mode", ["frozen", "per_rollout"])
@pytest.mark.parametrize("H,n", [(512, 3), (128, 3), (64, 1), (256, 2)])
def test_batch_equals_separate_handles(H, n, waypoint_mode):
    """B = 5 agents, 6 closed-loop iterations, obstacles some samples hit: every agent's nominal controls, state and costs
    equal those of a single-agent handle with noise_stream = the agent bit for bit (the same arithmetic, other offsets)."""
    B, K, T, n_it = 5, 300, 30, 6
    cfg = base_cfg(waypoint_mode, T)
    w = weights(H, n, 7 + H + n)
    x0, u = agent_inputs(B, T)
    batch = make(cfg, K, w, x0, u, n_agents=B)
    batch.run_closed_loop(n_it)
    assert batch.rollout_kernel() == batched_name(H, n)
    ub, xb, Sb = batch.get_u_prev(), batch.get_state(), batch.costs()
    assert ub.shape == (B, T, 2) and xb.shape == (B, 3) and Sb.shape == (B, K)
    assert batch.counters()["rollout_launches"] == n_it and batch.counters()["finalize_launches"] == n_it
    assert (Sb >= 1e10).any() and (Sb < 1e10).any()  # some samples collide, some do not
    for a in range(B):
        one = make(cfg, K, w, x0[a], u[a], noise_stream=a)
        one.run_closed_loop(n_it)
        np.testing.assert_array_equal(ub[a], one.get_u_prev())
        np.testing.assert_array_equal(xb[a], one.get_state())
        np.testing.assert_array_equal(Sb[a], one.costs())
    for a in range(1, B):  # the agents are different problems
        assert not np.array_equal(ub[a], ub[0]) and not np.array_equal(xb[a], xb[0])


@pytest.mark.parametrize("H,n", [(512, 3), (128, 3)])
def test_noise_ring_equals_the_sampler_and_the_oracle(H, n):
    """A batched ring [slots, B, K, T, 2] filled by sample_epsilon reproduces the in-kernel Philox run (to the last-bit
    differences test_noise_ring_with_learned_dynamics allows the single agent), and one agent of the batch (a = 2) equals
    the f64 oracle on the injected noise of one iteration: u within 1e-4 RMSE, S within 1e-3."""
    import torch
    B, K, T = 3, 512, 30
    cfg = base_cfg("frozen", T, obstacles=False)
    w = weights(H, n, 31 + H)
    x0, u = agent_inputs(B, T)
    a_run, b_run = (make(cfg, K, w, x0, u, n_agents=B, obstacles=False) for _ in range(2))
    ring = torch.stack([b_run.sample_epsilon(i) for i in range(4)])
    assert tuple(ring.shape) == (4, B, K, T, 2)
    b_run.set_noise_ring(ring)
    a_run.run_closed_loop(4)
    b_run.run_closed_loop(4)
    assert b_run.rollout_kernel() == batched_name(H, n)
    np.testing.assert_allclose(b_run.get_u_prev(), a_run.get_u_prev(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(b_run.get_state(), a_run.get_state(), rtol=0, atol=1e-6)

    # the oracle anchor: one iteration from the injected noise, agent 2 of the batch
    e = make(cfg, K, w, x0, u, n_agents=B, obstacles=False)
    eps = e.sample_epsilon(0)
    e.set_noise_ring(eps[None].contiguous())
    e.run_closed_loop(1)
    ag = 2
    kw = dict(delta_t=0.1, ref_path=REF, max_speed=5.0, max_omega=3.14, num_samples_K=K, num_horizons_T=T,
              param_exploration=0.05, param_lambda=1.0, param_alpha=0.99, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              stage_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]), terminal_cost_weight=0.01 * np.array([5.0, 5.0, 10.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
    S_ref, _, u_ref = frozen_reference(o, x0[ag], u[ag], eps[ag].cpu().numpy(), K)
    np.testing.assert_allclose(e.costs()[ag], S_ref, rtol=1e-3, atol=1e-3)
    assert rmse(e.get_u_prev()[ag], u_ref) <= 1e-4


def test_graph_replay_equals_eager_launches(monkeypatch):
    """MPPI_GRAPH=1: 150 batched iterations, a model reloaded, 150 more -- bit for bit the eagerly launched run."""
    B, K, T = 4, 256, 30
    cfg = base_cfg("frozen", T)
    w1, w2 = weights(128, 3, 5), weights(128, 2, 6)
    x0, u = agent_inputs(B, T)

    def run():
        e = make(cfg, K, w1, x0, u, n_agents=B)
        out = []
        e.run_closed_loop(150)
        out.append((e.get_u_prev(), e.get_state(), e.costs()))
        e.set_mlp(w2)
        e.run_closed_loop(150)
        out.append((e.get_u_prev(), e.get_state(), e.costs()))
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
    assert not np.array_equal(eager[0][0][0], eager[0][0][1])


def test_refusals_and_single_agent_names(monkeypatch):
    """What stays refused with MPPI_ERR_UNSUPPORTED on a batched learned-dynamics handle, and the single-agent handles'
    kernel names, which bench.py and the profiles look launches up by."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    T = 30
    cfg = base_cfg("frozen", T)
    w = weights(128, 3, 1)

    def refused(fn):
        with pytest.raises(pkg.MppiError) as ex:
            fn()
        assert ex.value.code == capi.ERR_UNSUPPORTED, ex.value

    refused(lambda: pkg.Engine(K=256, n_agents=2, **dict(cfg, waypoint_mode=capi.WAYPOINT_SEQUENTIAL)))
    refused(lambda: pkg.Engine(K=40000, n_agents=2, **cfg))
    refused(lambda: pkg.Engine(K=256, K_global=512, n_agents=2, **cfg))
    pkg.Engine(K=32768, n_agents=2, **cfg).close()  # 512 workgroups per agent: the limit, admitted

    x0, u = agent_inputs(2, T)
    e = make(cfg, 256, w, x0, u, n_agents=2)
    e.run_closed_loop(1)
    refused(lambda: e.step(x0[0]))
    refused(lambda: e.rollout_viz())
    w_big = weights(512, 3, 2)
    w_big["input_layer.weight"] = (w_big["input_layer.weight"] * 1e5).astype(np.float32)  # beyond the f16 range
    refused(lambda: e.set_mlp(w_big))
    monkeypatch.setenv("MPPI_MLP_F32", "1")
    refused(lambda: e.set_mlp(weights(512, 3, 3)))
    monkeypatch.delenv("MPPI_MLP_F32")
    e.run_closed_loop(1)  # the handle still serves its model
    assert e.rollout_kernel() == "k_rollout_mlp_w_agents<128>"

    for (H, n), name in (((512, 3), "k_rollout_mlp_h3<false, 8, 2, 3>"), ((512, 2), "k_rollout_mlp_h3<false, 8, 2, 3>"),
                         ((128, 3), "k_rollout_mlp_w<128, false>"), ((64, 1), "k_rollout_mlp_w<64, false>")):
        one = make(cfg, 256, weights(H, n, 4), x0[0], u[0])
        one.run_closed_loop(1)
        assert one.rollout_kernel() == name
