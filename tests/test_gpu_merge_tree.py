"""GPU: every branch of the merge tree between a rollout launch's softmin records and the update -- one window of 256
records, two windows, the 512 records the finalize kernel merges itself, the first 64:1 and the first 256:1 merge launch
in front of it -- and the same tree on the way down to a rank's one record of the split step.  The one-sample-per-wave
layout (`MPPI_DUAL=0`, T <= 64) leaves one record per 16 samples, so the record counts below follow from K alone."""
import numpy as np
import pytest

from oracle import c_oracle, mppi_oracle, philox

pytestmark = pytest.mark.gpu

T = 10
SAMPLES_PER_RECORD = 16


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, float) - np.asarray(b, float)) ** 2)))


@pytest.mark.parametrize("K,records", [(4096, 256), (4112, 257), (8192, 512), (8208, 513), (262160, 16385)])
def test_merge_tree_branches_of_one_handle_against_the_c_oracle(monkeypatch, K, records):
    """Diff-drive, frozen waypoint index, f64, injected noise, one iteration against the plain-C restatement of the
    reference loop (the f64 bars of the streaming-rollout test).  256 records: one window of the finalize kernel; 257: two
    windows; 512: the most it merges directly; 513: the first 64:1 merge launch in front of it; 16385: the first 256:1."""
    import torch

    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    monkeypatch.setenv("MPPI_DUAL", "0")
    assert (K + SAMPLES_PER_RECORD - 1) // SAMPLES_PER_RECORD == records
    kw = dict(delta_t=0.1, ref_path=mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100),
              max_speed=5.0, max_omega=3.14, num_samples_K=K, num_horizons_T=T, param_exploration=0.05,
              param_lambda=1.0, param_alpha=0.2, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              stage_cost_weight=np.array([5.0, 5.0, 10.0]), terminal_cost_weight=np.array([5.0, 5.0, 10.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    tt = np.arange(T)
    u_in = np.stack([1.0 + 0.3 * np.sin(0.2 * tt), 0.05 * np.cos(0.1 * tt)], axis=1)
    x0 = np.array([0.4, -0.1, -0.35])
    eps = philox.sample_epsilon(kw["sigma"], 77, 0, K, T)
    c = pkg.MPPIAlgorithms(**kw, precision="f64", waypoint_mode="frozen", seed=1)
    c.u_prev[:] = u_in
    c._calc_epsilon = lambda *a, **k: torch.from_numpy(eps).cuda()
    u0, u, _, _ = c._calc_input_control(x0)
    assert c._engine.counters()["rollout_layout"] == capi.LAYOUT_FUSED  # one sample per wave: 16 samples per record
    assert c._engine.rollout_kernel().startswith("k_rollout_fused<")
    o = c_oracle.DiffDriveC(**kw)
    o.u_prev[:] = u_in
    ref = o.iteration(x0, eps, frozen_threads=8)
    S = c.sample_costs()
    print(f"K={K} records={records}: max |S - ref| {np.max(np.abs(S - ref['S'])):.3e}  u RMSE {rmse(u, ref['u_returned']):.3e}")
    np.testing.assert_allclose(S, ref["S"], rtol=1e-9, atol=1e-9)
    assert rmse(u, ref["u_returned"]) <= 1e-8
    assert c.prev_way_point_idx == ref["idx_after"]


@pytest.mark.parametrize("shards", [(4096, 4112), (8208, 4096)])
def test_merge_tree_branches_of_the_split_step(monkeypatch, shards):
    """Two shards merged through the split-step ABI against the unsharded handle, one iteration (the configuration and
    tolerances of test_shard_invariance_two_shards_one_gpu, T = 10).  (4096, 4112): 256 and 257 records -- 256 go to the
    rank's record in one merge, 257 take a 64:1 merge first.  (8208, 4096): 513 records -- more than the finalize kernel
    would take, a 64:1 merge and then the rank's record.  The unsharded handles leave 513 and 769 records."""
    import torch

    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    monkeypatch.setenv("MPPI_DUAL", "0")
    lem = mppi_oracle.generate_lemniscate_racecar(100, 10.0)
    base = dict(model=capi.MODEL_RACECAR, T=T, delta_t=0.05, u_max=[0.523, 2.0], wheel_base=2.5,
                param_exploration=0.1, param_lambda=50.0, param_alpha=0.9, sigma=[0.5, 0.0, 0.0, 0.1],
                stage_cost_weight=[50.0, 50.0, 1.0, 20.0], terminal_cost_weight=[50.0, 50.0, 1.0, 20.0],
                beta_mode=capi.BETA_INV_LAMBDA, accumulate_stage_cost=1, waypoint_mode=capi.WAYPOINT_FROZEN,
                search_window=200, wrap_yaw_stage=1, wrap_yaw_terminal=1, clamp_rollout=1, clamp_u_after_update=1,
                filter_mode=capi.FILTER_RACECAR, filter_window=10, obstacle_model=capi.OBSTACLE_NONE,
                collision_penalty=1e10, seed=4242, precision=capi.PREC_F64)
    K = sum(shards)
    whole = pkg.Engine(K=K, **base)
    parts = [pkg.Engine(K=shards[0], K_global=K, k_offset=0, **base),
             pkg.Engine(K=shards[1], K_global=K, k_offset=shards[0], **base)]
    for e in [whole] + parts:
        e.set_ref_path(lem)
        assert e.counters()["rollout_layout"] == capi.LAYOUT_FUSED  # one sample per wave: 16 samples per record
    x0 = lem[2].astype(np.float64)
    n = whole.partial_len()
    u_ref, u0_ref, _ = whole.step(x0)
    gathered = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    for r, e in enumerate(parts):
        e.step_begin(x0, None, gathered[r * n:(r + 1) * n])
    outs = [e.step_end(gathered, 2) for e in parts]
    for u, u0, _ in outs:
        print(f"shards={shards}: max |u - whole| {np.max(np.abs(u - u_ref)):.3e}")
        np.testing.assert_allclose(u, u_ref, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(u0, u0_ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.concatenate([e.costs() for e in parts]), whole.costs(), rtol=1e-12)
