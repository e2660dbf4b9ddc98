"""GPU: the one-launch resolution of the sequential waypoint index (fused_lookback, k_rollout_dual<..., LB>) held to what it must
do, not only to results its fallback delivers as well.  The speculation rounds are exact too, so index, costs and controls
cannot tell a look-back that works from one that marks everything bad; `rounds` can.  tests/lookback_checks.py predicts from the
oracle's rollout whether an iteration must resolve in its one launch (rounds == 1) or must fall back (rounds > 1) and why, and
tests/test_lookback_cases.py checks the cases on the CPU.  Here: (a) inputs predicted good, several workgroups, offsets threaded
both ways; (b) each cause of the fallback alone; (c) one offending sample at the first, the last and a ragged workgroup; (d) a
look-back that times out (MPPI_LB_TIMEOUT_TICKS=0).  Tolerances: those of test_gpu_edges.py."""
import numpy as np
import pytest

import lookback_checks as lc

pytestmark = pytest.mark.gpu


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, float) - np.asarray(b, float)) ** 2)))


def run_case(case, precision="f64", f32_bits=False):
    """Runs the case's iterations on the device beside the oracle; asserts the kernel name where the look-back is in play and
    the oracle's index, costs and controls everywhere.  Returns [(rounds, prediction, in play)] per iteration."""
    import dnn_mppi_mpc_amd as pkg
    its = case.run_oracle(f32_bits=f32_bits)
    c = pkg.MPPIAlgorithms(**case.kw, precision=precision, variant=case.variant)
    c.u_prev[:] = case.u_in
    c.prev_way_point_idx = case.prev_idx
    c._calc_epsilon = lambda *a, **k: case.eps
    out = []
    for it, (x0, ref, pred, play) in enumerate(its):
        assert pred["gap"] >= lc.GAP_FLOOR, (case.name, it, pred["gap"])  # the device and NumPy cannot disagree on a descent bit
        u = c._calc_input_control(x0)[1]
        rounds = c.last_stats.rounds
        print(case.name, "iteration", it, "rounds", rounds, "predicted bad", pred["bad"], "largest offset", int(pred["m"].max()),
              c._engine.rollout_kernel())
        if play:
            assert c._engine.rollout_kernel().endswith(", true>"), c._engine.rollout_kernel()
        assert c.prev_way_point_idx == ref["idx_after"], (case.name, it)
        if precision == "f64":
            np.testing.assert_allclose(c.sample_costs(), ref["S"], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(u, ref["u_returned"], rtol=1e-7, atol=1e-9)
        else:
            np.testing.assert_allclose(c.sample_costs(), ref["S"], rtol=3e-4, atol=3e-4)
            assert rmse(u, ref["u_returned"]) <= 1e-4
        out.append((rounds, pred, play))
    return out


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("dual", ["0", "1"])
@pytest.mark.parametrize("K,T", lc.GOOD_KT)
def test_lookback_resolves_predicted_good_iterations_in_one_launch(monkeypatch, K, T, dual):
    """Arcs and a line, 53 / 129 / 200 samples over workgroups of 16 and of 32 with a ragged last one: workgroups that take their
    index from the words before them and workgroups that raise it (checked on the CPU).  rounds > 1 <=> predicted bad: a
    look-back that silently hands good iterations to the fallback fails here."""
    monkeypatch.setenv("MPPI_DUAL", dual)
    case = lc.good_case(K, T)
    res = run_case(case)
    assert all(play for _, _, play in res)
    for it, (rounds, pred, _) in enumerate(res):
        assert (rounds > 1) == pred["bad"], (case.name, it, rounds, pred["bad"])
    assert sum(rounds == 1 for rounds, _, _ in res) >= 2


# ------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("dual", ["0", "1"])
@pytest.mark.parametrize("cause", ["nonunimodal", "reach-numpy", "reach-cuda"])
def test_each_cause_of_the_fallback_alone(monkeypatch, cause, dual):
    monkeypatch.setenv("MPPI_DUAL", dual)
    case = lc.hairpin_case() if cause == "nonunimodal" else lc.reach_case(cause.split("-")[1])
    (rounds, pred, play), = run_case(case)
    assert play and pred["any_nonunimodal"] == (cause == "nonunimodal") and pred["reach"] == (cause == "nonunimodal")
    assert rounds > 1


# ------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("dual,K,k_star", lc.ONE_SAMPLE)
def test_one_offending_sample_hands_the_iteration_to_the_fallback(monkeypatch, dual, K, k_star):
    """All noise zero but sample k*'s: the first sample, the last one -- alone in a ragged last workgroup -- or one at a
    workgroup's edge.  A bad bit dropped from a partial workgroup, or a word beyond the finalize's scan, would pass as good."""
    monkeypatch.setenv("MPPI_DUAL", dual)
    (rounds, pred, play), = run_case(lc.one_sample_case(K, k_star))
    assert play and pred["reach"] and list(np.nonzero(pred["nonunimodal"])[0]) == [k_star]
    assert rounds > 1


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dual", ["0", "1"])
@pytest.mark.parametrize("K,T", lc.TIMEOUT_GOOD)
def test_a_lookback_that_times_out_falls_back(monkeypatch, K, T, dual, precision):
    """MPPI_LB_TIMEOUT_TICKS=0: every workgroup behind the first gives up before its first poll.  Inputs predicted good, so
    nothing else raises a bad bit: rounds > 1 is the timeout's doing, and the results stay exact."""
    monkeypatch.setenv("MPPI_DUAL", dual)
    monkeypatch.setenv("MPPI_LB_TIMEOUT_TICKS", "0")
    res = run_case(lc.good_case(K, T), precision, f32_bits=True)
    for rounds, pred, play in res:
        assert play and not pred["bad"] and pred["same_bits_f32"]
        assert rounds > 1


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dual", ["0", "1"])
def test_a_single_workgroup_never_waits(monkeypatch, dual, precision):
    """K = 16 / 32: one workgroup, nothing before it -- limit 0 changes nothing and the iteration resolves in its launch."""
    monkeypatch.setenv("MPPI_DUAL", dual)
    monkeypatch.setenv("MPPI_LB_TIMEOUT_TICKS", "0")
    res = run_case(lc.single_workgroup_case(dual), precision, f32_bits=True)
    for rounds, pred, play in res:
        assert play and not pred["bad"] and pred["same_bits_f32"]
        assert rounds == 1
