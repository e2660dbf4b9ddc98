"""The inputs of tests/test_gpu_lookback.py are what they claim to be -- checked on the CPU, from the oracle and the NumPy
restatement of the kernels' conditions (tests/lookback_checks.py), so that a GPU test that passes has passed for the reason it
names: which iterations the look-back serves, whether it must succeed and why not, which workgroups decide by their own offset
and which by the offsets before them, and how far every comparison is from a tie.  Also the CPU side of the lb_scan unit tests:
the share of real-valued calls left out of the bitwise comparison."""
import numpy as np
import pytest

import lookback_checks as lc
import prims_checks as pc


@pytest.mark.parametrize("dtype", [pc.F32, pc.F64], ids=["f32", "f64"])
def test_lb_scan_real_data_leaves_out_at_most_2_percent(dtype):
    _, _, m, bad, compared = pc.lb_real_reference(dtype)
    assert 1.0 - compared.mean() <= pc.LB_LEFT_OUT_MAX
    assert len(np.unique(m)) == 32  # every candidate is some call's first minimum


def test_lb_scan_lattice_covers_the_edges_the_issue_names():
    pos = pc.lb_lattice_positions()
    seen = set()
    for name, row in pc.lb_lattice_rows().items():
        m, bad, g, gap = pc.lb_scan_reference(row.astype(pc.F32), pos.astype(pc.F32))
        m64, bad64, _, _ = pc.lb_scan_reference(row, pos)
        assert np.array_equal(m, m64) and np.array_equal(bad, bad64), name  # exact in float: the same bits from either width
        rest = g[:, 1:]
        found = {"tie": (gap == 0).any(), "bad": bad.any(), "idle": (m == -1).any(),
                 "first only": (g[:, 0] & ~rest.any(axis=1)).any(), "all 32": g.all(axis=1).any(),
                 "last only": (g[:, 0] & g[:, 31] & ~g[:, 1:31].any(axis=1)).any()}
        seen |= {k for k, v in found.items() if v}
        if "_nc" in name:
            nc = int(name.split("_nc")[1])
            assert not g[:, nc:].any(), name  # an absent candidate never descends
            assert (m[np.isfinite(pos[:, 0])] <= nc - 1).all()
    on_candidate = (pos[:, None, :] == pc.lb_lattice_rows()["line"][None, :, :]).all(axis=2).any()
    assert on_candidate and seen == {"tie", "bad", "idle", "first only", "all 32", "last only"}, seen


def test_lb_reach_formula_equals_the_brute_force_statement():
    table, want = pc.lb_reach_table()
    formula = np.array([leave < W and (leave + W <= pc.LB_CAND or n_ref - c <= pc.LB_CAND) for leave, W, n_ref, c in table])
    assert np.array_equal(formula, want)


# ------------------------------------------------------------------------------------------ end-to-end cases
def _all_in_play_and_clear_of_ties(its, floor=lc.GAP_FLOOR):
    for _, _, pred, play in its:
        assert play
        assert pred["gap"] >= floor, pred["gap"]


@pytest.mark.parametrize("K,T", lc.GOOD_KT)
def test_good_cases_are_predicted_good_and_thread_the_offset_both_ways(K, T):
    case = lc.good_case(K, T)
    its = case.run_oracle()
    _all_in_play_and_clear_of_ties(its)
    assert sum(not pred["bad"] for _, _, pred, _ in its) >= 2
    first = its[0][2]
    assert not first["bad"] and first["m"].max() >= 3
    for per_wg in lc.WG_SAMPLES.values():
        e_decides, own_decides = lc.e_decides_and_own_decides(first["m"], per_wg)
        if -(-K // per_wg) >= 3:
            assert e_decides and own_decides, (per_wg, lc.workgroup_maxima(first["m"], per_wg))
        else:  # two workgroups: the second one is the one or the other (both occur: the test below)
            assert e_decides or own_decides


def test_two_workgroup_cases_cover_both_ways():
    kinds = {lc.e_decides_and_own_decides(lc.good_case(53, T).run_oracle()[0][2]["m"], 32) for T in (10, 33, 64)}
    assert kinds == {(True, False), (False, True)}, kinds


def test_variants_and_paths_are_spread_over_the_good_cases():
    names = [lc.good_case(K, T).name for K, T in lc.GOOD_KT]
    for variant in ("numpy", "cuda"):
        mine = [n for n in names if f"-{variant}-" in n]
        assert {n.split("-T")[1] for n in mine} == {"10", "33", "64"}, mine
        assert len({n.split("-")[0] for n in mine}) == 3, mine


def test_hairpin_case_is_bad_for_non_unimodal_calls_alone():
    its = lc.hairpin_case().run_oracle()
    _all_in_play_and_clear_of_ties(its)
    assert its[0][2]["any_nonunimodal"] and its[0][2]["reach"]


@pytest.mark.parametrize("variant", ["numpy", "cuda"])
def test_reach_case_is_bad_for_the_reach_alone(variant):
    its = lc.reach_case(variant).run_oracle()
    _all_in_play_and_clear_of_ties(its)
    assert not its[0][2]["any_nonunimodal"] and not its[0][2]["reach"]


@pytest.mark.parametrize("dual,K,k_star", lc.ONE_SAMPLE)
def test_one_sample_cases_have_exactly_one_offending_sample(dual, K, k_star):
    its = lc.one_sample_case(K, k_star).run_oracle()
    _all_in_play_and_clear_of_ties(its)
    pred = its[0][2]
    assert np.array_equal(np.nonzero(pred["nonunimodal"])[0], [k_star]) and pred["reach"]
    per_wg = lc.WG_SAMPLES[dual]
    assert K % per_wg == 1  # a ragged last workgroup of one sample
    assert k_star in (0, K - 1) or k_star % 16 in (0, 15)


@pytest.mark.parametrize("K,T", lc.TIMEOUT_GOOD)
def test_timeout_cases_have_the_same_descent_bits_in_float(K, T):
    its = lc.good_case(K, T).run_oracle(f32_bits=True)
    _all_in_play_and_clear_of_ties(its)
    assert -(-K // 32) >= 2
    for _, _, pred, _ in its:
        assert not pred["bad"] and pred["same_bits_f32"] and pred["gap_f32"] >= lc.GAP_FLOOR_F32, pred["gap_f32"]


@pytest.mark.parametrize("dual", ["0", "1"])
def test_single_workgroup_case_is_predicted_good_in_both_widths(dual):
    its = lc.single_workgroup_case(dual).run_oracle(f32_bits=True)
    _all_in_play_and_clear_of_ties(its)
    for _, _, pred, _ in its:
        assert not pred["bad"] and pred["same_bits_f32"] and pred["gap_f32"] >= lc.GAP_FLOOR_F32
