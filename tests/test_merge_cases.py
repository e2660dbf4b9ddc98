"""The references and the inputs of the merge tests are what they claim to be -- checked on the CPU (tests/merge_checks.py), so
that a GPU test that passes has passed for the reason it names: merging group records is the softmin over all samples, every
record family meets the condition it states in both precisions, and the bounds behave like bounds."""
import math

import numpy as np
import pytest

import merge_checks as mc
from oracle import mppi_oracle

PRECISIONS = ("f32", "f64")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("K,per,T", [(1, 16, 3), (17, 16, 10), (100, 16, 33), (499, 32, 10), (1025, 16, 5), (4112, 16, 2)])
def test_merging_group_records_is_the_softmin_over_all_samples(precision, K, per, T):
    rng = np.random.default_rng([K, per, T])
    beta = 0.7
    S = 100.0 + rng.gamma(2.0, 8.0, K)
    S[rng.integers(0, K)] -= 30.0  # one clear minimum somewhere
    eps = rng.normal(size=(K, T, 2)).astype(np.float32)
    groups, whole = mc.records_from_samples(S, eps, beta, mc.even_bounds(K, per), precision)
    assert groups[0].shape == ((K + per - 1) // per,)
    # (the group records are intermediate values in f64: merged as such, whatever the handle's precision)
    rho, eta, eta2, w = mc.merge(*groups, float(mc.rounded(beta, precision)), "f64")
    assert rho == whole[0] == mc.rounded(S, precision).min()
    assert abs(eta - whole[1]) <= 1e-12 * whole[1] and abs(eta2 - whole[2]) <= 1e-12 * whole[2]
    want = whole[3] / whole[1]
    assert np.max(np.abs(w - want)) <= 1e-12 * np.max(np.abs(want))
    # and both are the plain softmin weights applied to the noise
    Sr, b = mc.rounded(S, precision), float(mc.rounded(beta, precision))
    wk = np.exp(-b * (Sr - Sr.min()))
    np.testing.assert_allclose(want, np.einsum("k,ki->i", wk / wk.sum(), eps.reshape(K, -1).astype(np.float64)),
                               rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T", mc.ABI_T)
def test_abi_case_tables_meet_their_conditions(precision, T):
    cases = mc.abi_cases(T)
    for c in cases:
        mc.check_case(c, precision)
    assert {c["n"] for c in cases} == set(mc.ABI_NRANKS) and {c["family"] for c in cases} == set(mc.FAMILIES)
    at = {(c["n"], c["pos"]) for c in cases if c["family"] == "dominant"}
    assert {(256, 0), (256, 63), (256, 64), (256, 255), (65, 64), (64, 63), (1, 0)} <= at
    assert len({c["name"] for c in cases}) == len(cases)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nwin", [1, 2])
def test_window_case_tables_meet_their_conditions(precision, nwin):
    for T in mc.WINDOW_T:
        cases = mc.window_cases(T, nwin)
        for c in cases:
            mc.check_case(c, precision)
            assert c["n"] <= nwin * mc.MERGE_MAX_RECORDS
        lone = {c["pos"] for c in cases if c["family"] == "lone_min"}
        assert {32 * g for g in range(8)} <= lone  # the minimum alone in each of the eight 32-record groups
        assert nwin == 1 or {256, 288, 511} <= lone  # and in the second window
        assert set(mc.WINDOW_N[nwin]) <= {c["n"] for c in cases}


def test_collided_records_need_the_exact_difference():
    """At 1e10 T one f32 spacing is worth a quarter of a unit of beta (rho_b - rho): the scales are exp(-k / 4) for whole k, so a
    merge that lost one spacing anywhere (a difference formed from rounded halves, say) is off by 22 percent of that scale."""
    for T in mc.ABI_T + (1,):
        c = mc.make_case("collided", 64, T)
        assert mc.collided_spacing(T) >= 1024.0 and c["beta"] * mc.collided_spacing(T) == mc.COLLIDED_STEP_ARG
        for p in ("f32", "f64"):
            _, s = mc.scales(c["rho"], c["beta"], p)
            k = np.round(-4.0 * np.log(s))
            assert len(set(k)) >= 5 and np.max(np.abs(s - np.exp(-k / 4.0))) < 1e-12
            _, s1 = mc.scales(c["rho"] + mc.collided_spacing(T) * (np.arange(64) == int(np.argmax(k))), c["beta"], p)
            assert abs(s1[int(np.argmax(k))] / s[int(np.argmax(k))] - math.exp(-0.25)) < 1e-12


@pytest.mark.parametrize("mode", sorted(mc.FILTER_MODES))
@pytest.mark.parametrize("window", [1, 2, 3, 10, 11])
def test_finish_and_its_bound(mode, window):
    """finish() is the oracle's filter, update, clamp and shift; bound_u is linear, non-negative and covers an f32 evaluation
    of the same sums."""
    m = mc.FILTER_MODES[mode]
    T = 2 * window + 3
    rng = np.random.default_rng([m, window])
    w = rng.normal(size=(T, 2))
    u_prev = mc.u_prev_signal(T)
    fin = mc.finish(w.reshape(-1), u_prev, m, window, False, [0.5, 0.05])
    np.testing.assert_array_equal(fin["u"][:-1], fin["u_updated"][1:])
    np.testing.assert_array_equal(fin["u"][-1], fin["u_updated"][-1])
    np.testing.assert_array_equal(fin["u0"], fin["u_updated"][1])
    cl = mc.finish(w.reshape(-1), u_prev, m, window, True, [0.5, 0.05])
    assert (np.abs(cl["u_updated"]) <= [0.5, 0.05]).all() and (np.abs(fin["u_updated"]) > [0.5, 0.05]).any()
    bw = 1e-6 * np.abs(rng.normal(size=2 * T))
    b = mc.bound_u(bw, w, u_prev, m, window, "f32")
    assert (b > 0).all()
    # a perturbation of w_eps within bound_w moves u by less than the bound
    moved = mc.finish(w.reshape(-1) + bw * rng.choice([-1.0, 1.0], 2 * T), u_prev, m, window, False, [0.5, 0.05])
    assert (np.abs(moved["u_updated"] - fin["u_updated"]) <= b).all()
    if m == mc.FILTER_RACECAR:  # the f32 filter of the oracle against the f64 one
        f32 = mppi_oracle.moving_average_racecar(w.astype(np.float32), window)
        b0 = mc.bound_u(np.zeros(2 * T), w, np.zeros((T, 2)), m, window, "f32")
        assert (np.abs(f32 - mc.moving_average(w.astype(np.float32).astype(np.float64), m, window)) <= b0).all()


def test_bound_scales_with_the_terms():
    c = mc.make_case("benign", 64, 10)
    b32, b64 = (mc.bound(c["rho"], c["eta"], c["eta2"], c["W"], c["beta"], p) for p in PRECISIONS)
    assert (b32["w_eps"] > 0).all() and b32["eta"] > 0
    np.testing.assert_allclose(b32["w_eps"] / b64["w_eps"], 2.0 ** 29, rtol=1e-5)
    bk = mc.bound(c["rho"], c["eta"], c["eta2"], c["W"], c["beta"], "f64", n=4096)
    np.testing.assert_allclose(bk["w_eps"] / b64["w_eps"], (4096 + 24) / (64 + 24), rtol=1e-12)
    assert mc.ratio([1.0, 2.0], [1.0, 2.5], [0.0, 1.0]) == 0.5 and math.isinf(mc.ratio([1.0], [1.1], [0.0]))
