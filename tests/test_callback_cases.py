"""The references and the inputs of the callback-controller tests are what they claim to be -- checked on the CPU
(tests/callback_checks.py), so that a GPU test that passes has passed for the reason it names: the f64 reference and the f32
restatement agree within the distance that is reported, the restated sampler draws N(0, Sigma), every case keeps enough
samples away from the inverse cost's step and enough of them near an obstacle, the spread cases do spread, and the factor
and the inverse the tables expect are the ones plain numpy.linalg gives."""
import math

import numpy as np
import pytest

import callback_checks as cc
from oracle import mppi_cb_oracle as cbo
from oracle import philox


@pytest.mark.parametrize("name", list(cc.cases()))
def test_command_cases_meet_their_conditions(name):
    cc.check_case(name)
    c = cc.cases()[name]
    ref, o, dist = cc.reference(name)
    kept = int(ref["keep"].sum())
    print(f"{name}: K {c['K']} T {c['T']} lambda {c['lam']:.6g} left out {c['K'] - kept} active "
          f"{int((ref['active'] & ref['keep']).sum())} ESS {cc.ess(ref['omega']):.1f} restatement distance {dist:.3g}")
    assert abs(math.fsum(ref["omega"]) - 1.0) < 1e-12
    np.testing.assert_array_equal(ref["action"], ref["U_new"][0])


def test_the_case_table_covers_what_it_must():
    cs = cc.cases().values()
    shapes = {(c["dyn"], c["K"], c["T"]) for c in cs if c["family"] == "clamp"}
    assert {("unicycle", 1, 25), ("unicycle", 255, 1), ("unicycle", 256, 25), ("unicycle", 257, 128), ("skid_steer", 1, 64),
            ("skid_steer", 257, 64), ("skid_steer", 256, 7)} <= shapes
    assert any(c["T"] * cc.NU[c["dyn"]] == 256 for c in cs)
    assert {c["null"] for c in cs} == {False, True}
    assert any(not c["bounded"] for c in cs if c["family"] == "clamp")
    assert any(c["dyn"] == "skid_steer" and c["cost"]["kind"] == "exponential" for c in cs)
    assert any(c["u_init"].any() for c in cs)
    assert sum(c["family"] == "spread" for c in cs) >= 4 and any(c["family"] == "clamp" and c["K"] > 1 for c in cs)
    for c in cs:
        assert np.count_nonzero(c["sigma"]) == c["sigma"].size and cc.is_symmetric(c["sigma"])
    rho = cc.SIGMA2[0, 1] / math.sqrt(cc.SIGMA2[0, 0] * cc.SIGMA2[1, 1])
    assert 0.45 < rho < 0.55


def test_a_start_on_a_safety_boundary_is_the_counter_example():
    """The unicycle from (4.3, 3.5): d = 0.8 from the obstacle at (3.5, 3.5), every sample is left out."""
    c = dict(cc.cases()["spread-uni-inv-K256-T25"])
    ref = cc.command(c, (4.3, 3.5, 0.9), c["U"], c["noise"])
    assert (~ref["keep"]).sum() > cc.EXCLUDED_CAP * c["K"]


@pytest.mark.parametrize("dyn", ["unicycle", "skid_steer"])
def test_models_in_f64_agree_with_the_restatement(dyn):
    rng = np.random.default_rng(5)
    n, nx, nu = 300, cc.NX[dyn], cc.NU[dyn]
    s = rng.normal(0, 3, (n, nx)).astype(np.float32)
    a = rng.normal(0, 1.5, (n, nu)).astype(np.float32)
    got, bound = cc.dynamics(dyn, s, a, cc.DT[dyn])
    want = {"unicycle": cbo.unicycle, "skid_steer": cbo.skid_steer}[dyn](s, a, dt=cc.DT[dyn])
    assert cc.ratio(want, got, bound) <= 1.0  # the f32 restatement is itself inside the bound the device is held to
    for cost_name in [p[1] for p in cc.MODEL_PAIRS if p[0] == dyn]:
        cost = cc._cost(cost_name)
        for t in (0, 24):
            c, b, _ = cc.running_cost(s, a, t, cost)
            w = cbo.running_cost(s, a, t, goal=cost["goal"], q_diag=cost["q"], r_diag=cost["r"], obstacles=cost["obstacles"],
                                 safety=cost["safety"], weight=cost["weight"], kind=cost["kind"])
            assert cc.ratio(w, c, b) <= 1.0, (cost_name, t)


@pytest.mark.parametrize("dyn,cost_name", cc.MODEL_PAIRS)
def test_model_rows_are_what_they_claim(dyn, cost_name):
    for n in cc.MODEL_N:
        for n_obs in cc.MODEL_N_OBS:
            for t in (0, cc.MODEL_T - 1):
                s, a, cost = cc.check_model_rows(dyn, cost_name, n, n_obs, t)
                assert s.shape == (n, cc.NX[dyn]) and a.shape == (n, cc.NU[dyn]) and cost["obstacles"].shape == (n_obs, 4)
                # and the f32 restatement of the cost stays inside the bound on them
                c, b, _ = cc.running_cost(s, a, t, cost)
                w = cbo.running_cost(s, a, t, goal=cost["goal"], q_diag=cost["q"], r_diag=cost["r"],
                                     obstacles=cost["obstacles"], safety=cost["safety"], weight=cost["weight"], kind=cost["kind"])
                assert cc.ratio(w, c, b) <= 1.0, (n, n_obs, t)


@pytest.mark.parametrize("sigma", [cc.SIGMA2, cc.SIGMA4, np.eye(4), np.diag([0.5, 0.3])], ids=["2x2", "4x4", "I4", "diag2"])
def test_factor_and_inverse_agree_with_the_host_recurrences(sigma):
    nu = sigma.shape[0]
    L, Li, Sinv = cc.host_factor(sigma)
    wantL, wantS = np.linalg.cholesky(sigma), np.linalg.inv(sigma)
    np.testing.assert_allclose(L[:nu, :nu], wantL, rtol=0, atol=1e-14)
    np.testing.assert_allclose(Li[:nu, :nu], np.linalg.inv(wantL), rtol=0, atol=1e-13)
    np.testing.assert_allclose(Sinv[:nu, :nu], wantS, rtol=0, atol=1e-13)
    assert not L[nu:].any() and not L[:, nu:].any() and not Sinv[nu:].any() and not Sinv[:, nu:].any()
    fL, fS = cc.factor(sigma)  # what the tables use: the same, rounded to f32
    np.testing.assert_array_equal(fL, cc.rounded(L[:nu, :nu]))
    np.testing.assert_allclose(fS, Sinv[:nu, :nu], rtol=0, atol=2 * cc.EPS * np.abs(wantS).max())
    np.testing.assert_allclose(fL @ fL.T, sigma, atol=1e-6)
    if np.count_nonzero(sigma) == sigma.size:
        assert np.count_nonzero(np.tril(wantL)) == nu * (nu + 1) // 2  # a transposed factor cannot look the same


def test_the_host_recurrences_read_one_triangle_and_the_symmetry_test_sees_the_other():
    bad = cc.SIGMA4.copy()
    bad[0, 3] += 1e-3
    np.testing.assert_array_equal(cc.host_factor(bad)[0], cc.host_factor(cc.SIGMA4)[0])
    assert not cc.is_symmetric(bad) and cc.is_symmetric(cc.SIGMA4) and cc.is_symmetric(cc.SIGMA4 * (1 + 1e-12 * np.eye(4)))
    with pytest.raises(ValueError):
        cc.host_factor(np.array([[1.0, 2.0], [2.0, 1.0]]))


@pytest.mark.parametrize("sigma", [cc.SIGMA2, cc.SIGMA4], ids=["2x2", "4x4"])
def test_restated_sampler_has_mean_zero_and_the_covariance(sigma):
    K, T, nu = 1000, 64, sigma.shape[0]
    n = cc.cb_noise(sigma, 0x1234567890ABCDEF, 3, K, T).reshape(-1, nu)
    N = n.shape[0]
    sd = np.sqrt(np.diag(sigma))
    assert (np.abs(n.mean(0)) < 5.0 * sd / math.sqrt(N)).all()  # five standard errors
    # Var(sample covariance_ij) = (S_ii S_jj + S_ij^2) / N for a normal draw
    se = np.sqrt((np.outer(np.diag(sigma), np.diag(sigma)) + sigma ** 2) / N)
    assert (np.abs(np.cov(n.T) - sigma) < 5.0 * se).all()
    z = cc.cb_normals(0x1234567890ABCDEF, 3, K, T).reshape(-1, 4)
    assert (np.abs(np.cov(z.T) - np.eye(4)) < 5.0 * np.sqrt((1 + np.eye(4)) / N)).all()  # the four normals are independent
    assert np.abs(z).max() < 7.0  # |1 + n| < 8 for Sigma = I: the probe's rounding term holds


def test_restated_sampler_is_keyed_as_the_kernel_says():
    """Counter (k, t, iteration, 0x6362), key = the seed's halves; one element by hand."""
    seed, it, k, t = 0xABCDEF0123456789, 5, 7, 2
    r = philox.philox4x32_10(np.uint32(k), np.uint32(t), np.uint32(it), np.uint32(0x6362), seed & 0xFFFFFFFF, seed >> 32)
    u = [float(philox.uniform_open(x)) for x in r]
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    z = cc.cb_normals(seed, it, 8, 3)
    np.testing.assert_allclose(z[k, t], want, rtol=1e-13)
    assert not np.array_equal(z, cc.cb_normals(seed, it + 1, 8, 3)) and not np.array_equal(z, cc.cb_normals(seed + 1, it, 8, 3))
    val, tol = cc.probe_value(cc.SIGMA4, seed, it, 8, 3, t, 1)
    LiT = np.linalg.inv(np.linalg.cholesky(cc.SIGMA4)).T
    np.testing.assert_allclose(val, z[:, t] @ LiT[1], rtol=0, atol=1e-6)  # (Sigma^-1 L z)_i = (L^-T z)_i up to the f32 casts
    assert tol == pytest.approx((4e-6 + 2.0 ** -21) * np.abs(LiT[1]).sum())


def test_error_models_behave_like_bounds():
    rng = np.random.default_rng(3)
    K = 257
    c = 1000.0 + rng.gamma(2.0, 50.0, K)
    lam = cc._r(np.std(c))
    omega, x = cc.softmin(c, lam)
    # an f32 evaluation in another order stays inside the omega model
    c32 = c.astype(np.float32)
    e32 = np.exp(-(c32 - c32.min()) / np.float32(lam)).astype(np.float32)
    w32 = e32 / e32[::-1].sum(dtype=np.float32)
    w64, x64 = cc.softmin(c32.astype(np.float64), lam)
    assert cc.ratio(w32, w64, cc.bound_omega(w64, x64, K)) <= 1.0
    noise = rng.normal(size=(K, 5, 2)).astype(np.float32).astype(np.float64)
    U = rng.normal(size=(5, 2)).astype(np.float32).astype(np.float64)
    new, bound = cc.update(U, w64, noise)
    got = U.astype(np.float32) + np.einsum("k,kti->ti", w64.astype(np.float32), noise.astype(np.float32), dtype=np.float32)
    assert 0 < cc.ratio(got, new, bound) <= 1.0
    assert cc.ratio(new + 3 * bound, new, bound) > 1.0 and cc.ratio([1.0], [1.0 + 1e-9], [0.0]) == math.inf


def test_cost_factor_follows_from_the_measured_ratios():
    """COST_FACTOR is the smallest power of two that is at least twice the largest measured cost_total ratio
    (profiles/callback_measured.json, written by tools/callback_report.py on the MI355X), and no ratio is a finding."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "callback_measured.json")
    with open(path) as fh:
        rep = json.load(fh)
    ratios = rep["ratios"]["cost_total"]
    assert set(cc.cases()) <= set(ratios)
    largest = max(ratios.values())
    assert largest <= cc.COST_RATIO_FINDING
    f = 1
    while f < 2.0 * largest:
        f *= 2
    assert cc.COST_FACTOR == f, (largest, f)
    for kind in ("omega", "U", "sampler", "models.dynamics", "models.cost"):
        assert 0 <= max(rep["ratios"][kind].values()) <= 1.0, kind
