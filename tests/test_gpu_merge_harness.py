"""GPU: the rescale merge of csrc/mppi_merge.h on records of our own making, in the product's instantiations --
merge_combine<A, 256, 1 / 2> (k_merge, k_finalize) and merge_abi<A> -- through the test-only harness
(tests/device/prims_harness.hip), which allocates the record buffers as the product does.  References, bounds and the case
tables: tests/merge_checks.py (the tables' own conditions are checked on the CPU, tests/test_merge_cases.py).  No tolerance is
chosen here: every figure is held to the error model of merge_checks, rho and the collision count exactly."""
import numpy as np
import pytest

import merge_checks as mc
import prims_checks as pc
from prims_checks import F32, F64

pytestmark = pytest.mark.gpu

FP = [pytest.param(F32, "f32", id="f32"), pytest.param(F64, "f64", id="f64")]


@pytest.fixture(scope="module")
def P():
    import dnn_mppi_mpc_amd as pkg
    return pc.Prims(pkg.build.prims_library())


def held(case, precision, got, n_hit_want=None):
    """Ratios error / bound of one merge result (rho, eta, eta2, n_hit or None, w_eps) against merge_checks; asserts the exact
    parts.  Returns {"w_eps", "eta", "eta2"}."""
    rho, eta, eta2, n_hit, w = got
    r_rho, r_eta, r_eta2, r_w = mc.merge(case["rho"], case["eta"], case["eta2"], case["W"], case["beta"], precision)
    b = mc.bound(case["rho"], case["eta"], case["eta2"], case["W"], case["beta"], precision)
    assert float(rho) == r_rho, (case["name"], float(rho), r_rho)  # the minimum of the rounded inputs, exactly
    if n_hit_want is not None:
        assert float(n_hit) == n_hit_want, (case["name"], float(n_hit), n_hit_want)
    out = {"w_eps": mc.ratio(w, r_w, b["w_eps"]), "eta": mc.ratio(eta, r_eta, b["eta"]), "eta2": mc.ratio(eta2, r_eta2, b["eta2"])}
    if case["family"] == "dominant":  # the single-record answer W_b / eta_b within a few ulp (s = 1, every other scale 0)
        p = case["pos"]
        one = mc.rounded(case["W"][p], precision) / mc.rounded(case["eta"][p], precision)
        assert np.all(np.abs(w - one) <= 6 * mc.EPS[precision] * np.abs(one)), case["name"]
        assert float(eta) == float(mc.rounded(case["eta"][p], precision)), case["name"]
    if case["family"] == "ties":
        assert abs(float(eta) - r_eta) <= b["eta"], case["name"]
    return out


def run_cases(P, dtype, precision, nwin, T):
    worst, over = {}, []
    for case in mc.window_cases(T, nwin):
        n = case["n"]
        hits = np.random.default_rng([n, T]).integers(0, 17, n).astype(np.float64)
        got = P.merge_combine(dtype, nwin, case["rho"], case["eta"], case["eta2"], hits, case["W"], n, case["beta"])
        r = held(case, precision, got, n_hit_want=float(hits.sum()))
        for k, v in r.items():
            worst[(case["family"], k)] = max(worst.get((case["family"], k), 0.0), v)
            if not v <= 1.0:
                over.append((case["name"], k, v))
    return worst, over


@pytest.mark.parametrize("T", mc.WINDOW_T)
@pytest.mark.parametrize("nwin", [1, 2])
@pytest.mark.parametrize("dtype,precision", FP)
def test_merge_combine_families_within_the_error_model(P, dtype, precision, nwin, T):
    """Every family of merge_checks.window_cases -- benign, ties, one dominant record (at 0, 63, 64, n - 1 and the first slot of
    the second window), collided magnitudes, sign-cancelling W, the minimum alone in each 32-record group -- at n next to
    32 / 64 / 256 / 512; n_hit counts of 0 .. 16 per record sum exactly."""
    worst, over = run_cases(P, dtype, precision, nwin, T)
    print(f"merge_combine<{precision}, 256, {nwin}> T={T}: max error / bound",
          {f"{f}.{k}": round(v, 4) for (f, k), v in sorted(worst.items())})
    assert not over, over[:10]


@pytest.mark.parametrize("dtype,precision", FP)
def test_merge_combine_leaves_the_count_out_when_asked(P, dtype, precision):
    case = mc.make_case("benign", 65, 10)
    hits = np.full(65, 3.0)
    with_hits = P.merge_combine(dtype, 1, case["rho"], case["eta"], case["eta2"], hits, case["W"], 65, case["beta"])
    without = P.merge_combine(dtype, 1, case["rho"], case["eta"], case["eta2"], hits, case["W"], 65, case["beta"], want_hits=False)
    assert float(with_hits[3]) == 195.0 and float(without[3]) == -1.0
    assert with_hits[0] == without[0] and with_hits[1] == without[1] and np.array_equal(with_hits[4], without[4])


@pytest.mark.parametrize("nwin,ns", [(1, mc.WINDOW_N[1]), (2, mc.WINDOW_N[2])])
@pytest.mark.parametrize("dtype,precision", FP)
def test_absent_slots_with_finite_garbage_change_nothing(P, dtype, precision, nwin, ns):
    """Slots >= n hold finite garbage -- heads below the true minimum, huge W, counts, the pad words -- up to the end of the
    buffer: bit for bit the result of zero-filled ones.  (NaN there is outside the stated contract of mppi_merge.h.)"""
    cap = nwin * 256 + 256
    for T in (10, 65):
        for n in ns:
            case = mc.make_case("benign", n, T)
            hits = np.arange(n, dtype=np.float64) % 17
            clean = P.merge_combine(dtype, nwin, case["rho"], case["eta"], case["eta2"], hits, case["W"], n, case["beta"])
            rng = np.random.default_rng([n, T, 5])
            g = cap - n
            fill = lambda a, junk: np.concatenate([a, junk], axis=0)
            dirty = P.merge_combine(dtype, nwin, fill(case["rho"], -1e6 * rng.uniform(1, 2, g)), fill(case["eta"], rng.uniform(1, 1e6, g)),
                                    fill(case["eta2"], rng.uniform(1, 1e6, g)), fill(hits, rng.integers(1, 99, g).astype(float)),
                                    fill(case["W"], 1e20 * rng.normal(size=(g, 2 * T))), n, case["beta"], pad=-7.5e18)
            for a, b in zip(clean, dirty):
                assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8)), (precision, nwin, n, T)


@pytest.mark.parametrize("T", mc.ABI_T + (1,))
@pytest.mark.parametrize("dtype,precision", FP)
def test_merge_abi_families_within_the_error_model(P, dtype, precision, T):
    """merge_abi<A> (the per-rank records of the split step, doubles) at nranks 1 .. 256: the same families."""
    worst, over = {}, []
    for case in mc.abi_cases(T):
        got = P.merge_abi(dtype, case["rho"], case["eta"], case["eta2"], case["W"], case["beta"])
        r = held(case, precision, (got[0], got[1], got[2], None, got[3]))
        for k, v in r.items():
            worst[(case["family"], k)] = max(worst.get((case["family"], k), 0.0), v)
            if not v <= 1.0:
                over.append((case["name"], k, v))
    print(f"merge_abi<{precision}> T={T}: max error / bound", {f"{f}.{k}": round(v, 4) for (f, k), v in sorted(worst.items())})
    assert not over, over[:10]
