"""References, error bounds and case tables for everything after the rollout: the softmin records {rho, eta, eta2, W[2T]}, the
rescale merge (merge_combine / merge_abi / k_merge of csrc/mppi_kernels.hip), the moving average, update, clamp and shift.
TEST INFRASTRUCTURE, no device import: tests/test_merge_cases.py checks these functions and tables on the CPU,
tests/test_gpu_merge_records.py and tests/test_gpu_filter_windows.py hold the kernels to them, tools/merge_report.py prints
the same figures.

Every function takes ``precision`` ("f32" / "f64", the handle's).  For f32 the inputs are first rounded to f32 -- what the
kernel's casts do to the doubles of the ABI -- and from there everything is f64 with `math.fsum` for the sums, so the reference
is the exactly rounded result of the rounded inputs.

Error model (first-order rounding; no tolerance is fixed by hand):

    bound(w_eps[i]) = c eps_A sum_b s_b |W_b[i]| / eta,   c = n + 24,   eps_A = 2^-24 / 2^-53,   s_b the reference scales

a plain sum of n terms costs (n - 1) eps; a scale that still matters has |beta (rho_b - rho)| <= ln(1 / eps_A), so the argument
rounding of exp2(x log2 e) costs about 9 eps and the hardware exp and rcp 1 ulp each; the rest is headroom for the products.
eta and eta2 take the same form (relative (n + 24) eps: all terms are positive) and ess = eta^2 / eta2 what follows from the
two.  u goes through the reference filter itself, which is linear with non-negative taps (the diff-drive edge factors
included):

    bound(u) = filter(bound(w_eps)) + (W + 8) eps_A (filter(|w_eps|) + |u_prev|)

The clamp is 1-Lipschitz and the shift a permutation: both carry the bound along unchanged.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import mppi_oracle

EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
# mppi_filter_mode of include/mppi_hip.h (tests/test_gpu_merge_records.py holds these to _capi's)
FILTER_DIFFDRIVE, FILTER_RACECAR, FILTER_NONE, FILTER_TORCH = 0, 1, 2, 3
FILTER_MODES = {"diffdrive": FILTER_DIFFDRIVE, "racecar": FILTER_RACECAR, "none": FILTER_NONE, "torch": FILTER_TORCH}
MERGE_MAX_RECORDS = 256  # per window (mppi_kernels.h)


def rounded(x, precision):
    """What the kernel's cast to the handle's precision leaves of a double, widened back to f64."""
    x = np.asarray(x, np.float64)
    return x.astype(np.float32).astype(np.float64) if precision == "f32" else x.copy()


def _fsum_cols(M):
    """Exactly rounded column sums of M[n, m]."""
    M = np.asarray(M, np.float64)
    return np.array([math.fsum(M[:, j]) for j in range(M.shape[1])]) if M.size else np.zeros(M.shape[1])


def scales(rho, beta, precision="f64"):
    """(min rho_b, s_b = exp(-beta (rho_b - min))) of the rounded inputs."""
    rho = rounded(np.reshape(rho, -1), precision)
    beta = float(rounded(beta, precision))
    r = float(rho.min())
    return r, np.array([math.exp(-beta * (x - r)) for x in rho])


def merge(rho, eta, eta2, W, beta, precision="f64"):
    """The rescale merge of records b = 0 .. n-1: rho = min rho_b, s_b = exp(-beta (rho_b - rho)), eta = sum s_b eta_b,
    eta2 = sum s_b^2 eta2_b, w_eps = sum s_b W_b / eta.  Returns (rho, eta, eta2, w_eps[2T]) in f64."""
    eta, eta2 = rounded(np.reshape(eta, -1), precision), rounded(np.reshape(eta2, -1), precision)
    W = rounded(np.reshape(W, (eta.size, -1)), precision)
    r, s = scales(rho, beta, precision)
    eta_m = math.fsum(s * eta)
    eta2_m = math.fsum(s * s * eta2)
    return r, eta_m, eta2_m, _fsum_cols(s[:, None] * W) / eta_m


def records_from_samples(S, eps, beta, bounds, precision="f64"):
    """Softmin records of sample groups.  S[K] the costs, eps[K, T, 2] the noise, ``bounds`` a list of (lo, hi) sample ranges.
    Returns (groups, whole): ``groups`` = (rho[g], eta[g], eta2[g], W[g, 2T]) with one record per range, ``whole`` the one
    record of all the samples the ranges cover, as (rho, eta, eta2, W[2T])."""
    S = rounded(np.reshape(S, -1), precision)
    beta = float(rounded(beta, precision))
    E = np.asarray(eps, np.float64).reshape(S.size, -1)

    def record(idx):
        r = float(S[idx].min())
        e = np.array([math.exp(-beta * (x - r)) for x in S[idx]])
        return r, math.fsum(e), math.fsum(e * e), _fsum_cols(e[:, None] * E[idx])

    recs = [record(np.arange(lo, hi)) for lo, hi in bounds]
    groups = (np.array([r[0] for r in recs]), np.array([r[1] for r in recs]), np.array([r[2] for r in recs]),
              np.stack([r[3] for r in recs]))
    whole = record(np.concatenate([np.arange(lo, hi) for lo, hi in bounds]))
    return groups, whole


def even_bounds(K, per):
    """Consecutive groups of ``per`` samples (the last one ragged)."""
    return [(lo, min(K, lo + per)) for lo in range(0, K, per)]


def moving_average(xx, mode, window):
    """The oracle's three filters in f64 (mode: mppi_filter_mode)."""
    xx = np.asarray(xx, np.float64)
    if mode == FILTER_NONE:
        return xx.copy()
    if mode == FILTER_DIFFDRIVE:
        return mppi_oracle.moving_average_diffdrive(xx, window)
    if mode == FILTER_RACECAR:
        return mppi_oracle.moving_average_racecar(xx, window, kernel_dtype=np.float64)
    if mode == FILTER_TORCH:
        return mppi_oracle.moving_average_torch(xx, window, dtype=np.float64)
    raise ValueError(f"filter mode {mode}")


def shift(u):
    """u_prev[:-1] = u[1:], u_prev[-1] = u[-1] (mppi_differential_drive.py:162-163)."""
    return np.concatenate([u[1:], u[-1:]], axis=0)


def finish(w_eps, u_prev, mode, window, clamp, umax, precision="f64"):
    """Filter, update, clamp and shift.  Returns {"u_updated": u + filter(w_eps), clamped to +-umax if ``clamp``; "u": the
    shifted sequence the step returns; "u0": its first row}."""
    w = np.asarray(w_eps, np.float64).reshape(-1, 2)
    un = rounded(u_prev, precision) + moving_average(w, mode, window)
    if clamp:
        m = rounded(umax, precision)
        un = np.clip(un, -m, m)
    u = shift(un)
    return {"u_updated": un, "u": u, "u0": u[0].copy()}


def bound(rho, eta, eta2, W, beta, precision="f64", n=None):
    """The error model of the module docstring for a merge of these records; ``n``: the number of summed terms (default: the
    number of records; K for a record reduced from K samples).  Returns {"w_eps": [2T], "eta", "eta2", "ess"}."""
    e = EPS[precision]
    eta, eta2 = rounded(np.reshape(eta, -1), precision), rounded(np.reshape(eta2, -1), precision)
    W = rounded(np.reshape(W, (eta.size, -1)), precision)
    _, s = scales(rho, beta, precision)
    c = (eta.size if n is None else n) + 24
    eta_m, eta2_m = math.fsum(s * eta), math.fsum(s * s * eta2)
    rel = c * e
    return {"w_eps": rel * _fsum_cols(s[:, None] * np.abs(W)) / eta_m, "eta": rel * eta_m, "eta2": rel * eta2_m,
            "ess": 3 * rel * eta_m * eta_m / eta2_m}


def bound_u(bound_w, w_eps, u_prev, mode, window, precision="f64"):
    """bound(u) of the module docstring for the updated sequence; `shift` it for the returned one."""
    bw = np.asarray(bound_w, np.float64).reshape(-1, 2)
    w = np.abs(np.asarray(w_eps, np.float64).reshape(-1, 2))
    return (moving_average(bw, mode, window) +
            (window + 8) * EPS[precision] * (moving_average(w, mode, window) + np.abs(rounded(u_prev, precision))))


def ratio(got, want, bnd):
    """Largest |got - want| / bound; an element with a zero bound must match exactly (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).reshape(-1)
    b = np.broadcast_to(np.asarray(bnd, np.float64), np.shape(got)).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(b > 0, err / b, np.inf))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------
# case tables: records of our own making.  A case is a dict {name, family, n, T, beta, rho, eta, eta2, W, ...}; the arrays are
# doubles as the ABI takes them (an f32 handle rounds them).  `check_case` asserts what the family states.
# ------------------------------------------------------------------------------------------------------------------
BETA = 0.5            # 1 / param_lambda of the test handles
COLLIDED_STEP_ARG = 0.25  # beta x the f32 spacing at the collided magnitude (the handles of that family: lambda = 4 spacing)
ABI_NRANKS = (1, 2, 3, 63, 64, 65, 255, 256)
ABI_T = (10, 33, 65)
FAMILIES = ("benign", "ties", "dominant", "collided", "cancelling")
# the internal-layout merge: records per window next to 32 / 64 / 256 / 512
WINDOW_N = {1: (1, 31, 32, 33, 63, 64, 65, 255, 256), 2: (257, 300, 511, 512)}
WINDOW_T = (1, 10, 33, 65)


def _rng(*key):
    return np.random.default_rng([20240809] + [int(k) for k in key])


def _heads(rng, n):
    eta = rng.uniform(1.0, 64.0, n)
    return eta, eta * rng.uniform(0.3, 1.0, n)  # eta2 <= eta (every term of a real record is <= 1)


def collided_spacing(T):
    """The f32 spacing at the cost of a sample that collided in every stage: 1e10 T."""
    return float(np.spacing(np.float32(1e10 * T)))


def collided_beta(T):
    return COLLIDED_STEP_ARG / collided_spacing(T)


def make_case(family, n, T, pos=None, seed=0):
    """One record set.  ``pos``: the record that carries the minimum (dominant / lone-minimum families)."""
    rng = _rng(FAMILIES.index(family) if family in FAMILIES else 9, n, T, 0 if pos is None else pos + 1, seed)
    eta, eta2 = _heads(rng, n)
    W = rng.normal(size=(n, 2 * T)) * eta[:, None] * 0.3
    beta = BETA
    if family == "benign":  # rho_b uniform in [0, 20 / beta]
        rho = rng.uniform(0.0, 20.0 / beta, n)
    elif family == "ties":  # every scale is exactly 1
        rho = np.full(n, 37.625)
    elif family == "dominant":  # one record at 0, the rest at or above 200 / beta
        rho = rng.uniform(200.0 / beta, 400.0 / beta, n)
        rho[pos] = 0.0
    elif family == "collided":  # 1e10 T plus multiples of the f32 spacing there: the difference must stay exact
        sp, beta = collided_spacing(T), collided_beta(T)
        k = rng.integers(0, 9, n)
        k[rng.integers(0, n)] = 0
        rho = float(np.float32(1e10 * T)) + sp * k
    elif family == "cancelling":  # W_b of alternating sign and nearly equal weight: the sum is far below its terms
        rho = rng.uniform(0.0, 2.0 / beta, n)
        base = rng.normal(size=2 * T)
        sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        W = sgn[:, None] * base[None, :] * np.exp(beta * (rho - rho.min()))[:, None] * (1.0 + 1e-3 * rng.normal(size=(n, 2 * T)))
    elif family == "lone_min":  # the minimum alone in one place, every other record a few units above
        rho = rng.uniform(3.0 / beta, 6.0 / beta, n)
        rho[pos] = 1.25
    else:
        raise ValueError(family)
    name = f"{family}-n{n}-T{T}" + ("" if pos is None else f"-at{pos}")
    return dict(name=name, family=family, n=n, T=T, beta=beta, pos=pos, rho=rho, eta=eta, eta2=eta2, W=W)


def dominant_positions(n):
    return sorted({p for p in (0, 63, 64, n - 1) if p < n})


def abi_cases(T, nranks_list=ABI_NRANKS):
    """The record families of the ABI merge (mppi_step_end) at horizon T, every nranks."""
    out = []
    for n in nranks_list:
        for fam in FAMILIES:
            if fam == "dominant":
                out += [make_case(fam, n, T, pos=p) for p in dominant_positions(n)]
            elif fam == "cancelling" and n < 2:
                continue  # (one record cancels nothing)
            else:
                out.append(make_case(fam, n, T))
    return out


def lone_min_positions(n):
    """The minimum alone in each of the eight 32-record groups of a window, at a wave boundary, and in the second window."""
    want = [32 * g for g in range(8)] + [32 * g + 31 for g in range(8)] + [63, 64, 256, 256 + 31, 256 + 32, 511]
    return sorted({p for p in want if p < n})


def window_cases(T, nwin):
    """The same families for the internal-layout merge (merge_combine<A, 256, NWIN>), plus the lone minimum."""
    out = []
    for n in WINDOW_N[nwin] if nwin == 1 else WINDOW_N[1][-2:] + WINDOW_N[2]:
        for fam in FAMILIES:
            if fam == "dominant":
                out += [make_case(fam, n, T, pos=p) for p in sorted(set(dominant_positions(n)) | ({256} if n > 256 else set()))]
            elif fam == "cancelling" and n < 2:
                continue
            else:
                out.append(make_case(fam, n, T))
        if n in (256, 512):
            out += [make_case("lone_min", n, T, pos=p) for p in lone_min_positions(n)]
    return out


def check_case(case, precision):
    """The conditions a family states, on the inputs as the kernel sees them.  Raises AssertionError with the case's name."""
    name, n, beta = case["name"], case["n"], case["beta"]
    rho = rounded(case["rho"], precision)
    r, s = scales(case["rho"], beta, precision)
    eta = rounded(case["eta"], precision)
    assert rho.shape == (n,) and case["W"].shape == (n, 2 * case["T"]) and (eta >= 1).all(), name
    assert np.isfinite(case["W"]).all() and np.isfinite(rho).all(), name
    fam = case["family"]
    if fam == "benign":
        assert (rho >= 0).all() and (rho <= 20.0 / beta * (1 + 1e-6)).all(), name
        assert n < 8 or s.min() < 1e-3, name  # the scales do spread
    elif fam == "ties":
        assert (s == 1.0).all() and (rho == rho[0]).all(), name
    elif fam == "dominant":
        p = case["pos"]
        assert rho[p] == 0.0 and r == 0.0 and (np.delete(rho, p) >= 200.0 / beta * (1 - 1e-6)).all(), name
        wgt = s * eta / math.fsum(s * eta)
        assert (np.delete(wgt, p) < 1e-30).all(), name  # every other reference weight
    elif fam == "collided":
        sp = collided_spacing(case["T"])
        assert (rho == case["rho"]).all(), name  # on the f32 grid: the cast changes nothing
        k = (rho - r) / sp
        assert (k == np.round(k)).all() and k.max() <= 8 and r >= 1e10 * case["T"] * (1 - 1e-6), name
        assert n < 4 or s.min() < 1.0, name  # not all of them tie
        np.testing.assert_allclose(s, np.exp(-COLLIDED_STEP_ARG * k), rtol=1e-6, err_msg=name)
    elif fam == "cancelling":
        W = rounded(case["W"], precision)
        tot, mag = np.abs((s[:, None] * W).sum(0)), (s[:, None] * np.abs(W)).sum(0)
        assert np.median(tot / mag) < (0.05 if n % 2 == 0 else 1.5 / n + 0.05), name
    elif fam == "lone_min":
        p = case["pos"]
        assert int(np.argmin(rho)) == p and (np.delete(rho, p) > rho[p] + 1.0).all(), name
        assert s[p] == 1.0 and np.delete(s, p).max() < 0.5 and np.delete(s, p).min() > 1e-3, name


def u_prev_signal(T):
    tt = np.arange(T)
    return np.stack([0.8 + 0.3 * np.sin(0.2 * tt), 0.05 * np.cos(0.1 * tt) - 0.02], axis=1)


def reference_step(case, u_prev, mode, window, clamp, umax, precision):
    """merge -> finish with every bound: what mppi_step_end must return for these records."""
    rho, eta, eta2, w = merge(case["rho"], case["eta"], case["eta2"], case["W"], case["beta"], precision)
    b = bound(case["rho"], case["eta"], case["eta2"], case["W"], case["beta"], precision)
    fin = finish(w, u_prev, mode, window, clamp, umax, precision)
    bu = shift(bound_u(b["w_eps"], w, u_prev, mode, window, precision))
    return dict(rho=rho, eta=eta, eta2=eta2, ess=eta * eta / eta2, w_eps=w, bounds=b, bound_u=bu, **fin)
