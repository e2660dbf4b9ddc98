"""References, error bounds and case tables for the `pytorch_mppi`-style controller (csrc/mppi_cb.hip behind
callback_mppi.py): the two dynamics, the running cost, the whole `command` (shift, clamp, noise taken back from the clamped
action, rollout, perturbation term, softmin, update), the in-kernel sampler `cb_noise` and the host's Cholesky factor and
inverse.  TEST INFRASTRUCTURE, no device import: tests/test_callback_cases.py checks these functions and tables on the CPU,
tests/test_gpu_callback_edges.py holds the kernels to them, tools/callback_report.py prints the same figures.

PARITY UNPINNED, as everywhere around this controller: the reference here is the restated algorithm of
oracle/mppi_cb_oracle.py carried out in f64, not an execution of the library.

Every reference first rounds its inputs to f32 -- what the ABI's casts do to the doubles it is handed (`rounded`, as in
tests/merge_checks.py) -- and from there everything is f64, with `math.fsum` for the sums over K.  The covariance is the one
input the ABI does not cast: the host factors and inverts it in f64 and casts L and Sigma^-1, and so do the references.

Error models (first-order rounding, EPS = 2^-24; no tolerance is fixed by hand)

  dynamics     every component is s + dt * (a short sum of products of the inputs, sin / cos of the heading):
                   bound = DYN_OPS EPS (|s| + dt sum |terms|),   DYN_OPS = 10
               the longest chain is the skid-steer's dv: the constant r / (4 m) 2 roundings, the sum of four forces 3, its
               product 1, damp * v 1, the difference 1, the product with dt 1, the sum with s 1 = 10; the x and y rows
               need 5 (sin / cos 2 ulp at any heading, two products, one sum).

  running cost (s - g)^T Q (s - g) + u^T R u + w sum_m o_m(d_m), n = nx + nu + n_obs summed terms:
                   bound = COST(n) EPS sum |terms| + w sum_m |o_m'(d_m)| bound(d_m),   COST(n) = n + 8
               a sum of n terms costs n - 1 roundings of the partial sums, each term carries at most 4 of its own
               (difference, square, product with the weight; for an obstacle term the sum d + 1e-6 and the division, or
               the difference d - safety, its sign and a 2-ulp exp), the product with w and the last sum 2, 2 to spare.
               The distance is not well conditioned where an obstacle moves: its centre is c + v t in f32,
                   bound(d) = EPS (5 d + [vx t != 0] 2 (|cx| + |vx t|) + [vy t != 0] 2 (|cy| + |vy t|))
               (each difference 1 ulp of itself, the squares, their sum and the root 3 ulps of d; a static centre is
               exact, so a state ON it gives d = 0 exactly and the 1 / (0 + 1e-6) term its 1e6), and the obstacle term
               passes that on with its slope: 1 / (d + 1e-6)^2 for the inverse cost, o itself for the exponential one.
               The exponential's argument adds EXP_ARG |d - safety| EPS o (x log2 e rounded once inside expf).

  cost_total   no a-priori model: T steps of dynamics feed each other.  The yardstick is the distance of the f32
               restatement (oracle/mppi_cb_oracle.py, unchanged) from the f64 reference on the same inputs,
                   dist = max_k |c_k - c64_k| / max(|c64_k|, 1)   over the samples that are kept,
               and the device is entitled to COST_FACTOR times that: it sums in another order and uses other
               sin / cos / exp / sqrt than NumPy.  COST_FACTOR is the smallest power of two that is at least twice the
               largest ratio device distance / restatement distance measured on the MI355X over every case
               (profiles/callback_measured.json, tools/callback_report.py).

  omega        against the f64 softmin of the costs the device returned, x_k = (c_k - beta) / lambda:
                   relative (|x_k| + K + 16) EPS
               (the argument's rounding |x_k|, the exp, the K-term sum and the division), plus 2^-126 absolute: a weight
               below the smallest normal f32 may be flushed to zero.

  U            against U + sum_k omega_k noise_k in f64 with the omega the device returned:
                   (K + 8) EPS sum_k omega_k |noise_k| + EPS |U_new|

  sampler      |z - z_ref| <= SAMPLER_ATOL + 2^-21: the project's tolerance for its Philox / Box-Muller sampler
               (tests/test_gpu_engine.py::test_sampler_matches_numpy_restatement) plus the rounding of (1 + n) - 1 at
               |1 + n| < 8, which is how the probe reads a number out of the kernel (`probe_value`).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import mppi_cb_oracle as cbo
from oracle import philox

EPS = 2.0 ** -24
DYN_OPS = 10
EXP_ARG = 2
SAMPLER_ATOL = 4e-6            # tests/test_gpu_engine.py::test_sampler_matches_numpy_restatement
PROBE_ROUNDING = 2.0 ** -21    # (1 + n) - 1 in f32 at |1 + n| < 8
COST_FACTOR = 4                # measured: see the module docstring and profiles/callback_measured.json
COST_RATIO_FINDING = 16        # a device / restatement ratio above this is a defect to explain, not a tolerance
STEP_MARGIN = 1e-3             # a sample within this of a safety boundary at any step is left out of the cost comparison
EXCLUDED_CAP = 0.10            # ... at most this share of K
ACTIVE_FLOOR = 0.20            # inverse cost: at least this share of the kept samples meets an obstacle at some step
ESS_FLOOR = 1.0 / 8.0          # spread cases: ESS >= K / 8
NOMINAL_SHARE = 0.02           # spread cases: |U| <= 2 % of the bounds
OMEGA_FLOOR = 2.0 ** -126     # exp(-x) below the smallest normal f32 may come back as 0
CB_STREAM = 0x6362             # the fourth counter word of cb_noise
SKID = dict(m=2.0, I=0.05, r=0.1, L=0.4, damping=0.1)  # callback_mppi.py's constants (test/test_mppi_diff_dyna.py:15-19, :29-30)
NX = {"unicycle": 3, "skid_steer": 5}
NU = {"unicycle": 2, "skid_steer": 4}
DT = {"unicycle": 0.05, "skid_steer": 0.02}


def rounded(x):
    """What the ABI's cast to f32 leaves of a double, widened back to f64."""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _r(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------
# the covariance: a transcription of mppi_cb_create's recurrences (stride 4, f64) next to plain numpy.linalg
# ------------------------------------------------------------------------------------------------------------------
SIGMA2 = np.array([[0.5, 0.19], [0.19, 0.3]])  # correlation 0.19 / sqrt(0.15) = 0.49
SIGMA4 = np.array([[1.30, 0.40, -0.30, 0.20],
                   [0.40, 0.90, 0.25, -0.15],
                   [-0.30, 0.25, 1.10, 0.35],
                   [0.20, -0.15, 0.35, 0.80]])  # no zero entry
SIGMAS = {"unicycle": SIGMA2, "skid_steer": SIGMA4}
SYMMETRY_RTOL = 1e-9  # mppi_cb_create: |S_ij - S_ji| <= this * sqrt(S_ii S_jj)


def host_factor(sigma):
    """(L, L^-1, Sigma^-1) as 4 x 4 f64 arrays by the recurrences of mppi_cb_create: only the lower triangle of sigma is read.
    Raises ValueError where the host refuses (a pivot that is not positive)."""
    s = np.asarray(sigma, np.float64)
    nu = s.shape[0]
    S = np.zeros(16)
    for i in range(nu):
        for j in range(nu):
            S[4 * i + j] = s[i, j]
    L, Li, Sinv = np.zeros(16), np.zeros(16), np.zeros(16)
    for i in range(nu):
        for j in range(i + 1):
            a = S[i * 4 + j]
            for k in range(j):
                a -= L[i * 4 + k] * L[j * 4 + k]
            if i == j:
                if not a > 0:
                    raise ValueError("noise_sigma must be symmetric positive definite")
                L[i * 4 + i] = math.sqrt(a)
            else:
                L[i * 4 + j] = a / L[j * 4 + j]
    for i in range(nu):
        Li[i * 4 + i] = 1.0 / L[i * 4 + i]
        for j in range(i):
            a = 0.0
            for k in range(j, i):
                a -= L[i * 4 + k] * Li[k * 4 + j]
            Li[i * 4 + j] = a / L[i * 4 + i]
    for i in range(nu):
        for j in range(nu):
            a = 0.0
            for k in range(nu):
                a += Li[k * 4 + i] * Li[k * 4 + j]
            Sinv[i * 4 + j] = a
    return L.reshape(4, 4), Li.reshape(4, 4), Sinv.reshape(4, 4)


def factor(sigma):
    """(L, Sigma^-1) by numpy.linalg in f64, each rounded to f32 the way the handle stores it."""
    s = np.asarray(sigma, np.float64)
    return rounded(np.linalg.cholesky(s)), rounded(np.linalg.inv(s))


def is_symmetric(sigma):
    """The host's test: the two triangles agree within SYMMETRY_RTOL of the diagonal's scale."""
    s = np.asarray(sigma, np.float64)
    d = np.sqrt(np.abs(np.outer(np.diag(s), np.diag(s))))
    return bool((np.abs(s - s.T) <= SYMMETRY_RTOL * d).all())


# ------------------------------------------------------------------------------------------------------------------
# the models in f64
# ------------------------------------------------------------------------------------------------------------------
def dynamics_terms(dyn, s, u):
    """(s, inc[n, nx, m]): the state and, per component, the terms whose sum times dt is added to it.  Inputs as given."""
    s, u = np.asarray(s, np.float64), np.asarray(u, np.float64)
    n = s.shape[0]
    th = s[:, 2]
    if dyn == "unicycle":
        inc = np.zeros((n, 3, 1))
        inc[:, 0, 0], inc[:, 1, 0], inc[:, 2, 0] = u[:, 0] * np.cos(th), u[:, 0] * np.sin(th), u[:, 1]
    else:
        m, I, r, L, damp = (_r(SKID[k]) for k in ("m", "I", "r", "L", "damping"))
        v, om = s[:, 3], s[:, 4]
        inc = np.zeros((n, 5, 5))
        inc[:, 0, 0], inc[:, 1, 0], inc[:, 2, 0] = v * np.cos(th), v * np.sin(th), om
        inc[:, 3, :4] = (r / (4.0 * m)) * u
        inc[:, 3, 4] = -damp * v
        inc[:, 4, :4] = (r / (L * I)) * u * np.array([1.0, -1.0, 1.0, -1.0]) / 2.0
        inc[:, 4, 4] = -damp * om
    return s, inc


def dynamics(dyn, s, u, dt, inputs_f32=True):
    """One step of the model in f64 on inputs rounded to f32 (``inputs_f32=False``: on the f64 inputs as they are, for the
    steps inside a rollout).  Returns (next[n, nx], bound[n, nx])."""
    dt = _r(dt)
    s, inc = dynamics_terms(dyn, *((rounded(s), rounded(u)) if inputs_f32 else (s, u)))
    nxt = s + dt * inc.sum(-1)
    return nxt, DYN_OPS * EPS * (np.abs(s) + dt * np.abs(inc).sum(-1))


def cost_ops(n_terms):
    """COST(n) of the module docstring."""
    return n_terms + 8


def running_cost(s, u, t, cost, inputs_f32=True):
    """The running cost in f64 on inputs rounded to f32 (``inputs_f32`` as in `dynamics`; the parameters are rounded either
    way).  ``cost``: dict(goal, q, r, obstacles[m, 4], safety, weight, kind).
    Returns (c[n], bound[n], d[n, m]): the cost, its error bound and the distance to every obstacle's centre."""
    s, u = (rounded(s), rounded(u)) if inputs_f32 else (np.asarray(s, np.float64), np.asarray(u, np.float64))
    n, nx, nu = s.shape[0], s.shape[1], u.shape[1]
    goal, q, r = rounded(cost["goal"])[:nx], rounded(cost["q"])[:nx], rounded(cost["r"])[:nu]
    obs = rounded(cost["obstacles"]).reshape(-1, 4)
    safety, w, tiny = _r(cost["safety"]), _r(cost["weight"]), _r(1e-6)
    e = s - goal
    terms = [q * e * e, r * u * u]
    d = np.zeros((n, obs.shape[0]))
    o, slope_err = np.zeros((n, obs.shape[0])), np.zeros((n, obs.shape[0]))
    for m, (cx, cy, vx, vy) in enumerate(obs):
        ox, oy = cx + vx * float(t), cy + vy * float(t)
        d[:, m] = np.sqrt((s[:, 0] - ox) ** 2 + (s[:, 1] - oy) ** 2)
        bd = EPS * (5.0 * d[:, m] + (2.0 * (abs(cx) + abs(vx * t)) if vx * t != 0 else 0.0)
                    + (2.0 * (abs(cy) + abs(vy * t)) if vy * t != 0 else 0.0))
        if cost["kind"] == "inverse":
            inside = d[:, m] < safety
            o[:, m] = np.where(inside, 1.0 / (d[:, m] + tiny), 0.0)
            slope_err[:, m] = o[:, m] ** 2 * bd
        else:
            o[:, m] = np.exp(-(d[:, m] - safety))
            slope_err[:, m] = o[:, m] * (bd + EXP_ARG * EPS * np.abs(d[:, m] - safety))
    terms.append(w * o)
    T = np.concatenate(terms, axis=1)
    c = np.array([math.fsum(row) for row in T])
    bound = cost_ops(T.shape[1]) * EPS * np.abs(T).sum(1) + abs(w) * slope_err.sum(1)
    return c, bound, d


def step_margin(d, cost):
    """Smallest |d - safety| over the obstacles (inf for the continuous exponential cost or no obstacle)."""
    if cost["kind"] != "inverse" or d.shape[1] == 0:
        return np.full(d.shape[0], np.inf)
    return np.abs(d - _r(cost["safety"])).min(1)


# ------------------------------------------------------------------------------------------------------------------
# the whole command in f64
# ------------------------------------------------------------------------------------------------------------------
def shift(U, u_init):
    return np.vstack([U[1:], rounded(u_init)[None]])


def softmin(c, lam):
    """(omega[K], x[K]) of costs c: x = (c - min c) / lambda, omega = exp(-x) / fsum."""
    c = np.asarray(c, np.float64)
    x = (c - c.min()) / lam
    e = np.exp(-x)
    return e / math.fsum(e), x


def bound_omega(omega, x, K):
    """Error bound of omega_k: relative (|x_k| + K + 16) EPS, and the smallest normal f32 below which a weight may be flushed."""
    return (np.abs(x) + K + 16) * EPS * np.asarray(omega, np.float64) + OMEGA_FLOOR


def update(U, omega, noise):
    """(U_new[T, nu], bound[T, nu]) = U + sum_k omega_k noise_k with fsum over K, and the U error model."""
    K = noise.shape[0]
    wn = np.asarray(omega, np.float64)[:, None, None] * noise
    flat = wn.reshape(K, -1)
    acc = np.array([math.fsum(flat[:, j]) for j in range(flat.shape[1])]).reshape(U.shape)
    mag = np.array([math.fsum(np.abs(flat[:, j])) for j in range(flat.shape[1])]).reshape(U.shape)
    new = U + acc
    return new, (K + 8) * EPS * mag + EPS * np.abs(new)


def clamped_noise(case, U, noise, do_shift=True):
    """(U after the shift, the clamped actions [K, T, nu], the noise taken back from them) of a command on the nominal
    sequence ``U`` with the draw ``noise``, both rounded to f32 here; the last sample is the null action where the case says."""
    K, T, nu = case["K"], case["T"], NU[case["dyn"]]
    U = rounded(U).reshape(T, nu)
    if do_shift:
        U = shift(U, case["u_init"])
    act = U[None] + rounded(noise).reshape(K, T, nu)
    if case["null"]:
        act[K - 1] = 0.0
    act = np.clip(act, rounded(case["u_min"]), rounded(case["u_max"]))
    return U, act, act - U[None]


def command(case, state, U, noise, do_shift=True):
    """One `command` in f64.  ``case``: a dict of the tables below; ``U`` the nominal sequence before the call and ``noise``
    [K, T, nu] the injected draw, both rounded to f32 here.  Returns a dict: U_shifted, act, noise (taken back from the
    clamped action), running (the sum of running costs), pert, cost_total, omega, x, U_new, action, margin[K] (the closest
    any step came to a safety boundary), active[K] (an obstacle term was non-zero at some step), keep[K]."""
    dyn, cost, lam, dt = case["dyn"], case["cost"], _r(case["lam"]), case["dt"]
    K, T = case["K"], case["T"]
    U, act, nz = clamped_noise(case, U, noise, do_shift)
    _, sinv = factor(case["sigma"])
    s = np.tile(rounded(state), (K, 1))
    per_step = np.zeros((T, K))
    margin, active = np.full(K, np.inf), np.zeros(K, bool)
    for t in range(T):
        s, _ = dynamics(dyn, s, act[:, t], dt, inputs_f32=False)
        per_step[t], _, d = running_cost(s, act[:, t], t, cost, inputs_f32=False)
        margin = np.minimum(margin, step_margin(d, cost))
        if cost["kind"] == "inverse" and d.shape[1]:
            active |= (d < _r(cost["safety"])).any(1)
    running = np.array([math.fsum(per_step[:, k]) for k in range(K)])
    pterm = (U[None] * lam * (nz @ sinv)).reshape(K, -1)  # sum_j noise_j sinv[j, i], times U_i lambda
    pert = np.array([math.fsum(row) for row in pterm])
    total = running + pert
    omega, x = softmin(total, lam)
    U_new, _ = update(U, omega, nz)
    return dict(U_shifted=U, act=act, noise=nz, running=running, pert=pert, cost_total=total, omega=omega, x=x, U_new=U_new,
                action=U_new[0].copy(), margin=margin, active=active, keep=margin >= STEP_MARGIN)


def ess(omega):
    return 1.0 / math.fsum(np.asarray(omega, np.float64) ** 2)


def restatement(case, state, U, noise, do_shift=True):
    """The same command by oracle/mppi_cb_oracle.py, unchanged (f32).  Returns the oracle after the call."""
    dyn, cost = case["dyn"], case["cost"]
    kw = dict(goal=cost["goal"], q_diag=cost["q"], r_diag=cost["r"], obstacles=cost["obstacles"], safety=cost["safety"],
              weight=cost["weight"], kind=cost["kind"])
    o = cbo.MPPIOracle(dyn, kw, NX[dyn], np.asarray(case["sigma"]), case["K"], case["T"], case["lam"], case["u_min"], case["u_max"],
                       u_init=case["u_init"], sample_null_action=case["null"], dyn_kw=dict(dt=case["dt"]))
    o.U = np.asarray(U, np.float32).reshape(case["T"], NU[dyn]).copy()
    o.command(np.asarray(state, np.float32), np.asarray(noise, np.float32), shift=do_shift)
    return o


def cost_distance(c, c64, keep):
    """max_k |c_k - c64_k| / max(|c64_k|, 1) over the kept samples."""
    c, c64 = np.asarray(c, np.float64)[keep], np.asarray(c64, np.float64)[keep]
    return float(np.max(np.abs(c - c64) / np.maximum(np.abs(c64), 1.0))) if c.size else 0.0


def ratio(got, want, bnd):
    """Largest |got - want| / bound; an element with a zero bound must match exactly (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).reshape(-1)
    b = np.broadcast_to(np.asarray(bnd, np.float64), np.shape(got)).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(b > 0, err / b, np.inf))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------
# the in-kernel sampler
# ------------------------------------------------------------------------------------------------------------------
def cb_normals(seed, iteration, K, T):
    """z[K, T, 4] in f64: Philox4x32-10 with counter (k, t, iteration, 0x6362) and the seed's halves as the key; words
    (r0, r1) give (z0, z1) and (r2, r3) give (z2, z3) by Box-Muller (radius from the first word, angle from the second)."""
    k = np.arange(K, dtype=np.uint32)[:, None]
    t = np.arange(T, dtype=np.uint32)[None, :]
    r = philox.philox4x32_10(k, t, np.uint32(iteration & 0xFFFFFFFF), np.uint32(CB_STREAM), seed & 0xFFFFFFFF,
                             (seed >> 32) & 0xFFFFFFFF)
    out = []
    for ra, rb in ((r[0], r[1]), (r[2], r[3])):
        rad = np.sqrt(-2.0 * np.log(philox.uniform_open(ra)))
        ang = 2.0 * np.pi * philox.uniform_open(rb)
        out += [rad * np.cos(ang), rad * np.sin(ang)]
    return np.stack(out, axis=-1)


def cb_noise(sigma, seed, iteration, K, T):
    """noise[K, T, nu] = L z in f64 with L rounded to f32."""
    L, _ = factor(sigma)
    nu = L.shape[0]
    return cb_normals(seed, iteration, K, T)[..., :nu] @ L.T


def probe_value(sigma, seed, iteration, K, T, t0, i):
    """What `cost_total` holds after a command on the probe handle (q = r = 0, no obstacle, no bounds, lambda = 1, no shift)
    whose nominal sequence is 1 at (t0, i) and 0 elsewhere: (Sigma^-1 noise[k, t0])_i, and its tolerance
    (SAMPLER_ATOL + 2^-21) * sum_j |L^-T[i, j]|  (= SAMPLER_ATOL + 2^-21 for Sigma = I, where the value is z_i)."""
    _, sinv = factor(sigma)
    n = cb_noise(sigma, seed, iteration, K, T)[:, t0]
    LiT = np.linalg.inv(np.linalg.cholesky(np.asarray(sigma, np.float64))).T
    return n @ sinv[:, i], (SAMPLER_ATOL + PROBE_ROUNDING) * np.abs(LiT[i]).sum()


def probe_cost():
    return dict(goal=np.zeros(5), q=np.zeros(5), r=np.zeros(4), obstacles=np.zeros((0, 4)), safety=1.0, weight=0.0,
                kind="inverse")


# ------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------
def _cost(name, n_obs=None):
    """The callers' three running costs (callback_mppi.RunningCost's constructors) by name, as plain data."""
    table = {
        "static": dict(goal=[6.0, 6.0, 1.57], q=[20, 5, 9], r=[0.1, 0.1], obstacles=[[5.0, 4.0, 0, 0], [3.5, 3.5, 0, 0]],
                       safety=0.8, weight=10.0, kind="inverse"),
        "moving": dict(goal=[5.0, 4.0, 1.57], q=[10.0, 5.0, 9.0], r=[1.0, 10.0],
                       obstacles=[[5.0, 5.0, 0.0, -0.05], [7.0, 3.0, 0.0, 0.05]], safety=1.0, weight=1.0, kind="exponential"),
        "skid": dict(goal=[6.0, 6.0, 1.57, 2.0, 0.0], q=[200, 200, 20, 10, 20], r=[0.001] * 4,
                     obstacles=[[5.0, 4.0, 0, 0], [3.5, 3.5, 0, 0]], safety=0.8, weight=10.0, kind="inverse"),
        # the fourth crossing: skid-steer with the exponential cost and moving obstacles
        "skid_exp": dict(goal=[6.0, 6.0, 1.57, 2.0, 0.0], q=[200, 200, 20, 10, 20], r=[0.001] * 4,
                         obstacles=[[5.0, 5.0, 0.0, -0.05], [7.0, 3.0, 0.0, 0.05]], safety=1.0, weight=1.0, kind="exponential"),
        # and the unicycle crossed the other way, with moving obstacles under the inverse cost
        "uni_inv_moving": dict(goal=[6.0, 6.0, 1.57], q=[20, 5, 9], r=[0.1, 0.1],
                               obstacles=[[5.0, 4.0, 0.01, -0.02], [3.5, 3.5, -0.015, 0.01]], safety=0.8, weight=10.0,
                               kind="inverse"),
    }
    c = {k: (np.asarray(v, np.float64) if k not in ("kind", "safety", "weight") else v) for k, v in table[name].items()}
    c["obstacles"] = c["obstacles"].reshape(-1, 4)
    if n_obs is not None:
        c["obstacles"] = obstacle_field(c["obstacles"], n_obs)
    return c


def obstacle_field(base, n_obs):
    """``n_obs`` obstacles: the base ones first, then more on a ring around (4.5, 4) with small velocities."""
    rows = [r for r in base[:n_obs]]
    for m in range(len(rows), n_obs):
        a = 0.7 * m
        rows.append(np.array([4.5 + 2.5 * math.cos(a), 4.0 + 2.5 * math.sin(a), 0.02 * math.sin(3 * a), 0.02 * math.cos(5 * a)]))
    return np.array(rows).reshape(-1, 4)


def _rng(*key):
    return np.random.default_rng([20250117] + [int(k) for k in key])


def _case(name, family, dyn, cost, K, T, state, null=False, bounded=True, lam=1.0, u_init=None, seed=0):
    nu = NU[dyn]
    lim = 2.0 if dyn == "unicycle" else 5.0
    c = dict(name=name, family=family, dyn=dyn, cost=_cost(cost), cost_name=cost, K=K, T=T, dt=DT[dyn], sigma=SIGMAS[dyn],
             null=null, lam=lam, state=np.asarray(state, np.float64), bounded=bounded, lim=lim,
             u_min=np.full(nu, -lim if bounded else -1e30), u_max=np.full(nu, lim if bounded else 1e30),
             u_init=np.zeros(nu) if u_init is None else np.asarray(u_init, np.float64), seed=seed)
    rng = _rng(K, T, nu, seed, 0 if family == "clamp" else 1)
    L = np.linalg.cholesky(c["sigma"])
    c["noise"] = (rng.normal(size=(K, T, nu)) @ L.T).astype(np.float32)
    sd = np.sqrt(np.diag(c["sigma"]))
    if family == "clamp":
        # the nominal sequence sits half a standard deviation inside a bound on every third entry (the clamp binds on about a
        # third of those draws), at a moderate value elsewhere (it binds on none): the sequence before the shift
        U = rng.uniform(-0.3, 0.3, (T, nu)) * lim
        idx = np.arange(T * nu).reshape(T, nu)
        edge = (lim - 0.5 * sd)[None, :] * np.where(idx % 2 == 0, 1.0, -1.0)
        U = np.where(idx % 3 == 0, edge, U)
    else:
        U = rng.uniform(-1.0, 1.0, (T, nu)) * nominal_amplitude(c["sigma"], T, lim)
    c["U"] = U.astype(np.float32)
    return c


def nominal_amplitude(sigma, T, lim):
    """The amplitude of a spread case's nominal sequence: at most NOMINAL_SHARE of the bounds, and small enough that the
    perturbation term leaves the weights spread.  That term enters the softmin's argument as U^T Sigma^-1 noise whatever
    lambda is; for U uniform in +-a its standard deviation is sqrt(sum_t U_t^T Sigma^-1 U_t) <= a sqrt(T tr(Sigma^-1) / 3),
    held to 1/2 here."""
    tr = float(np.trace(np.linalg.inv(np.asarray(sigma, np.float64))))
    return min(NOMINAL_SHARE * lim, 0.5 / math.sqrt(T * tr / 3.0))


def _spread(case):
    """lambda of a spread case: the standard deviation of the reference's summed running costs (the perturbation term
    scales with lambda itself, so it stays out of the figure that fixes lambda), as the f32 the handle will hold."""
    ref = command(dict(case, lam=1.0), case["state"], case["U"], case["noise"])
    case["lam"] = _r(np.std(ref["running"]))
    return case


UNI_START = (4.0, 3.0, 0.9)               # heads between the two static obstacles
UNI_CLAMP_START = (3.8, 3.2, 1.1)         # the same for the faster nominal sequences of the clamp family
SKID_START = (4.75, 3.8, 0.3, 4.0, 0.0)   # inside the first obstacle's distance at 4 m/s: the forces change the speed slowly

_CASES = None


def cases():
    """Every command case.  family "clamp": lambda = 1 (all the weight on one sample, the callers' regime) and a nominal
    sequence on which the clamp binds in places; family "spread": a small nominal sequence and lambda = std of the costs."""
    global _CASES
    if _CASES is None:
        cl = [
            _case("uni-inv-K1-T25", "clamp", "unicycle", "static", 1, 25, UNI_CLAMP_START),
            _case("uni-exp-K255-T1-null", "clamp", "unicycle", "moving", 255, 1, UNI_CLAMP_START, null=True, u_init=[1.7, -0.4]),
            _case("uni-inv-K256-T25-null", "clamp", "unicycle", "static", 256, 25, UNI_CLAMP_START, null=True),
            _case("uni-inv-K257-T25", "clamp", "unicycle", "uni_inv_moving", 257, 25, UNI_CLAMP_START, u_init=[0.4, -0.3]),
            _case("uni-exp-K257-T128", "clamp", "unicycle", "moving", 257, 128, UNI_CLAMP_START),
            _case("skid-inv-K1-T64", "clamp", "skid_steer", "skid", 1, 64, SKID_START),
            _case("skid-exp-K257-T64-null", "clamp", "skid_steer", "skid_exp", 257, 64, SKID_START, null=True),
            _case("skid-inv-K256-T7-free", "clamp", "skid_steer", "skid", 256, 7, SKID_START, bounded=False),
            _case("skid-inv-K257-T64", "clamp", "skid_steer", "skid", 257, 64, SKID_START, u_init=[3.0, -2.0, 1.0, 0.5]),
        ]
        sp = [
            _case("spread-uni-inv-K256-T25", "spread", "unicycle", "static", 256, 25, UNI_START),
            _case("spread-uni-exp-K257-T128", "spread", "unicycle", "moving", 257, 128, UNI_START, null=True),
            _case("spread-uni-exp-K255-T1", "spread", "unicycle", "moving", 255, 1, UNI_START),
            _case("spread-uni-inv-K1000-T25", "spread", "unicycle", "static", 1000, 25, UNI_START),
            _case("spread-skid-inv-K257-T64", "spread", "skid_steer", "skid", 257, 64, SKID_START, null=True),
            _case("spread-skid-exp-K256-T7-free", "spread", "skid_steer", "skid_exp", 256, 7, SKID_START, bounded=False),
        ]
        _CASES = {c["name"]: c for c in cl + [_spread(c) for c in sp]}
    return _CASES


_REFS = {}


def reference(name):
    """(f64 reference, f32 restatement, restatement's distance) of a case: computed once, shared, not to be modified."""
    if name not in _REFS:
        c = cases()[name]
        ref = command(c, c["state"], c["U"], c["noise"])
        o = restatement(c, c["state"], c["U"], c["noise"])
        _REFS[name] = (ref, o, cost_distance(o.cost_total, ref["cost_total"], ref["keep"]))
    return _REFS[name]


def check_case(name):
    """The conditions a case states, from the references alone.  Raises AssertionError with the case's name."""
    c = cases()[name]
    ref, o, dist = reference(name)
    K, lim = c["K"], c["lim"]
    assert K <= 1000 and c["T"] * NU[c["dyn"]] <= 256, name
    left_out = int((~ref["keep"]).sum())
    assert left_out <= EXCLUDED_CAP * K, (name, left_out)
    if c["cost"]["kind"] == "inverse":
        kept_active = int((ref["active"] & ref["keep"]).sum())
        assert kept_active >= ACTIVE_FLOOR * int(ref["keep"].sum()), (name, kept_active)
    else:
        assert left_out == 0, name
    # an honest f32 evaluation and not an exact one: within 16 roundings a step of the running sum's magnitude
    assert np.isfinite(ref["cost_total"]).all() and 0 < dist <= 16 * c["T"] * EPS, (name, dist)
    raw = ref["U_shifted"][None] + rounded(c["noise"])
    if c["null"]:
        raw[K - 1] = 0.0
    bind = (raw != ref["act"])
    if c["family"] == "clamp":
        assert c["lam"] == 1.0, name
        if c["bounded"]:
            per_entry = bind.mean(0)  # the share of samples on which each (t, i) is clamped
            assert (per_entry > 0.1).any() and (per_entry == 0).any(), name
        else:
            assert not bind.any(), name
    else:
        assert np.abs(ref["U_shifted"]).max() <= NOMINAL_SHARE * lim * (1 + 1e-6), name
        assert ess(ref["omega"]) >= ESS_FLOOR * K, (name, ess(ref["omega"]))
        assert ess(ref["omega"]) <= 0.9 * K, (name, ess(ref["omega"]))  # and the weights are not all equal either


# ------------------------------------------------------------------------------------------------------------------
# the models alone: rows for mppi_cb_eval
# ------------------------------------------------------------------------------------------------------------------
MODEL_N = (1, 255, 256, 257)
MODEL_N_OBS = (0, 1, 16)
MODEL_PAIRS = (("unicycle", "static"), ("unicycle", "moving"), ("skid_steer", "skid"), ("skid_steer", "skid_exp"))
MODEL_T = 25
RIM = 1e-3  # rows at d = safety (1 +- RIM)


def model_rows(dyn, cost_name, n, n_obs, t):
    """(states[n, nx], actions[n, nu], cost) for `_dynamics` / `_running_cost` at step t: random rows, headings up to 1e3, and
    -- in this order from row 0, as far as n reaches -- a row ON obstacle 0's centre (static obstacles only: d = 0), rows at
    d = safety (1 - RIM) and safety (1 + RIM) from it, and rows scattered inside its safety distance."""
    nx, nu = NX[dyn], NU[dyn]
    cost = _cost(cost_name, n_obs)
    rng = _rng(n, n_obs, t, nx, len(cost_name))
    s = rng.normal(0, 3, (n, nx))
    s[:, 2] = rng.uniform(-1e3, 1e3, n)
    if n > 1:
        s[n // 2, 2], s[n - 1, 2] = 1e3, -1e3
    a = rng.normal(0, 1.5, (n, nu)) * (1.0 if dyn == "unicycle" else 30.0)
    if n_obs:
        cx, cy, vx, vy = rounded(cost["obstacles"][0])
        # the centre as the kernel forms it, in f32: c + v t with both roundings (or one, fused: the rows below keep RIM away)
        ox = float(np.float32(np.float32(cx) + np.float32(np.float32(vx) * np.float32(t))))
        oy = float(np.float32(np.float32(cy) + np.float32(np.float32(vy) * np.float32(t))))
        safety = _r(cost["safety"])
        special = []
        if vx * t == 0 and vy * t == 0:
            special.append((ox, oy))
        for k, f in enumerate((1 - RIM, 1 + RIM, 1 - RIM, 1 + RIM)):
            ang = 0.4 + 1.3 * k
            special.append((ox + safety * f * math.cos(ang), oy + safety * f * math.sin(ang)))
        for _ in range(12):
            rad, ang = rng.uniform(0.05, 0.95) * safety, rng.uniform(0, 2 * math.pi)
            special.append((ox + rad * math.cos(ang), oy + rad * math.sin(ang)))
        for row, (x, y) in enumerate(special[:n]):
            s[row, 0], s[row, 1] = x, y
    return s.astype(np.float32), a.astype(np.float32), cost


def check_model_rows(dyn, cost_name, n, n_obs, t):
    """The rows are what `model_rows` says: a row at d = 0 where the obstacle stands still, rows on either side of the inverse
    cost's step and none so near it that f32 could flip it, headings that reach 1e3."""
    s, a, cost = model_rows(dyn, cost_name, n, n_obs, t)
    c, bound, d = running_cost(s, a, t, cost)
    name = (dyn, cost_name, n, n_obs, t)
    assert np.isfinite(c).all() and (bound > 0).all() and (bound <= 1e-4 * np.maximum(np.abs(c), 1.0)).all(), name
    if n > 1:
        assert np.abs(s[:, 2]).max() == 1e3, name
    if n_obs and cost["kind"] == "inverse":
        safety = _r(cost["safety"])
        assert (np.abs(d - safety) > 1e-5 * safety).all(), name  # 5 ulps of d are 3e-7 d: the step cannot flip
        if n >= 8:
            still = not (cost["obstacles"][0, 2:] * t).any()
            assert (d[0, 0] == 0.0 and c[0] >= 1e6 * _r(cost["weight"]) * 0.99) if still else True, name
            rim = d[1 if still else 0:][:4, 0] / safety - 1.0
            np.testing.assert_allclose(rim, [-RIM, RIM, -RIM, RIM], atol=2e-6, err_msg=str(name))
    return s, a, cost
