"""References, error rule and case tables for what csrc/mppi_cb.hip gained after tests/callback_checks.py was written: the
models "racecar" (test/test_mppi_racecar.py:13-30), "racecar_dynamic" (test/test_torch_mppi_race_car.py:7-39) and
"double_integrator" (test/test_torch_mppi.py:5-15), the terminal state cost, the options `noise_mu`, `u_scale`,
`noise_abs_cost` and `u_per_command`, the perturbed actions and the rank that orders the cheapest samples.  TEST
INFRASTRUCTURE, no device import: tests/test_callback_models_cases.py checks these functions and tables on the CPU,
tests/test_gpu_callback_models.py holds the kernels to them, tools/callback_models_report.py collects the figures the tests print.

PARITY UNPINNED as in callback_checks.py: the reference is the restated algorithm carried out in f64 on inputs rounded to f32
(`cc.rounded`), with `math.fsum` for the sums over T; the covariance is factored and inverted in f64 and then cast.

The error rule (no tolerance is fixed by hand).  There is no a-priori model for tan, atan2 and T steps that feed each other, so
every comparison follows the measured-ratio rule of callback_checks.py: next to the f64 definition stands an UNCHANGED f32
NumPy restatement of the same formula, evaluated on the same inputs, and the device is entitled to

    |device - f64|  <=  max(COST_FACTOR * dist32 * scale,  ulp_f32(largest term))         per element,
    dist32 = max over the elements of |restatement - f64| / scale,

COST_FACTOR = cc.COST_FACTOR = 4: the device sums in another order, contracts a * b + c into one rounding and uses other
sin / cos / tan / atan2 / exp / sqrt than NumPy.  `scale` is max(|f64 value|, 1) for cost_total (cc.cost_distance) and the
largest term's magnitude for a model's output; the floor of one f32 ulp of the largest term keeps a restatement that happens
to land exactly from making the bound zero.  The value returned is itself the last sum's result and counts among the terms:
where the summands add up past a power of two (41.4 + ... = 80.9 in the one-row case of the dynamic race car's running cost,
on which the restatement lands within 0.14 * 2^-24) its ulp is the larger one, and no f32 evaluation can be held to a step
finer than that of the number it returns.  `held` returns the ratio device distance / restatement distance that every test
prints; a ratio above cc.COST_RATIO_FINDING = 16 is a defect to explain.

START STATES.  They come from a scan on the CPU (three seeds, K in {255, 256, 257}, T in {7, 25, 50}, nominal sequences of
cc.NOMINAL_SHARE of the bounds, the scripts' Sigma and bounds):
  racecar          (5.6, 4.1, 0.9, 1.0): every sample enters an obstacle's safety distance; samples within cc.STEP_MARGIN of
                   the rim at some step are 0.8 - 2.0 % at T = 7, 1.6 - 2.7 % at T = 25 and 4.7 - 7.8 % at T = 50, so the
                   racecar cases use T <= 25 and stay under cc.EXCLUDED_CAP.
  racecar_dynamic  (3.6, 3.9, 0.2, 3.0): v cos(delta) stays >= 2.45 over 50 steps, atan2 never comes near its branch cut and
                   no sample is left out for it.
MOVED, as the conditions of `check_case` asked (the scan above had small nominal sequences and T >= 7 only):
  racecar, family "clamp"  (5.6, 4.12, 0.9, 1.0).  With the scan's state the clamp family's nominal sequence, which all samples
                   share up to their noise, puts a step within cc.STEP_MARGIN of the first obstacle's rim for a fifth of
                   the samples (48 - 72 of 256 over six seeds); 2 cm further on none is.  Its K > 1 cases stay at T <= 7: at
                   T = 25 that nominal sequence drives through the obstacle's centre, where 1 / d makes the f32 restatement
                   itself 4e-5 .. 1e-3 away from f64, beyond what the error rule assumes of it.
  racecar, T = 1   (5.6, 4.35, 0.9, 1.0): one step from the scan's state ends 0.94 from the obstacle and no sample is active;
                   from here every sample is inside (d = 0.72 .. 0.76).
  racecar_dynamic  keeps its bounds at T = 25: without them 6425 draws of sigma = 0.32 reach |delta| = 1.25 and v cos(delta)
                   falls to 0.94, below V_COS_FLOOR.
"""
from __future__ import annotations

import math

import numpy as np

import callback_checks as cc
from oracle import mppi_cb_oracle as cbo

F = np.float32
EPS = cc.EPS
NX = {"racecar": 4, "racecar_dynamic": 4, "double_integrator": 2}
NU = {"racecar": 2, "racecar_dynamic": 2, "double_integrator": 1}
DT = {"racecar": 0.05, "racecar_dynamic": 0.05, "double_integrator": 0.1}
DYN_ID = {"racecar": 2, "racecar_dynamic": 3, "double_integrator": 4}
# the scripts' constants (callback_mppi.MODEL_PARAMS), noise covariances and bounds
MODEL = {"racecar": dict(L=0.3), "racecar_dynamic": dict(lr=1.5, lf=1.0, m=1000.0, Cf=1000.0, Cr=1000.0), "double_integrator": {}}
SIGMA = {"racecar": np.diag([0.05, 0.05]),           # test/test_mppi_racecar.py:169
         "racecar_dynamic": 0.1 * np.eye(2),         # test/test_torch_mppi_race_car.py:71
         "double_integrator": np.array([[0.5]])}     # test/test_torch_mppi.py:33 (one control)
U_MAX = {"racecar": np.array([0.5, 1.0]),            # test/test_mppi_racecar.py:172-173
         "racecar_dynamic": np.array([1.0, 0.5]),    # test/test_torch_mppi_race_car.py:69-70
         "double_integrator": np.array([2.0])}       # test/test_torch_mppi.py:40
COSTS = {
    "racecar": dict(goal=[6.0, 5.0, 0.0, 0.0], q=[50.0, 35.0, 90.0, 0.1], r=[0.1, 0.1],
                    obstacles=[[6.0, 5.0, 0, 0], [7.0, 3.0, 0, 0]], safety=0.8, weight=10.0, kind="inverse"),
    "racecar_dynamic": dict(goal=[5.0, 5.0, 1.57, 1.0], q=[10.0, 5.0, 9.0, 1.0], r=[1.0, 10.0],
                            obstacles=[[5.0, 5.0, 0, 0], [7.0, 3.0, 0, 0]], safety=0.0, weight=1.0, kind="exponential"),
    "double_integrator": dict(goal=[0.0, 0.0], q=[1.0, 1.0], r=[1.0], obstacles=[], safety=0.0, weight=0.0, kind="inverse"),
}
TERMINAL = {"double_integrator": dict(goal=[0.0, 0.0], q=[1.0, 1.0]),        # test/test_torch_mppi.py:23-25
            # no caller has one for the race cars: a goal and weights of the running cost's size, so that the term is neither
            # negligible next to the running costs nor all of them
            "racecar": dict(goal=[6.0, 5.0, 0.0, 0.0], q=[500.0, 350.0, 900.0, 1.0]),
            "racecar_dynamic": dict(goal=[5.0, 5.0, 1.57, 1.0], q=[100.0, 50.0, 90.0, 10.0])}
RACECAR_CLAMP_START, RACECAR_T1_START = (5.6, 4.12, 0.9, 1.0), (5.6, 4.35, 0.9, 1.0)  # (MOVED, see the module docstring)
START = {"racecar": (5.6, 4.1, 0.9, 1.0), "racecar_dynamic": (3.6, 3.9, 0.2, 3.0), "double_integrator": (1.0, 0.0)}
V_COS_FLOOR = 1.0  # dynamic cases: v cos(delta) at every step of every sample


def cost_of(dyn):
    c = {k: (np.asarray(v, np.float64) if k not in ("kind", "safety", "weight") else v) for k, v in COSTS[dyn].items()}
    c["obstacles"] = c["obstacles"].reshape(-1, 4)
    return c


# ------------------------------------------------------------------------------------------------------------------
# the three models: f64 definition and f32 restatement
# ------------------------------------------------------------------------------------------------------------------
def dynamics(dyn, s, u, dt, inputs_f32=True, swap_controls=False):
    """One Euler step in f64, every component from the OLD state.  Returns (next[n, nx], largest[n, nx]): the new state and the
    magnitude of the largest term that went into each component.  ``swap_controls``: the racecar with its two controls read
    in the other order (the deliberate break the GPU file is run against once)."""
    s, u = (cc.rounded(s), cc.rounded(u)) if inputs_f32 else (np.asarray(s, np.float64), np.asarray(u, np.float64))
    dt, p = cc._r(dt), {k: cc._r(v) for k, v in MODEL[dyn].items()}
    if dyn == "double_integrator":
        inc = np.stack([dt * s[:, 1], dt * u[:, 0]], axis=1)
        return s + inc, np.maximum(np.abs(s), np.abs(inc))
    x, y, th, v = s.T
    if dyn == "racecar":
        delta, a = (u[:, 1], u[:, 0]) if swap_controls else (u[:, 0], u[:, 1])
        inc = np.stack([v * np.cos(th) * dt, v * np.sin(th) * dt, v / p["L"] * np.tan(delta) * dt, a * dt], axis=1)
        return s + inc, np.maximum(np.abs(s), np.abs(inc))
    acc, delta = u[:, 0], u[:, 1]
    sd, cd = np.sin(delta), np.cos(delta)
    af = np.arctan2(v * sd + p["lf"] * th, v * cd) - delta
    ar = np.arctan2(v * sd - p["lr"] * th, v * cd)
    ff, fr = p["Cf"] * af * sd / p["m"], p["Cr"] * ar / p["m"]
    inc = np.stack([v * np.cos(th) * dt, v * np.sin(th) * dt, (v / p["lr"]) * sd * dt, (acc - (ff + fr)) * dt], axis=1)
    largest = np.maximum(np.abs(s), np.abs(inc))
    largest[:, 3] = np.maximum(largest[:, 3], dt * np.maximum(np.abs(acc), np.maximum(np.abs(ff), np.abs(fr))))
    return s + inc, largest


def dynamics32(dyn, s, u, dt):
    """The same step in f32 NumPy, operation by operation as the scripts write it."""
    s, u, dt = np.asarray(s, F), np.asarray(u, F), F(dt)
    p = {k: F(v) for k, v in MODEL[dyn].items()}
    if dyn == "double_integrator":
        return np.stack([s[:, 0] + dt * s[:, 1], s[:, 1] + dt * u[:, 0]], axis=1).astype(F)
    x, y, th, v = s.T
    if dyn == "racecar":
        delta, a = u[:, 0], u[:, 1]
        return np.stack([x + v * np.cos(th) * dt, y + v * np.sin(th) * dt, th + v / p["L"] * np.tan(delta) * dt, v + a * dt],
                        axis=1).astype(F)
    acc, delta = u[:, 0], u[:, 1]
    af = np.arctan2(v * np.sin(delta) + p["lf"] * th, v * np.cos(delta)) - delta
    ar = np.arctan2(v * np.sin(delta) - p["lr"] * th, v * np.cos(delta))
    fyf, fyr = p["Cf"] * af, p["Cr"] * ar
    return np.stack([x + v * np.cos(th) * dt, y + v * np.sin(th) * dt, th + (v / p["lr"]) * np.sin(delta) * dt,
                     v + (acc - (fyf * np.sin(delta) + fyr) / p["m"]) * dt], axis=1).astype(F)


def terminal_cost(s, term, inputs_f32=True):
    """(c[n], largest[n]) of (s - goal)^T diag(q) (s - goal) in f64."""
    s = cc.rounded(s) if inputs_f32 else np.asarray(s, np.float64)
    nx = s.shape[1]
    terms = cc.rounded(term["q"])[:nx] * (s - cc.rounded(term["goal"])[:nx]) ** 2
    return np.array([math.fsum(r) for r in terms]), np.abs(terms).max(1)


def terminal_cost32(s, term):
    s = np.asarray(s, F)
    e = s - np.asarray(term["goal"], F)[:s.shape[1]]
    return (np.asarray(term["q"], F)[:s.shape[1]] * e * e).sum(1).astype(F)


def cost_largest(s, u, t, cost):
    """The magnitude of the largest term of the running cost per row: the quadratic terms and the weighted obstacle terms."""
    _, _, d = cc.running_cost(s, u, t, cost)
    s, u = cc.rounded(s), cc.rounded(u)
    terms = [cc.rounded(cost["q"])[:s.shape[1]] * (s - cc.rounded(cost["goal"])[:s.shape[1]]) ** 2,
             cc.rounded(cost["r"])[:u.shape[1]] * u * u]
    if d.shape[1]:
        safety, w = cc._r(cost["safety"]), cc._r(cost["weight"])
        terms.append(abs(w) * (np.where(d < safety, 1.0 / (d + cc._r(1e-6)), 0.0) if cost["kind"] == "inverse"
                               else np.exp(-(d - safety))))
    return np.concatenate(terms, axis=1).max(1)


def held(got, want, rst, scale, largest):
    """The error rule of the module docstring.  Returns (ratio, ok): device distance / restatement distance (inf where the
    restatement is exact and the device is not) and whether every element is inside max(COST_FACTOR * dist32 * scale, one f32
    ulp of the largest term, the value itself included)."""
    got, want, rst = (np.asarray(a, np.float64) for a in (got, want, rst))
    scale = np.broadcast_to(np.asarray(scale, np.float64), want.shape)
    floor = np.spacing(np.maximum(np.abs(want), np.abs(np.asarray(largest, np.float64))).astype(F)).astype(np.float64)
    if want.size == 0:
        return 0.0, True
    dist32 = float(np.max(np.abs(rst - want) / scale))
    err = np.abs(got - want)
    dev = float(np.max(err / scale))
    ok = bool(np.isfinite(got).all() and (err <= np.maximum(cc.COST_FACTOR * dist32 * scale, floor)).all())
    return (dev / dist32 if dist32 > 0 else (0.0 if dev == 0 else math.inf)), ok


# ------------------------------------------------------------------------------------------------------------------
# the rank that orders the cheapest samples
# ------------------------------------------------------------------------------------------------------------------
def ranks(c):
    """rank[k] = number of samples j with c_j < c_k, or c_j == c_k and j < k; a NaN counts as larger than every number and
    NaNs are ordered among themselves by index.  A permutation of 0 .. K - 1 whatever ``c`` holds."""
    c = np.asarray(c, np.float64)
    j = np.arange(c.size)
    nan = np.isnan(c)
    with np.errstate(invalid="ignore"):
        less, eq = c[:, None] < c[None, :], c[:, None] == c[None, :]
    lower = j[:, None] < j[None, :]
    before = np.where(nan[:, None] & nan[None, :], lower, np.where(nan[None, :], True, np.where(nan[:, None], False,
                                                                                               less | (eq & lower))))
    return before.sum(0)


def cheapest(c, n):
    """The indices of the n samples of lowest rank, in ascending order of rank."""
    r = ranks(c)
    order = np.empty(r.size, np.int64)
    order[r] = np.arange(r.size)
    return order[:n]


# ------------------------------------------------------------------------------------------------------------------
# the whole command with the new terms: f64 definition and f32 restatement
# ------------------------------------------------------------------------------------------------------------------
def clamped(case, U, noise, do_shift=True, actions=None):
    """(U after the shift, the clamped UNSCALED actions [K, T, nu], the noise taken back from them), as cc.clamped_noise.
    ``actions``: the clamped actions themselves in place of a draw (what `perturbed_action` returned after an in-kernel draw)."""
    K, T, nu = case["K"], case["T"], NU[case["dyn"]]
    U = cc.rounded(U).reshape(T, nu)
    if do_shift:
        U = cc.shift(U, case["u_init"])
    if actions is not None:
        act = cc.rounded(actions).reshape(K, T, nu)
        return U, act, act - U[None]
    act = U[None] + cc.rounded(noise).reshape(K, T, nu)
    if case["null"]:
        act[K - 1] = 0.0
    act = np.clip(act, cc.rounded(case["u_min"]), cc.rounded(case["u_max"]))
    return U, act, act - U[None]


def rollout(dyn, state, actions, dt, **kw):
    """traj[n, T, nx] in f64 of the action sequences ``actions`` [n, T, nu] (as given) from ``state`` (rounded to f32)."""
    n, T = actions.shape[:2]
    s = np.tile(cc.rounded(state), (n, 1))
    out = np.zeros((n, T, s.shape[1]))
    for t in range(T):
        s, _ = dynamics(dyn, s, actions[:, t], dt, inputs_f32=False, **kw)
        out[:, t] = s
    return out


def rollout32(dyn, state, actions, dt):
    actions = np.asarray(actions, F)
    n, T = actions.shape[:2]
    s = np.tile(np.asarray(state, F), (n, 1))
    out = np.zeros((n, T, s.shape[1]), F)
    for t in range(T):
        s = dynamics32(dyn, s, actions[:, t], dt)
        out[:, t] = s
    return out


def command(case, state, U, noise, do_shift=True, swap_controls=False, terminal_before_last=False, actions=None):
    """One `command` in f64 with the terms a case may switch on: ``terminal`` (dict(goal, q) or None), ``u_scale``,
    ``abs_cost``.  ``noise`` is the whole draw (an in-kernel draw with `noise_mu` is mu + L z, formed by the caller).
    Returns what cc.command returns, and terminal[K], v_cos[K] (the smallest v cos(delta) over the steps, dynamic model),
    largest[K] (the largest of |running|, |terminal|, |pert|).  The two keyword breaks restate the deliberately broken builds."""
    dyn, cost, lam, dt = case["dyn"], case["cost"], cc._r(case["lam"]), case["dt"]
    K, T = case["K"], case["T"]
    scale = cc._r(case.get("u_scale", 1.0))
    U, act, nz = clamped(case, U, noise, do_shift, actions)
    _, sinv = cc.factor(case["sigma"])
    s = np.tile(cc.rounded(state), (K, 1))
    per_step = np.zeros((T, K))
    margin, active, v_cos = np.full(K, np.inf), np.zeros(K, bool), np.full(K, np.inf)
    s_before = s
    for t in range(T):
        a = scale * act[:, t]
        if dyn == "racecar_dynamic":
            v_cos = np.minimum(v_cos, s[:, 3] * np.cos(a[:, 1]))
        s_before = s
        s, _ = dynamics(dyn, s, a, dt, inputs_f32=False, swap_controls=swap_controls)
        per_step[t], _, d = cc.running_cost(s, a, t, cost, inputs_f32=False)
        margin = np.minimum(margin, cc.step_margin(d, cost))
        if cost["kind"] == "inverse" and d.shape[1]:
            active |= (d < cc._r(cost["safety"])).any(1)
    running = np.array([math.fsum(per_step[:, k]) for k in range(K)])
    term = np.zeros(K)
    if case.get("terminal") is not None:
        term, _ = terminal_cost(s_before if terminal_before_last else s, case["terminal"], inputs_f32=False)
    npert = np.abs(nz) if case.get("abs_cost") else nz
    pterm = (U[None] * lam * (npert @ sinv)).reshape(K, -1)
    pert = np.array([math.fsum(row) for row in pterm])
    total = running + term + pert
    omega, x = cc.softmin(total, lam)
    U_new, _ = cc.update(U, omega, nz)
    return dict(U_shifted=U, act=act, noise=nz, running=running, terminal=term, pert=pert, cost_total=total, omega=omega, x=x,
                U_new=U_new, action=U_new[0].copy(), margin=margin, active=active, keep=margin >= cc.STEP_MARGIN, v_cos=v_cos,
                largest=np.maximum(np.abs(running), np.maximum(np.abs(term), np.abs(pert))))


def restatement(case, state, U, noise, do_shift=True, actions=None):
    """The same command in f32 NumPy, arranged as oracle/mppi_cb_oracle.py arranges the loop (whose running cost it calls).
    Returns dict(cost_total, omega, U, act)."""
    dyn, cost = case["dyn"], case["cost"]
    K, T, nu = case["K"], case["T"], NU[dyn]
    kw = dict(goal=cost["goal"], q_diag=cost["q"], r_diag=cost["r"], obstacles=cost["obstacles"], safety=cost["safety"],
              weight=cost["weight"], kind=cost["kind"])
    lam, scale = F(case["lam"]), F(case.get("u_scale", 1.0))
    U = np.asarray(U, F).reshape(T, nu).copy()
    if do_shift:
        U = np.vstack([U[1:], np.asarray(case["u_init"], F)[None]]).astype(F)
    if actions is None:
        act = U[None] + np.asarray(noise, F).reshape(K, T, nu)
        if case["null"]:
            act[K - 1] = 0
        act = np.clip(act, np.asarray(case["u_min"], F), np.asarray(case["u_max"], F)).astype(F)
    else:
        act = np.asarray(actions, F).reshape(K, T, nu)
    nz = act - U[None]
    npert = np.abs(nz) if case.get("abs_cost") else nz
    action_cost = lam * npert @ np.linalg.inv(np.asarray(case["sigma"], np.float64)).astype(F)
    s = np.tile(np.asarray(state, F), (K, 1))
    c = np.zeros(K, F)
    for t in range(T):
        a = (scale * act[:, t]).astype(F)
        s = dynamics32(dyn, s, a, case["dt"])
        c += cbo.running_cost(s, a, t, **kw)
    if case.get("terminal") is not None:
        c = c + terminal_cost32(s, case["terminal"])
    c = (c + (U[None] * action_cost).sum(axis=(1, 2))).astype(F)
    w = np.exp(-(c - c.min()) / lam)
    w = w / w.sum()
    return dict(cost_total=c, omega=w, U=(U + (w[:, None, None] * nz).sum(0)).astype(F), act=act)


def cost_held(got, ref, rst):
    """`held` for cost_total over the kept samples: scale max(|c64|, 1) as cc.cost_distance, floor one ulp of the largest of
    the sample's three summands."""
    k = ref["keep"]
    return held(np.asarray(got)[k], ref["cost_total"][k], np.asarray(rst, np.float64)[k], np.maximum(np.abs(ref["cost_total"][k]), 1.0),
                ref["largest"][k])


# ------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20250930] + [int(k) for k in key])


def _case(name, family, dyn, K, T, null=False, bounded=True, terminal=False, u_init=None, seed=0, state=None, **options):
    """family "clamp": lambda = 1 (the callers' regime) and a nominal sequence that sits half a standard deviation inside a
    bound on every third entry, so the clamp binds there; family "spread": a nominal sequence of cc.NOMINAL_SHARE of the bounds
    and lambda = std of the running costs (`_spread`)."""
    nu, lim = NU[dyn], U_MAX[dyn]
    c = dict(name=name, family=family, dyn=dyn, cost=cost_of(dyn), K=K, T=T, dt=DT[dyn], sigma=SIGMA[dyn], null=null, lam=1.0,
             state=np.asarray(START[dyn] if state is None else state, np.float64), bounded=bounded, lim=lim,
             u_min=-lim if bounded else np.full(nu, -1e30), u_max=lim if bounded else np.full(nu, 1e30),
             u_init=np.zeros(nu) if u_init is None else np.asarray(u_init, np.float64), seed=seed,
             terminal=TERMINAL[dyn] if terminal else None, u_scale=1.0, abs_cost=False)
    c.update(options)
    rng = _rng(K, T, nu, seed, 0 if family == "clamp" else 1, DYN_ID[dyn])
    L = np.linalg.cholesky(c["sigma"])
    c["noise"] = (rng.normal(size=(K, T, nu)) @ L.T).astype(F)
    sd = np.sqrt(np.diag(c["sigma"]))
    if family == "clamp":
        U = rng.uniform(-1.0, 1.0, (T, nu)) * cc.NOMINAL_SHARE * lim
        idx = np.arange(T * nu).reshape(T, nu)
        edge = (lim - 0.5 * sd)[None, :] * np.where(idx % 2 == 0, 1.0, -1.0)
        U = np.where(idx % 3 == 0, edge, U)
    else:
        U = rng.uniform(-1.0, 1.0, (T, nu)) * np.minimum(cc.NOMINAL_SHARE * lim, cc.nominal_amplitude(c["sigma"], T, np.inf))
    c["U"] = U.astype(F)
    return c


def _spread(case):
    ref = command(dict(case, lam=1.0), case["state"], case["U"], case["noise"])
    case["lam"] = cc._r(np.std(ref["running"] + ref["terminal"])) if case["K"] > 1 else 1.0
    return case


OPTION_BASE = "spread-racecar-K257-T25"   # the one racecar case the options are switched on
OPTION_MU = np.array([0.08, -0.15])       # noise_mu of the option cases: a third to two thirds of a standard deviation
OPTION_SCALE = 0.5
_CASES = None


def cases():
    """Every command case: K in {1, 255, 256, 257}, T in {1, 7, 25} and T * nu = 256 (128 for the dynamic race car, whose
    exponential cost leaves no sample out, and 256 for the double integrator; the racecar stays at T <= 25, see START STATES),
    each model
    with the null action, without bounds, with a non-zero u_init and with a terminal cost."""
    global _CASES
    if _CASES is None:
        cl = [
            _case("racecar-K1-T25", "clamp", "racecar", 1, 25, state=RACECAR_CLAMP_START),
            _case("racecar-K255-T1-null", "clamp", "racecar", 255, 1, null=True, u_init=[0.35, -0.1], state=RACECAR_T1_START),
            _case("racecar-K256-T7-free", "clamp", "racecar", 256, 7, bounded=False, state=RACECAR_CLAMP_START),
            _case("racecar-K257-T7-term", "clamp", "racecar", 257, 7, terminal=True, u_init=[-0.1, 0.3], state=RACECAR_CLAMP_START),
            _case("dynamic-K1-T7-free", "clamp", "racecar_dynamic", 1, 7, bounded=False),
            _case("dynamic-K255-T7-null", "clamp", "racecar_dynamic", 255, 7, null=True, u_init=[0.3, -0.2]),
            _case("dynamic-K257-T25-term", "clamp", "racecar_dynamic", 257, 25, terminal=True),
            _case("dynamic-K256-T128", "clamp", "racecar_dynamic", 256, 128),
            _case("double-K1-T7-term", "clamp", "double_integrator", 1, 7, terminal=True),
            _case("double-K257-T256-term", "clamp", "double_integrator", 257, 256, terminal=True, u_init=[0.5]),
            _case("double-K256-T25-free-null", "clamp", "double_integrator", 256, 25, bounded=False, null=True),
        ]
        sp = [
            _case(OPTION_BASE, "spread", "racecar", 257, 25),
            _case("spread-racecar-K255-T25-term", "spread", "racecar", 255, 25, terminal=True),
            _case("spread-racecar-K256-T7-null", "spread", "racecar", 256, 7, null=True),
            _case("spread-dynamic-K257-T25", "spread", "racecar_dynamic", 257, 25),
            _case("spread-dynamic-K255-T1", "spread", "racecar_dynamic", 255, 1),
            _case("spread-double-K255-T25-term", "spread", "double_integrator", 255, 25, terminal=True),
            _case("spread-double-K256-T1", "spread", "double_integrator", 256, 1, null=True),
        ]
        base = next(c for c in sp if c["name"] == OPTION_BASE)
        _CASES = {c["name"]: c for c in cl + [_spread(c) for c in sp]}
        # the options, each alone and all together, on the one racecar case (lambda stays the base case's)
        for name, opt in (("option-abs", dict(abs_cost=True)), ("option-scale", dict(u_scale=OPTION_SCALE)),
                          ("option-terminal", dict(terminal=TERMINAL["racecar"])),
                          ("option-all", dict(abs_cost=True, u_scale=OPTION_SCALE, terminal=TERMINAL["racecar"]))):
            _CASES[name] = dict(base, name=name, family="option", **opt)
    return _CASES


_REFS = {}


def reference(name):
    """(f64 reference, f32 restatement) of a case: computed once, shared, not to be modified."""
    if name not in _REFS:
        c = cases()[name]
        _REFS[name] = (command(c, c["state"], c["U"], c["noise"]), restatement(c, c["state"], c["U"], c["noise"]))
    return _REFS[name]


def restatement_distance(name):
    ref, rst = reference(name)
    return cc.cost_distance(rst["cost_total"], ref["cost_total"], ref["keep"])


def check_case(name):
    """The conditions a case states, from the references alone.  Raises AssertionError with the case's name."""
    c = cases()[name]
    ref, rst = reference(name)
    K, T = c["K"], c["T"]
    assert T * NU[c["dyn"]] <= 256, name
    left_out = int((~ref["keep"]).sum())
    assert left_out <= cc.EXCLUDED_CAP * K, (name, left_out)
    if c["cost"]["kind"] == "inverse" and len(c["cost"]["obstacles"]):
        kept_active = int((ref["active"] & ref["keep"]).sum())
        assert kept_active >= cc.ACTIVE_FLOOR * int(ref["keep"].sum()), (name, kept_active)
    else:
        assert left_out == 0, name
    if c["dyn"] == "racecar_dynamic":
        assert ref["v_cos"].min() >= V_COS_FLOOR, (name, ref["v_cos"].min())
    # an honest f32 evaluation and not an exact one: within 16 roundings a step of the cost's magnitude (the level the error
    # rule assumes of the restatement, as cc.check_case asks of the existing models)
    dist = restatement_distance(name)
    assert np.isfinite(ref["cost_total"]).all() and 0 < dist <= 16 * T * EPS, (name, dist)
    raw = ref["U_shifted"][None] + cc.rounded(c["noise"])
    if c["null"]:
        raw[K - 1] = 0.0
    bind = raw != ref["act"]
    if c["family"] == "clamp":
        assert c["lam"] == 1.0, name
        if c["bounded"] and K > 1:
            per_entry = bind.mean(0)
            assert (per_entry > 0.1).any() and (per_entry == 0).any(), name
        elif not c["bounded"]:
            assert not bind.any(), name
    elif K > 1:
        assert np.abs(ref["U_shifted"]).max() <= (cc.NOMINAL_SHARE * c["lim"]).max() * (1 + 1e-6), name
        assert cc.ess(ref["omega"]) >= cc.ESS_FLOOR * K, (name, cc.ess(ref["omega"]))
        assert cc.ess(ref["omega"]) <= 0.9 * K, (name, cc.ess(ref["omega"]))


def term_moves_the_cost(base_name, **change):
    """The share of the kept samples of ``base_name`` whose f64 cost_total moves by more than ten times the GPU test's
    tolerance (COST_FACTOR * restatement distance * scale) when the case is changed by ``change`` (a case field, or
    ``noise=`` for another draw)."""
    c = cases()[base_name]
    ref, _ = reference(base_name)
    noise = change.pop("noise", c["noise"])
    other = command(dict(c, **change), c["state"], c["U"], noise)
    k = ref["keep"] & other["keep"]
    tol = cc.COST_FACTOR * restatement_distance(base_name) * np.maximum(np.abs(ref["cost_total"]), 1.0)
    return float((np.abs(other["cost_total"] - ref["cost_total"])[k] > 10.0 * tol[k]).mean())


# ------------------------------------------------------------------------------------------------------------------
# the models alone: rows for mppi_cb_eval
# ------------------------------------------------------------------------------------------------------------------
MODEL_N = (1, 255, 256, 257)


def model_rows(dyn, n):
    """(states[n, nx], actions[n, nu]) for `_dynamics` / `_running_cost` / `_terminal_cost`: random rows around the start state,
    controls inside the script's bounds and up to twice beyond, headings up to 1e3 for the kinematic racecar; the dynamic model
    keeps |theta| <= 3 and v in [1.5, 6], so that v cos(delta) >= V_COS_FLOOR with |delta| <= 0.8 and atan2 stays off its cut."""
    nx, nu = NX[dyn], NU[dyn]
    rng = _rng(n, nx, nu, DYN_ID[dyn], 7)
    s = np.asarray(START[dyn]) + rng.normal(0, 1.0, (n, nx))
    a = rng.uniform(-2.0, 2.0, (n, nu)) * U_MAX[dyn]
    if dyn == "racecar":
        s[:, 2] = rng.uniform(-1e3, 1e3, n)
        if n > 1:
            s[n // 2, 2], s[n - 1, 2] = 1e3, -1e3
        s[:, 3] = rng.uniform(-3.0, 6.0, n)
    elif dyn == "racecar_dynamic":
        s[:, 2] = rng.uniform(-3.0, 3.0, n)
        s[:, 3] = rng.uniform(1.5, 6.0, n)
        a[:, 1] = rng.uniform(-0.8, 0.8, n)
    if dyn != "double_integrator" and n >= 8:  # rows inside the first obstacle's safety distance (the racecar's inverse cost)
        ox, oy = COSTS[dyn]["obstacles"][0][:2]
        for row in range(8):
            rad, ang = rng.uniform(0.05, 0.75), rng.uniform(0, 2 * math.pi)
            s[row, 0], s[row, 1] = ox + rad * math.cos(ang), oy + rad * math.sin(ang)
    return s.astype(F), a.astype(F)
