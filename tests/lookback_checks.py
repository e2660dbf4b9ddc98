"""What the one-launch resolution of the sequential waypoint index must do on a given input, predicted on the CPU from the
oracle's rollout, and the inputs of tests/test_gpu_lookback.py.  TEST INFRASTRUCTURE: tests/test_lookback_cases.py checks without
a device that every case is what it claims to be (predicted good or bad, for which reason, how far from a tie),
tests/test_gpu_lookback.py runs the cases.

The prediction restates pass A of the kernels (lb_scan: a call's descents over the 32 candidates behind c) and lb_reach in
NumPy f64 (prims_checks.lb_scan_reference / lb_reach_reference, the references of the unit tests).  It does not depend on how
the samples are laid out over workgroups: lb_reach is monotone in `leave` and every workgroup's max(E, own) is a prefix
maximum, so "some word is marked" <=> a call is not unimodal, or the largest offset of all calls is out of reach.
"""
from __future__ import annotations

import numpy as np

import prims_checks as pc
from oracle import mppi_oracle

LB_CAND = pc.LB_CAND
WINDOW = {"numpy": 20, "cuda": 10}
GAP_FLOOR = 1e-10       # f64: the device's positions differ from NumPy's in the last bits; no descent bit can then differ
GAP_FLOOR_F32 = 1e-4    # f32 cases: positions carry about 1e-6; the cases chosen stay far from it
WG_SAMPLES = {"0": 16, "1": 32}  # MPPI_DUAL: samples per workgroup


def lookback_prediction(X, ref_path, c, W):
    """X: the oracle's rollout [K][T][>= 2]; the T stage calls and the terminal call (the last state again) of every sample.
    Returns m[K] (the largest offset of the sample's calls), nonunimodal[K], any_nonunimodal, reach (of the largest offset of
    all), bad (what the kernels must conclude), gap (the smallest relative gap between consecutive candidate distances)."""
    X = np.asarray(X)
    K, T = X.shape[:2]
    n_ref = ref_path.shape[0]
    nc = min(LB_CAND, n_ref - c)
    cand = np.full((LB_CAND, 2), pc.LB_ABSENT)
    cand[:nc] = np.asarray(ref_path, np.float64)[c:c + nc, :2]
    pos = np.concatenate([X[:, :, :2], X[:, -1:, :2]], axis=1).reshape(-1, 2).astype(np.float64)
    m, bad, g, gap = pc.lb_scan_reference(cand, pos)
    m_k, bad_k = m.reshape(K, T + 1).max(axis=1), bad.reshape(K, T + 1).any(axis=1)
    reach = pc.lb_reach_reference(int(m_k.max()), W, n_ref, c)
    return {"m": m_k, "nonunimodal": bad_k, "any_nonunimodal": bool(bad_k.any()), "reach": reach,
            "bad": bool(bad_k.any() or not reach), "gap": float(gap.min()), "bits": g}


def in_play(T, W, n_ref, c, path_end):
    """the look-back serves the iteration (the kernel name must then end ', true>')"""
    return T <= 64 and min(W, n_ref - c) > 1 and not path_end


def workgroup_maxima(m, per_wg):
    return np.array([m[i:i + per_wg].max() for i in range(0, m.size, per_wg)])


def e_decides_and_own_decides(m, per_wg):
    """(a workgroup b > 0 whose own largest offset is below that of the workgroups before it, one whose own is above)"""
    M = workgroup_maxima(m, per_wg)
    before = np.maximum.accumulate(M)[:-1]
    return bool((M[1:] < before).any()), bool((M[1:] > before).any())


def rollout_f32(o, x0, eps):
    """the oracle's rollout in float32 throughout: what a float handle's positions look like"""
    f = np.float32
    K, T = o.K, o.T
    thr = mppi_oracle.exploit_threshold(o.param_exploration, K)
    u = o.u_prev.astype(f)
    e = np.asarray(eps, f)
    v = np.where((np.arange(K) < thr)[:, None, None], u[None] + e, e)
    v[..., 0] = np.clip(v[..., 0], f(-o.max_speed), f(o.max_speed))
    v[..., 1] = np.clip(v[..., 1], f(-o.max_omega), f(o.max_omega))
    dt = f(o.delta_t)
    x, y, yaw = (np.full(K, f(x0[i]), f) for i in range(3))
    X = np.empty((K, T, 3), f)
    for t in range(T):
        x, y, yaw = x + v[:, t, 0] * np.cos(yaw) * dt, y + v[:, t, 0] * np.sin(yaw) * dt, yaw + v[:, t, 1] * dt
        X[:, t, 0], X[:, t, 1], X[:, t, 2] = x, y, yaw
    return X


# ------------------------------------------------------------------------------------------ paths
def _with_yaw(xy):
    xy = np.asarray(xy, np.float64)
    d = np.gradient(xy, axis=0)
    return np.column_stack([xy, np.arctan2(d[:, 1], d[:, 0])])


def arc_path(n, spacing, radius):
    a = spacing * np.arange(n) / radius
    return _with_yaw(np.stack([radius * np.sin(a), radius * (1.0 - np.cos(a))], 1))


def line_path(n, spacing, slope=-0.35):
    s = spacing * np.arange(n) / np.hypot(1.0, slope)
    return _with_yaw(np.stack([s, slope * s], 1))


def hairpin_path(spacing=0.1, leg=13, sep=0.15, tail=40):
    """Out along +x for `leg` waypoints, back beside it `sep` apart, and on in -x.  Seen from beside the first leg, short of the
    turn, the distances fall, rise towards the turn and fall again along the way back: not unimodal.  Seen from beyond the turn
    they only rise."""
    out = np.stack([spacing * np.arange(leg), np.zeros(leg)], 1)
    back = np.stack([spacing * np.arange(leg - 1, -tail, -1.0), np.full(leg - 1 + tail, sep)], 1)
    return _with_yaw(np.concatenate([out, back]))


PATHS = {"arc12": lambda: arc_path(120, 0.1, 12.0), "arc5": lambda: arc_path(120, 0.08, -5.0), "line": lambda: line_path(120, 0.1)}


# ------------------------------------------------------------------------------------------ cases
def base_kwargs(ref, K, T, **over):
    kw = dict(delta_t=0.1, ref_path=ref, max_speed=3.0, max_omega=1.5, num_samples_K=K, num_horizons_T=T,
              param_exploration=0.1, param_lambda=5.0, param_alpha=0.9, sigma=np.array([[0.09, 0.0], [0.0, 0.04]]),
              stage_cost_weight=np.array([5.0, 5.0, 1.0]), terminal_cost_weight=np.array([8.0, 8.0, 2.0]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    kw.update(over)
    return kw


class Case:
    """One controller input: keyword arguments, start state, nominal controls, noise, variant, how many iterations."""

    def __init__(self, name, kw, x0, u_in, eps, variant="numpy", iters=1, prev_idx=0):
        self.name, self.kw, self.x0, self.u_in, self.eps = name, kw, np.asarray(x0, np.float64), u_in, eps
        self.variant, self.iters, self.prev_idx = variant, iters, prev_idx
        self.K, self.T = kw["num_samples_K"], kw["num_horizons_T"]
        self.W = WINDOW[variant]

    def oracle(self):
        o = mppi_oracle.DiffDriveOracle(**self.kw)
        if self.variant == "cuda":
            o.SEARCH_IDX_LEN, o.WRAP_YAW_TERMINAL = 10, True
        o.u_prev[:] = self.u_in
        o.prev_way_point_idx = self.prev_idx
        return o

    def run_oracle(self, f32_bits=False):
        """per iteration: (x0, the oracle's results, the prediction, in play); f32_bits: also whether a float rollout gives the
        same descent bits ("same_bits_f32") and its smallest gap ("gap_f32")"""
        o, x0, out = self.oracle(), self.x0.copy(), []
        n_ref = self.kw["ref_path"].shape[0]
        for _ in range(self.iters):
            u_before = o.u_prev.copy()
            ref = o.iteration(x0, self.eps.astype(np.float64))
            pred = lookback_prediction(ref["X"], self.kw["ref_path"], ref["idx_start"], self.W)
            if f32_bits:
                o32 = self.oracle()
                o32.u_prev[:] = u_before
                p32 = lookback_prediction(rollout_f32(o32, x0, self.eps), self.kw["ref_path"].astype(np.float32), ref["idx_start"],
                                          self.W)
                pred["same_bits_f32"] = bool(np.array_equal(p32["bits"], pred["bits"]))
                pred["gap_f32"] = p32["gap"]
            out.append((x0.copy(), ref, pred, in_play(self.T, self.W, n_ref, ref["idx_start"], ref["path_end"])))
            x0 = mppi_oracle.diffdrive_plant_step(x0, ref["u0_returned"], self.kw["delta_t"])
        return out


def _noise(seed, K, T, sigma):
    return (np.random.default_rng(seed).standard_normal((K, T, 2)) @ np.linalg.cholesky(sigma).T).astype(np.float32)


# (a) the look-back itself: paths spaced so that the samples carry the index 3 .. 9 waypoints on, differently per sample
GOOD_KT = [(53, 10), (53, 33), (53, 64), (129, 10), (129, 33), (129, 64), (200, 10), (200, 33), (200, 64)]
# (K, T) -> noise seed, picked on the CPU (tests/test_lookback_cases.py states what the cases satisfy)
GOOD_SEEDS = {(53, 10): 2, (53, 33): 3, (53, 64): 1, (129, 10): 1, (129, 33): 2, (129, 64): 1, (200, 10): 1, (200, 33): 2,
              (200, 64): 2}


def good_case(K, T, seed=None):
    i = GOOD_KT.index((K, T))
    pname = list(PATHS)[i % 3]
    variant = ("numpy", "cuda")[i % 2]
    ref = PATHS[pname]()
    spacing = float(np.hypot(*(ref[1, :2] - ref[0, :2])))
    dt = 0.1
    # five waypoints over the horizon and about two more or fewer per sample; the 10-candidate window reaches 9: 3.5 and 1.2
    ahead, spread = (5.0, 2.0) if variant == "numpy" else (3.5, 1.2)
    speed = ahead * spacing / (dt * T)
    s_speed = spread * spacing / (dt * np.sqrt(T))
    sigma = np.array([[s_speed ** 2, 0.0], [0.0, 0.02 ** 2]])
    kw = base_kwargs(ref, K, T, sigma=sigma, max_speed=speed + 6.0 * s_speed)
    start = 4
    x0 = np.array([ref[start, 0] + 0.01, ref[start, 1] - 0.02, ref[start, 2]])
    curv = (ref[start + 1, 2] - ref[start, 2]) / spacing
    u_in = np.column_stack([np.full(T, speed), np.full(T, speed * curv)])
    seed = GOOD_SEEDS.get((K, T), 0) if seed is None else seed
    return Case(f"{pname}-{variant}-K{K}-T{T}", kw, x0, u_in, _noise(seed, K, T, sigma), variant, iters=3, prev_idx=start - 2)


def good_cases():
    return [good_case(K, T) for K, T in GOOD_KT]


# (b) each cause alone
def hairpin_case(K=40, T=12, dual_k=None):
    """every sample beside the first leg, short of the turn: calls that are not unimodal, offsets within reach"""
    ref = hairpin_path()
    sigma = np.array([[0.05 ** 2, 0.0], [0.0, 0.05 ** 2]])
    kw = base_kwargs(ref, K, T, sigma=sigma, max_speed=1.0)
    u_in = np.column_stack([np.full(T, 0.1), np.zeros(T)])
    return Case("hairpin", kw, [0.85, -0.03, 0.0], u_in, _noise(3, K, T, sigma), "numpy")


def reach_case(variant="numpy"):
    """the dense path and the fast robot of test_one_launch_index_resolution_and_its_fallback: the index leaves the candidates"""
    K, T, n_ref = 200, 40, 400
    ref = mppi_oracle.generate_point_trajectory((0.0, 0.0), (8.0, -3.0), n_ref)
    sigma = np.array([[0.1, 0.0], [0.0, 0.01]])
    kw = base_kwargs(ref, K, T, sigma=sigma, max_speed=5.0)
    u_in = np.column_stack([np.full(T, 4.0), np.zeros(T)])
    x0 = ref[0, :3] + np.array([0.05, -0.03, 0.0])
    return Case(f"reach-{variant}", kw, x0, u_in, _noise(5, K, T, sigma), variant)


# (c) one offending sample: everyone waits beyond the turn of the hairpin and drives on, away from it -- distances that only
# rise -- except sample k*, which reverses along the first leg to where the way back comes into view
def one_sample_case(K, k_star, T=10):
    ref = hairpin_path()
    kw = base_kwargs(ref, K, T, param_exploration=0.01, max_speed=2.0, sigma=np.array([[0.04, 0.0], [0.0, 0.01]]))
    assert mppi_oracle.exploit_threshold(0.01, K) > K - 1  # every sample follows the nominal controls plus its noise
    u_in = np.column_stack([np.full(T, 0.3), np.zeros(T)])
    eps = np.zeros((K, T, 2), np.float32)
    eps[k_star, :, 0] = -1.03  # 0.3 - 1.03: 0.073 back per step (never halfway between two waypoints)
    return Case(f"one-K{K}-k{k_star}", kw, [1.25, -0.01, 0.0], u_in, eps, "numpy")


ONE_SAMPLE = [("0", 17, 0), ("0", 17, 16), ("0", 49, 48), ("0", 33, 16), ("1", 33, 0), ("1", 33, 32), ("1", 65, 64), ("1", 65, 31)]


# (d) timeout: the (a) inputs with two workgroups or more, and one workgroup that never waits
def single_workgroup_case(dual):
    K = WG_SAMPLES[dual]
    c = good_case(53, 33)
    kw = dict(c.kw, num_samples_K=K)
    return Case(f"single-K{K}", kw, c.x0, c.u_in, c.eps[:K], c.variant, iters=2, prev_idx=c.prev_idx)


TIMEOUT_GOOD = [(53, 33), (129, 33)]
