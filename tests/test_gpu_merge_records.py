"""GPU, public C ABI only: the record merge, the moving average, update, clamp and shift apart from the rollout.

(a) Records of our own making go into `mppi_step_end` (merge_abi and the finalize's tail): both precisions x every filter mode
    x the clamp on and off x T in {10, 33, 65} x nranks in {1, 2, 3, 63, 64, 65, 255, 256} x the record families of
    tests/merge_checks.py.
(b) The rank's one record that `mppi_step_begin` leaves is compared with the softmin record of the handle's own costs and the
    injected noise -- S taken as given, which isolates reduce and merge from the rollout -- under the three rollout layouts, at
    record counts next to every branch of the merge tree; and a whole `mppi_step` at the same shapes, whose finalize merges
    one or two windows of block records itself, in f32 as well as f64.

References, bounds and case tables: tests/merge_checks.py; no tolerance is chosen here."""
import functools

import numpy as np
import pytest

import merge_checks as mc
from oracle import mppi_oracle, philox

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "f64")
UMAX = (0.9, 0.04)  # small enough that some elements of the updated sequence clamp
X0 = np.array([0.4, -0.1, -0.35])
SIGMA = np.array([[0.1, 0.0], [0.0, 0.01]])


def engine(precision, K, T, beta, mode, window=10, clamp=0):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    assert (capi.FILTER_DIFFDRIVE, capi.FILTER_RACECAR, capi.FILTER_NONE, capi.FILTER_TORCH) == (
        mc.FILTER_DIFFDRIVE, mc.FILTER_RACECAR, mc.FILTER_NONE, mc.FILTER_TORCH)
    e = pkg.Engine(model=capi.MODEL_DIFFDRIVE, K=K, T=T, delta_t=0.1, u_max=list(UMAX), param_exploration=0.1,
                   param_lambda=1.0 / beta, param_alpha=0.2, sigma=SIGMA.reshape(-1).tolist(), stage_cost_weight=[5, 5, 10, 0],
                   terminal_cost_weight=[5, 5, 10, 0], beta_mode=capi.BETA_INV_LAMBDA, waypoint_mode=capi.WAYPOINT_FROZEN,
                   search_window=20, clamp_rollout=1, clamp_u_after_update=int(clamp), filter_mode=mode, filter_window=window,
                   seed=7, precision=capi.PREC_F32 if precision == "f32" else capi.PREC_F64)
    e.set_ref_path(mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100))
    return e


@functools.lru_cache(maxsize=None)
def merged(T, precision):
    """[(case, merge result, bounds)] of the ABI case table at horizon T: shared by every filter mode and clamp setting."""
    out = []
    for c in mc.abi_cases(T):
        out.append((c, mc.merge(c["rho"], c["eta"], c["eta2"], c["W"], c["beta"], precision),
                    mc.bound(c["rho"], c["eta"], c["eta2"], c["W"], c["beta"], precision)))
    return out


def step_end_with(e, case, u_prev):
    import torch
    recs = np.concatenate([np.stack([case["rho"], case["eta"], case["eta2"]], axis=1), case["W"]], axis=1)
    assert recs.shape[1] == e.partial_len()
    own = torch.empty(e.partial_len(), dtype=torch.float64, device="cuda")
    e.set_u_prev(u_prev)
    e.step_begin(X0, None, own)
    return e.step_end(torch.from_numpy(np.ascontiguousarray(recs)).cuda().reshape(-1), case["n"])


@pytest.mark.parametrize("mode", sorted(mc.FILTER_MODES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_step_end_on_synthetic_records(precision, mode):
    """u, u0, stats.rho / eta / ess / n_collided of `mppi_step_end` on records we built (K = 16 handle, frozen index, a non-trivial
    u_prev): within the bounds of merge_checks, stats.rho the minimum of the rounded inputs exactly."""
    m = mc.FILTER_MODES[mode]
    worst, over, n_cases, clamped = {}, [], 0, 0
    for T in mc.ABI_T:
        u_prev = mc.u_prev_signal(T)
        for clamp in (0, 1):
            handles = {}
            for case, (rho, eta, eta2, w), b in merged(T, precision):
                if case["beta"] not in handles:
                    handles[case["beta"]] = engine(precision, 16, T, case["beta"], m, clamp=clamp)
                u, u0, st = step_end_with(handles[case["beta"]], case, u_prev)
                fin = mc.finish(w, u_prev, m, 10, clamp, UMAX, precision)
                bu = mc.shift(mc.bound_u(b["w_eps"], w, u_prev, m, 10, precision))
                assert st.rho == rho and st.n_collided == -1, (case["name"], st.rho, rho, st.n_collided)
                r = {"u": mc.ratio(u, fin["u"], bu), "u0": mc.ratio(u0, fin["u0"], bu[0]), "eta": mc.ratio(st.eta, eta, b["eta"]),
                     "ess": mc.ratio(st.ess, eta * eta / eta2, b["ess"])}
                if case["family"] == "dominant":  # the single-record answer, held to the single record's own bound
                    p = case["pos"]
                    one = dict(case, n=1, rho=case["rho"][p:p + 1], eta=case["eta"][p:p + 1], eta2=case["eta2"][p:p + 1], W=case["W"][p:p + 1])
                    ref1 = mc.reference_step(one, u_prev, m, 10, clamp, UMAX, precision)
                    r["u_single"] = mc.ratio(u, ref1["u"], ref1["bound_u"])
                n_cases += 1
                clamped += int(clamp and (np.abs(fin["u_updated"]) == mc.rounded(UMAX, precision)).any())
                for k, v in r.items():
                    worst[(case["family"], k)] = max(worst.get((case["family"], k), 0.0), v)
                    if not v <= 1.0:
                        over.append((case["name"], f"T={T} clamp={clamp}", k, v))
            for h in handles.values():
                h.close()
    print(f"step_end {precision} {mode}: {n_cases} cases, max error / bound",
          {f"{f}.{k}": round(v, 4) for (f, k), v in sorted(worst.items())})
    assert clamped > n_cases // 4  # the clamp did act
    assert not over, over[:10]


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the rank's record out of mppi_step_begin, and a whole step
# ---------------------------------------------------------------------------------------------------------------------------
RECORD_K = (1, 17, 100, 16 * 31 + 3, 16 * 64 + 1, 4096, 4112)  # 1, 2, 7, 32, 65, 256, 257 records of 16 samples
STEP_K = RECORD_K + (8192, 8208)                                # 512 and 513: two windows, and the first 64:1 merge in front
RECORD_T = (10, 32, 33, 64, 65, 97)                             # one to four 16-byte column tiles in f64, one or two in f32
LAYOUTS = {"dual0": {"MPPI_DUAL": "0"}, "dual1": {"MPPI_DUAL": "1"}, "unfused": {"MPPI_FORCE_UNFUSED": "1"}}
BETA_B = 1.0


@functools.lru_cache(maxsize=None)
def noise(K, T):
    return philox.sample_epsilon(SIGMA, 77, 0, K, T)


def assert_layout(e, layout, T):
    from dnn_mppi_mpc_amd import _capi as capi
    kind, name = e.counters()["rollout_layout"] & capi.LAYOUT_KIND, e.rollout_kernel()
    if layout == "unfused":
        assert name.startswith("k_rollout<"), name  # the separate rollout: k_reduce leaves the records
    elif T > 64:
        assert kind == capi.LAYOUT_PAIR and name.startswith("k_rollout_dual<"), (kind, name)  # one sample per wave, two steps per lane
    elif layout == "dual0":
        assert e.counters()["rollout_layout"] == capi.LAYOUT_FUSED and name.startswith("k_rollout_fused<"), (kind, name)
    else:
        assert kind == capi.LAYOUT_DUAL, (kind, name)  # two samples per wave


def sample_reference(S, eps, precision, K):
    """Every sample as a record of its own {S_k, 1, 1, eps_k}: their merge is the record of all samples; n = K terms."""
    one = np.ones(K)
    E = eps.reshape(K, -1).astype(np.float64)
    rho, eta, eta2, w = mc.merge(S, one, one, E, BETA_B, precision)
    return rho, eta, eta2, w, mc.bound(S, one, one, E, BETA_B, precision, n=K)


@pytest.mark.parametrize("T", RECORD_T)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rank_record_and_whole_step_against_the_costs_and_the_noise(monkeypatch, precision, layout, T):
    """`mppi_step_begin`'s record {rho, eta, eta2, W} against the softmin record of costs() and the injected noise (rho == min S
    exactly), then `mppi_step_end` on that one record and a whole `mppi_step` (the finalize's own merge of one or two windows
    of block records) against finish(merge(...)) -- n = K summed terms in every bound."""
    import torch
    for k in ("MPPI_DUAL", "MPPI_FORCE_UNFUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    u_prev = mc.u_prev_signal(T)
    worst, over = {}, []

    def note(K, what, v):
        worst[what] = max(worst.get(what, 0.0), v)
        if not v <= 1.0:
            over.append((f"K={K}", what, v))

    for K in STEP_K:
        eps = torch.from_numpy(noise(K, T)).cuda()
        if K in RECORD_K:
            e = engine(precision, K, T, BETA_B, mc.FILTER_DIFFDRIVE, clamp=1)
            e.set_u_prev(u_prev)
            rec = torch.empty(e.partial_len(), dtype=torch.float64, device="cuda")
            e.step_begin(X0, eps, rec)
            assert_layout(e, layout, T)
            S, got = e.costs(), rec.cpu().numpy()
            rho, eta, eta2, w, b = sample_reference(S, noise(K, T), precision, K)
            assert got[0] == rho == S.min(), (K, got[0], rho)
            note(K, "record.eta", mc.ratio(got[1], eta, b["eta"]))
            note(K, "record.eta2", mc.ratio(got[2], eta2, b["eta2"]))
            note(K, "record.W", mc.ratio(got[3:], w * eta, b["w_eps"] * eta))
            u, u0, st = e.step_end(rec, 1)
            fin = mc.finish(w, u_prev, mc.FILTER_DIFFDRIVE, 10, 1, UMAX, precision)
            bu = mc.shift(mc.bound_u(b["w_eps"], w, u_prev, mc.FILTER_DIFFDRIVE, 10, precision))
            note(K, "step_end.u", mc.ratio(u, fin["u"], bu))
            e.close()
        e = engine(precision, K, T, BETA_B, mc.FILTER_DIFFDRIVE, clamp=1)
        e.set_u_prev(u_prev)
        u, u0, st = e.step(X0, eps)
        assert_layout(e, layout, T)
        S = e.costs()
        rho, eta, eta2, w, b = sample_reference(S, noise(K, T), precision, K)
        fin = mc.finish(w, u_prev, mc.FILTER_DIFFDRIVE, 10, 1, UMAX, precision)
        bu = mc.shift(mc.bound_u(b["w_eps"], w, u_prev, mc.FILTER_DIFFDRIVE, 10, precision))
        assert st.rho == rho == S.min(), (K, st.rho, rho)
        note(K, "step.u", mc.ratio(u, fin["u"], bu))
        note(K, "step.u0", mc.ratio(u0, fin["u0"], bu[0]))
        note(K, "step.eta", mc.ratio(st.eta, eta, b["eta"]))
        note(K, "step.ess", mc.ratio(st.ess, eta * eta / eta2, b["ess"]))
        e.close()
    print(f"records {precision} {layout} T={T}: max error / bound", {k: round(v, 4) for k, v in sorted(worst.items())})
    assert not over, over[:10]
