"""GPU: the `pytorch_mppi`-style controller (csrc/mppi_cb.hip behind callback_mppi.py) held to the f64 references, error models
and case tables of tests/callback_checks.py, which tests/test_callback_cases.py checks without a device: the models alone,
`cost_total` with injected noise at the shapes where the kernels change behaviour, softmin and update from the device's own
costs with weights that spread, the in-kernel sampler number by number, and the refusals.  PARITY UNPINNED as in
tests/test_gpu_callback_mppi.py: these tests hold the kernels to the restated algorithm more tightly, they do not pin the
library.  Every tolerance is one derived in callback_checks.py or its measured-ratio rule (profiles/callback_measured.json,
tools/callback_report.py reads the figures every test prints)."""
import functools

import numpy as np
import pytest

import callback_checks as cc

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF


def _running_cost(cost):
    from dnn_mppi_mpc_amd.callback_mppi import RunningCost
    return RunningCost(cost["goal"], cost["q"], cost["r"], cost["obstacles"], cost["safety"], cost["weight"], cost["kind"])


def _ctrl(case, **over):
    from dnn_mppi_mpc_amd.callback_mppi import MPPI
    kw = dict(num_samples=case["K"], horizon=case["T"], lambda_=case["lam"], u_init=case["u_init"],
              sample_null_action=case["null"], seed=SEED, dt=case["dt"])
    if case["bounded"]:
        kw.update(u_min=case["u_min"], u_max=case["u_max"])
    kw.update(over)
    return MPPI(case["dyn"], _running_cost(case["cost"]), cc.NX[case["dyn"]], case["sigma"], **kw)


def _cuda(noise):
    import torch
    return torch.from_numpy(np.ascontiguousarray(noise, np.float32)).cuda()


# ------------------------------------------------------------------------------------------------------------------
# the models alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs", cc.MODEL_N_OBS)
@pytest.mark.parametrize("dyn,cost_name", cc.MODEL_PAIRS)
def test_models_alone_against_f64(dyn, cost_name, n_obs):
    """`_dynamics` and `_running_cost` (mppi_cb_eval) at n = 1 and across the 256 boundary, first and last step of the horizon,
    headings up to 1e3, rows on the centre of an obstacle and on either side of the inverse cost's step."""
    case = dict(dyn=dyn, cost=cc._cost(cost_name, n_obs), K=4, T=cc.MODEL_T, lam=1.0, u_init=np.zeros(cc.NU[dyn]), null=False,
                dt=cc.DT[dyn], bounded=False, sigma=cc.SIGMAS[dyn])
    ctrl = _ctrl(case)
    worst = {"dynamics": 0.0, "cost": 0.0}
    for n in cc.MODEL_N:
        for t in (0, cc.MODEL_T - 1):
            s, a, cost = cc.model_rows(dyn, cost_name, n, n_obs, t)
            want, bound = cc.dynamics(dyn, s, a, cc.DT[dyn])
            got = ctrl._dynamics(s, a, t)
            assert got.shape == want.shape
            worst["dynamics"] = max(worst["dynamics"], cc.ratio(got, want, bound))
            c, cbound, _ = cc.running_cost(s, a, t, cost)
            gc = ctrl._running_cost(s, a, t)
            assert gc.shape == c.shape
            worst["cost"] = max(worst["cost"], cc.ratio(gc, c, cbound))
    print(f"callback models {dyn}-{cost_name}-obs{n_obs}: max error / bound {worst}")
    assert worst["dynamics"] <= 1.0 and worst["cost"] <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------
# one command per case with injected noise, run once and shared
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(name):
    c = cc.cases()[name]
    ctrl = _ctrl(c)
    ctrl.U = c["U"]
    action = ctrl.command(c["state"], noise=_cuda(c["noise"]))
    return dict(action=action, cost_total=ctrl.cost_total, omega=ctrl.omega, U=ctrl.U, ctrl=ctrl)


@pytest.mark.parametrize("name", list(cc.cases()))
def test_cost_total_against_f64(name):
    """The rollout and the perturbation term: the device's distance from the f64 reference over the kept samples against the
    f32 restatement's own distance on the same inputs."""
    ref, _, dist = cc.reference(name)
    got = _run(name)["cost_total"]
    assert np.isfinite(got).all()
    dev = cc.cost_distance(got, ref["cost_total"], ref["keep"])
    print(f"callback cost_total {name}: device distance {dev:.4g} restatement distance {dist:.4g} ratio {dev / dist:.4g}")
    assert dev <= cc.COST_FACTOR * dist


@pytest.mark.parametrize("name", list(cc.cases()))
def test_softmin_and_update_from_the_device_costs(name):
    """omega against the f64 softmin of the costs the device returned, U against U + sum omega noise with the omega the device
    returned, the action against U[0] bit for bit."""
    c = cc.cases()[name]
    ref, _, _ = cc.reference(name)
    r = _run(name)
    K = c["K"]
    want, x = cc.softmin(r["cost_total"], cc._r(c["lam"]))
    rw = cc.ratio(r["omega"], want, cc.bound_omega(want, x, K))
    U_new, bound = cc.update(ref["U_shifted"], r["omega"], ref["noise"])
    ru = cc.ratio(r["U"], U_new, bound)
    print(f"callback omega {name}: ESS {cc.ess(r['omega']):.1f} of {K} ratio {rw:.4g}")
    print(f"callback U {name}: ratio {ru:.4g}")
    assert rw <= 1.0 and ru <= 1.0, (rw, ru)
    np.testing.assert_array_equal(r["action"], r["U"][0])
    if c["family"] == "spread":
        assert cc.ess(r["omega"]) >= cc.ESS_FLOOR * K  # the weighted reduction is what this case reads


def test_next_command_shifts_by_one_row_and_appends_u_init():
    """Two more commands on a handle with a non-zero u_init: each starts from the previous sequence moved by one row."""
    name = "uni-inv-K257-T25"
    c = cc.cases()[name]
    assert c["u_init"].any()
    ctrl = _ctrl(c)
    ctrl.U = c["U"]
    rng = np.random.default_rng(11)
    L = np.linalg.cholesky(c["sigma"])
    U = c["U"]
    for it in range(3):
        noise = (rng.normal(size=c["noise"].shape) @ L.T).astype(np.float32)
        a = ctrl.command(c["state"], noise=_cuda(noise))
        Us, _, nz = cc.clamped_noise(c, U, noise)
        np.testing.assert_array_equal(Us[-1], cc.rounded(c["u_init"]))
        want, bound = cc.update(Us, ctrl.omega, nz)
        U = ctrl.U
        ratio = cc.ratio(U, want, bound)
        print(f"callback U shift-{it}: ratio {ratio:.4g}")
        assert ratio <= 1.0
        np.testing.assert_array_equal(a, U[0])


@pytest.mark.parametrize("name", ["uni-inv-K256-T25-null", "spread-skid-inv-K257-T64"])
def test_no_shift_and_U_init(name):
    """`U_init=` at construction and `shift_nominal_trajectory=False`: the command works on the sequence as it stands."""
    c = cc.cases()[name]
    ctrl = _ctrl(c, U_init=c["U"])
    np.testing.assert_array_equal(ctrl.U, cc.rounded(c["U"]))
    a = ctrl.command(c["state"], shift_nominal_trajectory=False, noise=_cuda(c["noise"]))
    ref = cc.command(c, c["state"], c["U"], c["noise"], do_shift=False)
    np.testing.assert_array_equal(ref["U_shifted"], cc.rounded(c["U"]))
    dist = cc.cost_distance(cc.restatement(c, c["state"], c["U"], c["noise"], do_shift=False).cost_total, ref["cost_total"],
                            ref["keep"])
    dev = cc.cost_distance(ctrl.cost_total, ref["cost_total"], ref["keep"])
    want, bound = cc.update(ref["U_shifted"], ctrl.omega, ref["noise"])
    ru = cc.ratio(ctrl.U, want, bound)
    print(f"callback cost_total noshift-{name}: device distance {dev:.4g} restatement distance {dist:.4g} ratio {dev / dist:.4g}")
    print(f"callback U noshift-{name}: ratio {ru:.4g}")
    assert dev <= cc.COST_FACTOR * dist and ru <= 1.0
    np.testing.assert_array_equal(a, ctrl.U[0])


# ------------------------------------------------------------------------------------------------------------------
# the in-kernel sampler, number by number
# ------------------------------------------------------------------------------------------------------------------
PROBE_K, PROBE_T = 300, 3


def _probe(dyn, sigma, seed=SEED):
    case = dict(dyn=dyn, cost=cc.probe_cost(), K=PROBE_K, T=PROBE_T, lam=1.0, u_init=np.zeros(cc.NU[dyn]), null=False,
                dt=cc.DT[dyn], bounded=False, sigma=sigma)
    return _ctrl(case, seed=seed)


def _read(ctrl, dyn, t0, i):
    """One command of the probe: cost_total[k] = (Sigma^-1 noise[k, t0])_i of the iteration it ran at."""
    U = np.zeros((PROBE_T, cc.NU[dyn]))
    U[t0, i] = 1.0
    ctrl.U = U
    ctrl.command(np.zeros(cc.NX[dyn]), shift_nominal_trajectory=False)
    return ctrl.cost_total


@pytest.mark.parametrize("dyn,sigma", [("unicycle", np.eye(2)), ("skid_steer", np.eye(4)), ("skid_steer", cc.SIGMA4),
                                       ("unicycle", cc.SIGMA2)], ids=["uni-I", "skid-I", "skid-S4", "uni-S2"])
def test_in_kernel_sampler_number_by_number(dyn, sigma):
    """Sigma = I: every standard normal the kernel draws, (k, t, iteration) by (k, t, iteration), against the restatement on
    oracle/philox.py.  Non-diagonal Sigma: (L^-T z)_i, which holds the factor and the inverse together."""
    ctrl = _probe(dyn, sigma)
    iteration, worst = 0, 0.0
    for t0 in range(PROBE_T):
        for i in range(cc.NU[dyn]):
            got = _read(ctrl, dyn, t0, i)
            want, tol = cc.probe_value(sigma, SEED, iteration, PROBE_K, PROBE_T, t0, i)
            assert np.abs(want).max() > 1.0  # (there is a number to compare)
            worst = max(worst, float(np.abs(got - want).max() / tol))
            iteration += 1
    print(f"callback sampler {dyn}-{'I' if not (sigma - np.eye(len(sigma))).any() else 'S'}: ratio {worst:.4g}")
    assert worst <= 1.0


def test_in_kernel_sampler_same_seed_same_numbers_other_seed_or_iteration_others():
    a, b, other = _probe("skid_steer", np.eye(4)), _probe("skid_steer", np.eye(4)), _probe("skid_steer", np.eye(4), seed=SEED + 1)
    za0, zb0, zo0 = (_read(h, "skid_steer", 1, 2) for h in (a, b, other))
    np.testing.assert_array_equal(za0, zb0)
    assert not np.array_equal(za0, zo0) and np.abs(za0 - zo0).max() > 1.0
    za1 = _read(a, "skid_steer", 1, 2)  # iteration 1
    assert not np.array_equal(za0, za1) and np.abs(za0 - za1).max() > 1.0
    np.testing.assert_array_equal(za1, _read(b, "skid_steer", 1, 2))


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refused_noise_leaves_the_handle_as_it_was():
    c = cc.cases()["uni-inv-K256-T25-null"]
    used, fresh = _ctrl(c), _ctrl(c)
    used.U = fresh.U = c["U"]
    good = _cuda(c["noise"])
    for bad in (good.double(), good.half(), good[:-1].contiguous(), good[:, :-1].contiguous(), good.reshape(c["K"], -1),
                good.transpose(0, 1), good.cpu()):
        with pytest.raises(ValueError):
            used.command(c["state"], noise=bad)
    np.testing.assert_array_equal(used.U, fresh.U)
    for noise in (good, None):  # (None: the in-kernel draw -- no refused call moved the iteration counter)
        np.testing.assert_array_equal(used.command(c["state"], noise=noise), fresh.command(c["state"], noise=noise))
        np.testing.assert_array_equal(used.cost_total, fresh.cost_total)
        np.testing.assert_array_equal(used.omega, fresh.omega)
        np.testing.assert_array_equal(used.U, fresh.U)


def test_refused_configurations_and_a_usable_library_after_them():
    import dnn_mppi_mpc_amd as pkg
    c = cc.cases()["uni-inv-K256-T25-null"]
    before = _ctrl(c)
    before.U = c["U"]
    want = before.command(c["state"], noise=_cuda(c["noise"]))
    asym = cc.SIGMA2.copy()
    asym[0, 1] += 1e-3
    asym4 = cc.SIGMA4.copy()
    asym4[1, 3] *= -1.0
    many = dict(c["cost"], obstacles=cc.obstacle_field(c["cost"]["obstacles"], 17))
    sk = cc.cases()["skid-inv-K256-T7-free"]
    refused = [lambda: _ctrl(dict(c, sigma=asym)), lambda: _ctrl(dict(sk, sigma=asym4)), lambda: _ctrl(dict(c, T=129)),
               lambda: _ctrl(dict(sk, T=65)), lambda: _ctrl(dict(c, cost=many)), lambda: _ctrl(dict(c, lam=0.0)),
               lambda: _ctrl(dict(c, dt=0.0)), lambda: _ctrl(dict(c, K=0))]
    for make in refused:
        with pytest.raises(pkg.MppiError):
            make()
    # what stands next to each of them is accepted
    _ctrl(dict(c, T=128))
    _ctrl(dict(c, cost=dict(c["cost"], obstacles=cc.obstacle_field(c["cost"]["obstacles"], 16))))
    _ctrl(dict(c, sigma=cc.SIGMA2 * (1.0 + 1e-13 * np.array([[0, 1], [0, 0]]))))  # symmetric within rounding
    after = _ctrl(c)
    after.U = c["U"]
    np.testing.assert_array_equal(after.command(c["state"], noise=_cuda(c["noise"])), want)
    np.testing.assert_array_equal(after.cost_total, before.cost_total)
