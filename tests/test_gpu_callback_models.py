"""GPU: the callback controller's race-car and double-integrator models, terminal cost, the options `noise_mu`, `u_scale`,
`noise_abs_cost`, `u_per_command`, the perturbed actions and the cheapest samples' trajectories (csrc/mppi_cb.hip behind
callback_mppi.py), held to the f64 definitions, the error rule and the case tables of tests/callback_models_checks.py, which
tests/test_callback_models_cases.py checks without a device.  PARITY UNPINNED as in tests/test_gpu_callback_mppi.py.

Every comparison with a tolerance follows the measured-ratio rule (`cm.held`: the device within cc.COST_FACTOR times the
unchanged f32 restatement's own distance from f64, floored at one f32 ulp of the largest term) and prints its ratio;
tools/callback_models_report.py collects them into profiles/callback_models_measured.json.  omega and U are compared from
the device's own costs against the first-order bounds of callback_checks.py; indices, perturbed actions and everything
compared between two handles are compared exactly."""
import functools

import numpy as np
import pytest

import callback_checks as cc
import callback_models_checks as cm
from oracle import mppi_cb_oracle as cbo

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
F = np.float32


def _running_cost(cost):
    from dnn_mppi_mpc_amd.callback_mppi import RunningCost
    return RunningCost(cost["goal"], cost["q"], cost["r"], cost["obstacles"], cost["safety"], cost["weight"], cost["kind"])


def _ctrl(case, **over):
    from dnn_mppi_mpc_amd.callback_mppi import MPPI, TerminalCost
    kw = dict(num_samples=case["K"], horizon=case["T"], lambda_=case["lam"], u_init=case["u_init"],
              sample_null_action=case["null"], seed=SEED, dt=case["dt"], u_scale=case.get("u_scale", 1.0),
              noise_abs_cost=case.get("abs_cost", False))
    if case.get("terminal") is not None:
        kw["terminal_state_cost"] = TerminalCost(case["terminal"]["goal"], case["terminal"]["q"])
    if case["bounded"]:
        kw.update(u_min=case["u_min"], u_max=case["u_max"])
    kw.update(over)
    return MPPI(case["dyn"], _running_cost(case["cost"]), cm.NX[case["dyn"]], case["sigma"], **kw)


def _cuda(noise):
    import torch
    return torch.from_numpy(np.ascontiguousarray(noise, F)).cuda()


def _plain(dyn, K=4, T=25, **kw):
    return dict(dyn=dyn, cost=cm.cost_of(dyn), K=K, T=T, lam=1.0, u_init=np.zeros(cm.NU[dyn]), null=False, dt=cm.DT[dyn],
                bounded=False, sigma=cm.SIGMA[dyn], terminal=cm.TERMINAL[dyn], **kw)


# ------------------------------------------------------------------------------------------------------------------
# 1. the models alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dyn", list(cm.NX))
def test_models_alone_against_f64(dyn):
    """`_dynamics`, `_running_cost` and `_terminal_cost` (mppi_cb_eval, what = 0, 1, 2) on 1, 255, 256 and 257 rows."""
    ctrl = _ctrl(_plain(dyn))
    cost, term = cm.cost_of(dyn), cm.TERMINAL[dyn]
    kw = dict(goal=cost["goal"], q_diag=cost["q"], r_diag=cost["r"], obstacles=cost["obstacles"], safety=cost["safety"],
              weight=cost["weight"], kind=cost["kind"])
    fine = True
    for n in cm.MODEL_N:
        worst = {"dynamics": 0.0, "cost": 0.0, "terminal": 0.0}
        s, a = cm.model_rows(dyn, n)
        want, largest = cm.dynamics(dyn, s, a, cm.DT[dyn])
        got = ctrl._dynamics(s, a)
        assert got.shape == want.shape
        r, ok = cm.held(got, want, cm.dynamics32(dyn, s, a, cm.DT[dyn]), np.maximum(np.abs(want), largest), largest)
        worst["dynamics"], fine = max(worst["dynamics"], r), fine and ok
        for t in (0, 24):
            c, _, _ = cc.running_cost(s, a, t, cost)
            gc = ctrl._running_cost(s, a, t)
            assert gc.shape == c.shape
            big = cm.cost_largest(s, a, t, cost)
            r, ok = cm.held(gc, c, cbo.running_cost(s, a, t, **kw), np.maximum(np.abs(c), big), big)
            worst["cost"], fine = max(worst["cost"], r), fine and ok
        tc, big = cm.terminal_cost(s, term)
        gt = ctrl._terminal_cost(s)
        assert gt.shape == tc.shape
        r, ok = cm.held(gt, tc, cm.terminal_cost32(s, term), np.maximum(np.abs(tc), big), big)
        worst["terminal"], fine = max(worst["terminal"], r), fine and ok
        print(f"callback models {dyn}-n{n}: device / restatement ratio {worst}")
    assert fine


def test_terminal_cost_needs_one():
    import dnn_mppi_mpc_amd as pkg
    ctrl = _ctrl(dict(_plain("double_integrator"), terminal=None))
    with pytest.raises(pkg.MppiError) as e:
        ctrl._terminal_cost(np.zeros((3, 2)))
    assert e.value.code == -7  # MPPI_ERR_STATE
    assert ctrl._running_cost(np.ones((3, 2)), np.ones((3, 1))).tolist() == [3.0, 3.0, 3.0]


# ------------------------------------------------------------------------------------------------------------------
# 2. one command per case with injected noise, run once and shared
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(name):
    c = cm.cases()[name]
    ctrl = _ctrl(c)
    ctrl.U = c["U"]
    noise = _cuda(c["noise"])
    action = ctrl.command(c["state"], noise=noise)
    return dict(action=action, cost_total=ctrl.cost_total, omega=ctrl.omega, U=ctrl.U, ctrl=ctrl, noise=noise)


@pytest.mark.parametrize("name", list(cm.cases()))
def test_cost_total_against_f64(name):
    """The rollout with the new models, the terminal term, u_scale and the perturbation term in both forms."""
    ref, rst = cm.reference(name)
    got = _run(name)["cost_total"]
    assert np.isfinite(got).all()
    ratio, ok = cm.cost_held(got, ref, rst["cost_total"])
    dev = cc.cost_distance(got, ref["cost_total"], ref["keep"])
    print(f"callback models cost_total {name}: device distance {dev:.4g} restatement distance "
          f"{cm.restatement_distance(name):.4g} ratio {ratio:.4g}")
    assert ok, ratio


@pytest.mark.parametrize("name", list(cm.cases()))
def test_softmin_and_update_from_the_device_costs(name):
    """omega against the f64 softmin of the costs the device returned, U against U + sum omega noise with the omega the device
    returned (the SIGNED noise, with noise_abs_cost too), the action against U[0] bit for bit."""
    c = cm.cases()[name]
    ref, _ = cm.reference(name)
    r = _run(name)
    K = c["K"]
    want, x = cc.softmin(r["cost_total"], cc._r(c["lam"]))
    rw = cc.ratio(r["omega"], want, cc.bound_omega(want, x, K))
    U_new, bound = cc.update(ref["U_shifted"], r["omega"], ref["noise"])
    ru = cc.ratio(r["U"], U_new, bound)
    print(f"callback models omega {name}: ESS {cc.ess(r['omega']):.1f} of {K} ratio {rw:.4g}")
    print(f"callback models U {name}: ratio {ru:.4g}")
    assert rw <= 1.0 and ru <= 1.0, (rw, ru)
    np.testing.assert_array_equal(r["action"], r["U"][0])
    if c["family"] == "spread" and K > 1:
        assert cc.ess(r["omega"]) >= cc.ESS_FLOOR * K


def test_horizon_limit_stands_next_to_the_longest_accepted():
    """T * nu <= 256: the double integrator runs at T = 256 and the dynamic race car at T = 128 (both in the case table); the
    kinematic one is accepted there too; one step more is refused."""
    import dnn_mppi_mpc_amd as pkg
    assert cm.cases()["double-K257-T256-term"]["T"] == 256 and cm.cases()["dynamic-K256-T128"]["T"] == 128
    for dyn, T in (("double_integrator", 257), ("racecar", 129), ("racecar_dynamic", 129)):
        with pytest.raises(pkg.MppiError) as e:
            _ctrl(_plain(dyn, T=T))
        assert e.value.code == -2  # MPPI_ERR_SHAPE
    ctrl = _ctrl(_plain("racecar", K=8, T=128))
    ctrl.command(cm.START["racecar"])
    assert np.isfinite(ctrl.cost_total).all() and ctrl.U.shape == (128, 2)


# ------------------------------------------------------------------------------------------------------------------
# 3. the options
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 25])
def test_u_per_command_returns_the_first_rows_and_shifts_by_one(n):
    c = cm.cases()[cm.OPTION_BASE]
    one, many = _ctrl(c), _ctrl(c, u_per_command=n)
    one.U = many.U = c["U"]
    rng = np.random.default_rng(3)
    for _ in range(2):
        noise = _cuda(rng.normal(0, 0.2, c["noise"].shape))
        a1, an = one.command(c["state"], noise=noise), many.command(c["state"], noise=noise)
        assert an.shape == ((2,) if n == 1 else (n, 2)) and a1.shape == (2,)
        np.testing.assert_array_equal(an, one.U[0] if n == 1 else one.U[:n])
        np.testing.assert_array_equal(many.U, one.U)  # (so the second command started from a shift by ONE row)
        np.testing.assert_array_equal(many.cost_total, one.cost_total)


MU_K, MU_T = 4000, 3  # 12000 draws: five standard errors of the mean are 0.032 and 0.025, under half of |mu| = (0.08, 0.15)


def _mu_probe(**over):
    """A handle whose cost is zero whatever it does (cc.probe_cost), without bounds, lambda = 1: what is left of cost_total
    is the perturbation term, and with U = 0 the perturbed actions ARE the draw."""
    case = dict(_plain("racecar", K=MU_K, T=MU_T), cost=cc.probe_cost(), sigma=cc.SIGMA2, terminal=None)
    return _ctrl(case, noise_mu=cm.OPTION_MU, **over)


def test_noise_mu_moves_the_in_kernel_draw_and_nothing_else():
    """The in-kernel draw is mu + L z.  Mean: over K * T draws within 5 standard errors of mu.  Number by number: with U = 0 and
    no bounds `perturbed_action` is the draw itself, held to cc.cb_noise + mu; and through the probe of
    cc.probe_cost / cc.probe_value, cost_total = (Sigma^-1 (mu + L z)[k, t0])_i.  Tolerance: the sampler's (cc.SAMPLER_ATOL per
    normal, times sum_j |L_ij|) plus two roundings at magnitude < 8 (the sum with mu, and the probe's (1 + n) - 1)."""
    ctrl = _mu_probe()
    L, sinv = cc.factor(cc.SIGMA2)
    absL = np.abs(L).sum(1)
    iteration = 0
    ctrl.command(np.zeros(4), shift_nominal_trajectory=False)  # U = 0 at creation
    draw = ctrl.perturbed_action
    want = cc.cb_noise(cc.SIGMA2, SEED, iteration, MU_K, MU_T) + cc.rounded(cm.OPTION_MU)
    assert np.abs(want).max() < 7.0
    worst = float((np.abs(draw - want) / (cc.SAMPLER_ATOL * absL + 2 * cc.PROBE_ROUNDING)).max())
    err = np.abs(draw.reshape(-1, 2).mean(0) - cm.OPTION_MU)
    allowed = 5.0 * np.sqrt(np.diag(cc.SIGMA2) / (MU_K * MU_T))
    print(f"callback models sampler noise_mu-draw: mean error {err} allowed {allowed} ratio {worst:.4g}")
    assert (err <= allowed).all() and (np.abs(cm.OPTION_MU) > 2 * allowed).all()
    assert worst <= 1.0
    iteration += 1
    for t0 in range(MU_T):
        for i in range(2):
            U = np.zeros((MU_T, 2))
            U[t0, i] = 1.0
            ctrl.U = U
            ctrl.command(np.zeros(4), shift_nominal_trajectory=False)
            value, tol = cc.probe_value(cc.SIGMA2, SEED, iteration, MU_K, MU_T, t0, i)
            value = value + cc.rounded(cm.OPTION_MU) @ sinv[:, i]
            tol = tol + cc.PROBE_ROUNDING * np.abs(sinv[:, i]).sum()
            worst = max(worst, float(np.abs(ctrl.cost_total - value).max() / tol))
            iteration += 1
    print(f"callback models sampler noise_mu-probe: ratio {worst:.4g}")
    assert worst <= 1.0
    # an injected tensor stands for the whole draw: mu is not added to it
    other = _ctrl(dict(_plain("racecar", K=MU_K, T=MU_T), cost=cc.probe_cost(), sigma=cc.SIGMA2, terminal=None))
    noise = _cuda(np.random.default_rng(2).normal(0, 0.3, (MU_K, MU_T, 2)))
    ctrl.U = other.U = np.zeros((MU_T, 2))
    ctrl.command(np.zeros(4), shift_nominal_trajectory=False, noise=noise)
    other.command(np.zeros(4), shift_nominal_trajectory=False, noise=noise)
    np.testing.assert_array_equal(ctrl.get_perturbed_action(noise), noise.cpu().numpy())
    np.testing.assert_array_equal(ctrl.cost_total, other.cost_total)


def test_all_four_options_together_with_the_in_kernel_draw():
    """noise_mu, u_scale, noise_abs_cost and u_per_command on the one racecar case, drawn in the kernel: the clamped actions the
    device reports are the draw cc.cb_noise + mu, clamped; cost_total, omega and U follow from them by the f64 command."""
    c = dict(cm.cases()["option-all"], terminal=None)
    ctrl = _ctrl(c, noise_mu=cm.OPTION_MU, u_per_command=3)
    ctrl.U = c["U"]
    a = ctrl.command(c["state"])
    pa = ctrl.perturbed_action
    U_shifted = cc.shift(cc.rounded(c["U"]), c["u_init"])
    raw = U_shifted[None] + cc.cb_noise(c["sigma"], SEED, 0, c["K"], c["T"]) + cc.rounded(cm.OPTION_MU)
    want = np.clip(raw, cc.rounded(c["u_min"]), cc.rounded(c["u_max"]))
    L, _ = cc.factor(c["sigma"])
    tol = cc.SAMPLER_ATOL * np.abs(L).sum(1) + 2 * cc.PROBE_ROUNDING
    assert (np.abs(pa - want) <= tol).all() and (pa != raw.astype(F)).any() and (np.abs(pa) <= c["lim"]).all()
    ref = cm.command(c, c["state"], c["U"], None, actions=pa)
    rst = cm.restatement(c, c["state"], c["U"], None, actions=pa)
    ratio, ok = cm.cost_held(ctrl.cost_total, ref, rst["cost_total"])
    print(f"callback models cost_total option-all-in-kernel: ratio {ratio:.4g}")
    assert ok, ratio
    om, x = cc.softmin(ctrl.cost_total, cc._r(c["lam"]))
    U_new, bound = cc.update(ref["U_shifted"], ctrl.omega, ref["noise"])
    rw, ru = cc.ratio(ctrl.omega, om, cc.bound_omega(om, x, c["K"])), cc.ratio(ctrl.U, U_new, bound)
    print(f"callback models omega option-all-in-kernel: ratio {rw:.4g}")
    print(f"callback models U option-all-in-kernel: ratio {ru:.4g}")
    assert rw <= 1.0 and ru <= 1.0
    assert a.shape == (3, 2)
    np.testing.assert_array_equal(a, ctrl.U[:3])
    # the nominal trajectory applies u_scale to U, as the callers' self.u_scale * self.U[t] does
    traj = ctrl.get_optimal_trajectory(c["state"])
    want_t = cm.rollout(c["dyn"], c["state"], cc._r(cm.OPTION_SCALE) * ctrl.U[None], c["dt"])
    big = np.maximum.accumulate(np.abs(want_t), axis=1)
    r, ok = cm.held(traj[None], want_t, cm.rollout32(c["dyn"], c["state"], (F(cm.OPTION_SCALE) * ctrl.U.astype(F))[None], c["dt"]),
                    np.maximum(big, np.abs(cc.rounded(c["state"]))), big)
    print(f"callback models trajectory option-all-nominal: ratio {r:.4g}")
    assert ok, r


# ------------------------------------------------------------------------------------------------------------------
# 4. perturbed actions
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["racecar-K255-T1-null", "racecar-K257-T7-term", "dynamic-K255-T7-null", "double-K257-T256-term",
                                  "double-K256-T25-free-null", "option-all"])
def test_perturbed_actions_bit_for_bit(name):
    """clip(U_before + noise) of the f32 restatement, the null row included; U_before is the sequence after the shift and
    before the update, which the handle kept."""
    c = cm.cases()[name]
    r = _run(name)
    _, rst = cm.reference(name)
    pa = r["ctrl"].get_perturbed_action(r["noise"])
    assert pa.shape == (c["K"], c["T"], cm.NU[c["dyn"]])
    np.testing.assert_array_equal(pa, rst["act"])
    if c["null"]:
        assert not pa[-1].any() and pa[:-1].any()
    assert not np.array_equal(r["U"], cm.reference(name)[0]["U_shifted"])  # (the update did move U away from U_before)
    np.testing.assert_array_equal(r["ctrl"].get_perturbed_action(r["noise"]), pa)


# ------------------------------------------------------------------------------------------------------------------
# 5. the cheapest samples
# ------------------------------------------------------------------------------------------------------------------
TIES, NAN_ROW = (3, 5, 200), 7


@functools.lru_cache(maxsize=None)
def _fan(name):
    """A case without bounds whose injected noise repeats row 3 in rows 5 and 200 (bit-equal costs) and is NaN in row 7."""
    c = dict(cm.cases()[name], bounded=False)
    c["u_min"], c["u_max"] = np.full(2, -1e30), np.full(2, 1e30)
    noise = c["noise"].copy()
    noise[TIES[1]] = noise[TIES[2]] = noise[TIES[0]]
    noise[NAN_ROW] = np.nan
    ctrl = _ctrl(c)
    ctrl.U = c["U"]
    t = _cuda(noise)
    ctrl.command(c["state"], noise=t)
    return c, ctrl, t, ctrl.cost_total, ctrl.get_perturbed_action(t)


@pytest.mark.parametrize("n", [1, 10, None])
@pytest.mark.parametrize("name", ["spread-racecar-K255-T25-term", "option-scale"])
def test_cheapest_samples(name, n):
    """index_out against the rank definition applied to the device's own cost_total, exactly; equal costs in index order, the
    NaN sample last; the trajectories against the f64 rollout of u_scale * those samples' perturbed actions."""
    c, ctrl, noise, cost, pa = _fan(name)
    K = c["K"]
    n = K if n is None else n
    traj, idx = ctrl.get_sampled_trajectories(c["state"], n=n, noise=noise)
    assert traj.shape == (n, c["T"], 4) and idx.shape == (n,) and idx.dtype == np.int32
    np.testing.assert_array_equal(idx, cm.cheapest(cost, n))
    assert cost[TIES[0]] == cost[TIES[1]] == cost[TIES[2]] and not np.isfinite(cost[NAN_ROW])
    if n == K:
        assert idx[-1] == NAN_ROW and sorted(idx) == list(range(K))
        at = [int(np.where(idx == k)[0][0]) for k in TIES]
        assert at[1] == at[0] + 1 and at[2] == at[0] + 2  # the lower index comes first
        np.testing.assert_array_equal(traj[at[0]], traj[at[1]])
    fine = idx != NAN_ROW
    scale = cc._r(c["u_scale"])
    want = cm.rollout(c["dyn"], c["state"], scale * pa[idx[fine]], c["dt"])
    rst = cm.rollout32(c["dyn"], c["state"], F(c["u_scale"]) * pa[idx[fine]].astype(F), c["dt"])
    big = np.maximum(np.maximum.accumulate(np.abs(want), axis=1), np.abs(cc.rounded(c["state"])))
    ratio, ok = cm.held(traj[fine], want, rst, big, big)
    print(f"callback models trajectory {name}-n{n}: ratio {ratio:.4g}")
    assert ok, ratio
    # the default n is the callers' max(10, K // 10)
    if n == 10:
        d_traj, d_idx = ctrl.get_sampled_trajectories(c["state"], noise=noise)
        assert d_idx.shape == (max(10, K // 10),)
        np.testing.assert_array_equal(d_idx[:10], idx)
        np.testing.assert_array_equal(d_traj[:10], traj)


def test_get_trajectories_is_command_then_the_two_getters():
    c = cm.cases()["spread-dynamic-K257-T25"]
    a, b = _ctrl(c), _ctrl(c)
    a.U = b.U = c["U"]
    state = c["state"]
    for it in range(2):  # in-kernel noise of iteration 0 and 1, then an injected tensor
        opt, fan = a.get_trajectories(state)
        b.command(state)
        np.testing.assert_array_equal(opt, b.get_optimal_trajectory(state))
        want, idx = b.get_sampled_trajectories(state)
        np.testing.assert_array_equal(fan, want)
        assert fan.shape == (25, c["T"], 4) and opt.shape == (c["T"], 4)
        np.testing.assert_array_equal(idx, cm.cheapest(b.cost_total, 25))
        np.testing.assert_array_equal(b.perturbed_action, a.perturbed_action)
        # the cheapest sample's trajectory is the rollout of its perturbed action (K small enough to check it all here)
        np.testing.assert_array_equal(a.get_sampled_trajectories(state, n=c["K"])[0][:25], fan)
    noise = _cuda(c["noise"])
    opt, fan = a.get_trajectories(state, noise=noise)
    b.command(state, noise=noise)
    np.testing.assert_array_equal(opt, b.get_optimal_trajectory(state))
    np.testing.assert_array_equal(fan, b.get_sampled_trajectories(state, noise=noise)[0])


CALLERS = {  # the three scripts' constructor arguments
    "racecar": dict(nx=4, sigma=[[0.05, 0.0], [0.0, 0.05]], K=200, T=50, kw=dict(u_min=[-0.5, -1.0], u_max=[0.5, 1.0]),
                    state=[0.0, 0.0, 0.0, 0.0]),                                 # test/test_mppi_racecar.py:165-186
    "racecar_dynamic": dict(nx=4, sigma=(0.1 * np.eye(2)).tolist(), K=2000, T=50, kw=dict(u_min=[-1.0, -0.5], u_max=[1.0, 0.5]),
                            state=[0.0, 0.0, 0.0, 1.0]),                         # test/test_torch_mppi_race_car.py:63-79
    "double_integrator": dict(nx=2, sigma=[[0.5]], K=1000, T=20, kw=dict(u_min=[-2.0], u_max=[2.0]), state=[1.0, 0.0]),
}                                                                                # test/test_torch_mppi.py:31-44


@pytest.mark.parametrize("dyn", list(CALLERS))
def test_the_callers_loops_can_be_written(dyn):
    """command -> plant step -> get_trajectories with the scripts' own arguments: shapes, bounds, finite numbers, and a cost
    that the loop brings down."""
    from dnn_mppi_mpc_amd.callback_mppi import MPPI, RunningCost, TerminalCost
    p = CALLERS[dyn]
    term = TerminalCost.double_integrator() if dyn == "double_integrator" else None
    ctrl = MPPI(dyn, getattr(RunningCost, dyn)(), p["nx"], np.array(p["sigma"]), num_samples=p["K"], horizon=p["T"], lambda_=1.0,
                terminal_state_cost=term, seed=SEED, **p["kw"])
    state = np.array(p["state"], F)
    first = None
    for it in range(12):
        a = ctrl.command(state)
        assert a.shape == (cm.NU[dyn],) and (np.abs(a) <= np.array(p["kw"]["u_max"]) + 1e-6).all()
        state = cm.dynamics32(dyn, state[None], a[None].astype(F), cm.DT[dyn])[0]
        opt, fan = ctrl.get_trajectories(state)
        assert opt.shape == (p["T"], p["nx"]) and fan.shape == (max(10, p["K"] // 10), p["T"], p["nx"])
        assert np.isfinite(opt).all() and np.isfinite(fan).all() and np.isfinite(ctrl.cost_total).all()
        first = float(ctrl.cost_total.min()) if first is None else first
    if dyn == "double_integrator":
        assert float(ctrl.cost_total.min()) < first


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_usable_handle():
    import dnn_mppi_mpc_amd as pkg
    c = cm.cases()["racecar-K256-T7-free"]
    noise = _cuda(c["noise"])
    used, fresh = _ctrl(c), _ctrl(c)
    used.U = fresh.U = c["U"]
    state = c["state"]
    for call in (lambda: used.perturbed_action, lambda: used.get_sampled_trajectories(state),
                 lambda: used.get_sampled_trajectories(state, n=3, noise=noise)):  # before the first command
        with pytest.raises(pkg.MppiError) as e:
            call()
        assert e.value.code == -7  # MPPI_ERR_STATE
    want = fresh.command(state, noise=noise)
    np.testing.assert_array_equal(used.command(state, noise=noise), want)
    for n in (0, c["K"] + 1, -1):
        with pytest.raises(pkg.MppiError) as e:
            used.get_sampled_trajectories(state, n=n, noise=noise)
        assert e.value.code == -2  # MPPI_ERR_SHAPE
    for call in (lambda: used.perturbed_action, lambda: used.get_sampled_trajectories(state, n=3)):
        with pytest.raises(pkg.MppiError) as e:  # the last command's noise was injected: it has to be handed in again
            call()
        assert e.value.code == -7
    with pytest.raises(ValueError):
        used.get_perturbed_action(noise[:-1].contiguous())
    with pytest.raises(ValueError):
        _ctrl(c, u_scale=0.0)
    with pytest.raises(ValueError):
        _ctrl(c, u_per_command=c["T"] + 1)
    with pytest.raises(pkg.MppiError) as e:
        _ctrl(c, model_params=[0.0])
    assert e.value.code == -1  # MPPI_ERR_BAD_ARG
    with pytest.raises(NotImplementedError):
        _ctrl(c, rollout_samples=2)
    # the handle that saw the refusals goes on as one that did not
    tr_u, idx_u = used.get_sampled_trajectories(state, n=c["K"], noise=noise)
    tr_f, idx_f = fresh.get_sampled_trajectories(state, n=c["K"], noise=noise)
    np.testing.assert_array_equal(idx_u, idx_f)
    np.testing.assert_array_equal(tr_u, tr_f)
    np.testing.assert_array_equal(used.get_perturbed_action(noise), fresh.get_perturbed_action(noise))
    np.testing.assert_array_equal(used.command(state), fresh.command(state))
    np.testing.assert_array_equal(used.perturbed_action, fresh.perturbed_action)  # (in-kernel now: no tensor needed)
    np.testing.assert_array_equal(used.cost_total, fresh.cost_total)
    _ctrl(c, u_per_command=c["T"])
    _ctrl(c, model_params=[0.25])
