"""CPU: the references and case tables of tests/callback_models_checks.py, from the references alone -- conditions, not
measurements.  A case that misses one is moved and the move is written down in that module's docstring (MOVED), as
tests/mlp_scene_checks.py does with TUNE."""
import numpy as np
import pytest

import callback_checks as cc
import callback_models_checks as cm

F = np.float32


@pytest.mark.parametrize("name", list(cm.cases()))
def test_case_states_its_conditions(name):
    """Left-out samples <= EXCLUDED_CAP, inverse-cost cases meet ACTIVE_FLOOR, spread cases ESS_FLOOR, dynamic cases keep
    v cos(delta) >= 1, and the f32 restatement is as near the f64 definition as the error rule assumes."""
    cm.check_case(name)


def test_case_table_covers_the_shapes():
    cs = cm.cases().values()
    for dyn in cm.NX:
        mine = [c for c in cs if c["dyn"] == dyn and c["family"] != "option"]
        assert {1, 255, 256, 257} <= {c["K"] for c in mine}, dyn
        assert {1, 7, 25} <= {c["T"] for c in mine}, dyn
        assert any(c["null"] for c in mine) and any(not c["bounded"] for c in mine) and any(c["terminal"] for c in mine), dyn
        assert any(c["family"] == "spread" for c in mine) and any(c["u_init"].any() for c in mine), dyn
    assert any(c["T"] * cm.NU[c["dyn"]] == 256 for c in cs if c["dyn"] == "double_integrator")
    assert any(c["T"] * cm.NU[c["dyn"]] == 256 for c in cs if c["dyn"] == "racecar_dynamic")
    assert all(c["T"] <= 25 for c in cs if c["dyn"] == "racecar")


def test_every_new_term_moves_the_cost_beyond_the_tolerance():
    """The terminal term, noise_abs_cost against the signed term, u_scale = 0.5 against 1 and noise_mu != 0 against 0 each change
    cost_total by more than ten times the GPU test's tolerance for at least half of the kept samples: a dropped or mis-wired
    term cannot hide inside the bound."""
    b = cm.OPTION_BASE
    c = cm.cases()[b]
    shares = dict(terminal=cm.term_moves_the_cost(b, terminal=cm.TERMINAL["racecar"]),
                  abs_cost=cm.term_moves_the_cost(b, abs_cost=True),
                  u_scale=cm.term_moves_the_cost(b, u_scale=cm.OPTION_SCALE),
                  noise_mu=cm.term_moves_the_cost(b, noise=c["noise"] + cm.OPTION_MU.astype(F)))
    assert min(shares.values()) >= 0.5, shares
    # ... and in every case with a terminal cost the term is there to be missed
    for name, case in cm.cases().items():
        if case["terminal"] is not None and case["K"] > 1:
            assert cm.term_moves_the_cost(name, terminal=None) >= 0.5, name


def test_the_two_deliberate_breaks_are_visible_to_the_reference():
    """What the broken builds compute (the racecar's controls swapped; the terminal cost priced one step early) is further
    from the reference than ten tolerances for half the samples of every case they should fail, so running the GPU file
    against them must fail those cases."""
    for name, c in cm.cases().items():
        if c["K"] == 1:
            continue
        ref, _ = cm.reference(name)
        tol = cc.COST_FACTOR * cm.restatement_distance(name) * np.maximum(np.abs(ref["cost_total"]), 1.0)
        if c["dyn"] == "racecar":
            broken = cm.command(c, c["state"], c["U"], c["noise"], swap_controls=True)
            assert (np.abs(broken["cost_total"] - ref["cost_total"]) > 10 * tol)[ref["keep"]].mean() >= 0.5, name
        if c["terminal"] is not None:
            broken = cm.command(c, c["state"], c["U"], c["noise"], terminal_before_last=True)
            assert (np.abs(broken["cost_total"] - ref["cost_total"]) > 10 * tol)[ref["keep"]].mean() >= 0.5, name


@pytest.mark.parametrize("dyn", list(cm.NX))
def test_model_rows_and_restatement(dyn):
    """The rows for `mppi_cb_eval`: finite, off the inverse cost's step, v cos(delta) >= 1 for the dynamic model, and the f32
    restatement of the step within a few roundings of the f64 definition."""
    cost = cm.cost_of(dyn)
    for n in cm.MODEL_N:
        s, a = cm.model_rows(dyn, n)
        assert s.shape == (n, cm.NX[dyn]) and a.shape == (n, cm.NU[dyn])
        want, largest = cm.dynamics(dyn, s, a, cm.DT[dyn])
        rst = cm.dynamics32(dyn, s, a, cm.DT[dyn])
        assert np.isfinite(want).all() and rst.dtype == F
        dist = np.max(np.abs(rst - want) / np.maximum(np.abs(want), largest))
        assert dist <= 8 * cc.EPS, (dyn, n, dist)
        if n > 1:
            assert dist > 0, (dyn, n)
        if dyn == "racecar_dynamic":
            assert (cc.rounded(s)[:, 3] * np.cos(cc.rounded(a)[:, 1])).min() >= cm.V_COS_FLOOR
        if dyn == "racecar" and n >= 8:
            _, _, d = cc.running_cost(s, a, 0, cost)
            assert (np.abs(d - cc._r(cost["safety"])) > 1e-5).all()
            assert (d[:8, 0] < cost["safety"]).all()
        t, big = cm.terminal_cost(s, cm.TERMINAL[dyn])
        np.testing.assert_allclose(cm.terminal_cost32(s, cm.TERMINAL[dyn]), t, rtol=8 * cc.EPS)
        assert (big <= t).all() and (t <= cm.NX[dyn] * big).all()


def test_models_follow_the_issue_table():
    """Spot values by hand: one step of each model from a state whose increments can be read off."""
    s, _ = cm.dynamics("double_integrator", [[1.0, 2.0]], [[3.0]], 0.1)
    np.testing.assert_allclose(s, [[1.0 + cc._r(0.1) * 2.0, 2.0 + cc._r(0.1) * 3.0]], rtol=1e-15)
    s, _ = cm.dynamics("racecar", [[0.0, 0.0, 0.0, 2.0]], [[0.25, 1.0]], 0.05)
    dt, L = cc._r(0.05), cc._r(0.3)
    np.testing.assert_allclose(s, [[2.0 * dt, 0.0, 2.0 / L * np.tan(0.25) * dt, 2.0 + dt]], rtol=1e-15)
    sw, _ = cm.dynamics("racecar", [[0.0, 0.0, 0.0, 2.0]], [[1.0, 0.25]], 0.05, swap_controls=True)
    np.testing.assert_array_equal(sw, s)
    # the dynamic model with theta = 0: atan2(v sin d, v cos d) = d, so alpha_f = 0 and alpha_r = d: v += (acc - C_r d / m) dt
    s, _ = cm.dynamics("racecar_dynamic", [[1.0, 2.0, 0.0, 3.0]], [[0.5, 0.25]], 0.05)
    np.testing.assert_allclose(s, [[1.0 + 3.0 * dt, 2.0, 3.0 / 1.5 * np.sin(0.25) * dt, 3.0 + (0.5 - 0.25) * dt]], rtol=1e-12)
    # ... and with theta != 0 the yaw enters the slip angles as the script has it
    th, v, d = 0.5, 3.0, 0.25
    af = np.arctan2(v * np.sin(d) + 1.0 * th, v * np.cos(d)) - d
    ar = np.arctan2(v * np.sin(d) - 1.5 * th, v * np.cos(d))
    s, _ = cm.dynamics("racecar_dynamic", [[0.0, 0.0, th, v]], [[0.5, d]], 0.05)
    np.testing.assert_allclose(s[0, 3], v + (0.5 - (1000.0 * af * np.sin(d) + 1000.0 * ar) / 1000.0) * dt, rtol=1e-12)


def test_rank_is_a_permutation_that_agrees_with_a_stable_argsort():
    rng = np.random.default_rng(5)
    vectors = [np.array([3.0]), np.array([np.nan]), np.zeros(7), np.array([0.0, -0.0, 0.0]), np.full(5, np.nan),
               np.array([2.0, np.nan, 1.0, np.nan, 1.0, np.inf, -np.inf, 2.0])]
    for K in (255, 257):
        c = rng.normal(size=K).astype(F).astype(np.float64)
        c[rng.integers(0, K, 40)] = c[rng.integers(0, K, 40)]  # ties
        c[rng.integers(0, K, 9)] = np.nan
        c[rng.integers(0, K, 3)] = np.inf
        vectors.append(c)
    for c in vectors:
        r = cm.ranks(c)
        assert sorted(r) == list(range(c.size))
        order = np.argsort(c, kind="stable")  # NumPy sorts NaN last, and a stable sort keeps equal keys in index order
        np.testing.assert_array_equal(cm.cheapest(c, c.size), order)
        np.testing.assert_array_equal(cm.cheapest(c, 1), order[:1])
        nan = np.isnan(c)
        if nan.any() and not nan.all():
            assert r[nan].min() > r[~nan].max()


def test_command_reduces_to_the_existing_reference_without_the_new_terms():
    """With no terminal cost, u_scale = 1 and the signed perturbation term the f64 command here is callback_checks.command's
    loop around another model: same shift, clamp, noise taken back, softmin and update (checked on the double integrator by
    hand: cost_total = sum of squares + perturbation term)."""
    c = dict(cm.cases()["double-K256-T25-free-null"])
    ref = cm.command(c, c["state"], c["U"], c["noise"])
    U, act, nz = cm.clamped(c, c["U"], c["noise"])
    s = np.tile(cc.rounded(c["state"]), (c["K"], 1))
    total = np.zeros(c["K"])
    dt = cc._r(c["dt"])
    for t in range(c["T"]):
        s = np.stack([s[:, 0] + dt * s[:, 1], s[:, 1] + dt * act[:, t, 0]], axis=1)
        total += (s ** 2).sum(1) + act[:, t, 0] ** 2
    total += (U[None] * nz * 2.0).sum(axis=(1, 2))  # lambda = 1, Sigma^-1 = 1 / 0.5
    np.testing.assert_allclose(ref["cost_total"], total, rtol=1e-12)
    assert (act[-1] == 0).all() and ref["terminal"].max() == 0
    om, _ = cc.softmin(total, 1.0)
    np.testing.assert_allclose(ref["omega"], om, rtol=1e-9, atol=1e-300)
