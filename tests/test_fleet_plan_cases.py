"""CPU: the scenes of tests/fleet_plan_checks.py do what the GPU tests need them to do -- on the f64 reference alone the mates'
plans decide samples that neither the constant-velocity rows, nor no mates, nor mates frozen where they stand decide the same
way, and few samples sit on the threshold -- and the definition `plans` agrees with the closed forms."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import fleet_plan_checks as pc
import moving_obstacle_checks as mc

K = mc.K_CASE


@functools.lru_cache(maxsize=None)
def runs_of(model, T, accumulate, mode, what, own=False):
    """(the noise the GPU tests' handles draw: their seeds, oracle/philox.py)"""
    sc = pc.arc_scene(T, accumulate) if model == "diff" else pc.race_curve_scene()
    B = len(sc["refs"])
    sigma = mc.DIFF_KW["sigma"] if model == "diff" else np.array([[0.5, 0.0], [0.0, 0.1]])
    eps = fc.numpy_noise(sigma, pc.eps_seed(T, accumulate, mode) if model == "diff" else 7, 0, B, K, T)
    return pc.one_iteration(sc, eps, K, T, mode, accumulate, what=what, own=pc.arc_own(sc) if own else None)


def four_conditions(model, T, accumulate, mode):
    plan = runs_of(model, T, accumulate, mode, "plan")
    hit = pc.penalised_of(plan)
    shares = {what: float((hit != pc.penalised_of(runs_of(model, T, accumulate, mode, what))).mean()) for what in ("cv", "none", "frozen0")}
    left = max(float((o.sample_margin() <= mc.MARGIN).mean()) for o, _ in plan)  # (every agent: the GPU tests compare them all)
    print(f"{model} T={T} acc={accumulate} {mode}: penalised {hit.mean():.3f} decided against {shares} left out {left:.4f}")
    return shares, left


@pytest.mark.parametrize("T,accumulate,mode", pc.arc_cases())
def test_arc_scene_needs_the_plans(T, accumulate, mode):
    shares, left = four_conditions("diff", T, accumulate, mode)
    for what, share in shares.items():
        assert share >= 1.0 / 16.0, (what, share)
    assert left <= mc.MAX_LEFT_OUT


@pytest.mark.parametrize("T,accumulate", [(50, True), (65, False)])
def test_arc_scene_with_own_circles_keeps_its_samples(T, accumulate):
    plan = runs_of("diff", T, accumulate, "frozen", "plan", own=True)
    assert max(float((o.sample_margin() <= mc.MARGIN).mean()) for o, _ in plan) <= mc.MAX_LEFT_OUT
    assert pc.penalised_of(plan).mean() >= 1.0 / 16.0


def test_race_pair_on_the_curve_needs_the_plans():
    shares, left = four_conditions("race", mc.RACE_T, True, "frozen")
    for what, share in shares.items():
        assert share >= 1.0 / 16.0, (what, share)
    assert left <= mc.MAX_LEFT_OUT


def test_plan_of_a_straight_line():
    T, dt = 50, 0.1
    u = np.tile(np.array([1.3, 0.0]), (1, T, 1))
    P = pc.plans([[0.5, -2.0, 0.7]], u, "diff", pc.plan_cfg("diff"))[0]
    j = np.arange(T + 1)
    want = np.array([0.5, -2.0]) + (1.3 * dt * j)[:, None] * np.array([np.cos(0.7), np.sin(0.7)])
    np.testing.assert_allclose(P, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("T", [7, 65, 128])
def test_plan_of_a_constant_turn_rate_is_eulers_polygon(T):
    """v and omega constant: the Euler steps are chords of equal length, each turned by theta = omega dt against the last --
    the sums of cos / sin over an arithmetic progression of angles."""
    dt, v, w, yaw0 = 0.1, 2.0, -0.6, 0.3
    u = np.tile(np.array([v, w]), (1, T, 1))
    P = pc.plans([[1.0, 2.0, yaw0]], u, "diff", pc.plan_cfg("diff"))[0]
    j = np.arange(T + 1)
    th = w * dt
    amp = v * dt * np.sin(0.5 * j * th) / np.sin(0.5 * th)
    want = np.stack([1.0 + amp * np.cos(yaw0 + 0.5 * (j - 1) * th), 2.0 + amp * np.sin(yaw0 + 0.5 * (j - 1) * th)], axis=1)
    np.testing.assert_allclose(P, want, rtol=0, atol=1e-12)


def test_plan_clamps_where_the_rollout_does():
    u = np.array([[[9.0, 7.0], [-9.0, -7.0]]])
    lim = np.array([[[5.0, 3.14], [-5.0, -3.14]]])
    cfg = pc.plan_cfg("diff")
    assert np.array_equal(pc.plans([[0.0, 0.0, 0.0]], u, "diff", cfg), pc.plans([[0.0, 0.0, 0.0]], lim, "diff", cfg))
    assert not np.array_equal(pc.plans([[0.0, 0.0, 0.0]], u, "diff", pc.plan_cfg("diff", clamp=False)), pc.plans([[0.0, 0.0, 0.0]], lim, "diff", cfg))


def test_race_plan_follows_the_bicycle():
    """One step by hand, then the speed ramp: x moves with the speed before the step, the speed with the acceleration."""
    cfg = pc.plan_cfg("race")
    u = np.tile(np.array([0.2, 1.0]), (1, 3, 1))
    P = pc.plans([[0.0, 0.0, 0.0, 4.0]], u, "race", cfg)[0]
    np.testing.assert_allclose(P[1], [4.0 * 0.05, 0.0], atol=1e-15)
    yaw1 = 4.0 / 2.5 * np.tan(0.2) * 0.05
    np.testing.assert_allclose(P[2], [0.2 + 4.05 * np.cos(yaw1) * 0.05, 4.05 * np.sin(yaw1) * 0.05], atol=1e-15)


def test_error_model_covers_an_f32_restatement():
    """The model against a sequential f32 restatement of the definition (not the kernel's association, but the same roundings
    per step): every point inside its bound, and the bound within a few hundred f32 spacings of the coordinates."""
    sc = pc.scatter_scene("diff", 5, 128)
    cfg = pc.plan_cfg("diff")
    f = np.float32
    x, v = sc["x0"].astype(f), pc.clamped(sc["u"].astype(f), cfg).astype(f)
    dt = f(cfg["dt"])
    got = np.empty((5, 129, 2))
    for a in range(5):
        px, py, yaw = x[a]
        got[a, 0] = px, py
        for j in range(128):
            px, py, yaw = f(px + f(f(v[a, j, 0] * np.cos(yaw, dtype=f)) * dt)), f(py + f(f(v[a, j, 0] * np.sin(yaw, dtype=f)) * dt)), f(yaw + f(v[a, j, 1] * dt))
            got[a, j + 1] = px, py
    worst = pc.check_plans(got, sc["x0"], sc["u"].astype(f), "diff", cfg, "f32")
    bound = pc.plan_bounds(sc["x0"], sc["u"], "diff", cfg, "f32")
    print("f32 restatement: largest error / bound", worst, "largest bound", bound.max())
    assert bound.max() < 0.05
