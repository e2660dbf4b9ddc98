"""CPU: conditions on the one-iteration cases of tests/mlp_fleet_checks.py, of the f64 reference alone -- the mates decide a real
share of agent 0's samples, the learned plan decides otherwise than the analytic plan (and than the plan through the wrong
model), and the margin rule leaves out next to nothing -- and two identities of the reference itself."""
import numpy as np
import pytest

import fleet_plan_checks as fp
import mlp_fleet_checks as mf
import mlp_scene_checks as ms
import moving_obstacle_checks as mc
import scene_checks as sk

SHARE = 1.0 / 16.0
CASES = mf.cases()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_mates_plans_decide_and_differ(case):
    T, accumulate, mode, H, n, per_agent = case
    sc, _, eps, runs = mf.case(*case)
    hit = mf.penalised_of(runs)
    print(case, "penalised", hit.mean())
    assert SHARE <= hit.mean() <= 1.0 - SHARE
    analytic = mf.one_iteration(sc, eps, T, mode, accumulate, plans=fp.plans(sc["x0"], sc["u"], "diff", fp.plan_cfg("diff")))
    assert (hit != mf.penalised_of(analytic)).mean() >= SHARE
    if per_agent:
        wrong = mf.one_iteration(sc, eps, T, mode, accumulate, plans=mf.learned_plans(sc["x0"], sc["u"], [sc["w"][0]] * 3))
        assert (hit != mf.penalised_of(wrong)).mean() >= SHARE
    for what in ("plan", "velocity"):
        for a, (o, _) in enumerate(mf.case(*case, what=what)[3]):
            assert (~mf.kept(o)).mean() <= mf.MAX_LEFT_OUT, (what, a)


@pytest.mark.parametrize("what", ["plan", "velocity"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_the_outline_scene_decides_a_share_and_leaves_out_little(accumulate, what):
    sc = mf.outline_scene(50)
    runs = mf.one_iteration(sc, mf.numpy_noise(50), 50, "frozen", accumulate, what)
    assert SHARE <= mf.penalised_of(runs).mean() <= 1.0 - SHARE
    assert isinstance(runs[0][0], mf.LearnedFleetOutlineOracle) and runs[0][0].outline
    for a, (o, _) in enumerate(runs):
        assert (~mf.kept(o)).mean() <= mf.MAX_LEFT_OUT, a
    disc = mf.one_iteration(dict(sc, outline=False), mf.numpy_noise(50), 50, "frozen", accumulate, what)
    assert (mf.penalised_of(runs) != mf.penalised_of(disc)).mean() >= SHARE  # the outline decides otherwise than the disc


@pytest.mark.parametrize("mode", ["frozen", "per_rollout"])
@pytest.mark.parametrize("T,accumulate", [(50, False), (50, True)])
def test_velocity_mode_decides_a_share_of_some_agent(T, accumulate, mode):
    runs = mf.case(T, accumulate, mode, what="velocity")[3]
    shares = [mf.penalised_of(runs, a).mean() for a in range(3)]
    assert any(SHARE <= s <= 1.0 - SHARE for s in shares), shares


def test_own_circles_keep_the_margin_rule():
    for what in ("plan", "velocity"):
        sc, own, eps, runs = mf.case(50, True, "frozen", what=what, with_own=True)
        for a, (o, _) in enumerate(runs):
            assert (~mf.kept(o)).mean() <= mf.MAX_LEFT_OUT, (what, a)


def test_a_far_apart_fleet_gives_the_scene_handles_costs_exactly():
    """nobody in reach: every agent's S is what mlp_scene_checks' oracle gives for the agent alone"""
    T, B = 20, 3
    sc = mf.far_scene(B, T)
    eps = mf.numpy_noise(T, B)
    for what in ("plan", "velocity"):
        runs = mf.one_iteration(sc, eps, T, "frozen", False, what)
        for a, (_, res) in enumerate(runs):
            o = sk.aim(ms.scene_oracle(sc["refs"][a], sc["u"][a], mf.K, T, sc["w"][a]), {})
            alone = o.iteration_general(sc["x0"][a], eps[a].astype(np.float64), "frozen", False)
            assert np.array_equal(res["S"], alone["S"]) and not mc.penalised(res["S"]).any(), (what, a)


def test_learned_plans_with_a_zeroed_output_layer_are_the_analytic_plans():
    sc = fp.scatter_scene("diff", 3, 50)
    w = [mf.zeroed(ms.weights(64, 1, 100 + a)) for a in range(3)]
    got, want = mf.learned_plans(sc["x0"], sc["u"], w), fp.plans(sc["x0"], sc["u"], "diff", fp.plan_cfg("diff"))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_the_composed_scene_prices_every_ingredient_and_the_mates():
    """tracks, a grid, own circles and the mates' plans on agent 0: each hits a share by itself, and the mates alone decide a
    share of agent 1, which owns nothing"""
    sc = mf.composed_scene()
    runs = mf.composed_iteration(sc, mf.numpy_noise(50))
    o = runs[0][0]
    for part in ("circles", "tracks", "plans"):
        share = np.concatenate(o.part_hits[part], axis=1).any(axis=1).mean()
        assert SHARE <= share <= 1.0 - SHARE, (part, share)
    assert SHARE <= mf.penalised_of(runs, 1).mean() <= 1.0 - SHARE
    assert (~ms.kept(o)).mean() <= mf.MAX_LEFT_OUT and all((~mf.kept(r[0])).mean() <= mf.MAX_LEFT_OUT for r in runs[1:])
