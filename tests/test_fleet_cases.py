"""Fleet avoidance: conditions on the inputs of tests/test_gpu_fleet.py, checked on the f64 reference alone (no device)."""
import functools

import numpy as np
import pytest

import fleet_checks as fc
import moving_obstacle_checks as mc

K = mc.K_CASE


@functools.lru_cache(maxsize=None)
def case(model, T, accumulate, mode):
    sc = fc.crossing_scene(T, accumulate) if model == "diff" else fc.race_pair_scene()
    B = len(sc["refs"])
    sigma, seed = (mc.DIFF_KW["sigma"], 99) if model == "diff" else (np.array([[0.5, 0.0], [0.0, 0.1]]), 7)
    eps = fc.numpy_noise(sigma, seed, 0, B, K, T)
    runs = {name: fc.one_iteration(sc, eps, K, T, mode, accumulate, **kw)
            for name, kw in (("fleet", {}), ("alone", dict(mates=False)), ("frozen", dict(freeze_at=0)))}
    return sc, runs


CASES = [("diff", T, acc, mode) for T, acc, mode in fc.diff_cases()] + [("race", mc.RACE_T, True, "frozen")]


@pytest.mark.parametrize("model,T,accumulate,mode", CASES)
def test_the_mates_and_their_motion_decide_samples(model, T, accumulate, mode):
    sc, runs = case(model, T, accumulate, mode)
    hit = {name: np.stack([mc.penalised(res["S"]) for _, res in run]) for name, run in runs.items()}  # [B, K]
    # agent 0 and the mate that crosses its path (the last agent of the diff-drive scene runs out of reach)
    for a in (0, 1):
        by_mates = (hit["fleet"][a] != hit["alone"][a]).mean()
        by_motion = (hit["fleet"][a] != hit["frozen"][a]).mean()
        left_out = 1.0 - float(mc.kept(runs["fleet"][a][0], False).mean())
        print(model, T, accumulate, mode, "agent", a, "decided by the mates", by_mates, "by their motion", by_motion, "left out", left_out,
              "penalised", hit["fleet"][a].mean())
        assert by_mates >= 1 / 16 and by_motion >= 1 / 16
        assert left_out <= mc.MAX_LEFT_OUT
        assert not hit["alone"][a].any()
    if model == "diff":
        assert not hit["fleet"][2].any() or hit["fleet"][2].mean() < hit["fleet"][0].mean()


def test_mate_rows_against_a_closed_form_for_two_agents():
    x = np.array([[1.0, 2.0, np.pi / 6], [-3.0, 0.5, np.pi / 2]])
    u = np.array([[0.8, 0.3], [7.0, -0.1]])  # (7.0 is clamped to u_max0 = 5)
    c, v = fc.mate_rows(x, u, "diff", dict(fleet_radius=0.25, u_max0=5.0))
    assert c.shape == (2, 1, 3) and v.shape == (2, 1, 2)
    np.testing.assert_allclose(c[0, 0], [-3.0, 0.5, 0.25], rtol=0, atol=0)     # agent 0 sees agent 1
    np.testing.assert_allclose(v[0, 0], [0.0, 5.0], rtol=0, atol=5 * 2.0 ** -52)  # 5 (cos, sin)(pi / 2)
    np.testing.assert_allclose(c[1, 0], [1.0, 2.0, 0.25], rtol=0, atol=0)
    np.testing.assert_allclose(v[1, 0], [0.8 * np.sqrt(3.0) / 2.0, 0.4], rtol=0, atol=2.0 ** -52)
    xr = np.array([[1.0, 2.0, np.pi, 4.0], [0.0, 0.0, 0.0, -2.0]])  # race car: the state's v, the controls do not enter
    c, v = fc.mate_rows(xr, u, "race", dict(fleet_radius=1.0, u_max0=0.523))
    np.testing.assert_allclose(v[1, 0], [-4.0, 0.0], rtol=0, atol=4 * 2.0 ** -52)
    np.testing.assert_allclose(v[0, 0], [-2.0, 0.0], rtol=0, atol=0)
    # three agents: ascending order with oneself skipped
    x3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    c, _ = fc.mate_rows(x3, np.zeros((3, 2)), "diff", dict(fleet_radius=0.1, u_max0=5.0))
    assert [list(c[b, :, 0]) for b in range(3)] == [[1.0, 2.0], [0.0, 2.0], [0.0, 1.0]]


def test_back_dating_lands_on_the_definition():
    """table_of at clock n and mc.centres at step j give p + v dt j"""
    p, v = np.array([[3.0, -1.0, 0.4]]), np.array([[0.7, -0.2]])
    for n in (0, 3, 1000):
        c, vv = fc.table_of(np.zeros((0, 3)), np.zeros((0, 2)), p, v, 0.1, n)
        for j in (0, 1, 25):
            np.testing.assert_allclose(mc.centres(c, vv, 0.1, n, j)[0], p[0, :2] + v[0] * 0.1 * j, rtol=0, atol=1e-12)


BEHAVIOUR = dict(K=512, T=20, n_iters=45, seed=99)


@functools.lru_cache(maxsize=None)
def behaviour_reference():
    b = BEHAVIOUR
    sc = fc.head_on_scene(b["T"])
    return fc.closed_loop(sc, lambda i: fc.numpy_noise(mc.DIFF_KW["sigma"], b["seed"], i, 2, b["K"], b["T"]), b["n_iters"], b["K"], b["T"],
                          mates=False)


def test_without_avoidance_the_head_on_robots_touch():
    ref = behaviour_reference()
    d = np.array([fc.min_mate_distance(x)[0] for x in ref["x"]])
    print("smallest centre distance over the run", d.min(), "at iteration", int(d.argmin()))
    assert d.min() < 2 * fc.RADIUS


def test_error_model_is_monotone_and_small():
    assert fc.centre_bound(10.0, 5.0, fc.EPS["f32"]) < 1e-5 and fc.centre_bound(10.0, 5.0, fc.EPS["f64"]) < 1e-13
    assert fc.centre_bound(10.0, 6.0, fc.EPS["f32"]) > fc.centre_bound(10.0, 5.0, fc.EPS["f32"])
