"""CPU: the cases of tests/grid_footprint_checks.py are what they claim -- the outline decides samples the centre spares, some
are spared by both, the outline's extra soft cost shows, the margin rule leaves out next to nothing, an f32 ulp of position or
yaw moves S by less than a quarter of the f32 tolerance -- and g_foot holds by hand for three poses."""
import functools

import numpy as np
import pytest

import grid_footprint_checks as fc

K = fc.K_CASE


@functools.lru_cache(maxsize=None)
def case(T, accumulate, mode):
    return fc.diff_case(T, accumulate, mode)


@functools.lru_cache(maxsize=None)
def race():
    return fc.race_case()


def check_case(o, res):
    S = np.asarray(res["S"], np.float64)
    foot, centre, extra = o.sample_grid_lethal(), o.sample_centre_lethal(), o.sample_extra_term()
    only_outline, spared = foot & ~centre, ~foot & ~centre
    shows = extra > 10.0 * fc.f32_tolerance(S)
    left_out = 1.0 - fc.kept(o, False).mean()
    print("outline alone", only_outline.mean(), "centre", centre.mean(), "spared by both", spared.mean(),
          "extra term shows on", (shows & spared).sum() / max(spared.sum(), 1), "of the spared", "left out", left_out)
    assert not (centre & ~foot).any()  # the centre is one of the nine points
    assert only_outline.sum() * 16 >= K  # sampling the centre only must fail
    assert spared.sum() * 16 >= K
    assert np.array_equal(fc.penalised(S), foot | o.sample_circle_hit())
    assert 2 * (shows & spared).sum() >= spared.sum()  # pricing weight * g(centre) must fail
    assert left_out <= fc.MAX_LEFT_OUT


@pytest.mark.parametrize("T,accumulate,mode", fc.diff_cases())
def test_diff_case_is_what_it_claims(T, accumulate, mode):
    sc, eps, o, res = case(T, accumulate, mode)
    assert len(sc["circles"]) == 0  # (the diff-drive oracle has no outline test against circles)
    check_case(o, res)


def test_race_case_is_what_it_claims():
    sc, eps, o, res = race()
    assert len(sc["circles"]) == 2
    check_case(o, res)


def moved(make, S0, o0):
    """S of the reference with every position, then every yaw, moved by +-1 f32 ulp, against a quarter of the f32 tolerance, on
    the samples no decision of which lies inside the margin (a flipped decision moves S by the penalty)"""
    worst = 0.0
    for kw in (dict(shift=+1), dict(shift=-1), dict(shift_yaw=+1), dict(shift_yaw=-1)):
        _, _, o, res = make(**kw)
        keep = fc.kept(o, False) & fc.kept(o0, False)
        S = np.asarray(res["S"], np.float64)
        assert np.array_equal(fc.penalised(S)[keep], fc.penalised(S0)[keep])
        ratio = np.abs(S - S0)[keep] / (0.25 * fc.f32_tolerance(S0)[keep])
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("T,accumulate,mode", fc.diff_cases())
def test_an_f32_ulp_of_position_or_yaw_stays_inside_the_tolerance(T, accumulate, mode):
    _, _, o0, res0 = case(T, accumulate, mode)
    worst = moved(lambda **kw: fc.diff_case(T, accumulate, mode, **kw), np.asarray(res0["S"], np.float64), o0)
    print("largest |dS| / (tolerance / 4):", worst)
    assert worst <= 1.0


def test_an_f32_ulp_of_position_or_yaw_stays_inside_the_tolerance_race():
    _, _, o0, res0 = race()
    worst = moved(lambda **kw: fc.race_case(**kw), np.asarray(res0["S"], np.float64), o0)
    print("largest |dS| / (tolerance / 4):", worst)
    assert worst <= 1.0


def test_the_points_and_g_foot_by_hand():
    """A ramp g = x on a 9 x 9 grid of 1 m cells over [-4, 4]^2, a box of half-sides a = 2, b = 1."""
    cells = np.broadcast_to(np.arange(-4.0, 5.0), (9, 9)).copy()
    grid = fc.Grid(cells, (-4.0, -4.0), 1.0)
    a, b = 2.0, 1.0
    # yaw 0 at the origin: the front points (a, .) carry the largest x
    p = fc.world_points(np.float64(0.0), np.float64(0.0), np.float64(0.0), a, b)
    assert p.tolist() == [[0, 0], [-2, 0], [-2, 1], [0, 1], [2, 1], [2, 0], [2, -1], [0, -1], [-2, -1]]
    g, g0 = fc.footprint_value(grid, np.float64(0.0), np.float64(0.0), np.float64(0.0), a, b)
    assert g == 2.0 and g0 == 0.0
    # yaw pi / 2 at (1, -1): the body's x axis points along +y, its left (+b) along -x; the right side reaches x = 1 + b
    p = fc.world_points(np.float64(1.0), np.float64(-1.0), np.float64(np.pi / 2), a, b)
    np.testing.assert_allclose(p, [[1, -1], [1, -3], [0, -3], [0, -1], [0, 1], [1, 1], [2, 1], [2, -1], [2, -3]], atol=1e-15)
    g, g0 = fc.footprint_value(grid, np.float64(1.0), np.float64(-1.0), np.float64(np.pi / 2), a, b)
    assert g == pytest.approx(2.0, abs=1e-15) and g0 == 1.0
    # yaw pi at (3.5, 0): the rear points lie ahead in x, at 5.5 -- outside the grid, where the edge value 4 continues
    g, g0 = fc.footprint_value(grid, np.float64(3.5), np.float64(0.0), np.float64(np.pi), a, b)
    assert g == 4.0 and g0 == 3.5
    # a lone peak under one corner: yaw 0 at (-2, -1) puts point 4 = (a, b) on node (0, 0)
    peak = np.zeros((9, 9))
    peak[4, 4] = 7.0
    g, g0 = fc.footprint_value(fc.Grid(peak, (-4.0, -4.0), 1.0), np.float64(-2.0), np.float64(-1.0), np.float64(0.0), a, b)
    assert g == 7.0 and g0 == 0.0
