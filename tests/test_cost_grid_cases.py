"""CPU: the cases of tests/cost_grid_checks.py are what they claim -- the grid decides, its soft cost shows, the margin rule
leaves out next to nothing, an f32 ulp of position moves S by less than a quarter of the f32 tolerance -- and the bilinear
formula holds by hand at nodes, mid-cell, on edges, outside and at non-finite points."""
import functools

import numpy as np
import pytest

import cost_grid_checks as gc

K = gc.K_CASE


@functools.lru_cache(maxsize=None)
def case(T, accumulate, mode, grid):
    return gc.diff_case(T, accumulate, mode, grid)


def check_case(o, res, circles_decide):
    S = np.asarray(res["S"], np.float64)
    lethal, term = o.sample_grid_lethal(), o.sample_grid_term()
    spared = ~lethal
    shows = term > 10.0 * gc.f32_tolerance(S)
    only_circle = o.sample_circle_hit() & spared
    left_out = 1.0 - gc.kept(o, False).mean()
    print("lethal", lethal.mean(), "spared", spared.mean(), "term shows on", (shows & spared).sum() / spared.sum(), "of the spared",
          "circles alone decide", only_circle.mean(), "left out", left_out)
    assert lethal.sum() * 16 >= K and spared.sum() * 16 >= K
    assert np.array_equal(gc.penalised(S), lethal | o.sample_circle_hit())
    assert 2 * (shows & spared).sum() >= spared.sum()  # dropping weight * g must fail
    assert left_out <= gc.MAX_LEFT_OUT
    if circles_decide:
        assert only_circle.sum() * 64 >= K


@pytest.mark.parametrize("T,accumulate,mode,grid", gc.diff_cases())
def test_diff_case_is_what_it_claims(T, accumulate, mode, grid):
    sc, eps, o, res = case(T, accumulate, mode, grid)
    # (T = 7: a step covers 0.43 m and with every step priced the crosser passes between two of them -- at that horizon the
    # circles are priced beside the grid but need not decide a sample it spares; DESIGN 3.12 says so)
    check_case(o, res, circles_decide=T >= 50)
    # the margin rule of the grid alone: the band |g - lethal| <= MARGIN lethal around the contour is 6e-5 m wide
    o2 = gc.diff_oracle(dict(sc, circles=np.zeros((0, 3)), vel=np.zeros((0, 2))), K, T)
    o2.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    assert (o2.sample_margin() <= gc.MARGIN).sum() <= 1


def test_race_case_is_what_it_claims():
    sc, eps, o, res = gc.race_case()
    check_case(o, res, circles_decide=True)


def moved(make, S0, o0):
    """S of the f64 reference with every position moved by +-1 f32 ulp, against a quarter of the f32 tolerance, on the samples
    no decision of which lies inside the margin (a flipped decision moves S by the penalty)"""
    worst = 0.0
    for shift in (+1, -1):
        _, _, o, res = make(shift)
        keep = gc.kept(o, False) & gc.kept(o0, False)
        S = np.asarray(res["S"], np.float64)
        assert np.array_equal(gc.penalised(S)[keep], gc.penalised(S0)[keep])
        ratio = np.abs(S - S0)[keep] / (0.25 * gc.f32_tolerance(S0)[keep])
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("T,accumulate,mode,grid", gc.diff_cases())
def test_an_f32_ulp_of_position_stays_inside_the_tolerance(T, accumulate, mode, grid):
    _, _, o0, res0 = case(T, accumulate, mode, grid)
    worst = moved(lambda s: gc.diff_case(T, accumulate, mode, grid, shift=s), np.asarray(res0["S"], np.float64), o0)
    print("largest |dS| / (tolerance / 4):", worst)
    assert worst <= 1.0


def test_an_f32_ulp_of_position_stays_inside_the_tolerance_race():
    _, _, o0, res0 = gc.race_case()
    worst = moved(lambda s: gc.race_case(shift=s), np.asarray(res0["S"], np.float64), o0)
    print("largest |dS| / (tolerance / 4):", worst)
    assert worst <= 1.0


def test_the_formula_by_hand():
    G = np.array([[0.0, 1.0, 4.0], [2.0, 3.0, 8.0], [5.0, 7.0, 6.0], [9.0, 1.0, 2.0]])  # ny = 4, nx = 3
    origin, res = (-1.0, 2.0), 0.5
    v = functools.partial(gc.grid_value, G, origin, res)
    for iy in range(4):  # a node returns its cell exactly
        for ix in range(3):
            assert v(origin[0] + res * ix, origin[1] + res * iy) == G[iy, ix]
    assert v(-0.75, 2.25) == 0.25 * (0.0 + 1.0 + 2.0 + 3.0)           # mid-cell
    assert v(-0.5, 2.75) == 0.5 * (3.0 + 7.0)                          # on an edge between two nodes
    assert v(-0.375, 3.5) == 0.75 * 1.0 + 0.25 * 2.0                   # on the grid's last row: iy = ny - 2, fy = 1
    assert v(0.0, 3.125) == 0.75 * 6.0 + 0.25 * 2.0                    # on its last column: ix = nx - 2, fx = 1
    for far in (1.0e6, -1.0e6):                                        # outside, the edge value continues
        assert v(far, 2.5) == (8.0 if far > 0 else 2.0)
        assert v(-0.5, far) == (1.0 if far > 0 else 1.0) and v(-1.0, far) == (9.0 if far > 0 else 0.0)
        assert v(far, far) == (2.0 if far > 0 else 0.0)
    assert v(np.inf, -np.inf) == 4.0 and v(-np.inf, np.inf) == 9.0     # a non-finite coordinate lands on an edge node
    assert v(np.nan, 2.5) == 2.0 and v(0.0, np.nan) == 4.0 and v(np.nan, np.nan) == 0.0  # (NaN: node 0 of its axis)
    for n in (2, 3, 4096):                                             # the index stays inside [0, n - 2], the fraction in [0, 1]
        i, f = gc.axis_index(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 1e-30, n - 1.0, n - 1.5]), 0.0, 1.0, n)
        assert i.min() >= 0 and i.max() <= n - 2 and f.min() >= 0.0 and f.max() <= 1.0
