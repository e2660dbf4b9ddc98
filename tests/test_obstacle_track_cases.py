"""CPU: every scene of tests/obstacle_track_checks.py is what it claims -- the tracks decide samples that neither a
constant-velocity extrapolation of their first two points nor the obstacles frozen where they stand decides the same way, the
f64 reference itself leaves out at most 1 % of a case's samples -- and the index clamps as the header says."""
import numpy as np
import pytest

import obstacle_track_checks as tc

SIXTEENTH = 1.0 / 16.0


@pytest.mark.parametrize("T,accumulate,mode", tc.diff_cases())
def test_diff_scene_tracks_decide(T, accumulate, mode):
    _, _, o, res = tc.diff_case(T, accumulate, mode)
    tracks = tc.penalised(res["S"])
    left_out = float((o.sample_margin() <= tc.MARGIN).mean())
    velocity = tc.penalised(tc.diff_case(T, accumulate, mode, variant="velocity")[3]["S"])
    frozen = tc.penalised(tc.diff_case(T, accumulate, mode, variant="frozen")[3]["S"])
    print(T, accumulate, mode, "penalised", tracks.mean(), "vs constant velocity", (tracks != velocity).mean(), "vs frozen",
          (tracks != frozen).mean(), "left out", left_out)
    assert 0.1 < tracks.mean() < 0.9
    assert (tracks != velocity).mean() >= SIXTEENTH
    assert (tracks != frozen).mean() >= SIXTEENTH
    assert left_out <= tc.MAX_LEFT_OUT
    assert tc.kept(o, f64=True).all()  # an f64 handle leaves out nothing


@pytest.mark.parametrize("T,accumulate,mode", tc.diff_cases())
def test_the_seed_table_holds_the_first_seed_that_meets_the_rule(T, accumulate, mode):
    """EPS_SEED records, per case, the first noise seed at which at most 1 % of the samples lie inside the margin."""
    want = tc.eps_seed(T, accumulate, mode)
    saved = dict(tc.EPS_SEED)
    try:
        for seed in range(want):
            tc.EPS_SEED[(T, accumulate, mode)] = seed
            o = tc.diff_case(T, accumulate, mode)[2]
            assert float((o.sample_margin() <= tc.MARGIN).mean()) > tc.MAX_LEFT_OUT, seed
    finally:
        tc.EPS_SEED.clear()
        tc.EPS_SEED.update(saved)


def test_race_scene_tracks_decide():
    _, _, o, res = tc.race_case()
    tracks = tc.penalised(res["S"])
    left_out = float((o.sample_margin() <= tc.MARGIN).mean())
    velocity = tc.penalised(tc.race_case(variant="velocity")[3]["S"])
    frozen = tc.penalised(tc.race_case(variant="frozen")[3]["S"])
    print("penalised", tracks.mean(), "vs constant velocity", (tracks != velocity).mean(), "vs frozen", (tracks != frozen).mean(), left_out)
    assert 0.1 < tracks.mean() < 0.9
    assert (tracks != velocity).mean() >= SIXTEENTH and (tracks != frozen).mean() >= SIXTEENTH
    assert left_out <= tc.MAX_LEFT_OUT


def test_closed_loop_scene_depends_on_the_clock():
    """Tracks alone: the trace differs from the one with the clock held.  With the own circles: tracks and circles each decide
    at least one sample in 16 of the first iteration that the other does not, the hits change under the loop, and the
    reference leaves out at most 1 % of any iteration's samples."""
    import moving_obstacle_checks as mc
    from oracle import philox
    T = 50
    tr = [tc.diff_closed_loop(T, 6, own=False, tick=t)["u0"] for t in (True, False)]
    assert np.abs(tr[0] - tr[1]).max() > 1e-3
    ref = tc.diff_closed_loop(T, 6)
    assert max(ref["n_hit"]) - min(ref["n_hit"]) > tc.K_CASE // 16 and min(ref["kept"]) >= 1.0 - tc.MAX_LEFT_OUT
    sc = ref["scene"]
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], 31, 0, tc.K_CASE, T).astype(np.float64)
    scenes = (sc, dict(sc, tracks=None, radii=np.zeros(0)), dict(sc, circles=tc.NO_CIRCLES, vel=np.zeros((0, 2))))
    both, own_only, tracks_only = [tc.penalised(tc.diff_oracle(s, tc.K_CASE, T, **mc.LOOP_KW).iteration_general(sc["x0"], eps, "frozen", True)["S"])
                                   for s in scenes]
    assert (both != own_only).mean() >= SIXTEENTH and (both != tracks_only).mean() >= SIXTEENTH


def test_the_index_clamps_by_hand():
    """A track of L = 3 at clock 5: every step reads point 2.  At clock 1: step 0 reads point 1, every later step point 2."""
    trk = np.array([[[0.0, 0.0], [1.0, 0.5], [2.0, 1.0]]])
    for j in (0, 1, 7, 200):
        assert np.array_equal(tc.track_centres(trk, 5, j), [[2.0, 1.0]])
    assert np.array_equal(tc.track_centres(trk, 1, np.array([0, 1, 2])), [[[1.0, 0.5]], [[2.0, 1.0]], [[2.0, 1.0]]])
    assert np.array_equal(tc.track_index(0, np.array([0, 1, 2, 3]), 3), [0, 1, 2, 2])
    # one circle of threshold radius 0.8 that a robot at the origin meets only at the held point
    sc = dict(ref=np.zeros((30, 3)), circles=tc.NO_CIRCLES, vel=np.zeros((0, 2)), u=np.zeros((20, 2)),
              tracks=np.array([[[3.0, 0.0], [2.0, 0.0], [0.5, 0.0]]]), radii=np.array([0.4]))
    o = tc.diff_oracle(sc, 4, 20)
    z = np.zeros((4, 20))
    assert np.array_equal(o.collided(z, z)[0], (np.arange(1, 21) >= 2).astype(float))  # clock 0: step 2 reads point 2
    o.set_tracks(sc["tracks"], sc["radii"], clock=5)
    assert o.collided(z, z).all() and o.collided(np.zeros(4), np.zeros(4), steps=0).all()
    o.set_tracks(sc["tracks"], sc["radii"], clock=0, variant="frozen")
    assert not o.collided(z, z).any()


def test_a_track_of_one_point_is_a_static_circle():
    import moving_obstacle_checks as mc
    T = 50
    sc = mc.diff_scene(T, True)
    met = sc["circles"].copy()
    met[:, :2] = mc.centres(sc["circles"], sc["vel"], 0.1, 0, T // 2)
    from oracle import philox
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], 0, 0, tc.K_CASE, T).astype(np.float64)
    static = mc.diff_oracle(dict(sc, circles=met, vel=np.zeros_like(sc["vel"])), tc.K_CASE, T)
    want = static.iteration_general(sc["x0"], eps, "frozen", True)
    for clock in (0, 9):
        o = tc.diff_oracle(dict(sc, circles=tc.NO_CIRCLES, vel=np.zeros((0, 2)), tracks=met[:, None, :2], radii=met[:, 2]), tc.K_CASE, T)
        o.set_tracks(met[:, None, :2], met[:, 2], clock)
        got = o.iteration_general(sc["x0"], eps, "frozen", True)
        assert 0 < tc.penalised(got["S"]).sum() < tc.K_CASE
        assert np.array_equal(got["S"], want["S"]) and np.array_equal(got["u_returned"], want["u_returned"])
