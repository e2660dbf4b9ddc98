"""CPU: every scene of tests/moving_obstacle_checks.py is what it claims -- motion decides which samples are penalised, the f64
reference itself leaves out at most 1 % of a case's samples, and the helper's moving centres are the closed form."""
import numpy as np
import pytest

import moving_obstacle_checks as mc

SIXTEENTH = 1.0 / 16.0


@pytest.mark.parametrize("T,accumulate,mode", mc.diff_cases())
def test_diff_scene_motion_decides(T, accumulate, mode):
    """(a) the penalised set under motion differs from the set with the circles frozen where they stand at step 0 in at least
    one sample in 16 -- and, where every step is priced, from the set frozen at step T as well.  (`S[k] =` prices the state
    after step T only: the circles frozen at step T are then the moving ones by construction.  What a wrong step does there
    is asserted against the circles at step T - 64 instead, for the horizons with a second chunk.)  (b) at most 1 % of the
    samples have a tested pose inside the decision margin."""
    _, _, o, res = mc.diff_case(T, accumulate, mode)
    moving = mc.penalised(res["S"])
    left_out = float((o.sample_margin() <= mc.MARGIN).mean())
    frozen0 = mc.penalised(mc.diff_case(T, accumulate, mode, freeze_at=0)[3]["S"])
    print(T, accumulate, mode, "penalised", moving.mean(), "vs step 0", (moving != frozen0).mean(), "left out", left_out)
    assert 0.1 < moving.mean() < 0.9
    assert (moving != frozen0).mean() >= SIXTEENTH
    if accumulate:
        frozenT = mc.penalised(mc.diff_case(T, accumulate, mode, freeze_at=T)[3]["S"])
        assert (moving != frozenT).mean() >= SIXTEENTH
    elif T > 64:
        seam = mc.penalised(mc.diff_case(T, accumulate, mode, freeze_at=T - 64)[3]["S"])
        assert (moving != seam).mean() >= SIXTEENTH
    assert left_out <= mc.MAX_LEFT_OUT
    assert mc.kept(o, f64=True).all()  # an f64 handle leaves out nothing


def test_race_scene_motion_decides():
    _, _, o, res = mc.race_case()
    moving = mc.penalised(res["S"])
    left_out = float((o.sample_margin() <= mc.MARGIN).mean())
    frozen0 = mc.penalised(mc.race_case(freeze_at=0)[3]["S"])
    frozenT = mc.penalised(mc.race_case(freeze_at=mc.RACE_T)[3]["S"])
    print("penalised", moving.mean(), "vs step 0", (moving != frozen0).mean(), "vs step T", (moving != frozenT).mean(), left_out)
    assert 0.1 < moving.mean() < 0.9
    assert (moving != frozen0).mean() >= SIXTEENTH and (moving != frozenT).mean() >= SIXTEENTH
    assert left_out <= mc.MAX_LEFT_OUT


def test_closed_loop_scene_depends_on_the_clock():
    """The closed-loop reference ticks the circles once per iteration: its trace differs from the one with the clock held."""
    tr = [mc.diff_closed_loop(50, 12, tick=t)["u0"] for t in (True, False)]
    assert np.abs(tr[0] - tr[1]).max() > 1e-3


def test_centres_are_the_closed_form():
    """(c) c + v dt (n + j), by hand: circle at (1, 2) moving (0.5, -0.25) m/s, dt = 0.1."""
    c, v = np.array([[1.0, 2.0, 0.4]]), np.array([[0.5, -0.25]])
    assert np.array_equal(mc.centres(c, v, 0.1, 0, 0), [[1.0, 2.0]])
    np.testing.assert_allclose(mc.centres(c, v, 0.1, 0, 10), [[1.5, 1.75]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(mc.centres(c, v, 0.1, 30, 10), [[3.0, 1.0]], rtol=0, atol=1e-15)  # 4 s
    np.testing.assert_allclose(mc.centres(c, v, 0.1, 2, np.array([0, 8])), [[[1.1, 1.95]], [[1.5, 1.75]]], rtol=0, atol=1e-15)
    assert np.array_equal(mc.centres(c, 0 * v, 0.1, 7, 5), [[1.0, 2.0]])  # zero velocity: the static centre exactly


def test_collided_takes_the_step_from_the_shape_of_the_call():
    """A diff-drive robot at the origin, one circle of threshold radius 0.8 that starts 2.05 m to its right and moves left
    at 1 m/s, dt = 0.1, T = 20: inside from step 13 on (2.05 - 1.3 = 0.75 < 0.8), not at step 12 (0.85)."""
    sc = dict(ref=np.zeros((30, 3)), circles=np.array([[2.05, 0.0, 0.4]]), vel=np.array([[-1.0, 0.0]]), u=np.zeros((20, 2)))
    o = mc.diff_oracle(sc, 4, 20)
    z = np.zeros((4, 20))
    stage = o.collided(z, z)  # [K, T]: column t is step t + 1
    assert np.array_equal(stage[0], (np.arange(1, 21) >= 13).astype(float)) and np.array_equal(stage[0], stage[3])
    assert o.collided(np.zeros(4), np.zeros(4)).all()  # [K]: step T = 20
    assert not o.collided(np.zeros(4), np.zeros(4), steps=12).any() and o.collided(np.zeros(4), np.zeros(4), steps=13).all()
    o.set_motion(sc["vel"], clock=5)  # five control steps later the same test is met five steps earlier
    assert np.array_equal(o.collided(z, z)[0], (np.arange(1, 21) >= 8).astype(float))
    o.set_motion(sc["vel"], clock=0, freeze_at=0)
    assert not o.collided(z, z).any()


def test_general_iteration_is_the_oracles_own_where_they_overlap():
    """iteration_general(sequential, S[k] =) restates DiffDriveOracle.iteration: same S, controls and index."""
    T = 50
    sc, eps, o, res = mc.diff_case(T, False, "sequential")
    ref = mc.diff_oracle(sc, mc.K_CASE, T)
    own = ref.iteration(sc["x0"], eps.astype(np.float64))
    np.testing.assert_allclose(res["S"], own["S"], rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(res["u_returned"], own["u_returned"], rtol=1e-12, atol=1e-14)
    assert res["idx_after"] == own["idx_after"] and res["idx_start"] == own["idx_start"]
