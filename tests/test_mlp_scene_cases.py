"""CPU: what the cases of tests/mlp_scene_checks.py must be for test_gpu_mlp_scenes.py to mean something -- asked of the f64
reference alone, no device.  For every case:

  * each ingredient present (circles, tracks, grid) by itself decides at least 1 sample in 16 as hit and spares at least 1 in 16;
  * the soft grid cost, weight g summed over the priced states, exceeds ten times the S tolerance of the GPU comparison
    (rtol = atol = 1e-3) for at least half of the spared samples -- a dropped or mis-weighted term cannot hide inside the bound;
  * the margin rule leaves out at most 2 % of the samples;
  * with zero velocities, no tracks and no grid the scene oracle gives the static oracle's S exactly
    (mppi_oracle.DiffDriveMlpOracle.iteration: the sequential index, `S[k] =`).

The scenes were moved until the reference met these (mlp_scene_checks.TUNE), never the bars."""
import numpy as np
import pytest

import mlp_scene_checks as ms
import moving_obstacle_checks as mc
import scene_checks as sk
from oracle import mppi_oracle

SHARE = 1.0 / 16.0
S_TOL = 1e-3  # rtol and atol of the S comparison in test_gpu_mlp_scenes.py


def present(sc):
    out = []
    if len(sc["circles"]):
        out.append("circles")
    if sc.get("tracks") is not None:
        out.append("tracks")
    if sc.get("grid") is not None:
        out.append("grid")
    return out


@pytest.mark.parametrize("case", ms.cases(), ids=str)
def test_every_ingredient_decides_and_spares_a_sixteenth(case):
    sc, eps, o, res = ms.case(*case)
    assert present(sc) == {"circles": ["circles"], "tracks": ["tracks"], "grid": ["grid"], "outline": ["grid"],
                           "composed": ["circles", "tracks", "grid"]}[case[0]]
    for name in present(sc):
        hit = o.sample_hit(name)
        print(case, name, "hits", int(hit.sum()), "of", ms.K)
        assert hit.mean() >= SHARE and (~hit).mean() >= SHARE, (name, int(hit.sum()))
    assert (~mc.penalised(res["S"])).mean() >= SHARE  # and all of them together spare a sixteenth


@pytest.mark.parametrize("case", [c for c in ms.cases() if c[0] in ("grid", "outline", "composed")], ids=str)
def test_the_soft_grid_cost_stands_clear_of_the_tolerance(case):
    sc, eps, o, res = ms.case(*case)
    S = np.asarray(res["S"], np.float64)
    spared = ~mc.penalised(S)
    soft = o.sample_grid_term()[spared]
    clear = soft > 10.0 * (S_TOL + S_TOL * np.abs(S[spared]))
    print(case, "spared", int(spared.sum()), "clear of ten tolerances", int(clear.sum()), "median soft", float(np.median(soft)))
    assert 2 * clear.sum() >= spared.sum() > 0


@pytest.mark.parametrize("case", ms.cases(), ids=str)
def test_the_margin_leaves_out_at_most_two_per_cent(case):
    sc, eps, o, res = ms.case(*case)
    keep = ms.kept(o, sc["outline"])
    print(case, "left out", int((~keep).sum()), "delta", ms.delta(sc["outline"]))
    assert (~keep).mean() <= ms.MAX_LEFT_OUT


def test_delta_is_four_times_the_measured_state_error():
    m = ms.measured()
    assert m["max_position_error"] == max(r["max_position_error"] for r in m["rows"])
    assert m["max_yaw_error"] == max(r["max_yaw_error"] for r in m["rows"])
    assert {(r["hidden"], r["n_hidden"]) for r in m["rows"]} == set(ms.SHAPES)
    assert ms.delta() == 4.0 * m["max_position_error"] and ms.delta(True) > ms.delta()
    assert 1e-7 < ms.delta() < 1e-4  # f32 states a few metres from the origin: ulps of 2.4e-7 m accumulated over 50 steps


@pytest.mark.parametrize("case", sorted({(c[0], c[1], c[2], c[4], c[5]) for c in ms.cases()}), ids=str)
def test_the_empty_scene_is_the_static_oracle_exactly(case):
    """the case's scene with its circles standing still and nothing else, priced the way the static oracle prices: S, the
    returned controls and the index are the same numbers"""
    kind, T, accumulate, H, n = case
    sc = ms.scene(kind, T, accumulate, H, n)
    eps = ms.philox.sample_epsilon(mc.DIFF_KW["sigma"], 1, 0, ms.K, T).astype(np.float64)
    kw = dict(mc.DIFF_KW)
    o = ms.scene_oracle(sc["ref"], sc["u"], ms.K, T, sc["w"])  # (the disc model: what the static oracle tests)
    sk.aim(o, dict(circles=sc["circles"], vel=np.zeros((len(sc["circles"]), 2))), 0)
    got = o.iteration_general(sc["x0"], eps, "sequential", False)

    class Static(mppi_oracle.DiffDriveMlpOracle):
        FILTER = staticmethod(lambda w, window: mppi_oracle.moving_average_diffdrive(w, mc.filter_window(T)))
    st = Static(ref_path=sc["ref"], num_samples_K=ms.K, num_horizons_T=T, obstacle_circles=sc["circles"], mlp_weights=sc["w"], **kw)
    st.u_prev[:] = sc["u"]
    want = st.iteration(sc["x0"], eps)
    assert np.array_equal(got["S"], want["S"])
    assert np.array_equal(got["u_returned"], want["u_returned"]) and got["idx_after"] == want["idx_after"]
