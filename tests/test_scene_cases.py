"""CPU: the scenes of tests/scene_checks.py discriminate, under the f64 reference alone.  For every case test_gpu_scene.py runs:
each ingredient the case has penalises, alone, at least one sample in 16 that the other ingredients and the circles spare (on
the agent the scene is built for: agent 0 of a batch) -- a kernel that drops any one of them fails; the grid's soft term
exceeds ten times the f32 tolerance for at least half of the spared samples; and the margin rule leaves out at most 1 % of
every agent's samples at the case's seed.  And the staging function of the composed launches (csrc/mppi_scene_staging.h), by
hand at its budget edges, through a C caller and through the restatement the GPU tests size their cases by."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import scene_checks as sk
from moving_obstacle_checks import RACE_T

K = sk.K_CASE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_agent(o, res, names, tag):
    S = np.asarray(res["S"], np.float64)
    left_out = 1.0 - float((o.sample_margin() > sk.MARGIN).mean())
    assert left_out <= sk.MAX_LEFT_OUT, (tag, left_out)
    alone = {n: int(v.sum()) for n, v in sk.exclusive_hits(o, names).items()}
    assert all(n >= K // 16 for n in alone.values()), (tag, alone)
    spared = ~sk.penalised(S)
    assert spared.any(), tag
    if "grid" in names:
        soft = o.sample_grid_term()[spared] > 10.0 * sk.f32_tolerance(S[spared])
        assert soft.mean() >= 0.5, (tag, float(soft.mean()))
    return alone


@pytest.mark.parametrize("case", sk.single_cases(), ids=str)
def test_single_agent_cases_discriminate(case):
    sc, eps, o, res = sk.single_case(*case)
    check_agent(o, res, ("grid", "tracks"), case)
    if case[4] < 0:  # the tracks run out inside the horizon
        assert sc["tracks"].shape[1] < case[3] + case[0] + 1


@pytest.mark.parametrize("case", sk.fleet_cases(), ids=str)
def test_fleet_cases_discriminate(case):
    T, accumulate, mode, what, clock, extra = case
    sc = sk.fleet_scene(T, accumulate, what, clock, extra)
    eps = sk.fleet_noise(sk.fleet_seed(*case), clock, K, T)
    runs = sk.fleet_iteration(sc, eps, K, T, mode, accumulate)
    check_agent(*runs[0], what, case)
    for a, (o, res) in enumerate(runs[1:], 1):  # the agents that lack an ingredient: the margin rule, and something decided
        assert 1.0 - float((o.sample_margin() > sk.MARGIN).mean()) <= sk.MAX_LEFT_OUT, (case, a)
    assert sc["per"][1]["tracks"] is None and sc["per"][2]["grid"] is None
    if what == sk.INGREDIENTS:
        hit1, hit2 = sk.penalised(runs[1][1]["S"]), sk.penalised(runs[2][1]["S"])
        assert hit1.any() and not hit1.all() and hit2.any() and not hit2.all()


@pytest.mark.parametrize("clock", [0, 3])
def test_race_car_discriminates(clock):
    sc, eps, o, res = sk.race_case(clock)
    check_agent(o, res, ("grid", "tracks"), ("race", clock))


def test_race_pair_discriminates():
    sc = sk.race_fleet_scene()
    eps = sk.fleet_noise(sk.RACE_FLEET_SEED, 0, K, RACE_T, 2, "race")
    runs = sk.race_fleet_iteration(sc, eps, K)
    check_agent(*runs[0], sk.INGREDIENTS, "race pair")
    assert 1.0 - float((runs[1][0].sample_margin() > sk.MARGIN).mean()) <= sk.MAX_LEFT_OUT


def test_dropping_an_ingredient_changes_the_reference():
    """the same case with one ingredient taken away: the costs of agent 0 differ in at least a sixteenth of the samples"""
    case = sk.fleet_cases()[0]
    T, accumulate, mode, what, clock, extra = case
    eps = sk.fleet_noise(sk.fleet_seed(*case), clock, K, T)
    full = np.asarray(sk.fleet_iteration(sk.fleet_scene(T, accumulate, what, clock, extra), eps, K, T, mode, accumulate)[0][1]["S"])
    for gone in what:
        rest = tuple(w for w in what if w != gone)
        S = np.asarray(sk.fleet_iteration(sk.fleet_scene(T, accumulate, rest, clock, extra), eps, K, T, mode, accumulate)[0][1]["S"])
        assert (sk.penalised(full) & ~sk.penalised(S)).sum() >= K // 16, gone


# ------------------------------------------------------------------------------------------ the staging function
# (elem, plan agents, largest track set, T) -> (plans, tracks) staged, by hand:
#   a plan table is B (T + 1) 2 elem bytes, a track window n ((T + 1) 2 + 1) elem bytes; T = 128: 2064 / 2072 per agent / track
#   in f64, 1032 / 1036 in f32; the budget is 16384 bytes in f64 and 40000 in f32
STAGING = [
    ((8, 3, 4, 128), (6192, 8288)),      # 6192 + 8288 = 14480 <= 16384: both fit
    ((8, 3, 5, 128), (6192, 0)),         # 6192 + 10360 = 16552 > 16384: the tracks from memory
    ((8, 7, 1, 128), (14448, 0)),        # 14448 + 2072 = 16520: the plans alone fit
    ((8, 7, 0, 128), (14448, 0)),
    ((8, 8, 4, 128), (0, 8288)),         # 16512 > 16384: the plans from memory, the tracks against the whole budget
    ((8, 8, 7, 128), (0, 14504)),
    ((8, 8, 8, 128), (0, 0)),            # 16576 > 16384 either
    ((8, 0, 7, 128), (0, 14504)),        # no plans: track_lds_bytes' limit
    ((8, 0, 8, 128), (0, 0)),
    ((4, 38, 0, 128), (39216, 0)),       # fleet_plan_lds_bytes' limit: 38 agents fit, 39 (40248) do not
    ((4, 39, 0, 128), (0, 0)),
    ((4, 3, 35, 128), (3096, 36260)),    # 3096 + 36260 = 39356 <= 40000
    ((4, 3, 36, 128), (3096, 0)),        # 3096 + 37296 = 40392 > 40000
    ((4, 39, 38, 128), (0, 39368)),      # plans too large: 38 tracks fit the whole budget, 39 (40404) do not
    ((4, 39, 39, 128), (0, 0)),
    ((4, 3, 2, 50), (1224, 824)),        # the cases of test_gpu_scene.py: everything staged
    ((8, 3, 2, 7), (384, 272)),
    ((4, 1, 1, 2), (24, 28)),            # 24 bytes of plans: the tracks start at byte 32
]


def test_staging_restated():
    for args, (plans, tracks) in STAGING:
        got = sk.scene_lds_bytes(*args)
        assert got[:2] == (plans, tracks), (args, got)
        assert got[2] % 16 == 0 and got[2] >= plans and got[3] <= (40000 if args[0] == 4 else 16384)
    assert sk.scene_lds_bytes(4, 1, 1, 2) == (24, 28, 32, 60)


def test_staging_as_the_library_compiles_it():
    """csrc/mppi_scene_staging.h through a plain C caller"""
    rows = "".join(f"{{{e}, {b}, {n}, {T}}}, " for (e, b, n, T), _ in STAGING)
    src = ('#include <stdio.h>\n#include "mppi_scene_staging.h"\nint main(void) { static const int c[][4] = {' + rows + '};\n'
           'for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); ++i) { mppi_scene_staging s = mppi_scene_lds_bytes(c[i][0], c[i][1], c[i][2], c[i][3]);\n'
           'printf("%d %d %d %d\\n", s.plans, s.tracks, mppi_scene_track_offset(s.plans), mppi_scene_lds_total(s)); } return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "dnn-mppi-mpc_amd", "csrc"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().split("\n")
    for (args, want), line in zip(STAGING, lines):
        got = tuple(int(v) for v in line.split())
        assert got[:2] == want and got == sk.scene_lds_bytes(*args), (args, got)
