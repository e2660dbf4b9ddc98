"""What a cost grid costs (mppi_set_cost_grid) against moving circles: closed loops on the device, frozen waypoint
index (so that nothing but the obstacle pricing differs), f32, T = 50.

    python tools/cost_grid.py [--out FILE] [--iters N] [--rounds R]

Two shapes: config 3's (diff-drive, K = 16384) and 32 batched diff-drive agents of K = 4096.  The robots lap a ring of 8 m
radius (the path holds 60 laps), so that every launch of a run prices states inside the grids: 25.6 m squares of 64 x 64 nodes
(0.4 m) and of 512 x 512 nodes (0.05 m, 1 MiB of f32 against the 4 MiB L2 of an XCD), the ring's inner and outer wall inflated.
Per shape eight handles, alternated in one process, R rounds each:
  circles 0 / 2 / 8 / 32  -- m moving circles around the ring: k_rollout_fused<..., SPEC = 3>
  grid 64 / 512, with 0 and with 2 circles: k_rollout_fused<..., SPEC = 6>
(A trial build also ran `staged 64` handles, the 64 x 64 grid staged in dynamic LDS: profiles/cost_grid_staged_trial.json.)
Timed by event pairs around the rollout launch (mppi_last_kernel_ms) and by wall time per iteration of mppi_run_closed_loop.
SPEC 3 on the same box in the same call is the yardstick, with its own spread over the rounds.  `break_even_circles`: the number
of circles at which SPEC 3's launch, interpolated linearly between the measured m, costs what the grid form costs.  Prints one
JSON line per shape; --out FILE writes them as one JSON document tagged with the build id."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dnn_mppi_mpc_amd as pkg  # noqa: E402
from dnn_mppi_mpc_amd import _capi as capi  # noqa: E402

ARGV = sys.argv[1:]
OUT = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else None
N_ITER = int(ARGV[ARGV.index("--iters") + 1]) if "--iters" in ARGV else 500
ROUNDS = int(ARGV[ARGV.index("--rounds") + 1]) if "--rounds" in ARGV else 5
CIRCLES = (0, 2, 8, 32)
GRIDS = {64: 0.4, 512: 0.05}  # nodes per side -> resolution: both span 25.2 / 25.55 m around the ring
VARIANTS = [f"circles {m}" for m in CIRCLES] + [f"grid {n} + {m} circles" for n in GRIDS for m in (0, 2)]
RING_R, LAPS, PER_LAP = 8.0, 60, 200


def ring_path():
    a = 2.0 * np.pi * np.arange(LAPS * PER_LAP) / PER_LAP
    return np.stack([RING_R * np.cos(a), RING_R * np.sin(a), a + 0.5 * np.pi, np.full(a.shape, 5.0)], axis=1)  # (yaw unwrapped)


def diff_cfg(T):
    return dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
                param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
                search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=capi.WAYPOINT_FROZEN,
                obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10, seed=5)


SHAPES = [
    dict(name="config 3 shape", cfg=diff_cfg(50), K=16384, agents=1),
    dict(name="32 agents of K = 4096", cfg=diff_cfg(50), K=4096, agents=32),
]
PATH = ring_path()


def circles_of(a, m):
    """Agent a's m circles around the outside of the ring and their (slow) velocities"""
    i = np.arange(m, dtype=np.float64)
    ang = 2.0 * np.pi * (i + 0.1 * a) / max(m, 1)
    circles = np.stack([(RING_R + 1.8) * np.cos(ang), (RING_R + 1.8) * np.sin(ang), np.full(m, 0.4)], axis=1)
    vel = np.stack([0.002 * np.cos(ang + 1.0), 0.002 * np.sin(ang + 1.0)], axis=1)
    return circles, vel


def grid_of(n):
    """The ring's walls at radius 6 and 10, inflated by 1.5 m: 0 on the centre line, lethal (0.8) within 0.3 m of a wall"""
    res = GRIDS[n]
    origin = -0.5 * res * (n - 1)
    c = origin + res * np.arange(n)
    r = np.hypot(c[None, :], c[:, None])
    cells = np.clip(1.0 - np.minimum(np.abs(r - (RING_R - 2.0)), np.abs(r - (RING_R + 2.0))) / 1.5, 0.0, 1.0)
    return dict(cells=cells, origin=(origin, origin), resolution=res, weight=1.0, lethal=0.8)


def make(shape, variant):
    B = shape["agents"]
    e = pkg.Engine(K=shape["K"], n_agents=B, obstacle_motion=1, precision=capi.PREC_F32, **shape["cfg"])
    e.set_ref_path(PATH[:, :e.nx])
    words = variant.split()
    m = int(words[1]) if words[0] == "circles" else int(words[3])
    for a in range(B):
        circles, vel = circles_of(a, m)
        e.set_obstacles(circles, agent=a if B > 1 else None, velocities=vel)
    if words[0] == "grid":
        e.set_cost_grid(**grid_of(int(words[1])))
    x0 = np.array([RING_R, 0.0, 0.5 * np.pi])
    e.set_state(np.tile(x0, (B, 1)) if B > 1 else x0)
    e.run_closed_loop(100)
    return e


def one_round(e):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run_closed_loop(N_ITER)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e.enable_timing(True)
    e.run_closed_loop(200)
    ms = e.last_kernel_ms()
    e.enable_timing(False)
    return 1e6 * wall / N_ITER, 1e3 * ms["rollout"]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def break_even(by_m, cost):
    """the m at which SPEC 3, interpolated linearly between the measured m, costs `cost` (None: beyond 32, or below 0)"""
    ms = sorted(by_m)
    if cost <= by_m[ms[0]]:
        return 0.0
    for lo, hi in zip(ms, ms[1:]):
        if by_m[lo] <= cost <= by_m[hi]:
            return lo + (hi - lo) * (cost - by_m[lo]) / (by_m[hi] - by_m[lo])
    return None


lines = []
for shape in SHAPES:
    handles = {v: make(shape, v) for v in VARIANTS}
    wall = {v: [] for v in VARIANTS}
    launch = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            w, r = one_round(handles[v])
            wall[v].append(w)
            launch[v].append(r)
    med_l = {m: statistics.median(launch[f"circles {m}"]) for m in CIRCLES}
    med_w = {m: statistics.median(wall[f"circles {m}"]) for m in CIRCLES}
    out = {"shape": shape["name"], "K": shape["K"], "T": shape["cfg"]["T"], "agents": shape["agents"], "iterations": N_ITER,
           "kernels": {v: handles[v].rollout_kernel() for v in VARIANTS},
           "rollout_launch_us": {v: spread(launch[v]) for v in VARIANTS},
           "us_per_iteration": {v: spread(wall[v]) for v in VARIANTS},
           "spec3_own_spread_us": {f"circles {m}": {"rollout_launch": max(launch[f"circles {m}"]) - min(launch[f"circles {m}"]),
                                                    "per_iteration": max(wall[f"circles {m}"]) - min(wall[f"circles {m}"])} for m in CIRCLES},
           "grid_minus_circles_0_launch_us": {f"grid {n}": statistics.median(launch[f"grid {n} + 0 circles"]) - med_l[0] for n in GRIDS},
           "break_even_circles": {f"grid {n}": {"rollout_launch": break_even(med_l, statistics.median(launch[f"grid {n} + 0 circles"])),
                                                "per_iteration": break_even(med_w, statistics.median(wall[f"grid {n} + 0 circles"]))}
                                  for n in GRIDS},
           "n_collided_last": {v: int(handles[v].stats.n_collided) for v in VARIANTS},
           "final_radius": {v: float(np.hypot(*np.atleast_2d(handles[v].get_state())[0, :2])) for v in VARIANTS}}
    for e in handles.values():
        e.close()
    lines.append(out)
    print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
