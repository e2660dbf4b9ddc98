"""What pricing the vehicle's outline against a cost grid costs (mppi_set_cost_grid_footprint): closed loops on the
device, frozen waypoint index (so that nothing but the grid pricing differs), f32, T = 50.

    python tools/grid_footprint.py [--out FILE] [--iters N] [--rounds R]

Two vehicles -- the race car (4 m x 3 m at a margin of 1.5) and a diff-drive box (0.75 m x 0.5 m) -- in two shapes each:
K = 16384, and 32 batched agents of K = 4096.  They lap a ring (the path holds 60 laps) between two inflated walls, so that every
launch prices states inside the grids: squares of 64 x 64 and of 512 x 512 nodes (1 MiB of f32 against the 4 MiB L2 of an XCD).
Per vehicle and shape seven handles, alternated in one process, R rounds each:
  circles 0 / 2 / 8        -- m moving circles and no grid: k_rollout_fused<..., SPEC = 3>, the yardstick
  centre 64 / 512          -- the grid at the state's (x, y): SPEC = 6
  outline 64 / 512         -- the grid under the nine points: SPEC = 8
Timed by event pairs around the rollout launch (mppi_last_kernel_ms) and by wall time per iteration of mppi_run_closed_loop,
median (min - max) over the rounds.  The footprint's cost is reported in centre lookups -- (outline - circles 0) / (centre -
circles 0) of the launch -- and in circles: the m at which SPEC 3, interpolated linearly, costs what the outline form costs.
Prints one JSON line per vehicle and shape; --out FILE writes them as one JSON document tagged with the build id."""
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
T = 50
CIRCLES = (0, 2, 8)
NODES = (64, 512)
VARIANTS = [f"circles {m}" for m in CIRCLES] + [f"{mode} {n}" for n in NODES for mode in ("centre", "outline")]
LAPS, PER_LAP = 60, 200

VEHICLES = {
    # ring radius, distance of the walls from the centre line, inflation, the grids' span
    "race car": dict(ring=24.0, wall=8.0, inflate=4.0, span=64.0, speed=5.0,
                     cfg=dict(model=capi.MODEL_RACECAR, T=T, delta_t=0.05, u_max=[0.523, 2.0], wheel_base=2.5, param_exploration=0.1,
                              param_lambda=50.0, param_alpha=0.9, sigma=[0.5, 0.0, 0.0, 0.1], stage_cost_weight=[50.0, 50.0, 1.0, 20.0],
                              terminal_cost_weight=[50.0, 50.0, 1.0, 20.0], beta_mode=capi.BETA_INV_LAMBDA, accumulate_stage_cost=1,
                              waypoint_mode=capi.WAYPOINT_FROZEN, search_window=200, wrap_yaw_stage=1, wrap_yaw_terminal=1,
                              clamp_rollout=1, clamp_u_after_update=1, filter_mode=capi.FILTER_RACECAR, filter_window=10,
                              obstacle_model=capi.OBSTACLE_OUTLINE, safety_margin=1.5, vehicle_w=3.0, vehicle_l=4.0,
                              collision_penalty=1e10, seed=7)),
    "diff-drive box": dict(ring=8.0, wall=2.0, inflate=1.5, span=25.6, speed=5.0,
                           cfg=dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                                    param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0],
                                    terminal_cost_weight=[5, 5, 10, 0], search_window=20, filter_window=10, clamp_rollout=1,
                                    waypoint_mode=capi.WAYPOINT_FROZEN, obstacle_model=capi.OBSTACLE_OUTLINE, safety_margin=1.0,
                                    vehicle_w=0.5, vehicle_l=0.75, collision_penalty=1e10, seed=5)),
}
SHAPES = [dict(name="K = 16384", K=16384, agents=1), dict(name="32 agents of K = 4096", K=4096, agents=32)]


def ring_path(v):
    a = 2.0 * np.pi * np.arange(LAPS * PER_LAP) / PER_LAP
    return np.stack([v["ring"] * np.cos(a), v["ring"] * np.sin(a), a + 0.5 * np.pi, np.full(a.shape, v["speed"])], axis=1)  # (yaw unwrapped)


def circles_of(v, a, m):
    """Agent a's m circles around the outside of the ring and their (slow) velocities"""
    i = np.arange(m, dtype=np.float64)
    ang = 2.0 * np.pi * (i + 0.1 * a) / max(m, 1)
    r = v["ring"] + 0.9 * v["wall"]
    circles = np.stack([r * np.cos(ang), r * np.sin(ang), np.full(m, 0.2 * v["wall"])], axis=1)
    vel = np.stack([0.002 * np.cos(ang + 1.0), 0.002 * np.sin(ang + 1.0)], axis=1)
    return circles, vel


def grid_of(v, n):
    """The ring's inner and outer wall, inflated: 0 on the centre line, lethal (0.8) near a wall"""
    res = v["span"] / n
    origin = -0.5 * res * (n - 1)
    c = origin + res * np.arange(n)
    r = np.hypot(c[None, :], c[:, None])
    cells = np.clip(1.0 - np.minimum(np.abs(r - (v["ring"] - v["wall"])), np.abs(r - (v["ring"] + v["wall"]))) / v["inflate"], 0.0, 1.0)
    return dict(cells=cells, origin=(origin, origin), resolution=res, weight=1.0, lethal=0.8)


def make(v, shape, variant):
    B = shape["agents"]
    e = pkg.Engine(K=shape["K"], n_agents=B, obstacle_motion=1, precision=capi.PREC_F32, **v["cfg"])
    e.set_ref_path(ring_path(v)[:, :e.nx])
    kind, n = variant.split()
    for a in range(B):
        circles, vel = circles_of(v, a, int(n) if kind == "circles" else 0)
        e.set_obstacles(circles, agent=a if B > 1 else None, velocities=vel)
    if kind != "circles":
        e.set_cost_grid_footprint(kind)
        e.set_cost_grid(**grid_of(v, int(n)))
    x0 = np.array([v["ring"], 0.0, 0.5 * np.pi, v["speed"]])[:e.nx]
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


def in_circles(by_m, cost):
    """the m at which SPEC 3, interpolated (beyond the last m: extrapolated) linearly between the measured m, costs `cost`"""
    ms = sorted(by_m)
    if cost <= by_m[ms[0]]:
        return 0.0
    for lo, hi in zip(ms, ms[1:]):
        if cost <= by_m[hi] or hi == ms[-1]:
            return lo + (hi - lo) * (cost - by_m[lo]) / (by_m[hi] - by_m[lo])


lines = []
for vname, v in VEHICLES.items():
    for shape in SHAPES:
        handles = {var: make(v, shape, var) for var in VARIANTS}
        wall = {var: [] for var in VARIANTS}
        launch = {var: [] for var in VARIANTS}
        for _ in range(ROUNDS):
            for var in VARIANTS:
                w, r = one_round(handles[var])
                wall[var].append(w)
                launch[var].append(r)
        med = {var: statistics.median(launch[var]) for var in VARIANTS}
        by_m = {m: med[f"circles {m}"] for m in CIRCLES}
        out = {"vehicle": vname, "shape": shape["name"], "K": shape["K"], "T": T, "agents": shape["agents"], "iterations": N_ITER,
               "kernels": {var: handles[var].rollout_kernel() for var in VARIANTS},
               "rollout_launch_us": {var: spread(launch[var]) for var in VARIANTS},
               "us_per_iteration": {var: spread(wall[var]) for var in VARIANTS},
               "outline_minus_centre_launch_us": {str(n): med[f"outline {n}"] - med[f"centre {n}"] for n in NODES},
               "outline_in_centre_lookups": {str(n): (med[f"outline {n}"] - by_m[0]) / max(med[f"centre {n}"] - by_m[0], 1e-9) for n in NODES},
               "outline_in_circles": {str(n): in_circles(by_m, med[f"outline {n}"]) for n in NODES},
               "n_collided_last": {var: int(handles[var].stats.n_collided) for var in VARIANTS}}
        for e in handles.values():
            e.close()
        lines.append(out)
        print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
