"""What obstacle tracks cost (mppi_set_obstacle_tracks): the same m obstacles as moving circles and as tracks
sampled from their velocities, closed loops on the device, frozen waypoint index (so that nothing but the collision test differs).

    python tools/obstacle_tracks.py [--out FILE] [--iters N] [--rounds R]

Two shapes: config 3's (diff-drive, K = 16384, T = 50) and 32 batched diff-drive agents of K = 4096 with their own sets; m = 2
and m = 32 obstacles.  Per shape and m three handles, alternated in one process, R rounds each:
  circles -- m circles at constant velocity: k_rollout_fused<..., SPEC = 3>
  tracks  -- the same obstacles as tracks of T + 1 points: k_rollout_fused<..., SPEC = 5>, the window staged in LDS
  none    -- no obstacles (the SPEC = 3 form with an empty table)
Timed by event pairs around the rollout launch (mppi_last_kernel_ms) and by wall time per iteration of mppi_run_closed_loop.
SPEC 3 on the same box in the same call is the yardstick: `tracks_minus_circles` stands beside the circles' own spread over the
rounds, and per collision test it is divided by agents * K * T * m.  Prints one JSON line per shape and m; --out FILE writes
them as one JSON document tagged with the build id."""
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
VARIANTS = ("circles", "tracks", "none")


def line_path(p, q, n):
    t = np.linspace(0.0, 1.0, n)
    yaw = np.arctan2(q[1] - p[1], q[0] - p[0])
    return np.stack([p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]), np.full(n, yaw), np.full(n, 5.0)], axis=1)


def diff_cfg(T):
    return dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
                param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
                search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=capi.WAYPOINT_FROZEN,
                obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10, seed=5)


SHAPES = [
    dict(name="config 3 shape", cfg=diff_cfg(50), K=16384, agents=1, x0=[0.0, 0.0, -0.46]),
    dict(name="32 agents of K = 4096, own sets", cfg=diff_cfg(50), K=4096, agents=32, x0=[0.0, 0.0, -0.46]),
]
PATH = line_path((0.0, 0.0), (1000.0, -500.0), 4000)  # (long enough that no closed loop here reaches its end)


def scene(a, m):
    """Agent a's m circles beside the start of the path and their velocities (slow: they stay in reach for the whole run)."""
    i = np.arange(m, dtype=np.float64)
    side = np.where(i % 2 == 0, 1.0, -1.0)
    circles = np.stack([3.0 + 0.1 * a + 0.7 * i, -1.5 - 0.35 * i + side * (1.6 + 0.05 * a), np.full(m, 0.4)], axis=1)
    vel = np.stack([0.02 * side, -0.03 + 0.001 * i], axis=1)
    return circles, vel


def make(shape, m, variant):
    B, T = shape["agents"], shape["cfg"]["T"]
    e = pkg.Engine(K=shape["K"], n_agents=B, obstacle_motion=1, precision=capi.PREC_F32, **shape["cfg"])
    e.set_ref_path(PATH[:, :e.nx])
    dt = shape["cfg"]["delta_t"]
    for a in range(B):
        circles, vel = scene(a, m)
        agent = a if B > 1 else None
        if variant == "circles":
            e.set_obstacles(circles, agent=agent, velocities=vel)
        elif variant == "tracks":
            # (the clock soon runs past the end and the tracks hold their last point: the work per test stays what it is)
            steps = np.arange(T + 1, dtype=np.float64)
            e.set_obstacle_tracks(circles[:, None, :2] + vel[:, None, :] * (dt * steps)[None, :, None], circles[:, 2], agent=agent)
    x0 = np.asarray(shape["x0"], dtype=np.float64)
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


lines = []
for shape in SHAPES:
    for m in (2, 32):
        handles = {v: make(shape, m, v) for v in VARIANTS}
        wall = {v: [] for v in VARIANTS}
        launch = {v: [] for v in VARIANTS}
        for _ in range(ROUNDS):
            for v in VARIANTS:
                w, r = one_round(handles[v])
                wall[v].append(w)
                launch[v].append(r)
        tests = shape["agents"] * shape["K"] * shape["cfg"]["T"] * m
        d_launch = statistics.median(launch["tracks"]) - statistics.median(launch["circles"])
        d_wall = statistics.median(wall["tracks"]) - statistics.median(wall["circles"])
        out = {"shape": shape["name"], "K": shape["K"], "T": shape["cfg"]["T"], "agents": shape["agents"], "m": m, "iterations": N_ITER,
               "kernels": {v: handles[v].rollout_kernel() for v in VARIANTS},
               "rollout_launch_us": {v: spread(launch[v]) for v in VARIANTS},
               "us_per_iteration": {v: spread(wall[v]) for v in VARIANTS},
               "tracks_minus_circles": {"rollout_launch_us": d_launch, "us_per_iteration": d_wall,
                                        "ps_per_test_launch": 1e6 * d_launch / tests, "ps_per_test_wall": 1e6 * d_wall / tests},
               "circles_own_spread_us": {"rollout_launch": max(launch["circles"]) - min(launch["circles"]),
                                         "per_iteration": max(wall["circles"]) - min(wall["circles"])},
               "n_collided_last": {v: int(handles[v].stats.n_collided) for v in VARIANTS}}
        for e in handles.values():
            e.close()
        lines.append(out)
        print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
