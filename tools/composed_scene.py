"""What a composed scene costs (mppi_set_scene_mode) against its parts: closed loops on the device, frozen waypoint
index (so that nothing but the obstacle pricing differs), f32, T = 50.

    python tools/composed_scene.py [--out FILE] [--iters N] [--rounds R]

Two shapes, as tools/cost_grid.py has them: config 3's (diff-drive, K = 16384, one agent) and 32 batched diff-drive agents of
K = 4096, each lapping its own copy of a ring of 8 m radius (turned by 1/32 of a lap per agent, so that the fleet's robots
stand apart).  Per shape the handles below, alternated in one process, R rounds each:
  none                       -- k_rollout_fused<..., SPEC = 3>
  grid                       -- the ring's walls on 64 x 64 nodes: SPEC = 6
  tracks                     -- two tracks beside the ring: SPEC = 5
  plans (batched only)       -- a fleet of 32 in plan mode: SPEC = 4 (k_fleet_plan in front)
  every pair and all three   -- MPPI_SCENE_COMPOSED: SPEC = 7
Timed by event pairs around the rollout launch (mppi_last_kernel_ms; a fleet handle: with its k_fleet_plan launch) and by wall
time per iteration of mppi_run_closed_loop.  `over_sum_of_parts_us`: what the composed form costs over SPEC 3 plus the sum of
its parts' own increments over SPEC 3 (medians).  Prints one JSON line per shape; --out FILE writes them as one JSON document
tagged with the build id."""
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
RING_R, LAPS, PER_LAP = 8.0, 60, 200
T = 50


def ring_path(turn=0.0):
    a = 2.0 * np.pi * np.arange(LAPS * PER_LAP) / PER_LAP + turn
    return np.stack([RING_R * np.cos(a), RING_R * np.sin(a), a + 0.5 * np.pi, np.full(a.shape, 5.0)], axis=1)  # (yaw unwrapped)


def diff_cfg():
    return dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
                param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
                search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=capi.WAYPOINT_FROZEN,
                obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10, seed=5)


SHAPES = [dict(name="config 3 shape", K=16384, agents=1), dict(name="32 agents of K = 4096", K=4096, agents=32)]


def variants(B):
    parts = ["grid", "tracks"] + (["plans"] if B > 1 else [])
    out = [()] + [(p,) for p in parts]
    out += [(a, b) for i, a in enumerate(parts) for b in parts[i + 1:]]
    if B > 1:
        out.append(tuple(parts))
    return out


def name_of(v):
    return " + ".join(v) if v else "none"


def grid_of(n=64, res=0.4):
    """The ring's walls at radius 6 and 10, inflated by 1.5 m (tools/cost_grid.py)"""
    origin = -0.5 * res * (n - 1)
    c = origin + res * np.arange(n)
    r = np.hypot(c[None, :], c[:, None])
    cells = np.clip(1.0 - np.minimum(np.abs(r - (RING_R - 2.0)), np.abs(r - (RING_R + 2.0))) / 1.5, 0.0, 1.0)
    return dict(cells=cells, origin=(origin, origin), resolution=res, weight=1.0, lethal=0.8)


def tracks_of(turn, L=4096):
    """two tracks that walk round the outside of agent's ring, 1.8 m off, a little slower than the robot"""
    i = np.arange(L, dtype=np.float64)
    out = []
    for k in range(2):
        ang = turn + np.pi * k + 0.0005 * i
        out.append(np.stack([(RING_R + 1.8) * np.cos(ang), (RING_R + 1.8) * np.sin(ang)], axis=1))
    return np.stack(out), np.full(2, 0.4)


def make(shape, v):
    B = shape["agents"]
    fleet = "plans" in v
    e = pkg.Engine(K=shape["K"], n_agents=B, obstacle_motion=1, precision=capi.PREC_F32, fleet_radius=0.3 if fleet else 0.0, **diff_cfg())
    if len(v) >= 2:
        e.set_scene_mode("composed")
    x0 = []
    for a in range(B):
        turn = 2.0 * np.pi * a / B
        e.set_ref_path(ring_path(turn)[:, :e.nx], agent=a if B > 1 else None)
        x0.append([RING_R * np.cos(turn), RING_R * np.sin(turn), turn + 0.5 * np.pi])
        if "tracks" in v:
            e.set_obstacle_tracks(*tracks_of(turn), agent=a if B > 1 else None)
    if fleet:
        e.set_fleet_prediction("plan")
    if "grid" in v:
        e.set_cost_grid(**grid_of())
    e.set_state(np.array(x0) if B > 1 else np.array(x0[0]))
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
    VS = variants(shape["agents"])
    handles = {v: make(shape, v) for v in VS}
    wall = {v: [] for v in VS}
    launch = {v: [] for v in VS}
    for _ in range(ROUNDS):
        for v in VS:
            w, r = one_round(handles[v])
            wall[v].append(w)
            launch[v].append(r)
    med_l = {v: statistics.median(launch[v]) for v in VS}
    med_w = {v: statistics.median(wall[v]) for v in VS}

    def over(med):
        return {name_of(v): (med[v] - med[()]) - sum(med[(p,)] - med[()] for p in v) for v in VS if len(v) >= 2}
    out = {"shape": shape["name"], "K": shape["K"], "T": T, "agents": shape["agents"], "iterations": N_ITER,
           "kernels": {name_of(v): handles[v].rollout_kernel() for v in VS},
           "rollout_launch_us": {name_of(v): spread(launch[v]) for v in VS},
           "us_per_iteration": {name_of(v): spread(wall[v]) for v in VS},
           "increment_over_spec3_us": {name_of(v): {"rollout_launch": med_l[v] - med_l[()], "per_iteration": med_w[v] - med_w[()]} for v in VS if v},
           "over_sum_of_parts_us": {"rollout_launch": over(med_l), "per_iteration": over(med_w)},
           "n_collided_last": {name_of(v): int(handles[v].stats.n_collided) for v in VS}}
    for e in handles.values():
        e.close()
    lines.append(out)
    print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
