"""What a learned-dynamics fleet costs (mppi_config.obstacle_motion = 3): batched learned handles, K = 4096 per
agent, T = 50, frozen waypoint index, every step priced, parallel paths 3 m apart, shapes 64 x 1, 128 x 3 and 512 x 3,
n_agents in {2, 8, 32}; per shape and size three handles in one process, alternated, five rounds:
  (v) velocity mode -- k_fleet_rows<float> leads every slot, the mates are rows of every agent's moving table
  (p) plan mode     -- k_fleet_plan_mlp_* leads every slot, the mates come from the plan table
  (s) the value-2 batch (k_rollout_mlp_*_scene_agents) with n_agents - 1 own circles per agent out of reach: the fleet forms'
      twin on the same number of table rows, no launch in front
Per handle and round: the rollout bracket of the library's event pairs (mppi_last_kernel_ms: the front launch and the rollout
launch together) and the kernel time per iteration.  (p) - (v) is what the plan launch and the plan test cost over the rows.

    python tools/mlp_fleet_cost.py [--out FILE] [--iters N] [--rounds R] [--sizes 2,8,32] [--shapes 64x1,128x3,512x3]
                                   [--variants velocity,plan,twin]

The launches apart -- k_fleet_plan_mlp_* and k_fleet_rows on their own, and the rollout launch behind each -- come from kernel
traces of one size and one variant at a time (a kernel's name does not say which handle launched it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mlp_fleet_cost.py --sizes 8 --variants plan --iters 20 --rounds 1
(the traces' average durations per kernel name; profiles/mlp_fleet_kernel_stats.json keeps them).
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import dnn_mppi_mpc_amd as pkg  # noqa: E402
from dnn_mppi_mpc_amd import _capi as capi  # noqa: E402
from test_gpu_mlp_shapes import weights  # noqa: E402

ARGV = sys.argv[1:]
OUT = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else None
N_ITER = int(ARGV[ARGV.index("--iters") + 1]) if "--iters" in ARGV else 40
ROUNDS = int(ARGV[ARGV.index("--rounds") + 1]) if "--rounds" in ARGV else 5
K, T, RADIUS = 4096, 50, 0.4
SIZES = tuple(int(v) for v in ARGV[ARGV.index("--sizes") + 1].split(",")) if "--sizes" in ARGV else (2, 8, 32)
SHAPES = tuple(tuple(int(x) for x in s.split("x")) for s in
               (ARGV[ARGV.index("--shapes") + 1] if "--shapes" in ARGV else "64x1,128x3,512x3").split(","))
VARIANTS = tuple({"twin": "value 2 twin"}.get(v, v) for v in ARGV[ARGV.index("--variants") + 1].split(",")) if "--variants" in ARGV \
    else ("velocity", "plan", "value 2 twin")


def cfg(B, fleet):
    return dict(model=capi.MODEL_DIFFDRIVE_MLP, precision=capi.PREC_F32, K=K, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0],
                terminal_cost_weight=[5, 5, 10, 0], search_window=20, filter_window=10, clamp_rollout=1, accumulate_stage_cost=1,
                waypoint_mode=capi.WAYPOINT_FROZEN, obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10,
                seed=5, n_agents=B, obstacle_motion=3 if fleet else 2, fleet_radius=RADIUS if fleet else 0.0)


def make(B, shape, variant):
    e = pkg.Engine(**cfg(B, variant != "value 2 twin"))
    for a in range(B):
        e.set_mlp(weights(*shape, 100 + a), agent=a)
    t = np.linspace(0.0, 1.0, 4000)
    x0 = []
    for a in range(B):
        e.set_ref_path(np.stack([1000.0 * t, np.full_like(t, 3.0 * a), np.zeros_like(t)], axis=1), agent=a)
        x0.append([0.0, 3.0 * a, 0.0])
    if variant == "value 2 twin":  # as many rows as a fleet table has, none in reach
        far = np.stack([np.full(B - 1, -500.0), 100.0 * np.arange(B - 1), np.full(B - 1, RADIUS)], axis=1)
        e.set_obstacles(far, velocities=np.zeros((B - 1, 2)))
    if variant == "plan":
        e.set_fleet_prediction("plan")
    e.set_state(np.array(x0))
    e.run_closed_loop(5)
    return e


def measure(e):
    e.enable_timing(True)
    e.run_closed_loop(N_ITER)
    torch.cuda.synchronize()
    ms = e.last_kernel_ms()
    e.enable_timing(False)
    return 1e3 * ms["rollout"], 1e3 * (ms["rollout"] + ms["reduce"] + ms["finalize"])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


lines = []
for shape in SHAPES:
    for B in SIZES:
        handles = {v: make(B, shape, v) for v in VARIANTS}
        got = {v: ([], []) for v in VARIANTS}
        for _ in range(ROUNDS):
            for v in VARIANTS:  # alternated: one measurement of each per round
                for dst, val in zip(got[v], measure(handles[v])):
                    dst.append(val)
        med = {v: statistics.median(got[v][0]) for v in VARIANTS}
        for v in VARIANTS:
            lines.append({"shape": "%dx%d" % shape, "n_agents": B, "variant": v, "K": K, "T": T, "iterations": N_ITER, "rounds": ROUNDS,
                          "kernel": handles[v].rollout_kernel(), "rollout_bracket_us": spread(got[v][0]),
                          "kernel_us_per_iteration": spread(got[v][1])})
            print(json.dumps(lines[-1]), flush=True)
        if len(med) == 3:
            lines.append({"shape": "%dx%d" % shape, "n_agents": B, "variant": "differences of medians (rollout bracket, us)",
                          "plan_minus_velocity": med["plan"] - med["velocity"], "velocity_minus_twin": med["velocity"] - med["value 2 twin"],
                          "twin_spread": max(got["value 2 twin"][0]) - min(got["value 2 twin"][0])})
            print(json.dumps(lines[-1]), flush=True)
        for e in handles.values():
            e.close()
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
