"""What the fleet's plan mode costs against its velocity mode (mppi_set_fleet_prediction): the handle shape of
tools/fleet_avoidance.py -- batched diff-drive agents, f32, K = 4096, T = 50, frozen waypoint index, n_agents in {2, 8, 32, 65},
parallel paths 3 m apart -- and per size three handles in one process, alternated, five rounds:
  (v) velocity mode -- k_fleet_rows leads every slot, the mates are rows of every agent's table (k_rollout_fused<.., 3>)
  (p) plan mode     -- k_fleet_plan leads every slot, the mates come from the plan table (k_rollout_fused<.., 4>)
  (o) fleet off     -- the moving instantiation with an empty table, no launch in front
(v) is the baseline; (p) - (v) is what the plans cost or save, launch and rollout form together (the two share one event
bracket: a kernel trace separates them, below).  Per handle and round: wall microseconds per iteration of
mppi_run_closed_loop, and the kernel time per iteration by the library's event pairs (mppi_last_kernel_ms).

    python tools/fleet_plan_cost.py [--out FILE] [--iters N] [--rounds R] [--sizes 2,8,32,65]

The two leading launches apart (k_fleet_plan against k_fleet_rows) come from a kernel trace of one size at a time:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fleet_plan_cost.py --sizes 32 --iters 100 --rounds 1
(the trace's average durations per kernel name; profiles/fleet_plan_kernel_stats.json keeps them).
"""
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
K, T, RADIUS = 4096, 50, 0.4
SIZES = tuple(int(v) for v in ARGV[ARGV.index("--sizes") + 1].split(",")) if "--sizes" in ARGV else (2, 8, 32, 65)
VARIANTS = ("velocity", "plan", "fleet off")


def cfg(B, fleet):
    return dict(model=capi.MODEL_DIFFDRIVE, precision=capi.PREC_F32, K=K, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0],
                terminal_cost_weight=[5, 5, 10, 0], search_window=20, filter_window=10, clamp_rollout=1,
                waypoint_mode=capi.WAYPOINT_FROZEN, obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10,
                seed=5, n_agents=B, obstacle_motion=1, fleet_radius=RADIUS if fleet else 0.0)


def make(B, variant):
    e = pkg.Engine(**cfg(B, variant != "fleet off"))
    if variant == "plan":
        e.set_fleet_prediction("plan")
    t = np.linspace(0.0, 1.0, 4000)
    x0 = []
    for a in range(B):
        e.set_ref_path(np.stack([1000.0 * t, np.full_like(t, 3.0 * a), np.zeros_like(t)], axis=1), agent=a)
        x0.append([0.0, 3.0 * a, 0.0])
    e.set_state(np.array(x0))
    e.run_closed_loop(50)
    return e


def measure(e):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run_closed_loop(N_ITER)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e.enable_timing(True)
    e.run_closed_loop(200)
    ms = e.last_kernel_ms()
    e.enable_timing(False)
    return 1e6 * wall / N_ITER, 1e3 * ms["rollout"], 1e3 * (ms["rollout"] + ms["reduce"] + ms["finalize"])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


lines = []
for B in SIZES:
    handles = {v: make(B, v) for v in VARIANTS}
    got = {v: ([], [], []) for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:  # alternated: one measurement of each per round
            for dst, val in zip(got[v], measure(handles[v])):
                dst.append(val)
    med = {}
    for v in VARIANTS:
        wall, roll, kern = got[v]
        med[v] = (statistics.median(wall), statistics.median(roll), statistics.median(kern))
        lines.append({"n_agents": B, "variant": v, "K": K, "T": T, "iterations": N_ITER, "rounds": ROUNDS, "kernel": handles[v].rollout_kernel(),
                      "wall_us_per_iteration": spread(wall), "rollout_bracket_us": spread(roll), "kernel_us_per_iteration": spread(kern)})
        print(json.dumps(lines[-1]), flush=True)
    v_, p_, o_ = (med[v] for v in VARIANTS)
    lines.append({"n_agents": B, "variant": "differences of medians",
                  "plan_minus_velocity_us": {"wall": p_[0] - v_[0], "rollout_bracket": p_[1] - v_[1], "kernels": p_[2] - v_[2]},
                  "velocity_minus_off_us": {"wall": v_[0] - o_[0], "rollout_bracket": v_[1] - o_[1], "kernels": v_[2] - o_[2]},
                  "velocity_wall_spread_us": max(got["velocity"][0]) - min(got["velocity"][0])})
    print(json.dumps(lines[-1]), flush=True)
    for e in handles.values():
        e.close()
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
