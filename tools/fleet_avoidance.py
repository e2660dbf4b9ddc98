"""What fleet avoidance costs (mppi_config.fleet_radius): batched diff-drive agents, f32, K = 4096, T = 50, frozen
waypoint index, n_agents in {2, 8, 32, 65}; per size three handles in one process, alternated, five rounds:
  (a) fleet on                   -- every agent tests its n_agents - 1 mates; one k_fleet_rows launch leads every slot
  (b) fleet off, as many circles -- every agent given n_agents - 1 far-away zero-velocity circles of its own: the same rollout
                                    work, no row launch
  (c) fleet off, no circles      -- the moving instantiation with an empty table
(a) - (b) is the price of the row launch, (b) - (c) that of the collision tests.  Per handle and round: wall microseconds per
iteration of mppi_run_closed_loop, and the kernel time per iteration by the library's event pairs (mppi_last_kernel_ms:
rollout bracket -- which holds the row launch --, merge, finalize).  Medians and spread (min, max) over the rounds.

    python tools/fleet_avoidance.py [--out FILE] [--iters N] [--rounds R]
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
SIZES = (2, 8, 32, 65)
VARIANTS = ("fleet on", "fleet off, as many circles", "fleet off, no circles")


def cfg(B, fleet):
    return dict(model=capi.MODEL_DIFFDRIVE, precision=capi.PREC_F32, K=K, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05,
                param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0],
                terminal_cost_weight=[5, 5, 10, 0], search_window=20, filter_window=10, clamp_rollout=1,
                waypoint_mode=capi.WAYPOINT_FROZEN, obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10,
                seed=5, n_agents=B, obstacle_motion=1, fleet_radius=RADIUS if fleet else 0.0)


def make(B, variant):
    """Agents on parallel paths 3 m apart (neighbours in sight of each other, nobody in contact), long enough for every run."""
    e = pkg.Engine(**cfg(B, variant == "fleet on"))
    t = np.linspace(0.0, 1.0, 4000)
    x0 = []
    for a in range(B):
        e.set_ref_path(np.stack([1000.0 * t, np.full_like(t, 3.0 * a), np.zeros_like(t)], axis=1), agent=a)
        x0.append([0.0, 3.0 * a, 0.0])
        if variant == "fleet off, as many circles":
            far = np.array([[1.0e6 + 10.0 * i, -1.0e6, RADIUS] for i in range(B - 1)])
            e.set_obstacles(far, agent=a, velocities=np.zeros((B - 1, 2)))
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
                      "circles_per_agent": handles[v].agent_circles(0)[0].shape[0], "wall_us_per_iteration": spread(wall),
                      "rollout_bracket_us": spread(roll), "kernel_us_per_iteration": spread(kern)})
        print(json.dumps(lines[-1]), flush=True)
    a, b, c = (med[v] for v in VARIANTS)
    lines.append({"n_agents": B, "variant": "differences of medians",
                  "row_launch_us": {"wall": a[0] - b[0], "rollout_bracket": a[1] - b[1], "kernels": a[2] - b[2]},
                  "collision_tests_us": {"wall": b[0] - c[0], "rollout_bracket": b[1] - c[1], "kernels": b[2] - c[2]}})
    print(json.dumps(lines[-1]), flush=True)
    for e in handles.values():
        e.close()
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
