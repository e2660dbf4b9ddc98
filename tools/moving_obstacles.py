"""What moving obstacles cost (mppi_config.obstacle_motion): the same scene with circles that stand still and with
circles that move, closed loops on the device, frozen waypoint index (so that nothing but the collision test differs).

    python tools/moving_obstacles.py [--out FILE] [--iters N]

Three shapes: config 3's (diff-drive, K = 16384, T = 50, 2 circles), config 4's (race car, K = 65536, T = 75, 2 circles) and 32
batched diff-drive agents of K = 4096 with their own sets.  Per shape three handles:
  static, default layout      -- what a handle without obstacle motion runs today
  static, one sample per wave -- MPPI_DUAL=0 MPPI_PAIR=0 MPPI_TRI=0: k_rollout_fused<..., SPEC = 0>, the layout the moving forms live in
  moving                      -- k_rollout_fused<..., SPEC = 3>
so that the price of being confined to the one-sample-per-wave layout and the price of the motion itself are on record apart.
Timed by event pairs around the rollout launch (mppi_last_kernel_ms) and by wall time per iteration of mppi_run_closed_loop.
Prints one JSON line per handle; --out FILE writes them as one JSON document tagged with the build id."""
import json
import os
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
N_ITER = int(ARGV[ARGV.index("--iters") + 1]) if "--iters" in ARGV else 1000
ONE_PER_WAVE = {"MPPI_DUAL": "0", "MPPI_PAIR": "0", "MPPI_TRI": "0"}


def line_path(p, q, n):
    t = np.linspace(0.0, 1.0, n)
    yaw = np.arctan2(q[1] - p[1], q[0] - p[0])
    return np.stack([p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]), np.full(n, yaw), np.full(n, 5.0)], axis=1)


def diff_cfg(T):
    return dict(model=capi.MODEL_DIFFDRIVE, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
                param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
                search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=capi.WAYPOINT_FROZEN,
                obstacle_model=capi.OBSTACLE_CIRCLE, safety_margin=0.8, collision_penalty=1e10, seed=5)


def race_cfg(T):
    return dict(model=capi.MODEL_RACECAR, T=T, delta_t=0.05, u_max=[0.523, 2.0], wheel_base=2.5, param_exploration=0.1,
                param_lambda=50.0, param_alpha=0.9, sigma=[0.5, 0.0, 0.0, 0.1], stage_cost_weight=[50.0, 50.0, 1.0, 20.0],
                terminal_cost_weight=[50.0, 50.0, 1.0, 20.0], beta_mode=capi.BETA_INV_LAMBDA, accumulate_stage_cost=1,
                waypoint_mode=capi.WAYPOINT_FROZEN, search_window=200, wrap_yaw_stage=1, wrap_yaw_terminal=1, clamp_rollout=1,
                clamp_u_after_update=1, filter_mode=capi.FILTER_RACECAR, filter_window=10, obstacle_model=capi.OBSTACLE_OUTLINE,
                safety_margin=1.5, vehicle_w=3.0, vehicle_l=4.0, collision_penalty=1e10, seed=7)


SHAPES = [
    dict(name="config 3 shape", cfg=diff_cfg(50), K=16384, agents=1, x0=[0.0, 0.0, -0.46]),
    dict(name="config 4 shape", cfg=race_cfg(75), K=65536, agents=1, x0=[0.0, 0.0, -0.46, 5.0]),
    dict(name="32 agents of K = 4096, own sets", cfg=diff_cfg(50), K=4096, agents=32, x0=[0.0, 0.0, -0.46]),
]
PATH = line_path((0.0, 0.0), (1000.0, -500.0), 4000)  # (long enough that no closed loop here reaches its end)


def scene(a):
    """Agent a's two circles beside the start of the path and their velocities (slow: they stay in reach for the whole run)."""
    circles = np.array([[3.0 + 0.1 * a, -0.2, 0.4], [5.0, -3.8 - 0.1 * a, 0.5]])
    vel = np.array([[0.02, -0.03], [-0.02, 0.01]])
    return circles, vel


def measure(shape, variant):
    env = dict(ONE_PER_WAVE) if variant != "static, default layout" else {}
    saved = {k: os.environ.get(k) for k in ONE_PER_WAVE}
    for k in ONE_PER_WAVE:
        os.environ.pop(k, None)
    os.environ.update(env)
    moving = variant == "moving"
    B = shape["agents"]
    try:
        e = pkg.Engine(K=shape["K"], n_agents=B, obstacle_motion=int(moving), precision=capi.PREC_F32, **shape["cfg"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    e.set_ref_path(PATH[:, :e.nx])
    for a in range(B):
        circles, vel = scene(a)
        e.set_obstacles(circles, agent=a if B > 1 else None, velocities=vel if moving else None)
    x0 = np.asarray(shape["x0"], dtype=np.float64)
    e.set_state(np.tile(x0, (B, 1)) if B > 1 else x0)
    e.run_closed_loop(100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run_closed_loop(N_ITER)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e.enable_timing(True)
    e.run_closed_loop(200)
    ms = e.last_kernel_ms()
    e.enable_timing(False)
    out = {"shape": shape["name"], "variant": variant, "K": shape["K"], "T": shape["cfg"]["T"], "agents": B, "iterations": N_ITER,
           "kernel": e.rollout_kernel(), "us_per_iteration": 1e6 * wall / N_ITER, "rollout_launch_us": 1e3 * ms["rollout"],
           "n_collided_last": int(e.stats.n_collided)}
    e.close()
    return out


lines = []
for shape in SHAPES:
    for variant in ("static, default layout", "static, one sample per wave", "moving"):
        lines.append(measure(shape, variant))
        print(json.dumps(lines[-1]), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump({"source_id": pkg.source_id(), "device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)
        f.write("\n")
