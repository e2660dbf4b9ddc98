#!/usr/bin/env python3
"""What the scene forms of the learned rollout cost: the rollout kernel of one call at K = 32768, T = 50 for
128 x 3 and 512 x 3 -- the static form with 0 and 8 circles, the scene form with 8 moving circles, with 8 tracks added, with a
512 x 512 grid added under the centre, and the same grid under the outline -- handles alternated, five rounds, median (min - max)
of the in-situ kernel time (event pair minus the empty-pair calibration).  Writes profiles/mlp_scene.json.

    python tools/mlp_scene.py [--out profiles/mlp_scene.json] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

K, T = 32768, 50
CONFIGS = ("static, no circles", "static, 8 circles", "scene, 8 moving circles", "scene, + 8 tracks", "scene, + 512 x 512 grid (centre)",
           "scene, + 512 x 512 grid (outline)")


def make(H, n, which):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    from oracle import mppi_oracle
    from test_gpu_mlp_shapes import weights
    scene = which >= 2
    cfg = dict(model=capi.MODEL_DIFFDRIVE_MLP, K=K, T=T, delta_t=0.1, u_max=[5.0, 3.14], param_exploration=0.05, param_lambda=1.0,
               param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01], stage_cost_weight=[5, 5, 10, 0], terminal_cost_weight=[5, 5, 10, 0],
               search_window=20, filter_window=10, clamp_rollout=1, waypoint_mode=capi.WAYPOINT_FROZEN, accumulate_stage_cost=1,
               obstacle_model=capi.OBSTACLE_OUTLINE if which > 0 else capi.OBSTACLE_NONE, safety_margin=1.0, vehicle_l=0.75, vehicle_w=0.5,
               collision_penalty=1e10, seed=5, precision=capi.PREC_F32, obstacle_motion=2 if scene else 0)
    e = pkg.Engine(**cfg)
    e.set_mlp(weights(H, n, 3))
    e.set_ref_path(mppi_oracle.generate_point_trajectory((0.0, 0.0), (10.0, -5.0), 100))
    rng = np.random.default_rng(1)
    circles = np.column_stack([rng.uniform(1, 4, 8), rng.uniform(-3, 0, 8), np.full(8, 0.2)])
    if which == 1:
        e.set_obstacles(circles)
    if scene:
        e.set_obstacles(circles, velocities=rng.uniform(-0.3, 0.3, (8, 2)))
    if which >= 3:
        start = np.column_stack([rng.uniform(1, 4, 8), rng.uniform(-3, 0, 8)])
        e.set_obstacle_tracks(start[:, None, :] + np.arange(T + 1)[None, :, None] * rng.uniform(-0.03, 0.03, (8, 1, 2)), np.full(8, 0.2))
    if which >= 4:
        e.set_scene_mode("composed")
        if which == 5:
            e.set_cost_grid_footprint("outline")
        yy, xx = np.mgrid[0:512, 0:512]
        cells = 0.4 * (0.5 + 0.5 * np.sin(0.05 * xx) * np.cos(0.07 * yy))
        e.set_cost_grid(cells, origin=(-2.0, -6.0), resolution=0.015625, weight=2.0, lethal=0.75)
    e.set_state(np.array([0.1, -0.05, -0.4]))
    tt = np.arange(T)
    e.set_u_prev(np.stack([1.2 + 0.3 * np.sin(0.2 * tt), 0.05 * np.cos(0.1 * tt)], axis=1))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_scene.json"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    rows = []
    for H, n in ((128, 3), (512, 3)):
        engines = [make(H, n, w) for w in range(len(CONFIGS))]
        for e in engines:  # warm-up: attributes raised, weights in L2
            e.run_closed_loop(1)
        samples = [[] for _ in engines]
        for _ in range(args.rounds):
            for i, e in enumerate(engines):  # handles alternated
                e.enable_timing(True)
                e.run_closed_loop(1)
                torch.cuda.synchronize()
                samples[i].append(1e3 * e.last_kernel_ms()["rollout"])
                e.enable_timing(False)
        for i, e in enumerate(engines):
            us = sorted(samples[i])
            rows.append(dict(hidden=H, n_hidden=n, K=K, T=T, config=CONFIGS[i], kernel=e.rollout_kernel(), n_collided=int(e.stats.n_collided),
                             rollout_us_median=float(np.median(us)), rollout_us_min=us[0], rollout_us_max=us[-1], rounds=args.rounds))
            print(rows[-1], flush=True)
            e.close()
    with open(args.out, "w") as f:
        json.dump(dict(what="rollout kernel of one call, K = 32768, T = 50, every step priced; handles alternated", rows=rows), f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
