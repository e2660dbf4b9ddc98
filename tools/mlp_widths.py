"""Config 5's closed loop with residual MLPs of other shapes (K = 32768, T = 50, frozen index, in-kernel Philox, seeded
random weights, fp32): H in {64, 128, 256, 512} with 3 hidden layers and H = 128 with 1, 2 and 4.  One JSON line per
shape: iteration period, rollout kernel time (event pairs, as tools/bench_configs.py), the kernel's name, the algorithmic
flop per trajectory-step 2 H (5 + n H + 3), and that flop over the kernel time as a fraction of the 2.5 PFLOP/s dense f16
peak (the split kernels issue every product three times: 3 x that is their matrix-pipe load), and the kernel time over
512 x 3's when that shape ran first.  `--out FILE` also writes them as one JSON document with the build id
(dnn_mppi_mpc_amd.source_id()), the command and the device: profiles/mlp_widths.json is

    python tools/mlp_widths.py --out profiles/mlp_widths.json

    python tools/mlp_widths.py [--out FILE] [HxN ...]      e.g. 128x3 256x3; default: the seven shapes above"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dnn_mppi_mpc_amd as pkg  # noqa: E402
from oracle import mppi_oracle as mo  # noqa: E402  (path generator / random weights only)

SHAPES = [(512, 3), (256, 3), (128, 3), (64, 3), (128, 1), (128, 2), (128, 4)]
K, T = 32768, 50


def timed(eng, n, warm):
    eng.run_closed_loop(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run_closed_loop(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def weights(H, n, seed=0):
    w = mo.random_mlp_weights(seed, hidden=H, n_hidden=n)
    for i in range(n):  # (the hidden layers' pre-activation spread of the 512-wide model at every width)
        w[f"hidden_layer.{i}.weight"] = (w[f"hidden_layer.{i}.weight"] * np.sqrt(512.0 / H)).astype(np.float32)
    return w


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    shapes = [tuple(int(v) for v in a.split("x")) for a in argv] or SHAPES
    results, base_us = [], None
    dd = dict(delta_t=0.1, max_speed=5.0, max_omega=3.14, sigma=np.array([[0.1, 0.0], [0.0, 0.01]]),
              visualize_optimal_traj=False, visualze_sampled_trajs=False)
    for H, n in shapes:
        c = pkg.MPPIAlgorithms(**dd, ref_path=mo.generate_point_trajectory((0, 0), (10, -5), 100), num_samples_K=K,
                               num_horizons_T=T, param_exploration=0.05, param_lambda=1.0, param_alpha=0.2,
                               stage_cost_weight=np.array([5.0, 5.0, 10.0]), terminal_cost_weight=np.array([5.0, 5.0, 10.0]),
                               learned_dynamics=weights(H, n), waypoint_mode="frozen")
        eng = c._engine
        eng.set_state(np.zeros(3))
        period = timed(eng, 10, 3)
        eng.enable_timing(True)  # in-situ duration of the rollout launch: event pair minus the empty-pair calibration
        eng.run_closed_loop(10)
        torch.cuda.synchronize()
        kms = eng.last_kernel_ms()
        eng.enable_timing(False)
        t_roll = max(kms["rollout"] * 1e-3, 1e-9)
        flop = 2.0 * H * (5 + n * H + 3)
        if (H, n) == (512, 3):
            base_us = 1e6 * t_roll
        r = {"hidden": H, "n_hidden": n, "K": K, "T": T, "us_per_iter": 1e6 * period,
             "rollout_kernel_us": 1e6 * t_roll, "kernel": eng.rollout_kernel(),
             "flop_per_traj_step": flop, "TFLOPs": flop * K * T / t_roll / 1e12,
             "f16_peak_frac": flop * K * T / t_roll / 2.5e15,
             "kernel_time_vs_512x3": None if base_us is None else 1e6 * t_roll / base_us}
        results.append(r)
        print(json.dumps(r), flush=True)
        del c, eng
    if out_path:
        doc = {"source_id": pkg.source_id(), "command": " ".join(["python tools/mlp_widths.py"] + argv),
               "device": torch.cuda.get_device_name(0),
               "kernel_stats": "profiles/mlp_widths_kernel_stats.csv (rocprofv3 --kernel-trace --stats of the same command, "
                               "same build)",
               "results": results}
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
