"""Learned dynamics with several agents per handle: config 5's closed loop (T = 50, frozen index, in-kernel
Philox, seeded random weights, fp32) for residual MLPs of H in {64, 128, 256, 512} x 3 hidden layers, K in {1024, 4096}
samples per agent and B in {1, 2, 4, 8, 16, 32} agents in one handle.  B = 1 is a single-agent handle (the single-agent
kernels); B > 1 runs k_rollout_mlp_h3_agents / k_rollout_mlp_w_agents, one launch for all agents.  One JSON line per point:
iteration period for all agents, rollout kernel time (event pairs, as tools/mlp_widths.py), the kernel's name, aggregate
trajectory-steps/s (B K T over the period), and vs_single = B x (the single-agent handle's period) / (the batched period):
what one handle for B agents gains over B single-agent handles run one after the other.  `--out FILE` also writes them as
one JSON document with the build id (dnn_mppi_mpc_amd.source_id()), the command and the device: profiles/mlp_agents.json is

    python tools/mlp_agents.py --out profiles/mlp_agents.json

`--own-models`: agent a of a batched handle gets its own model, the weights seeded `seed + a` (set_mlp(w_a, agent=a); the
batched kernels then stream B weight sets instead of one); without it every agent shares the weights seeded `seed`.
`--K 4096` / `--agents 8,32` restrict the points (vs_single is null without B = 1), `--seed S` moves the weights.

    python tools/mlp_agents.py [--out FILE] [--own-models] [--K K,..] [--agents B,..] [--seed S] [HxN ...]
                                                           e.g. 128x3; default: 64x3 128x3 256x3 512x3"""
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
from oracle import mppi_oracle as mo  # noqa: E402  (path generator / random weights only)

SHAPES = [(64, 3), (128, 3), (256, 3), (512, 3)]
KS = (1024, 4096)
AGENTS = (1, 2, 4, 8, 16, 32)
T = 50


def weights(H, n, seed=0):
    w = mo.random_mlp_weights(seed, hidden=H, n_hidden=n)
    for i in range(n):  # (the hidden layers' pre-activation spread of the 512-wide model at every width)
        w[f"hidden_layer.{i}.weight"] = (w[f"hidden_layer.{i}.weight"] * np.sqrt(512.0 / H)).astype(np.float32)
    return w


def engine(K, B, w, own=None):
    """Config 5's diff-drive parameters (as tools/mlp_widths.py), frozen index, B agents a little apart.  `own`: one model
    per agent instead of `w` for all."""
    e = pkg.Engine(model=capi.MODEL_DIFFDRIVE_MLP, K=K, T=T, n_agents=B, delta_t=0.1, u_max=[5.0, 3.14],
                   param_exploration=0.05, param_lambda=1.0, param_alpha=0.2, sigma=[0.1, 0.0, 0.0, 0.01],
                   stage_cost_weight=[5.0, 5.0, 10.0, 0.0], terminal_cost_weight=[5.0, 5.0, 10.0, 0.0],
                   beta_mode=capi.BETA_INV_EXPLORATION, waypoint_mode=capi.WAYPOINT_FROZEN, search_window=20,
                   filter_mode=capi.FILTER_DIFFDRIVE, filter_window=10, clamp_rollout=1, collision_penalty=1e10, seed=0,
                   precision=capi.PREC_F32)
    e.set_ref_path(mo.generate_point_trajectory((0, 0), (10, -5), 100))
    if own is not None and B > 1:
        for a in range(B):
            e.set_mlp(own[a], agent=a)
    else:
        e.set_mlp(w)
    x0 = np.stack([[0.05 * a, -0.02 * a, 0.01 * a] for a in range(B)])
    e.set_state(x0 if B > 1 else x0[0])
    return e


def measure(e, n, warm):
    """(seconds per iteration over n closed-loop iterations, rollout kernel ms from event pairs)"""
    e.run_closed_loop(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run_closed_loop(n)
    torch.cuda.synchronize()
    period = (time.perf_counter() - t0) / n
    e.enable_timing(True)  # in-situ duration of the rollout launch: event pair minus the empty-pair calibration
    e.run_closed_loop(n)
    torch.cuda.synchronize()
    kms = e.last_kernel_ms()
    e.enable_timing(False)
    return period, kms["rollout"]


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    command = " ".join(["python tools/mlp_agents.py"] + [a for a in argv if a != "--out"])

    def option(name, default):
        nonlocal argv
        if name not in argv:
            return default
        i = argv.index(name)
        v = tuple(int(t) for t in argv[i + 1].split(","))
        argv = argv[:i] + argv[i + 2:]
        return v

    own_models = "--own-models" in argv
    argv = [a for a in argv if a != "--own-models"]
    ks, agents, (seed,) = option("--K", KS), option("--agents", AGENTS), option("--seed", (0,))
    shapes = [tuple(int(v) for v in a.split("x")) for a in argv] or SHAPES
    results = []
    for H, n in shapes:
        w = weights(H, n, seed)
        own = [weights(H, n, seed + a) for a in range(max(agents))] if own_models else None
        for K in ks:
            single_us = None
            for B in agents:
                e = engine(K, B, w, own)
                period, k_ms = measure(e, 30, 5)
                us = 1e6 * period
                if B == 1:
                    single_us = us
                r = {"hidden": H, "n_hidden": n, "K": K, "T": T, "agents": B, "own_models": bool(own_models and B > 1),
                     "us_per_iter": us, "rollout_kernel_us": 1e3 * k_ms, "kernel": e.rollout_kernel(),
                     "traj_steps_per_s": B * K * T / period, "vs_single": B * single_us / us if single_us else None}
                results.append(r)
                print(json.dumps(r), flush=True)
                e.close()
    if out_path:
        doc = {"source_id": pkg.source_id(), "command": command,
               "device": torch.cuda.get_device_name(0),
               "kernel_stats": "profiles/mlp_agents_kernel_stats.csv (rocprofv3 --kernel-trace --stats of the same command, "
                               "same build)",
               "results": results}
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
