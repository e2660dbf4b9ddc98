"""Latency of the callback controller at the shapes of the three callers it gained (test/test_mppi_racecar.py: K = 200, T = 50;
test/test_torch_mppi_race_car.py: K = 2000, T = 50; test/test_torch_mppi.py: K = 1000, T = 20), as one JSON document:
profiles/callback_models.json.

    python3 tools/callback_models.py [--out FILE] [--no-trace]

Per shape: the wall time of `command` (a host clock around a call that ends in a stream synchronise), of
`get_sampled_trajectories` at n = K // 10 and of `perturbed_action`, each over --calls calls after --warmup; and, from a
`rocprofv3 --kernel-trace --stats` run of its own per shape (this script started again with --shape), the kernel times the
command splits into: k_cb_shift, k_cb_rollout, k_cb_update, and those of k_cb_top and k_cb_perturbed.  The traced run's
averages include its first launches; its minima do not.  No bar is set on any of these figures.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "racecar": dict(nx=4, sigma=np.diag([0.05, 0.05]), K=200, T=50, u_min=[-0.5, -1.0], u_max=[0.5, 1.0], state=[0.0, 0.0, 0.0, 0.0]),
    "racecar_dynamic": dict(nx=4, sigma=0.1 * np.eye(2), K=2000, T=50, u_min=[-1.0, -0.5], u_max=[1.0, 0.5], state=[0.0, 0.0, 0.0, 1.0]),
    "double_integrator": dict(nx=2, sigma=np.array([[0.5]]), K=1000, T=20, u_min=[-2.0], u_max=[2.0], state=[1.0, 0.0]),
}
KERNELS = ("k_cb_shift", "k_cb_rollout", "k_cb_update", "k_cb_top", "k_cb_perturbed")


def controller(name):
    from dnn_mppi_mpc_amd.callback_mppi import MPPI, RunningCost, TerminalCost
    p = SHAPES[name]
    term = TerminalCost.double_integrator() if name == "double_integrator" else None
    return MPPI(name, getattr(RunningCost, name)(), p["nx"], p["sigma"], num_samples=p["K"], horizon=p["T"], lambda_=1.0,
                u_min=p["u_min"], u_max=p["u_max"], terminal_state_cost=term, seed=1), np.array(p["state"])


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return {"median_us": round(float(np.median(t)) * 1e6, 2), "p10_us": round(float(np.percentile(t, 10)) * 1e6, 2),
            "p90_us": round(float(np.percentile(t, 90)) * 1e6, 2), "calls": calls}


def run_shape(name, calls, warmup):
    ctrl, state = controller(name)
    n = SHAPES[name]["K"] // 10
    out = {"K": SHAPES[name]["K"], "T": SHAPES[name]["T"], "n_sampled": n}
    out["command"] = timed(lambda: ctrl.command(state), calls, warmup)
    out["get_sampled_trajectories"] = timed(lambda: ctrl.get_sampled_trajectories(state, n=n), calls, warmup)
    out["perturbed_action"] = timed(lambda: ctrl.perturbed_action, max(calls // 4, 1), max(warmup // 4, 1))
    return out


def traced(name, calls, warmup):
    """Kernel times of one shape from a rocprofv3 run of its own."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--shape", name, "--calls", str(calls), "--warmup", str(warmup)]
        res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if res.returncode != 0 or not files:
            return {"error": f"rocprofv3 run ended with {res.returncode}", "tail": res.stdout[-400:]}
        rows = {}
        with open(files[0]) as fh:
            for r in csv.DictReader(fh):
                for k in KERNELS:
                    if k in r.get("Name", ""):
                        rows[k] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                   "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="run one shape's calls and print nothing else (the traced child)")
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.shape:
        print(json.dumps(run_shape(args.shape, args.calls, args.warmup)))
        return 0
    import dnn_mppi_mpc_amd as pkg
    rep = {"source_id": pkg.source_id(), "what": "callback controller (mppi_cb_*) at the new callers' shapes; wall times around "
           "synchronous calls, kernel times from rocprofv3 --kernel-trace --stats runs of their own", "shapes": {}}
    for name in SHAPES:
        rep["shapes"][name] = run_shape(name, args.calls, args.warmup)
    if not args.no_trace:
        for name in SHAPES:
            rep["shapes"][name]["kernels"] = traced(name, args.calls, args.warmup)
    text = json.dumps(rep, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
