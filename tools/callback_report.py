"""Measured ratios of the callback-controller tests (tests/test_gpu_callback_edges.py; references, bounds and cases:
tests/callback_checks.py) for every case, as one JSON document: profiles/callback_measured.json.

    python3 tools/callback_report.py [--out FILE]

cost_total: the device's distance from the f64 reference over the f32 restatement's own distance (the rule that fixes
callback_checks.COST_FACTOR: the smallest power of two that is at least twice the largest of these); omega, U, sampler, models:
the device's error over the bound of its error model, a ratio above 1 is a failed test there.  Runs that test file once in a
child pytest (`-s`: every test prints the figures it asserts on) and collects them.
"""
import argparse
import ast
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["tests/test_gpu_callback_edges.py"]
LINE = re.compile(r"^\.*callback (cost_total|omega|U|sampler) (\S+): (?:.* )?ratio (\S+)$")
MODELS = re.compile(r"^\.*callback models (\S+): max error / bound (\{.*\})$")
DURATION = re.compile(r"^([0-9.]+)s call\s+(tests/\S+?)::(\w+)(\[.*\])?$")


def factor_for(largest):
    """The smallest power of two that is at least twice ``largest``."""
    f = 1
    while f < 2.0 * largest:
        f *= 2
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import callback_checks as cc
    import dnn_mppi_mpc_amd as pkg
    res = subprocess.run([sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-s", "--durations=0", "--durations-min=0",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    rep = {"source_id": pkg.source_id(), "pytest_exit_code": res.returncode, "ratios": {}, "wall_time_s": {}}
    for line in res.stdout.splitlines():
        m = LINE.match(line.strip())
        if m:
            rep["ratios"].setdefault(m.group(1), {})[m.group(2)] = float(m.group(3))
        m = MODELS.match(line.strip())
        if m:
            for what, v in ast.literal_eval(m.group(2)).items():
                rep["ratios"].setdefault("models." + what, {})[m.group(1)] = float(v)
        d = DURATION.match(line.strip())
        if d:
            t = rep["wall_time_s"].setdefault(d.group(3), {"cases": 0, "total": 0.0, "slowest_case": 0.0})
            t["cases"] += 1
            t["total"] = round(t["total"] + float(d.group(1)), 3)
            t["slowest_case"] = max(t["slowest_case"], float(d.group(1)))
    rep["largest"] = {k: max(v.values()) for k, v in rep["ratios"].items()}
    if "cost_total" in rep["largest"]:
        rep["cost_factor"] = {"rule": "smallest power of two >= 2 x the largest cost_total ratio",
                              "from_this_run": factor_for(rep["largest"]["cost_total"]), "in_callback_checks": cc.COST_FACTOR}
    rep["summary"] = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    text = json.dumps(rep, indent=1, sort_keys=True)
    print(text)
    if res.returncode != 0:
        print(res.stdout[-6000:], file=sys.stderr)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if res.returncode == 0 and rep["ratios"] else 1


if __name__ == "__main__":
    sys.exit(main())
