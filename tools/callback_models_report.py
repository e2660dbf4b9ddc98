"""Measured ratios of tests/test_gpu_callback_models.py (references, error rule and cases: tests/callback_models_checks.py) for
every case, as one JSON document: profiles/callback_models_measured.json.  The sibling of tools/callback_report.py.

    python3 tools/callback_models_report.py [--out FILE]

cost_total, trajectory and models.*: the device's distance from the f64 definition over the unchanged f32 restatement's own
distance on the same inputs; the tests hold it to callback_checks.COST_FACTOR (floored at one f32 ulp of the largest term,
so a ratio above the factor passes where the restatement happens to land exactly), and a ratio above
callback_checks.COST_RATIO_FINDING is a defect to explain.  omega, U, sampler: the device's error over the bound of its error
model, a ratio above 1 is a failed test there.  Runs that test file once in a child pytest (`-s`) and collects what it prints.
"""
import argparse
import ast
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["tests/test_gpu_callback_models.py"]
LINE = re.compile(r"^\.*callback models (cost_total|omega|U|sampler|trajectory) (\S+): (?:.* )?ratio (\S+)$")
MODELS = re.compile(r"^\.*callback models (\S+): device / restatement ratio (\{.*\})$")
DURATION = re.compile(r"^([0-9.]+)s call\s+(tests/\S+?)::(\w+)(\[.*\])?$")


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
    held = [k for k in rep["largest"] if k in ("cost_total", "trajectory") or k.startswith("models.")]
    rep["cost_factor"] = {"in_callback_checks": cc.COST_FACTOR, "finding_above": cc.COST_RATIO_FINDING,
                          "largest_ratio_held_to_it": max([rep["largest"][k] for k in held], default=None)}
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
