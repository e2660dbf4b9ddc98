"""Largest observed error / bound ratios of the merge, record and filter tests (tests/test_gpu_merge_harness.py,
tests/test_gpu_merge_records.py, tests/test_gpu_filter_windows.py; references and bounds: tests/merge_checks.py) per test family
and precision, and what the tests cost in wall time, as one JSON document: profiles/merge_measured.json.

    python3 tools/merge_report.py [--out FILE]

Runs those test files once in a child pytest (`-s`: every test prints the ratios it asserts on) and collects the printed figures;
a ratio above 1 is a failed test there.
"""
import argparse
import ast
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["tests/test_gpu_merge_harness.py", "tests/test_gpu_merge_records.py", "tests/test_gpu_filter_windows.py"]
LINE = re.compile(r"^\.*(step_end|records|merge_combine|merge_abi|filter)\W.*?\b(f32|f64)\b.*max error / bound (.*)$")
DURATION = re.compile(r"^([0-9.]+)s call\s+(tests/\S+?)::(\w+)(\[.*\])?$")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import dnn_mppi_mpc_amd as pkg
    res = subprocess.run([sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-s", "--durations=0", "--durations-min=0",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    rep = {"source_id": pkg.source_id(), "pytest_exit_code": res.returncode, "ratios": {}, "wall_time_s": {}}
    for line in res.stdout.splitlines():
        m = LINE.match(line.strip())
        if m:
            what, precision, tail = m.groups()
            found = ast.literal_eval(tail) if tail.startswith("{") else {"filter.u": float(tail)}
            slot = rep["ratios"].setdefault(what, {}).setdefault(precision, {})
            for k, v in found.items():
                slot[k] = max(slot.get(k, 0.0), float(v))
        d = DURATION.match(line.strip())
        if d:
            t = rep["wall_time_s"].setdefault(d.group(3), {"cases": 0, "total": 0.0, "slowest_case": 0.0})
            t["cases"] += 1
            t["total"] = round(t["total"] + float(d.group(1)), 3)
            t["slowest_case"] = max(t["slowest_case"], float(d.group(1)))
    rep["summary"] = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    text = json.dumps(rep, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if res.returncode == 0 and rep["ratios"] else 1


if __name__ == "__main__":
    sys.exit(main())
