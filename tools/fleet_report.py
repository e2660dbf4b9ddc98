"""What tests/test_gpu_fleet.py measured, as one JSON document: profiles/fleet_measured.json -- per precision the largest
error / bound ratio of the mates' rows against the error model of tests/fleet_checks.py, the smallest distance of the head-on
pair with the switch off and on, and what the tests cost in wall time.

    python3 tools/fleet_report.py [--out FILE] [--log FILE]

Runs that test file once in a child pytest (`-s`: the tests print the figures they assert on) and collects the printed figures;
a ratio above 1 is a failed test there.  --log keeps the child's whole output.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = re.compile(r"fleet rows (\w+) B=(\d+) own=(\w+) (f32|f64) max error / bound ([0-9.eE+-]+)")
BEHAVIOUR = re.compile(r"fleet behaviour head-on smallest distance off ([0-9.]+) on ([0-9.]+)")
DURATION = re.compile(r"^([0-9.]+)s call\s+(tests/\S+?)::(\w+)(\[.*\])?$")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import dnn_mppi_mpc_amd as pkg
    res = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_fleet.py", "-m", "gpu", "-q", "-s", "--durations=0",
                          "--durations-min=0", "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(res.stdout)
    rep = {"source_id": pkg.source_id(), "pytest_exit_code": res.returncode, "rows_max_error_over_bound": {}, "wall_time_s": {}}
    for line in res.stdout.splitlines():
        m = ROWS.search(line)
        if m:
            model, B, own, precision, ratio = m.groups()
            slot = rep["rows_max_error_over_bound"].setdefault(precision, {"max": 0.0, "cases": 0, "worst_case": ""})
            slot["cases"] += 1
            if float(ratio) >= slot["max"]:
                slot["max"], slot["worst_case"] = float(ratio), f"{model} n_agents={B} own={own}"
        m = BEHAVIOUR.search(line)
        if m:
            rep["head_on_smallest_distance_m"] = {"fleet_radius_0": float(m.group(1)), "fleet_radius_0.4": float(m.group(2))}
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
    return 0 if res.returncode == 0 and rep["rows_max_error_over_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
