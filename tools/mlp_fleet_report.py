"""profiles/mlp_fleet_measured.json: what tests/test_gpu_mlp_fleet.py measured on this GPU.

  - per case the largest error / bound of the mates' rows read back (fleet_checks' f32 model) and the largest distance of a plan
    point read back from `mlp_fleet_checks.learned_plans`, in units of DELTA = mlp_scene_checks.delta() (the test's printed
    figures, `pytest -s`): above 1 the plan kernels would not share the rollout's arithmetic;
  - cases passed and wall time.

    python tools/mlp_fleet_report.py [--out FILE]
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlp_scene_checks as ms  # noqa: E402

ARGV = sys.argv[1:]
OUT = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else None

run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_mlp_fleet.py"), "-q", "-s", "-p", "no:cacheprovider"],
                     cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
text = run.stdout
rows = [dict(n_agents=int(m.group(1)), own=m.group(2), ratio=float(m.group(3)))
        for m in re.finditer(r"learned fleet rows B=(\d+) own=(\w+) max error / bound ([\d.]+)", text)]
plans = [dict(n_agents=int(m.group(1)), T=int(m.group(2)), shape=m.group(3), per_agent=m.group(4) == "True", ratio=float(m.group(5)))
         for m in re.finditer(r"learned fleet plans B=(\d+) T=(\d+) (\d+x\d+) per_agent=(\w+) max error / DELTA ([\d.]+)", text)]
summ = re.search(r"(\d+) passed.* in ([\d.]+)s", text)
if run.returncode != 0 or not rows or not plans or not summ:
    print(text[-3000:])
    sys.exit(run.returncode or 1)
out = {"delta_m": ms.delta(), "largest_plan_error_over_delta": max(plans, key=lambda r: r["ratio"]),
       "largest_row_error_over_bound": max(rows, key=lambda r: r["ratio"]), "plans": plans, "rows": rows,
       "run": {"passed": int(summ.group(1)), "seconds": float(summ.group(2))}}
print(json.dumps({k: out[k] for k in ("delta_m", "largest_plan_error_over_delta", "largest_row_error_over_bound", "run")}, indent=1))
if OUT:
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
