"""profiles/fleet_plan_measured.json: what tests/test_gpu_fleet_plan.py measured on this GPU, and the CPU reference loops
behind its behaviour figures.

  - per case and per precision the largest error / bound of the plans read back (the test's printed figures, `pytest -s`);
  - the arc scene in closed loop (T = 20, 30 iterations), smallest distance of agent 0 to a mate over the states every
    iteration starts from: on the device under both predictions (the test's print, K = 512), and by the f64 reference loops
    of tests/fleet_plan_checks.py (K = 256, the NumPy restatement of the handles' noise) under both;
  - cases passed and wall time.

    python tools/fleet_plan_report.py [--out FILE]
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fleet_checks as fc  # noqa: E402
import fleet_plan_checks as pc  # noqa: E402
import moving_obstacle_checks as mc  # noqa: E402

ARGV = sys.argv[1:]
OUT = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else None

run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_fleet_plan.py"), "-q", "-s", "-p", "no:cacheprovider"],
                     cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
text = run.stdout
rows = [dict(model=m.group(1), n_agents=int(m.group(2)), T=int(m.group(3)), precision=m.group(4), ratio=float(m.group(5)))
        for m in re.finditer(r"fleet plans (\w+) B=(\d+) T=(\d+) (f\d\d) max error / bound ([\d.]+)", text)]
beh = re.search(r"fleet plan behaviour arc smallest distance velocity ([\d.]+) plan ([\d.]+)", text)
summ = re.search(r"(\d+) passed.* in ([\d.]+)s", text)
if run.returncode != 0 or not rows or not beh or not summ:
    print(text[-3000:])
    sys.exit(run.returncode or 1)

T, n, K = 20, 30, 256
sc = pc.arc_scene(T, True)
cpu = {}
for what in ("cv", "plan"):
    ref = pc.closed_loop(sc, lambda i: fc.numpy_noise(mc.DIFF_KW["sigma"], 99, i, 3, K, T), n, K, T, what=what, accumulate=True, **mc.LOOP_KW)
    d = [float(fc.min_mate_distance(x)[0]) for x in ref["x"][:-1]]
    cpu["velocity" if what == "cv" else "plan"] = {"smallest_m": min(d), "at_iteration": d.index(min(d))}
out = {"largest_ratio": {p: max((r for r in rows if r["precision"] == p), key=lambda r: r["ratio"]) for p in ("f32", "f64")},
       "cases": rows,
       "behaviour_arc_smallest_distance_m": {"device_K512": {"velocity": float(beh.group(1)), "plan": float(beh.group(2))},
                                             "cpu_reference_K256": cpu},
       "run": {"passed": int(summ.group(1)), "seconds": float(summ.group(2))}}
print(json.dumps({k: out[k] for k in ("largest_ratio", "behaviour_arc_smallest_distance_m", "run")}, indent=1))
if OUT:
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
