"""Observed maxima of the device primitives against their f64 references (the comparisons of tests/prims_checks.py, which
tests/test_gpu_primitives.py bounds), as one JSON document: profiles/prims_measured.json.

    python3 tools/prims_report.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dnn_mppi_mpc_amd as pkg  # noqa: E402
import prims_checks as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    P = pc.Prims(pkg.build.prims_library())
    rep = {"source_id": pkg.source_id()}
    rep["sincos_"] = dict(pc.sincos_errors(P), bound_ulp=2.0, bound_library_abs=2.0 ** -22)
    rep["tan_"] = dict(pc.tan_errors(P), bound_ulp=2.0)
    r, a, circ = pc.pymod_check(P)
    rep["pymod"] = {"circular_err": float(circ.max()), "worst_a": float(a[circ.argmax()]), "bound": 2.0 ** -21,
                    "out_of_range": int((~((r >= 0) & (r < pc.PYMOD_M))).sum())}
    rel, bound = pc.exp_rel_err(P)
    rep["exp_"] = {"rel_err": float(rel.max()), "max_err_over_bound": float((rel / bound).max()),
                   "bound": "(2|x| + 4) 2^-24 on [-87, 0]"}
    rep["box_muller"] = {"abs_err": float(pc.box_muller_abs_err(P).max()), "bound": 4e-6}
    rep["collision"] = {"margin": pc.COLLISION_MARGIN, "poses": pc.N_POSES,
                        "flips": {f"{pc._sfx(t)}_n_obs_{n}": pc.collision_check(P, n, t) for t in (np.float32, np.float64)
                                  for n in pc.N_OBS}}
    rep["lb_scan"] = {}
    for t in (np.float32, np.float64):
        cand, pos, m, bad, compared = pc.lb_real_reference(t)
        gm, gb = P.lb_scan(1, cand, pos)
        rep["lb_scan"][pc._sfx(t)] = {"calls": int(m.size), "margin": pc.LB_GAP[t], "share_left_out": float(1.0 - compared.mean()),
                                      "bound_share_left_out": pc.LB_LEFT_OUT_MAX,
                                      "mismatches_compared": int((compared & ((gm != m) | (gb != bad))).sum()),
                                      "mismatches_left_out": int((~compared & ((gm != m) | (gb != bad))).sum())}
    text = json.dumps(rep, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
