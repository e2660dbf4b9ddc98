#!/usr/bin/env python3
"""The state error of the learned rollout against the f64 oracle, from which tests/mlp_scene_checks.py takes its margin DELTA
(DESIGN 3.16): for every shape and horizon of the scene cases one iteration with injected noise and the sampled-trajectory
visualisation on a handle WITHOUT a scene -- the transition code is the same in the static and the scene forms -- compared
state by state with mppi_oracle.DiffDriveMlpOracle.viz_trajectories.  Writes profiles/mlp_scene_measured.json.

    python tools/mlp_scene_report.py [--out profiles/mlp_scene_measured.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_scene_measured.json"))
    args = ap.parse_args()
    import dnn_mppi_mpc_amd as pkg
    import mlp_scene_checks as ms
    import moving_obstacle_checks as mc
    from oracle import mppi_oracle, philox
    rows = []
    for H, n in ms.SHAPES:
        for T in (50,):  # (MPPIAlgorithms refuses T < 10 as the reference does; the first 7 steps of these rollouts are the 7-step case)
            base = mc.diff_scene(T, False)
            w = ms.scene_weights(H, n, base["x0"], base["u"])
            kw = dict({k: v for k, v in mc.DIFF_KW.items() if k != "safety_margin_rate"}, ref_path=base["ref"], num_samples_K=ms.K,
                      num_horizons_T=T, visualize_optimal_traj=True, visualze_sampled_trajs=True)
            eps = philox.sample_epsilon(kw["sigma"], 0, 0, ms.K, T)
            o = mppi_oracle.DiffDriveMlpOracle(**kw, mlp_weights=w)
            o.u_prev[:] = base["u"]
            ref = o.iteration(base["x0"], eps.astype(np.float64))
            _, smp_ref = o.viz_trajectories(base["x0"], ref["u_pre_shift"], ref["v"])
            c = pkg.MPPIAlgorithms(**kw, learned_dynamics=w)
            c.u_prev[:] = base["u"]
            c._calc_epsilon = lambda *a, **k: eps
            _, _, _, smp = c._calc_input_control(base["x0"])
            smp, smp_ref = np.asarray(smp, np.float64), np.asarray(smp_ref, np.float64)
            pos = float(np.max(np.hypot(smp[..., 0] - smp_ref[..., 0], smp[..., 1] - smp_ref[..., 1])))
            yaw = float(np.max(np.abs(smp[..., 2] - smp_ref[..., 2])))
            rows.append(dict(hidden=H, n_hidden=n, T=T, K=ms.K, kernel=c._engine.rollout_kernel(), max_position_error=pos, max_yaw_error=yaw))
            print(rows[-1], flush=True)
    out = dict(what="largest |state - f64 oracle| of the learned rollout's sampled trajectories over the scene cases' shapes; measured on handles "
                    "without a scene (the static kernels, whose device text the scene forms' change left as it was) at T = 50, "
                    "whose first 7 steps are the 7-step cases",
               max_position_error=max(r["max_position_error"] for r in rows), max_yaw_error=max(r["max_yaw_error"] for r in rows), rows=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
