"""Several independent MPPI problems (agents) on ONE GPU: one handle + one HIP stream + one host thread per agent,
closed loops on the device.  Launches of different agents overlap (one agent's serial k_finalize runs beside the
others' rollouts), so the aggregate rate exceeds the single-agent one until the rollouts fill the chip.
Prints one JSON line per agent count.

    python tools/multi_agent.py [--batched-only] [--own-scenes] [--circles M] [--mlp HxN --K K [--own-models]] [--out FILE] [agents ...]

--own-scenes: every agent of the batched handle follows its own path (the shared one shifted by the agent) and sees its own M
circles (mppi_set_agent_ref_path / mppi_set_agent_obstacles) instead of the one scene all share; --circles M: M circles beside
the path (shared, or each agent's own); --mlp HxN: the batched handles run learned dynamics of that shape (seeded random
weights, K samples per agent) instead of config 2, with --own-models agent a on its own model (the weights seeded a,
Engine.set_mlp(w, agent=a)) instead of the one all share; --batched-only skips the one-handle-per-agent part; --out FILE appends the
batched lines to FILE as JSON lines tagged with the build id."""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dnn_mppi_mpc_amd as pkg  # noqa: E402
from bench import HORIZON, K_SAMPLES, config2_kwargs  # noqa: E402

ARGV = sys.argv[1:]


def flag(name):
    if name in ARGV:
        ARGV.remove(name)
        return True
    return False


def option(name, default=None):
    if name in ARGV:
        i = ARGV.index(name)
        v = ARGV[i + 1]
        del ARGV[i:i + 2]
        return v
    return default


BATCHED_ONLY, OWN_SCENES, OWN_MODELS = flag("--batched-only"), flag("--own-scenes"), flag("--own-models")
N_CIRCLES, MLP, OUT = int(option("--circles", "0")), option("--mlp"), option("--out")
K_AGENT = int(option("--K", str(K_SAMPLES)))
N_ITER = 3000 if not MLP else 100
for n_agents in [] if BATCHED_ONLY else [int(a) for a in (ARGV or ["1", "2", "4", "8"])]:
    ctrls = [pkg.MPPIAlgorithms(**config2_kwargs(), precision="f32", seed=100 + a) for a in range(n_agents)]
    streams = [torch.cuda.Stream() for _ in ctrls]
    for c in ctrls:
        c._engine.set_state(np.zeros(3))
        c._engine.run_closed_loop(200)
    torch.cuda.synchronize()
    go = threading.Barrier(n_agents + 1)

    def work(c, s):
        go.wait()
        c._engine.run_closed_loop(N_ITER, stream=s)

    ths = [threading.Thread(target=work, args=(c, s)) for c, s in zip(ctrls, streams)]
    for t in ths:
        t.start()
    go.wait()
    t0 = time.perf_counter()
    for t in ths:
        t.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"agents": n_agents, "K": K_SAMPLES, "T": HORIZON, "iterations_each": N_ITER,
                      "us_per_iteration_per_agent": 1e6 * dt / N_ITER,
                      "aggregate_traj_steps_per_s": n_agents * K_SAMPLES * HORIZON * N_ITER / dt}))

# the same agents BATCHED in one handle: agents as a grid dimension, one launch per stage for all of them
from dnn_mppi_mpc_amd import _capi as capi  # noqa: E402

kw = config2_kwargs()


def scene(a):
    """Agent a's own path and circles: the shared ones moved by (0.3 a, 0.2 a); a = 0 is the shared scene."""
    shift = np.array([0.3 * a, 0.2 * a, 0.0])
    path = np.asarray(kw["ref_path"], dtype=np.float64) + shift
    # circles 1.5 m beside the path, spread along it
    circles = np.array([[path[(7 * i + 5) % len(path), 0] + 1.5, path[(7 * i + 5) % len(path), 1] + 1.5, 0.4] for i in range(N_CIRCLES)])
    return path, circles.reshape(-1, 3), shift


mlp_weights = None
if MLP:
    from oracle import mppi_oracle as mo  # noqa: E402  (random weights only)
    H, NH = (int(v) for v in MLP.split("x"))
    mlp_weights = mo.random_mlp_weights(0, hidden=H, n_hidden=NH)
for n_agents in [int(a) for a in (ARGV or ["1", "2", "4", "8", "16", "32"])]:
    eng = pkg.Engine(model=capi.MODEL_DIFFDRIVE_MLP if MLP else capi.MODEL_DIFFDRIVE, K=K_AGENT, T=HORIZON,
                     obstacle_model=capi.OBSTACLE_CIRCLE if N_CIRCLES else capi.OBSTACLE_NONE, safety_margin=0.8,
                     collision_penalty=1e10, delta_t=kw["delta_t"], u_max=[kw["max_speed"], kw["max_omega"]],
                     param_exploration=kw["param_exploration"], param_lambda=kw["param_lambda"], param_alpha=kw["param_alpha"],
                     sigma=np.asarray(kw["sigma"]).reshape(-1), stage_cost_weight=list(kw["stage_cost_weight"]) + [0.0],
                     terminal_cost_weight=list(kw["terminal_cost_weight"]) + [0.0], search_window=20, filter_window=10,
                     clamp_rollout=1, clamp_u_after_update=0, waypoint_mode=capi.WAYPOINT_FROZEN, seed=5, n_agents=n_agents)
    x0 = np.zeros((n_agents, 3))
    if OWN_SCENES and n_agents > 1:
        for a in range(n_agents):
            path, circles, x0[a] = scene(a)
            eng.set_ref_path(path, agent=a)
            if N_CIRCLES:
                eng.set_obstacles(circles, agent=a)
    else:
        path, circles, _ = scene(0)
        eng.set_ref_path(path)
        if N_CIRCLES:
            eng.set_obstacles(circles)
    if MLP and OWN_MODELS and n_agents > 1:
        for a in range(n_agents):
            eng.set_mlp(mo.random_mlp_weights(a, hidden=H, n_hidden=NH), agent=a)
    elif MLP:
        eng.set_mlp(mlp_weights)
    eng.set_state(x0 if n_agents > 1 else x0[0])
    eng.run_closed_loop(200 if not MLP else 10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run_closed_loop(N_ITER)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    line = {"agents_batched_in_one_handle": n_agents, "K": K_AGENT, "T": HORIZON, "iterations": N_ITER,
            "scenes": "own" if OWN_SCENES and n_agents > 1 else "shared", "circles_per_agent": N_CIRCLES, "mlp": MLP,
            "models": "own" if MLP and OWN_MODELS and n_agents > 1 else "shared" if MLP else None,
            "kernel": eng.rollout_kernel(), "us_per_iteration_all_agents": 1e6 * dt / N_ITER,
            "aggregate_traj_steps_per_s": n_agents * K_AGENT * HORIZON * N_ITER / dt}
    print(json.dumps(line), flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(json.dumps(dict(line, source_id=pkg.source_id(), device=torch.cuda.get_device_name(0))) + "\n")
    eng.close()
