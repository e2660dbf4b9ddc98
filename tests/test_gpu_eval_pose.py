"""The per-pose stage methods of a handle with moving obstacles (k_eval_pose) at the edges of their launch: one
kernel serves every form -- circles only, the mates' plans, obstacle tracks, a cost grid, the composed scene, the last two also
under the vehicle's outline -- and the two entry points that read the grid alone.  A pose's hit flag, its two costs and its
grid values are bit for bit the same whatever batch it is evaluated in: 257 poses at once (a full workgroup and one lane of the
next), and in batches of 1, 64 (one wave) and 65 (a wave and one lane; the last batch is ragged each time).  No tolerance and no
reference: what the numbers are is held to the f64 references in the files of the features themselves."""
import numpy as np
import pytest

import grid_footprint_checks as gf
import moving_obstacle_checks as mc
import scene_checks as sk
from test_gpu_scene import fleet_engine, load_fleet

pytestmark = pytest.mark.gpu

N = 257
BATCHES = (1, 64, 65)
CLOCK = 2
DIFF_T = 20
# form -> (the ingredients agent 0's handle holds, composed, the grid under the outline)
FORMS = {
    "circles": ((), False, False),
    "plans": (("plans",), False, False),
    "tracks": (("tracks",), False, False),
    "grid": (("grid",), False, False),
    "grid_foot": (("grid",), False, True),
    "scene": (sk.INGREDIENTS, True, False),
    "scene_foot": (sk.INGREDIENTS, True, True),
}


def scene_of(model, what):
    """-> (T, scene): scene_checks' three robots (T = 20: two circles, two tracks that run out inside the horizon, a 64 x 64
    grid) or its two cars (one track, a 64 x 64 grid, and two circles of car 0's own), with the ingredients `what` names"""
    if model == "diff":
        return DIFF_T, sk.fleet_scene(DIFF_T, False, what=what, clock=0, extra=-8)
    sc = sk.race_fleet_scene()
    x0 = sc["x0"][0]
    h, nrm = sk.heading(x0)
    car0 = dict(circles=np.array([[*(x0[:2] + 8.0 * h), 1.0], [*(x0[:2] + 14.0 * h + 3.0 * nrm), 1.5]]), vel=np.stack([np.zeros(2), -1.0 * h]))
    if "grid" in what:
        car0["grid"] = sc["per"][0]["grid"]
    if "tracks" in what:
        car0.update(tracks=sc["per"][0]["tracks"], radii=sc["per"][0]["radii"])
    return mc.RACE_T, dict(sc, per=[car0, dict()], plans="plans" in what)


def poses_of(model, sc, T, nx, rng):
    """N poses scattered around what agent 0 can hit -- its circles, its tracks now and mid-horizon, its mates, the wall beside its
    nominal rollout -- and around its own state, with steps from {0, 1, T / 2, T}"""
    ing, x0 = sc["per"][0], sc["x0"][0]
    h, nrm = sk.heading(x0)
    anchors = [x0[:2]] + [c[:2] for c in ing["circles"]] + [x[:2] for x in sc["x0"][1:]]
    if ing.get("tracks") is not None:
        L = ing["tracks"].shape[1]
        anchors += [t[min(j, L - 1)] for t in ing["tracks"] for j in (CLOCK, CLOCK + T // 2)]
    far, off = ((mc.TRAVEL + 0.3), 0.55) if model == "diff" else (11.5, 2.5)
    anchors += [x0[:2] + t * far * h - off * nrm for t in (0.2, 0.5, 0.8)]
    anchors = np.array(anchors)
    poses = np.zeros((N, nx))
    poses[:, :2] = anchors[rng.integers(0, len(anchors), N)] + rng.normal(0.0, 0.5 if model == "diff" else 2.5, (N, 2))
    poses[:, 2] = rng.uniform(-np.pi, np.pi, N)
    if nx == 4:
        poses[:, 3] = rng.uniform(0.0, 8.0, N)
    return poses, rng.choice(np.array([0, 1, T // 2, T], np.int32), N)


def outputs(e, poses, steps, grid):
    out = [e.eval_is_collided(poses, steps=steps), e.eval_is_collided(poses)]
    for terminal in (False, True):
        c, idx, _ = e.eval_cost(poses, prev_idx=0, terminal=terminal)
        out += [c, idx.astype(np.float64)]
    if grid:  # (the entry points that read the grid alone)
        g, pts = e.cost_grid_footprint_at(poses[:, :3], points=True)
        out += [e.cost_grid_at(poses[:, :2]), g, pts.reshape(len(poses), 18)]
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("model", ["diff", "race"])
def test_a_pose_is_priced_the_same_in_every_batch(model, form, precision):
    from dnn_mppi_mpc_amd import _capi as capi
    what, composed, foot = FORMS[form]
    T, sc = scene_of(model, what)
    box = dict(gf.DIFF_BOX, obstacle_model=capi.OBSTACLE_OUTLINE) if model == "diff" else {}  # (the outline mode needs the outline model)
    e = load_fleet(fleet_engine(sc, precision, T, model=model, **box), sc, composed=composed)
    if foot:
        e.set_cost_grid_footprint("outline")
    e.run_closed_loop(CLOCK)
    e.set_state(sc["x0"])
    e.set_u_prev(sc["u"])
    poses, steps = poses_of(model, sc, T, e.nx, np.random.default_rng(11))
    grid = "grid" in what
    whole = outputs(e, poses, steps, grid)
    hit = whole[0] > 0
    print(model, form, precision, e.rollout_kernel(), "hit", hit.mean(), "hit now", (whole[1] > 0).mean())
    assert hit.any() and not hit.all()  # (the poses stand on either side of something)
    for m in BATCHES:
        parts = [outputs(e, poses[k:k + m], steps[k:k + m], grid) for k in range(0, N, m)]
        for q, want in enumerate(whole):
            got = np.concatenate([p[q] for p in parts])
            assert np.array_equal(bits(got), bits(want)), (m, q, int((bits(got) != bits(want)).sum()))
