"""Obstacle tracks (mppi_set_obstacle_tracks): the f64 reference and the scenes of test_obstacle_track_cases.py (CPU)
and test_gpu_obstacle_tracks.py.  No device import.

The reference is the oracles of tests/moving_obstacle_checks.py with `_test` taking, per track, the centre
trk[m, min(clock + j, L - 1)] beside whatever circles the scene has: j is the step the `collided` call means (there), the clock
counts the control steps since the tracks were uploaded, and a track holds its last point once it runs out.  MARGIN,
MAX_LEFT_OUT and `kept` are that file's."""
import numpy as np

import moving_obstacle_checks as mc
from moving_obstacle_checks import MARGIN, MAX_LEFT_OUT, kept, penalised  # noqa: F401  (the tests take them from here)
from oracle.mppi_oracle import F32

VARIANTS = ("tracks", "velocity", "frozen")


def track_index(clock, j, L):
    """The point a state j steps ahead is tested against at `clock`: min(clock + j, L - 1)."""
    return np.minimum(int(clock) + np.asarray(j, dtype=np.int64), L - 1)


def track_centres(trk, clock, j, variant="tracks"):
    """Centres [..., n, 2] of the tracks trk [n, L, 2] at rollout step(s) j of `clock`.  "tracks": the definition.  "velocity":
    what a constant-velocity predictor makes of points clock, clock + 1 (the comparison of the CPU tests); "frozen": the tracks
    where they stand now, point `clock`."""
    trk = np.asarray(trk, np.float64)
    L = trk.shape[1]
    j = np.asarray(j, dtype=np.int64)
    if variant == "tracks":
        return np.moveaxis(trk[:, track_index(clock, j, L)], 0, -2)
    p0, p1 = trk[:, min(clock, L - 1)], trk[:, min(clock + 1, L - 1)]
    if variant == "frozen":
        return np.broadcast_to(p0, j.shape + p0.shape).copy()
    return p0 + (p1 - p0) * j[..., None, None].astype(np.float64)


class _Tracks:
    """What both oracles share: the tracks, their clock (apart from the circles'), and the test of a pose against both."""

    def set_tracks(self, trk, radii, clock=0, variant="tracks"):
        self.tracks = np.zeros((0, 1, 2)) if trk is None else np.asarray(trk, np.float64).reshape(len(np.atleast_1d(radii)), -1, 2)
        self.track_radii = np.asarray(radii, np.float64).reshape(-1)
        self.track_clock = int(clock)
        self.track_variant = variant
        self.margins = []

    def tick(self):
        self.clock += 1
        self.track_clock += 1

    def _test(self, px, py, r2, steps):
        hit = np.zeros(px.shape[:-1], bool)
        margin = np.full(px.shape[:-1], np.inf)
        if len(self.obstacle_circles):
            c = mc.centres(self.obstacle_circles, self.obstacle_vel, float(self.delta_t), self.clock, steps)
            d2 = (px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2
            hit |= (d2 < r2).any(axis=(-1, -2))
            margin = np.minimum(margin, (np.abs(d2 - r2) / r2).min(axis=(-1, -2)))
        if len(self.track_radii):
            t2 = self._track_r2()
            c = track_centres(self.tracks, self.track_clock, steps, self.track_variant)
            d2 = (px[..., :, None] - c[..., None, :, 0]) ** 2 + (py[..., :, None] - c[..., None, :, 1]) ** 2
            hit |= (d2 < t2).any(axis=(-1, -2))
            margin = np.minimum(margin, (np.abs(d2 - t2) / t2).min(axis=(-1, -2)))
        self.margins.append(margin.reshape(margin.shape[0], -1))
        return hit


class TrackDiffDriveOracle(_Tracks, mc.MovingDiffDriveOracle):
    def __init__(self, *a, tracks=None, track_radii=(), **kw):
        super().__init__(*a, **kw)
        self.set_tracks(tracks, track_radii)

    def _track_r2(self):  # (as a circle of that radius: _obs.py:304-311)
        return (0.5 * self.safety_margin_rate + self.track_radii) ** 2


class TrackRaceCarOracle(_Tracks, mc.MovingRaceCarOracle):
    def __init__(self, *a, tracks=None, track_radii=(), **kw):
        super().__init__(*a, **kw)
        self.set_tracks(tracks, track_radii)

    def _track_r2(self):
        return self.track_radii ** 2


# ------------------------------------------------------------------------------------------ scenes
CLOCK = 3  # the cases run three control steps after the upload: point i of a track is the obstacle at rollout step i - CLOCK
NO_CIRCLES = np.zeros((0, 3))


def bend(E, h, nrm, arc, s_meet, s, after):
    """A quarter circle of length `arc` that ends at E, heading -h, at step s_meet; it starts heading -nrm.  s: steps [L]
    (before 0 the circle simply goes on backwards).  after: "hold" -- it stops at E; "straight" -- it goes on along -h."""
    rq = 2.0 * arc / np.pi
    C = E + rq * nrm
    s = np.asarray(s, np.float64)
    th = 0.5 * np.pi * (1.0 - np.minimum(s, s_meet) / s_meet)
    p = C + rq * (-np.cos(th)[:, None] * nrm + np.sin(th)[:, None] * h)
    if after == "straight":
        p = p - h * (arc / s_meet) * np.maximum(s - s_meet, 0.0)[:, None]
    return p


def diff_scene(T, accumulate, clock=CLOCK, extra=0, turner_after="hold"):
    """moving_obstacle_checks.diff_scene's geometry with tracks in the circles' place (all radii 0.4, threshold radius 0.8):
      turner  -- arrives beside the path on a quarter circle of radius 2 SWEEP meet / pi (as long as the crosser's way), ending
                 0.8 m to the left of the meeting point at the meeting step, where it stops; it starts out heading for the path.
      stopper -- walks towards the path from 0.9 + 0.75 SWEEP to its right, halts 0.9 m beside it at 0.6 of the meeting step
                 and stays: it catches the samples that stray 0.1 m that way.
      static  -- a track that does not move, 0.95 m to the left at half the way.
    Point i of a track is the obstacle at rollout step i - clock; L = clock + T + 1 + extra.  turner_after = "straight": the
    turner goes on down the path behind the bend instead (the closed loop: a turner that stops is met whenever it arrived).
    Returns dict(ref, x0, u, circles [0, 3], vel [0, 2], tracks [3, L, 2], radii [3])."""
    sc = mc.diff_scene(T, accumulate)
    x0 = sc["x0"]
    h = np.array([np.cos(x0[2]), np.sin(x0[2])])
    nrm = np.array([-h[1], h[0]])
    meet = round(0.5 * T) / T if accumulate else 1.0
    M = x0[:2] + meet * mc.TRAVEL * h
    s_meet = meet * T
    L = clock + T + 1 + extra
    s = np.arange(L) - clock
    turner = bend(M + 0.8 * nrm, h, nrm, mc.SWEEP * meet, s_meet, s, turner_after)
    A, B = M - (0.9 + 0.75 * mc.SWEEP) * nrm, M - 0.9 * nrm
    stopper = A + (B - A) * np.minimum(s / (0.6 * s_meet), 1.0)[:, None]
    static = np.broadcast_to(x0[:2] + 0.5 * meet * mc.TRAVEL * h + 0.95 * nrm, (L, 2))
    return dict(sc, circles=NO_CIRCLES, vel=np.zeros((0, 2)), tracks=np.stack([turner, stopper, static]), radii=np.full(3, 0.4))


def diff_oracle(sc, K, T, **kw):
    o = TrackDiffDriveOracle(ref_path=sc["ref"], num_samples_K=K, num_horizons_T=T, obstacle_circles=sc["circles"],
                             obstacle_velocities=sc["vel"], tracks=sc["tracks"], track_radii=sc["radii"], **dict(mc.DIFF_KW, **kw))
    o.u_prev[:] = sc["u"]
    return o


def race_scene(clock=CLOCK, extra=0):
    """moving_obstacle_checks.race_scene with its two movers as tracks: the crosser on a bend -- a quarter circle as long as
    its straight way to the meeting point, then on down the road --, the leaver sampled from its velocity; the static circle
    stays the handle's own (zero velocity): circles and tracks priced side by side."""
    sc = mc.race_scene()
    s0 = sc["x0"]
    h = np.array([np.cos(s0[2]), np.sin(s0[2])])
    nrm = np.array([-h[1], h[0]])
    T = mc.RACE_T
    L = clock + T + 1 + extra
    s = np.arange(L) - clock
    crosser = bend(s0[:2] + 5.0 * h + 3.7 * nrm, h, nrm, 12.0, 0.5 * T, s, "straight")
    leaver = sc["circles"][1, :2] + sc["vel"][1] * (0.05 * s)[:, None]
    return dict(sc, circles=sc["circles"][2:], vel=sc["vel"][2:], tracks=np.stack([crosser, leaver]), radii=np.full(2, 1.0))


def race_oracle(sc, K):
    o = TrackRaceCarOracle(ref_path=sc["ref"], number_of_samples_K=K, obstacle_circles=sc["circles"], obstacle_velocities=sc["vel"],
                           tracks=sc["tracks"], track_radii=sc["radii"], **mc.RACE_KW)
    o.u_prev[:] = sc["u"].astype(F32)
    return o


def far_tracks(n, L):
    """n tracks nothing comes near: they drift slowly a kilometre away (padding for the sets of the LDS limit)."""
    i = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(L, dtype=np.float64)[None, :]
    return np.stack([1.0e3 + 3.0 * i + 0.01 * j, 1.0e3 - 0.02 * j + 0.0 * i], axis=-1)


def sample_velocity(circles, vel, dt, L):
    """Tracks [m, L, 2] sampled from c + v dt i, in the arithmetic of moving_obstacle_checks.centres."""
    return np.moveaxis(mc.centres(circles, vel, dt, 0, np.arange(L)), 0, 1).copy()


# ------------------------------------------------------------------------------------------ cases
K_CASE = mc.K_CASE
HORIZONS = (7, 50, 64, 65, 100, 128)  # one chunk, the chunk seam, a full second chunk (T > 128: refused)


def diff_cases():
    """(T, accumulate, mode): every horizon with the frozen index, both sums; the threaded indices at T = 50 and 65"""
    out = [(T, acc, "frozen") for T in HORIZONS for acc in (False, True)]
    out += [(T, False, mode) for T in (50, 65) for mode in ("per_rollout", "sequential")]
    return out


# noise seeds: for each case the first seed at which the f64 reference itself leaves out at most MAX_LEFT_OUT of the samples
# (test_obstacle_track_cases.py asserts it); cases not listed take seed 0
EPS_SEED = {(65, True, "frozen"): 1, (100, True, "frozen"): 1, (128, True, "frozen"): 2}


def eps_seed(T, accumulate, mode):
    return EPS_SEED.get((T, accumulate, mode), 0)


def diff_case(T, accumulate, mode, K=K_CASE, clock=CLOCK, variant="tracks"):
    """-> (scene, eps [K, T, 2] float32, oracle after one iteration at `clock`, its result)"""
    from oracle import philox
    sc = diff_scene(T, accumulate, clock)
    eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], eps_seed(T, accumulate, mode), 0, K, T)
    o = diff_oracle(sc, K, T)
    o.set_tracks(sc["tracks"], sc["radii"], clock, variant)
    res = o.iteration_general(sc["x0"], eps.astype(np.float64), mode, accumulate)
    return sc, eps, o, res


def race_case(K=K_CASE, clock=CLOCK, variant="tracks", seed=0):
    from oracle import philox
    sc = race_scene(clock)
    eps = philox.sample_epsilon(np.array([[0.5, 0.0], [0.0, 0.1]]), seed, 0, K, mc.RACE_T)
    o = race_oracle(sc, K)
    o.set_motion(sc["vel"], clock)
    o.set_tracks(sc["tracks"], sc["radii"], clock, variant)
    res = o.iteration(sc["x0"], eps)
    return sc, eps, o, res


LOOP_ACCUMULATE = True  # (every step priced: `S[k] =` sees step T alone, where turner and stopper have arrived whatever the clock)


def loop_scene(T, extra=2, own=True):
    """The closed-loop scene: the tracks uploaded at iteration 0 (clock 0, L = T + 1 + extra: a run of more than `extra`
    iterations goes past the end of the tracks, so the hold is priced), the turner passing on, beside two moving circles of
    the handle's own: moving_obstacle_checks.diff_scene's leaver and static circle 1.2 m further down the path, where they
    decide samples the tracks do not (the crosser and the static circle themselves stand where turner and stopper end up)."""
    sc = diff_scene(T, LOOP_ACCUMULATE, clock=0, extra=extra, turner_after="straight")
    if not own:
        return sc
    base = mc.diff_scene(T, LOOP_ACCUMULATE)
    along = 1.2 * np.array([np.cos(base["x0"][2]), np.sin(base["x0"][2]), 0.0])
    return dict(sc, circles=base["circles"][[1, 2]] + along, vel=base["vel"][[1, 2]])


def diff_closed_loop(T, n_iters, own=True, K=K_CASE, seed=31, eps_of=None, extra=2, tick=True):
    """moving_obstacle_checks.diff_closed_loop on loop_scene: one iteration, the plant step with the returned u0, one tick of
    both clocks -- n_iters times."""
    from oracle import philox
    sc = loop_scene(T, extra, own)
    o = diff_oracle(sc, K, T, **mc.LOOP_KW)
    x = sc["x0"].copy()
    u0, hits, keep, xs, us, counted = [], [], [], [], [], []
    for i in range(n_iters):
        o.reset_margins()
        xs.append(x.copy())
        us.append(o.u_prev.copy())
        eps = philox.sample_epsilon(mc.DIFF_KW["sigma"], seed, i, K, T) if eps_of is None else eps_of(i)
        res = o.iteration_general(x, eps.astype(np.float64), "frozen", LOOP_ACCUMULATE)
        u0.append(res["u0_returned"].copy())
        hits.append(int(penalised(res["S"]).sum()))
        counted.append(int((res["S"] >= 1.0e10).sum()))
        keep.append(float((o.sample_margin() > MARGIN).mean()))
        x = mc.mppi_oracle.diffdrive_plant_step(x, res["u0_returned"], mc.DIFF_KW["delta_t"])
        if tick:
            o.tick()
    # (x_at / u_at: state and nominal controls every iteration started from, for a handle that is re-seeded per iteration;
    # n_counted: mppi_stats.n_collided by the kernels' definition, S >= collision_penalty -- under the loop's light weights a
    # penalised sample's other terms can sum below zero, and it is then not counted)
    return dict(scene=sc, u0=np.array(u0), x=x, idx=o.prev_way_point_idx, n_hit=hits, kept=keep, oracle=o, x_at=xs, u_at=us, n_counted=counted)
