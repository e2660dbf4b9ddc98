// Device helpers shared by the analytic (mppi_kernels.hip) and learned-dynamics (mppi_mlp.hip) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "mathfn.h"
#include "mppi_kernels.h"
#include "philox.h"
#include "wave_ops.h"

namespace mppi {

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------

template <typename R> __device__ __forceinline__ R dist2(const R *__restrict__ ref, int i, R x, R y) {
    const R dx = x - ref[4 * i], dy = y - ref[4 * i + 1];
    return dx * dx + dy * dy;
}

// first-minimum argmin over ref[c .. c+wlen) for this lane's (x, y); c, wlen wave-uniform
// (`get_nearest_waypoint` mppi_race_car.py:157-174, `_get_nearest_waypoint` mppi_differential_drive.py:201-220)
template <typename R>
__device__ __forceinline__ int nearest_in_window(const R *__restrict__ ref, int c, int wlen, R x, R y) {
    R best = dist2(ref, c, x, y);
    int bj = 0;
#pragma unroll 4
    for (int j = 1; j < wlen; ++j) {
        const R d = dist2(ref, c + j, x, y);
        if (d < best) { best = d; bj = j; }
    }
    return c + bj;
}

// ---- the same search with the window staged in LDS ------------------------------------------------------
// The frozen-index modes search the SAME window ref[c .. c+wlen) for every step of every sample of a
// workgroup (mppi_race_car.py:157-174: up to 200 candidates per call), so the window is copied to LDS once per
// workgroup as pairs {x_2q, x_2q+1, y_2q, y_2q+1}: one broadcast 16/32-byte LDS read serves two candidates and the
// distance arithmetic packs (v_pk_add / v_pk_mul / v_pk_fma), instead of a scalar load + address arithmetic
// per candidate.  An odd window is padded with a far-away point that can never win.
constexpr int WINDOW_LDS_MAX = 256;  // candidates

template <typename R> struct alignas(16) RefPair { R x0, x1, y0, y1; };
template <typename R> struct alignas(4 * sizeof(R)) VecT4 { R x, y, z, w; };  // four values, one aligned load / store

template <typename R>
__device__ __forceinline__ void stage_window(RefPair<R> *sh, const R *__restrict__ ref, int c, int wlen, int tid,
                                             int nthreads) {
    const int npairs = (wlen + 1) >> 1;
    for (int q = tid; q < npairs; q += nthreads) {
        const int j0 = c + 2 * q, j1 = j0 + 1;
        RefPair<R> r;
        r.x0 = ref[4 * j0];
        r.y0 = ref[4 * j0 + 1];
        const bool has1 = 2 * q + 1 < wlen;
        r.x1 = has1 ? ref[4 * j1] : R(1e30);
        r.y1 = has1 ? ref[4 * j1 + 1] : R(1e30);
        sh[q] = r;
    }
}

template <typename R>
__device__ __forceinline__ int nearest_in_window_lds(const RefPair<R> *sh, int c, int wlen, R x, R y) {
    const int npairs = (wlen + 1) >> 1;
    R best = R(INFINITY);
    int bj = 0;
#pragma unroll 4
    for (int q = 0; q < npairs; ++q) {
        const RefPair<R> r = sh[q];
        const R dx0 = x - r.x0, dx1 = x - r.x1, dy0 = y - r.y0, dy1 = y - r.y1;
        const R d0 = dx0 * dx0 + dy0 * dy0, d1 = dx1 * dx1 + dy1 * dy1;
        if (d0 < best) { best = d0; bj = 2 * q; }
        if (d1 < best) { best = d1; bj = 2 * q + 1; }
    }
    return c + bj;
}

// Few active steps in this chunk (the tail of a horizon that is not a multiple of 64): `split` lanes share
// one step's candidates (interleaved pairs), then combine with first-minimum semantics.  `split` is a power of
// two <= 16 and n_act * split <= 64.  Returns, on lane t (< n_act), the index for step t.
template <typename R>
__device__ __forceinline__ int nearest_in_window_split(const RefPair<R> *sh, int c, int wlen, R x, R y, int split,
                                                       int lane) {
    const int lg = 31 - __clz(split);
    const int src = lane >> lg, part = lane & (split - 1);
    const R xs = __shfl(x, src), ys = __shfl(y, src);
    const int npairs = (wlen + 1) >> 1;
    R best = R(INFINITY);
    int bj = 0x7fffffff;
    for (int q = part; q < npairs; q += split) {
        const RefPair<R> r = sh[q];
        const R dx0 = xs - r.x0, dx1 = xs - r.x1, dy0 = ys - r.y0, dy1 = ys - r.y1;
        const R d0 = dx0 * dx0 + dy0 * dy0, d1 = dx1 * dx1 + dy1 * dy1;
        if (d0 < best) { best = d0; bj = 2 * q; }
        if (d1 < best) { best = d1; bj = 2 * q + 1; }
    }
    for (int m = 1; m < split; m <<= 1) {  // (smallest d, then smallest j) over the `split` lanes of a step
        const R od = __shfl_xor(best, m);
        const int oj = __shfl_xor(bj, m);
        if (od < best || (od == best && oj < bj)) { best = od; bj = oj; }
    }
    const int j = __shfl(bj, lane << lg);  // lane t reads the result of its group's first lane
    return c + (j == 0x7fffffff ? 0 : j);  // (nothing compared smaller -- a NaN or overflowing position: the first candidate)
}

// Same search for ONE wave-uniform position with the candidates spread over the lanes.  (A position no candidate compares
// smaller for -- NaN, infinite, or so far that d overflows -- gives c like the serial searches above: wv::argmin_first.)
template <typename R>
__device__ __forceinline__ int nearest_uniform(const R *__restrict__ ref, int c, int wlen, R x, R y, int lane) {
    R best = R(INFINITY);
    int bj = INT_MAX;
    for (int j = lane; j < wlen; j += 64) {
        const R d = dist2(ref, c + j, x, y);
        if (d < best) { best = d; bj = j; }
    }
    wv::argmin_first(best, bj);
    return c + bj;
}

// The x0 call's search (mppi_differential_drive.py:96-99, mppi_race_car.py:61-65): nearest_uniform in f64 whatever the
// handle's precision, so that the closed loop on the device and the same loop stepped from the host take the same index
// at a near tie.
template <typename R>
__device__ __forceinline__ int nearest_x0(const R *__restrict__ ref, int p, int wlen, double x, double y, int lane) {
    double best = INFINITY;
    int bj = INT_MAX;
    for (int j = lane; j < wlen; j += 64) {
        const double dx = x - (double)ref[4 * (p + j)], dy = y - (double)ref[4 * (p + j) + 1];
        const double d = dx * dx + dy * dy;
        if (d < best) { best = d; bj = j; }
    }
    wv::argmin_first(best, bj);
    return p + bj;
}

// the noise tensor [K][T][2] of (iteration, agent): the caller's tensor of this call, or the slot of a noise ring
// (mppi_set_noise_ring: `_calc_epsilon` materialised for a closed loop; eps_slots is a power of two)
template <typename R> __device__ __forceinline__ const float *eps_tensor(const KParams<R> &P, unsigned iter, int agent) {
    size_t tensor = (size_t)agent;
    if (P.eps_slots > 0) tensor += (size_t)(iter & (unsigned)(P.eps_slots - 1)) * (size_t)(P.n_agents > 1 ? P.n_agents : 1);
    return P.eps + tensor * ((size_t)P.K * (size_t)P.T * 2);
}

template <typename R> __device__ __forceinline__ int window_len(int window, int n_ref, int c) {
    const int rem = n_ref - c;
    return rem < window ? rem : window;
}

// collision indicator of one state (mppi_differential_drive_obs.py:301-313,
// mppi_race_car_obstacle.py:241-274)
// The obstacle table lives in registers: lane m holds circle m {centre, squared radius} (one vector load issued at
// the top of the kernel, with all lanes active).  The loops below read one circle per iteration with v_readlane, so
// there is no memory wait inside them; a table walked through a pointer costs a load round trip per circle -- and
// the race car repeats the walk for each of its 8 outline points (config 4: 32 us per launch, 3/4 of it such waits).
// Circles beyond the 64th come from P.obs directly.
template <typename R> struct ObsLanes { R x, y, r2; };

template <typename R> __device__ __forceinline__ ObsLanes<R> load_obstacles(const KParams<R> &P, int lane) {
    ObsLanes<R> o{R(0), R(0), R(0)};
    if (P.obstacle_model != OBS_NONE && lane < P.n_obs) {
        const R *q = P.obs + 4 * lane;
        o.x = q[0]; o.y = q[1]; o.r2 = q[2];
    }
    return o;
}

// Moving obstacles (mppi_config.obstacle_motion, KParams::obs_motion): the table's twin with circle m's velocity on lane m as
// well.  The velocity rows {vx, vy, 0, 0} stand behind the n_obs circle rows of the same buffer.
template <typename R> struct ObsLanesMoving { R x, y, r2, vx, vy; };

template <typename R> __device__ __forceinline__ ObsLanesMoving<R> load_obstacles_moving(const KParams<R> &P, int lane) {
    ObsLanesMoving<R> o{R(0), R(0), R(0), R(0), R(0)};
    if (P.obstacle_model != OBS_NONE && lane < P.n_obs) {
        const R *q = P.obs + 4 * lane, *w = P.obs + 4 * (P.n_obs + lane);
        o.x = q[0]; o.y = q[1]; o.r2 = q[2];
        o.vx = w[0]; o.vy = w[1];
    }
    return o;
}
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
// The obstacle clock: control steps since the set was uploaded (n = DevState::iter - iter0) plus the j rollout steps ahead a
// state lies, as the time tau = dt (n + j) in the handle's precision -- the integer converted exactly, one product.  A circle's
// centre at that state is then one fma per coordinate: c + v tau (zero velocities give c back exactly).
__device__ __forceinline__ int obstacle_clock(long long iter, long long iter0) { return (int)(iter - iter0); }
template <typename R> __device__ __forceinline__ R obstacle_time(const KParams<R> &P, int n_plus_j) { return P.dt * (R)n_plus_j; }

// WIDE: the 8 outline points stay in registers and each circle is read once (the race-car kernels); otherwise the
// points are visited one after the other, which keeps the diff-drive kernels at their register count
// (`have_sc`: the caller already holds sin/cos of this yaw)
// MOVING: `tab` carries velocities and every centre is taken at this lane's time `tau` (obstacle_time); false compiles to the
// static test.
template <bool WIDE, bool MOVING = false, typename R, typename TAB>
__device__ __forceinline__ bool collided(const KParams<R> &P, R x, R y, R yaw, const TAB &tab, bool have_sc = false,
                                         R sn_in = R(0), R cs_in = R(1), R tau = R(0)) {
    if (P.obstacle_model == OBS_NONE) return false;
    bool hit = false;
    const int n_reg = P.n_obs < 64 ? P.n_obs : 64;
    // circle m's centre: from lane m of the table (m < 64) or from its rows in memory
    auto lane_x = [&](int m) { R c = wv::read_lane(tab.x, m); if constexpr (MOVING) c = fma_(wv::read_lane(tab.vx, m), tau, c); return c; };
    auto lane_y = [&](int m) { R c = wv::read_lane(tab.y, m); if constexpr (MOVING) c = fma_(wv::read_lane(tab.vy, m), tau, c); return c; };
    auto mem_x = [&](int m) { R c = P.obs[4 * m]; if constexpr (MOVING) c = fma_(P.obs[4 * (P.n_obs + m)], tau, c); return c; };
    auto mem_y = [&](int m) { R c = P.obs[4 * m + 1]; if constexpr (MOVING) c = fma_(P.obs[4 * (P.n_obs + m) + 1], tau, c); return c; };
    if (P.obstacle_model == OBS_CIRCLE) {
        for (int m = 0; m < n_reg; ++m) {
            const R dx = x - lane_x(m), dy = y - lane_y(m);
            hit |= dx * dx + dy * dy < wv::read_lane(tab.r2, m);
        }
        for (int m = 64; m < P.n_obs; ++m) {
            const R dx = x - mem_x(m), dy = y - mem_y(m);
            hit |= dx * dx + dy * dy < P.obs[4 * m + 2];
        }
        return hit;
    }
    // OBS_OUTLINE; the reference's 9th point repeats the 1st (mppi_race_car_obstacle.py:263-264)
    R sn = sn_in, cs = cs_in;
    if (!have_sc) mf::sincos_(yaw, sn, cs);
    if (WIDE) {
        // The outline is the reference's fixed pattern -- (+-a, 0), (+-a, +-b), (0, +-b) in the body frame, a and b half the
        // scaled length and width (:260-261) -- and closed under mirroring in both axes.  So instead of rotating eight
        // points into the world, each circle's centre is rotated into the body frame and folded into the first quadrant,
        // where the nearest outline point is one of (a, 0), (a, b), (0, b): 16 instructions per circle instead of 32 per
        // pose + 43 per circle (14 % of the race-car launch with its two circles).  Same squared distances up to f32
        // rounding of the rotation.
        const R a = P.shape_x[3], b = P.shape_y[3];
        auto circle = [&](R ox, R oy, R r2) {
            const R dx = ox - x, dy = oy - y;
            const R bx = fabs(dx * cs + dy * sn), by = fabs(dy * cs - dx * sn);
            const R ex = bx - a, ey = by - b;
            const R ex2 = ex * ex, ey2 = ey * ey;
            hit |= fmin(fmin(ex2 + by * by, ex2 + ey2), bx * bx + ey2) < r2;
        };
        for (int m = 0; m < n_reg; ++m) circle(lane_x(m), lane_y(m), wv::read_lane(tab.r2, m));
        for (int m = 64; m < P.n_obs; ++m) circle(mem_x(m), mem_y(m), P.obs[4 * m + 2]);
    } else {
        for (int q = 0; q < 8; ++q) {
            const R px = P.shape_x[q] * cs - P.shape_y[q] * sn + x;
            const R py = P.shape_x[q] * sn + P.shape_y[q] * cs + y;
            for (int m = 0; m < n_reg; ++m) {
                const R dx = px - lane_x(m), dy = py - lane_y(m);
                hit |= dx * dx + dy * dy < wv::read_lane(tab.r2, m);
            }
            for (int m = 64; m < P.n_obs; ++m) {
                const R dx = px - mem_x(m), dy = py - mem_y(m);
                hit |= dx * dx + dy * dy < P.obs[4 * m + 2];
            }
        }
    }
    return hit;
}

// Fleet plans (MPPI_FLEET_PLAN): the mates of agent `self` at point j of their plans (j in [0, P.T]: the caller's business)
// against this lane's state.  The centres differ per lane -- lane l of a rollout owns its own step -- so they cannot come out
// of a lane table by v_readlane: every lane reads point j of mate a, one 8-byte (f32) element, consecutive lanes consecutive
// addresses -- from `table`, the handle's table in memory or the workgroup's copy of it in LDS (conflict-free `ds_read_b64`; the
// caller makes one call per address space, so that each compiles to its own load).  OBS_CIRCLE: the circle test of collided(); OBS_OUTLINE: its folded outline form, for both models.  A function of
// its own beside collided(), whose text and callers stay as they are.
template <typename R>
__device__ __forceinline__ bool mates_collided(const KParams<R> &P, const PlanPoint<R> *table, R x, R y, R yaw, int self, int j) {
    const PlanPoint<R> *pt = table + j;
    const R thr2 = fleet_plan_thr2(P);
    const size_t stride = (size_t)P.T + 1;
    bool hit = false;
    if (P.obstacle_model == OBS_CIRCLE) {
        for (int a = 0; a < P.n_agents; ++a) {
            if (a == self) continue;
            const PlanPoint<R> c = pt[a * stride];
            const R dx = x - c.x, dy = y - c.y;
            hit |= dx * dx + dy * dy < thr2;
        }
        return hit;
    }
    R sn, cs;
    mf::sincos_(yaw, sn, cs);
    const R ha = P.shape_x[3], hb = P.shape_y[3];
    for (int a = 0; a < P.n_agents; ++a) {
        if (a == self) continue;
        const PlanPoint<R> c = pt[a * stride];
        const R dx = c.x - x, dy = c.y - y;
        const R bx = fabs(dx * cs + dy * sn), by = fabs(dy * cs - dx * sn);
        const R ex = bx - ha, ey = by - hb;
        const R ex2 = ex * ex, ey2 = ey * ey;
        hit |= fmin(fmin(ex2 + by * by, ex2 + ey2), bx * bx + ey2) < thr2;
    }
    return hit;
}

// Obstacle tracks (mppi_set_obstacle_tracks): this lane's state against the point of every track that its step owns.  `pt` is
// that point of track 0 -- the caller has folded step and clock into it -- and track m's stands `stride` points behind: T + 1
// in the workgroup's staged window (LDS, one conflict-free `ds_read_b64` per f32 test, consecutive lanes consecutive
// addresses), L in the table in memory; `thr2[m]` is track m's own squared threshold (a wave-uniform read).  The caller makes
// one call per address space, so that each compiles to its own load.  OBS_CIRCLE: the circle test of collided(); OBS_OUTLINE:
// its folded outline form, for both models, as mates_collided has it.  No self to skip.  A function of its own beside
// collided() and mates_collided(), whose text and callers stay as they are.
template <typename R>
__device__ __forceinline__ bool tracks_collided(const KParams<R> &P, const PlanPoint<R> *pt, const R *thr2, int n, int stride,
                                                R x, R y, R yaw) {
    bool hit = false;
    if (P.obstacle_model == OBS_CIRCLE) {
        for (int m = 0; m < n; ++m) {
            const PlanPoint<R> c = pt[(size_t)m * stride];
            const R dx = x - c.x, dy = y - c.y;
            hit |= dx * dx + dy * dy < thr2[m];
        }
        return hit;
    }
    R sn, cs;
    mf::sincos_(yaw, sn, cs);
    const R ha = P.shape_x[3], hb = P.shape_y[3];
    for (int m = 0; m < n; ++m) {
        const PlanPoint<R> c = pt[(size_t)m * stride];
        const R dx = c.x - x, dy = c.y - y;
        const R bx = fabs(dx * cs + dy * sn), by = fabs(dy * cs - dx * sn);
        const R ex = bx - ha, ey = by - hb;
        const R ex2 = ex * ex, ey2 = ey * ey;
        hit |= fmin(fmin(ex2 + by * by, ex2 + ey2), bx * bx + ey2) < thr2[m];
    }
    return hit;
}

// Cost grids (mppi_set_cost_grid): the bilinear value of grid G at this lane's position, in R.  The positions differ per lane,
// so every lane gathers its own cell: the two nodes of row iy and the two of row iy + 1, all four reads issued before the
// first use, so that the lane waits once.  A row pair starts at any node, so it is aligned to one element only: two loads
// of one element each per row (DESIGN 3.12 says what the compiler makes of them).  grid_index keeps every read inside the
// table whatever the state is.  A function of its own beside collided(), mates_collided() and tracks_collided().
template <typename R> __device__ __forceinline__ R grid_value(const GridSet<R> &G, R x, R y) {
    R fx, fy;
    const int ix = grid_index(x, G.ox, G.inv, G.nx, fx), iy = grid_index(y, G.oy, G.inv, G.ny, fy);
    const R *r0 = G.cells + (size_t)iy * G.nx + ix, *r1 = r0 + G.nx;
    const R a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
    const R c0 = fma_(fx, a1 - a0, a0), c1 = fma_(fx, b1 - b0, b0);
    return fma_(fy, c1 - c0, c0);
}

// Cost grids under the vehicle's outline (mppi_set_cost_grid_footprint: MPPI_GRID_FOOTPRINT_OUTLINE).  Point q = 1 .. 8 of the
// outline -- (P.shape_x, P.shape_y)[q - 1], the points collided() tests -- of a pose in the world, sn / cs = mf::sincos_ of its
// yaw: two fmas per coordinate, the offset folded into the first (the order include/mppi_hip.h documents).  Point 0 is the
// pose's own (x, y), untouched.  The outline is (+-a, 0), (+-a, +-b), (0, +-b) with a = shape_x[3], b = shape_y[3]: the signs
// come out of two packed words (two bits per point, sign + 1), the products with them are exact -- so that a loop over q
// indexes nothing (an index into the kernel's own copy of its argument would put that copy into scratch).
constexpr unsigned OUTLINE_SIGNS_X = 0x1A90u, OUTLINE_SIGNS_Y = 0x01A9u;  // -a -a 0 a a a 0 -a  /  0 b b b 0 -b -b -b
template <typename R>
__device__ __forceinline__ void outline_point(const KParams<R> &P, unsigned wx, unsigned wy, R x, R y, R sn, R cs, R &px, R &py) {
    const R qx = (R)((int)(wx & 3u) - 1) * P.shape_x[3];  // (wx, wy: the words shifted down to this point)
    const R qy = (R)((int)(wy & 3u) - 1) * P.shape_y[3];
    px = fma_(qx, cs, fma_(-qy, sn, x));
    py = fma_(qx, sn, fma_(qy, cs, y));
}
// g_foot = fmax over the nine points of grid_value: the centre first, then the outline in order, each point a grid_value of its
// own -- its four reads issued before its first use -- folded into a running fmax (the plain form; DESIGN 3.14 says what was
// tried beside it).  The loop stays a loop: unrolled, the scheduler keeps the reads of all nine points in flight and the f64
// and composed forms spill.  One sincos per state.  grid_index keeps every read inside the table whatever the pose is: a NaN or
// infinite yaw makes the outline's points NaN, which land on node 0 of each axis.  `pts` (the eval kernels' window, else null)
// receives the nine world points [9][2].
template <typename R>
__device__ __forceinline__ R grid_value_outline(const GridSet<R> &G, const KParams<R> &P, R x, R y, R yaw, R *pts = nullptr) {
    R sn, cs;
    mf::sincos_(yaw, sn, cs);
    R g = grid_value(G, x, y);
    if (pts) { pts[0] = x; pts[1] = y; }
#pragma unroll 1
    for (unsigned wx = OUTLINE_SIGNS_X | 0x10000u, wy = OUTLINE_SIGNS_Y; wx != 1u; wx >>= 2, wy >>= 2) {  // (bit 16: the end mark)
        R px, py;
        outline_point(P, wx, wy, x, y, sn, cs, px, py);
        if (pts) { pts += 2; pts[0] = px; pts[1] = py; }
        g = fmax(g, grid_value(G, px, py));
    }
    return g;
}

// weighted squared tracking error against waypoint i (`_compute_cost` :222-236, `_c` mppi_race_car.py:137-146)
template <typename R, int MODEL>
__device__ __forceinline__ R tracking_cost_row(const KParams<R> &P, const R (&w)[4], bool wrap, const R *r, R x, R y, R yaw,
                                               R vel) {  // r: the waypoint's row {x, y, yaw, v}
    if (wrap) yaw = mf::pymod(yaw + P.two_pi, P.two_pi);
    const R ex = x - r[0], ey = y - r[1], eyaw = yaw - r[2];
    R c = w[0] * (ex * ex) + w[1] * (ey * ey) + w[2] * (eyaw * eyaw);
    if (MODEL == MODEL_RACE) {
        const R ev = vel - r[3];
        c += w[3] * (ev * ev);
    }
    return c;
}
template <typename R, int MODEL>
__device__ __forceinline__ R tracking_cost(const KParams<R> &P, const R (&w)[4], bool wrap, int i, R x, R y, R yaw,
                                           R vel) {
    return tracking_cost_row<R, MODEL>(P, w, wrap, P.ref + 4 * i, x, y, yaw, vel);
}

// ------------------------------------------------------------------------------------------
// The per-step formulas of the reference, one definition each, for every rollout layout to call ("Per-step
// formulas", lists the callers and the sites that keep their own text).  Which lane owns which step, what is masked beyond
// the horizon and what stays in registers is the kernels' business.
// ------------------------------------------------------------------------------------------
// noise of sample k at step t (`_calc_epsilon` mppi_differential_drive.py:273-283): drawn (philox.h; k_offset: the shard's
// first sample, noise_stream + agent: the counter's fourth word) or read from the tensor of (iter, agent).  The caller
// keeps t inside the horizon.  `philox`: P.use_philox, or the constant true of a PLAIN instantiation.
template <typename R>
__device__ __forceinline__ void noise_at(const KParams<R> &P, bool philox, unsigned iter, int agent, int k, int t, float &e0, float &e1) {
    if (philox) {
        px::sample(P.seed_lo, P.seed_hi, iter, (unsigned)(k + P.k_offset), t, P.chol, e0, e1, (unsigned)(P.noise_stream + agent));
    } else {
        const float2 e = *reinterpret_cast<const float2 *>(eps_tensor(P, iter, agent) + ((size_t)k * P.T + t) * 2);
        e0 = e.x; e1 = e.y;
    }
}
// the same for a lane that owns steps 2l and 2l+1: ONE Philox block feeds both (words r0,r1 -> step 2l, r2,r3 -> step
// 2l+1: the sampler's layout), or two 8-byte loads.  Step 2l lies inside the horizon (the caller's condition); `a1`: so does
// step 2l+1 -- otherwise its noise comes back 0.
template <typename R>
__device__ __forceinline__ void noise_pair(const KParams<R> &P, bool philox, unsigned iter, int agent, int k, int l, bool a1,
                                           float &e00, float &e01, float &e10, float &e11) {
    e10 = 0.f; e11 = 0.f;
    if (philox) {
        unsigned r[4];
        px::philox4x32_10((unsigned)(k + P.k_offset), (unsigned)l, iter, (unsigned)(P.noise_stream + agent), P.seed_lo, P.seed_hi, r);
        px::box_muller(r[0], r[1], P.chol, e00, e01);
        px::box_muller(r[2], r[3], P.chol, e10, e11);
        if (!a1) { e10 = 0.f; e11 = 0.f; }
    } else {
        const float *pe = eps_tensor(P, iter, agent) + ((size_t)k * P.T + 2 * l) * 2;
        const float2 ea = *reinterpret_cast<const float2 *>(pe);
        e00 = ea.x; e01 = ea.y;
        if (a1) {
            const float2 eb = *reinterpret_cast<const float2 *>(pe + 2);
            e10 = eb.x; e11 = eb.y;
        }
    }
}

// perturb (the first (1 - exploration) K samples explore around u, the rest around 0: :116-119) and clamp (`_g` :285-289;
// the visualisation rollouts always clamp, :148,:158)
// (the two halves apart for the learned model's visualisation rows, which clamp the nominal row in the same statement)
template <typename R> __device__ __forceinline__ void perturb(bool exploit, R u0, R u1, float e0, float e1, R &v0, R &v1) {
    v0 = exploit ? u0 + (R)e0 : (R)e0;
    v1 = exploit ? u1 + (R)e1 : (R)e1;
}
template <typename R> __device__ __forceinline__ void clamp_controls(const KParams<R> &P, R &v0, R &v1) {
    v0 = mf::clamp(v0, P.umax0);
    v1 = mf::clamp(v1, P.umax1);
}
template <typename R>
__device__ __forceinline__ void perturb_clamp(const KParams<R> &P, bool exploit, bool clamp, R u0, R u1, float e0, float e1, R &v0, R &v1) {
    perturb(exploit, u0, u1, e0, e1, v0, v1);
    if (clamp) clamp_controls(P, v0, v1);
}

// the control term of the stage cost.  The two models associate it differently and f32 parity depends on that:
// u^T Sigma^-1 v (mppi_differential_drive.py:124) and u (Sigma^-1 v) (mppi_race_car.py:84)
template <typename R, int MODEL> __device__ __forceinline__ R control_cost(const KParams<R> &P, R u0, R u1, R v0, R v1) {
    if (MODEL == MODEL_DIFF) return (u0 * P.sinv[0] + u1 * P.sinv[2]) * v0 + (u0 * P.sinv[1] + u1 * P.sinv[3]) * v1;
    return u0 * (P.sinv[0] * v0 + P.sinv[1] * v1) + u1 * (P.sinv[2] * v0 + P.sinv[3] * v1);
}

// cost of one state: tracking error + the collision penalty (`_compute_cost` / `_c`, `_terminal_cost` / `_phi` with
// `_is_collided`); stage cost = that under the stage weights + gamma * control term (:124, mppi_race_car.py:84), terminal
// cost = that under the terminal weights (:128).  `hit`: collided() of the state; `ctrl`: control_cost of the step where
// the caller already holds it (the look-back moves it across lanes), else stage_cost takes it behind the tracking error.
// _row: against a waypoint's row {x, y, yaw, v} instead of its index (the look-back prices a sample under every candidate).
template <typename R, int MODEL>
__device__ __forceinline__ R state_cost_row(const KParams<R> &P, const R (&w)[4], bool wrap, const R *r, R x, R y, R yaw, R vel, bool hit) {
    R c = tracking_cost_row<R, MODEL>(P, w, wrap, r, x, y, yaw, vel);
    if (hit) c += P.penalty;
    return c;
}
template <typename R, int MODEL>
__device__ __forceinline__ R stage_cost_row(const KParams<R> &P, bool wrap, const R *r, R x, R y, R yaw, R vel, bool hit, R ctrl) {
    return state_cost_row<R, MODEL>(P, P.ws, wrap, r, x, y, yaw, vel, hit) + P.gamma * ctrl;
}
template <typename R, int MODEL>
__device__ __forceinline__ R stage_cost(const KParams<R> &P, bool wrap, int i, R x, R y, R yaw, R vel, bool hit, R u0, R u1, R v0, R v1) {
    const R c = state_cost_row<R, MODEL>(P, P.ws, wrap, P.ref + 4 * i, x, y, yaw, vel, hit);
    return c + P.gamma * control_cost<R, MODEL>(P, u0, u1, v0, v1);
}
template <typename R, int MODEL>
__device__ __forceinline__ R terminal_cost_row(const KParams<R> &P, bool wrap, const R *r, R x, R y, R yaw, R vel, bool hit) {
    return state_cost_row<R, MODEL>(P, P.wt, wrap, r, x, y, yaw, vel, hit);
}
template <typename R, int MODEL>
__device__ __forceinline__ R terminal_cost(const KParams<R> &P, bool wrap, int i, R x, R y, R yaw, R vel, bool hit) {
    return terminal_cost_row<R, MODEL>(P, wrap, P.ref + 4 * i, x, y, yaw, vel, hit);
}

// `S[k] += ...` one step at a time (mppi_race_car.py:84) over a sample's T stage costs and its terminal cost in a row of
// LDS: in f32 with 1e10 collision penalties the order of the additions decides which tracking terms survive
__device__ __forceinline__ float sum_rows_in_order(const float *row, int T) {
    float S = 0.f;
    for (int t = 0; t <= T; ++t) S += row[t];
    return S;
}

// The workgroup's softmin record {rho_b, eta_b, eta2_b, pad, W_b[T][2]} (:132-135, :175 with the 1/eta factored out):
// column i of W_b = the sum over the rows of sh_acc (row q: e_q eps[q, :, :], or a half-wave's private sums) ...
template <int ROWS, int PITCH, typename R>
__device__ __forceinline__ void record_columns(R *out, const R (&sh_acc)[ROWS][PITCH], int T) {
    for (int i = threadIdx.x; i < 2 * T; i += blockDim.x) {
        R s = 0;
#pragma unroll
        for (int q = 0; q < ROWS; ++q) s += sh_acc[q][i];
        out[4 + i] = s;
    }
}
// ... and its head (one thread): eta = sum e, eta2 = sum e^2 over sh_e, or over the half-waves' rescaled {eta, eta2, n_hit}
// of sh_eta; {rho, eta, eta2} into the record and {rho, eta, eta2, n_hit} into the compact copy the merge kernels read
// (n_hit: samples whose cost carries a collision penalty, mppi_stats::n_collided)
template <typename R> __device__ __forceinline__ void record_head_store(const KParams<R> &P, R *out, size_t slot, R rho, R eta, R eta2, R n_hit) {
    out[0] = rho; out[1] = eta; out[2] = eta2;
    *reinterpret_cast<VecT4<R> *>(P.heads + 4 * slot) = VecT4<R>{rho, eta, eta2, n_hit};
}
template <int N, typename R>
__device__ __forceinline__ void record_head(const KParams<R> &P, R *out, size_t slot, R rho, const R (&sh_e)[N], R n_hit) {
    R eta = 0, eta2 = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) { const R ew = sh_e[q]; eta += ew; eta2 += ew * ew; }
    record_head_store(P, out, slot, rho, eta, eta2, n_hit);
}
template <int N, typename R>
__device__ __forceinline__ void record_head(const KParams<R> &P, R *out, size_t slot, R rho, const R (&sh_eta)[N][3]) {
    R eta = 0, eta2 = 0, n_hit = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) { eta += sh_eta[q][0]; eta2 += sh_eta[q][1]; n_hit += sh_eta[q][2]; }
    record_head_store(P, out, slot, rho, eta, eta2, n_hit);
}

// controller state of this launch: *st, with the observed state / x0 index overridden by kernel arguments
// The controller state as ONE vector load (lane i <- dword i) + readlanes: a struct copy through scalar loads is
// split by the compiler into dependent pieces (pointer, then the field the first branch needs, then the rest),
// one memory round trip each.
__device__ __forceinline__ DevState load_state_words(const DevState *st) {
    static_assert(sizeof(DevState) == 72, "DevState layout");
    const int lane = wv::lane_id();
    const int w = reinterpret_cast<const int *>(st)[lane < 18 ? lane : 0];
    auto word = [&](int i) { return __builtin_amdgcn_readlane(w, i); };
    auto dbl = [&](int i) { return __builtin_bit_cast(double, ((long long)word(i + 1) << 32) | (unsigned int)word(i)); };
    DevState sv;
    sv.x0[0] = dbl(0); sv.x0[1] = dbl(2); sv.x0[2] = dbl(4); sv.x0[3] = dbl(6);
    sv.p = word(8); sv.c = word(9); sv.k_start = word(10); sv.first_k = word(11);
    sv.round = word(12); sv.path_end = word(13); sv.idx_start = word(14); sv.pad = 0;
    sv.iter = ((long long)word(17) << 32) | (unsigned int)word(16);
    return sv;
}

// `st` = P.st; the hot kernels take it as their FIRST kernel argument as well, where the dispatcher preloads it
// into SGPRs (-amdgpu-kernarg-preload-count), so that this load does not wait for the kernel-argument fetch
template <typename R> __device__ __forceinline__ DevState load_state(const KParams<R> &P, const DevState *st) {
    DevState sv = load_state_words(st);
    if (P.use_args) {
        sv.x0[0] = P.x0_arg[0]; sv.x0[1] = P.x0_arg[1]; sv.x0[2] = P.x0_arg[2]; sv.x0[3] = P.x0_arg[3];
        sv.c = P.c_arg;
    }
    return sv;
}

// Several agents per launch: agent a's view of the handle's parameters -- its own path and obstacle table (AgentScene) in
// place of ref / obs / n_ref / n_obs, resolved once at the top of the kernel (a is wave-uniform: scalar loads) in the kernel's
// own copy of its argument, so that Rollout, stage_window, load_obstacles and the searches read P as they always did.  The
// single-agent instantiations do not call it and compile to the code they had.
template <typename R> __device__ __forceinline__ void agent_scene(KParams<R> &A, const AgentScene *__restrict__ scenes, int a) {
    const AgentScene sc = scenes[a];
    A.ref = reinterpret_cast<const R *>(sc.ref);
    A.obs = reinterpret_cast<const R *>(sc.obs);
    A.n_ref = sc.n_ref;
    A.n_obs = sc.n_obs;
}
__device__ __forceinline__ bool round_unresolved(const DevState *st, int K) {
    const int fk = st->first_k;
    return fk != NO_TRIGGER && fk + 1 < K;
}


// ------------------------------------------------------------------------------------------
// The pieces of the one-launch resolution of the sequential waypoint index (LB_CAND in mppi_kernels.h; fused_lookback and
// k_rollout_dual<..., LB> in mppi_kernels.hip put them together).  Here so that the test harness reaches them one by one.
// ------------------------------------------------------------------------------------------
// Look-back (one wave): waits until the words of workgroups [0, b) carry this iteration's tag; E = the largest offset among
// them, bad = one of them is marked.  Four words per lane and 16-byte load, copy b mod LB_COPIES of the words; volatile =
// loads that bypass this XCD's L2 (the words come from the other XCDs' workgroups).  Returns false when the wait timed out
// (never seen: the iteration is then redone by the speculation rounds) -- after `limit` ticks of the 100 MHz clock
// (KParams::lb_timeout); limit 0: a workgroup with b > 0 gives up before its first poll, which is how a test times out
// without a race.
__device__ __forceinline__ bool lb_wait(const unsigned *slots, int b, unsigned tag, int lane, int &E, bool &bad, int limit) {
    static_assert(HYP_MAX_BLOCKS <= 512, "two 16-byte loads per lane cover the words");
    typedef unsigned lb_u4 __attribute__((ext_vector_type(4)));
    const volatile __attribute__((address_space(1))) lb_u4 *src =
        (const volatile __attribute__((address_space(1))) lb_u4 *)(slots + (b & (LB_COPIES - 1)) * LB_COPY_STRIDE);
    E = 0;
    bad = false;
    if (b <= 0) return true;
    if (limit <= 0) return false;
    unsigned long long t0 = 0ull;
    for (int n = 0;; ++n) {
        bool ready = true, bd = false;
        int mx = 0;
#pragma unroll
        for (int i = 0; i < HYP_MAX_BLOCKS / 256; ++i) {
            const int first = 4 * (lane + 64 * i);
            if (first < b) {
                const lb_u4 w4 = src[lane + 64 * i];
                const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (first + j < b) {
                        ready &= (w[j] & LB_TAG_MASK) == tag;
                        bd |= (w[j] & LB_BAD) != 0u;
                        mx = max(mx, (int)(w[j] & (LB_BAD - 1)));
                    }
                }
            }
        }
        if (__ballot(!ready) == 0ull) {
            E = wv::reduce<wv::OpMaxInt>(mx);
            bad = __ballot(bd) != 0ull;
            return true;
        }
        if ((n & 15) == 15) {  // (the clock is a memory round trip of its own: looked at every 16th poll only)
            const unsigned long long now = wall_clock64();
            if (t0 == 0ull) t0 = now;
            if (now - t0 > (unsigned long long)limit) return false;
        }
    }
}
// the word of workgroup b into every copy (lanes < LB_COPIES of one wave)
__device__ __forceinline__ void lb_publish(unsigned *slots, int b, unsigned word, int lane) {
    if (lane < LB_COPIES) __hip_atomic_store(&slots[b + lane * LB_COPY_STRIDE], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the offsets a workgroup's calls were entered at stay within the candidates' reach (see LB_CAND)
__device__ __forceinline__ bool lb_reach(int leave, int window, int n_ref, int c) {
    return leave < window && (leave + window <= LB_CAND || n_ref - c <= LB_CAND);
}

// pass A of one pair of candidates {x_2q, x_2q+1, y_2q, y_2q+1}: does this lane's distance fall at the first / the second
// of them (f32: two packed subtractions, a packed product and a packed fma)
typedef float lb_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lb_pair(const RefPair<float> &rp, float x, float y, float &prev, bool &g0, bool &g1) {
    const lb_f2 dx = lb_f2{x, x} - lb_f2{rp.x0, rp.x1}, dy = lb_f2{y, y} - lb_f2{rp.y0, rp.y1};
    const lb_f2 d = dx * dx + dy * dy;
    g0 = d.x < prev;
    g1 = d.y < d.x;
    prev = d.y;
}
__device__ __forceinline__ void lb_pair(const RefPair<double> &rp, double x, double y, double &prev, bool &g0, bool &g1) {
    const double dx0 = x - rp.x0, dx1 = x - rp.x1, dy0 = y - rp.y0, dy1 = y - rp.y1;
    const double d0 = dx0 * dx0 + dy0 * dy0, d1 = dx1 * dx1 + dy1 * dy1;
    g0 = d0 < prev;
    g1 = d1 < d0;
    prev = d1;
}

// Pass A for the NP positions a lane owns (an idle one: x = NaN, it never descends): m[i] = this lane's count of descents
// over the LB_CAND candidates of sh_c, `bad` = a call of this lane whose descents do not all come first.  Per candidate a
// comparison and ONE add-with-carry per lane: the comparisons are shifted into a word, first candidate in the top bit
// (w <- w + w + g), so that the count is a population count and "the descents come first" reads w == 1..10..0.  (Nothing
// on the scalar unit: lane masks per candidate had the compiler spill SGPRs into VGPR lanes in the two-samples-per-wave
// kernel, 330 lane moves per wave.)
template <int NP, typename R>
__device__ __forceinline__ void lb_scan(const RefPair<R> *sh_c, const R (&x)[NP], const R (&y)[NP], int (&m)[NP], bool &bad) {
    static_assert(LB_CAND == 32, "one bit per candidate");
    unsigned w[NP];
    R prev[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        w[i] = 0u;
        prev[i] = R(INFINITY);  // (candidate 0 is compared against +inf: the top bit, counted off below)
    }
#pragma unroll
    for (int q0 = 0; q0 < LB_CAND / 2; q0 += 4) {
        RefPair<R> rp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rp[j] = sh_c[q0 + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                bool g0, g1;
                lb_pair(rp[j], x[i], y[i], prev[i], g0, g1);
                w[i] = w[i] + w[i] + (g0 ? 1u : 0u);
                w[i] = w[i] + w[i] + (g1 ? 1u : 0u);
            }
        }
    }
    bad = false;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pc = __popc(w[i]);
        m[i] = pc - 1;
        // (an idle position: w = 0, nothing to check)
        bad |= pc > 0 && w[i] != (0xffffffffu << (32 - pc));
    }
}

}  // namespace mppi
