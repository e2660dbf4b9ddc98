// Internal interface between the C ABI (mppi_capi.hip) and the gfx950 kernels (mppi_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "mppi_grid_index.h"
#include "mppi_scene_staging.h"

namespace mppi {

constexpr int MODEL_DIFF = 0, MODEL_RACE = 1;
constexpr int OBS_NONE = 0, OBS_CIRCLE = 1, OBS_OUTLINE = 2;
constexpr int FILTER_DIFF = 0, FILTER_RACE = 1, FILTER_NONE = 2, FILTER_TORCH = 3;
constexpr int NO_TRIGGER = 0x7fffffff;
constexpr int STATUS_DONE = 0, STATUS_NEED_ROUND = 1, STATUS_PATH_END = 2, STATUS_EXCHANGE_FAILED = 3;

// Peer-to-peer exchange buffer of one rank (mppi_comm_*), fine-grained device memory every rank maps:
// two slots (iteration parity), each {long long flag[XCHG_MAX_RANKS]; double rec[nranks][xchg_rec_len(T)]}.
// Rank r owns flag[r] / rec[r] of every buffer.
constexpr int XCHG_MAX_RANKS = 64;
constexpr int XCHG_LDS_RANKS = 16;  // up to this many ranks' records are staged in LDS before they are merged
__host__ __device__ inline int xchg_rec_len(int T) { return (3 + 2 * T + 1) & ~1; }
__host__ __device__ inline size_t xchg_slot_bytes(int T, int nranks) {
    return sizeof(long long) * XCHG_MAX_RANKS + sizeof(double) * (size_t)nranks * xchg_rec_len(T);
}

// Sequential waypoint index resolved in ONE launch (mppi_differential_drive.py:201-249: one `prev_way_point_idx`
// threaded through all K (T+1) cost calls in k-major order, each call `p <- first nearest waypoint in [p, p+W)`).
// Where a call's distances to the candidates behind c first fall strictly and then never fall again -- a position
// beside a path that does not fold back within the candidates -- its first minimum over ALL of them is m = the number
// of descents, and the search entered at any p returns max(p, m) (p <= m: m is the first minimum of [p, p+W) as long
// as m - p < W; p > m: nothing behind p is smaller).  The threaded index is then a running maximum of the calls' m in
// call order: a wave reduction per sample, a row reduction per workgroup, and across workgroups a decoupled look-back
// on one word per workgroup (fused_lookback) -- every sample is priced once, with its exact index, in the one rollout
// launch, and k_finalize only reads the largest offset.  LB_CAND candidates are examined: exact while every realised
// index p keeps [p, p+W) inside them (p <= LB_CAND - W, or the path ends inside them) and below W; a call that is not
// unimodal, an index beyond that reach or a look-back that times out sets the `bad` bit of the workgroup's word, and
// k_finalize hands the iteration to the speculation rounds (exact either way).
// Word of workgroup b: [31:8] the launch pair's tag, [7] bad, [6:0] largest offset of the workgroup's own calls.
constexpr int HYP_WINDOW = 20, HYP_WINDOW_CUDA = 10;  // the search windows of the reference's files
constexpr int LB_CAND = 32, LB_BAD = 0x80;
constexpr unsigned LB_TAG_MASK = 0xffffff00u;
constexpr unsigned long long LB_TIMEOUT_TICKS = 20000ull;  // 200 us at 100 MHz
constexpr int HYP_MAX_BLOCKS = 512;  // workgroups whose words one wave reads (four per lane and 16-byte load)
constexpr int LB_COPIES = 8, LB_COPY_STRIDE = 2048;  // copies of the words and the distance between them (in words: 8 KB)
// (the tag: a sequence number the host draws per rollout / finalize launch pair -- KParams::lb_seq, never 0 mod 2^24 --, so
// that no word of an earlier launch can be taken for this one's, whatever the caller does to the iteration counter)
__host__ __device__ inline unsigned lb_tag(unsigned seq) { return (seq & 0xffffffu) << 8; }

// Controller state that lives on the device (so closed loops need no host round trip).
struct DevState {
    double x0[4];      // observed state of the current iteration
    int p;             // prev_way_point_idx at the iteration boundary
    int c;             // waypoint index the pending rollouts start from
    int k_start;       // first sample whose cost is not final yet (sequential mode rounds)
    int first_k;       // atomicMin: first sample that moved the waypoint index this round
    int round;         // speculation rounds used by the current iteration
    int path_end;      // x0's nearest waypoint is the last one
    int idx_start;     // c right after the x0 call
    int pad;
    long long iter;    // completed iterations == sampler counter
};

// What the host reads back after a step (followed by 2*T doubles: the returned u).
struct StepResult {
    int status, k_next, c_next, idx_start;
    int idx_after, path_end, rounds;
    int costs_hyp;  // the iteration's sequential index was resolved in its one rollout launch (fused_lookback)
    int n_collided, pad_res;  // samples of this handle whose cost carries a collision penalty (-1: records of other ranks merged)
    long long iter;
    double rho, eta, ess;
    double u0[2];
    double x_next[4];
    long long seq;  // written LAST (after a system-scope fence) when the host polls mapped memory for completion
};

// Per-rank softmin partial of the split step (ABI layout): {rho, eta, eta2, W[T][2]} in doubles.
__host__ __device__ inline int partial_len(int T) { return 3 + 2 * T; }
// Per-block record (internal layout, handle precision): {rho, eta, eta2, pad, W[2T] padded to 16 bytes}.
__host__ __device__ inline int record_len(int T, int elem_bytes) {
    const int vw = 16 / elem_bytes;
    return 4 + ((2 * T + vw - 1) / vw) * vw;
}

// LDS of the merge code (k_merge / k_finalize), in elements of the handle's precision: the weighted noise in the
// filter's padded layout [2 (T + W + 1)], the updated controls [2T], 64 record scales per wave and window, block
// reductions, per-group partial sums.  Every region starts on a 16-byte boundary.
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_MAX_RECORDS = 256;  // per window: what one k_merge workgroup takes, and the ABI records (one per rank) of a finalize
constexpr int MERGE_MAX_WINDOWS = 2;    // k_finalize takes up to 512 records itself (K = 16384 in the dual layout)
__host__ __device__ inline size_t merge_lds_elems(int T, int W, size_t elem, int nt = MERGE_THREADS) {
    const size_t r4 = 3, nw = (2 * (size_t)(T + W + 1) + r4) & ~r4, nu = (2 * (size_t)T + r4) & ~r4;
    return nw + nu + (size_t)MERGE_MAX_WINDOWS * nt + 64 + (size_t)(nt / 32) * 32 * (16 / elem);
}
// The merge tree between the n records a rollout launch leaves (per agent) and their reader, the one place that knows its
// shape.  k_finalize reads up to MERGE_MAX_WINDOWS windows, the k_merge that writes a rank's one record (split step) one;
// more records than that go through ONE k_merge launch first, `group` records per workgroup: 64, or a whole window where
// 64:1 would leave more than a window.  What it leaves fits a window (n <= 256 * 256: K <= 2^20 samples, >= 16 per record).
// group: records per workgroup of the merge launch in front of the reader, 0: none; n_out: records the reader takes, in
// `windows` windows of MERGE_MAX_RECORDS
struct MergeTree { int group, n_out, windows; };
inline MergeTree merge_tree(int n, bool finalize_reads) {
    MergeTree t = {0, n, 1};
    if (n > (finalize_reads ? MERGE_MAX_WINDOWS : 1) * MERGE_MAX_RECORDS) {
        t.group = n > 64 * MERGE_MAX_RECORDS ? MERGE_MAX_RECORDS : 64;
        t.n_out = (n + t.group - 1) / t.group;
    }
    t.windows = (t.n_out + MERGE_MAX_RECORDS - 1) / MERGE_MAX_RECORDS;
    return t;
}

// One agent's scene (several agents per handle, mppi_config.n_agents > 1): its reference path and obstacle table in the
// handle's precision and their lengths.  The handle keeps AgentScene[n_agents] in device memory and rewrites it on every
// setter; agents that share a scene carry the same pointers.  The batched kernels read entry blockIdx.y (scalar loads) and
// see the handle's parameters with these four fields in place of ref / obs / n_ref / n_obs (agent_scene, mppi_device.h); the
// single-agent kernels never read the table.
struct alignas(32) AgentScene {
    const void *ref, *obs;  // [n_ref][4], [n_obs][4] as KParams::ref / obs
    int n_ref, n_obs;       // (n_obs: 0 for a handle without an obstacle model)
    long long iter0;        // moving obstacles: DevState::iter when this agent's set was uploaded (KParams::iter0)
};
static_assert(sizeof(AgentScene) == 32 && offsetof(AgentScene, iter0) == 24, "AgentScene layout");

template <typename R> struct KParams {
    int K, T, k_offset, noise_stream;  // noise_stream: fourth Philox counter word (of agent 0) -- kept in the first
                                       // kernel-argument fetch: the draw is the first thing a wave does
    int n_exploit, n_ref, n_obs, window;
    int model, accumulate, sequential, obstacle_model;
    int clamp_rollout, wrap_stage, wrap_term, use_philox;
    int traj_per_block, slots;  // slots: several agents per launch, records per agent in the partials / heads buffers
    unsigned seed_lo, seed_hi;
    R dt, umax0, umax1, wheel_base;
    R beta, gamma, penalty, two_pi;
    R sinv[4], ws[4], wt[4];
    R shape_x[9], shape_y[9];
    float chol[3];
    const R *ref;      // [n_ref][4]  x, y, yaw, v
    const R *obs;      // [n_obs][4]  x, y, threshold^2, 0; obs_motion: followed by [n_obs][4]  vx, vy, 0, 0 (row n_obs + m: circle m)
    const R *u;        // [T][2] nominal controls
    const float *eps;  // [K][T][2] or nullptr (Philox); with eps_slots > 0: a ring [eps_slots][n_agents][K][T][2]
    int eps_slots;     // 0: `eps` is this call's tensor; 2^n: iteration i reads slot i mod eps_slots (mppi_set_noise_ring)
    int obs_motion;    // mppi_config.obstacle_motion: the circles carry velocities and the moving instantiations serve; 2
                       // (OBS_MOTION_TRACKS): some agent has obstacle tracks as well and the track forms serve; 3
                       // (OBS_MOTION_GRID): some agent has a cost grid and the grid forms serve (this word was padding:
                       // the layout stays)
    R *S;              // [K]
    int *pout;         // [K] waypoint index after sample k (sequential mode)
    DevState *st;
    R *heads;          // [n records][4] {rho, eta, eta2, 0}: compact copy of the record heads, so that the merge
                       // kernels read them coalesced (inside the records they sit 16 + 8T bytes apart)
    // synchronous step: the observed state and its nearest-waypoint index arrive as kernel arguments (the x0
    // call, mppi_differential_drive.py:96-99, was made by the host side of the ABI) instead of through *st
    int use_args, c_arg;
    double x0_arg[4];
    // several agents per launch (blockIdx.y): agent a's u / S / pout / state / records / heads follow agent a-1's
    int n_agents, layout;   // layout: rollout_layout() of the handle (host side only)
    // MPPI_WAYPOINT_PER_ROLLOUT: the index threads through a sample's own cost calls (as `sequential` threads it through
    // all samples' calls) and starts from the x0 call's index at every sample: samples stay independent
    int per_rollout;
    int lb_timeout;         // ticks of the 100 MHz clock a look-back may wait (lb_wait; Switches::lb_timeout_ticks), 0: not at all
    // one-launch resolution of the sequential index (see LB_CAND)
    int hyp;                // the look-back serves the handle (lookback_serves, mppi_capi.hip) and the index can still move:
                            // what the rollout planners read; RolloutPlan::lookback says whether the launch they picked publishes words
    unsigned lb_seq;        // this launch pair's tag (see lb_tag)
    unsigned *hyp_slots;    // [HYP_MAX_BLOCKS] one word per workgroup
    // several agents per launch: every agent's scene (null for a single agent).  ref / obs / n_ref / n_obs above are agent
    // 0's then -- what anything that does not read the table sees -- and obstacle_model says whether ANY agent has obstacles.
    // Last, so that the first kernel-argument fetch keeps its layout; padded to 32 bytes, so that the arguments behind the
    // struct keep their alignment and the compiler merges their loads as it did (the single-agent kernels' code is unchanged).
    const AgentScene *scenes;
    // moving obstacles: the value of DevState::iter when the set (agent 0's here, every agent's in the table) was uploaded.  A
    // rollout step j steps ahead tests against c + v dt (iter - iter0 + j).  (It took a padding word: the layout stays.)
    long long iter0;
    // Fleet plans (mppi_set_fleet_prediction, MPPI_FLEET_PLAN): word 0 the address of the plan table R[n_agents][T + 1][2], word 1
    // the mates' squared threshold as an R in its low bytes (fleet_plan_table / fleet_plan_thr2 below); both 0 otherwise.  (The
    // two words were padding: the layout stays.)
    long long pad_scenes[2];
};
// One point of a plan: agent a's position after j rollout steps of its nominal controls is row a (T + 1) + j of the table
template <typename R> struct alignas(2 * sizeof(R)) PlanPoint { R x, y; };
template <typename R> __host__ __device__ inline const PlanPoint<R> *fleet_plan_table(const KParams<R> &P) {
    return reinterpret_cast<const PlanPoint<R> *>(P.pad_scenes[0]);
}
template <typename R> __host__ __device__ inline R fleet_plan_thr2(const KParams<R> &P) {
    R v;
    __builtin_memcpy(&v, &P.pad_scenes[1], sizeof(R));
    return v;
}
// The plan forms stage the whole table into dynamic LDS where it fits beside their own LDS within the 64 KB a workgroup gets
// without raising a limit: up to 40000 bytes beside the f32 forms' 18.6 / 24.8 KB, 16384 beside the f64 forms' 37.2 / 47.5 KB.
// (Every form runs ONE workgroup of 16 waves per CU -- occupancy 4 - 7 waves per SIMD -- so no size lowers that; staging
// costs the forms no register, scratch or occupancy: DESIGN 3.10.)  Larger tables are read from memory.  One function for the
// planner, which sizes the launch's dynamic LDS by it, and the kernel, which decides by it where it reads.
template <typename R> __host__ __device__ inline int fleet_plan_lds_bytes(int n_agents, int T) {
    const long long bytes = (long long)n_agents * (T + 1) * 2 * (long long)sizeof(R);
    return bytes <= (sizeof(R) == 4 ? 40000 : 16384) ? (int)bytes : 0;
}
template <typename R> inline void set_fleet_plan(KParams<R> &P, const void *table, R thr2) {
    P.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(table);
    P.pad_scenes[1] = 0;
    __builtin_memcpy(&P.pad_scenes[1], &thr2, sizeof(R));
}
// Obstacle tracks (mppi_set_obstacle_tracks; a handle with obstacle_motion and no fleet, so pad_scenes is free): one descriptor
// per agent in device memory, rewritten by every setter and read afresh by every launch (a replayed graph too).  Track m's
// point i -- its centre i control steps after the upload -- is pts[m L + i]; thr2[m] is its squared threshold, packed as
// set_circles packs a circle of that radius; iter0 is the agent's DevState::iter at the upload.  The state a rollout reaches
// after j steps is tested against point track_index(clock, j, L).  n = 0: the agent has no tracks.
struct alignas(32) TrackSet {
    const void *pts;   // PlanPoint<R>[n][L]
    const void *thr2;  // R[n]
    int n, L;
    long long iter0;
};
static_assert(sizeof(TrackSet) == 32, "TrackSet layout");
constexpr int TRACKS_MAX = 256, TRACK_LEN_MAX = 65536;
// KParams::pad_scenes on such a handle: word 0 the address of TrackSet[n_agents] (0: no agent has tracks, the SPEC = 3 forms
// serve), word 1 the bytes of dynamic LDS the launch was sized for (0: the points are read from memory)
template <typename R> __host__ __device__ inline const TrackSet *track_sets(const KParams<R> &P) {
    return reinterpret_cast<const TrackSet *>(P.pad_scenes[0]);
}
// (KParams::obs_motion says which of the two users of pad_scenes a handle is: the planners read it, no kernel does)
constexpr int OBS_MOTION_TRACKS = 2;
template <typename R> __host__ __device__ inline int track_staged_bytes(const KParams<R> &P) { return (int)P.pad_scenes[1]; }
// the control steps since the upload, kept inside the table whatever the counter says
__host__ __device__ inline int track_clock(long long iter, long long iter0, int L) {
    const long long c = iter - iter0;
    return c < 0 ? 0 : c > L - 1 ? L - 1 : (int)c;
}
// the point a state j >= 0 steps ahead is tested against: a track holds its last point once it runs out
__host__ __device__ inline int track_index(int clock, int j, int L) { return j < L - 1 - clock ? clock + j : L - 1; }
// A workgroup of the track forms stages the window its clock selects -- T + 1 points per track, then the thresholds -- into
// dynamic LDS where the largest set among the agents fits beside the forms' own LDS within the 64 KB a workgroup gets without
// raising a limit: fleet_plan_lds_bytes' limits, for its reason.  Larger sets are read from memory with the clamped index.
// One function for the planner, which sizes the launch by it, and (through pad_scenes[1]) the kernel.
template <typename R> __host__ __device__ inline int track_lds_bytes(int n_max, int T) {
    const long long bytes = (long long)n_max * ((T + 1) * 2 + 1) * (long long)sizeof(R);
    return bytes <= (sizeof(R) == 4 ? 40000 : 16384) ? (int)bytes : 0;
}
template <typename R> inline void set_tracks(KParams<R> &P, const TrackSet *sets, int n_max) {
    P.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(sets);
    P.pad_scenes[1] = sets ? track_lds_bytes<R>(n_max, P.T) : 0;
    if (sets) P.obs_motion = OBS_MOTION_TRACKS;
}
// Cost grids (mppi_set_cost_grid; a handle with obstacle_motion, no fleet and no tracks, so pad_scenes is free): one descriptor
// per agent in device memory, rewritten by every setter and read afresh by every launch (a replayed graph too).  cells is the
// table [ny][nx], row-major, node (ix, iy) at the world point (ox + ix / inv, oy + iy / inv); everything in the handle's
// precision.  nx = 0: the agent has no grid.
template <typename R> struct alignas(8) GridSet {
    const R *cells;
    int nx, ny;
    R ox, oy, inv, weight, lethal;
};
static_assert(sizeof(GridSet<float>) == 40 && sizeof(GridSet<double>) == 56, "GridSet layout");
constexpr int GRID_DIM_MIN = 2, GRID_DIM_MAX = 4096;
// KParams::pad_scenes on such a handle: word 0 the address of GridSet<R>[n_agents] (0: no agent has a grid, the SPEC = 3 forms
// serve), word 1 is 0 (the cells are read from memory: a staged window was tried and cost more).
// KParams::obs_motion = OBS_MOTION_GRID marks the third user of those words (the planners read it)
constexpr int OBS_MOTION_GRID = 3;
template <typename R> __host__ __device__ inline const GridSet<R> *grid_sets(const KParams<R> &P) {
    return reinterpret_cast<const GridSet<R> *>(P.pad_scenes[0]);
}
template <typename R> inline void set_grids(KParams<R> &P, const void *sets) {
    P.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(sets);
    P.pad_scenes[1] = 0;
    if (sets) P.obs_motion = OBS_MOTION_GRID;
}
// Composed scenes (mppi_set_scene_mode: MPPI_SCENE_COMPOSED; a handle that holds at least two of {plans, tracks, a grid}): the
// three users of pad_scenes behind one carrier.  KParams::obs_motion = OBS_MOTION_SCENE marks a launch whose pad_scenes[0] is
// the address of ONE SceneTable<R> in device memory -- the handle's, rewritten by every setter and read afresh by every launch
// (a replayed graph too) -- that points at the per-agent arrays the host keeps anyway; a null pointer: no agent has that
// ingredient.  pad_scenes[1] carries the two staged byte counts of the launch: the plans' in its low 32 bits, the tracks' in
// its high 32 bits (0: read from memory); the tracks stand 16-byte aligned behind the plans in dynamic LDS.
constexpr int OBS_MOTION_SCENE = 4;
template <typename R> struct alignas(16) SceneTable {
    const PlanPoint<R> *plans;  // R[n_agents][T + 1][2] (fleet_plan_table), or null
    const TrackSet *tracks;     // [n_agents], or null
    const GridSet<R> *grids;    // [n_agents], or null
    R thr2;                     // the mates' squared threshold (fleet_plan_thr2)
};
static_assert(sizeof(SceneTable<float>) == 32 && sizeof(SceneTable<double>) == 32, "SceneTable layout");
template <typename R> __host__ __device__ inline const SceneTable<R> *scene_table(const KParams<R> &P) {
    return reinterpret_cast<const SceneTable<R> *>(P.pad_scenes[0]);
}
// What a composed launch stages into dynamic LDS: mppi_scene_lds_bytes (mppi_scene_staging.h), one function for the planner,
// which sizes the launch by it, and -- through pad_scenes[1] -- the kernel.  Plans first, the tracks' window 16-byte aligned
// behind them, each only if it fits the budget of fleet_plan_lds_bytes; whatever does not fit is read from memory.
template <typename R> __host__ __device__ inline mppi_scene_staging scene_lds_bytes(int n_plan_agents, int n_max, int T) {
    return mppi_scene_lds_bytes((int)sizeof(R), n_plan_agents, n_max, T);
}
template <typename R> __host__ __device__ inline mppi_scene_staging scene_staged(const KParams<R> &P) {
    const unsigned long long w = (unsigned long long)P.pad_scenes[1];
    return mppi_scene_staging{(int)(w & 0xffffffffull), (int)(w >> 32)};
}
// (table: the handle's SceneTable<R>; n_plan_agents: n_agents where the handle is in plan mode, else 0; n_max: its largest
// track set)
template <typename R> inline void set_scene(KParams<R> &P, const void *table, int n_plan_agents, int n_max) {
    const mppi_scene_staging s = scene_lds_bytes<R>(n_plan_agents, n_max, P.T);
    P.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(table);
    P.pad_scenes[1] = (long long)(((unsigned long long)(unsigned)s.tracks << 32) | (unsigned long long)(unsigned)s.plans);
    P.obs_motion = OBS_MOTION_SCENE;
}
// Learned-dynamics scene handles (mppi_config.obstacle_motion = 2; mppi_mlp.hip) use this carrier for EVERY launch,
// whatever the handle holds: moving circles alone, tracks, a grid or both.  `plans` stays null except on a fleet handle
// (obstacle_motion = 3) in plan mode, whose fleet forms read the table and `thr2` from here (mlp_mates_collided),
// and nothing is staged in LDS -- at a step of the learned rollout every lane reads the same track point --, so pad_scenes[1],
// the staged byte counts of the analytic composed launch, is free there: it carries the footprint word (MPPI_GRID_FOOTPRINT_*),
// which the learned scene forms read at run time where the analytic forms take a template argument.  No pinned layout moves:
// KParams, SceneTable and GridSet are what they were, and k_eval_pose overwrites both words itself (scene_plan_words).
template <typename R> inline void set_scene_learned(KParams<R> &P, const void *table, int footprint) {
    P.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(table);
    P.pad_scenes[1] = (long long)footprint;
    P.obs_motion = OBS_MOTION_SCENE;
}
template <typename R> __host__ __device__ inline int learned_scene_footprint(const KParams<R> &P) { return (int)P.pad_scenes[1]; }
// the lower node and the fraction of coordinate x along an axis of n >= 2 nodes (mppi_grid_index.h: inside [0, n - 2] and
// [0, 1] whatever x is, a NaN included)
__host__ __device__ inline int grid_index(float x, float o, float inv, int n, float &f) { return mppi_grid_index_f32(x, o, inv, n, &f); }
__host__ __device__ inline int grid_index(double x, double o, double inv, int n, double &f) { return mppi_grid_index_f64(x, o, inv, n, &f); }
// (lb_timeout took the place of a padding word: the layout the kernels' argument loads were tuned for stays as it was)
static_assert(sizeof(KParams<float>) == 424 && sizeof(KParams<double>) == 576, "KParams layout");
static_assert(offsetof(KParams<float>, hyp) == 376 && offsetof(KParams<double>, hyp) == 528, "KParams layout");
static_assert(offsetof(KParams<float>, scenes) == 392 && offsetof(KParams<double>, scenes) == 544, "KParams layout");
static_assert(offsetof(KParams<float>, iter0) == 400 && offsetof(KParams<double>, iter0) == 552, "KParams layout");

struct FinalizeParams {
    int T, K, n_part, pad2;
    int filter_mode, filter_window, clamp_u, raise_at_path_end;
    int model, sequential, plant, n_ref;
    int window, is_f64, count_hits, pad1;  // count_hits: the block records' heads carry collision counts (a handle with obstacles;
                                           // batched: an agent with n_obs > 0, or -- 2, fleet plans -- every agent)
    double beta, dt, wheel_base, umax0, umax1;
    const void *partials;    // [n_part] records: the slot plan's, or the caller's ABI records [n_part][partial_len], n_part <= 256
    const void *heads;       // compact heads of `partials` (KParams::heads); unused for the ABI layout
    void *u;                 // [T][2] in the kernel precision: the controls the finished rollouts used
    void *u_out;             // where the updated, shifted controls go (== u: in place)
    DevState *st_out;        // where the state after this call goes (== st: in place)
    void *u_before;          // copy of u before the update (for the viz rollouts)
    const void *ref;         // [n_ref][4] kernel precision
    const int *pout;
    DevState *st;
    StepResult *res;         // followed by 2*T doubles (device memory, or host memory mapped into the device)
    double *u0_trace;        // nullable: closed-loop trace [iter][2]
    long long seq;           // != 0: publish res->seq = seq last, behind a system-scope fence (host polls it)
    int use_args, c_arg;     // see KParams
    double x0_arg[4];
    // K sharded over GPUs with the records exchanged peer to peer: after merging its own block records the
    // block stores this rank's record into slot (x_seq & 1) of EVERY rank's exchange buffer, raises its
    // flag there to x_seq, waits for all flags in its own buffer and merges the x_nranks records
    int x_nranks, x_rank;    // x_nranks <= 1: no exchange
    long long x_seq;         // > 0, the same on every rank for the same iteration, increasing
    long long x_timeout;     // 100 MHz ticks the wait may take before the iteration is abandoned
    char *const *x_peers;    // device array [x_nranks]: every rank's exchange buffer (own one included)
    int *x_err;              // sticky device flag: an exchange timed out, later slots return at once
    // several agents per launch (blockIdx.y), see KParams
    int slots, n_agents;
    size_t res_stride;       // bytes between two agents' StepResult (+ returned u)
    // one-launch resolution of the sequential index (see LB_CAND / KParams): filled from the slot plan -- hyp its `lookback`
    // (plan_finalize picks the HYPK kernel from that flag), hyp_blocks the rollout plan's record count
    int hyp, hyp_blocks;
    const unsigned *hyp_slots;
    unsigned lb_seq, pad_lb;
    const AgentScene *scenes;  // see KParams: ref / n_ref above are agent 0's, count_hits says whether any agent has obstacles
    long long pad_scenes[3];
};

// learned residual dynamics (mppi_mlp.hip): device pointers to fragment-packed weights.  Hidden width H in {64, 128, 256, 512}
// and depth n_hidden in {1, 2, 3, 4} (mppi_set_mlp); 512 x 3 and 512 x 2 run k_rollout_mlp_h3 / k_rollout_mlp, the other
// shapes k_rollout_mlp_w<H, ...>
constexpr int MLP_MAX_HIDDEN = 4;
struct MlpParams {
    const float *w_in, *b_in;        // Linear(5 -> H): packed [H / 32][1][64][4], bias [H]
    const float *w_h[MLP_MAX_HIDDEN], *b_h[MLP_MAX_HIDDEN];  // Linear(H -> H): packed [H / 32][H / 8][64][4], bias [H]
    const float *w_out;              // Linear(H -> 3): [3][H] as in the checkpoint
    float b_out[3];
    // the f16-split kernels (k_rollout_mlp_h3, k_rollout_mlp_w): per layer two f16 planes (hi, then lo) in their fragment order
    int use_h3;
    const unsigned short *h3_w_in;   // [2][H / 32][1][64][8]
    const unsigned short *h3_w_h[MLP_MAX_HIDDEN]; // [2][H / 32][H / 16][64][8]
    // |W_in z + b_in|_inf <= in_gain |z|_inf + in_bias: the split kernel derives the per-sample power-of-two scale of the
    // first layer's output from it, so that no f16 half overflows whatever the magnitude of the inputs
    float in_gain, in_bias;
    int n_hidden;  // hidden Linear(H, H) + tanh layers: 3 (the architecture train/train_diff_mlp.py:13-36 builds), 2 (the
                   // reference's older checkpoints, saved_models/mlp_diff.pth, mlp_diff_300x100.pth, ..._v2.pth), 1 or 4
    int hidden;    // H
};

// the shapes k_rollout_mlp_h3 (and the f32-input k_rollout_mlp) serve; every other supported shape runs k_rollout_mlp_w
inline bool mlp_shape_is_h3(int hidden, int n_hidden) { return hidden == 512 && (n_hidden == 2 || n_hidden == 3); }
inline bool mlp_shape_supported(int hidden, int n_hidden) {
    return (hidden == 64 || hidden == 128 || hidden == 256 || hidden == 512) && n_hidden >= 1 && n_hidden <= MLP_MAX_HIDDEN;
}

struct VizParams {
    int K, T, model, clamp_rollout;
    int k_offset, n_exploit, use_philox, pad;
    unsigned seed_lo, seed_hi;
    long long iter;
};

template <typename R> void launch_set_state(const KParams<R> &P, const double *x0_or_null, hipStream_t s);
// softmin partial records are stored in the handle's precision R (block partials) or as double (the
// per-rank record of the split step, include/mppi_hip.h)
template <typename R> void launch_reduce(const KParams<R> &P, void *partials, int n_blocks, hipStream_t s);
bool fused_supported(int T);

// The environment switches, read in ONE place -- read_switches() in mppi_capi.hip -- when a handle is
// created (the learned-dynamics ones again at mppi_set_mlp, the exchange timeout at mppi_comm_connect) and kept in the
// handle: rollout_layout() and the planners below take them as an argument, so that a launch costs no environment lookups
// and the plan, the launch and the reported kernel name cannot disagree.
struct Switches {
    int dual = -1, pair = -1, tri = -1;  // MPPI_DUAL / MPPI_PAIR / MPPI_TRI: -1 unset, else 0 / 1
    int seq = -1;                        // MPPI_SEQ: -1 unset, else its value (2: two passes per workgroup, else one)
    bool no_stream = false;              // MPPI_NO_STREAM
    int stream_passes = 0;               // MPPI_STREAM_PASSES (> 0: forced)
    bool force_unfused = false, no_hyp = false, no_poll = false, no_args = false;  // MPPI_FORCE_UNFUSED / _NO_HYP / _NO_POLL / _NO_ARGS
    int traj_per_block = 0;              // MPPI_TRAJ_PER_BLOCK
    bool graph = false, graph_verbose = false;  // MPPI_GRAPH / MPPI_GRAPH_VERBOSE
    int graph_slots = 64;                // MPPI_GRAPH_SLOTS
    // the learned-dynamics switches, as the last mppi_set_mlp found them: MPPI_MLP_F32, MPPI_MLP_TERMS (2 or 3), MPPI_MLP_FORM
    // (-1 the default form, 0 "4x64", 1 "8x64")
    struct Mlp { bool f32 = false; int terms = 3, form = -1; } mlp;
    long long exchange_timeout_ms = 0;   // MPPI_EXCHANGE_TIMEOUT_MS (> 0: set)
    int lb_timeout_ticks = (int)LB_TIMEOUT_TICKS;  // MPPI_LB_TIMEOUT_TICKS (>= 0; 0: a look-back never waits -- see lb_wait)
};

// One kernel launch, resolved once: which instantiation and how it is launched.  Made by the planners -- plan_rollout, plan_merge,
// plan_finalize (mppi_kernels.hip), plan_mlp (mppi_mlp.hip): pure functions of the kernel parameters and the switches, a
// handful of branches -- and executed by launch_plan.  A new kernel variant is one more entry in its family's planner.
struct KernelLaunch {
    const void *fn = nullptr;    // the __global__ instantiation
    const char *name = "";       // as rocprofv3 spells it ("k_rollout_dual<float, 1, 1, false, 2, true, false>"); static storage
    dim3 grid, block;
    size_t lds = 0;              // dynamic LDS bytes
    bool *lds_raised = nullptr;  // per device: hipFuncAttributeMaxDynamicSharedMemorySize was raised to `lds` (null: not needed)
};
// A rollout launch and what it leaves
struct RolloutPlan {
    KernelLaunch k;
    int records = 0;        // softmin records per agent the launch leaves (k_rollout: what launch_reduce leaves behind it)
    int passes = 0;         // k_rollout_stream's batches per workgroup, else 0
    bool lookback = false;  // the instantiation publishes look-back words (LB_CAND): only then does k_finalize<..., HYPK> follow
};
// A k_merge launch: groups of `group` <= 256 records (handle precision) of recs[n] -> out[ceil(n / group)], internal layout
// with compact heads, or -- out_heads null -- the ABI layout in doubles
struct MergeStep {
    KernelLaunch k;
    const void *recs = nullptr, *heads = nullptr;
    int n = 0, group = 0;
    void *out = nullptr, *out_heads = nullptr;
};
constexpr int PLAN_MAX_DEVICES = 64;
// What is static about one instantiation, kept as a function-local static of its *_entry template beside the function
// pointer: the name, formatted once from the template arguments it is launched with, and the `lds_raised` flags
struct KernelEntry {
    char name[96];
    bool lds_raised[PLAN_MAX_DEVICES] = {};
    __attribute__((format(printf, 2, 3))) explicit KernelEntry(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(name, sizeof(name), fmt, ap);
        va_end(ap);
    }
    static const char *of(bool b) { return b ? "true" : "false"; }
};
inline KernelLaunch plan_entry(const void *fn, KernelEntry &e, int threads, size_t lds = 0) {
    KernelLaunch p;
    p.fn = fn;
    p.name = e.name;
    p.block = dim3(threads);
    p.lds = lds;
    p.lds_raised = lds ? e.lds_raised : nullptr;
    return p;
}
// `args`: the kernel's arguments in order (a kernel with a shorter list takes the first ones).  Every kernel is launched
// from the file that defines it: this is inline so that each of the two files carries its own copy.
inline void launch_plan(const KernelLaunch &p, void **args, hipStream_t s) {
    if (p.lds_raised) {  // (the attribute belongs to the device's copy of the code object: one process may drive several GPUs)
        int dev = 0;
        (void)hipGetDevice(&dev);
        const bool known = dev >= 0 && dev < PLAN_MAX_DEVICES;
        if (!known || !p.lds_raised[dev]) {
            (void)hipFuncSetAttribute(p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
            if (known) p.lds_raised[dev] = true;
        }
    }
    (void)hipLaunchKernel(p.fn, p.grid, p.block, args, p.lds, s);
}

// Which fused rollout kernel serves (K, T): decided ONCE per handle (the MPPI_DUAL / MPPI_PAIR / MPPI_TRI / MPPI_SEQ
// overrides arrive in `sw`) and carried in KParams::layout.
enum { LAYOUT_FUSED = 0, LAYOUT_DUAL = 1, LAYOUT_PAIR = 2, LAYOUT_TRI = 3, LAYOUT_KIND = 3, LAYOUT_TWICE = 4 };  // (KIND: mask)
// n_agents: problems batched in one launch; tri_ok: the handle is what k_rollout_tri serves (race car, f32, frozen index,
// `S[k] +=`, one agent) -- it takes horizons of 65 .. 96 steps then
// moving: mppi_config.obstacle_motion -- the one-sample-per-wave layout for every K (the only one with moving instantiations)
int rollout_layout(const Switches &sw, int K, int T, int n_agents, int model, bool f64, bool per_rollout = false, bool tri_ok = false,
                   bool moving = false);
int fused_blocks(int K, int T, int layout);  // workgroups = block records of a launch of the layout's own kernels
// the most records per agent any fused launch of this layout can leave (the streaming kernel, which serves the two-samples-
// per-wave layout where it can, leaves up to one per batch): what a handle sizes its record buffers by
int fused_max_records(int K, int T, int layout);
// the rollout launch of an analytic-model handle: k_rollout (fused false; launch_reduce follows, `records` is its count),
// else k_rollout_fused / _dual / _tri by P.layout, or k_rollout_stream where it serves (T <= 128)
// footprint: the handle prices its cost grid under the vehicle's outline (mppi_set_cost_grid_footprint) -- a property of the
// launch's form, carried by no descriptor: where the grid form or the composed form would have served, the one beside it
template <typename R> RolloutPlan plan_rollout(const KParams<R> &P, bool fused, const Switches &sw, bool footprint = false);
template <typename R> void launch_rollout(const RolloutPlan &plan, const KParams<R> &P, void *partials, hipStream_t s);
template <typename R> MergeStep plan_merge(const void *recs, const void *heads, int n, int group, int T, void *out, void *out_heads);
template <typename R> void launch_merge(const MergeStep &m, int T, double beta, hipStream_t s);
// k_finalize over F.partials: F.n_part <= 512 records of precision R -- with F.x_nranks > 1 the peer-to-peer exchange variant --
// or (abi_recs) <= 256 ABI records in doubles.  lookback: RolloutPlan::lookback of the rollout in front of it
template <typename R> KernelLaunch plan_finalize(const FinalizeParams &F, bool abi_recs, bool lookback);
void launch_finalize(const KernelLaunch &k, const FinalizeParams &F, hipStream_t s);
// exchange self-test: one flag round over the peers, no records
void launch_exchange_probe(const FinalizeParams &F, int *ok_out, hipStream_t s);
// batched stage methods (mppi_eval_*): `what` of launch_eval
enum { EVAL_TRANSITION = 0, EVAL_COST_STAGE = 1, EVAL_COST_TERMINAL = 2, EVAL_COLLIDED = 3, EVAL_CLAMP = 4 };
template <typename R>
void launch_eval_index(const KParams<R> &P, const R *xy, int stride, int n, int p0, int sequential, int *idx_out, int *p_out,
                       hipStream_t s);
template <typename R>
void launch_eval(const KParams<R> &P, int what, const R *x, const R *v, const int *idx, int n, R *out, hipStream_t s);
// the same for a handle with moving obstacles (k_eval_pose): pose i is tested against P's circles steps[i] rollout steps ahead of
// the current clock (steps null: 0), and against what `form` says P carries for agent `agent` -- its mates at point steps[i] of
// their plans (set_fleet_plan; steps inside [0, T]), its tracks at point track_index(clock, steps[i], L) (set_tracks; any step
// >= 0), its cost grid at the state's position in the hit and in the cost (set_grids), or all of them behind the SceneTable
// (set_scene); | EVAL_FORM_FOOT: the grid priced under the vehicle's outline (the pose's yaw column).
// what: EVAL_COST_STAGE, EVAL_COST_TERMINAL or EVAL_COLLIDED, or one of the two that read the grid alone (form: GRID or SCENE;
// idx and steps are not read) -- EVAL_GRID_POINTS: x is xy[n][2] and out[i] the raw value of the grid there;
// EVAL_GRID_FOOTPRINT: x is pose[n][3] = x, y, yaw, out[i] = g_foot of the grid there and pts (nullable) [n][9][2] its nine
// world points.  pts is read by no other `what`.
enum { EVAL_FORM_CIRCLES = 0, EVAL_FORM_PLANS = 1, EVAL_FORM_TRACKS = 2, EVAL_FORM_GRID = 3, EVAL_FORM_SCENE = 4, EVAL_FORM_FOOT = 8 };
constexpr int EVAL_GRID_POINTS = 16, EVAL_GRID_FOOTPRINT = 17;
template <typename R>
void launch_eval_pose(const KParams<R> &P, int form, int what, int agent, const R *x, const int *idx, const int *steps, int n, R *out,
                      R *pts, hipStream_t s);
// Fleet avoidance (mppi_config.fleet_radius): what k_fleet_rows takes.  Agent b's table (AgentScene::obs, n_obs rows of circles
// then n_obs rows of velocities) ends in n_agents - 1 mate rows; FleetClear is agent b's persistent clearance record.
struct FleetClear {
    double min_dist;          // smallest centre distance to a mate over the counted launches (+inf: none)
    long long contact_iters;  // counted launches that found it below `contact`
};
struct FleetParams {
    const AgentScene *scenes;  // [n_agents]
    const DevState *st;        // [n_agents]
    const void *u;             // [n_agents][T][2] nominal controls in the handle's precision
    FleetClear *clear;         // [n_agents]
    int n_agents, T, model;
    int count;                 // 1: an iteration starts here (the clearance records it); 0: a refresh for a getter / mppi_eval_*
    double dt, umax0;          // dt: as KParams::dt (already rounded to the handle's precision)
    double thr2;               // a mate's packed threshold, as set_circles packs a circle of radius fleet_radius
    double contact;            // 2 * fleet_radius
    // MPPI_FLEET_PLAN (appended: k_fleet_rows reads none of it).  plans != null: k_fleet_plan takes the launch's place and writes
    // every agent's plan -- its nominal controls rolled out from its state, clamped where the rollout clamps -- instead of rows
    void *plans;               // [n_agents][T + 1][2] in the handle's precision, or null (MPPI_FLEET_VELOCITY)
    int clamp_rollout, pad_plan;
    double umax1, wheel_base;
};
// the launch at the front of a fleet handle's slot: k_fleet_rows, or k_fleet_plan where F.plans is set
template <typename R> void launch_fleet_rows(const FleetParams &F, hipStream_t s);
template <typename R> void launch_eval_filter(const R *xx, R *out, int T, int W, int mode, hipStream_t s);
void launch_eval_weights(const double *S, int n, double beta, double *w, hipStream_t s);
template <typename R> void launch_set_state_dev(const KParams<R> &P, const double *x_dev, int nx, hipStream_t s);
template <typename R> void launch_weights(const KParams<R> &P, double rho, double eta, double *w_out, hipStream_t s);
void launch_sample(unsigned seed_lo, unsigned seed_hi, unsigned iter, int K, int T, int k_offset, const float *chol,
                   float *eps_out, hipStream_t s, unsigned stream_word = 0);
template <typename R>
void launch_viz(const KParams<R> &P, const R *u_before, const R *u_after_pre_shift, long long iter, float *opt,
                float *smp, hipStream_t s);
int reduce_blocks(int K, int traj_per_block);
// config 5: rollout through the residual MLP on MFMA, one record per 64-sample tile.  plan_mlp covers the three forms of
// that launch: the rollout (viz null; `records` per agent), the visualisation rollouts and the batched transition
struct MlpViz;
// fleet: the handle is a learned fleet handle (mppi_config.obstacle_motion = 3): its rollout takes the fleet forms
RolloutPlan plan_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const MlpViz *viz = nullptr, bool fleet = false);
// a learned fleet handle in plan mode: every agent's plan through its own model (k_fleet_plan_mlp_*), in launch_fleet_rows' place
void launch_fleet_plan_mlp(const KParams<float> &P, const MlpParams &Q, const MlpParams *models, const FleetParams &F, hipStream_t s);
void launch_mlp(const RolloutPlan &plan, const KParams<float> &P, const MlpParams &Q, const MlpParams *models, void *partials,
                const MlpViz *viz, hipStream_t s);
// the visualisation rollouts (mppi_differential_drive.py:144-159) with the learned model: opt [T][3], smp [K][T][3] (either
// may be null); u_before / u_upd: the nominal controls before the update and the updated, unshifted ones
void launch_viz_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const float *u_before, const float *u_upd,
                    long long iter, float *opt, float *smp, hipStream_t s);
// `_state_transition` with the learned model for n (state, control) rows: x [n][3], v [n][2] -> out [n][3]
void launch_eval_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const float *x, const float *v, int n,
                     float *out, hipStream_t s);
int mlp_blocks(int K, int tile);            // workgroups = softmin records of a launch over K samples
void pack_linear(const float *w, int n_in, float *packed, int n_out = 512);  // host: [n_out][n_in] -> fragment order
void pack_linear_h3(const float *w, int n_in, unsigned short *packed, int n_out = 512);  // host: -> two f16 planes in fragment order
constexpr int MODEL_DIFF_MLP = 2;

}  // namespace mppi
