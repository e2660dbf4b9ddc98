// C ABI of libmppi_hip.so (include/mppi_hip.h): handle management, parameter packing and
// the launch sequence of one MPPI iteration.  No algorithmic arithmetic happens on the host.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <time.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mppi_hip.h"
#include "mppi_kernels.h"
#include "mppi_owner.h"

using namespace mppi;

static thread_local std::string g_create_error;

static double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// Every environment switch of the library (INTEGRATION.md section 4 lists them and when each is read): the one place that
// looks at the environment.  mppi_create keeps the result in the handle; mppi_set_mlp takes the three learned-dynamics
// switches from a fresh reading and mppi_comm_connect the exchange timeout.
static Switches read_switches() {
    const auto set = [](const char *name) { return getenv(name) != nullptr; };
    const auto num = [](const char *name, int unset) {
        const char *e = getenv(name);
        return e ? atoi(e) : unset;
    };
    const auto on_off = [&](const char *name) { return set(name) ? (int)(num(name, 0) != 0) : -1; };  // -1 unset, else 0 / 1
    Switches sw;
    sw.dual = on_off("MPPI_DUAL");
    sw.pair = on_off("MPPI_PAIR");
    sw.tri = on_off("MPPI_TRI");
    sw.seq = set("MPPI_SEQ") ? (num("MPPI_SEQ", 0) == 2 ? 2 : 1) : -1;
    sw.no_stream = set("MPPI_NO_STREAM");
    sw.stream_passes = num("MPPI_STREAM_PASSES", 0);
    sw.force_unfused = set("MPPI_FORCE_UNFUSED");
    sw.no_hyp = set("MPPI_NO_HYP");
    sw.no_poll = set("MPPI_NO_POLL");
    sw.no_args = set("MPPI_NO_ARGS");
    sw.traj_per_block = num("MPPI_TRAJ_PER_BLOCK", 0);
    sw.graph = on_off("MPPI_GRAPH") == 1;  // (opt-in: see ensure_graph)
    sw.graph_verbose = set("MPPI_GRAPH_VERBOSE");
    sw.graph_slots = std::max(1, num("MPPI_GRAPH_SLOTS", 64));
    sw.mlp.f32 = set("MPPI_MLP_F32");
    sw.mlp.terms = num("MPPI_MLP_TERMS", 3) == 2 ? 2 : 3;
    const char *form = getenv("MPPI_MLP_FORM");
    sw.mlp.form = form && !strcmp(form, "4x64") ? 0 : form && !strcmp(form, "8x64") ? 1 : -1;
    if (const char *e = getenv("MPPI_EXCHANGE_TIMEOUT_MS")) sw.exchange_timeout_ms = atoll(e);
    sw.lb_timeout_ticks = std::max(0, num("MPPI_LB_TIMEOUT_TICKS", (int)LB_TIMEOUT_TICKS));
    return sw;
}

struct RcclUniqueId { char internal[128]; };  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES), passed by value to ncclCommInitRank

struct mppi_handle {
    mppi_config cfg;
    Switches sw;              // the environment as mppi_create found it (sw.mlp: as the last model setter did)
    bool f64 = false;
    int nx = 3, n_ref = 0, n_obs = 0, n_blocks = 0, traj_per_block = 0;
    bool fused = false;       // rollout + softmin partial in one launch (T <= 128)
    int B = 1;                // agents (mppi_config.n_agents); per-agent buffers are B consecutive copies
    int slots = 0;            // records per agent in d_partials / d_heads (the most a launch leaves + zero padding)
    // Everything the runtime hands out is held by an owner (mppi_owner.h) and released by `delete h`, last member first, on the
    // device mppi_destroy selected: a new buffer is a field, nothing else.  The events, the stream and the graph objects stand
    // before the buffers, so they go after them as they always have (the first hipFree waits for the device); the graph
    // executables stand behind the stream and the events their launches use, so they go first of these.
    std::vector<Event> ev;  // pairs around the rollout / reduce / finalize kernels
    size_t ev_used = 0;
    Event ev_step[2];
    // closed-loop iterations replayed from a HIP graph once the waypoint index rests (closed_loop_impl)
    bool graph_on = false;
    std::vector<char> graph_key;      // the kernel arguments the cached graph was captured with
    Stream graph_stream;              // (stream and events: created by the first capture, reused by every later one)
    Event graph_ev_in, graph_ev_out;
    Event graph_done[2];
    GraphExec graph_exec[2];          // two instances, launched in turn (see closed_loop_impl)
    DevBuf<void> d_partials2;       // what a merge launch in front of the reader leaves (merge_tree)
    DevBuf<void> d_heads, d_heads2;  // compact {rho, eta, eta2, 0} of d_partials / d_partials2
    DevBuf<float> d_mlp;            // packed residual-model weights (config 5): the model every agent shares (mppi_set_mlp)
    DevBuf<unsigned short> d_mlp16;  // the same as f16 hi / lo planes (k_rollout_mlp_h3, k_rollout_mlp_w)
    size_t mlp_cap = 0, mlp16_cap = 0;  // their sizes in elements
    // one-launch resolution of the sequential waypoint index (LB_CAND in mppi_kernels.h)
    bool hyp = false;
    DevBuf<unsigned> d_hyp_slots;     // one look-back word per workgroup (LB_COPIES copies)
    unsigned lb_seq = 0;              // tag of the last rollout / finalize launch pair that used them
    std::vector<double> ref_host;   // [n_ref][4] as the kernels see it (rounded to the handle's precision)
    StepResult *res_mapped = nullptr;  // borrowed: device-side address of h_res, the pinned host result (polled completion)
    long long seq = 0;
    bool idx_valid = true;
    int layout = 0;  // rollout_layout(K, T): which fused rollout kernel serves this handle
    const char *rollout_kernel = "";  // borrowed: RolloutPlan::name of the last rollout launch, or of the model mppi_set_mlp loaded (mppi_get_rollout_kernel)
    // The learned model.  mlp_shared / shared_set: the kernels' view of d_mlp / d_mlp16, what mppi_set_mlp loaded for every
    // agent.  Several agents: own_mlp[a] holds what mppi_set_agent_mlp gave agent a instead (a buffer pair it owns, reused
    // while large enough), and d_models is the table the batched kernels read: every agent's view, rewritten by every model
    // setter (model_of, upload_models).  A single-agent handle has neither.  `mlp` -- what a launch carries by value and the
    // planners read -- is agent 0's view; hidden, n_hidden and use_h3 in it are the batch's (one shape per handle).
    MlpParams mlp = {}, mlp_shared = {};
    bool shared_set = false;
    struct OwnModel {  // (move-only; `o = OwnModel{}` releases the pair)
        DevBuf<float> d_mlp;
        DevBuf<unsigned short> d_mlp16;
        size_t cap = 0, cap16 = 0;
        MlpParams q = {};
        bool set = false;
    };
    std::vector<OwnModel> own_mlp;
    DevBuf<MlpParams> d_models;
    DevBuf<void> d_ref, d_obs, d_u, d_uhist, d_S;
    // Several agents: d_ref / n_ref / d_obs / n_obs above are the scene every agent shares (mppi_set_ref_path /
    // mppi_set_obstacles); own[a] holds what mppi_set_agent_ref_path / mppi_set_agent_obstacles gave agent a instead (buffers
    // it owns), and d_scenes is the table the batched kernels read: every agent's view, rewritten by every setter (scene_of,
    // upload_scenes).  A single-agent handle has neither.
    struct OwnScene {  // (move-only)
        DevBuf<void> d_ref, d_obs;
        int n_ref = 0, n_obs = 0;
        bool has_obs = false;  // (an own set of m = 0 circles has no buffer)
        long long obs_iter0 = 0;  // moving obstacles: the agent's iteration counter when its own set was uploaded
        std::vector<double> obs_host;  // fleet handles: the packed rows of d_obs as uploaded ([n_obs] circles, [n_obs] velocities)
    };
    std::vector<OwnScene> own;
    DevBuf<AgentScene> d_scenes;
    long long obs_iter0 = 0;  // moving obstacles (mppi_config.obstacle_motion): the iteration counter when d_obs was uploaded
    // Fleet avoidance (mppi_config.fleet_radius > 0): every agent b owns a table of m_b + B - 1 circle rows and as many velocity
    // rows -- its own circles (the shared set's or its own: written by the host at every setter, build_fleet_tables) followed by its
    // mates' rows, which k_fleet_rows writes at the front of every slot.  scene_of hands these tables to the kernels; d_obs and
    // own[a].d_obs keep what the setters uploaded and are not read by a launch.  d_clear: the agents' clearance records.
    bool fleet = false;
    std::vector<double> obs_host;  // the shared set's packed rows, as OwnScene::obs_host
    std::vector<DevBuf<void>> fleet_tab;
    DevBuf<FleetClear> d_clear;
    // MPPI_FLEET_PLAN (mppi_set_fleet_prediction): the tables hold the own rows alone, k_fleet_plan leads the slots in
    // k_fleet_rows' place and writes d_plans, [B][T + 1][2] in the handle's precision, which the plan rollout forms read
    bool fleet_plan = false;
    DevBuf<void> d_plans;
    // Obstacle tracks (mppi_set_obstacle_tracks): the set every agent shares, what mppi_set_agent_obstacle_tracks gave an agent
    // instead (own_tracks[a], several agents only), and d_tracks, the descriptors the track forms read: every agent's view,
    // rewritten by every setter (tracks_of, upload_tracks) and allocated by the first one.
    struct TrackOwn {  // (move-only)
        DevBuf<void> d_pts, d_thr;  // PlanPoint<R>[n][L], R[n]
        int n = 0, L = 1;
        bool has = false;           // (an own set of n = 0 tracks has no buffer)
        long long iter0 = 0;        // the agent's iteration counter when the set was uploaded
        std::vector<double> radius;  // as given (mppi_get_obstacle_tracks_at)
    };
    TrackOwn tracks;
    std::vector<TrackOwn> own_tracks;
    DevBuf<TrackSet> d_tracks;
    int tracks_max = 0;  // the largest set among the agents, kept by upload_tracks (0: a handle that never had any)
    // Cost grids (mppi_set_cost_grid): the grid every agent shares, what mppi_set_agent_cost_grid gave an agent instead
    // (own_grids[a], several agents only), and d_grids, the descriptors the grid forms read (GridSet<R>[n_agents]): every
    // agent's view, rewritten by every setter (grid_of, upload_grids) and allocated by the first one.
    struct GridOwn {  // (move-only)
        DevBuf<void> d_cells;  // R[ny][nx]
        int nx = 0, ny = 0;    // (0: none)
        bool has = false;      // an agent's own entry stands in place of the shared one (also an own "none")
        double ox = 0, oy = 0, inv = 0, weight = 0, lethal = 0;
    };
    GridOwn grid;
    std::vector<GridOwn> own_grids;
    DevBuf<void> d_grids;
    bool any_grid = false;  // some agent has a grid, kept by upload_grids (false: a handle that never had one, or cleared)
    // mppi_set_cost_grid_footprint: every grid of the handle is priced under the vehicle's outline (MPPI_GRID_FOOTPRINT_OUTLINE).
    // A property of the launch's form: front_plan hands it to the planner, the eval entry points pick their form by it (eval_form).
    int grid_footprint = MPPI_GRID_FOOTPRINT_CENTRE;
    // Composed scenes (mppi_set_scene_mode): in MPPI_SCENE_COMPOSED the three above may stand together, and d_scene is the one
    // SceneTable<R> a launch with two or more of them reads: the addresses of d_plans, d_tracks and d_grids (null: none) and the
    // mates' threshold, rewritten by every setter that changes an ingredient (upload_scene_table), allocated by the first switch
    int scene_mode = MPPI_SCENE_EXCLUSIVE;
    DevBuf<void> d_scene;
    DevBuf<int> d_pout;
    DevBuf<void> d_partials;        // block records in the handle's precision
    DevBuf<double> d_w, d_trace;
    long long trace_cap = 0;
    DevBuf<DevState> d_st;
    DevBuf<StepResult> d_res;
    PinnedBuf<StepResult> h_res;
    size_t res_bytes = 0;
    const float *last_eps = nullptr;    // borrowed: the tensor the last iteration drew its noise from (null: the in-kernel sampler)
    const float *noise_ring = nullptr;  // borrowed: mppi_set_noise_ring: [noise_slots][n_agents][K][T][2] device floats (caller's)
    int noise_slots = 0;
    bool begun = false, timing = false, dev_loop_primed = false, slot_timed = false;
    long long iter = 0;
    int idx = 0, rollout_repeats = 1;
    float last_ms[4] = {0, 0, 0, 0};
    double last_iter_us = 0.0;  // host wall time per iteration of the last step / closed-loop call (mppi_stats::iter_us)
    // peer-to-peer exchange (mppi_comm_*)
    FineBuf<char> xbuf;              // this rank's exchange buffer (fine-grained device memory)
    size_t xbuf_bytes = 0;
    int x_rank = 0, x_nranks = 0, x_export_nranks = 0;
    std::vector<IpcMap> x_opened;    // peers' buffers mapped through IPC handles
    DevBuf<char *> d_xpeers;         // device array [x_nranks]
    DevBuf<int> d_xerr, d_xok;
    long long xseq = 0, x_timeout = 300000000LL;
    // RCCL carrier inside the library (mppi_comm_init): communicator, this rank's record and the gathered records
    void *rccl_comm = nullptr;  // (released through the dlopen'ed API: rccl_release)
    int rccl_rank = 0, rccl_nranks = 0;
    DevBuf<double> d_rccl_part, d_rccl_gath;
    long long n_rollout_launches = 0, n_finalize_launches = 0;  // mppi_get_counters
    double t_enqueue_s = 0.0, t_loop_s = 0.0;  // mppi_get_host_timing: closed-loop calls, enqueueing / whole call
    std::string err;
};

#define FAIL(h, code, ...)                                   \
    do {                                                     \
        char _b[512];                                        \
        snprintf(_b, sizeof(_b), __VA_ARGS__);               \
        if (h) (h)->err = _b; else g_create_error = _b;      \
        return (code);                                       \
    } while (0)
#define CREATE_FAIL(code, ...) FAIL((mppi_handle *)nullptr, code, __VA_ARGS__)  // (before there is a handle)

#define HIPCHECK(h, call)                                                                          \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) FAIL(h, MPPI_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
    } while (0)

extern "C" int mppi_abi_version(void) { return MPPI_ABI_VERSION; }

extern "C" const char *mppi_last_error(const mppi_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" int mppi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The one precision dispatch: f is called with float{} or double{}, the handle's real type (`using R = decltype(r)`).  Every
// entry point that launches goes through it once per ABI call; below it everything is a template on R.
template <typename Fn> static auto with_real(const mppi_handle *h, Fn &&f) { return h->f64 ? f(double{}) : f(float{}); }

static size_t rsz(const mppi_handle *h) { return with_real(h, [](auto r) { return sizeof(r); }); }

// ABI model -> the kernels' model (the learned model rolls the diff-drive state)
static int kernel_model(const mppi_config &c) { return c.model == MPPI_MODEL_RACECAR ? MODEL_RACE : MODEL_DIFF; }
// the softmin rate
static double softmin_beta(const mppi_config &c) {
    return c.beta_mode == MPPI_BETA_INV_EXPLORATION ? 1.0 / c.param_exploration
           : c.beta_mode == MPPI_BETA_INV_LAMBDA    ? 1.0 / c.param_lambda
                                                    : c.param_lambda;
}
// The sequential index only grows: once it sits on the last waypoint every search window holds one candidate and nothing
// can move.  index_can_move: the handle runs the kernels that resolve the index in one launch, and it has not got there.
static bool at_path_end(const mppi_handle *h, int idx) { return idx >= h->n_ref - 1; }  // (sequential index: one agent)
// Agent a's scene: what it was given for itself, else the shared one.  n_obs counts only where the handle tests collisions.
static AgentScene scene_of(const mppi_handle *h, int a) {
    AgentScene sc = {h->d_ref, h->d_obs, h->n_ref, h->n_obs, h->obs_iter0};
    if (a < (int)h->own.size()) {
        const mppi_handle::OwnScene &o = h->own[a];
        if (o.d_ref) sc.ref = o.d_ref, sc.n_ref = o.n_ref;
        if (o.has_obs) sc.obs = o.d_obs, sc.n_obs = o.n_obs, sc.iter0 = o.obs_iter0;
    }
    if (h->cfg.obstacle_model == MPPI_OBSTACLE_NONE) sc.n_obs = 0;
    // (its own rows first, then one per mate: build_fleet_tables; plan mode: the own rows alone, the mates come from d_plans)
    if (h->fleet) sc.obs = h->fleet_tab[a], sc.n_obs += h->fleet_plan ? 0 : h->B - 1;
    return sc;
}
// Agent a's obstacle tracks: what it was given for itself, else the shared set
static const mppi_handle::TrackOwn &tracks_of(const mppi_handle *h, int a) {
    return a < (int)h->own_tracks.size() && h->own_tracks[a].has ? h->own_tracks[a] : h->tracks;
}
// the largest track set among the agents (0: no agent has tracks and the handle is one that never had any); a field, so that
// the per-iteration parameter packing of a handle without tracks does what it did
static int max_tracks(const mppi_handle *h) { return h->tracks_max; }
// Agent a's cost grid: what it was given for itself, else the shared one
static const mppi_handle::GridOwn &grid_of(const mppi_handle *h, int a) {
    return a < (int)h->own_grids.size() && h->own_grids[a].has ? h->own_grids[a] : h->grid;
}
// composed scenes: how many of {plan mode, tracks on some agent, a grid on some agent} the handle holds; two or more run the
// composed rollout form behind the SceneTable, fewer the single-ingredient forms with their own carriers
static bool scene_composed(const mppi_handle *h) { return h->scene_mode == MPPI_SCENE_COMPOSED; }
static int scene_ingredients(const mppi_handle *h) { return (h->fleet_plan ? 1 : 0) + (max_tracks(h) > 0 ? 1 : 0) + (h->any_grid ? 1 : 0); }
static bool scene_form(const mppi_handle *h) { return scene_composed(h) && scene_ingredients(h) >= 2; }
// the learned model's scene handle (mppi_config.obstacle_motion = 2): every launch carries the SceneTable (set_scene_learned)
static bool learned_scene(const mppi_handle *h) { return h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP && h->cfg.obstacle_motion >= 2; }
// its fleet handle (obstacle_motion = 3, MPPI_OBSTACLE_MOTION_LEARNED_FLEET): a scene handle whose agents see each other -- the
// fleet forms of the batched scene kernels, and in plan mode the plans rolled out through every agent's own model
static bool learned_fleet(const mppi_handle *h) { return h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP && h->cfg.obstacle_motion == 3; }
// the create-time value a handle of this model needs for a scene, as the setters' refusals name it
static int motion_value(const mppi_handle *h) { return h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP ? 2 : 1; }
// some agent has obstacles: the obstacle instantiations serve and the records carry collision counts
static bool any_obstacles(const mppi_handle *h) {
    if (max_tracks(h) > 0) return true;  // (tracks stand in no circle table: a handle may have tracks and no circles)
    if (h->any_grid) return true;        // (nor does a grid)
    if (h->fleet) return true;  // (the mates: rows of every table, or -- plan mode, where an agent may have n_obs = 0 -- their plans)
    for (int a = 0; a < h->B; ++a)
        if (scene_of(h, a).n_obs > 0) return true;
    return false;
}
// The sequential index in one launch (look-back, LB_CAND in mppi_kernels.h) serves this handle: horizons of one 64-step pass
// in the one-sample-per-wave layout or the two-samples-per-wave layout with one pass per workgroup, the reference's 20- / 10-
// candidate windows, `S[k] =`, one agent, at most 512 workgroups = records (K <= 16384: configs 2 and 3).  Anything else keeps
// the speculation rounds alone (they also serve as this path's fallback).  MPPI_NO_HYP=1 switches it off for A/B runs.
// The one place that decides it: KParams::hyp carries it (while the index can move) to the rollout planners, and what they
// picked comes back as RolloutPlan::lookback.
static bool lookback_serves(const mppi_handle *h, int records) {
    const mppi_config &c = h->cfg;
    const bool lb_layout = (h->layout & LAYOUT_KIND) == LAYOUT_FUSED || h->layout == LAYOUT_DUAL;  // (one pass per workgroup)
    return h->fused && lb_layout && c.T <= 64 && c.model == MPPI_MODEL_DIFFDRIVE && c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL &&
           !c.accumulate_stage_cost && (c.search_window == HYP_WINDOW || c.search_window == HYP_WINDOW_CUDA) && c.n_agents == 1 &&
           records <= HYP_MAX_BLOCKS && !h->sw.no_hyp &&
           !c.obstacle_motion;  // (the look-back prices the last state with a collision test of its own: static circles only)
}
static bool index_can_move(const mppi_handle *h) { return h->hyp && !(h->idx_valid && h->n_ref > 0 && at_path_end(h, h->idx)); }
template <typename R> static KParams<R> make_params(const mppi_handle *h, const float *eps);
template <typename R> static RolloutPlan front_plan(const mppi_handle *h, const KParams<R> &P);
static int upload_scenes(mppi_handle *h);
static int upload_tracks(mppi_handle *h);
static int upload_grids(mppi_handle *h);
static int upload_scene_table(mppi_handle *h);
static void drop_graph(mppi_handle *h);
static int build_fleet_tables(mppi_handle *h, int only);

// host double[] -> device array in the kernel precision
static int upload_real(mppi_handle *h, void *dst, const double *src, size_t n) {
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        const std::vector<R> tmp(src, src + n);
        HIPCHECK(h, hipMemcpy(dst, tmp.data(), n * sizeof(R), hipMemcpyHostToDevice));
        return MPPI_OK;
    });
}

static int download_real(mppi_handle *h, double *dst, const void *src, size_t n) {
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        std::vector<R> tmp(n);
        HIPCHECK(h, hipMemcpy(tmp.data(), src, n * sizeof(R), hipMemcpyDeviceToHost));
        std::copy(tmp.begin(), tmp.end(), dst);
        return MPPI_OK;
    });
}

extern "C" int mppi_create(const mppi_config *cfg, mppi_handle **out) {
    if (!cfg || !out) CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(mppi_config))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: struct_size %d != %zu (ABI mismatch)", cfg->struct_size, sizeof(mppi_config));
    mppi_config c = *cfg;
    const Switches sw = read_switches();
    if (c.K_global == 0) c.K_global = c.K;
    if (c.K > (1 << 20) || c.T > 2048)
        CREATE_FAIL(MPPI_ERR_SHAPE, "K=%d / T=%d beyond the supported 2^20 samples / 2048 steps", c.K, c.T);
    if (c.K < 1 || c.T < 1 || c.K_global < c.K || c.k_offset < 0 || c.k_offset + c.K > c.K_global)
        CREATE_FAIL(MPPI_ERR_SHAPE, "mppi_create: bad K=%d T=%d K_global=%d k_offset=%d", c.K, c.T, c.K_global, c.k_offset);
    if (c.model != MPPI_MODEL_DIFFDRIVE && c.model != MPPI_MODEL_RACECAR && c.model != MPPI_MODEL_DIFFDRIVE_MLP)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: unknown model %d", c.model);
    if (c.model == MPPI_MODEL_DIFFDRIVE_MLP && c.precision != MPPI_PREC_F32)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "the learned-dynamics rollout runs on the f32 MFMA path only");
    if (c.precision != MPPI_PREC_F32 && c.precision != MPPI_PREC_F64)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: unknown precision %d", c.precision);
    if (c.waypoint_mode != MPPI_WAYPOINT_SEQUENTIAL && c.waypoint_mode != MPPI_WAYPOINT_FROZEN && c.waypoint_mode != MPPI_WAYPOINT_PER_ROLLOUT)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: unknown waypoint_mode %d", c.waypoint_mode);
    if (c.waypoint_mode == MPPI_WAYPOINT_PER_ROLLOUT && c.model == MPPI_MODEL_RACECAR)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED,
             "MPPI_WAYPOINT_PER_ROLLOUT restates the diff-drive files' index bookkeeping (mppi_differential_drive.py:228,:244); "
             "the race-car files search from the x0 call's index (MPPI_WAYPOINT_FROZEN)");
    // (2, MPPI_OBSTACLE_MOTION_LEARNED: the learned model's scene handle -- inside the library it is value 1 everywhere)
    // (3, MPPI_OBSTACLE_MOTION_LEARNED_FLEET: a scene handle whose agents see each other -- likewise)
    const bool fleet_handle = c.obstacle_motion == 3 && c.model == MPPI_MODEL_DIFFDRIVE_MLP;
    const bool scene_handle = (c.obstacle_motion == 2 && c.model == MPPI_MODEL_DIFFDRIVE_MLP) || fleet_handle;
    if (c.obstacle_motion != 0 && c.obstacle_motion != 1 && !scene_handle)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: obstacle_motion %d is neither 0 (static) nor 1 (constant velocity)%s", c.obstacle_motion,
                    c.obstacle_motion == 2   ? "; 2 (the learned model's scene handle) goes with MPPI_MODEL_DIFFDRIVE_MLP only"
                    : c.obstacle_motion == 3 ? "; 3 (the learned model's fleet handle) goes with MPPI_MODEL_DIFFDRIVE_MLP only (limit: an "
                                               "analytic fleet is obstacle_motion = 1 with fleet_radius > 0)"
                                             : "");
    if (fleet_handle && !(c.fleet_radius > 0) && std::isfinite(c.fleet_radius))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: obstacle_motion = 3 (the learned model's fleet handle) needs fleet_radius > 0, got %g "
                                      "(limit: without a fleet the scene handle is obstacle_motion = 2)", c.fleet_radius);
    if (fleet_handle && c.n_agents < 2)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: obstacle_motion = 3 (the learned model's fleet handle) needs n_agents >= 2 (an agent's "
                                      "mates are the other agents of its handle), got %d", c.n_agents);
    if (c.obstacle_motion && c.obstacle_model == MPPI_OBSTACLE_NONE)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: obstacle_motion = %d needs an obstacle model (MPPI_OBSTACLE_CIRCLE or _OUTLINE), got MPPI_OBSTACLE_NONE", c.obstacle_motion);
    if (c.obstacle_motion == 1 && c.model == MPPI_MODEL_DIFFDRIVE_MLP)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "moving obstacles (obstacle_motion = 1) are served by the analytic models only: the "
                                          "learned-dynamics rollout (MPPI_MODEL_DIFFDRIVE_MLP) tests static circles; its scene "
                                          "handle is obstacle_motion = 2 (moving circles, obstacle tracks and cost grids)");
    if (scene_handle && !fleet_handle && c.fleet_radius > 0)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "fleet avoidance (fleet_radius = %g) on an obstacle_motion = 2 handle is served by the analytic "
                                          "models only: the mates' plans are rolled out with analytic dynamics (limit: fleet_radius = 0 "
                                          "with obstacle_motion = 2; a learned-dynamics fleet is obstacle_motion = 3)", c.fleet_radius);
    if (scene_handle && c.K_global != c.K)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "a learned-dynamics scene handle (obstacle_motion = %d) is not sharded (limit: K_global = K, "
                                          "got K = %d, K_global = %d)", c.obstacle_motion, c.K, c.K_global);
    if (!(c.fleet_radius >= 0) || !std::isfinite(c.fleet_radius))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: fleet_radius %g is not a finite radius >= 0 (0: fleet avoidance off)", c.fleet_radius);
    if (c.fleet_radius > 0 && c.n_agents < 2)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: fleet_radius > 0 needs n_agents >= 2 (an agent's mates are the other agents of its handle), got %d", c.n_agents);
    if (c.fleet_radius > 0 && !c.obstacle_motion)
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: fleet_radius > 0 needs obstacle_motion = 1 (the mates are moving circles)");
    if (c.fleet_radius > 0 && c.n_agents > 256)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "fleet avoidance serves at most 256 agents per handle (n_agents = %d): every agent tests every other", c.n_agents);
    if (c.filter_window < 1) c.filter_window = 10;
    if (c.search_window < 1) CREATE_FAIL(MPPI_ERR_BAD_ARG, "mppi_create: search_window must be >= 1");
    // the reference's filters fail on short horizons (np.convolve 'same' returns max(M, N) samples)
    if (c.filter_mode == MPPI_FILTER_DIFFDRIVE && c.T < c.filter_window)
        CREATE_FAIL(MPPI_ERR_SHAPE, "horizon T=%d is shorter than the moving-average window %d", c.T, c.filter_window);
    // (the padded variants copy the last -(-window // 2) = (window + 1) / 2 rows, mppi_race_car.py:219)
    if ((c.filter_mode == MPPI_FILTER_RACECAR || c.filter_mode == MPPI_FILTER_TORCH) && c.T < (c.filter_window + 1) / 2)
        CREATE_FAIL(MPPI_ERR_SHAPE, "horizon T=%d is shorter than half the filter window %d (rounded up)", c.T, c.filter_window);
    if (c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL && c.K_global != c.K)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED,
             "the sequential waypoint index threads through all samples in order and cannot be sharded; "
             "use MPPI_WAYPOINT_PER_ROLLOUT or MPPI_WAYPOINT_FROZEN with K_global > K");
    if (c.n_agents < 1) c.n_agents = 1;
    if (c.n_agents > 1) {
        if (c.n_agents > 4096) CREATE_FAIL(MPPI_ERR_SHAPE, "mppi_create: n_agents %d > 4096", c.n_agents);
        if (c.model == MPPI_MODEL_DIFFDRIVE_MLP) {
            // one learned model for every agent: k_rollout_mlp_h3_agents / k_rollout_mlp_w_agents, one 64-sample tile per
            // workgroup and agent; at most the 512 records per agent k_finalize merges itself (k_merge is not agent-aware)
            if (c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL || c.K_global != c.K || merge_tree(mlp_blocks(c.K, 64), true).group)
                CREATE_FAIL(MPPI_ERR_UNSUPPORTED,
                     "several agents per learned-dynamics handle need MPPI_WAYPOINT_FROZEN or _PER_ROLLOUT, at most 512 rollout "
                     "workgroups of 64 samples per agent (K <= 32768) and no sharding (got K = %d, K_global = %d)", c.K, c.K_global);
        } else if (c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL || c.K_global != c.K || !fused_supported(c.T) ||
                   merge_tree(fused_blocks(c.K, c.T, rollout_layout(sw, c.K, c.T, c.n_agents, kernel_model(c), c.precision == MPPI_PREC_F64, c.waypoint_mode == MPPI_WAYPOINT_PER_ROLLOUT, false, c.obstacle_motion != 0)), true).group) {
            CREATE_FAIL(MPPI_ERR_UNSUPPORTED,
                 "several agents per handle need MPPI_WAYPOINT_FROZEN or _PER_ROLLOUT, T <= 128, at most 512 rollout workgroups "
                 "(K <= 8192) and no sharding");
        }
    }
    const double det = c.sigma[0] * c.sigma[3] - c.sigma[1] * c.sigma[2];
    if (!(c.sigma[0] > 0) || !(det > 0))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "sigma must be a symmetric positive definite 2x2 matrix");
    if (!(c.param_exploration >= 0) || !(c.param_lambda > 0))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "param_exploration must be >= 0 and param_lambda > 0");
    if (c.beta_mode == MPPI_BETA_INV_EXPLORATION && !(c.param_exploration > 0))
        CREATE_FAIL(MPPI_ERR_BAD_ARG, "beta = 1/param_exploration needs param_exploration > 0");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        CREATE_FAIL(MPPI_ERR_NO_DEVICE, "no HIP device is visible: libmppi_hip.so needs an MI355X");
    if (c.device < 0 || c.device >= ndev)
        CREATE_FAIL(MPPI_ERR_NO_DEVICE, "device %d out of range (%d visible)", c.device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) CREATE_FAIL(MPPI_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        CREATE_FAIL(MPPI_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", c.device, prop.gcnArchName);

    if (c.n_agents > 1 && c.model != MPPI_MODEL_DIFFDRIVE_MLP && sw.force_unfused)
        CREATE_FAIL(MPPI_ERR_UNSUPPORTED, "several agents per handle need the fused rollout kernels");
    mppi_handle *h = new mppi_handle();
    h->cfg = c;
    h->sw = sw;
    h->f64 = c.precision == MPPI_PREC_F64;
    h->nx = c.model == MPPI_MODEL_RACECAR ? 4 : 3;
    int tpb = sw.traj_per_block;
    if (tpb < 1) tpb = (c.K + 127) / 128;
    tpb = ((tpb + 3) / 4) * 4;
    if (tpb > 2048) tpb = 2048;
    h->traj_per_block = tpb;
    h->n_blocks = reduce_blocks(c.K, tpb);
    h->fused = fused_supported(c.T) && !sw.force_unfused;
    h->graph_on = sw.graph;
    // (k_rollout_tri: the race car as the reference runs it -- frozen index, `S[k] +=` -- one agent, f32)
    const bool tri_ok = c.model == MPPI_MODEL_RACECAR && !h->f64 && c.n_agents == 1 && c.waypoint_mode == MPPI_WAYPOINT_FROZEN &&
                        c.accumulate_stage_cost;
    h->layout = rollout_layout(sw, c.K, c.T, c.n_agents, kernel_model(c), h->f64, c.waypoint_mode == MPPI_WAYPOINT_PER_ROLLOUT, tri_ok, c.obstacle_motion != 0);
    h->B = c.n_agents;
    // records per agent of this handle's own rollout launch: its plan's count (every learned-dynamics kernel leaves the same)
    const int n_part = with_real(h, [&](auto r) { return front_plan<decltype(r)>(h, make_params<decltype(r)>(h, nullptr)).records; });
    h->res_bytes = sizeof(StepResult) + sizeof(double) * 2 * c.T;
    auto fail = [&](hipError_t e, const char *what) {
        g_create_error = std::string(what) + " failed: " + hipGetErrorString(e);
        mppi_destroy(h);
        return (int)MPPI_ERR_HIP;
    };
    // a device buffer, allocated and zero-filled; a failure names the call that failed
    const auto zeroed = [&](auto &buf, size_t bytes, const char *malloc_call) -> int {
        hipError_t e;
        if ((e = buf.alloc(bytes)) != hipSuccess) return fail(e, malloc_call);
        if ((e = hipMemset(buf, 0, bytes)) != hipSuccess) return fail(e, "hipMemset");
        return MPPI_OK;
    };
    hipError_t e;
    if ((e = hipSetDevice(c.device)) != hipSuccess) return fail(e, "hipSetDevice");
    const size_t r = rsz(h), B = (size_t)c.n_agents;
    if (int rc = zeroed(h->d_u, B * r * 2 * c.T, "hipMalloc(u)")) return rc;  // u_prev = 0 (:82)
    if (int rc = zeroed(h->d_uhist, B * r * 4 * c.T, "hipMalloc(u history)")) return rc;
    if (int rc = zeroed(h->d_S, B * r * c.K, "hipMalloc(S)")) return rc;
    if (int rc = zeroed(h->d_pout, B * sizeof(int) * c.K, "hipMalloc(pout)")) return rc;
    const size_t rec_bytes = sizeof(double) * (size_t)record_len(c.T, 8);  // enough for either precision
    // zero-filled and padded by 256 records: the merge kernels read 256 slots unconditionally
    // (a launch may leave more records than the handle's own count -- fused_max_records: room for the larger of the two)
    const size_t n_rec_max = (size_t)std::max(n_part, fused_max_records(c.K, c.T, h->layout));
    // (the second level: a merge launch leaves at most one window, and only more records than a window are ever merged)
    const size_t slots = n_rec_max + 256, n1 = B * slots, n2 = (merge_tree((int)n_rec_max, false).group ? MERGE_MAX_RECORDS : 0) + 256;
    h->slots = (int)slots;
    if (int rc = zeroed(h->d_partials, rec_bytes * n1, "hipMalloc(partials)")) return rc;
    if (int rc = zeroed(h->d_partials2, rec_bytes * n2, "hipMalloc(partials2)")) return rc;
    if (int rc = zeroed(h->d_heads, 32 * n1, "hipMalloc(heads)")) return rc;
    if (int rc = zeroed(h->d_heads2, 32 * n2, "hipMalloc(heads2)")) return rc;
    h->hyp = lookback_serves(h, n_part);
    if (h->hyp)
        if (int rc = zeroed(h->d_hyp_slots, sizeof(unsigned) * (size_t)LB_COPIES * LB_COPY_STRIDE, "hipMalloc(look-back words)")) return rc;
    h->res_bytes = (h->res_bytes + 15) & ~(size_t)15;  // (the agents' results are stored back to back)
    if ((e = h->d_st.alloc(B * sizeof(DevState))) != hipSuccess) return fail(e, "hipMalloc(state)");  // (filled below)
    if (int rc = zeroed(h->d_res, B * h->res_bytes, "hipMalloc(result)")) return rc;
    if ((e = h->h_res.alloc(B * h->res_bytes)) != hipSuccess) return fail(e, "hipHostMalloc(result)");
    if ((e = hipHostGetDevicePointer((void **)&h->res_mapped, h->h_res, 0)) != hipSuccess)
        return fail(e, "hipHostGetDevicePointer(result)");
    if (B > 1) {
        h->own.resize(B);
        if (int rc = zeroed(h->d_scenes, B * sizeof(AgentScene), "hipMalloc(agent scenes)")) return rc;
        if (c.model == MPPI_MODEL_DIFFDRIVE_MLP) {
            h->own_mlp.resize(B);
            if (int rc = zeroed(h->d_models, B * sizeof(MlpParams), "hipMalloc(agent models)")) return rc;
        }
    }
    if (c.fleet_radius > 0) {
        h->fleet = true;
        h->fleet_tab.resize(B);
        if ((e = h->d_clear.alloc(B * sizeof(FleetClear))) != hipSuccess) return fail(e, "hipMalloc(fleet clearance)");
        const std::vector<FleetClear> none(B, FleetClear{INFINITY, 0});
        if ((e = hipMemcpy(h->d_clear, none.data(), B * sizeof(FleetClear), hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
        if (build_fleet_tables(h, -1) != MPPI_OK || upload_scenes(h) != MPPI_OK) {  // (no own circles yet: the mates' rows alone)
            g_create_error = h->err;
            mppi_destroy(h);
            return MPPI_ERR_HIP;
        }
    }
    if (scene_handle) {  // every launch of such a handle reads the table (make_params): all null until a setter fills it
        if (int rc = zeroed(h->d_scene, sizeof(SceneTable<double>), "hipMalloc(scene table)")) return rc;
        if (upload_scene_table(h) != MPPI_OK) {
            g_create_error = h->err;
            mppi_destroy(h);
            return MPPI_ERR_HIP;
        }
    }
    DevState st0;
    memset(&st0, 0, sizeof(st0));  // prev_way_point_idx = 0 (:85)
    st0.first_k = NO_TRIGGER;
    for (size_t a = 0; a < B; ++a)
        if ((e = hipMemcpy(h->d_st + a, &st0, sizeof(st0), hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    memset(h->h_res, 0, B * h->res_bytes);
    if ((e = hipEventCreate(h->ev_step[0].put())) != hipSuccess) return fail(e, "hipEventCreate");
    if ((e = hipEventCreate(h->ev_step[1].put())) != hipSuccess) return fail(e, "hipEventCreate");
    *out = h;
    return MPPI_OK;
}

extern "C" int mppi_comm_close(mppi_handle *h);

extern "C" int mppi_destroy(mppi_handle *h) {
    if (!h) return MPPI_OK;
    hipSetDevice(h->cfg.device);
    if (h->xbuf || h->rccl_comm) mppi_comm_close(h);
    delete h;
    return MPPI_OK;
}

// Fleet handles: agent `only`'s table (-1: every agent's) made again from the host's copy of its own rows -- m_b circle rows,
// B - 1 mate rows, the same of velocities -- with the mate rows zero (a threshold of 0 collides with nothing) until
// k_fleet_rows writes them.  The caller has synchronised the device and uploads the scenes afterwards.
static int build_fleet_tables(mppi_handle *h, int only) {
    for (int a = 0; h->fleet && a < h->B; ++a) {
        if (only >= 0 && a != only) continue;
        const mppi_handle::OwnScene &o = h->own[a];
        const int m = o.has_obs ? o.n_obs : h->n_obs, n = m + (h->fleet_plan ? 0 : h->B - 1);
        const std::vector<double> &src = o.has_obs ? o.obs_host : h->obs_host;
        std::vector<double> rows((size_t)8 * n, 0.0);
        if (src.size() == (size_t)8 * m) {
            std::copy(src.begin(), src.begin() + 4 * (size_t)m, rows.begin());
            std::copy(src.begin() + 4 * (size_t)m, src.end(), rows.begin() + 4 * (size_t)n);
        } else if (m > 0) {
            FAIL(h, MPPI_ERR_STATE, "fleet table of agent %d: the host copy of its %d circles is missing", a, m);
        }
        HIPCHECK(h, h->fleet_tab[a].reset());
        if (n == 0) continue;  // (plan mode, no own circles: no table, n_obs = 0)
        HIPCHECK(h, h->fleet_tab[a].alloc(rsz(h) * rows.size()));
        if (int rc = upload_real(h, h->fleet_tab[a], rows.data(), rows.size())) return rc;
    }
    return MPPI_OK;
}
// The batched kernels' table (AgentScene[n_agents]), rewritten from the host's view of every agent (the caller has synchronised
// the device).  The table is read at run time, so a cached graph (ensure_graph) replays the new scenes; what a launch carries
// by value -- agent 0's scene and the "any agent has obstacles" decisions in KParams / FinalizeParams -- is part of the graph's key.
static int upload_scenes(mppi_handle *h) {
    if (!h->d_scenes) return MPPI_OK;
    std::vector<AgentScene> tab(h->B);
    for (int a = 0; a < h->B; ++a) tab[a] = scene_of(h, a);
    HIPCHECK(h, hipMemcpy(h->d_scenes, tab.data(), sizeof(AgentScene) * tab.size(), hipMemcpyHostToDevice));
    return MPPI_OK;
}

// `self.ref_path` into *d_ref / *n_ref (the shared scene's or one agent's): validated, packed to [n][4], the device idle before
// the old buffer goes; host_copy (nullable): the packed path as the kernels see it
static int set_path(mppi_handle *h, const char *who, const double *path, int32_t n, int32_t ncols, DevBuf<void> *d_ref,
                    int *n_ref, std::vector<double> *host_copy) {
    if (!path) FAIL(h, MPPI_ERR_BAD_ARG, "%s: null argument", who);
    const int need = h->cfg.model == MPPI_MODEL_RACECAR ? 4 : 3;
    if (n < 1 || ncols < need || ncols > 4)
        FAIL(h, MPPI_ERR_SHAPE, "ref_path must be [n>=1, %d] (got [%d, %d])", need, n, ncols);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    std::vector<double> packed((size_t)n * 4, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < ncols; ++j) packed[(size_t)i * 4 + j] = path[(size_t)i * ncols + j];
    HIPCHECK(h, hipDeviceSynchronize());
    *n_ref = 0;
    HIPCHECK(h, d_ref->reset());
    HIPCHECK(h, d_ref->alloc(rsz(h) * 4 * n));
    *n_ref = n;
    h->dev_loop_primed = false;
    if (host_copy) {
        *host_copy = packed;
        if (!h->f64)
            for (double &v : *host_copy) v = (double)(float)v;
    }
    return upload_real(h, *d_ref, packed.data(), packed.size());
}

// `self.obstacle_circles` into *d_obs / *n_obs, likewise.  A handle with obstacle_motion: the velocity rows {vx, vy, 0, 0}
// follow the m circle rows (vel null: zeros) and *iter0 receives agent `clock_agent`'s iteration counter as of now.
// Everything that can refuse the arguments stands before the first change.
static int set_circles(mppi_handle *h, const char *who, const double *xyr, const double *vel, int32_t m, DevBuf<void> *d_obs,
                       int *n_obs, long long *iter0, int clock_agent, std::vector<double> *host_copy) {
    if (m > 0 && !xyr) FAIL(h, MPPI_ERR_BAD_ARG, "%s: null argument", who);
    if (m < 0) FAIL(h, MPPI_ERR_SHAPE, "%s: m < 0", who);
    const bool moving = h->cfg.obstacle_motion != 0;
    for (int i = 0; vel && i < 2 * m; ++i)
        if (!std::isfinite(vel[i]))
            FAIL(h, MPPI_ERR_BAD_ARG, "%s: the velocity of circle %d is not finite (a moving circle needs finite vx, vy)", who, i / 2);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    long long now = 0;
    if (moving) HIPCHECK(h, hipMemcpy(&now, &h->d_st[clock_agent].iter, sizeof(now), hipMemcpyDeviceToHost));
    HIPCHECK(h, d_obs->reset());
    *n_obs = m;
    *iter0 = now;
    host_copy->clear();
    if (m == 0) return MPPI_OK;
    std::vector<double> packed((size_t)m * (moving ? 8 : 4), 0.0);
    for (int i = 0; moving && vel && i < m; ++i) {
        packed[4 * (size_t)(m + i)] = vel[2 * i];
        packed[4 * (size_t)(m + i) + 1] = vel[2 * i + 1];
    }
    for (int i = 0; i < m; ++i) {
        const double r = xyr[3 * i + 2];
        // mppi_differential_drive_obs.py:304-311: (0.5*margin + r)^2 ; mppi_race_car_obstacle.py:272: r^2
        const double thr = h->cfg.obstacle_model == MPPI_OBSTACLE_CIRCLE ? 0.5 * h->cfg.safety_margin + r : r;
        packed[4 * i] = xyr[3 * i];
        packed[4 * i + 1] = xyr[3 * i + 1];
        packed[4 * i + 2] = thr * thr;
    }
    HIPCHECK(h, d_obs->alloc(rsz(h) * packed.size()));
    if (h->fleet) *host_copy = packed;  // (what build_fleet_tables copies into the agents' tables)
    return upload_real(h, *d_obs, packed.data(), packed.size());
}

extern "C" int mppi_set_ref_path(mppi_handle *h, const double *path, int32_t n, int32_t ncols) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (int rc = set_path(h, "mppi_set_ref_path", path, n, ncols, &h->d_ref, &h->n_ref, &h->ref_host)) return rc;
    for (mppi_handle::OwnScene &o : h->own) {  // several agents: every agent follows this path again
        o.n_ref = 0;
        HIPCHECK(h, o.d_ref.reset());
    }
    return upload_scenes(h);
}

static int set_shared_circles(mppi_handle *h, const char *who, const double *xyr, const double *vel, int32_t m) {
    if (int rc = set_circles(h, who, xyr, vel, m, &h->d_obs, &h->n_obs, &h->obs_iter0, 0, &h->obs_host)) return rc;
    for (mppi_handle::OwnScene &o : h->own) {
        o.n_obs = 0;
        o.has_obs = false;
        o.obs_host.clear();
        HIPCHECK(h, o.d_obs.reset());
    }
    if (int rc = build_fleet_tables(h, -1)) return rc;
    return upload_scenes(h);
}
static int set_agent_circles(mppi_handle *h, const char *who, int32_t agent, const double *xyr, const double *vel, int32_t m) {
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "%s: agent %d not in [0, %d)", who, agent, h->B);
    if (h->B == 1) return set_shared_circles(h, who, xyr, vel, m);
    mppi_handle::OwnScene &o = h->own[agent];
    h->dev_loop_primed = false;
    const int rc = set_circles(h, who, xyr, vel, m, &o.d_obs, &o.n_obs, &o.obs_iter0, agent, &o.obs_host);
    if (rc == MPPI_OK || rc == MPPI_ERR_HIP) o.has_obs = rc == MPPI_OK;  // (refused arguments change nothing)
    if (rc == MPPI_OK || rc == MPPI_ERR_HIP)
        if (int rc2 = build_fleet_tables(h, agent)) return rc ? rc : rc2;
    if (int rc2 = upload_scenes(h)) return rc ? rc : rc2;
    return rc;
}
#define NEEDS_MOTION(h, who)                                                                                            \
    if (!(h)->cfg.obstacle_motion)                                                                                      \
        FAIL(h, MPPI_ERR_STATE, "%s: the handle was created with obstacle_motion = 0 (static circles: mppi_set_obstacles); " \
                                "moving circles need mppi_config.obstacle_motion = %d at mppi_create", who, motion_value(h))

extern "C" int mppi_set_obstacles(mppi_handle *h, const double *xyr, int32_t m) {
    if (!h) return MPPI_ERR_BAD_ARG;
    return set_shared_circles(h, "mppi_set_obstacles", xyr, nullptr, m);
}
extern "C" int mppi_set_obstacles_moving(mppi_handle *h, const double *xyr, const double *vel, int32_t m) {
    if (!h) return MPPI_ERR_BAD_ARG;
    NEEDS_MOTION(h, "mppi_set_obstacles_moving");
    if (m > 0 && !vel) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_obstacles_moving: null argument");
    return set_shared_circles(h, "mppi_set_obstacles_moving", xyr, vel, m);
}

extern "C" int mppi_set_agent_ref_path(mppi_handle *h, int32_t agent, const double *path, int32_t n, int32_t ncols) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_ref_path: agent %d not in [0, %d)", agent, h->B);
    if (h->B == 1) return mppi_set_ref_path(h, path, n, ncols);
    mppi_handle::OwnScene &o = h->own[agent];
    if (int rc = set_path(h, "mppi_set_agent_ref_path", path, n, ncols, &o.d_ref, &o.n_ref, nullptr)) {
        (void)upload_scenes(h);  // (a failed allocation left the agent on the shared path)
        return rc;
    }
    return upload_scenes(h);
}

extern "C" int mppi_set_agent_obstacles(mppi_handle *h, int32_t agent, const double *xyr, int32_t m) {
    if (!h) return MPPI_ERR_BAD_ARG;
    return set_agent_circles(h, "mppi_set_agent_obstacles", agent, xyr, nullptr, m);
}
extern "C" int mppi_set_agent_obstacles_moving(mppi_handle *h, int32_t agent, const double *xyr, const double *vel, int32_t m) {
    if (!h) return MPPI_ERR_BAD_ARG;
    NEEDS_MOTION(h, "mppi_set_agent_obstacles_moving");
    if (m > 0 && !vel) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_obstacles_moving: null argument");
    return set_agent_circles(h, "mppi_set_agent_obstacles_moving", agent, xyr, vel, m);
}

// ------------------------------------------------------------------------------------------
// obstacle tracks
// ------------------------------------------------------------------------------------------
// The track forms' table (TrackSet[n_agents]), rewritten from the host's view of every agent (the caller has synchronised the
// device).  It is read at run time, so a replayed graph sees the new sets; what a launch carries by value -- the table's
// address and the staged bytes in KParams -- is part of the graph's key.
static int upload_scene_table(mppi_handle *h);
static int upload_tracks(mppi_handle *h) {
    if (!h->d_tracks) return MPPI_OK;
    std::vector<TrackSet> tab(h->B);
    h->tracks_max = 0;
    for (int a = 0; a < h->B; ++a) {
        const mppi_handle::TrackOwn &t = tracks_of(h, a);
        h->tracks_max = std::max(h->tracks_max, t.n);
        tab[a] = TrackSet{t.d_pts.get(), t.d_thr.get(), t.n, t.n > 0 ? t.L : 1, t.iter0};
    }
    HIPCHECK(h, hipMemcpy(h->d_tracks, tab.data(), sizeof(TrackSet) * tab.size(), hipMemcpyHostToDevice));
    return upload_scene_table(h);
}

// agent < 0: the set every agent shares.  Everything that can refuse the call stands before the device is touched; the new
// buffers are allocated into locals and moved in, so a failed allocation leaves the previous set.
static int set_tracks_impl(mppi_handle *h, const char *who, int agent, const double *xy, const double *radius, int32_t n, int32_t L) {
    if (!h->cfg.obstacle_motion)
        FAIL(h, MPPI_ERR_STATE, "%s: the handle was created with obstacle_motion = 0; obstacle tracks need "
                                "mppi_config.obstacle_motion = %d at mppi_create", who, motion_value(h));
    if (h->fleet && !scene_composed(h))
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: a fleet handle (fleet_radius > 0) takes no obstacle tracks: its plan mode uses the same "
                                      "parameter words (limit: fleet_radius = 0)", who);
    if (!h->fused)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: obstacle tracks are served for horizons T <= 128 (T = %d runs the unfused rollout)", who, h->cfg.T);
    if (h->any_grid && !scene_composed(h))
        FAIL(h, MPPI_ERR_STATE, "%s: the handle has a cost grid, which uses the same parameter words (limit: remove it first, "
                                "mppi_set_cost_grid with cells = NULL)", who);
    if (agent >= h->B || (agent < 0 && agent != -1)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: agent %d not in [0, %d)", who, agent, h->B);
    if (n < 0 || n > TRACKS_MAX) FAIL(h, MPPI_ERR_SHAPE, "%s: n = %d tracks, not in [0, %d]", who, n, TRACKS_MAX);
    if (n > 0 && (L < 1 || L > TRACK_LEN_MAX)) FAIL(h, MPPI_ERR_SHAPE, "%s: L = %d points per track, not in [1, %d]", who, L, TRACK_LEN_MAX);
    if (n > 0 && (!xy || !radius)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: null argument", who);
    for (size_t i = 0; n > 0 && i < (size_t)2 * n * L; ++i)
        if (!std::isfinite(xy[i])) FAIL(h, MPPI_ERR_BAD_ARG, "%s: point %zu of track %zu is not finite", who, (i / 2) % L, i / 2 / L);
    for (int m = 0; m < n; ++m)
        if (!std::isfinite(radius[m]) || radius[m] < 0) FAIL(h, MPPI_ERR_BAD_ARG, "%s: the radius of track %d is not finite and >= 0", who, m);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    long long now = 0;
    HIPCHECK(h, hipMemcpy(&now, &h->d_st[agent < 0 ? 0 : agent].iter, sizeof(now), hipMemcpyDeviceToHost));
    DevBuf<void> pts, thr;
    DevBuf<TrackSet> table;
    if (n > 0) {
        std::vector<double> thr2(n);
        for (int m = 0; m < n; ++m) {  // (as set_circles packs a circle of this radius)
            const double t = h->cfg.obstacle_model == MPPI_OBSTACLE_CIRCLE ? 0.5 * h->cfg.safety_margin + radius[m] : radius[m];
            thr2[m] = t * t;
        }
        HIPCHECK(h, pts.alloc(rsz(h) * 2 * (size_t)n * L));
        HIPCHECK(h, thr.alloc(rsz(h) * (size_t)n));
        if (int rc = upload_real(h, pts, xy, (size_t)2 * n * L)) return rc;  // (rounded to the handle's precision, nothing else)
        if (int rc = upload_real(h, thr, thr2.data(), (size_t)n)) return rc;
    }
    if (!h->d_tracks) HIPCHECK(h, table.alloc(sizeof(TrackSet) * (size_t)h->B));
    // (nothing below refuses: the previous set goes, behind the synchronisation above)
    if (table) h->d_tracks = std::move(table);
    if (agent < 0) {
        for (mppi_handle::TrackOwn &o : h->own_tracks) o = mppi_handle::TrackOwn{};
    } else if (h->own_tracks.empty()) {
        h->own_tracks.resize(h->B);
    }
    mppi_handle::TrackOwn &t = agent < 0 ? h->tracks : h->own_tracks[agent];
    t.d_pts = std::move(pts);
    t.d_thr = std::move(thr);
    t.n = n;
    t.L = n > 0 ? L : 1;
    t.has = agent >= 0;
    t.iter0 = now;
    t.radius.assign(radius, radius + (n > 0 ? n : 0));
    h->dev_loop_primed = false;
    drop_graph(h);
    return upload_tracks(h);
}

extern "C" int mppi_set_obstacle_tracks(mppi_handle *h, const double *xy, const double *radius, int32_t n, int32_t L) {
    if (!h) return MPPI_ERR_BAD_ARG;
    return set_tracks_impl(h, "mppi_set_obstacle_tracks", -1, xy, radius, n, L);
}
extern "C" int mppi_set_agent_obstacle_tracks(mppi_handle *h, int32_t agent, const double *xy, const double *radius, int32_t n, int32_t L) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (agent < 0) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_obstacle_tracks: agent %d not in [0, %d)", agent, h->B);
    return set_tracks_impl(h, "mppi_set_agent_obstacle_tracks", h->B == 1 && agent == 0 ? -1 : agent, xy, radius, n, L);
}

extern "C" int mppi_get_obstacle_tracks_at(mppi_handle *h, int32_t agent, int32_t step, double *xyr_out, int32_t cap, int32_t *n_out) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!n_out || cap < 0 || (cap > 0 && !xyr_out)) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_obstacle_tracks_at: bad argument");
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_obstacle_tracks_at: agent %d not in [0, %d)", agent, h->B);
    if (step < 0) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_obstacle_tracks_at: step %d is negative (steps count ahead of the clock)", step);
    const mppi_handle::TrackOwn &t = tracks_of(h, agent);
    *n_out = t.n;
    if (cap < t.n) FAIL(h, MPPI_ERR_SHAPE, "mppi_get_obstacle_tracks_at: agent %d has %d tracks, cap = %d", agent, t.n, cap);
    if (t.n == 0) return MPPI_OK;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    long long now = 0;
    HIPCHECK(h, hipMemcpy(&now, &h->d_st[agent].iter, sizeof(now), hipMemcpyDeviceToHost));
    const int at = track_index(track_clock(now, t.iter0, t.L), step, t.L);
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        std::vector<R> pt((size_t)2 * t.n);  // (point `at` of every track: rows L points apart)
        HIPCHECK(h, hipMemcpy2D(pt.data(), 2 * sizeof(R), static_cast<const R *>(t.d_pts.get()) + (size_t)2 * at, 2 * sizeof(R) * (size_t)t.L,
                                2 * sizeof(R), (size_t)t.n, hipMemcpyDeviceToHost));
        for (int m = 0; m < t.n; ++m) {
            xyr_out[3 * m] = (double)pt[2 * m];
            xyr_out[3 * m + 1] = (double)pt[2 * m + 1];
            xyr_out[3 * m + 2] = t.radius[m];
        }
        return MPPI_OK;
    });
}

// ------------------------------------------------------------------------------------------
// cost grids
// ------------------------------------------------------------------------------------------
// The grid forms' table (GridSet<R>[n_agents]), rewritten from the host's view of every agent (the caller has synchronised the
// device).  It is read at run time, so a replayed graph sees the new grids; the table's address, which a launch carries by
// value in KParams, stays for the handle's life.
static int upload_grids(mppi_handle *h) {
    if (!h->d_grids) return MPPI_OK;
    h->any_grid = false;
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        std::vector<GridSet<R>> tab(h->B);
        for (int a = 0; a < h->B; ++a) {
            const mppi_handle::GridOwn &g = grid_of(h, a);
            h->any_grid |= g.nx > 0;
            tab[a] = GridSet<R>{static_cast<const R *>(g.d_cells.get()), g.nx, g.ny, (R)g.ox, (R)g.oy, (R)g.inv, (R)g.weight, (R)g.lethal};
        }
        HIPCHECK(h, hipMemcpy(h->d_grids, tab.data(), sizeof(GridSet<R>) * tab.size(), hipMemcpyHostToDevice));
        return upload_scene_table(h);
    });
}

// The composed form's table (SceneTable<R>), rewritten from the host's view of the three ingredients (the caller has
// synchronised the device).  It is read at run time, so a replayed graph sees an ingredient come or go as far as the launch it
// captured still serves; the table's address, which a launch carries by value in KParams, stays for the handle's life.
static int upload_scene_table(mppi_handle *h) {
    if (!h->d_scene) return MPPI_OK;
    const mppi_config &c = h->cfg;
    const double thr = c.obstacle_model == MPPI_OBSTACLE_CIRCLE ? 0.5 * c.safety_margin + c.fleet_radius : c.fleet_radius;
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        const SceneTable<R> tb = {h->fleet_plan ? static_cast<const PlanPoint<R> *>(h->d_plans.get()) : nullptr,
                                  max_tracks(h) > 0 ? h->d_tracks.get() : nullptr,
                                  h->any_grid ? static_cast<const GridSet<R> *>(h->d_grids.get()) : nullptr, (R)(thr * thr)};
        HIPCHECK(h, hipMemcpy(h->d_scene, &tb, sizeof(tb), hipMemcpyHostToDevice));
        return MPPI_OK;
    });
}

// agent < 0: the grid every agent shares.  Everything that can refuse the call stands before the device is touched; new
// buffers are allocated into locals and moved in, so a failed allocation leaves the previous grid.  A grid of the shape the
// entry already has is copied into its buffer: the descriptor's addresses, the plan and a cached graph stay.
static int set_grid_impl(mppi_handle *h, const char *who, int agent, const double *cells, int32_t nx, int32_t ny, double ox, double oy,
                         double resolution, double weight, double lethal) {
    if (!h->cfg.obstacle_motion)
        FAIL(h, MPPI_ERR_STATE, "%s: the handle was created with obstacle_motion = 0; a cost grid needs "
                                "mppi_config.obstacle_motion = %d at mppi_create", who, motion_value(h));
    if (h->fleet && !scene_composed(h))
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: a fleet handle (fleet_radius > 0) takes no cost grid: its plan mode uses the same "
                                      "parameter words (limit: fleet_radius = 0)", who);
    if (!h->fused)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: cost grids are served for horizons T <= 128 (T = %d runs the unfused rollout)", who, h->cfg.T);
    if (max_tracks(h) > 0 && !scene_composed(h))
        FAIL(h, MPPI_ERR_STATE, "%s: the handle has obstacle tracks, which use the same parameter words (limit: remove them first, "
                                "mppi_set_obstacle_tracks with n = 0)", who);
    if (agent >= h->B || (agent < 0 && agent != -1)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: agent %d not in [0, %d)", who, agent, h->B);
    const bool clear = !cells || nx == 0;
    if (!clear) {
        if (nx < GRID_DIM_MIN || nx > GRID_DIM_MAX || ny < GRID_DIM_MIN || ny > GRID_DIM_MAX)
            FAIL(h, MPPI_ERR_BAD_ARG, "%s: a grid of %d x %d nodes, each side not in [%d, %d]", who, nx, ny, GRID_DIM_MIN, GRID_DIM_MAX);
        if (!std::isfinite(ox) || !std::isfinite(oy)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: the origin (%g, %g) is not finite", who, ox, oy);
        if (!std::isfinite(resolution) || !(resolution > 0)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: resolution %g is not finite and > 0", who, resolution);
        if (!std::isfinite(weight) || weight < 0) FAIL(h, MPPI_ERR_BAD_ARG, "%s: weight %g is not finite and >= 0", who, weight);
        if (std::isnan(lethal) || !(lethal > 0)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: lethal %g is not > 0 (+inf: soft cost only)", who, lethal);
        for (size_t i = 0; i < (size_t)nx * ny; ++i)
            if (!std::isfinite(cells[i])) FAIL(h, MPPI_ERR_BAD_ARG, "%s: cell (%zu, %zu) is not finite", who, i % nx, i / nx);
    }
    if (clear && !h->d_grids) return MPPI_OK;  // (nothing to remove: the handle stays the one that never called the setter)
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    mppi_handle::GridOwn *cur = agent < 0 ? &h->grid : !h->own_grids.empty() ? &h->own_grids[agent] : nullptr;
    // (the shared setter takes back what the agent setter gave, so it keeps its buffers only while no agent has an own entry)
    bool own_any = false;
    for (const mppi_handle::GridOwn &o : h->own_grids) own_any |= o.has;
    const bool same = !clear && cur && cur->nx == nx && cur->ny == ny && (agent < 0 ? !own_any : cur->has);
    DevBuf<void> buf, table;
    if (!clear && !same) HIPCHECK(h, buf.alloc(rsz(h) * (size_t)nx * ny));
    if (!h->d_grids) HIPCHECK(h, table.alloc(sizeof(GridSet<double>) * (size_t)h->B));
    if (!clear)
        if (int rc = upload_real(h, same ? cur->d_cells.get() : buf.get(), cells, (size_t)nx * ny)) return rc;
    // (nothing below refuses)
    if (table) h->d_grids = std::move(table);
    if (agent < 0) {
        for (mppi_handle::GridOwn &o : h->own_grids) o = mppi_handle::GridOwn{};
    } else if (h->own_grids.empty()) {
        h->own_grids.resize(h->B);
    }
    mppi_handle::GridOwn &g = agent < 0 ? h->grid : h->own_grids[agent];
    if (!same) g.d_cells = std::move(buf);
    g.nx = clear ? 0 : nx;
    g.ny = clear ? 0 : ny;
    g.has = agent >= 0;
    g.ox = ox; g.oy = oy; g.inv = clear ? 0.0 : 1.0 / resolution; g.weight = weight; g.lethal = lethal;
    h->dev_loop_primed = false;
    if (!same) drop_graph(h);
    return upload_grids(h);
}

extern "C" int mppi_set_cost_grid(mppi_handle *h, const double *cells, int32_t nx, int32_t ny, double origin_x, double origin_y,
                                  double resolution, double weight, double lethal) {
    if (!h) return MPPI_ERR_BAD_ARG;
    return set_grid_impl(h, "mppi_set_cost_grid", -1, cells, nx, ny, origin_x, origin_y, resolution, weight, lethal);
}
extern "C" int mppi_set_agent_cost_grid(mppi_handle *h, int32_t agent, const double *cells, int32_t nx, int32_t ny, double origin_x,
                                        double origin_y, double resolution, double weight, double lethal) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (agent < 0) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_cost_grid: agent %d not in [0, %d)", agent, h->B);
    return set_grid_impl(h, "mppi_set_agent_cost_grid", h->B == 1 && agent == 0 ? -1 : agent, cells, nx, ny, origin_x, origin_y,
                         resolution, weight, lethal);
}
// mppi_eval_cost_grid / mppi_eval_cost_grid_footprint: agent `agent`'s grid alone at n rows of `width` numbers (what ==
// EVAL_GRID_POINTS: xy, EVAL_GRID_FOOTPRINT: x, y, yaw), and -- points not null -- the nine world points of every row
static int eval_grid_impl(mppi_handle *h, const char *who, int what, int32_t agent, const double *in, int width, int32_t n, double *value,
                          double *points) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!in || !value || n < 1) FAIL(h, MPPI_ERR_BAD_ARG, "%s: bad argument", who);
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "%s: agent %d not in [0, %d)", who, agent, h->B);
    if (grid_of(h, agent).nx == 0) FAIL(h, MPPI_ERR_STATE, "%s: agent %d has no cost grid", who, agent);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) -> int {
        using R = decltype(r);
        const KParams<R> P = make_params<R>(h, nullptr);
        DevBuf<R> din, dout, dpts;
        HIPCHECK(h, din.alloc(sizeof(R) * (size_t)n * width));
        HIPCHECK(h, dout.alloc(sizeof(R) * (size_t)n));
        if (points) HIPCHECK(h, dpts.alloc(sizeof(R) * (size_t)n * 18));
        if (int rc = upload_real(h, din, in, (size_t)n * width)) return rc;
        launch_eval_pose<R>(P, P.obs_motion == OBS_MOTION_SCENE ? EVAL_FORM_SCENE : EVAL_FORM_GRID, what, agent, din, nullptr, nullptr, n,
                            dout, points ? dpts.get() : nullptr, nullptr);
        HIPCHECK(h, hipGetLastError());
        HIPCHECK(h, hipDeviceSynchronize());
        if (points)
            if (int rc = download_real(h, points, dpts, (size_t)n * 18)) return rc;
        return download_real(h, value, dout, (size_t)n);
    });
}
// the raw value of agent `agent`'s grid at n points, from the device helper the rollout prices with (grid_value)
extern "C" int mppi_eval_cost_grid(mppi_handle *h, int32_t agent, const double *xy, int32_t n, double *value) {
    return eval_grid_impl(h, "mppi_eval_cost_grid", EVAL_GRID_POINTS, agent, xy, 2, n, value, nullptr);
}

// The footprint mode: one for every agent, kept across grid uploads and removals.  Every refusal stands before the device is
// touched; a call that leaves the mode as it is changes nothing.
extern "C" int mppi_set_cost_grid_footprint(mppi_handle *h, int32_t mode) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (mode != MPPI_GRID_FOOTPRINT_CENTRE && mode != MPPI_GRID_FOOTPRINT_OUTLINE)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_cost_grid_footprint: mode %d is neither MPPI_GRID_FOOTPRINT_CENTRE nor MPPI_GRID_FOOTPRINT_OUTLINE", mode);
    if (!h->cfg.obstacle_motion)
        FAIL(h, MPPI_ERR_STATE, "mppi_set_cost_grid_footprint: the handle was created with obstacle_motion = 0; a cost grid needs "
                                "mppi_config.obstacle_motion = %d at mppi_create", motion_value(h));
    if (mode == MPPI_GRID_FOOTPRINT_OUTLINE && h->cfg.obstacle_model != MPPI_OBSTACLE_OUTLINE)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_set_cost_grid_footprint: the outline footprint needs obstacle_model = MPPI_OBSTACLE_OUTLINE "
                                      "(limit: a disc is served by inflating the map by its radius)");
    if (mode == MPPI_GRID_FOOTPRINT_OUTLINE && !h->fused)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_set_cost_grid_footprint: cost grids are served for horizons T <= 128 (T = %d runs the unfused rollout)",
             h->cfg.T);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (mode == h->grid_footprint) return MPPI_OK;
    h->grid_footprint = mode;
    h->dev_loop_primed = false;
    drop_graph(h);
    return MPPI_OK;
}
extern "C" int mppi_get_cost_grid_footprint(const mppi_handle *h, int32_t *mode) {
    if (!h || !mode) return MPPI_ERR_BAD_ARG;
    *mode = h->grid_footprint;
    return MPPI_OK;
}
// g_foot of agent `agent`'s grid at n poses, and the nine world points, from the device function the rollout prices with
// (grid_value_outline), whatever the handle's mode
extern "C" int mppi_eval_cost_grid_footprint(mppi_handle *h, int32_t agent, const double *pose, int32_t n, double *value, double *points) {
    return eval_grid_impl(h, "mppi_eval_cost_grid_footprint", EVAL_GRID_FOOTPRINT, agent, pose, 3, n, value, points);
}

extern "C" int mppi_get_agent_status(mppi_handle *h, int32_t *idx_out, int32_t *path_end_out) {
    if (!h) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    std::vector<DevState> st(h->B);
    HIPCHECK(h, hipMemcpy(st.data(), h->d_st, sizeof(DevState) * st.size(), hipMemcpyDeviceToHost));
    for (int a = 0; a < h->B; ++a) {
        if (idx_out) idx_out[a] = st[a].p;
        if (path_end_out) path_end_out[a] = st[a].path_end;
    }
    return MPPI_OK;
}

// (the caller has synchronised the device: no instance is running)
static void drop_graph(mppi_handle *h) {
    for (GraphExec &g : h->graph_exec) (void)g.reset();
    h->graph_key.clear();
}

#define MLP_SUPPORTED_SET "hidden H in {64, 128, 256, 512} x n_hidden in {1, 2, 3, 4}"

// Agent a's model: what it was given for itself, else the shared one
static bool has_model(const mppi_handle *h, int a) { return (a < (int)h->own_mlp.size() && h->own_mlp[a].set) || h->shared_set; }
static const MlpParams &model_of(const mppi_handle *h, int a) {
    return a < (int)h->own_mlp.size() && h->own_mlp[a].set ? h->own_mlp[a].q : h->mlp_shared;
}
// The batched kernels' table (MlpParams[n_agents]) and the by-value copy of agent 0's entry, rewritten from the host's view of
// every agent (the caller has synchronised the device, as for upload_scenes).  The table is read at run time, so a cached graph
// (ensure_graph) replays the new models; its address and agent 0's entry are part of the graph's key.
static int upload_models(mppi_handle *h) {
    if (has_model(h, 0)) h->mlp = model_of(h, 0);
    if (!h->d_models) return MPPI_OK;
    std::vector<MlpParams> tab(h->B);
    for (int a = 0; a < h->B; ++a) tab[a] = has_model(h, a) ? model_of(h, a) : MlpParams{};
    HIPCHECK(h, hipMemcpy(h->d_models, tab.data(), sizeof(MlpParams) * tab.size(), hipMemcpyHostToDevice));
    return MPPI_OK;
}

// A model as the setters hold it before the handle is touched: both packings on the host and MlpParams with offsets into
// them where the device pointers go (place_mlp)
struct HostMlp {
    std::vector<float> f32;            // f32 fragment order (k_rollout_mlp, 512 only) + the biases and the output layer every kernel reads
    std::vector<unsigned short> f16;   // the same weights as f16 (hi, lo) planes for the split kernels
    size_t o_win = 0, o_bin = 0, o_wh[MLP_MAX_HIDDEN], o_bh[MLP_MAX_HIDDEN], o_wo = 0, n_in16 = 0, n_h16 = 0;
    MlpParams q = {};                  // b_out, use_h3, in_gain / in_bias, shape
    double wmax = 0.0;
    bool f16_range = true;
    Switches sw;
};

// Validation and packing of one model for `who` (any model setter): nothing in the handle changes (but its error text).
// read_switches is consulted here and nowhere else in the model setters.
static int pack_mlp(mppi_handle *h, const char *who, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                    const float *const *w_hidden, const float *const *b_hidden, const float *w_out, const float *b_out, HostMlp *m) {
    if (!h || !w_in || !b_in || !w_hidden || !b_hidden || !w_out || !b_out) FAIL(h, MPPI_ERR_BAD_ARG, "%s: null argument", who);
    if (h->cfg.model != MPPI_MODEL_DIFFDRIVE_MLP) FAIL(h, MPPI_ERR_STATE, "%s needs MPPI_MODEL_DIFFDRIVE_MLP", who);
    if (!mlp_shape_supported(hidden, n_hidden))
        FAIL(h, MPPI_ERR_SHAPE, "%s: Linear(5,H) -> n x [Linear(H,H), tanh] -> Linear(H,3) is built for " MLP_SUPPORTED_SET
                                " (got hidden = %d, n = %d)", who, hidden, n_hidden);
    for (int l = 0; l < n_hidden; ++l)
        if (!w_hidden[l] || !b_hidden[l]) FAIL(h, MPPI_ERR_BAD_ARG, "%s: null hidden layer %d", who, l);
    const int H = hidden;
    const bool h3_shape = mlp_shape_is_h3(H, n_hidden);  // 512 x 3, 512 x 2: k_rollout_mlp_h3 / k_rollout_mlp; else k_rollout_mlp_w
    // The split kernels carry every WEIGHT as two f16 numbers: one beyond the f16 range (65504; e.g. W_in / in_scale with a
    // StandardScaler scale near 1e-6) would become inf in the high plane.  At 512 x 3 and 512 x 2 such a model takes the
    // f32-input MFMA kernel, which has no range limit, and the handle says so (mppi_last_error; mppi_get_mlp_kernel); the other
    // shapes have no f32-input kernel and refuse it.  Inputs and first-layer pre-activations of any magnitude are handled
    // inside the split kernels (per-sample power-of-two scales).
    double wmax = 0.0;
    for (size_t i = 0; i < (size_t)H * 5; ++i) wmax = fmax(wmax, fabs((double)w_in[i]));
    for (int l = 0; l < n_hidden; ++l)
        for (size_t i = 0; i < (size_t)H * H; ++i) wmax = fmax(wmax, fabs((double)w_hidden[l][i]));
    const bool f16_range = wmax <= 65504.0;  // (false for NaN too)
    m->wmax = wmax;
    m->f16_range = f16_range;
    m->sw = read_switches();  // (MPPI_MLP_F32 / _TERMS / _FORM hold for this model until the next model setter)
    const Switches &sw = m->sw;
    if (!h3_shape && !f16_range)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: max |weight| = %.4g exceeds the f16 range, and only the 512 x 3 and 512 x 2 "
                                      "models have an f32-input kernel to serve that (got hidden = %d, n = %d)", who, wmax, H, n_hidden);
    if (!h3_shape && sw.mlp.f32)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: MPPI_MLP_F32 is set, and the f32-input kernel serves only the 512 x 3 and "
                                      "512 x 2 models (got hidden = %d, n = %d)", who, H, n_hidden);
    // several agents per handle run the split kernels only (k_rollout_mlp_h3_agents, k_rollout_mlp_w_agents)
    if (h->B > 1 && !f16_range)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: max |weight| = %.4g exceeds the f16 range, and the f32-input kernel that "
                                      "serves such a model runs one agent per handle (n_agents = %d)", who, wmax, h->B);
    if (h->B > 1 && sw.mlp.f32)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: MPPI_MLP_F32 is set, and the f32-input kernel runs one agent per handle "
                                      "(n_agents = %d)", who, h->B);
    // a scene handle (obstacle_motion = 2) has scene forms of the split kernels only
    if (learned_scene(h) && !f16_range)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: max |weight| = %.4g exceeds the f16 range, and the f32-input kernel that serves such a "
                                      "model has no scene form (limit: obstacle_motion = 0)", who, wmax);
    if (learned_scene(h) && sw.mlp.f32)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "%s: MPPI_MLP_F32 is set, and the f32-input kernel has no scene form (limit: obstacle_motion = 0)", who);
    const int CT = H / 32;  // column tiles of 32 outputs
    const size_t n_in = (size_t)CT * 1 * 64 * 4, n_h = (size_t)CT * (H / 8) * 64 * 4;
    const size_t total = n_in + H + MLP_MAX_HIDDEN * (n_h + H) + 3 * (size_t)H;
    std::vector<float> &host = m->f32;
    host.assign(total, 0.f);
    size_t o = 0;
    m->o_win = o; pack_linear(w_in, 5, host.data() + o, H); o += n_in;
    m->o_bin = o; memcpy(host.data() + o, b_in, H * sizeof(float)); o += H;
    for (int l = 0; l < MLP_MAX_HIDDEN; ++l) {  // (a shallower model leaves the last slots unused)
        m->o_wh[l] = o; m->o_bh[l] = o + n_h;
        if (l < n_hidden) {
            pack_linear(w_hidden[l], H, host.data() + o, H);
            memcpy(host.data() + o + n_h, b_hidden[l], H * sizeof(float));
        }
        o += n_h + H;
    }
    m->o_wo = o; memcpy(host.data() + o, w_out, 3 * (size_t)H * sizeof(float)); o += 3 * (size_t)H;
    m->n_in16 = (size_t)2 * CT * 1 * 64 * 8;
    m->n_h16 = (size_t)2 * CT * (H / 16) * 64 * 8;
    m->f16.assign(m->n_in16 + MLP_MAX_HIDDEN * m->n_h16, 0);
    pack_linear_h3(w_in, 5, m->f16.data(), H);
    for (int l = 0; l < n_hidden; ++l) pack_linear_h3(w_hidden[l], H, m->f16.data() + m->n_in16 + (size_t)l * m->n_h16, H);
    for (int i = 0; i < 3; ++i) m->q.b_out[i] = b_out[i];
    m->q.use_h3 = sw.mlp.f32 || !f16_range ? 0 : 1;  // (!f16_range: 512 x 3 / 512 x 2 on one agent only, refused above otherwise)
    {   // bounds the split kernel scales the first layer's output with: |W_in z + b_in|_inf <= in_gain |z|_inf + in_bias
        double gain = 0.0, bias = 0.0;
        for (int n = 0; n < H; ++n) {
            double row = 0.0;
            for (int j = 0; j < 5; ++j) row += fabs((double)w_in[n * 5 + j]);
            gain = fmax(gain, row);
            bias = fmax(bias, fabs((double)b_in[n]));
        }
        m->q.in_gain = (float)(gain * (1.0 + 1e-6));
        m->q.in_bias = (float)(bias * (1.0 + 1e-6));
    }
    m->q.n_hidden = n_hidden;
    m->q.hidden = H;
    return MPPI_OK;
}

// A packed model into a buffer pair (the shared one or an agent's own; grown when too small -- the new buffers are
// allocated before the old ones go, so a failed allocation leaves the pair and *q as they were) and its view into *q.
// The caller has synchronised the device.
static int place_mlp(mppi_handle *h, const HostMlp &m, DevBuf<float> *d, size_t *cap, DevBuf<unsigned short> *d16, size_t *cap16,
                     MlpParams *q) {
    DevBuf<float> nd;  // (released on the way out unless they move in)
    DevBuf<unsigned short> nd16;
    if (!*d || *cap < m.f32.size()) HIPCHECK(h, nd.alloc(m.f32.size() * sizeof(float)));
    if (!*d16 || *cap16 < m.f16.size()) {
        const hipError_t e = nd16.alloc(m.f16.size() * sizeof(unsigned short));
        if (e != hipSuccess) FAIL(h, MPPI_ERR_HIP, "hipMalloc(model) failed: %s", hipGetErrorString(e));
    }
    if (nd) *d = std::move(nd), *cap = m.f32.size();  // (the old buffer goes here, behind both allocations)
    if (nd16) *d16 = std::move(nd16), *cap16 = m.f16.size();
    HIPCHECK(h, hipMemcpy(*d, m.f32.data(), m.f32.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemcpy(*d16, m.f16.data(), m.f16.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    *q = m.q;
    q->w_in = *d + m.o_win;
    q->b_in = *d + m.o_bin;
    for (int l = 0; l < MLP_MAX_HIDDEN; ++l) { q->w_h[l] = *d + m.o_wh[l]; q->b_h[l] = *d + m.o_bh[l]; }
    q->w_out = *d + m.o_wo;
    q->h3_w_in = *d16;
    for (int l = 0; l < MLP_MAX_HIDDEN; ++l) q->h3_w_h[l] = *d16 + m.n_in16 + (size_t)l * m.n_h16;
    return MPPI_OK;
}

// Every model setter behind its argument checks.  agent < 0: the model of every agent (mppi_set_mlp) -- the agents' own
// copies are released; else agent's own model on a batched handle.
static int set_model(mppi_handle *h, const char *who, int agent, const HostMlp &m) {
    if (agent >= 0)  // one launch is one instantiation: one shape per batch
        for (int a = 0; a < h->B; ++a)
            if (a != agent && has_model(h, a) && (model_of(h, a).hidden != m.q.hidden || model_of(h, a).n_hidden != m.q.n_hidden))
                FAIL(h, MPPI_ERR_SHAPE, "%s: a %d x %d model for agent %d beside the %d x %d model of agent %d: the agents of a handle "
                                        "share one shape (mppi_set_mlp changes it for all of them)", who, m.q.hidden, m.q.n_hidden,
                     agent, model_of(h, a).hidden, model_of(h, a).n_hidden, a);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (agent < 0) {
        // A cached closed-loop graph (ensure_graph) holds the previous model's MlpParams -- device pointers into the buffers
        // below, which may now move or be repacked for another shape: it is dropped here, before anything changes.
        drop_graph(h);
        if (int rc = place_mlp(h, m, &h->d_mlp, &h->mlp_cap, &h->d_mlp16, &h->mlp16_cap, &h->mlp_shared)) return rc;
        h->shared_set = true;
        for (mppi_handle::OwnModel &o : h->own_mlp) o = mppi_handle::OwnModel{};  // several agents: every agent runs this model again
    } else {
        mppi_handle::OwnModel &o = h->own_mlp[agent];
        if (int rc = place_mlp(h, m, &o.d_mlp, &o.cap, &o.d_mlp16, &o.cap16, &o.q)) return rc;
        o.set = true;
    }
    h->sw.mlp = m.sw.mlp;
    if (int rc = upload_models(h)) return rc;
    if (!m.f16_range) {  // (512 x 3 / 512 x 2 on a single-agent handle only: refused by pack_mlp otherwise)
        char b[256];
        snprintf(b, sizeof(b), "%s: max |weight| = %.4g exceeds the f16 range: the f32-input MFMA kernel serves this model", who, m.wmax);
        h->err = b;
    }
    // the rollout kernel that serves this model: its name before the first launch already
    h->rollout_kernel = plan_mlp(make_params<float>(h, nullptr), has_model(h, 0) ? h->mlp : m.q, h->sw, nullptr, learned_fleet(h)).k.name;
    return MPPI_OK;
}

extern "C" int mppi_set_mlp(mppi_handle *h, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                            const float *const *w_hidden, const float *const *b_hidden, const float *w_out,
                            const float *b_out) {
    HostMlp m;
    if (int rc = pack_mlp(h, "mppi_set_mlp", hidden, n_hidden, w_in, b_in, w_hidden, b_hidden, w_out, b_out, &m)) return rc;
    return set_model(h, "mppi_set_mlp", -1, m);
}

extern "C" int mppi_set_agent_mlp(mppi_handle *h, int32_t agent, int32_t hidden, int32_t n_hidden, const float *w_in,
                                  const float *b_in, const float *const *w_hidden, const float *const *b_hidden,
                                  const float *w_out, const float *b_out) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_mlp: agent %d not in [0, %d)", agent, h->B);
    if (h->B == 1) return mppi_set_mlp(h, hidden, n_hidden, w_in, b_in, w_hidden, b_hidden, w_out, b_out);
    HostMlp m;
    if (int rc = pack_mlp(h, "mppi_set_agent_mlp", hidden, n_hidden, w_in, b_in, w_hidden, b_hidden, w_out, b_out, &m)) return rc;
    return set_model(h, "mppi_set_agent_mlp", agent, m);
}

// The StandardScaler statistics folded into the first and the last Linear (include/mppi_hip.h), then the plain setter:
// agent < 0 mppi_set_mlp, else mppi_set_agent_mlp
static int set_mlp_scaled(mppi_handle *h, int agent, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                          const float *const *w_hidden, const float *const *b_hidden, const float *w_out, const float *b_out,
                          const double *in_mean, const double *in_scale, const double *out_mean, const double *out_scale) {
    if (!h || !w_in || !b_in || !w_out || !b_out) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_mlp_scaled: null argument");
    if ((in_mean == nullptr) != (in_scale == nullptr) || (out_mean == nullptr) != (out_scale == nullptr))
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_mlp_scaled: a mean without its scale (or the reverse)");
    if (!mlp_shape_supported(hidden, n_hidden))
        FAIL(h, MPPI_ERR_SHAPE, "mppi_set_mlp_scaled: Linear(5,H) -> n x [Linear(H,H), tanh] -> Linear(H,3) is built for " MLP_SUPPORTED_SET
                                " (got hidden = %d, n = %d)", hidden, n_hidden);
    std::vector<float> wi(w_in, w_in + (size_t)hidden * 5), bi(b_in, b_in + hidden), wo(w_out, w_out + (size_t)3 * hidden),
        bo(b_out, b_out + 3);
    if (in_mean) {
        for (int j = 0; j < 5; ++j)
            if (!(in_scale[j] != 0.0)) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_mlp_scaled: in_scale[%d] is zero", j);
        for (int n = 0; n < hidden; ++n) {
            double shift = 0.0;
            for (int j = 0; j < 5; ++j) {
                const double w = (double)w_in[(size_t)n * 5 + j] / in_scale[j];
                wi[(size_t)n * 5 + j] = (float)w;
                shift += w * in_mean[j];
            }
            bi[n] = (float)((double)b_in[n] - shift);
        }
    }
    if (out_mean) {
        for (int j = 0; j < 3; ++j) {
            for (int n = 0; n < hidden; ++n) wo[(size_t)j * hidden + n] = (float)((double)w_out[(size_t)j * hidden + n] * out_scale[j]);
            bo[j] = (float)((double)b_out[j] * out_scale[j] + out_mean[j]);
        }
    }
    if (agent >= 0) return mppi_set_agent_mlp(h, agent, hidden, n_hidden, wi.data(), bi.data(), w_hidden, b_hidden, wo.data(), bo.data());
    return mppi_set_mlp(h, hidden, n_hidden, wi.data(), bi.data(), w_hidden, b_hidden, wo.data(), bo.data());
}

extern "C" int mppi_set_mlp_scaled(mppi_handle *h, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                                   const float *const *w_hidden, const float *const *b_hidden, const float *w_out,
                                   const float *b_out, const double *in_mean, const double *in_scale, const double *out_mean,
                                   const double *out_scale) {
    return set_mlp_scaled(h, -1, hidden, n_hidden, w_in, b_in, w_hidden, b_hidden, w_out, b_out, in_mean, in_scale, out_mean, out_scale);
}

extern "C" int mppi_set_agent_mlp_scaled(mppi_handle *h, int32_t agent, int32_t hidden, int32_t n_hidden, const float *w_in,
                                         const float *b_in, const float *const *w_hidden, const float *const *b_hidden,
                                         const float *w_out, const float *b_out, const double *in_mean, const double *in_scale,
                                         const double *out_mean, const double *out_scale) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_agent_mlp_scaled: agent %d not in [0, %d)", agent, h->B);
    return set_mlp_scaled(h, agent, hidden, n_hidden, w_in, b_in, w_hidden, b_hidden, w_out, b_out, in_mean, in_scale, out_mean, out_scale);
}

extern "C" int mppi_set_u_prev(mppi_handle *h, const double *u) {
    if (!h || !u) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_u_prev: null argument");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    return upload_real(h, h->d_u, u, (size_t)h->B * 2 * h->cfg.T);  // [n_agents][T][2]
}

extern "C" int mppi_get_u_prev(mppi_handle *h, double *u) {
    if (!h || !u) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_u_prev: null argument");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    return download_real(h, u, h->d_u, (size_t)h->B * 2 * h->cfg.T);  // [n_agents][T][2]
}

extern "C" int mppi_set_waypoint_idx(mppi_handle *h, int32_t idx) {
    if (!h) return MPPI_ERR_BAD_ARG;
    for (int a = 0; a < h->B; ++a) {  // (every agent's path, where it has one yet)
        const int n = scene_of(h, a).n_ref;
        if (idx < 0 || (n > 0 && idx >= n)) FAIL(h, MPPI_ERR_BAD_ARG, "waypoint index %d out of range", idx);
    }
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    for (int a = 0; a < h->B; ++a)  // (every agent of a batched handle)
        HIPCHECK(h, hipMemcpy(&h->d_st[a].p, &idx, sizeof(int), hipMemcpyHostToDevice));
    h->idx = idx;
    h->dev_loop_primed = false;
    return MPPI_OK;
}

extern "C" int mppi_get_waypoint_idx(mppi_handle *h, int32_t *idx) {
    if (!h || !idx) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    HIPCHECK(h, hipMemcpy(idx, &h->d_st->p, sizeof(int), hipMemcpyDeviceToHost));
    h->idx = *idx;
    return MPPI_OK;
}

extern "C" int mppi_set_iteration(mppi_handle *h, int64_t iteration) {
    if (!h || iteration < 0) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    long long it = iteration;
    for (int a = 0; a < h->B; ++a) {
        if (h->cfg.obstacle_motion) {  // the counter replays noise, it does not move obstacles: their clocks' origins follow it
            long long old = 0;
            HIPCHECK(h, hipMemcpy(&old, &h->d_st[a].iter, sizeof(old), hipMemcpyDeviceToHost));
            if (a == 0) h->obs_iter0 += it - old;
            if (a < (int)h->own.size()) h->own[a].obs_iter0 += it - old;
            if (a == 0) h->tracks.iter0 += it - old;  // (and the tracks' with the circles')
            if (a < (int)h->own_tracks.size()) h->own_tracks[a].iter0 += it - old;
        }
        HIPCHECK(h, hipMemcpy(&h->d_st[a].iter, &it, sizeof(it), hipMemcpyHostToDevice));
    }
    h->iter = it;
    if (h->cfg.obstacle_motion) {
        h->dev_loop_primed = false;
        if (int rc = upload_tracks(h)) return rc;
        return upload_scenes(h);
    }
    return MPPI_OK;
}

extern "C" int mppi_set_state(mppi_handle *h, const double *x) {  // x: [n_agents][nx]
    if (!h || !x) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    for (int a = 0; a < h->B; ++a) {
        double v[4] = {0, 0, 0, 0};
        for (int i = 0; i < h->nx; ++i) v[i] = x[(size_t)a * h->nx + i];
        HIPCHECK(h, hipMemcpy(h->d_st[a].x0, v, sizeof(v), hipMemcpyHostToDevice));
    }
    h->dev_loop_primed = false;
    return MPPI_OK;
}

extern "C" int mppi_get_state(mppi_handle *h, double *x) {  // x: [n_agents][nx]
    if (!h || !x) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    for (int a = 0; a < h->B; ++a) {
        double v[4];
        HIPCHECK(h, hipMemcpy(v, h->d_st[a].x0, sizeof(v), hipMemcpyDeviceToHost));
        for (int i = 0; i < h->nx; ++i) x[(size_t)a * h->nx + i] = v[i];
    }
    return MPPI_OK;
}

// ------------------------------------------------------------------------------------------
// parameter packing
// ------------------------------------------------------------------------------------------
template <typename R> static KParams<R> make_params(const mppi_handle *h, const float *eps) {
    const mppi_config &c = h->cfg;
    KParams<R> P;
    memset(&P, 0, sizeof(P));
    P.K = c.K;
    P.T = c.T;
    P.k_offset = c.k_offset;
    const double thr = (1.0 - c.param_exploration) * c.K_global;  // k < thr, mppi_differential_drive.py:116
    double ne = ceil(thr);
    if (ne < 0) ne = 0;
    if (ne > c.K_global) ne = c.K_global;
    P.n_exploit = (int)ne;
    // (several agents: agent 0's scene here, every agent's in the table -- see KParams::scenes)
    const AgentScene sc0 = scene_of(h, 0);
    P.n_ref = sc0.n_ref;
    P.n_obs = sc0.n_obs;
    P.window = c.search_window;
    P.model = kernel_model(c);
    P.accumulate = c.accumulate_stage_cost;
    P.sequential = c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL;
    P.per_rollout = c.waypoint_mode == MPPI_WAYPOINT_PER_ROLLOUT;
    P.lb_timeout = h->sw.lb_timeout_ticks;
    P.obstacle_model = any_obstacles(h) ? c.obstacle_model : OBS_NONE;
    P.clamp_rollout = c.clamp_rollout;
    P.wrap_stage = c.wrap_yaw_stage;
    P.wrap_term = c.wrap_yaw_terminal;
    // this call's tensor, else the noise ring when one is set (slot = iteration mod slots, picked in the kernels), else Philox
    const float *noise = eps ? eps : h->noise_ring;
    P.eps_slots = eps ? 0 : (h->noise_ring ? h->noise_slots : 0);
    P.use_philox = noise == nullptr;
    P.traj_per_block = h->traj_per_block;
    P.seed_lo = (unsigned)(c.seed & 0xffffffffu);
    P.seed_hi = (unsigned)(c.seed >> 32);
    P.dt = (R)c.delta_t;
    P.umax0 = (R)c.u_max[0];
    P.umax1 = (R)c.u_max[1];
    P.wheel_base = (R)c.wheel_base;
    P.beta = (R)softmin_beta(c);
    P.gamma = (R)(c.param_lambda * (1.0 - c.param_alpha));  // :74
    P.penalty = (R)c.collision_penalty;
    P.two_pi = (R)(2.0 * M_PI);
    const double det = c.sigma[0] * c.sigma[3] - c.sigma[1] * c.sigma[2];
    const double si[4] = {c.sigma[3] / det, -c.sigma[1] / det, -c.sigma[2] / det, c.sigma[0] / det};
    for (int i = 0; i < 4; ++i) {
        P.sinv[i] = (R)si[i];
        P.ws[i] = (R)c.stage_cost_weight[i];
        P.wt[i] = (R)c.terminal_cost_weight[i];
    }
    // vehicle outline, mppi_race_car_obstacle.py:256-264
    const double vw = c.vehicle_w * c.safety_margin, vl = c.vehicle_l * c.safety_margin;
    const double sx[9] = {-0.5 * vl, -0.5 * vl, 0.0, 0.5 * vl, 0.5 * vl, 0.5 * vl, 0.0, -0.5 * vl, -0.5 * vl};
    const double sy[9] = {0.0, 0.5 * vw, 0.5 * vw, 0.5 * vw, 0.0, -0.5 * vw, -0.5 * vw, -0.5 * vw, 0.0};
    for (int i = 0; i < 9; ++i) {
        P.shape_x[i] = (R)sx[i];
        P.shape_y[i] = (R)sy[i];
    }
    const double l00 = sqrt(c.sigma[0]), l10 = c.sigma[2] / l00, l11 = sqrt(c.sigma[3] - l10 * l10);
    P.chol[0] = (float)l00;
    P.chol[1] = (float)l10;
    P.chol[2] = (float)l11;
    P.ref = (const R *)sc0.ref;
    P.obs = (const R *)sc0.obs;
    P.obs_motion = c.obstacle_motion ? 1 : 0;  // (2 and 3, the learned scene and fleet handles, are 1 in here; the carriers below overwrite it)
    P.iter0 = sc0.iter0;
    P.scenes = h->d_scenes;
    P.u = (const R *)h->d_u.get();
    P.eps = noise;
    P.S = (R *)h->d_S.get();
    P.pout = h->d_pout;
    P.st = h->d_st;
    P.noise_stream = c.noise_stream;
    P.slots = h->slots;
    P.n_agents = h->B;
    P.layout = h->layout;
    P.heads = (R *)h->d_heads.get();
    // the kernels that can resolve the sequential index in one launch -- while that index can still move: after that the
    // lean kernels serve
    P.hyp = index_can_move(h);
    P.lb_seq = 0;
    P.hyp_slots = h->d_hyp_slots;
    // (a composed handle with two or more of the three below: the one table that points at all of them, and the launch's
    // staged bytes of plans and tracks; with fewer it takes the single-ingredient carrier like any other handle)
    if (learned_scene(h)) {  // (one carrier whatever the handle holds: the table built from the owners that exist, and the footprint word)
        set_scene_learned<R>(P, h->d_scene.get(), h->grid_footprint);
        return P;
    }
    if (scene_form(h)) {
        set_scene<R>(P, h->d_scene.get(), h->fleet_plan ? h->B : 0, max_tracks(h));
        return P;
    }
    if (h->fleet_plan) {  // (the threshold as make_fleet packs it for a mate row)
        const double thr = c.obstacle_model == MPPI_OBSTACLE_CIRCLE ? 0.5 * c.safety_margin + c.fleet_radius : c.fleet_radius;
        set_fleet_plan<R>(P, h->d_plans, (R)(thr * thr));
    }
    // (obstacle tracks, beside plans or a grid only behind the table above: the descriptors and the launch's staged bytes, sized
    // by the largest set)
    if (const int n_max = max_tracks(h)) set_tracks<R>(P, h->d_tracks, n_max);
    // (a cost grid, likewise: the descriptors)
    if (h->any_grid) set_grids<R>(P, h->d_grids.get());
    return P;
}

// Fleet handles: the arguments of the k_fleet_rows launch at the front of a slot (count = 1) or of the refresh in front of a
// getter or an mppi_eval_* call (count = 0: the clearance records stay).  A mate's threshold is packed as set_circles packs a
// circle of radius fleet_radius; dt is rounded as KParams::dt is.
static FleetParams make_fleet(const mppi_handle *h, int count) {
    const mppi_config &c = h->cfg;
    FleetParams F;
    memset(&F, 0, sizeof(F));
    F.scenes = h->d_scenes;
    F.st = h->d_st;
    F.u = h->d_u;
    F.clear = h->d_clear;
    F.n_agents = h->B;
    F.T = c.T;
    F.model = kernel_model(c);
    F.count = count;
    F.dt = h->f64 ? c.delta_t : (double)(float)c.delta_t;
    F.umax0 = c.u_max[0];
    const double thr = c.obstacle_model == MPPI_OBSTACLE_CIRCLE ? 0.5 * c.safety_margin + c.fleet_radius : c.fleet_radius;
    F.thr2 = thr * thr;
    F.contact = 2.0 * c.fleet_radius;
    if (h->fleet_plan) {
        F.plans = h->d_plans;
        F.clamp_rollout = c.clamp_rollout;
        F.umax1 = c.u_max[1];
        F.wheel_base = c.wheel_base;
    }
    return F;
}

// The launch at the front of a fleet handle's slot, or the refresh in front of a getter or an mppi_eval_* call: the mates' rows
// (k_fleet_rows) or their plans -- k_fleet_plan with the analytic dynamics, and on a learned fleet handle (obstacle_motion = 3)
// the plan kernels of mppi_mlp.hip, every agent's nominal controls through its own model.  P: the parameters of the rollout
// behind it (the learned plan kernels read the agents' states, controls and clamp from them).
template <typename R> static void launch_fleet_front(const mppi_handle *h, const KParams<R> &P, int count, hipStream_t s) {
    if constexpr (sizeof(R) == 4)
        if (learned_fleet(h) && h->fleet_plan) {
            launch_fleet_plan_mlp(P, h->mlp, h->d_models, make_fleet(h, count), s);
            return;
        }
    launch_fleet_rows<R>(make_fleet(h, count), s);
}

// the softmin rate as the records carry it
static double record_beta(const mppi_handle *h) {
    const double beta = softmin_beta(h->cfg);
    return h->f64 ? beta : (double)(float)beta;  // the block partials were scaled with the f32 rate
}

// abi_recs / n_recs: the caller's records in the ABI layout (the split step's, the gathered ones); null: the records, their
// count and the look-back fields are the slot plan's (plan_slot)
static FinalizeParams make_finalize(const mppi_handle *h, int plant, const void *abi_recs = nullptr, int n_recs = 0) {
    const mppi_config &c = h->cfg;
    FinalizeParams F;
    memset(&F, 0, sizeof(F));
    F.T = c.T;
    F.K = c.K;
    F.n_part = n_recs;
    F.filter_mode = c.filter_mode;
    F.filter_window = c.filter_window;
    F.clamp_u = c.clamp_u_after_update;
    F.raise_at_path_end = c.raise_at_path_end;
    F.model = kernel_model(c);
    F.sequential = c.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL;
    F.plant = plant;
    const AgentScene sc0 = scene_of(h, 0);
    F.n_ref = sc0.n_ref;
    F.window = c.search_window;
    F.is_f64 = h->f64;
    // (2: every agent counts, also one without rows of its own -- its mates' plans, its obstacle tracks or its cost grid)
    F.count_hits = h->fleet_plan || (h->B > 1 && (max_tracks(h) > 0 || h->any_grid)) ? 2 : any_obstacles(h);
    F.beta = record_beta(h);
    F.dt = c.delta_t;
    F.wheel_base = c.wheel_base;
    F.umax0 = c.u_max[0];
    F.umax1 = c.u_max[1];
    F.partials = abi_recs;
    F.heads = h->d_heads;  // (unused for the ABI layout)
    F.u = h->d_u;
    F.u_out = h->d_u;
    F.u_before = h->d_uhist;
    F.ref = sc0.ref;
    F.scenes = h->d_scenes;
    F.pout = h->d_pout;
    F.st = h->d_st;
    F.st_out = h->d_st;
    F.res = h->d_res;
    F.slots = h->slots;
    F.n_agents = h->B;
    F.res_stride = h->res_bytes;
    F.u0_trace = nullptr;
    F.hyp_slots = h->d_hyp_slots;
    F.lb_seq = 0;
    F.pad_lb = 0;
    return F;
}

// Timing (mppi_enable_timing): every launch group of a slot is bracketed by a pair of events on the
// launch stream -- [rollout] [reduce/merge] [finalize] -- plus one EMPTY pair that measures what a pair
// of hipEventRecord costs on this stream (several microseconds); mppi_last_kernel_ms reports the
// averages with that calibration subtracted.
constexpr int EV_PER_SLOT = 8;
constexpr size_t EV_MAX = 8u * 200000u;

static hipEvent_t next_event(mppi_handle *h) {
    if (h->ev_used == h->ev.size()) hipEventCreate(h->ev.emplace_back().put());
    return h->ev[h->ev_used++];
}

static bool timing_on(const mppi_handle *h) { return h->timing && h->ev_used + EV_PER_SLOT <= EV_MAX; }

// the peer-to-peer exchange as mppi_comm_connect wired it (x_seq: drawn per launch)
static void wire_exchange(const mppi_handle *h, FinalizeParams &F) {
    if (h->x_nranks <= 1) return;
    F.x_nranks = h->x_nranks;
    F.x_rank = h->x_rank;
    F.x_timeout = h->x_timeout;
    F.x_peers = h->d_xpeers;
    F.x_err = h->d_xerr;
}

// the rollout launch of this handle (the learned model: f32 handles only, mppi_create refuses the rest)
template <typename R> static RolloutPlan front_plan(const mppi_handle *h, const KParams<R> &P) {
    if constexpr (sizeof(R) == 4)
        if (h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP) return plan_mlp(P, h->mlp, h->sw, nullptr, learned_fleet(h));
    return plan_rollout<R>(P, h->fused, h->sw, h->grid_footprint == MPPI_GRID_FOOTPRINT_OUTLINE);
}

// One iteration slot, resolved once and executed many times: rollout (-> reduce) (-> merge) -> its reader.  The reader is
// k_finalize -- local, or with the peer-to-peer exchange once mppi_comm_connect has wired it -- or, for the carriers that
// exchange records outside the slot (split step, RCCL), the k_merge that writes this rank's ONE record {rho, eta, eta2,
// W[T][2]} in f64; their finalize over the gathered records is plan_finalize(..., abi_recs) alone.  plan_slot is a pure
// function of P, the handle's switches and wiring and the carrier; it aims F at the records the finalize reads.  Nothing in
// it depends on what changes from slot to slot: the look-back tag, the exchange sequence number, use_args, res / seq.
struct SlotPlan {
    RolloutPlan front;      // front.lookback: the slot draws a tag and k_finalize<..., HYPK> reads the words
    bool reduce = false;    // k_reduce follows the rollout (k_rollout)
    int n_merges = 0;       // k_merge launches: the tree's (merge_tree), then the one that writes the rank's record
    MergeStep merge[2];
    double beta = 0.0;      // record_beta: the rate the merges scale with
    KernelLaunch fin;       // (none with rank_record)
};
template <typename R>
static SlotPlan plan_slot(const mppi_handle *h, const KParams<R> &P, FinalizeParams *F, double *rank_record = nullptr) {
    SlotPlan sp;
    sp.front = front_plan<R>(h, P);
    sp.reduce = h->cfg.model != MPPI_MODEL_DIFFDRIVE_MLP && !h->fused;
    sp.beta = record_beta(h);
    const void *recs = h->d_partials, *heads = h->d_heads;
    const MergeTree tree = merge_tree(sp.front.records, rank_record == nullptr);
    if (tree.group) {
        sp.merge[sp.n_merges++] = plan_merge<R>(recs, heads, sp.front.records, tree.group, h->cfg.T, h->d_partials2, h->d_heads2);
        recs = h->d_partials2;
        heads = h->d_heads2;
    }
    if (rank_record) {
        sp.merge[sp.n_merges++] = plan_merge<R>(recs, heads, tree.n_out, tree.n_out, h->cfg.T, rank_record, nullptr);
        return sp;
    }
    F->partials = recs;
    F->heads = heads;
    F->n_part = tree.n_out;
    F->hyp = sp.front.lookback;
    F->hyp_blocks = sp.front.records;
    wire_exchange(h, *F);
    sp.fin = plan_finalize<R>(*F, false, sp.front.lookback);
    return sp;
}

// the plan's launches up to its reader: [rollout] [reduce / merge].  A fleet handle: k_fleet_rows (plan mode: k_fleet_plan) leads the slot, inside the
// rollout's event pair (mppi_last_kernel_ms out[0]) and outside the launch counters (mppi_get_counters)
template <typename R> static void launch_records(mppi_handle *h, const SlotPlan &sp, const KParams<R> &P, hipStream_t s, bool tm) {
    if (tm) hipEventRecord(next_event(h), s);
    if (h->fleet) launch_fleet_front<R>(h, P, 1, s);
    h->n_rollout_launches += h->rollout_repeats;
    for (int rep = 0; rep < h->rollout_repeats; ++rep) {
        if constexpr (sizeof(R) == 4)
            if (h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP) {
                launch_mlp(sp.front, P, h->mlp, h->d_models, h->d_partials, nullptr, s);
                continue;
            }
        launch_rollout<R>(sp.front, P, h->d_partials, s);
    }
    h->rollout_kernel = sp.front.k.name;
    if (tm) hipEventRecord(next_event(h), s);
    if (tm) hipEventRecord(next_event(h), s);
    if (sp.reduce) launch_reduce<R>(P, h->d_partials, sp.front.records, s);
    for (int i = 0; i < sp.n_merges; ++i) launch_merge<R>(sp.merge[i], h->cfg.T, sp.beta, s);
    if (tm) hipEventRecord(next_event(h), s);
}

// [finalize] [empty]
static void launch_back(mppi_handle *h, const KernelLaunch &fin, const FinalizeParams &F, hipStream_t s, bool tm) {
    if (tm) hipEventRecord(next_event(h), s);
    ++h->n_finalize_launches;
    launch_finalize(fin, F, s);
    if (tm) hipEventRecord(next_event(h), s);
    if (tm) hipEventRecord(next_event(h), s);  // empty pair: the cost of the bracketing itself
    if (tm) hipEventRecord(next_event(h), s);
}

// One execution of a slot plan that ends in k_finalize.  Per slot: the exchange's sequence number, the look-back tag, the
// optional events, the rollout_repeats loop, the launches and the counters.
template <typename R>
static void launch_slot(mppi_handle *h, const SlotPlan &sp, const KParams<R> &P, FinalizeParams F, hipStream_t s) {
    const bool tm = timing_on(h);
    if (F.x_nranks > 1) F.x_seq = ++h->xseq;
    if (sp.front.lookback) {  // the look-back words of this launch pair carry its own tag (lb_tag)
        if ((++h->lb_seq & 0xffffffu) == 0u) ++h->lb_seq;
        KParams<R> Pl = P;
        Pl.lb_seq = F.lb_seq = h->lb_seq;
        launch_records<R>(h, sp, Pl, s, tm);
    } else {
        launch_records<R>(h, sp, P, s, tm);
    }
    launch_back(h, sp.fin, F, s, tm);
}

static void collect_timing(mppi_handle *h) {
    double acc[4] = {0, 0, 0, 0};
    const size_t slots = h->ev_used / EV_PER_SLOT;
    for (size_t i = 0; i < slots; ++i)
        for (int j = 0; j < 4; ++j) {
            float ms = 0;
            hipEventElapsedTime(&ms, h->ev[EV_PER_SLOT * i + 2 * j], h->ev[EV_PER_SLOT * i + 2 * j + 1]);
            acc[j] += ms;
        }
    const double cal = slots ? acc[3] / slots : 0.0;
    for (int j = 0; j < 3; ++j) {
        const double v = slots ? acc[j] / slots - cal : 0.0;
        h->last_ms[j] = (float)(v > 0 ? v : 0);
    }
    h->last_ms[3] = (float)cal;
}

static int check_ready(mppi_handle *h, const char *who) {
    if (!h) return MPPI_ERR_BAD_ARG;
    for (int a = 0; a < h->B; ++a) {
        const AgentScene sc = scene_of(h, a);
        if (!sc.ref || sc.n_ref < 1) {
            if (h->B > 1) FAIL(h, MPPI_ERR_STATE, "%s: ref_path of agent %d has not been set", who, a);
            FAIL(h, MPPI_ERR_STATE, "%s: ref_path has not been set", who);
        }
        if (sc.n_obs > 0 && !sc.obs) FAIL(h, MPPI_ERR_STATE, "%s: obstacles not uploaded", who);
    }
    if (h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP)
        for (int a = 0; a < h->B; ++a)
            if (!has_model(h, a)) {
                if (h->B > 1) FAIL(h, MPPI_ERR_STATE, "%s: agent %d has no model (mppi_set_mlp / mppi_set_agent_mlp)", who, a);
                FAIL(h, MPPI_ERR_STATE, "%s: mppi_set_mlp has not been called", who);
            }
    return MPPI_OK;
}

// entry points that serve one agent only (the host-in-the-loop and split steps, visualisation, the exchange)
#define SINGLE_AGENT_ONLY(h, who)                                                                                     \
    do {                                                                                                              \
        if ((h)->B > 1) FAIL(h, MPPI_ERR_UNSUPPORTED, "%s serves single-agent handles (n_agents = %d)", who, (h)->B); \
    } while (0)

static void fill_stats(mppi_handle *h, mppi_stats *stats) {
    if (!stats) return;
    if (h->timing && h->ev_used >= EV_PER_SLOT) {  // kernel_us: the window's averages as of this call
        if (hipEventSynchronize(h->ev[h->ev_used - 1]) == hipSuccess) collect_timing(h);
        else (void)hipGetLastError();
    }
    const StepResult *r = h->h_res;
    stats->rho = r->rho;
    stats->eta = r->eta;
    stats->ess = r->ess;
    stats->idx_start = r->idx_start;
    stats->idx_after = r->idx_after;
    stats->path_end = r->path_end;
    stats->rounds = r->rounds;
    stats->iteration = r->iter;
    stats->n_collided = r->n_collided;
    stats->reserved = 0;
    stats->iter_us = h->last_iter_us;
    stats->kernel_us = h->timing ? 1e3 * ((double)h->last_ms[0] + h->last_ms[1] + h->last_ms[2]) : 0.0;
}

// The x0 call (mppi_differential_drive.py:96-99 / mppi_race_car.py:61): nearest waypoint of the observed state
// in the window that starts at prev_way_point_idx, first minimum.  Same f64 arithmetic as k_set_state, on the
// host so that the synchronous step needs no extra launch; the result travels as a kernel argument.
static int host_x0_call(const mppi_handle *h, const double *x0) {
    const int p = h->idx, n = h->n_ref, w = h->cfg.search_window;
    int best_j = 0;
    double best = INFINITY;
    for (int j = 0; j < w && p + j < n; ++j) {
        const double dx = x0[0] - h->ref_host[4 * (size_t)(p + j)], dy = x0[1] - h->ref_host[4 * (size_t)(p + j) + 1];
        const double d = dx * dx + dy * dy;
        if (d < best) { best = d; best_j = j; }
    }
    return p + best_j;
}

// The result path, first half: `bytes` of the device-side result (one agent's, or every agent's of a batched handle) copied
// into h_res behind the launches on s, and the stream synchronised.
static int fetch_result(mppi_handle *h, size_t bytes, hipStream_t s, bool check_launches = true) {
    HIPCHECK(h, hipMemcpyAsync(h->h_res, h->d_res, bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (check_launches) HIPCHECK(h, hipGetLastError());
    return MPPI_OK;
}

// wait for the result of the launches just enqueued: poll the completion word the finalize kernel writes into
// mapped host memory (saves the device-to-host copy launch and the stream synchronisation), or copy + synchronise
static int wait_result(mppi_handle *h, long long seq, hipStream_t s) {
    if (seq) {
        volatile long long *flag = &h->h_res->seq;
        // The poll saves a copy launch and a stream synchronisation (~7 us) on short calls, and on long ones the wake-up of
        // hipStreamSynchronize (up to 0.4 ms per call on some boxes: 200 iterations per call 11.0 us per iteration against
        // 9.2 at 50).  So the host spins for up to 20 ms -- two episodes of the reference driver's run at config 2 -- and only
        // then hands the wait to the runtime (config 5's tens of milliseconds per call; it also surfaces a failed launch).
        // (Sleeping through an ESTIMATE of the call's duration was tried: the pace of the previous call is the wrong
        // estimate across a phase change, and an overslept call costs more than the spin saves.)
        const double t0 = now_s();
        for (long long spins = 0; *flag != seq; ++spins) {
            __builtin_ia32_pause();
            if ((spins & 1023) == 1023 && now_s() - t0 > 0.020) {
                HIPCHECK(h, hipStreamSynchronize(s));
                HIPCHECK(h, hipGetLastError());
                if (*flag != seq) FAIL(h, MPPI_ERR_HIP, "the finalize kernel never published its result");
                break;
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        return MPPI_OK;
    }
    return fetch_result(h, h->res_bytes, s);
}

// What the iteration just enqueued drew its noise from (mppi_rollout_viz replays it).  observed_state: the iteration took its
// state from the caller, so the next closed-loop call has to make its own x0 call.
static void note_noise(mppi_handle *h, const float *eps, bool observed_state) {
    h->last_eps = eps;
    if (observed_state) h->dev_loop_primed = false;
}

// The result path, second half: the finished result in h_res becomes the handle's state and the caller's outputs -- waypoint
// index, stats, the kernel's status as an error code, then the iteration counter and the controls.  An iteration refused at
// the end of the path has moved the index but is not counted.  Every entry point that ends an iteration on the host calls
// this; what the entry points do differently (kept as it was) comes in through `keep`.
enum : unsigned {
    KEEP_IDX_VALID = 1u,  // leave idx_valid as it is (otherwise: the index is the host's again)
    KEEP_GOING = 2u,      // ignore the kernel's status
};
static int adopt_result(mppi_handle *h, unsigned keep, double *u_out, double *u0_out, mppi_stats *stats) {
    const StepResult *res = h->h_res;
    h->idx = res->idx_after;
    if (!(keep & KEEP_IDX_VALID)) h->idx_valid = true;
    fill_stats(h, stats);
    if (!(keep & KEEP_GOING)) {
        // (only a finalize launch that carries the peer-to-peer exchange writes this status: k_finalize, MODE 2)
        if (res->status == STATUS_EXCHANGE_FAILED)
            FAIL(h, MPPI_ERR_COMM, "peer-to-peer exchange: a rank did not arrive within the timeout");
        if (res->status == STATUS_PATH_END) FAIL(h, MPPI_ERR_PATH_END, "[ERROR] Reached the end of the reference path.");
    }
    h->iter = res->iter;
    if (u_out) memcpy(u_out, reinterpret_cast<const double *>(h->h_res + 1), sizeof(double) * 2 * h->cfg.T);  // u[T][2] follows the header
    if (u0_out) { u0_out[0] = res->u0[0]; u0_out[1] = res->u0[1]; }
    return MPPI_OK;
}

// (the RCCL carrier of a K-sharded handle, further down)
template <typename R>
static int step_rccl(mppi_handle *h, const double *x0, const double *x0_dev, const float *eps, double *u_out, double *u0_out,
                     mppi_stats *stats, hipStream_t s);
template <typename R>
static int closed_loop_rccl(mppi_handle *h, int n_iters, double *u0_trace, mppi_stats *stats, hipStream_t s);

// x0: host (the observed state travels as kernel arguments) or, when null, x0_dev: device memory (a small kernel moves
// it into the controller state and makes the x0 call)
template <typename R>
static int step_impl(mppi_handle *h, const double *x0, const double *x0_dev, const float *eps, double *u_out, double *u0_out,
                     mppi_stats *stats, hipStream_t s) {
    if (h->rccl_comm && h->x_nranks <= 1) return step_rccl<R>(h, x0, x0_dev, eps, u_out, u0_out, stats, s);
    const double t_call = now_s();
    KParams<R> P = make_params<R>(h, eps);
    FinalizeParams F = make_finalize(h, 0);
    const bool by_args = x0 && h->idx_valid && !h->sw.no_args;
    if (!x0) {
        if (!h->idx_valid) FAIL(h, MPPI_ERR_STATE, "mppi_step_device_x0 after an asynchronous split step: call mppi_sync_result first");
        launch_set_state_dev<R>(P, x0_dev, h->nx, s);
    } else if (by_args) {
        P.use_args = F.use_args = 1;
        P.c_arg = F.c_arg = host_x0_call(h, x0);
        P.hyp = h->hyp && !at_path_end(h, P.c_arg);
        for (int i = 0; i < 4; ++i) P.x0_arg[i] = F.x0_arg[i] = x0[i];
    } else {
        launch_set_state<R>(P, x0, s);
    }
    if (!h->sw.no_poll) F.res = h->res_mapped;
    const SlotPlan sp = plan_slot<R>(h, P, &F);  // (the speculation rounds reuse it)
    for (int round = 0;; ++round) {
        F.seq = !h->sw.no_poll ? ++h->seq : 0;
        launch_slot<R>(h, sp, P, F, s);
        HIPCHECK(h, hipGetLastError());  // a refused launch would otherwise show only as the poll's timeout
        int rc = wait_result(h, F.seq, s);
        if (rc) return rc;
        if (h->h_res->status != STATUS_NEED_ROUND) break;
        if (round > h->cfg.K + 1) FAIL(h, MPPI_ERR_STATE, "waypoint speculation did not converge");
        P.use_args = 0;  // repair rounds take the state the finalize kernel left in *st
    }
    note_noise(h, eps, true);
    h->last_iter_us = 1e6 * (now_s() - t_call);
    return adopt_result(h, 0, u_out, u0_out, stats);
}

extern "C" int mppi_step(mppi_handle *h, const double *x0, const float *eps, double *u_out, double *u0_out,
                         mppi_stats *stats, void *stream) {
    int rc = check_ready(h, "mppi_step");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_step");
    if (!x0) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_step: x0 is null");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    double x[4] = {0, 0, 0, 0};
    for (int i = 0; i < h->nx; ++i) x[i] = x0[i];
    return with_real(h, [&](auto r) { return step_impl<decltype(r)>(h, x, nullptr, eps, u_out, u0_out, stats, (hipStream_t)stream); });
}

extern "C" int mppi_step_device_x0(mppi_handle *h, const double *x0_device, const float *eps, double *u_out, double *u0_out,
                                   mppi_stats *stats, void *stream) {
    int rc = check_ready(h, "mppi_step_device_x0");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_step_device_x0");
    if (!x0_device) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_step_device_x0: x0 is null");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) { return step_impl<decltype(r)>(h, nullptr, x0_device, eps, u_out, u0_out, stats, (hipStream_t)stream); });
}

extern "C" int mppi_partial_len(const mppi_handle *h, int32_t *n) {
    if (!h || !n) return MPPI_ERR_BAD_ARG;
    *n = partial_len(h->cfg.T);
    return MPPI_OK;
}

template <typename R>
static int begin_impl(mppi_handle *h, const double *x0, const float *eps, double *partial, hipStream_t s) {
    KParams<R> P = make_params<R>(h, eps);
    // closed loop on the device: the previous end_async already made the x0 call for the new state
    if (x0 || !h->dev_loop_primed) launch_set_state<R>(P, x0, s);
    h->dev_loop_primed = x0 == nullptr;
    h->slot_timed = timing_on(h);
    launch_records<R>(h, plan_slot<R>(h, P, nullptr, partial), P, s, h->slot_timed);
    HIPCHECK(h, hipGetLastError());
    note_noise(h, eps, false);  // (dev_loop_primed: set above)
    h->begun = true;
    return MPPI_OK;
}

extern "C" int mppi_step_begin(mppi_handle *h, const double *x0, const float *eps, double *partial, void *stream) {
    int rc = check_ready(h, "mppi_step_begin");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_step_begin");
    if (!partial) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_step_begin: null argument");
    if (h->cfg.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "the split step needs MPPI_WAYPOINT_FROZEN (no cross-sample waypoint state)");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    double x[4] = {0, 0, 0, 0};
    if (x0)
        for (int i = 0; i < h->nx; ++i) x[i] = x0[i];
    return with_real(h, [&](auto r) { return begin_impl<decltype(r)>(h, x0 ? x : nullptr, eps, partial, (hipStream_t)stream); });
}

extern "C" int mppi_step_end(mppi_handle *h, const double *partials, int32_t nranks, double *u_out, double *u0_out,
                             mppi_stats *stats, void *stream) {
    int rc = check_ready(h, "mppi_step_end");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_step_end");
    if (!partials || nranks < 1 || nranks > MERGE_MAX_RECORDS)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_step_end: bad partials/nranks (1..%d)", MERGE_MAX_RECORDS);
    if (!h->begun) FAIL(h, MPPI_ERR_STATE, "mppi_step_end without mppi_step_begin");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const FinalizeParams F = make_finalize(h, 0, partials, nranks);
    with_real(h, [&](auto r) { launch_back(h, plan_finalize<decltype(r)>(F, true, false), F, s, h->slot_timed); });
    if ((rc = fetch_result(h, h->res_bytes, s))) return rc;
    h->begun = false;
    h->dev_loop_primed = false;  // no plant ran: the next device-state step makes its own x0 call
    // kept: after an asynchronous split step this does not hand the index back to the host (idx_valid stays as it is)
    return adopt_result(h, KEEP_IDX_VALID, u_out, u0_out, stats);
}

extern "C" int mppi_step_end_async(mppi_handle *h, const double *partials, int32_t nranks, void *stream) {
    int rc = check_ready(h, "mppi_step_end_async");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_step_end_async");
    if (!partials || nranks < 1 || nranks > MERGE_MAX_RECORDS)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_step_end_async: bad partials/nranks (1..%d)", MERGE_MAX_RECORDS);
    if (!h->begun) FAIL(h, MPPI_ERR_STATE, "mppi_step_end_async without mppi_step_begin");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    const FinalizeParams F = make_finalize(h, 1, partials, nranks);  // plant on: the state advances on the device
    with_real(h, [&](auto r) { launch_back(h, plan_finalize<decltype(r)>(F, true, false), F, (hipStream_t)stream, h->slot_timed); });
    HIPCHECK(h, hipGetLastError());
    h->begun = false;
    h->idx_valid = false;  // the waypoint index now advances on the device until mppi_sync_result
    return MPPI_OK;
}

extern "C" int mppi_sync_result(mppi_handle *h, double *u_out, double *u0_out, mppi_stats *stats, void *stream) {
    if (!h) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    // kept: no hipGetLastError after the synchronise (a launch that failed shows at the next call that asks)
    if (int rc = fetch_result(h, h->res_bytes, (hipStream_t)stream, false)) return rc;
    return adopt_result(h, 0, u_out, u0_out, stats);
}

extern "C" int mppi_get_costs(mppi_handle *h, double *S) {
    if (!h || !S) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    return download_real(h, S, h->d_S, (size_t)h->B * h->cfg.K);  // [n_agents][K]
}

extern "C" int mppi_get_weights(mppi_handle *h, double *w) {
    if (!h || !w) return MPPI_ERR_BAD_ARG;
    SINGLE_AGENT_ONLY(h, "mppi_get_weights");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (!h->d_w) HIPCHECK(h, h->d_w.alloc(sizeof(double) * h->cfg.K));
    with_real(h, [&](auto r) {
        using R = decltype(r);
        launch_weights<R>(make_params<R>(h, nullptr), h->h_res->rho, h->h_res->eta, h->d_w, nullptr);
    });
    HIPCHECK(h, hipDeviceSynchronize());
    HIPCHECK(h, hipMemcpy(w, h->d_w, sizeof(double) * h->cfg.K, hipMemcpyDeviceToHost));
    return MPPI_OK;
}

extern "C" int mppi_sample_epsilon(mppi_handle *h, int64_t iteration, float *eps_out, void *stream) {
    if (!h || !eps_out || iteration < 0) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    KParams<float> P = make_params<float>(h, nullptr);
    for (int a = 0; a < h->B; ++a)  // [n_agents][K][T][2]: agent a draws with stream word noise_stream + a
        launch_sample(P.seed_lo, P.seed_hi, (unsigned)iteration, h->cfg.K, h->cfg.T, h->cfg.k_offset, P.chol,
                      eps_out + (size_t)a * h->cfg.K * h->cfg.T * 2, (hipStream_t)stream, (unsigned)(h->cfg.noise_stream + a));
    HIPCHECK(h, hipGetLastError());
    return MPPI_OK;
}

extern "C" int mppi_set_noise_ring(mppi_handle *h, const float *eps_ring, int32_t n_slots) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!eps_ring || n_slots == 0) {  // back to the in-kernel sampler
        h->noise_ring = nullptr;
        h->noise_slots = 0;
        return MPPI_OK;
    }
    if (n_slots < 1 || (n_slots & (n_slots - 1)) != 0)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_noise_ring: n_slots must be a power of two (got %d)", n_slots);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, eps_ring) != hipSuccess || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeUnregistered ||
        at.device != h->cfg.device) {
        (void)hipGetLastError();
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_noise_ring: the ring must be device memory on the handle's GPU (device %d)", h->cfg.device);
    }
    h->noise_ring = eps_ring;
    h->noise_slots = n_slots;
    return MPPI_OK;
}

extern "C" int mppi_rollout_viz(mppi_handle *h, float *optimal_traj, float *sampled_traj, void *stream) {
    int rc = check_ready(h, "mppi_rollout_viz");
    if (rc) return rc;
    SINGLE_AGENT_ONLY(h, "mppi_rollout_viz");
    if (h->iter < 1) FAIL(h, MPPI_ERR_STATE, "mppi_rollout_viz before the first mppi_step");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    with_real(h, [&](auto r) {
        using R = decltype(r);
        const KParams<R> P = make_params<R>(h, h->last_eps);
        const R *hist = (const R *)h->d_uhist.get(), *hist_after = hist + 2 * h->cfg.T;
        if constexpr (sizeof(R) == 4)  // (the learned model: f32 handles only, checked at create)
            if (h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP)
                return launch_viz_mlp(P, h->mlp, h->sw, hist, hist_after, h->iter - 1, optimal_traj, sampled_traj, (hipStream_t)stream);
        launch_viz<R>(P, hist, hist_after, h->iter - 1, optimal_traj, sampled_traj, (hipStream_t)stream);
    });
    HIPCHECK(h, hipGetLastError());
    return MPPI_OK;
}


// ------------------------------------------------------------------------------------------
// RCCL carrier of the same exchange inside the library (include/mppi_hip.h, mppi_comm_init):
// one ncclAllGather of the per-rank record per iteration, enqueued on the caller's stream between the rollout and the
// finalize launches -- no host code per iteration beyond the three enqueues.  librccl.so.1 is resolved at run time
// (dlopen by soname: in a PyTorch-ROCm process that is the copy torch has already loaded), so the library has no
// link-time dependency on RCCL and single-GPU users never load it.
// ------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, RcclUniqueId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
};
RcclApi rccl_load() {
    RcclApi a;
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
        a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (a.lib) break;
    }
    if (!a.lib) {
        a.why = std::string("librccl.so.1 could not be loaded: ") + dlerror();
        return a;
    }
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) {
        a.why = "librccl.so.1 lacks an expected symbol";
        a.lib = nullptr;
    }
    return a;
}
RcclApi &rccl_api() {
    static RcclApi a = rccl_load();  // (one load per process; the language makes the initialisation thread-safe)
    return a;
}
}  // namespace

static void rccl_release(mppi_handle *h) {
    if (h->rccl_comm) rccl_api().CommDestroy(h->rccl_comm);
    (void)h->d_rccl_part.reset();
    (void)h->d_rccl_gath.reset();
    h->rccl_comm = nullptr;
    h->rccl_nranks = 0;
}

#define RCCLCHECK(h, call)                                                                                   \
    do {                                                                                                     \
        const int _r = (call);                                                                               \
        if (_r != 0) FAIL(h, MPPI_ERR_COMM, "%s failed: %s", #call, rccl_api().GetErrorString(_r));          \
    } while (0)

extern "C" int mppi_comm_unique_id_bytes(void) { return (int)sizeof(RcclUniqueId); }

extern "C" int mppi_comm_unique_id(void *id_out) {
    if (!id_out) return MPPI_ERR_BAD_ARG;
    RcclApi &a = rccl_api();
    if (!a.lib) {
        g_create_error = a.why;
        return MPPI_ERR_COMM;
    }
    if (a.GetUniqueId(id_out) != 0) {
        g_create_error = "ncclGetUniqueId failed";
        return MPPI_ERR_COMM;
    }
    return MPPI_OK;
}

extern "C" int mppi_comm_init(mppi_handle *h, const void *unique_id, int32_t rank, int32_t nranks) {
    if (!h || !unique_id) return MPPI_ERR_BAD_ARG;
    SINGLE_AGENT_ONLY(h, "mppi_comm_init");
    if (nranks < 1 || nranks > MERGE_MAX_RECORDS || rank < 0 || rank >= nranks)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_comm_init: rank %d of %d (1..%d ranks)", rank, nranks, MERGE_MAX_RECORDS);
    if (h->cfg.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "the exchange needs MPPI_WAYPOINT_FROZEN (no cross-sample waypoint state)");
    RcclApi &a = rccl_api();
    if (!a.lib) FAIL(h, MPPI_ERR_COMM, "mppi_comm_init: %s", a.why.c_str());
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    rccl_release(h);
    RcclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    RCCLCHECK(h, a.CommInitRank(&h->rccl_comm, nranks, id, rank));
    const size_t len = (size_t)partial_len(h->cfg.T);
    HIPCHECK(h, h->d_rccl_part.alloc(sizeof(double) * len));
    HIPCHECK(h, h->d_rccl_gath.alloc(sizeof(double) * len * nranks));
    h->rccl_rank = rank;
    h->rccl_nranks = nranks;
    return MPPI_OK;
}

// The device buffer of the closed loop's u0 trace, grown to n_iters rows.  *rows: where the finalize kernel, which indexes by
// the absolute iteration, finds row h->iter.
static int trace_rows(mppi_handle *h, int n_iters, double **rows) {
    if (h->trace_cap < n_iters) {
        h->trace_cap = 0;
        HIPCHECK(h, h->d_trace.reset());
        HIPCHECK(h, h->d_trace.alloc(sizeof(double) * 2 * n_iters));
        h->trace_cap = n_iters;
    }
    *rows = h->d_trace.get() - 2 * h->iter;
    return MPPI_OK;
}

// One iteration on the stream with the collective in the middle: rollout -> this rank's record -> ncclAllGather ->
// finalize over the gathered records (identical on every rank, so u stays replicated without a broadcast).
template <typename R>
static int rccl_iteration(mppi_handle *h, const KParams<R> &P, int plant, double *u0_trace_dev, hipStream_t s) {
    const bool tm = timing_on(h);
    launch_records<R>(h, plan_slot<R>(h, P, nullptr, h->d_rccl_part), P, s, tm);
    RCCLCHECK(h, rccl_api().AllGather(h->d_rccl_part, h->d_rccl_gath, (size_t)partial_len(h->cfg.T), 8 /* ncclFloat64 */,
                                      h->rccl_comm, s));
    FinalizeParams F = make_finalize(h, plant, h->d_rccl_gath, h->rccl_nranks);
    F.u0_trace = u0_trace_dev;
    launch_back(h, plan_finalize<R>(F, true, false), F, s, tm);
    return MPPI_OK;
}

// outputs of the last finished iteration -> host (copy + synchronise; the collective paces the stream anyway)
static int rccl_fetch(mppi_handle *h, double *u_out, double *u0_out, mppi_stats *stats, hipStream_t s) {
    HIPCHECK(h, hipGetLastError());
    if (int rc = fetch_result(h, h->res_bytes, s)) return rc;
    return adopt_result(h, 0, u_out, u0_out, stats);
}

template <typename R>
static int step_rccl(mppi_handle *h, const double *x0, const double *x0_dev, const float *eps, double *u_out, double *u0_out,
                     mppi_stats *stats, hipStream_t s) {
    const KParams<R> P = make_params<R>(h, eps);
    if (x0) launch_set_state<R>(P, x0, s);
    else launch_set_state_dev<R>(P, x0_dev, h->nx, s);  // the observed state in device memory (mppi_step_device_x0)
    if (int rc = rccl_iteration<R>(h, P, 0, nullptr, s)) return rc;
    note_noise(h, eps, true);
    // kept: this carrier leaves last_iter_us (mppi_stats::iter_us) as the last call of another path set it
    return rccl_fetch(h, u_out, u0_out, stats, s);
}

template <typename R>
static int closed_loop_rccl(mppi_handle *h, int n_iters, double *u0_trace, mppi_stats *stats, hipStream_t s) {
    const KParams<R> P = make_params<R>(h, nullptr);
    double *trace = nullptr;
    if (u0_trace)
        if (int rc = trace_rows(h, n_iters, &trace)) return rc;
    if (!h->dev_loop_primed) launch_set_state<R>(P, nullptr, s);  // (see closed_loop_impl)
    h->dev_loop_primed = false;
    for (int i = 0; i < n_iters; ++i)
        if (int rc = rccl_iteration<R>(h, P, 1, trace, s)) return rc;
    note_noise(h, nullptr, false);
    // kept: this carrier leaves last_iter_us, t_enqueue_s and t_loop_s (mppi_get_host_timing) alone
    if (int rc = rccl_fetch(h, nullptr, nullptr, stats, s)) return rc;
    if (u0_trace) HIPCHECK(h, hipMemcpy(u0_trace, h->d_trace, sizeof(double) * 2 * n_iters, hipMemcpyDeviceToHost));
    h->dev_loop_primed = true;  // the last finalize made the next iteration's x0 call
    return MPPI_OK;
}

// ------------------------------------------------------------------------------------------
// Peer-to-peer exchange of the per-rank softmin record (include/mppi_hip.h, mppi_comm_*)
// ------------------------------------------------------------------------------------------
extern "C" int mppi_comm_handle_bytes(void) { return (int)sizeof(hipIpcMemHandle_t); }

extern "C" int mppi_comm_close(mppi_handle *h) {
    if (!h) return MPPI_ERR_BAD_ARG;
    hipSetDevice(h->cfg.device);
    hipDeviceSynchronize();
    h->x_opened.clear();
    (void)h->d_xpeers.reset();
    (void)h->d_xerr.reset();
    (void)h->d_xok.reset();
    (void)h->xbuf.reset();
    h->x_nranks = h->x_export_nranks = 0;
    rccl_release(h);
    return MPPI_OK;
}

extern "C" int mppi_comm_export(mppi_handle *h, int32_t nranks, void *handle_out) {
    if (!h || !handle_out) return MPPI_ERR_BAD_ARG;
    SINGLE_AGENT_ONLY(h, "mppi_comm_export");
    if (nranks < 2 || nranks > XCHG_MAX_RANKS)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_comm_export: nranks must be 2..%d (got %d)", XCHG_MAX_RANKS, nranks);
    if (h->cfg.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "the exchange needs MPPI_WAYPOINT_FROZEN (no cross-sample waypoint state)");
    // the finalize kernel stages up to XCHG_LDS_RANKS rank records in LDS next to its merge workspace
    if (merge_lds_elems(h->cfg.T, h->cfg.filter_window, rsz(h)) * rsz(h) + sizeof(double) * XCHG_LDS_RANKS * xchg_rec_len(h->cfg.T) > 64 * 1024)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "the peer-to-peer exchange stages the rank records in LDS: horizon T=%d is too long for it "
                                      "(use the split step with a collective)", h->cfg.T);
    if (h->xbuf) mppi_comm_close(h);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    h->xbuf_bytes = 2 * xchg_slot_bytes(h->cfg.T, nranks);
    HIPCHECK(h, h->xbuf.alloc(h->xbuf_bytes));  // (fine-grained: a peer's stores are visible here without a cache writeback)
    HIPCHECK(h, hipMemset(h->xbuf, 0, h->xbuf_bytes));
    HIPCHECK(h, hipDeviceSynchronize());
    hipIpcMemHandle_t ipc;
    HIPCHECK(h, hipIpcGetMemHandle(&ipc, h->xbuf));
    memcpy(handle_out, &ipc, sizeof(ipc));
    h->x_export_nranks = nranks;
    return MPPI_OK;
}

extern "C" int mppi_comm_buffer(mppi_handle *h, void **device_ptr) {
    if (!h || !device_ptr) return MPPI_ERR_BAD_ARG;
    if (!h->xbuf) FAIL(h, MPPI_ERR_STATE, "mppi_comm_buffer before mppi_comm_export");
    *device_ptr = h->xbuf;
    return MPPI_OK;
}

extern "C" int mppi_comm_connect(mppi_handle *h, int32_t rank, int32_t nranks, const void *handles,
                                 void *const *local_ptrs) {
    if (!h || (!handles && !local_ptrs)) return MPPI_ERR_BAD_ARG;
    if (!h->xbuf || nranks != h->x_export_nranks)
        FAIL(h, MPPI_ERR_STATE, "mppi_comm_connect: call mppi_comm_export with the same nranks first");
    if (rank < 0 || rank >= nranks) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_comm_connect: rank %d of %d", rank, nranks);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    // The new wiring is built in local owners and moves into the handle once all of it stands: a failure on the way leaves
    // the previous wiring as it was and nothing behind.
    std::vector<char *> peers(nranks, nullptr);
    std::vector<IpcMap> opened;
    for (int r = 0; r < nranks; ++r) {
        if (r == rank) {
            peers[r] = h->xbuf;
        } else if (local_ptrs && local_ptrs[r]) {
            // a peer living in this process: its buffer must be device memory, and when it sits on ANOTHER GPU this
            // handle's device needs peer access to it (the IPC route below enables that lazily; a raw pointer does not)
            hipPointerAttribute_t at;
            memset(&at, 0, sizeof(at));
            if (hipPointerGetAttributes(&at, local_ptrs[r]) != hipSuccess || at.type == hipMemoryTypeHost ||
                at.type == hipMemoryTypeUnregistered) {
                (void)hipGetLastError();
                FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_comm_connect: local_ptrs[%d] is not device memory (pass the peer's mppi_comm_buffer)", r);
            }
            if (at.device != h->cfg.device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, h->cfg.device, at.device) != hipSuccess || !can)
                    FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_comm_connect: device %d cannot access rank %d's buffer on device %d "
                                                  "(no peer access: use the collective carrier)", h->cfg.device, r, at.device);
                const hipError_t pe = hipDeviceEnablePeerAccess(at.device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                    FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_comm_connect: hipDeviceEnablePeerAccess(%d) failed: %s", at.device,
                         hipGetErrorString(pe));
                (void)hipGetLastError();
            }
            peers[r] = (char *)local_ptrs[r];
        } else {
            if (!handles) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_comm_connect: no handle for rank %d", r);
            hipIpcMemHandle_t ipc;
            memcpy(&ipc, (const char *)handles + sizeof(ipc) * (size_t)r, sizeof(ipc));
            HIPCHECK(h, hipIpcOpenMemHandle(opened.emplace_back().put(), ipc, hipIpcMemLazyEnablePeerAccess));
            peers[r] = (char *)opened.back().get();
        }
    }
    DevBuf<char *> d_xpeers;
    DevBuf<int> d_xerr, d_xok;
    HIPCHECK(h, d_xpeers.alloc(sizeof(char *) * nranks));
    HIPCHECK(h, hipMemcpy(d_xpeers, peers.data(), sizeof(char *) * nranks, hipMemcpyHostToDevice));
    HIPCHECK(h, d_xerr.alloc(sizeof(int)));
    HIPCHECK(h, d_xok.alloc(sizeof(int)));
    HIPCHECK(h, hipMemset(d_xerr, 0, sizeof(int)));
    h->d_xpeers = std::move(d_xpeers);  // (connected before: the new wiring replaces the old one, whose mappings stay open
    h->d_xerr = std::move(d_xerr);      // until mppi_comm_close, as they always have)
    h->d_xok = std::move(d_xok);
    for (IpcMap &m : opened) h->x_opened.push_back(std::move(m));
    if (const long long ms = read_switches().exchange_timeout_ms; ms > 0) h->x_timeout = ms * 100000LL;  // the wall clock counts at 100 MHz
    h->x_rank = rank;
    h->x_nranks = nranks;
    h->xseq = 0;
    return MPPI_OK;
}

extern "C" int mppi_comm_probe(mppi_handle *h, void *stream) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (h->x_nranks <= 1) FAIL(h, MPPI_ERR_STATE, "mppi_comm_probe before mppi_comm_connect");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    FinalizeParams F = make_finalize(h, 0);
    wire_exchange(h, F);
    F.x_seq = ++h->xseq;
    launch_exchange_probe(F, h->d_xok, (hipStream_t)stream);
    int ok = 0;
    HIPCHECK(h, hipMemcpyAsync(&ok, h->d_xok, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHECK(h, hipStreamSynchronize((hipStream_t)stream));
    if (!ok) {
        HIPCHECK(h, hipMemset(h->d_xerr, 0, sizeof(int)));  // the caller may fall back and retry later
        FAIL(h, MPPI_ERR_COMM, "peer-to-peer exchange probe: a rank did not arrive within the timeout");
    }
    return MPPI_OK;
}

// GRAPH_SLOTS closed-loop iterations (rollout -> finalize, the device-resident plant, next x0 call) as an instantiated HIP
// graph, cached per handle and re-captured when a kernel argument changes.  Replayed, an iteration costs the host a
// 64th of a graph launch instead of two kernel launches (2.8 us each against the GPU's 4.4 us per kernel: a slower or
// shared host core paces the eager loop, 10-12 us per iteration on such boxes of the pool), and the GPU side runs the
// chain at 8.7 us per iteration on every box (mppi_time_rollout_launch measures exactly this).  Two instances of the
// graph are launched in turn and an instance is launched again only when its previous run has finished: several queued
// launches of ONE instance take a slow path in the runtime (11.2 us per iteration with 19 of them queued, measured).
// Only iterations that cannot ask for another round: frozen waypoint index, or the sequential one resting at the end of
// the path.  OPT-IN (MPPI_GRAPH=1): on the pool's boxes the replayed loop holds 9.6-9.7 us per iteration where the eager
// one wanders between 9.7 and 11.2, but over whole episodes (restarts, the eager traversal, re-captures when an argument
// changes) it came out 0.1-0.4 us per iteration behind, so eager launches stay the default.  MPPI_GRAPH_SLOTS: iterations
// per graph (experiments).
#define GRAPH_SLOTS (h->sw.graph_slots)

// The one graph capture: n executions of a slot plan (launch_slot) captured from gs, thread-local mode, into *graph.  The launch
// counters come back as they were: a captured launch has not run (replays are counted where they are launched).
// Instantiation, caching and replay are the caller's.
template <typename R>
static hipError_t capture_slots(mppi_handle *h, const SlotPlan &sp, const KParams<R> &P, const FinalizeParams &F, int n, hipStream_t gs,
                                hipGraph_t *graph) {
    const long long l0 = h->n_rollout_launches, f0 = h->n_finalize_launches;
    hipError_t e = hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        for (int j = 0; j < n; ++j) launch_slot<R>(h, sp, P, F, gs);
        e = hipStreamEndCapture(gs, graph);
    }
    h->n_rollout_launches = l0;
    h->n_finalize_launches = f0;
    return e;
}

template <typename R>
static bool ensure_graph(mppi_handle *h, const SlotPlan &sp, const KParams<R> &P, const FinalizeParams &F) {
    // (the learned model's parameters too: its launches carry MlpParams -- weight pointers, shape, output bias -- by value,
    // agent 0's; a batched launch carries the address of the agents' table instead, whose entries a replay reads afresh)
    const MlpParams *const models = h->d_models;  // (the raw address: that is what a launch carries)
    const FleetParams fleet = h->fleet ? make_fleet(h, 1) : FleetParams{};  // (the k_fleet_rows launch of a slot)
    std::vector<char> key(sizeof(P) + sizeof(F) + 2 * sizeof(int) + sizeof(MlpParams) + sizeof(models) + sizeof(fleet));
    memcpy(key.data(), &P, sizeof(P));
    memcpy(key.data() + sizeof(P), &F, sizeof(F));
    const int tail[2] = {h->rollout_repeats, (int)sizeof(R)};
    memcpy(key.data() + sizeof(P) + sizeof(F), tail, sizeof(tail));
    memcpy(key.data() + sizeof(P) + sizeof(F) + sizeof(tail), &h->mlp, sizeof(MlpParams));
    memcpy(key.data() + sizeof(P) + sizeof(F) + sizeof(tail) + sizeof(MlpParams), &models, sizeof(models));
    memcpy(key.data() + sizeof(P) + sizeof(F) + sizeof(tail) + sizeof(MlpParams) + sizeof(models), &fleet, sizeof(fleet));
    if (h->graph_exec[0] && key == h->graph_key) return true;
    if (h->sw.graph_verbose) fprintf(stderr, "[mppi] capturing a graph of %d iterations\n", GRAPH_SLOTS);
    drop_graph(h);
    hipError_t e = hipSuccess;
    if (!h->graph_stream) e = hipStreamCreateWithFlags(h->graph_stream.put(), hipStreamNonBlocking);
    if (e == hipSuccess && !h->graph_ev_in) e = hipEventCreateWithFlags(h->graph_ev_in.put(), hipEventDisableTiming);
    if (e == hipSuccess && !h->graph_ev_out) e = hipEventCreateWithFlags(h->graph_ev_out.put(), hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i)
        if (!h->graph_done[i]) e = hipEventCreateWithFlags(h->graph_done[i].put(), hipEventDisableTiming);
    {
        Graph graph;  // (the executables keep what they need of it)
        if (e == hipSuccess) e = capture_slots<R>(h, sp, P, F, GRAPH_SLOTS, h->graph_stream, graph.put());
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipGraphInstantiate(h->graph_exec[i].put(), graph, nullptr, nullptr, 0);
    }
    if (e != hipSuccess) {  // no graphs on this runtime: the eager loop serves
        (void)hipGetLastError();
        drop_graph(h);
        h->graph_on = false;
        return false;
    }
    h->graph_key.swap(key);
    return true;
}

template <typename R>
static int closed_loop_impl(mppi_handle *h, int n_iters, double *u0_trace, mppi_stats *stats, hipStream_t s) {
    if (h->rccl_comm && h->x_nranks <= 1) return closed_loop_rccl<R>(h, n_iters, u0_trace, stats, s);
    KParams<R> P = make_params<R>(h, nullptr);
    FinalizeParams F = make_finalize(h, 1);
    if (u0_trace)
        if (int rc = trace_rows(h, n_iters, &F.u0_trace)) return rc;
    SlotPlan sp = plan_slot<R>(h, P, &F);  // for the whole call -- made again where the look-back is dropped at the path end
    const long long target = h->iter + n_iters;
    // x0 call for the state already on the device -- unless the finalize kernel of the previous closed-loop iteration
    // has made it (a second call would search from the index the first one left: with the frozen index that is c, not
    // prev_waypoints_idx, and the result would depend on how a run is cut into calls)
    if (!h->dev_loop_primed) launch_set_state<R>(P, nullptr, s);
    h->dev_loop_primed = false;
    long long done = h->iter;
    int guard = 0;
    const double t_call = now_s();
    // While the HYPK kernels are in use the host looks in on the waypoint index after 32, 64, 128 ... slots: at the end
    // of the path (the reference driver's run reaches it after some 23 of its 1000 iterations) the lean kernels take over
    long long batch = P.hyp ? 32 : (1LL << 62);
    int idx_now = h->idx_valid ? h->idx : -1;
    while (done < target) {
        const long long todo = target - done < batch ? target - done : batch;
        // The last slot of the batch writes its result straight into mapped host memory and publishes a sequence word
        // the host polls (as mppi_step does): no copy launch and no stream synchronisation at the end of the call
        // (14 -> 7 us of fixed cost per call).  Several agents per handle: one result per agent, copied as before.
        const bool poll = !h->sw.no_poll && h->B == 1;
        const double t_enq = now_s();
        // the bulk of a long batch from the cached graph (see ensure_graph), the rest -- and the slot that publishes the
        // result -- eagerly behind it, all on the graph's stream, which waits for and is waited for by the caller's
        const bool rests = h->cfg.waypoint_mode != MPPI_WAYPOINT_SEQUENTIAL || (idx_now >= 0 && at_path_end(h, idx_now));
        hipStream_t ls = s;
        long long i = 0;
        if (h->graph_on && rests && !P.hyp && !u0_trace && h->x_nranks <= 1 && !timing_on(h) && todo > GRAPH_SLOTS &&
            ensure_graph<R>(h, sp, P, F)) {
            ls = h->graph_stream;
            HIPCHECK(h, hipEventRecord(h->graph_ev_in, s));
            HIPCHECK(h, hipStreamWaitEvent(ls, h->graph_ev_in, 0));
            const long long reps = (todo - 1) / GRAPH_SLOTS;
            for (long long r = 0; r < reps; ++r) {
                const int inst = (int)(r & 1);
                if (r >= 2) HIPCHECK(h, hipEventSynchronize(h->graph_done[inst]));  // that instance's previous run is over
                HIPCHECK(h, hipGraphLaunch(h->graph_exec[inst], ls));
                HIPCHECK(h, hipEventRecord(h->graph_done[inst], ls));
            }
            i = reps * GRAPH_SLOTS;
            h->n_rollout_launches += i * h->rollout_repeats;
            h->n_finalize_launches += i;
        }
        for (; i < todo; ++i) {
            if (poll && i == todo - 1) {
                FinalizeParams Fl = F;
                Fl.res = h->res_mapped;
                Fl.seq = ++h->seq;
                launch_slot<R>(h, sp, P, Fl, ls);
            } else {
                launch_slot<R>(h, sp, P, F, ls);
            }
        }
        if (ls != s) {
            HIPCHECK(h, hipEventRecord(h->graph_ev_out, ls));
            HIPCHECK(h, hipStreamWaitEvent(s, h->graph_ev_out, 0));
        }
        HIPCHECK(h, hipGetLastError());
        h->t_enqueue_s += now_s() - t_enq;
        if (poll) {
            if (int rc = wait_result(h, h->seq, s)) return rc;
        } else if (int rc = fetch_result(h, (size_t)h->B * h->res_bytes, s)) {
            return rc;
        }
        for (int a = 1; a < h->B; ++a) {  // an agent at the end of its path stops the batch like the single agent does
            const StepResult *ra =
                reinterpret_cast<const StepResult *>(reinterpret_cast<const char *>(h->h_res.get()) + (size_t)a * h->res_bytes);
            if (ra->status == STATUS_PATH_END) h->h_res->status = STATUS_PATH_END;
        }
        if (h->h_res->status == STATUS_PATH_END || h->h_res->status == STATUS_EXCHANGE_FAILED) break;
        done = h->h_res->iter;  // slots spent on speculation rounds did not complete an iteration
        idx_now = h->h_res->idx_after;
        if (P.hyp) {
            if (h->B == 1 && at_path_end(h, h->h_res->idx_after)) {
                P.hyp = 0;
                sp = plan_slot<R>(h, P, &F);
                batch = 1LL << 62;
            } else {
                batch *= 2;
            }
        }
        if (++guard > h->cfg.K + 64) FAIL(h, MPPI_ERR_STATE, "closed loop did not make progress");
    }
    h->t_loop_s += now_s() - t_call;
    h->last_iter_us = 1e6 * (now_s() - t_call) / (n_iters > 0 ? n_iters : 1);
    note_noise(h, nullptr, false);
    // kept: after an asynchronous split step this does not hand the index back to the host (idx_valid stays as it is)
    if (int rc = adopt_result(h, KEEP_IDX_VALID, nullptr, nullptr, stats)) return rc;
    if (u0_trace)
        HIPCHECK(h, hipMemcpy(u0_trace, h->d_trace, sizeof(double) * 2 * n_iters, hipMemcpyDeviceToHost));
    h->dev_loop_primed = true;  // the last finalize made the next iteration's x0 call
    return MPPI_OK;
}

extern "C" int mppi_run_closed_loop(mppi_handle *h, int32_t n_iters, double *u0_trace, mppi_stats *stats,
                                    void *stream) {
    int rc = check_ready(h, "mppi_run_closed_loop");
    if (rc) return rc;
    if (n_iters < 1) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_run_closed_loop: n_iters < 1");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) { return closed_loop_impl<decltype(r)>(h, n_iters, u0_trace, stats, (hipStream_t)stream); });
}

// ------------------------------------------------------------------------------------------
// Launch-to-launch duration of the rollout kernel on the GPU, with the host out of the loop (include/mppi_hip.h,
// mppi_time_rollout_launch): n_slots closed-loop iterations captured into a HIP graph twice -- as they are, and with the
// (idempotent) rollout kernel launched 1 + extra times per iteration -- and replayed between two events each; the
// difference per extra launch is what one more launch of that kernel costs the stream.  Eager launches measure the same
// on a host that keeps the queue full; on a slow or shared host core they measure the host.
// ------------------------------------------------------------------------------------------
template <typename R>
static int time_rollout_impl(mppi_handle *h, int n_slots, int extra, hipStream_t s, double *us_out) {
    KParams<R> P = make_params<R>(h, nullptr);
    FinalizeParams F = make_finalize(h, 1);
    const SlotPlan sp = plan_slot<R>(h, P, &F);
    if (P.hyp || (h->cfg.waypoint_mode == MPPI_WAYPOINT_SEQUENTIAL && !at_path_end(h, h->idx)))
        FAIL(h, MPPI_ERR_STATE, "mppi_time_rollout_launch: the sequential waypoint index can still move (speculation rounds "
                                "cannot be replayed from a graph); call it once the index rests at the end of the path");
    if (timing_on(h))
        FAIL(h, MPPI_ERR_STATE, "mppi_time_rollout_launch: switch mppi_enable_timing off first (its events cannot be recorded "
                                "inside a stream capture)");
    if (!h->dev_loop_primed) launch_set_state<R>(P, nullptr, s);
    HIPCHECK(h, hipStreamSynchronize(s));
    Stream gs;  // (the events go before the stream, on every exit)
    Event e1, e0;
    HIPCHECK(h, hipStreamCreateWithFlags(gs.put(), hipStreamNonBlocking));
    HIPCHECK(h, hipEventCreate(e0.put()));
    HIPCHECK(h, hipEventCreate(e1.put()));
    const int saved = h->rollout_repeats, reps = 4;
    double ms[2] = {0.0, 0.0};
    int rc = MPPI_OK;
    for (int v = 0; v < 2 && rc == MPPI_OK; ++v) {
        h->rollout_repeats = v == 0 ? 1 : 1 + extra;
        Graph graph;  // (both go at the end of the variant, the executable first)
        GraphExec exec;
        hipError_t e = capture_slots<R>(h, sp, P, F, n_slots, gs, graph.put());  // (a diagnostic: the caller's launch counters stay)
        if (e == hipSuccess) e = hipGraphInstantiate(exec.put(), graph, nullptr, nullptr, 0);
        if (e == hipSuccess) e = hipGraphLaunch(exec, gs);  // warm
        if (e == hipSuccess) e = hipStreamSynchronize(gs);
        const double w0 = now_s();
        if (e == hipSuccess) e = hipEventRecord(e0, gs);
        for (int r = 0; r < reps && e == hipSuccess; ++r) e = hipGraphLaunch(exec, gs);
        if (e == hipSuccess) e = hipEventRecord(e1, gs);
        if (e == hipSuccess) e = hipStreamSynchronize(gs);
        if (h->sw.graph_verbose) fprintf(stderr, "[mppi] variant %d: wall %.2f us per iteration\n", v, 1e6 * (now_s() - w0) / (reps * n_slots));
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        ms[v] = t;
        if (e != hipSuccess) {
            h->err = std::string("mppi_time_rollout_launch: ") + hipGetErrorString(e);
            rc = MPPI_ERR_HIP;
        }
    }
    h->rollout_repeats = saved;
    if (rc != MPPI_OK) return rc;
    // the replays advanced the closed loop like any other run: pick the state up where they left it
    HIPCHECK(h, hipMemcpy(h->h_res, h->d_res, h->res_bytes, hipMemcpyDeviceToHost));
    // kept: a diagnostic -- whatever status the last replayed slot left (a path end with raise_at_path_end) is not an error
    // here, and idx_valid stays as it is
    (void)adopt_result(h, KEEP_IDX_VALID | KEEP_GOING, nullptr, nullptr, nullptr);
    h->dev_loop_primed = true;
    note_noise(h, nullptr, false);
    const double per = (double)reps * n_slots;
    us_out[0] = 1e3 * (ms[1] - ms[0]) / (per * extra);
    us_out[1] = 1e3 * ms[0] / per;
    return MPPI_OK;
}

extern "C" int mppi_time_rollout_launch(mppi_handle *h, int32_t n_slots, int32_t extra, void *stream, double *us_out2) {
    int rc = check_ready(h, "mppi_time_rollout_launch");
    if (rc) return rc;
    if (!us_out2 || n_slots < 1 || n_slots > 4096 || extra < 1 || extra > 16)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_time_rollout_launch: n_slots 1..4096, extra 1..16");
    if (h->x_nranks > 1 || h->rccl_comm)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_time_rollout_launch: not with an exchange between ranks (its sequence numbers cannot be replayed)");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) { return time_rollout_impl<decltype(r)>(h, n_slots, extra, (hipStream_t)stream, us_out2); });
}

// ------------------------------------------------------------------------------------------
// Batched stage methods (include/mppi_hip.h, mppi_eval_*): host arrays in, host arrays out; the arithmetic is the
// device code of the rollout kernels in the handle's precision.
// ------------------------------------------------------------------------------------------
static void eval_transition_mlp(mppi_handle *h, const KParams<float> &P, const void *x, const void *v, int n, void *out) {
    launch_eval_mlp(P, h->mlp, h->sw, (const float *)x, (const float *)v, n, (float *)out, nullptr);
}
static void eval_transition_mlp(mppi_handle *, const KParams<double> &, const void *, const void *, int, void *) {}  // rejected at create
// What k_eval_pose finds behind the words make_params set, for agent 0: the composed table, else the one ingredient the handle
// holds (a handle whose agent 0 has none: its circles alone); the grid under the outline, by the pose's yaw, where the mode says so
static int eval_form(const mppi_handle *h, int obs_motion) {
    const int foot = h->grid_footprint == MPPI_GRID_FOOTPRINT_OUTLINE ? EVAL_FORM_FOOT : 0;
    if (obs_motion == OBS_MOTION_SCENE) return EVAL_FORM_SCENE | foot;
    if (h->fleet_plan) return EVAL_FORM_PLANS;
    if (tracks_of(h, 0).n > 0) return EVAL_FORM_TRACKS;
    if (grid_of(h, 0).nx > 0) return EVAL_FORM_GRID | foot;
    return EVAL_FORM_CIRCLES;
}

template <typename R>
static int eval_impl(mppi_handle *h, int what, const double *x, const double *v, int n, int32_t *prev_idx, int update,
                     double *out, int32_t *idx_out, const int32_t *steps = nullptr) {
    const KParams<R> P = make_params<R>(h, nullptr);
    const int nx = h->nx;
    const bool need_x = what != EVAL_CLAMP, need_v = what == EVAL_TRANSITION || what == EVAL_CLAMP;
    const bool need_idx = what == EVAL_COST_STAGE || what == EVAL_COST_TERMINAL || what < 0;  // what < 0: index only
    const int n_out = what == EVAL_TRANSITION ? nx : what == EVAL_CLAMP ? 2 : 1;
    DevBuf<R> dx, dv, dout;
    DevBuf<int> di, dp, ds;
    // moving obstacles: the collision test (alone or inside a cost) takes the kernel that knows the clock; steps null: "now"
    const bool at = h->cfg.obstacle_motion && (what == EVAL_COLLIDED || what == EVAL_COST_STAGE || what == EVAL_COST_TERMINAL);
    if (at && steps) {
        HIPCHECK(h, ds.alloc(sizeof(int) * (size_t)n));
        HIPCHECK(h, hipMemcpy(ds, steps, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    if (need_x) {
        HIPCHECK(h, dx.alloc(sizeof(R) * (size_t)n * nx));
        if (int rc = upload_real(h, dx, x, (size_t)n * nx)) return rc;
    }
    if (need_v) {
        HIPCHECK(h, dv.alloc(sizeof(R) * (size_t)n * 2));
        if (int rc = upload_real(h, dv, v, (size_t)n * 2)) return rc;
    }
    if (need_idx) {
        if (!prev_idx) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval: prev_idx is null");
        if (*prev_idx < 0 || *prev_idx >= P.n_ref) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval: waypoint index %d out of range", *prev_idx);
        HIPCHECK(h, di.alloc(sizeof(int) * (size_t)n));
        HIPCHECK(h, dp.alloc(sizeof(int)));
        launch_eval_index<R>(P, dx, nx, n, *prev_idx, update ? 1 : 0, di, dp, nullptr);
    }
    if (what >= 0) {
        HIPCHECK(h, dout.alloc(sizeof(R) * (size_t)n * n_out));
        if (what == EVAL_TRANSITION && h->cfg.model == MPPI_MODEL_DIFFDRIVE_MLP)  // x + dt (f + MLP([x, v])), fp32 handles only
            eval_transition_mlp(h, P, dx, dv, n, dout);
        else if (at) {
            if (h->fleet) launch_fleet_front<R>(h, P, 0, nullptr);  // agent 0's mates as of the current states
            launch_eval_pose<R>(P, eval_form(h, P.obs_motion), what, 0, dx, di, ds, n, dout, nullptr, nullptr);
        }
        else
            launch_eval<R>(P, what, dx, dv, di, n, dout, nullptr);
    }
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipDeviceSynchronize());
    if (what >= 0)
        if (int rc = download_real(h, out, dout, (size_t)n * n_out)) return rc;
    if (need_idx) {
        if (idx_out) HIPCHECK(h, hipMemcpy(idx_out, di, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        int pn = *prev_idx;
        HIPCHECK(h, hipMemcpy(&pn, dp, sizeof(int), hipMemcpyDeviceToHost));
        if (update) *prev_idx = pn;
    }
    return MPPI_OK;
}

static int eval_entry(mppi_handle *h, const char *who, int what, const double *x, const double *v, int n, int32_t *prev_idx,
                      int update, double *out, int32_t *idx_out, const int32_t *steps = nullptr) {
    int rc = check_ready(h, who);
    if (rc) return rc;
    if (n < 1 || (what >= 0 && !out)) FAIL(h, MPPI_ERR_BAD_ARG, "%s: bad argument", who);
    if ((what != EVAL_CLAMP && !x) || ((what == EVAL_TRANSITION || what == EVAL_CLAMP) && !v))
        FAIL(h, MPPI_ERR_BAD_ARG, "%s: null input", who);
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) { return eval_impl<decltype(r)>(h, what, x, v, n, prev_idx, update, out, idx_out, steps); });
}

extern "C" int mppi_eval_state_transition(mppi_handle *h, const double *x, const double *v, int32_t n, double *x_next) {
    return eval_entry(h, "mppi_eval_state_transition", EVAL_TRANSITION, x, v, n, nullptr, 0, x_next, nullptr);
}
extern "C" int mppi_eval_clamp(mppi_handle *h, const double *v, int32_t n, double *out) {
    return eval_entry(h, "mppi_eval_clamp", EVAL_CLAMP, nullptr, v, n, nullptr, 0, out, nullptr);
}
extern "C" int mppi_eval_is_collided(mppi_handle *h, const double *x, int32_t n, double *out) {
    return eval_entry(h, "mppi_eval_is_collided", EVAL_COLLIDED, x, nullptr, n, nullptr, 0, out, nullptr);
}
extern "C" int mppi_eval_is_collided_at(mppi_handle *h, const double *x, int32_t n, const int32_t *steps, double *out) {
    if (h && !steps) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval_is_collided_at: steps is null");
    for (int i = 0; h && steps && i < n; ++i)
        if (steps[i] < 0) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval_is_collided_at: steps[%d] = %d is negative (steps count ahead of the clock)", i, steps[i]);
    for (int i = 0; h && h->fleet_plan && steps && i < n; ++i)
        if (steps[i] > h->cfg.T) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval_is_collided_at: steps[%d] = %d lies beyond the mates' plans (T = %d points ahead)", i, steps[i], h->cfg.T);
    return eval_entry(h, "mppi_eval_is_collided_at", EVAL_COLLIDED, x, nullptr, n, nullptr, 0, out, nullptr, steps);
}

// The circles agent `agent`'s next iteration tests, read back from its table (a fleet handle: the mates' rows made afresh first)
template <typename R>
static int agent_circles_impl(mppi_handle *h, int agent, double *xyr_out, double *vel_out, int cap, int32_t *m_out) {
    const AgentScene sc = scene_of(h, agent);
    const int m = sc.n_obs;
    *m_out = m;
    if (cap < m) FAIL(h, MPPI_ERR_SHAPE, "mppi_get_agent_circles: agent %d has %d circles, cap = %d", agent, m, cap);
    if (m == 0) return MPPI_OK;
    if (!sc.obs) FAIL(h, MPPI_ERR_STATE, "mppi_get_agent_circles: obstacles not uploaded");
    const bool moving = h->cfg.obstacle_motion != 0;
    HIPCHECK(h, hipDeviceSynchronize());
    if (h->fleet && !h->fleet_plan) {  // (plan mode: the table holds the own rows alone)
        launch_fleet_rows<R>(make_fleet(h, 0), nullptr);
        HIPCHECK(h, hipDeviceSynchronize());
    }
    std::vector<R> rows((size_t)(moving ? 8 : 4) * m, R(0));
    long long now = 0;
    HIPCHECK(h, hipMemcpy(rows.data(), sc.obs, sizeof(R) * rows.size(), hipMemcpyDeviceToHost));
    if (moving) HIPCHECK(h, hipMemcpy(&now, &h->d_st[agent].iter, sizeof(now), hipMemcpyDeviceToHost));
    const R tau = (R)h->cfg.delta_t * (R)(int)(now - sc.iter0);  // (obstacle_time at j = 0)
    for (int i = 0; i < m; ++i) {
        const R vx = moving ? rows[4 * (size_t)(m + i)] : R(0), vy = moving ? rows[4 * (size_t)(m + i) + 1] : R(0);
        const double thr = sqrt((double)rows[4 * (size_t)i + 2]);
        xyr_out[3 * i] = (double)std::fma(vx, tau, rows[4 * (size_t)i]);
        xyr_out[3 * i + 1] = (double)std::fma(vy, tau, rows[4 * (size_t)i + 1]);
        xyr_out[3 * i + 2] = h->cfg.obstacle_model == MPPI_OBSTACLE_CIRCLE ? thr - 0.5 * h->cfg.safety_margin : thr;
        vel_out[2 * i] = (double)vx;
        vel_out[2 * i + 1] = (double)vy;
    }
    return MPPI_OK;
}

extern "C" int mppi_get_agent_circles(mppi_handle *h, int32_t agent, double *xyr_out, double *vel_out, int32_t cap, int32_t *m_out) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!m_out || cap < 0 || (cap > 0 && (!xyr_out || !vel_out))) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_agent_circles: bad argument");
    if (agent < 0 || agent >= h->B) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_agent_circles: agent %d not in [0, %d)", agent, h->B);
    if (h->cfg.obstacle_model == MPPI_OBSTACLE_NONE)
        FAIL(h, MPPI_ERR_STATE, "mppi_get_agent_circles: the handle has no obstacle model (MPPI_OBSTACLE_NONE)");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    return with_real(h, [&](auto r) { return agent_circles_impl<decltype(r)>(h, agent, xyr_out, vel_out, cap, m_out); });
}

extern "C" int mppi_get_fleet_clearance(mppi_handle *h, double *min_dist, int64_t *contact_iters, int32_t reset) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!h->fleet)
        FAIL(h, MPPI_ERR_STATE, "mppi_get_fleet_clearance: the handle was created with fleet_radius = 0 (no fleet avoidance)");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    std::vector<FleetClear> rec(h->B);
    HIPCHECK(h, hipMemcpy(rec.data(), h->d_clear, sizeof(FleetClear) * rec.size(), hipMemcpyDeviceToHost));
    for (int a = 0; a < h->B; ++a) {
        if (min_dist) min_dist[a] = rec[a].min_dist;
        if (contact_iters) contact_iters[a] = rec[a].contact_iters;
    }
    if (reset) {
        std::fill(rec.begin(), rec.end(), FleetClear{INFINITY, 0});
        HIPCHECK(h, hipMemcpy(h->d_clear, rec.data(), sizeof(FleetClear) * rec.size(), hipMemcpyHostToDevice));
    }
    return MPPI_OK;
}

extern "C" int mppi_set_fleet_prediction(mppi_handle *h, int32_t mode) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (mode != MPPI_FLEET_VELOCITY && mode != MPPI_FLEET_PLAN)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_fleet_prediction: mode %d is neither MPPI_FLEET_VELOCITY nor MPPI_FLEET_PLAN", mode);
    if (!h->fleet)
        FAIL(h, MPPI_ERR_STATE, "mppi_set_fleet_prediction: the handle was created with fleet_radius = 0 (no fleet avoidance)");
    if (mode == MPPI_FLEET_PLAN && !scene_composed(h) && (max_tracks(h) > 0 || h->any_grid))
        FAIL(h, MPPI_ERR_STATE, "mppi_set_fleet_prediction: the handle holds %s, which use the same parameter words as the mates' plans "
                                "(limit: mppi_set_scene_mode with MPPI_SCENE_COMPOSED, or remove them first)",
             max_tracks(h) > 0 && h->any_grid ? "obstacle tracks and a cost grid" : h->any_grid ? "a cost grid" : "obstacle tracks");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (mode == MPPI_FLEET_PLAN && !h->d_plans) {
        const size_t bytes = rsz(h) * 2 * (size_t)(h->cfg.T + 1) * (size_t)h->B;
        HIPCHECK(h, h->d_plans.alloc(bytes));
        HIPCHECK(h, hipMemset(h->d_plans, 0, bytes));
    }
    h->fleet_plan = mode == MPPI_FLEET_PLAN;
    h->dev_loop_primed = false;
    drop_graph(h);
    if (int rc = build_fleet_tables(h, -1)) return rc;  // (the mate rows come or go; iter0 and the own rows stay)
    if (int rc = upload_scene_table(h)) return rc;
    return upload_scenes(h);
}

extern "C" int mppi_set_scene_mode(mppi_handle *h, int32_t mode) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (mode != MPPI_SCENE_EXCLUSIVE && mode != MPPI_SCENE_COMPOSED)
        FAIL(h, MPPI_ERR_BAD_ARG, "mppi_set_scene_mode: mode %d is neither MPPI_SCENE_EXCLUSIVE nor MPPI_SCENE_COMPOSED", mode);
    if (!h->cfg.obstacle_motion)
        FAIL(h, MPPI_ERR_STATE, "mppi_set_scene_mode: the handle was created with obstacle_motion = 0; fleet plans, obstacle tracks and "
                                "cost grids need mppi_config.obstacle_motion = %d at mppi_create", motion_value(h));
    if (!h->fused)
        FAIL(h, MPPI_ERR_UNSUPPORTED, "mppi_set_scene_mode: composed scenes are served for horizons T <= 128 (T = %d runs the unfused rollout)",
             h->cfg.T);
    if (mode == MPPI_SCENE_EXCLUSIVE && scene_ingredients(h) > 1)
        FAIL(h, MPPI_ERR_STATE, "mppi_set_scene_mode: the handle holds%s%s%s, which exclude each other in MPPI_SCENE_EXCLUSIVE "
                                "(limit: remove all but one first)",
             h->fleet_plan ? " the mates' plans (MPPI_FLEET_PLAN)" : "", max_tracks(h) > 0 ? (h->fleet_plan ? ", obstacle tracks" : " obstacle tracks") : "",
             h->any_grid ? (h->fleet_plan || max_tracks(h) > 0 ? " and a cost grid" : " a cost grid") : "");
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    if (mode == MPPI_SCENE_COMPOSED && !h->d_scene) HIPCHECK(h, h->d_scene.alloc(sizeof(SceneTable<double>)));
    if (mode != h->scene_mode) {
        h->scene_mode = mode;
        h->dev_loop_primed = false;
        drop_graph(h);
    }
    return upload_scene_table(h);
}
extern "C" int mppi_get_scene_mode(const mppi_handle *h, int32_t *mode) {
    if (!h || !mode) return MPPI_ERR_BAD_ARG;
    *mode = h->scene_mode;
    return MPPI_OK;
}

extern "C" int mppi_get_fleet_plans(mppi_handle *h, double *xy) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (!xy) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_get_fleet_plans: xy is null");
    if (!h->fleet_plan)
        FAIL(h, MPPI_ERR_STATE, "mppi_get_fleet_plans: the handle predicts its mates at constant velocity (mppi_set_fleet_prediction: MPPI_FLEET_PLAN)");
    if (learned_fleet(h))  // (the plans run through the agents' models)
        if (int rc = check_ready(h, "mppi_get_fleet_plans")) return rc;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    with_real(h, [&](auto r) { launch_fleet_front<decltype(r)>(h, make_params<decltype(r)>(h, nullptr), 0, nullptr); return 0; });
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipDeviceSynchronize());
    return download_real(h, xy, h->d_plans, 2 * (size_t)(h->cfg.T + 1) * (size_t)h->B);
}

extern "C" int mppi_eval_nearest_waypoint(mppi_handle *h, const double *x, int32_t n, int32_t *prev_idx, int32_t update_prev_idx,
                                          int32_t *idx_out) {
    if (h && !idx_out) FAIL(h, MPPI_ERR_BAD_ARG, "mppi_eval_nearest_waypoint: idx_out is null");
    return eval_entry(h, "mppi_eval_nearest_waypoint", -1, x, nullptr, n, prev_idx, update_prev_idx, nullptr, idx_out);
}
extern "C" int mppi_eval_cost(mppi_handle *h, int32_t terminal, const double *x, int32_t n, int32_t *prev_idx,
                              int32_t update_prev_idx, double *cost, int32_t *idx_out) {
    return eval_entry(h, "mppi_eval_cost", terminal ? EVAL_COST_TERMINAL : EVAL_COST_STAGE, x, nullptr, n, prev_idx,
                      update_prev_idx, cost, idx_out);
}

extern "C" int mppi_eval_moving_average(mppi_handle *h, const double *xx, double *out) {
    if (!h || !xx || !out) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    const int T = h->cfg.T;
    DevBuf<void> in, o;
    HIPCHECK(h, in.alloc(rsz(h) * 2 * T));
    HIPCHECK(h, o.alloc(rsz(h) * 2 * T));
    if (int rc = upload_real(h, in, xx, (size_t)2 * T)) return rc;
    with_real(h, [&](auto r) {
        using R = decltype(r);
        launch_eval_filter<R>((const R *)in.get(), (R *)o.get(), T, h->cfg.filter_window, h->cfg.filter_mode, nullptr);
    });
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipDeviceSynchronize());
    return download_real(h, out, o, (size_t)2 * T);
}

extern "C" int mppi_eval_weights(mppi_handle *h, const double *S, int32_t n, double *w) {
    if (!h || !S || !w || n < 1) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    DevBuf<double> in, o;
    HIPCHECK(h, in.alloc(sizeof(double) * (size_t)n));
    HIPCHECK(h, o.alloc(sizeof(double) * (size_t)n));
    HIPCHECK(h, hipMemcpy(in, S, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    launch_eval_weights(in, n, softmin_beta(h->cfg), o, nullptr);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipDeviceSynchronize());
    HIPCHECK(h, hipMemcpy(w, o, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return MPPI_OK;
}

extern "C" int mppi_get_counters(mppi_handle *h, int64_t *out3) {
    if (!h || !out3) return MPPI_ERR_BAD_ARG;
    out3[0] = h->iter;
    out3[1] = h->n_rollout_launches;
    out3[2] = h->n_finalize_launches;
    return MPPI_OK;
}

extern "C" int mppi_get_host_timing(const mppi_handle *h, double *out2) {
    if (!h || !out2) return MPPI_ERR_BAD_ARG;
    out2[0] = h->t_enqueue_s;
    out2[1] = h->t_loop_s;
    return MPPI_OK;
}

extern "C" int mppi_get_rollout_layout(const mppi_handle *h, int32_t *layout) {
    if (!h || !layout) return MPPI_ERR_BAD_ARG;
    *layout = (h->fused && h->cfg.model != MPPI_MODEL_DIFFDRIVE_MLP) ? h->layout : -1;
    return MPPI_OK;
}

extern "C" int mppi_get_rollout_kernel(const mppi_handle *h, char *buf, int32_t n) {
    if (!h || !buf || n < 1) return MPPI_ERR_BAD_ARG;
    snprintf(buf, (size_t)n, "%s", h->rollout_kernel);
    return MPPI_OK;
}

extern "C" int mppi_enable_timing(mppi_handle *h, int32_t on) {
    if (!h) return MPPI_ERR_BAD_ARG;
    if (on && !h->timing) h->ev_used = 0;  // a new measurement window
    h->timing = on != 0;
    return MPPI_OK;
}

extern "C" int mppi_set_rollout_repeats(mppi_handle *h, int32_t n) {
    if (!h || n < 1 || n > 64) return MPPI_ERR_BAD_ARG;
    h->rollout_repeats = n;
    return MPPI_OK;
}

extern "C" int mppi_last_kernel_ms(mppi_handle *h, float *out4) {
    if (!h || !out4) return MPPI_ERR_BAD_ARG;
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());  // every recorded event has completed
    collect_timing(h);
    memcpy(out4, h->last_ms, sizeof(h->last_ms));
    return MPPI_OK;
}
