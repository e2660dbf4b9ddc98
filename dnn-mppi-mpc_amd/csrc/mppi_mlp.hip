// BASELINE config 5: the MPPI rollout with LEARNED residual dynamics on the gfx950 matrix cores.
//
//   x_{t+1} = x_t + dt * ( f(x_t, v_t) + MLP([x_t, v_t]) ),   f = [v cos(yaw), v sin(yaw), w]
//   (test/bullet_differential_drive_dnn.py:79-92; MLP = train/train_diff_mlp.py:13-36:
//    Linear(5,512) -> 3 x [Linear(512,512) + tanh] -> Linear(512,3), first layer without activation)
//
// The recurrence is serial in t and dense in K, so the mapping differs from the analytic kernels: a
// workgroup (4 waves, one per SIMD, the whole CU) owns a tile of 64 samples and keeps its activations
// [64 x 512] f32 in LDS (132 KB of the CU's 160 KB) across all layers and all T steps; every wave owns
// 128 output columns of every layer as 2x4 accumulator tiles of v_mfma_f32_32x32x2_f32 (exact f32, the
// rate of the f32 vector unit but one VGPR per operand).  Weights (3.2 MB, L2-resident) are streamed as
// fully coalesced 16-byte-per-lane loads from a fragment-ordered copy packed once on the host: for the
// k-group g (8 reduction indices) lane l of a wave reads W[n = 32 ct + (l & 31)][8 g + 4 (l >> 5) + s],
// s = 0..3, which are the B fragments of four consecutive MFMA k-steps; the A fragments of the same four
// steps are one ds_read_b128 of the activation row (row pitch 516 floats: conflict-free for 16-lane
// groups).  Per k-group: 2 LDS reads + 4 global loads feed 32 MFMAs (2048 cycles), so the loop is
// MFMA-bound; the next group's operands are loaded before the current group's MFMAs issue.
// 1 581 056 flop per trajectory-step.
#include <string.h>

#include "mppi_device.h"

namespace mppi {

constexpr int MLP_M = 64, MLP_H = 512, MLP_PITCH = 516, MLP_WAVES = 4, MLP_GROUPS = MLP_H / 8;

using f32x16 = __attribute__((ext_vector_type(16))) float;
struct alignas(16) F4 { float v[4]; };

// Wave 0 searches the nearest waypoint of 64 samples every step while the other waves wait for it: the path (x, y, yaw, v
// per waypoint) is copied to LDS once per launch when it fits the 16 KB left beside the activations, so the search reads
// LDS instead of walking global memory (20 dependent loads per call, 5 % of the launch).
constexpr int MLP_REF_LDS_MAX = 768;  // (12 KB: what the 8-wave form of the f16-split kernel leaves beside its buffers)

// the path in LDS (returns the parameter block the per-sample code should use)
constexpr int H3_REF_LDS_32 = 256;  // the same beside a 32-sample tile (two workgroups share the CU's LDS)
__device__ __forceinline__ KParams<float> mlp_stage_path(const KParams<float> &P, float *ref_lds, int cap = MLP_REF_LDS_MAX) {
    KParams<float> PL = P;
    if (P.n_ref <= cap) {
        for (int i = threadIdx.x; i < P.n_ref; i += blockDim.x)
            reinterpret_cast<F4 *>(ref_lds)[i] = reinterpret_cast<const F4 *>(P.ref)[i];
        PL.ref = ref_lds;  // (first read behind the first workgroup barrier of the step loop)
    }
    return PL;
}

__device__ __forceinline__ float fast_tanh(float x) {  // 1 - 2 / (exp(2x) + 1): abs error ~2e-7
    const float e = __expf(2.0f * x);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);  // (v_rcp_f32, 1 ulp; `__fdividef` is the 10-instruction IEEE division here)
}

// acc[rt][ct] += A[rt] (64 x 8 slab of the activations) * B[ct] for one k-group
__device__ __forceinline__ void mfma_group(f32x16 (&acc)[2][4], const F4 (&a)[2], const F4 (&b)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt].v[s], b[ct].v[s], acc[rt][ct], 0, 0, 0);
}

// One Linear(n_groups*8 -> 512) of the tile: acc = act[64, :] @ W^T, this wave's 128 columns.
// `a_base` points at the A matrix in LDS (row pitch `pitch` floats), `wp` at this layer's packed weights.
__device__ __forceinline__ void gemm_layer(f32x16 (&acc)[2][4], const float *a_base, int pitch, const float *wp,
                                           int n_groups, int wid, int lane) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.f;
    const float *arow0 = a_base + (lane & 31) * pitch + 4 * (lane >> 5);
    const float *arow1 = arow0 + 32 * pitch;
    const float *wl = wp + ((size_t)(wid * 4) * n_groups * 64 + lane) * 4;  // + (ct * n_groups + g) * 256
    F4 a0[2], b0[4], a1[2], b1[4];
    auto load = [&](int g, F4 (&a)[2], F4 (&b)[4]) {
        a[0] = *reinterpret_cast<const F4 *>(arow0 + 8 * g);
        a[1] = *reinterpret_cast<const F4 *>(arow1 + 8 * g);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) b[ct] = *reinterpret_cast<const F4 *>(wl + ((size_t)ct * n_groups + g) * 256);
    };
    load(0, a0, b0);
    for (int g = 0; g < n_groups; g += 2) {  // two groups per trip: static register names for the prefetch
        if (g + 1 < n_groups) load(g + 1, a1, b1);
        mfma_group(acc, a0, b0);
        if (g + 1 < n_groups) {
            if (g + 2 < n_groups) load(g + 2, a0, b0);
            mfma_group(acc, a1, b1);
        }
    }
}

// bias (+ tanh), then this wave's [64 x 128] slice of the activations back to LDS.
// C/D layout of 32x32 tiles: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <bool TANH>
__device__ __forceinline__ void store_layer(float *act, const f32x16 (&acc)[2][4], const float *bias, int wid, int lane) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int n = wid * 128 + ct * 32 + (lane & 31);
        const float bn = bias[n];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const float v = acc[rt][ct][r] + bn;
                act[row * MLP_PITCH + n] = TANH ? fast_tanh(v) : v;
            }
    }
}

// ---- what the lanes of wave 0 (one lane = one sample of the tile) do around the network, shared by both kernels ----
struct MlpLane {
    float x, y, yaw, S;
    int p;
};

// this sample's controls at step t: noise (Philox or the caller's tensor), perturb, clamp (:116-121)
__device__ __forceinline__ void mlp_controls(const KParams<float> &P, unsigned iter, int k, int t, bool valid, bool exploit,
                                             float &u0, float &u1, float &v0, float &v1) {
    float e0 = 0.f, e1 = 0.f;
    if (valid) noise_at(P, (bool)P.use_philox, iter, 0, k, t, e0, e1);
    u0 = P.u[2 * t];
    u1 = P.u[2 * t + 1];
    perturb_clamp(P, exploit, (bool)P.clamp_rollout, u0, u1, e0, e1, v0, v1);
}

// Euler step of f + MLP (bullet_differential_drive_dnn.py:79-92)
__device__ __forceinline__ void mlp_euler(const KParams<float> &P, float r0, float r1, float r2, float v0, float v1, MlpLane &L) {
    float sn, cs;
    mf::sincos_(L.yaw, sn, cs);
    L.x = L.x + P.dt * (v0 * cs + r0);
    L.y = L.y + P.dt * (v0 * sn + r1);
    L.yaw = L.yaw + P.dt * (v1 + r2);
}

// The visualisation rollouts with this model (mppi_differential_drive.py:144-159; the reference never wires the learned
// model into MPPI, so this is the analytic controllers' loop with the transition swapped, like the rollout itself): step t
// is driven by control (t-1) mod T -- the reference's `[t-1]` indexing --, always clamped (:148,:158); rows 0..K-1 the
// samples' perturbed controls of the iteration just finished (its noise regenerated), one extra row the updated nominal
// sequence.  `VIZ` instantiation of the rollout kernel: same network code, no costs, the states stored instead.
struct MlpViz {
    const float *u_before, *u_upd;  // [T][2]: nominal controls before the update / updated, unshifted
    float *opt, *smp;               // [T][3], [K][T][3] (either may be null)
    unsigned iter;                  // the iteration whose noise the samples used
    int block0;                     // first workgroup of the launch (the samples' workgroups are left out without `smp`)
    // `_state_transition` of the learned model, batched (mppi_eval_state_transition): row k takes ONE Euler step from
    // ex[k] under the control ev[k] as it is given
    const float *ex, *ev;           // [en][3], [en][2]
    float *eout;                    // [en][3]
    int en;
};
__device__ __forceinline__ void mlp_controls_viz(const KParams<float> &P, const MlpViz &V, int k, int t, bool sample_row,
                                                 bool opt_row, bool exploit, float &v0, float &v1) {
    const int tc = (t + P.T - 1) % P.T;
    v0 = 0.f;
    v1 = 0.f;
    if (opt_row) {
        v0 = V.u_upd[2 * tc];
        v1 = V.u_upd[2 * tc + 1];
    } else if (sample_row) {
        float e0, e1;
        noise_at(P, (bool)P.use_philox, V.iter, 0, k, tc, e0, e1);
        perturb(exploit, V.u_before[2 * tc], V.u_before[2 * tc + 1], e0, e1, v0, v1);
    }
    clamp_controls(P, v0, v1);  // every row, the nominal one included (:148,:158)
}

// ---- fleet plans with the learned model (mppi_config.obstacle_motion = 3) --------------------------------------
// The plan form's controls: row t of the agent's nominal sequence -- control t at step t, not the visualisation's (t - 1) mod T
// --, clamped where the rollout clamps (perturb_clamp of an exploiting sample at zero noise).
__device__ __forceinline__ void mlp_controls_plan(const KParams<float> &P, int t, float &v0, float &v1) {
    v0 = P.u[2 * t];
    v1 = P.u[2 * t + 1];
    if (P.clamp_rollout) clamp_controls(P, v0, v1);
}
// agent a's clearance record, as k_fleet_rows and k_fleet_plan keep it (mppi_kernels.hip): lanes over the mates, their squared
// centre distances in f64, one minimum; updated where F.count says that an iteration starts here (wave 0 of the agent's one
// workgroup, stream order: a plain read-modify-write)
__device__ __forceinline__ void fleet_clearance(const FleetParams &F, int a, int lane) {
    const double *x0 = F.st[a].x0;
    double d2 = INFINITY;
    for (int m = lane; m < F.n_agents; m += 64) {
        if (m == a) continue;
        const double dx = F.st[m].x0[0] - x0[0], dy = F.st[m].x0[1] - x0[1];
        d2 = fmin(d2, dx * dx + dy * dy);
    }
    d2 = wv::reduce<wv::OpMin>(d2);
    if (F.count && lane == 0) {
        FleetClear *q = F.clear + a;
        const double d = sqrt(d2);
        q->min_dist = fmin(q->min_dist, d);
        if (d < F.contact) q->contact_iters += 1;
    }
}
// the mates of `agent` at point j of their plans: the table and the threshold out of the handle's SceneTable, handed to
// mates_collided through the two words the analytic plan mode reads them from (fleet_plan_table / fleet_plan_thr2) in a copy
// of the parameters -- on a learned handle those words carry the table's address and the footprint word.  At a step every lane
// reads the same point of mate a (j is uniform over the wave): from memory.  A null table (MPPI_FLEET_VELOCITY): no test.
__device__ __forceinline__ bool mlp_mates_collided(const KParams<float> &P, float x, float y, float yaw, int agent, int j) {
    const SceneTable<float> tb = *scene_table(P);
    if (tb.plans == nullptr) return false;
    KParams<float> PM = P;
    PM.pad_scenes[0] = (long long)reinterpret_cast<uintptr_t>(tb.plans);
    PM.pad_scenes[1] = 0;
    __builtin_memcpy(&PM.pad_scenes[1], &tb.thr2, sizeof(float));
    return mates_collided(PM, tb.plans, x, y, yaw, agent, j);
}

// ---- scene handles (mppi_config.obstacle_motion = 2) ----------------------------------------------------------
// What wave 0 of a scene form carries across the step loop beside the moving table: the iteration counter the clocks count from
// and its agent -- two scalar registers.  The descriptors themselves are NOT kept: held across the layers' GEMMs they cost the
// kernels 100 - 170 bytes of scratch per lane beyond their static twins, so mlp_scene_at reads them afresh at
// every priced step, three dependent scalar loads that hit the scalar cache, under ~0.5 % of a step.
struct MlpScene {
    long long iter;
    int agent;
};
// The agent's track and grid descriptors out of the handle's SceneTable (KParams::pad_scenes[0], OBS_MOTION_SCENE; `plans` is
// read by the fleet forms alone, mlp_mates_collided), the two clocks and the footprint word (KParams::pad_scenes[1], learned_scene_footprint).
// The step is uniform over the wave, so everything here but the grid's cells is: the uniform words go through readfirstlane
// and sit in SGPRs.  A missing ingredient is a null table, trk_n == 0 or nx == 0.
struct MlpSceneAt {
    const PlanPoint<float> *trk_pts = nullptr;
    const float *trk_thr2 = nullptr;
    int trk_n = 0, trk_L = 1, trk_clock = 0;
    GridSet<float> grid = {nullptr, 0, 0, 0.f, 0.f, 0.f, 0.f, 0.f};
    int foot = 0;   // MPPI_GRID_FOOTPRINT_OUTLINE: the grid under the nine outline points
    int clock = 0;  // the circles' (obstacle_clock)
};
__device__ __forceinline__ MlpSceneAt mlp_scene_at(const KParams<float> &P, const MlpScene &S) {
    MlpSceneAt sc;
    const SceneTable<float> tb = *scene_table(P);
    if (tb.tracks != nullptr) {
        const TrackSet ts = tb.tracks[S.agent];
        sc.trk_pts = static_cast<const PlanPoint<float> *>(ts.pts);
        sc.trk_thr2 = static_cast<const float *>(ts.thr2);
        sc.trk_n = __builtin_amdgcn_readfirstlane(ts.n);
        sc.trk_L = __builtin_amdgcn_readfirstlane(ts.L);
        sc.trk_clock = __builtin_amdgcn_readfirstlane(track_clock(S.iter, ts.iter0, ts.L));
    }
    if (tb.grids != nullptr) {
        sc.grid = tb.grids[S.agent];
        sc.grid.nx = __builtin_amdgcn_readfirstlane(sc.grid.nx);
        sc.grid.ny = __builtin_amdgcn_readfirstlane(sc.grid.ny);
    }
    sc.foot = __builtin_amdgcn_readfirstlane(learned_scene_footprint(P));
    sc.clock = __builtin_amdgcn_readfirstlane(obstacle_clock(S.iter, P.iter0));
    return sc;
}

// What wave 0's advance call prices a state against: the static kernels carry the obstacle table, the scene forms the moving
// table and their MlpScene.  One loader, called behind `sv` and in front of the early return.
template <bool SCENE> struct MlpObs {
    ObsLanes<float> obs;
};
template <> struct MlpObs<true> {
    ObsLanesMoving<float> obs;
    MlpScene scene;
};
template <bool SCENE>
__device__ __forceinline__ MlpObs<SCENE> mlp_obs_load(const KParams<float> &P, const DevState &sv, int lane, int agent) {
    if constexpr (SCENE) return MlpObs<true>{load_obstacles_moving(P, lane), MlpScene{sv.iter, agent}};
    else return MlpObs<false>{load_obstacles(P, lane)};
}

// this call's waypoint index and costs behind the Euler step.
// SCENE: the state after step t of the loop is stage call j = t + 1 -- the circles stand at c + v obstacle_time(clock + j), the
// tracks at point track_index(trk_clock, j, L) (read from memory: at a step every lane reads the same point), the grid is read
// at the state's position or under its outline -- and the terminal call prices the same state with j = T.  A state is hit when
// any ingredient says so; weight g joins the stage cost behind the control term and the terminal cost, as Rollout::costs has
// it (mppi_kernels.hip).
// FLEET (with SCENE; obstacle_motion = 3): behind the moving table, the tracks and the grid the state is tested against its
// mates at point j of their plans (mlp_mates_collided; skipped at run time in velocity mode, where the mates are rows of the
// moving table); the terminal call prices the same state, j = T.
template <bool SCENE, bool FLEET = false>
__device__ __forceinline__ void mlp_advance(const KParams<float> &P, const MlpObs<SCENE> &O, int c, int t, float r0, float r1, float r2,
                                            float u0, float u1, float v0, float v1, MlpLane &L) {
    const float *__restrict__ ref = P.ref;
    mlp_euler(P, r0, r1, r2, v0, v1, L);
    // waypoint index of this call: per-lane, so the sequential index threads through the sample's own
    // calls in order by construction (mppi_differential_drive.py:228)
    auto nearest = [&](int from) {
        float best = dist2(ref, from, L.x, L.y);
        int bj = 0;
#pragma unroll 4
        for (int j = 1; j < P.window; ++j) {
            const bool ok = from + j < P.n_ref;
            const float d = ok ? dist2(ref, min(from + j, P.n_ref - 1), L.x, L.y) : INFINITY;
            if (d < best) { best = d; bj = j; }
        }
        return from + bj;
    };
    const bool threads = P.sequential || P.per_rollout;  // the index moves with this sample's calls (:228)
    const int idx = nearest(threads ? L.p : c);
    if (threads) L.p = idx;
    if (P.accumulate || t == P.T - 1) {
        bool hit, has_grid = false;
        float wg = 0.f;
        if constexpr (SCENE) {
            const int j = t + 1;
            const MlpSceneAt SC = mlp_scene_at(P, O.scene);
            hit = collided<false, true>(P, L.x, L.y, L.yaw, O.obs, false, 0.f, 1.f, obstacle_time(P, SC.clock + j));
            if (SC.trk_n > 0)
                hit |= tracks_collided(P, SC.trk_pts + track_index(SC.trk_clock, j, SC.trk_L), SC.trk_thr2, SC.trk_n, SC.trk_L, L.x, L.y, L.yaw);
            has_grid = SC.grid.nx > 0;
            if (has_grid) {
                const float g = SC.foot ? grid_value_outline(SC.grid, P, L.x, L.y, L.yaw) : grid_value(SC.grid, L.x, L.y);
                hit |= g >= SC.grid.lethal;
                wg = SC.grid.weight * g;
            }
            if constexpr (FLEET) hit |= mlp_mates_collided(P, L.x, L.y, L.yaw, O.scene.agent, j);
        } else {
            hit = collided<false>(P, L.x, L.y, L.yaw, O.obs);
        }
        float stage = stage_cost<float, MODEL_DIFF>(P, (bool)P.wrap_stage, idx, L.x, L.y, L.yaw, 0.f, hit, u0, u1, v0, v1);
        if (has_grid) stage += wg;
        L.S = P.accumulate ? L.S + stage : stage;
        if (t == P.T - 1) {
            int idx_term = idx;
            if (threads) {  // the terminal call moves the index once more (:244)
                L.p = nearest(L.p);
                idx_term = L.p;
            }
            float term = terminal_cost<float, MODEL_DIFF>(P, (bool)P.wrap_term, idx_term, L.x, L.y, L.yaw, 0.f, hit);
            if (has_grid) term += wg;
            L.S += term;
        }
    }
}

// this tile's softmin record {rho, eta, eta2, pad, W[T][2]} (wave 0)
__device__ __forceinline__ void mlp_record(const KParams<float> &P, float *__restrict__ partials, unsigned iter, int k, int c,
                                           bool valid, bool live, MlpLane &L, int lane) {
    float S = L.S;
    if (live) {
        P.S[k] = S;
        P.pout[k] = L.p;
        if (P.sequential && L.p != c) atomicMin(&P.st->first_k, k);
    } else if (valid) {
        S = P.S[k];  // final from an earlier speculation round
    }
    const float Sm = valid ? S : INFINITY;
    const float rho = wv::reduce<wv::OpMin>(Sm);
    const float e = valid ? mf::exp_(-P.beta * (S - rho)) : 0.f;
    const float eta = wv::reduce<wv::OpAdd>(e), eta2 = wv::reduce<wv::OpAdd>(e * e);
    const float n_hit = P.obstacle_model != OBS_NONE ? wv::reduce<wv::OpAdd>(valid && S >= P.penalty ? 1.f : 0.f) : 0.f;
    float *out = partials + (size_t)blockIdx.x * record_len(P.T, 4);
    if (lane == 0) {
        out[0] = rho; out[1] = eta; out[2] = eta2;
        float *hd = P.heads + 4 * (size_t)blockIdx.x;  // the compact copy the merge kernels read
        hd[0] = rho; hd[1] = eta; hd[2] = eta2; hd[3] = n_hit;  // (n_hit: samples that carry a collision penalty)
    }
    for (int t = 0; t < P.T; ++t) {  // second pass over this tile's noise rows (regenerated / re-read)
        float e0 = 0.f, e1 = 0.f;
        if (valid) noise_at(P, (bool)P.use_philox, iter, 0, k, t, e0, e1);
        const float w0 = wv::reduce<wv::OpAdd>(e * e0), w1 = wv::reduce<wv::OpAdd>(e * e1);
        if (lane == 0) { out[4 + 2 * t] = w0; out[4 + 2 * t + 1] = w1; }
    }
}

__global__ __launch_bounds__(64 * MLP_WAVES, 1) void k_rollout_mlp(const KParams<float> P, const MlpParams Q,
                                                                    float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *act = smem;                       // [64][516]
    float *zbuf = act + MLP_M * MLP_PITCH;   // [64][8]   layer-0 input rows {x, y, yaw, v, w, 0, 0, 0}
    float *ypart = zbuf + MLP_M * 8;         // [4][64][4] partial outputs of the last Linear per wave
    float *ref_lds = ypart + MLP_WAVES * MLP_M * 4;  // [n_ref][4] when the path fits
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int k0 = blockIdx.x * MLP_M, k = k0 + lane;
    const KParams<float> PL = mlp_stage_path(P, ref_lds);
    const DevState sv = load_state(P, P.st);
    const MlpObs<false> obs = mlp_obs_load<false>(P, sv, lane, 0);
    if (k0 + MLP_M <= sv.k_start) return;  // every sample of the tile is final: its record stands
    const bool valid = k < P.K, live = valid && k >= sv.k_start;
    const int c = sv.c;
    const unsigned iter = (unsigned)sv.iter;

    // sample state lives in the lanes of wave 0 (one lane = one sample of the tile)
    MlpLane L{(float)sv.x0[0], (float)sv.x0[1], (float)sv.x0[2], 0.f, c};
    const bool exploit = (k + P.k_offset) < P.n_exploit;
    f32x16 acc[2][4];

    for (int t = 0; t < P.T; ++t) {
        float u0 = 0, u1 = 0, v0 = 0, v1 = 0;
        if (wid == 0) {
            mlp_controls(P, iter, k, t, valid, exploit, u0, u1, v0, v1);
            F4 z0 = {{L.x, L.y, L.yaw, v0}}, z1 = {{v1, 0.f, 0.f, 0.f}};
            *reinterpret_cast<F4 *>(zbuf + lane * 8) = z0;
            *reinterpret_cast<F4 *>(zbuf + lane * 8 + 4) = z1;
        }
        __syncthreads();
        // input_layer: Linear(5 -> 512), no activation (train/train_diff_mlp.py:32)
        gemm_layer(acc, zbuf, 8, Q.w_in, 1, wid, lane);
        store_layer<false>(act, acc, Q.b_in, wid, lane);
        __syncthreads();
        // hidden_layer[i]: tanh(Linear(512 -> 512)) (:33-34)
        for (int l = 0; l < Q.n_hidden; ++l) {
            gemm_layer(acc, act, MLP_PITCH, Q.w_h[l], MLP_GROUPS, wid, lane);
            __syncthreads();  // every wave has read the previous activations
            store_layer<true>(act, acc, Q.b_h[l], wid, lane);
            __syncthreads();
        }
        // out_layer: Linear(512 -> 3) (:35): lane = sample, this wave's 128 of the 512 inputs
        {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            const float *hrow = act + lane * MLP_PITCH + wid * 128;
            const float *w = Q.w_out + wid * 128;
#pragma unroll 8
            for (int n = 0; n < 128; n += 4) {
                const F4 h = *reinterpret_cast<const F4 *>(hrow + n);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s0 = fmaf(h.v[q], w[n + q], s0);
                    s1 = fmaf(h.v[q], w[MLP_H + n + q], s1);
                    s2 = fmaf(h.v[q], w[2 * MLP_H + n + q], s2);
                }
            }
            F4 o = {{s0, s1, s2, 0.f}};
            *reinterpret_cast<F4 *>(ypart + (wid * MLP_M + lane) * 4) = o;
        }
        __syncthreads();
        if (wid == 0) {
            float r0 = Q.b_out[0], r1 = Q.b_out[1], r2 = Q.b_out[2];
#pragma unroll
            for (int w = 0; w < MLP_WAVES; ++w) {
                const F4 o = *reinterpret_cast<const F4 *>(ypart + (w * MLP_M + lane) * 4);
                r0 += o.v[0];
                r1 += o.v[1];
                r2 += o.v[2];
            }
            mlp_advance<false>(PL, obs, c, t, r0, r1, r2, u0, u1, v0, v1, L);
        }
        // zbuf / ypart are rewritten only after the next barrier sequence: wave 0 writes zbuf at the top of
        // the next step while the others wait at that step's first barrier
    }
    if (wid == 0) mlp_record(P, partials, iter, k, c, valid, live, L, lane);
}

// ------------------------------------------------------------------------------------------
// The same rollout on the f16 matrix pipe, 16 x the rate of the f32-input MFMA, at f32-like accuracy: every operand
// is split into two f16 numbers, a = a_hi + a_lo (a_hi = f16(a), a_lo = f16(a - a_hi): 22 bits of significand, and
// below f16's normal range an absolute resolution of 2^-25), and a b is taken as a_hi b_hi + a_hi b_lo + a_lo b_hi --
// three `v_mfma_f32_32x32x16_f16` into the SAME f32 accumulator (every product of two f16 numbers is exact in f32).
// Relative error of a dot product ~2^-21 against ~2^-23 of the f32 chain; the parity tests (u within 1e-4 RMSE of the
// reference's class with the real checkpoint) hold with either kernel.  MPPI_MLP_F32=1 selects the f32-input kernel.
//
// Layout: activations as two f16 planes [64][520] in LDS (row pitch 1040 B: the 16-byte fragment reads of a 16-lane
// group fall into distinct banks); lane l of a wave (r = l & 31, h = l >> 5) reads A[row r][k = 16 s + 8 h + 0..7] for
// k-step s with one ds_read_b128 per plane and row tile.  Weights are packed on the host in fragment order
// [column tile][k-step][lane][8] per plane, so B[k = 16 s + 8 h + j][col = 32 ct + r] = W[col][k] is one coalesced
// 16-byte load per lane.  Per k-step and wave: 4 LDS reads + 8 global loads feed 24 MFMAs (768 cycles).
// ------------------------------------------------------------------------------------------
using half8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr int H3_ZPITCH = 24;  // (the activations' row pitch is H + 8 halfs, a layer's k-steps H / 16)
constexpr int H3_FORM_DEFAULT = 1;  // (H3_FORM_8x64, see the forms below)

__device__ __forceinline__ void split_h3(float v, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// The f16 range.  The input layer has no activation (train/train_diff_mlp.py:32), so raw [x, y, yaw, v, w] and the first
// layer's output h0 = W_in z + b_in travel through f16 halves at whatever magnitude the caller's coordinates have (a path in
// UTM metres: 1e5 .. 1e7): beyond 65504 a half is inf.  Per sample and step two powers of two keep every half below 2^15:
// z is split as z / s0, s0 = 2^max(0, exponent(|z|_inf) - 14), and h0 as h0 / s1 with s1 from the bound
// |h0|_inf <= in_gain |z|_inf + in_bias (host, mppi_set_mlp); the epilogues multiply the f32 accumulators back
// (store_layer_h3).  Exact scalings: only the absolute resolution of the low halves (2^-25) grows with them.  After the first
// tanh everything lies in [-1, 1].  s0 = s1 = 1 whenever |z|_inf < 2^15 and the bound stays below 2^15.
struct H3Scale { float s0, inv_s0, s1, inv_s1; };
__device__ __forceinline__ H3Scale h3_scale(const float (&z)[5], float in_gain, float in_bias) {
    const float zmax = fmaxf(fmaxf(fmaxf(fabsf(z[0]), fabsf(z[1])), fmaxf(fabsf(z[2]), fabsf(z[3]))), fabsf(z[4]));
    auto pow2_over = [](float m) {  // e = max(0, exponent(m) - 14): m / 2^e < 2^15
        const int e = max(0, (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127 - 14);
        return min(e, 100);  // (inf / NaN inputs stay what they are)
    };
    const int e0 = pow2_over(zmax), e1 = pow2_over(in_gain * zmax + in_bias);
    auto p2 = [](int e) { return __builtin_bit_cast(float, (unsigned)(127 + e) << 23); };
    return H3Scale{p2(e0), p2(-e0), p2(e1), p2(-e1)};
}

// acc[pass][rt][c2] = (A[64, 16 n_steps] @ W^T)^T for this wave's 128 columns (column tile ct = 2 pass + c2), i.e. the MFMA's
// "A" operand is the WEIGHT fragment and its "B" operand the activation fragment (both index a row / column by lane & 31
// and eight reduction indices by lane >> 5, so the fragments serve either role as they are): in the 32 x 32 result a lane
// then holds ONE sample (lane & 31 of row tile rt) and 16 output features in four runs of four consecutive ones -- which is
// what the epilogue wants to write: four f16 numbers = one 8-byte LDS store instead of four 2-byte ones (the 2-byte stores
// of the sample-per-register form held the LDS write port for a fifth of the launch).  a_hi / a_lo:
// the planes in LDS (row pitch `pitch` halfs).  Two passes of two column tiles each: the weights come from L2 (1 MB per
// layer and workgroup, the same MB for every workgroup), at 8 KB per k-step and wave their latency is what the loop has
// to cover -- so B runs THREE k-steps ahead in a ring of four register sets, and with two column tiles per pass that ring
// is 64 VGPRs (with four it spilled); the activations come from LDS just in time, twice per layer.
//
// The weight stream does not stop between the two passes of a layer: the last trip of the first pass requests the first
// three k-steps of the second into the ring sets it has just used up (an L2 round trip waited for at the top of every
// pass before).  Across layers the ring is not kept THROUGH the epilogue (that pushed the kernel into scratch spills, 8.3
// against 6.8 ms): the next layer's first k-steps are requested right behind the epilogue (h3_prime_layer).
struct H3FragA { half8 h[2], l[2]; };
struct H3FragB { half8 h[2], l[2]; };
struct H3Ring { H3FragB b0, b1, b2; };  // k-steps 0, 1, 2 of the pass about to run

// this lane's view of the two column tiles of (layer `w`, pass): + (c2 * n_steps + s) * 64
struct H3Pass { const half8 *hi, *lo; };
// NW waves per workgroup (4: one per SIMD, each owns 128 output columns = two passes of two column tiles; 8: two per SIMD,
// each owns 64 columns = one pass -- the same MFMAs, weight bytes and LDS reads per SIMD, but the two waves of a SIMD cover
// each other's waits in the GEMMs and share the VALU in the epilogues, which a single wave issues at half the pipe's rate)
// H: the layer's width (k_rollout_mlp_w; the 512-wide kernel uses the default), H / 32 column tiles
template <int NW, int H = MLP_H>
__device__ __forceinline__ H3Pass h3_pass(const unsigned short *layer, int n_steps, int wid, int pass, int lane) {
    constexpr int CT = H / 32;
    const half8 *w = reinterpret_cast<const half8 *>(layer);
    const size_t off = (size_t)(wid * (CT / NW) + 2 * pass) * n_steps * 64 + lane;
    return H3Pass{w + off, w + (size_t)CT * n_steps * 64 + off};
}
__device__ __forceinline__ void h3_load_b(const H3Pass &w, int n_steps, int s, H3FragB &f) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
        f.h[c2] = w.hi[((size_t)c2 * n_steps + s) * 64];
        f.l[c2] = w.lo[((size_t)c2 * n_steps + s) * 64];
    }
}
__device__ __forceinline__ void h3_prime(const H3Pass &w, int n_steps, H3Ring &r) {
    h3_load_b(w, n_steps, 0, r.b0);
    h3_load_b(w, n_steps, 1, r.b1);
    h3_load_b(w, n_steps, 2, r.b2);
}
// (the three terms as three sweeps over the four tiles: independent accumulators between two MFMAs on the same one)
// RT = row tiles of 32 samples a workgroup owns (2: the 64-sample tile; 1: a 32-sample tile, two workgroups per CU)
// TERMS = 2 (opt-in, MPPI_MLP_TERMS=2): without the a_lo b_hi term, i.e. with the activations rounded to f16 -- a third
// less matrix work (config 5: 6.5 -> 5.0 ms per iteration); u stays within 1e-7 RMSE of the reference, S within 3e-3
// relative, which is outside the 1e-3 the default is held to (see test_config5_two_term_split_is_an_opt_in).
template <int RT, int TERMS = 3> __device__ __forceinline__ void h3_mma(f32x16 (&ac)[RT][2], const H3FragA &a, const H3FragB &b) {
    if (TERMS == 3) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) ac[rt][c2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b.h[c2], a.l[rt], ac[rt][c2], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) ac[rt][c2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b.l[c2], a.h[rt], ac[rt][c2], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) ac[rt][c2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b.h[c2], a.h[rt], ac[rt][c2], 0, 0, 0);
}
template <int RT> __device__ __forceinline__ void h3_zero(f32x16 (&ac)[RT][2]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int r = 0; r < 16; ++r) ac[rt][c2][r] = 0.f;
}

// one pass (two column tiles) of an H-wide hidden layer: `ring` holds its k-steps 0..2 on entry and (HAS_NEXT) those of
// `next` on exit
template <bool HAS_NEXT, int RT, int TERMS = 3, int H = MLP_H>
__device__ __forceinline__ void gemm_pass_h3(f32x16 (&ac)[RT][2], const _Float16 *a_hi, const _Float16 *a_lo, const H3Pass &w,
                                             const H3Pass &next, H3Ring &ring, int lane) {
    constexpr int n_steps = H / 16, pitch = H + 8;
    const int aoff = (lane & 31) * pitch + 8 * (lane >> 5);
    auto load_a = [&](int s, H3FragA &f) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f.h[rt] = *reinterpret_cast<const half8 *>(a_hi + rt * 32 * pitch + aoff + 16 * s);
            f.l[rt] = *reinterpret_cast<const half8 *>(a_lo + rt * 32 * pitch + aoff + 16 * s);
        }
    };
    // (`sched_barrier`: the instruction scheduler would otherwise sink every load to just above its first use -- fewer
    // live registers, and the prefetch gone)
#define H3_FENCE() __builtin_amdgcn_sched_barrier(0)
    // One k-step = 12 MFMAs (384 cycles of the matrix pipe) + the requests that keep the ring and the activation fragments
    // ahead: 4 global loads + 4 LDS reads.  Issued as a block in front of the MFMAs they left the pipe idle while the
    // vector-memory unit took them; the group barriers below spread them, one behind each of the first eight MFMAs.
#define H3_SPREAD(n_vmem, n_lds)                                                                          \
    do {                                                                                                  \
        for (int _i = 0; _i < (n_vmem); ++_i) {                                                           \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); /* one MFMA */                             \
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); /* one vector-memory read */               \
        }                                                                                                 \
        for (int _i = 0; _i < (n_lds); ++_i) {                                                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                            \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* one LDS read */                         \
        }                                                                                                 \
        __builtin_amdgcn_sched_group_barrier(0x008, 6 * RT - (n_vmem) - (n_lds), 0);                      \
        H3_FENCE();                                                                                       \
    } while (0)
    h3_zero<RT>(ac);
    H3FragB b3;
    H3FragA a0, a1;
    load_a(0, a0);
    H3_FENCE();
#pragma unroll 1
    for (int s = 0; s < n_steps - 4; s += 4) {  // n_steps is a multiple of 4 (H / 16, H >= 64)
        h3_load_b(w, n_steps, s + 3, b3);
        load_a(s + 1, a1);
        h3_mma<RT, TERMS>(ac, a0, ring.b0);
        H3_SPREAD(4, 2 * RT);
        h3_load_b(w, n_steps, s + 4, ring.b0);
        load_a(s + 2, a0);
        h3_mma<RT, TERMS>(ac, a1, ring.b1);
        H3_SPREAD(4, 2 * RT);
        h3_load_b(w, n_steps, s + 5, ring.b1);
        load_a(s + 3, a1);
        h3_mma<RT, TERMS>(ac, a0, ring.b2);
        H3_SPREAD(4, 2 * RT);
        h3_load_b(w, n_steps, s + 6, ring.b2);
        load_a(s + 4, a0);
        h3_mma<RT, TERMS>(ac, a1, b3);
        H3_SPREAD(4, 2 * RT);
    }
    {   // the last four k-steps: the ring sets that fall free take the head of the next pass of the stream
        constexpr int s = n_steps - 4;
        h3_load_b(w, n_steps, s + 3, b3);
        load_a(s + 1, a1);
        h3_mma<RT, TERMS>(ac, a0, ring.b0);
        H3_SPREAD(4, 2 * RT);
        if (HAS_NEXT) h3_load_b(next, n_steps, 0, ring.b0);
        load_a(s + 2, a0);
        h3_mma<RT, TERMS>(ac, a1, ring.b1);
        H3_SPREAD(HAS_NEXT ? 4 : 0, 2 * RT);
        if (HAS_NEXT) h3_load_b(next, n_steps, 1, ring.b1);
        load_a(s + 3, a1);
        h3_mma<RT, TERMS>(ac, a0, ring.b2);
        H3_SPREAD(HAS_NEXT ? 4 : 0, 2 * RT);
        if (HAS_NEXT) h3_load_b(next, n_steps, 2, ring.b2);
        h3_mma<RT, TERMS>(ac, a1, b3);
        H3_SPREAD(HAS_NEXT ? 4 : 0, 0);
    }
#undef H3_SPREAD
#undef H3_FENCE
}

// a hidden layer: this wave's H / NW columns (one or two passes) of all 64 samples.  `ring`: the first three k-steps of the
// layer, requested by the caller (h3_prime_layer) once the previous layer's epilogue has let go of its registers -- they fly
// while the workgroup meets at the barrier in front of this layer.
template <int NW, int H = MLP_H>
__device__ __forceinline__ void h3_prime_layer(const unsigned short *layer, int wid, int lane, H3Ring &ring) {
    h3_prime(h3_pass<NW, H>(layer, H / 16, wid, 0, lane), H / 16, ring);
}
template <int NW, int RT, int TERMS = 3, int H = MLP_H>
__device__ __forceinline__ void gemm_layer_h3(f32x16 (&acc)[H / 64 / NW][RT][2], const _Float16 *a_hi, const _Float16 *a_lo,
                                              const unsigned short *layer, int wid, int lane, H3Ring &ring) {
    const H3Pass w0 = h3_pass<NW, H>(layer, H / 16, wid, 0, lane);
    if (H / 64 / NW == 2) {
        const H3Pass w1 = h3_pass<NW, H>(layer, H / 16, wid, 1, lane);
        gemm_pass_h3<true, RT, TERMS, H>(acc[0], a_hi, a_lo, w0, w1, ring, lane);
        gemm_pass_h3<false, RT, TERMS, H>(acc[H / 64 / NW - 1], a_hi, a_lo, w1, w1, ring, lane);
    } else {
        gemm_pass_h3<false, RT, TERMS, H>(acc[0], a_hi, a_lo, w0, w0, ring, lane);
    }
}

// Linear(5 -> H) of the step's inputs: one k-step (z rows padded to 16), every pass
template <int NW, int RT, int H = MLP_H>
__device__ __forceinline__ void gemm_input_h3(f32x16 (&acc)[H / 64 / NW][RT][2], const _Float16 *z_hi, const _Float16 *z_lo,
                                              const unsigned short *layer, int wid, int lane) {
    const int aoff = (lane & 31) * H3_ZPITCH + 8 * (lane >> 5);
    H3FragA a;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        a.h[rt] = *reinterpret_cast<const half8 *>(z_hi + rt * 32 * H3_ZPITCH + aoff);
        a.l[rt] = *reinterpret_cast<const half8 *>(z_lo + rt * 32 * H3_ZPITCH + aoff);
    }
#pragma unroll
    for (int pass = 0; pass < H / 64 / NW; ++pass) {
        const H3Pass w = h3_pass<NW, H>(layer, 1, wid, pass, lane);
        H3FragB b;
        h3_load_b(w, 1, 0, b);
        h3_zero<RT>(acc[pass]);
        h3_mma<RT>(acc[pass], a, b);
    }
}

// bias (+ tanh), split, then this wave's [64 x 128] slice of both planes back to LDS.  Result layout (see gemm_pass_h3):
// register r of tile (rt, ct) in lane l = sample 32 rt + (l & 31), feature 128 wid + 32 ct + (r & 3) + 8 (r >> 2) + 4 (l >> 5).
// The launch spends a fifth of its time here (one wave per SIMD: nothing else issues meanwhile), so two elements at a
// time: packed f32 arithmetic for the bias, the tanh's linear parts and the residual, and `v_cvt_pkrtz_f16_f32` for
// both conversions (the high part may round towards zero: the low part takes what is left, exactly) -- a converted
// pair IS two consecutive features, two pairs one 8-byte store.
using f32x2 = __attribute__((ext_vector_type(2))) float;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using half4v = __attribute__((ext_vector_type(4))) _Float16;
// Written in stages over the 16 registers of a tile (eight independent pairs per stage: with one wave per SIMD a chain
// of dependent instructions -- exp, add, rcp, fma, convert, subtract, convert -- runs at its latency, 90 cycles per
// element as the compiler first scheduled it, one pair after the other), and with four base addresses (plane x row tile)
// plus immediate offsets for the stores.
// LAST (the third hidden layer): its activations feed only the 512 -> 3 output layer, so they are not split or stored at
// all -- every lane multiplies its 64 features of a sample by the output weights as they leave the tanh (f32, `yo[rt][j]`),
// and the caller adds up the two lane halves and the four waves.  (Reading them back from LDS on the vector unit took 6 %
// of the launch, splitting and storing them another 2 %.)
// SCALE (the f16 range, see H3Scale): 0 none; 1 the input layer -- its accumulators are those of z / s0 and its output is
// stored as h0 / s1: v = (acc s0 + b) / s1; 2 the first hidden layer -- its accumulators are those of h0 / s1: v = acc s1 + b.
// `scale`: the per-sample {s0, 1 / s1, s1, 0} in LDS.  All three are 1 unless an input exceeds 2^15, and then exact powers
// of two: the common case is bit for bit the unscaled arithmetic.
template <int NW, int RT, bool TANH, bool LAST = false, int SCALE = 0, int H = MLP_H>
__device__ __forceinline__ void store_layer_h3(_Float16 *a_hi, _Float16 *a_lo, const f32x16 (&acc)[H / 64 / NW][RT][2], const float *bias,
                                               int wid, int lane, const float *w_out = nullptr, float (*yo)[3] = nullptr,
                                               const float *scale = nullptr) {
    F4 sc[2] = {{{1.f, 1.f, 1.f, 0.f}}, {{1.f, 1.f, 1.f, 0.f}}};
    if (SCALE != 0) {
        sc[0] = *reinterpret_cast<const F4 *>(scale + 4 * (lane & 31));
        if (RT == 2) sc[1] = *reinterpret_cast<const F4 *>(scale + 4 * (32 + (lane & 31)));
    }
    constexpr int COLS = H / NW, PITCH = H + 8;  // this wave's output features: H / 32 / NW column tiles of 32
    const int lane_off = (lane & 31) * PITCH + wid * COLS + 4 * (lane >> 5);
    _Float16 *const base[2][2] = {{a_hi + lane_off, a_hi + 32 * PITCH + lane_off},
                                  {a_lo + lane_off, a_lo + 32 * PITCH + lane_off}};
    const float *bl = bias + wid * COLS + 4 * (lane >> 5);
#pragma unroll
    for (int ct = 0; ct < H / 32 / NW; ++ct) {
        f32x2 bn[8];  // the biases of this lane's 16 features of the tile: four aligned 16-byte loads
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const F4 b4 = *reinterpret_cast<const F4 *>(bl + ct * 32 + 8 * q);
            bn[2 * q] = f32x2{b4.v[0], b4.v[1]};
            bn[2 * q + 1] = f32x2{b4.v[2], b4.v[3]};
        }
        F4 wo[3][4];  // LAST: the output layer's weights of the same 16 features, requested before the tanh arithmetic
        if (LAST) {
            const float *wl = w_out + wid * COLS + 4 * (lane >> 5) + ct * 32;
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) wo[j][q] = *reinterpret_cast<const F4 *>(wl + j * H + 8 * q);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x2 a = f32x2{acc[ct >> 1][rt][ct & 1][2 * i], acc[ct >> 1][rt][ct & 1][2 * i + 1]};
                if (SCALE == 1) v[i] = (a * sc[rt].v[0] + bn[i]) * sc[rt].v[1];
                else if (SCALE == 2) v[i] = a * sc[rt].v[2] + bn[i];
                else v[i] = a + bn[i];
            }
            if (TANH) {  // 1 - 2 / (exp(2x) + 1), exp(2x) = 2^(x * 2 log2(e))
                f32x2 e[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const f32x2 a = v[i] * 2.8853900817779268f;
                    e[i] = f32x2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)} + 1.0f;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) e[i] = f32x2{__builtin_amdgcn_rcpf(e[i].x), __builtin_amdgcn_rcpf(e[i].y)};
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = 1.0f - 2.0f * e[i];
            }
            if (LAST) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    f32x2 a = f32x2{0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        a = a + v[2 * q] * f32x2{wo[j][q].v[0], wo[j][q].v[1]} + v[2 * q + 1] * f32x2{wo[j][q].v[2], wo[j][q].v[3]};
                    yo[rt][j] += a.x + a.y;
                }
                continue;
            }
            half2v hi[8], lo[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) hi[i] = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(v[i].x, v[i].y));
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = v[i] - f32x2{(float)hi[i].x, (float)hi[i].y};
#pragma unroll
            for (int i = 0; i < 8; ++i) lo[i] = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(v[i].x, v[i].y));
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // registers 4q .. 4q + 3: features 8q .. 8q + 3 (+ lane, tile and wave parts)
                const int off = ct * 32 + 8 * q;
                *reinterpret_cast<half4v *>(base[0][rt] + off) = half4v{hi[2 * q].x, hi[2 * q].y, hi[2 * q + 1].x, hi[2 * q + 1].y};
                *reinterpret_cast<half4v *>(base[1][rt] + off) = half4v{lo[2 * q].x, lo[2 * q].y, lo[2 * q + 1].x, lo[2 * q + 1].y};
            }
        }
        // (one column tile at a time: unfenced, the scheduler lifts the bias / weight loads of all four tiles to the top of
        // the unrolled block and the kernel spills)
        __builtin_amdgcn_sched_barrier(0);
    }
}

#ifdef MPPI_STAMPS
__device__ unsigned long long g_mlp_phase[16];
#define PH(i)                                             \
    do {                                                  \
        const unsigned long long _n = clock64();          \
        ph[i] += _n - ph_t;                               \
        ph_t = _n;                                        \
    } while (0)
#else
#define PH(i) \
    do {      \
    } while (0)
#endif
// The path's room in LDS beside the buffers of a tile (mlp_stage_path): at H = 256 two workgroups share the CU's 160 KB,
// 80 KB each, and the activations, inputs and partial outputs take 78.8 KB of it
constexpr int W256_REF_LDS = 128;
constexpr int h3_ref_cap(int rt, int h) { return rt == 1 ? H3_REF_LDS_32 : h == 256 ? W256_REF_LDS : MLP_REF_LDS_MAX; }

// Several agents per launch (mppi_config.n_agents > 1): workgroup row a = blockIdx.y runs agent a, which sees
// the handle's parameters with its own nominal controls u + 2 T a, costs and waypoint outputs S / pout + K a, controller
// state st + a (x0, x0 index, iteration), noise (Philox stream noise_stream + a, or its tensor of the caller's ring) and
// record heads + 4 slots a, its reference path, obstacle table and the clock its circles were uploaded at (AgentScene; only a
// scene form reads iter0, in the static kernels the load is dead) -- the layout of k_rollout_fused<..., MULTI>, which
// k_finalize's batched path reads.  The
// records themselves: mlp_agent_records.  The single-agent kernels never call these, so their code stays what it was.
__device__ __forceinline__ KParams<float> mlp_agent(const KParams<float> &P, int a) {
    KParams<float> A = P;
    A.u += (size_t)a * 2 * P.T;
    A.S += (size_t)a * P.K;
    A.pout += (size_t)a * P.K;
    A.st += a;
    A.noise_stream += a;
    if (P.eps) A.eps += (size_t)a * P.K * P.T * 2;  // eps_tensor(A, iter, 0) == eps_tensor(P, iter, a)
    A.heads += (size_t)a * P.slots * 4;
    agent_scene(A, P.scenes, a);  // its path and obstacles: mlp_stage_path's "fits in LDS" falls out per agent
    A.iter0 = P.scenes[a].iter0;
    return A;
}
// Agent a's entry of the handle's model table (MlpParams[n_agents], mppi_set_agent_mlp), seen as CONSTANT memory: the host
// rewrites the table only between launches, the index is uniform over the workgroup, so every field arrives by a scalar load
// exactly as a field of the by-value kernel argument does (the kernel-argument segment is the same address space) -- and the
// weight pointers read from it are known to be global addresses, as kernel-argument pointers are (read through a generic
// pointer to the table they would be generic themselves and the weight stream would turn into flat loads, which wait on
// the LDS counter too).  A reference, not a copy: the layers index w_h / b_h by a run-time l, and a private copy of the
// struct would live in scratch.
using MlpParamsConst = const __attribute__((address_space(4))) MlpParams;
__device__ __forceinline__ MlpParamsConst &mlp_agent_model(const MlpParams *models, int a) { return ((MlpParamsConst *)models)[a]; }
__device__ __forceinline__ float *mlp_agent_records(const KParams<float> &P, float *partials, int a) {
    return partials + (size_t)a * P.slots * record_len(P.T, 4);
}

// The f16-split kernels: twelve wrappers (the last four: the fleet forms) around one textually included body (mppi_mlp_body.h, which lists what a wrapper has in
// scope).  The default-width family first: 512 x 3 and 512 x 2, NW waves on RT row tiles.
template <bool VIZ, int NW, int RT, int TERMS = 3>
__global__ __launch_bounds__(64 * NW, RT == 1 ? 2 : 1) void k_rollout_mlp_h3(const KParams<float> P, const MlpParams Q,
                                                               float *__restrict__ partials, const MlpViz V) {
    constexpr int H = MLP_H, scene_agent = 0;
    constexpr bool SCENE = false, ONE_HIDDEN = false, FLEET = false, PLAN = false;
    const FleetParams F{};
#include "mppi_mlp_body.h"
}
// several agents per launch, agent = blockIdx.y (grid (mlp_blocks(K, 64), n_agents)); no visualisation form.  `models`: every
// agent's MlpParams (its own weight buffers or the shared ones; one shape for all, mppi_set_agent_mlp): `Q` is this
// agent's entry (mlp_agent_model) where the single-agent kernel has its by-value argument
template <int NW, int RT, int TERMS>
__global__ __launch_bounds__(64 * NW, RT == 1 ? 2 : 1) void k_rollout_mlp_h3_agents(const KParams<float> P_all,
                                                                      const MlpParams *__restrict__ models,
                                                                      float *__restrict__ partials_all) {
    constexpr int H = MLP_H, scene_agent = 0;
    constexpr bool VIZ = false, SCENE = false, ONE_HIDDEN = false, FLEET = false, PLAN = false;
    const FleetParams F{};
    const KParams<float> P = mlp_agent(P_all, (int)blockIdx.y);
    MlpParamsConst &Q = mlp_agent_model(models, (int)blockIdx.y);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, (int)blockIdx.y);
    const MlpViz V{};
#include "mppi_mlp_body.h"
}

// ------------------------------------------------------------------------------------------
// Every other supported shape, H in {64, 128, 256, 512} x n_hidden in {1, 2, 3, 4}: the same body (kept as
// kernels of their own so that the 512 x 3 / 512 x 2 kernels compile to the code they always did), with H / 64 waves per
// workgroup, each owning 64 output columns of every layer (one pass of
// two 32-column tiles, as the 8-wave form of the 512-wide kernel), on a 64-sample tile: blockDim = H.  The LDS of a tile
// shrinks with H (38 KB at 64, 56 KB at 128, 79 KB at 256), so two (H = 256, 128) or four (H = 64) workgroups share a CU
// and one's serial part -- wave 0's controls, waypoint search, cost and Euler step -- runs under another's matrix work.
// ------------------------------------------------------------------------------------------
template <int H, bool VIZ>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_rollout_mlp_w(const KParams<float> P, const MlpParams Q, float *__restrict__ partials,
                                                                     const MlpViz V) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3, scene_agent = 0;
    constexpr bool SCENE = false, ONE_HIDDEN = true, FLEET = false, PLAN = false;
    const FleetParams F{};
#include "mppi_mlp_body.h"
}
// several agents per launch (see k_rollout_mlp_h3_agents)
template <int H>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_rollout_mlp_w_agents(const KParams<float> P_all,
                                                                            const MlpParams *__restrict__ models,
                                                                            float *__restrict__ partials_all) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3, scene_agent = 0;
    constexpr bool VIZ = false, SCENE = false, ONE_HIDDEN = true, FLEET = false, PLAN = false;
    const FleetParams F{};
    const KParams<float> P = mlp_agent(P_all, (int)blockIdx.y);
    MlpParamsConst &Q = mlp_agent_model(models, (int)blockIdx.y);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, (int)blockIdx.y);
    const MlpViz V{};
#include "mppi_mlp_body.h"
}

// ------------------------------------------------------------------------------------------
// The scene forms (mppi_config.obstacle_motion = 2): the same body with SCENE = true -- the moving table and the
// agent's MlpScene in `obs`, mlp_advance<true> -- so moving circles, obstacle tracks and a cost grid are priced along every
// learned rollout.  One form per width of k_rollout_mlp_w and one of the default 8-wave three-term k_rollout_mlp_h3, each
// single-agent and batched: ten symbols.  No visualisation form (the transition is the static kernels').  `scene_agent`: whose
// descriptors mlp_scene_at reads.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * 8, 1) void k_rollout_mlp_h3_scene(const KParams<float> P, const MlpParams Q, float *__restrict__ partials) {
    constexpr int H = MLP_H, NW = 8, RT = 2, TERMS = 3, scene_agent = 0;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = false, FLEET = false, PLAN = false;
    const FleetParams F{};
    const MlpViz V{};
#include "mppi_mlp_body.h"
}
__global__ __launch_bounds__(64 * 8, 1) void k_rollout_mlp_h3_scene_agents(const KParams<float> P_all, const MlpParams *__restrict__ models,
                                                                          float *__restrict__ partials_all) {
    constexpr int H = MLP_H, NW = 8, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = false, FLEET = false, PLAN = false;
    const FleetParams F{};
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, scene_agent);
    const MlpViz V{};
#include "mppi_mlp_body.h"
}
template <int H>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_rollout_mlp_w_scene(const KParams<float> P, const MlpParams Q, float *__restrict__ partials) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3, scene_agent = 0;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = true, FLEET = false, PLAN = false;
    const FleetParams F{};
    const MlpViz V{};
#include "mppi_mlp_body.h"
}
template <int H>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_rollout_mlp_w_scene_agents(const KParams<float> P_all,
                                                                                  const MlpParams *__restrict__ models,
                                                                                  float *__restrict__ partials_all) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = true, FLEET = false, PLAN = false;
    const FleetParams F{};
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, scene_agent);
    const MlpViz V{};
#include "mppi_mlp_body.h"
}

// ------------------------------------------------------------------------------------------
// The fleet forms (mppi_config.obstacle_motion = 3): a batch whose agents see each other.  The rollout kernels are
// the batched scene forms with FLEET = true: in velocity mode the mates are rows of the moving table (k_fleet_rows<float>), in
// plan mode points of the plan table behind SceneTable::plans.  The plan kernels write that table: the body with PLAN = true,
// one workgroup per agent (grid (1, n_agents)) with the agent's own model, at the front of every slot in k_fleet_plan's place.
// One of each per width of the _w family and one of the 8-wave three-term _h3 family: ten symbols.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * 8, 1) void k_rollout_mlp_h3_fleet_agents(const KParams<float> P_all, const MlpParams *__restrict__ models,
                                                                          float *__restrict__ partials_all) {
    constexpr int H = MLP_H, NW = 8, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = false, FLEET = true, PLAN = false;
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, scene_agent);
    const MlpViz V{};
    const FleetParams F{};
#include "mppi_mlp_body.h"
}
template <int H>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_rollout_mlp_w_fleet_agents(const KParams<float> P_all,
                                                                                  const MlpParams *__restrict__ models,
                                                                                  float *__restrict__ partials_all) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = true, ONE_HIDDEN = true, FLEET = true, PLAN = false;
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = mlp_agent_records(P_all, partials_all, scene_agent);
    const MlpViz V{};
    const FleetParams F{};
#include "mppi_mlp_body.h"
}
// the plan kernels: agent = blockIdx.y, its parameters and model as the batched rollouts see them; no records
__global__ __launch_bounds__(64 * 8, 1) void k_fleet_plan_mlp_h3(const KParams<float> P_all, const MlpParams *__restrict__ models,
                                                                const FleetParams F) {
    constexpr int H = MLP_H, NW = 8, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = false, ONE_HIDDEN = false, FLEET = false, PLAN = true;
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = nullptr;
    const MlpViz V{};
#include "mppi_mlp_body.h"
}
template <int H>
__global__ __launch_bounds__(H, H == 256 ? 2 : 1) void k_fleet_plan_mlp_w(const KParams<float> P_all, const MlpParams *__restrict__ models,
                                                                        const FleetParams F) {
    constexpr int NW = H / 64, RT = 2, TERMS = 3;
    constexpr bool VIZ = false, SCENE = false, ONE_HIDDEN = true, FLEET = false, PLAN = true;
    const int scene_agent = (int)blockIdx.y;
    const KParams<float> P = mlp_agent(P_all, scene_agent);
    MlpParamsConst &Q = mlp_agent_model(models, scene_agent);
    float *__restrict__ partials = nullptr;
    const MlpViz V{};
#include "mppi_mlp_body.h"
}
#undef PH
#ifdef MPPI_STAMPS
extern "C" int mppi_debug_mlp_phases(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mlp_phase), sizeof(unsigned long long) * 10);
}
#endif

// The forms of the f16-split rollout kernel (MPPI_MLP_FORM, for A/B runs): "4x64" one wave per SIMD, "8x64" two waves per
// SIMD, both on one 64-sample tile per workgroup.  (Tried and dropped: 32-sample tiles with two workgroups per CU, so that one
// workgroup's epilogues run under the other's GEMMs -- every weight byte then feeds half as many MFMAs, the weight stream
// from L2 doubles to ~85 B per clock and CU, and the launch went from 6.3 to 8.7 ms.)
// mppi_set_mlp captures the switch (Switches::mlp.form, these values; -1: H3_FORM_DEFAULT) together with MPPI_MLP_TERMS=2 --
// the split product without the a_lo b_hi term (see h3_mma) -- and MPPI_MLP_F32: a process compares forms with one
// handle, or one mppi_set_mlp call, per setting.
enum { H3_FORM_4x64 = 0, H3_FORM_8x64 = 1 };
int mlp_blocks(int K, int tile) { return (K + tile - 1) / tile; }

static size_t h3_shmem(int nw, int rt, int h = MLP_H) {
    const int m = 32 * rt;
    return sizeof(_Float16) * 2 * (m * (h + 8) + m * H3_ZPITCH) + sizeof(float) * (nw + 1) * m * 4 +
           sizeof(float) * 4 * h3_ref_cap(rt, h);
}
static_assert(2 * (sizeof(_Float16) * 2 * (64 * (256 + 8) + 64 * H3_ZPITCH) + sizeof(float) * 5 * 64 * 4 + sizeof(float) * 4 * W256_REF_LDS)
                  <= 160 * 1024, "two H = 256 workgroups per CU");

// Plan rows: the one place per kernel where template arguments meet the function to launch, its name as rocprofv3 prints it,
// its workgroup and its dynamic LDS (beyond 64 KB: launch_plan raises the attribute before the first launch on a device; the
// `lds_raised` flags live in the row's KernelEntry).  Three tables; their rows stand in the order the kernels have always been
// instantiated in, which is the order of the functions in the code object.
struct MlpKernel {
    const void *fn;
    KernelEntry e;
    int threads;
    size_t lds;
    KernelLaunch plan() { return plan_entry(fn, e, threads, lds); }
};
template <typename F> static const void *kfn(F *f) { return reinterpret_cast<const void *>(f); }
// k_rollout_mlp_w<H, VIZ> and its forms: H / 64 waves, 64-sample tiles
static size_t w_shmem(int h) { return h3_shmem(h / 64, 2, h); }
struct WSceneKernels { MlpKernel agents, one; };  // the scene handles' (obstacle_motion = 2)
template <int H> static WSceneKernels w_scene_rows() {
    return {{kfn(k_rollout_mlp_w_scene_agents<H>), KernelEntry("k_rollout_mlp_w_scene_agents<%d>", H), H, w_shmem(H)},
            {kfn(k_rollout_mlp_w_scene<H>), KernelEntry("k_rollout_mlp_w_scene<%d>", H), H, w_shmem(H)}};
}
struct WFleetKernels { MlpKernel rollout, plan; };  // the fleet handles' (obstacle_motion = 3)
template <int H> static WFleetKernels w_fleet_rows() {
    return {{kfn(k_rollout_mlp_w_fleet_agents<H>), KernelEntry("k_rollout_mlp_w_fleet_agents<%d>", H), H, w_shmem(H)},
            {kfn(k_fleet_plan_mlp_w<H>), KernelEntry("k_fleet_plan_mlp_w<%d>", H), H, w_shmem(H)}};
}
struct WKernels { MlpKernel viz, agents, one; };
template <int H> static WKernels w_rows() {
    return {{kfn(k_rollout_mlp_w<H, true>), KernelEntry("k_rollout_mlp_w<%d, true>", H), H, w_shmem(H)},
            {kfn(k_rollout_mlp_w_agents<H>), KernelEntry("k_rollout_mlp_w_agents<%d>", H), H, w_shmem(H)},
            {kfn(k_rollout_mlp_w<H, false>), KernelEntry("k_rollout_mlp_w<%d, false>", H), H, w_shmem(H)}};
}
// by width: 64, 128, 256, 512 (a further width is one more entry of each, and of plan_mlp's index)
static WSceneKernels w_scene_kernels[] = {w_scene_rows<64>(), w_scene_rows<128>(), w_scene_rows<256>(), w_scene_rows<512>()};
static WKernels w_kernels[] = {w_rows<64>(), w_rows<128>(), w_rows<256>(), w_rows<512>()};
static WFleetKernels w_fleet_kernels[] = {w_fleet_rows<64>(), w_fleet_rows<128>(), w_fleet_rows<256>(), w_fleet_rows<512>()};
// 512 x 3 and 512 x 2: the forms of k_rollout_mlp_h3, and the f32-input kernel
enum { H3_VIZ_8, H3_VIZ_4, H3_AGENTS, H3_F32, H3_8_TERMS_2, H3_8, H3_4, H3_SCENE, H3_SCENE_AGENTS };
static MlpKernel h3_kernels[] = {
    {kfn(k_rollout_mlp_h3<true, 8, 2, 3>), KernelEntry("k_rollout_mlp_h3<true, 8, 2, 3>"), 64 * 8, h3_shmem(8, 2)},
    {kfn(k_rollout_mlp_h3<true, 4, 2, 3>), KernelEntry("k_rollout_mlp_h3<true, 4, 2, 3>"), 64 * 4, h3_shmem(4, 2)},
    {kfn(k_rollout_mlp_h3_agents<8, 2, 3>), KernelEntry("k_rollout_mlp_h3_agents<8, 2, 3>"), 64 * 8, h3_shmem(8, 2)},
    // (the name up to the parenthesis: the other kernels' names begin with this one's)
    {kfn(k_rollout_mlp), KernelEntry("k_rollout_mlp("), 64 * MLP_WAVES,
     sizeof(float) * (MLP_M * MLP_PITCH + MLP_M * 8 + MLP_WAVES * MLP_M * 4) + sizeof(float) * 4 * MLP_REF_LDS_MAX},
    {kfn(k_rollout_mlp_h3<false, 8, 2, 2>), KernelEntry("k_rollout_mlp_h3<false, 8, 2, 2>"), 64 * 8, h3_shmem(8, 2)},
    {kfn(k_rollout_mlp_h3<false, 8, 2, 3>), KernelEntry("k_rollout_mlp_h3<false, 8, 2, 3>"), 64 * 8, h3_shmem(8, 2)},
    {kfn(k_rollout_mlp_h3<false, 4, 2, 3>), KernelEntry("k_rollout_mlp_h3<false, 4, 2, 3>"), 64 * 4, h3_shmem(4, 2)},
    {kfn(k_rollout_mlp_h3_scene), KernelEntry("k_rollout_mlp_h3_scene"), 64 * 8, h3_shmem(8, 2)},
    {kfn(k_rollout_mlp_h3_scene_agents), KernelEntry("k_rollout_mlp_h3_scene_agents"), 64 * 8, h3_shmem(8, 2)},
};
static MlpKernel h3_fleet_rollout = {kfn(k_rollout_mlp_h3_fleet_agents), KernelEntry("k_rollout_mlp_h3_fleet_agents"), 64 * 8, h3_shmem(8, 2)};
static MlpKernel h3_fleet_plan = {kfn(k_fleet_plan_mlp_h3), KernelEntry("k_fleet_plan_mlp_h3"), 64 * 8, h3_shmem(8, 2)};

// `fleet`: a fleet handle (obstacle_motion = 3; always a batch): the fleet forms of the batched scene kernels
RolloutPlan plan_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const MlpViz *viz, bool fleet) {
    const bool f8 = (sw.mlp.form < 0 ? H3_FORM_DEFAULT : sw.mlp.form) == H3_FORM_8x64;
    const int agents = !viz && P.n_agents > 1 ? P.n_agents : 1;
    // a scene handle (obstacle_motion = 2: make_params marks its launches OBS_MOTION_SCENE) takes the scene form of its shape;
    // the visualisation rollouts and the batched transition price nothing and keep the static kernels
    const bool scene = !viz && P.obs_motion == OBS_MOTION_SCENE;
    // the one dispatch on width: 512 x 3 / 512 x 2 have their own family (mppi_set_mlp admits only these four widths)
    const bool h3 = mlp_shape_is_h3(Q.hidden, Q.n_hidden);
    const int wi = Q.hidden == 64 ? 0 : Q.hidden == 128 ? 1 : Q.hidden == 256 ? 2 : 3;
    // MPPI_MLP_FORM / MPPI_MLP_TERMS / MPPI_MLP_F32 concern the single-agent rollouts of 512 x 3 / 512 x 2 only: scene handles
    // and batches take the default form (mppi_set_mlp refuses the f32-input cases for both), the visualisation rollouts the
    // f16-split kernel of the form whichever rollout kernel MPPI_MLP_F32 selects (both weight sets are packed)
    const bool batch = agents > 1;
    MlpKernel &k = scene && batch && fleet ? (h3 ? h3_fleet_rollout : w_fleet_kernels[wi].rollout)
                   : scene && h3 ? h3_kernels[batch ? H3_SCENE_AGENTS : H3_SCENE]
                   : scene     ? (batch ? w_scene_kernels[wi].agents : w_scene_kernels[wi].one)
                   : !h3       ? (viz ? w_kernels[wi].viz : batch ? w_kernels[wi].agents : w_kernels[wi].one)
                   : viz       ? h3_kernels[f8 ? H3_VIZ_8 : H3_VIZ_4]
                   : batch     ? h3_kernels[H3_AGENTS]
                   : !Q.use_h3 ? h3_kernels[H3_F32]
                   : !f8       ? h3_kernels[H3_4]
                               : h3_kernels[sw.mlp.terms == 2 ? H3_8_TERMS_2 : H3_8];
    RolloutPlan p;
    p.k = k.plan();
    p.records = mlp_blocks(P.K, MLP_M);  // every kernel: one 64-sample tile, one softmin record, per workgroup
    // viz: the samples' workgroups (when their trajectories are wanted) and one for the nominal sequence (likewise)
    if (viz) p.k.grid = dim3(viz->ex ? mlp_blocks(viz->en, MLP_M) : (viz->smp ? p.records : 0) + (viz->opt ? 1 : 0));
    else p.k.grid = dim3(p.records, agents);
    return p;
}
// `models`: the handle's device table MlpParams[n_agents] -- what the `agents` branch of plan_mlp (grid.y = the agents) takes
// in place of Q; every other kernel carries Q by value
void launch_mlp(const RolloutPlan &plan, const KParams<float> &P, const MlpParams &Q, const MlpParams *models, void *partials,
                const MlpViz *viz, hipStream_t s) {
    const MlpViz none{};
    const bool agents = plan.k.grid.y > 1;
    void *args[] = {const_cast<KParams<float> *>(&P), agents ? (void *)&models : (void *)const_cast<MlpParams *>(&Q), &partials,
                    const_cast<MlpViz *>(viz ? viz : &none)};
    launch_plan(plan.k, args, s);  // (k_rollout_mlp and the _agents kernels take no MlpViz)
}

// The launch at the front of a learned fleet handle's slot in plan mode (F.plans set), in launch_fleet_rows' place: every
// agent's plan through its own model, one workgroup per agent.  Q: the batch's shape (hidden, n_hidden).
void launch_fleet_plan_mlp(const KParams<float> &P, const MlpParams &Q, const MlpParams *models, const FleetParams &F, hipStream_t s) {
    const int wi = Q.hidden == 64 ? 0 : Q.hidden == 128 ? 1 : Q.hidden == 256 ? 2 : 3;
    MlpKernel &k = mlp_shape_is_h3(Q.hidden, Q.n_hidden) ? h3_fleet_plan : w_fleet_kernels[wi].plan;
    KernelLaunch l = k.plan();
    l.grid = dim3(1, F.n_agents);
    void *args[] = {const_cast<KParams<float> *>(&P), (void *)&models, const_cast<FleetParams *>(&F)};
    launch_plan(l, args, s);
}

void launch_viz_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const float *u_before, const float *u_upd,
                    long long iter, float *opt, float *smp, hipStream_t s) {
    if (!opt && !smp) return;
    const MlpViz v{u_before, u_upd, opt, smp, (unsigned)iter, smp ? 0 : mlp_blocks(P.K, MLP_M), nullptr, nullptr, nullptr, 0};
    launch_mlp(plan_mlp(P, Q, sw, &v), P, Q, nullptr, nullptr, &v, s);
}

void launch_eval_mlp(const KParams<float> &P, const MlpParams &Q, const Switches &sw, const float *x, const float *v, int n,
                     float *out, hipStream_t s) {
    const MlpViz e{nullptr, nullptr, nullptr, nullptr, 0u, 0, x, v, out, n};
    launch_mlp(plan_mlp(P, Q, sw, &e), P, Q, nullptr, nullptr, &e, s);
}

// Host-side packing of a torch Linear weight [n_out][n_in] (n_out a multiple of 32) into fragment order:
// packed[ct (n_out / 32)][g (n_groups)][lane (64)][s (4)] = W[32 ct + (lane & 31)][8 g + 4 (lane >> 5) + s] (0 beyond n_in)
void pack_linear(const float *w, int n_in, float *packed, int n_out) {
    const int n_groups = (n_in + 7) / 8;
    for (int ct = 0; ct < n_out / 32; ++ct)
        for (int g = 0; g < n_groups; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int n = 32 * ct + (lane & 31), kk = 8 * g + 4 * (lane >> 5) + s;
                    packed[(((size_t)ct * n_groups + g) * 64 + lane) * 4 + s] = kk < n_in ? w[(size_t)n * n_in + kk] : 0.f;
                }
}

// IEEE binary16 of a float, round to nearest even (host; the kernels' v_cvt_f16_f32 does the same)
static unsigned short f32_to_f16_bits(float f) {
    unsigned int x;
    memcpy(&x, &f, 4);
    const unsigned int sign = (x >> 16) & 0x8000u;
    const int exp = (int)((x >> 23) & 0xffu) - 127 + 15;
    unsigned int man = x & 0x7fffffu;
    if (((x >> 23) & 0xffu) == 0xffu) return (unsigned short)(sign | 0x7c00u | (man ? 0x200u : 0u));
    if (exp >= 31) return (unsigned short)(sign | 0x7c00u);
    if (exp <= 0) {  // subnormal or zero
        if (exp < -10) return (unsigned short)sign;
        man |= 0x800000u;
        const int shift = 14 - exp;
        unsigned int h = man >> shift;
        const unsigned int rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) ++h;
        return (unsigned short)(sign | h);
    }
    unsigned int h = ((unsigned int)exp << 10) | (man >> 13);
    const unsigned int rem = man & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;  // (a carry into the exponent is the right result)
    return (unsigned short)(sign | h);
}
static float f16_bits_to_f32(unsigned short h) {
    const unsigned int sign = (unsigned int)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    unsigned int x;
    if (exp == 0) {
        if (man == 0) x = sign;
        else {
            int e = -1;
            unsigned int m = man;
            do { ++e; m <<= 1; } while (!(m & 0x400u));
            x = sign | ((unsigned int)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13);
        }
    } else if (exp == 31) x = sign | 0x7f800000u | (man << 13);
    else x = sign | ((exp - 15 + 127) << 23) | (man << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// Host-side packing for the f16-split kernels: W [n_out][n_in] -> two f16 planes (hi, then lo) in fragment order
// plane[ct (n_out / 32)][s (n_steps)][lane (64)][j (8)] = W[32 ct + (lane & 31)][16 s + 8 (lane >> 5) + j]  (0 beyond n_in)
void pack_linear_h3(const float *w, int n_in, unsigned short *packed, int n_out) {
    const int n_steps = (n_in + 15) / 16;
    const size_t plane = (size_t)(n_out / 32) * n_steps * 64 * 8;
    for (int ct = 0; ct < n_out / 32; ++ct)
        for (int s = 0; s < n_steps; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int n = 32 * ct + (lane & 31), kk = 16 * s + 8 * (lane >> 5) + j;
                    const float v = kk < n_in ? w[(size_t)n * n_in + kk] : 0.f;
                    const unsigned short hi = f32_to_f16_bits(v);
                    const unsigned short lo = f32_to_f16_bits(v - f16_bits_to_f32(hi));
                    const size_t o = (((size_t)ct * n_steps + s) * 64 + lane) * 8 + j;
                    packed[o] = hi;
                    packed[plane + o] = lo;
                }
}

}  // namespace mppi
