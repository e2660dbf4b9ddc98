// mppi_mlp_body.h: the one body of every f16-split rollout kernel -- k_rollout_mlp_h3, k_rollout_mlp_w, their several-agents-
// per-launch forms, their scene and fleet forms and the fleet's plan kernels (mppi_mlp.hip): wrappers include it textually, so
// that each kernel compiles to exactly the code it did as a self-contained kernel (an inlined __device__ body is optimised before it is inlined and changed
// the register allocation and scratch of 21 of the 29 kernels: DESIGN 3.6.3).  Not a header: no include guard, nothing else may
// include it.  In scope at the point of inclusion:
//   P, Q, partials, V   the kernel's (or this agent's) parameters, model, records and visualisation block
//   H, NW, RT, TERMS    the layers' width, waves per workgroup, row tiles of 32 samples, terms of the split product
//   VIZ, SCENE          the visualisation form; the scene form (moving table and MlpScene in `obs`, mlp_advance<true>)
//   scene_agent         whose descriptors a scene form prices (0 where SCENE is false)
//   ONE_HIDDEN          constexpr bool: n_hidden == 1 is admitted (the _w family; the _h3 kernels run 2 or 3 hidden layers)
//   FLEET               constexpr bool: a scene form that also tests the mates' plans (mlp_advance<true, true>)
//   PLAN, F             constexpr bool: the fleet's plan form -- every row of the tile carries this agent's NOMINAL sequence (control t
//                       at step t, clamped where the rollout clamps), nothing is priced, lane 0 stores point t + 1 of the agent's
//                       plan into F.plans and the clearance record follows the step loop; F: the launch's FleetParams (else unused)
#ifdef MPPI_STAMPS
    unsigned long long ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ph_t = clock64();
#endif
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int M = 32 * RT;  // samples of this workgroup's tile
    constexpr int PITCH = H + 8;                           // (520 at 512)
    _Float16 *a_hi = reinterpret_cast<_Float16 *>(smem);   // [M][H + 8]
    _Float16 *a_lo = a_hi + M * PITCH;
    _Float16 *z_hi = a_lo + M * PITCH;                     // [M][24] layer-0 input rows {x, y, yaw, v, w, 0 ...}: one k-step
    _Float16 *z_lo = z_hi + M * H3_ZPITCH;
    float *ypart = reinterpret_cast<float *>(z_lo + M * H3_ZPITCH);  // [NW][M][4]
    float *zscale = ypart + NW * M * 4;                             // [M][4] per-sample {s0, 1 / s1, s1, 0} (H3Scale)
    float *ref_lds = zscale + M * 4;                                // [n_ref][4] when the path fits
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int k0 = ((int)blockIdx.x + (VIZ ? V.block0 : 0)) * M, k = k0 + lane;
    // (the plan form prices nothing: it neither stages the path nor loads an obstacle table)
    const KParams<float> PL = PLAN ? P : mlp_stage_path(P, ref_lds, h3_ref_cap(RT, H));
    const DevState sv = load_state(P, P.st);
    const MlpObs<SCENE> obs = PLAN ? MlpObs<SCENE>{} : mlp_obs_load<SCENE>(P, sv, lane, scene_agent);  // what wave 0's advance call prices against
    if (!VIZ && !PLAN && k0 + M <= sv.k_start) return;
    const bool in_tile = lane < M;  // (a 32-sample tile: the upper half of wave 0 carries no sample)
    const bool valid = in_tile && k < P.K, live = valid && k >= sv.k_start;
    // VIZ: the workgroup behind the samples' carries the nominal sequence in its lane 0
    const bool eval = VIZ && V.ex != nullptr, eval_row = eval && k < V.en;
    const bool opt_row = VIZ && !eval && k0 >= P.K && lane == 0 && V.opt != nullptr;
    const bool smp_row = VIZ && !eval && valid && V.smp != nullptr;
    const int c = sv.c;
    const unsigned iter = (unsigned)sv.iter;
    MlpLane L{(float)sv.x0[0], (float)sv.x0[1], (float)sv.x0[2], 0.f, c};
    if (eval_row) { L.x = V.ex[3 * k]; L.y = V.ex[3 * k + 1]; L.yaw = V.ex[3 * k + 2]; }
    const int n_steps = eval ? 1 : P.T;
    const bool exploit = (k + P.k_offset) < P.n_exploit;
    f32x16 acc[H / 64 / NW][RT][2];
    PlanPoint<float> *plan_out = nullptr;
    if constexpr (PLAN) {
        plan_out = static_cast<PlanPoint<float> *>(F.plans) + (size_t)scene_agent * (P.T + 1);
        if (threadIdx.x == 0) plan_out[0] = PlanPoint<float>{L.x, L.y};
    }
    if (wid == 0 && in_tile) {  // the padding of the layer-0 rows stays zero
        for (int q = 0; q < H3_ZPITCH; ++q) { z_hi[lane * H3_ZPITCH + q] = (_Float16)0.f; z_lo[lane * H3_ZPITCH + q] = (_Float16)0.f; }
    }
    for (int t = 0; t < n_steps; ++t) {
        float u0 = 0, u1 = 0, v0 = 0, v1 = 0;
        if (wid == 0) {
            if constexpr (PLAN) mlp_controls_plan(P, t, v0, v1);
            else if (eval) {
                if (eval_row) { v0 = V.ev[2 * k]; v1 = V.ev[2 * k + 1]; }
            } else if (VIZ) mlp_controls_viz(P, V, k, t, smp_row, opt_row, exploit, v0, v1);
            else mlp_controls(P, iter, k, t, valid, exploit, u0, u1, v0, v1);
            const float z[5] = {L.x, L.y, L.yaw, v0, v1};
            const H3Scale hs = h3_scale(z, Q.in_gain, Q.in_bias);
            if (in_tile) {
                *reinterpret_cast<F4 *>(zscale + 4 * lane) = F4{{hs.s0, hs.inv_s1, hs.s1, 0.f}};
#pragma unroll
                for (int q = 0; q < 5; ++q) split_h3(z[q] * hs.inv_s0, z_hi[lane * H3_ZPITCH + q], z_lo[lane * H3_ZPITCH + q]);
            }
        }
        __syncthreads();
        PH(0);
        gemm_input_h3<NW, RT, H>(acc, z_hi, z_lo, Q.h3_w_in, wid, lane);
        PH(1);
        store_layer_h3<NW, RT, false, false, 1, H>(a_hi, a_lo, acc, Q.b_in, wid, lane, nullptr, nullptr, zscale);
        H3Ring ring;
        h3_prime_layer<NW, H>(Q.h3_w_h[0], wid, lane, ring);
        PH(2);
        __syncthreads();
        PH(3);
        const int l_last = Q.n_hidden - 1;  // (1 to 4 hidden layers, mppi_set_mlp)
        for (int l = 0; l < l_last; ++l) {
            gemm_layer_h3<NW, RT, TERMS, H>(acc, a_hi, a_lo, Q.h3_w_h[l], wid, lane, ring);
            PH(4);
            __syncthreads();
            PH(5);
            if (l == 0) store_layer_h3<NW, RT, true, false, 2, H>(a_hi, a_lo, acc, Q.b_h[l], wid, lane, nullptr, nullptr, zscale);
            else store_layer_h3<NW, RT, true, false, 0, H>(a_hi, a_lo, acc, Q.b_h[l], wid, lane);
            h3_prime_layer<NW, H>(Q.h3_w_h[l + 1], wid, lane, ring);
            PH(6);
            __syncthreads();
            PH(7);
        }
        {   // the last hidden layer and out_layer (Linear(H -> 3), :35) in its epilogue: this wave's share of the H inputs
            gemm_layer_h3<NW, RT, TERMS, H>(acc, a_hi, a_lo, Q.h3_w_h[l_last], wid, lane, ring);
            PH(4);
            float yo[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            if (ONE_HIDDEN && l_last == 0)  // one hidden layer: it is also the first, its accumulators those of h0 / s1
                store_layer_h3<NW, RT, true, true, 2, H>(a_hi, a_lo, acc, Q.b_h[0], wid, lane, Q.w_out, yo, zscale);
            else store_layer_h3<NW, RT, true, true, 0, H>(a_hi, a_lo, acc, Q.b_h[l_last], wid, lane, Q.w_out, yo);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {  // the two lane halves hold the two halves of a sample's features
                F4 o;
#pragma unroll
                for (int j = 0; j < 3; ++j) o.v[j] = yo[rt][j] + __shfl_xor(yo[rt][j], 32);
                o.v[3] = 0.f;
                if (lane < 32) *reinterpret_cast<F4 *>(ypart + (wid * M + rt * 32 + lane) * 4) = o;
            }
        }
        PH(8);
        __syncthreads();
        if (wid == 0) {
            float r0 = Q.b_out[0], r1 = Q.b_out[1], r2 = Q.b_out[2];
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const F4 o = *reinterpret_cast<const F4 *>(ypart + (w * M + (in_tile ? lane : 0)) * 4);
                r0 += o.v[0];
                r1 += o.v[1];
                r2 += o.v[2];
            }
            if constexpr (PLAN) {
                mlp_euler(P, r0, r1, r2, v0, v1, L);
                if (lane == 0) plan_out[t + 1] = PlanPoint<float>{L.x, L.y};
            } else if (VIZ) {
                mlp_euler(P, r0, r1, r2, v0, v1, L);
                float *dst = eval_row ? V.eout + (size_t)k * 3
                             : opt_row ? V.opt + (size_t)t * 3 : smp_row ? V.smp + ((size_t)k * P.T + t) * 3 : nullptr;
                if (dst) { dst[0] = L.x; dst[1] = L.y; dst[2] = L.yaw; }
            } else {
                mlp_advance<SCENE, FLEET>(PL, obs, c, t, r0, r1, r2, u0, u1, v0, v1, L);
            }
        }
        PH(9);
    }
    if constexpr (PLAN) {
        if (wid == 0) fleet_clearance(F, scene_agent, lane);
    } else if (!VIZ && wid == 0) mlp_record(P, partials, iter, k, c, valid, live, L, lane);
#ifdef MPPI_STAMPS
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && wid == (NW > 1 ? 1 : 0))
        for (int i = 0; i < 10; ++i) g_mlp_phase[i] = ph[i];
#endif
