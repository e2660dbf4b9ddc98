// Test-only harness around the device primitives (mathfn.h, wave_ops.h, philox.h, mppi_device.h -- the pieces of the
// one-launch waypoint index, lb_*, among them): libmppi_prims.so.
// Every entry point takes HOST pointers, allocates, copies in, launches one tiny kernel, synchronises, copies out, frees and
// returns the hipError_t as an int.  Also the rescale merge of mppi_merge.h in the product's instantiations (merge_combine<A,
// 256, 1 / 2>, merge_abi<A>), on buffers allocated as the product allocates them.  Wave-level kernels run as ONE block of 64 threads with every lane active; the search
// kernels only STORE the index a search returns and never use it as an address.  tests/test_gpu_primitives.py drives it.
#include <hip/hip_runtime.h>

#include <vector>

#include "mppi_device.h"
#include "mppi_merge.h"

namespace {

using namespace mppi;

struct Scope {  // device buffers of one call, freed on every way out
    std::vector<void *> ptrs;
    ~Scope() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    hipError_t alloc(void **d, size_t bytes) {
        const hipError_t e = hipMalloc(d, bytes ? bytes : 1);
        if (e == hipSuccess) ptrs.push_back(*d);
        return e;
    }
    template <typename T> hipError_t in(T *&d, const T *h, size_t n) {
        hipError_t e = alloc((void **)&d, n * sizeof(T));
        if (e == hipSuccess && n) e = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    template <typename T> hipError_t out(T *&d, size_t n) {
        hipError_t e = alloc((void **)&d, n * sizeof(T));
        if (e == hipSuccess) e = hipMemset(d, 0xff, n * sizeof(T) ? n * sizeof(T) : 1);
        return e;
    }
};

#define CK(expr)                                \
    do {                                        \
        const hipError_t e_ = (expr);           \
        if (e_ != hipSuccess) return (int)e_;   \
    } while (0)

template <typename T> hipError_t finish(T *h, const T *d, size_t n) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && n) e = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    return e;
}

// ------------------------------------------------------------------------------------------ mathfn
enum { M_SINCOS = 0, M_TAN, M_PYMOD, M_EXP, M_CLAMP };

template <typename R> __global__ __launch_bounds__(256) void k_map(int fn, const R *a, R b, R *o0, R *o1, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const R x = a[i];
    switch (fn) {
        case M_SINCOS: { R s, c; mf::sincos_(x, s, c); o0[i] = s; o1[i] = c; break; }
        case M_TAN: o0[i] = mf::tan_(x); break;
        case M_PYMOD: o0[i] = mf::pymod(x, b); break;
        case M_EXP: o0[i] = mf::exp_(x); break;
        default: o0[i] = mf::clamp(x, b); break;
    }
}

template <typename R> int run_map(int fn, const R *a, R b, R *o0, R *o1, int n) {
    if (n < 0 || n > (1 << 21) || fn < M_SINCOS || fn > M_CLAMP) return (int)hipErrorInvalidValue;
    Scope sc;
    R *da, *d0, *d1;
    CK(sc.in(da, a, n));
    CK(sc.out(d0, n));
    CK(sc.out(d1, n));
    if (n) k_map<R><<<(n + 255) / 256, 256>>>(fn, da, b, d0, d1, n);
    CK(finish(o0, d0, n));
    if (o1) CK(hipMemcpy(o1, d1, (size_t)n * sizeof(R), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ wave_ops
enum { V_SCAN = 0, V_HALF, V_ROW, V_SEG1, V_SEG2, V_REDUCE };

template <typename Op, typename R> __device__ __forceinline__ R scan_variant(int variant, R x) {
    switch (variant) {
        case V_SCAN: return wv::scan_incl<Op>(x);
        case V_HALF: return wv::scan_incl_half<Op>(x);
        case V_ROW: return wv::scan_incl_row<Op>(x);
        case V_SEG1: return wv::scan_incl_seg<Op, 1>(x);
        case V_SEG2: return wv::scan_incl_seg<Op, 2>(x);
        default: return wv::reduce<Op>(x);
    }
}

// op 0: OpAdd (fp) / OpMinInt (int), op 1: OpMin (fp) / OpMaxInt (int)
template <typename R> __global__ __launch_bounds__(64) void k_scan(int op, int variant, const R *in, R *out) {
    const R x = in[threadIdx.x];
    out[threadIdx.x] = op == 0 ? scan_variant<wv::OpAdd>(variant, x) : scan_variant<wv::OpMin>(variant, x);
}
template <> __global__ __launch_bounds__(64) void k_scan<int>(int op, int variant, const int *in, int *out) {
    const int x = in[threadIdx.x];
    out[threadIdx.x] = op == 0 ? scan_variant<wv::OpMinInt>(variant, x) : scan_variant<wv::OpMaxInt>(variant, x);
}

template <typename R> int run_scan(int op, int variant, const R *in, R *out) {
    if (op < 0 || op > 1 || variant < V_SCAN || variant > V_REDUCE) return (int)hipErrorInvalidValue;
    Scope sc;
    R *di, *dout;
    CK(sc.in(di, in, 64));
    CK(sc.out(dout, 64));
    k_scan<R><<<1, 64>>>(op, variant, di, dout);
    return (int)finish(out, dout, 64);
}

// variant 0: shift_up1, 1: shift_up1_half, 2: shift_up1_seg<1>, 3: shift_up1_seg<2>
template <typename R> __global__ __launch_bounds__(64) void k_shift(int variant, const R *in, R carry, R *out) {
    const R x = in[threadIdx.x];
    R y;
    switch (variant) {
        case 0: y = wv::shift_up1(x, carry); break;
        case 1: y = wv::shift_up1_half(x, carry); break;
        case 2: y = wv::shift_up1_seg<1>(x, carry); break;
        default: y = wv::shift_up1_seg<2>(x, carry); break;
    }
    out[threadIdx.x] = y;
}
template <typename R> int run_shift(int variant, const R *in, R carry, R *out) {
    if (variant < 0 || variant > 3) return (int)hipErrorInvalidValue;
    Scope sc;
    R *di, *dout;
    CK(sc.in(di, in, 64));
    CK(sc.out(dout, 64));
    k_shift<R><<<1, 64>>>(variant, di, carry, dout);
    return (int)finish(out, dout, 64);
}

// out[l][lane] = read_lane(x, l)
template <typename R> __global__ __launch_bounds__(64) void k_read_lane(const R *in, R *out) {
    const R x = in[threadIdx.x];
    for (int l = 0; l < 64; ++l) out[64 * l + threadIdx.x] = wv::read_lane(x, l);
}
template <typename R> int run_read_lane(const R *in, R *out) {
    Scope sc;
    R *di, *dout;
    CK(sc.in(di, in, 64));
    CK(sc.out(dout, 64 * 64));
    k_read_lane<R><<<1, 64>>>(di, dout);
    return (int)finish(out, dout, 64 * 64);
}

template <typename R> __global__ __launch_bounds__(64) void k_shfl_xor(int m, const R *in, R *out) {
    out[threadIdx.x] = wv::shfl_xor(in[threadIdx.x], m);
}
template <typename R> int run_shfl_xor(int m, const R *in, R *out) {
    if (m < 1 || m > 63) return (int)hipErrorInvalidValue;
    Scope sc;
    R *di, *dout;
    CK(sc.in(di, in, 64));
    CK(sc.out(dout, 64));
    k_shfl_xor<R><<<1, 64>>>(m, di, dout);
    return (int)finish(out, dout, 64);
}

template <typename R> __global__ __launch_bounds__(64) void k_argmin(const R *d_in, const int *j_in, R *d_out, int *j_out) {
    R d = d_in[threadIdx.x];
    int j = j_in[threadIdx.x];
    wv::argmin_first(d, j);
    d_out[threadIdx.x] = d;
    j_out[threadIdx.x] = j;
}
template <typename R> int run_argmin(const R *d_in, const int *j_in, R *d_out, int *j_out) {
    Scope sc;
    R *dd, *dod;
    int *dj, *doj;
    CK(sc.in(dd, d_in, 64));
    CK(sc.in(dj, j_in, 64));
    CK(sc.out(dod, 64));
    CK(sc.out(doj, 64));
    k_argmin<R><<<1, 64>>>(dd, dj, dod, doj);
    CK(finish(d_out, dod, 64));
    return (int)hipMemcpy(j_out, doj, 64 * sizeof(int), hipMemcpyDeviceToHost);
}

template <typename R> __global__ __launch_bounds__(64) void k_ordered_sum(R acc, const R *v, int first, int n, R *out) {
    out[threadIdx.x] = wv::ordered_sum(acc, v[threadIdx.x], first, n);
}
template <typename R> int run_ordered_sum(R acc, const R *v, int first, int n, R *out) {
    if (first < 0 || n < 0 || first + n > 64) return (int)hipErrorInvalidValue;
    Scope sc;
    R *dv, *dout;
    CK(sc.in(dv, v, 64));
    CK(sc.out(dout, 64));
    k_ordered_sum<R><<<1, 64>>>(acc, dv, first, n, dout);
    return (int)finish(out, dout, 64);
}

// ------------------------------------------------------------------------------------------ searches
// out[row][64]: 0 nearest_in_window, 1 nearest_in_window_lds, 2..5 nearest_in_window_split (split 2, 4, 8, 16: lanes
// < 64 / split hold a result, the others -1), 6 nearest_uniform and 7 nearest_x0 for query q in entry q, 8: 1 where every
// lane of the wave got the same result from the two wave-level searches of query q
constexpr int SEARCH_ROWS = 9;

template <typename R>
__global__ __launch_bounds__(64) void k_search(const R *ref, int c, int wlen, const R *qx, const R *qy, int *out) {
    __shared__ RefPair<R> sh[WINDOW_LDS_MAX / 2];
    const int lane = threadIdx.x;
    const R x = qx[lane], y = qy[lane];
    stage_window(sh, ref, c, wlen, lane, 64);
    __syncthreads();
    out[0 * 64 + lane] = nearest_in_window(ref, c, wlen, x, y);
    out[1 * 64 + lane] = nearest_in_window_lds(sh, c, wlen, x, y);
    int row = 2;
    for (int split = 2; split <= 16; split <<= 1, ++row) {
        const int r = nearest_in_window_split(sh, c, wlen, x, y, split, lane);
        out[row * 64 + lane] = lane < 64 / split ? r : -1;
    }
    int mine_u = -1, mine_x0 = -1, same = 0;
    for (int q = 0; q < 64; ++q) {
        const R xq = wv::read_lane(x, q), yq = wv::read_lane(y, q);
        const int ru = nearest_uniform(ref, c, wlen, xq, yq, lane);
        const int rx = nearest_x0(ref, c, wlen, (double)xq, (double)yq, lane);
        const int all_same = __all(ru == wv::read_lane(ru, 0) && rx == wv::read_lane(rx, 0));
        if (lane == q) { mine_u = ru; mine_x0 = rx; same = all_same; }
    }
    out[6 * 64 + lane] = mine_u;
    out[7 * 64 + lane] = mine_x0;
    out[8 * 64 + lane] = same;
}

template <typename R> int run_search(const R *ref, int n_ref, int c, int wlen, const R *qx, const R *qy, int *out) {
    if (n_ref < 1 || c < 0 || wlen < 1 || wlen > WINDOW_LDS_MAX || c + wlen > n_ref) return (int)hipErrorInvalidValue;
    Scope sc;
    R *dref, *dx, *dy;
    int *dout;
    CK(sc.in(dref, ref, (size_t)n_ref * 4));
    CK(sc.in(dx, qx, 64));
    CK(sc.in(dy, qy, 64));
    CK(sc.out(dout, SEARCH_ROWS * 64));
    k_search<R><<<1, 64>>>(dref, c, wlen, dx, dy, dout);
    return (int)finish(out, dout, SEARCH_ROWS * 64);
}

// ------------------------------------------------------------------------------------------ collision
// out[0][n]: collided<true> / OBS_OUTLINE, out[1][n]: collided<false> / OBS_OUTLINE, out[2][n]: OBS_CIRCLE
template <typename R>
__global__ __launch_bounds__(64) void k_collide(int n_obs, const R *obs, const R *shape, const R *poses, int n, int *out) {
    KParams<R> P = {};
    P.n_obs = n_obs;
    P.obs = obs;
    for (int q = 0; q < 9; ++q) { P.shape_x[q] = shape[q]; P.shape_y[q] = shape[9 + q]; }
    P.obstacle_model = OBS_OUTLINE;
    const int lane = threadIdx.x;
    const ObsLanes<R> tab = load_obstacles(P, lane);
    for (int i = lane; i < n; i += 64) {  // n is a multiple of 64: every lane stays active
        const R x = poses[3 * i], y = poses[3 * i + 1], yaw = poses[3 * i + 2];
        P.obstacle_model = OBS_OUTLINE;
        out[i] = collided<true>(P, x, y, yaw, tab) ? 1 : 0;
        out[n + i] = collided<false>(P, x, y, yaw, tab) ? 1 : 0;
        P.obstacle_model = OBS_CIRCLE;
        out[2 * n + i] = collided<false>(P, x, y, yaw, tab) ? 1 : 0;
    }
}

template <typename R> int run_collide(int n_obs, const R *obs, const R *shape, const R *poses, int n, int *out) {
    if (n_obs < 1 || n_obs > 4096 || n < 64 || n % 64 || n > (1 << 20)) return (int)hipErrorInvalidValue;
    Scope sc;
    R *dobs, *dshape, *dposes;
    int *dout;
    CK(sc.in(dobs, obs, (size_t)n_obs * 4));
    CK(sc.in(dshape, shape, 18));
    CK(sc.in(dposes, poses, (size_t)n * 3));
    CK(sc.out(dout, (size_t)n * 3));
    k_collide<R><<<1, 64>>>(n_obs, dobs, dshape, dposes, n, dout);
    return (int)finish(out, dout, (size_t)n * 3);
}

// ------------------------------------------------------------------------------------------ sampler
__global__ __launch_bounds__(256) void k_philox(const unsigned *ctr, const unsigned *key, unsigned *out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned r[4];
    px::philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], r);
    for (int q = 0; q < 4; ++q) out[4 * i + q] = r[q];
}

__global__ __launch_bounds__(256) void k_uniform_open(const unsigned *r, float *out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = px::uniform_open(r[i]);
}

struct Chol { float v[3]; };

__global__ __launch_bounds__(256) void k_box_muller(const unsigned *ra, const unsigned *rb, Chol ch, float *e, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    px::box_muller(ra[i], rb[i], ch.v, e[2 * i], e[2 * i + 1]);
}

__global__ __launch_bounds__(256) void k_sample(unsigned seed_lo, unsigned seed_hi, unsigned iter, const unsigned *k,
                                                const int *t, unsigned stream, Chol ch, float *e, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    px::sample(seed_lo, seed_hi, iter, k[i], t[i], ch.v, e[2 * i], e[2 * i + 1], stream);
}

constexpr int SAMPLER_MAX = 1 << 20;

// noise_pair against noise_at (one wave): lane l owns steps 2l and 2l+1 of sample k as in k_rollout_dual, idle when 2l >= T.
// out[l][8] = {noise_pair's four values, noise_at(2l), noise_at(2l+1) -- 0 beyond the horizon}; the pair's second step starts
// as NaN, so that a 0 there is the helper's
__global__ __launch_bounds__(64) void k_noise_pair(const KParams<float> P, int philox, unsigned iter, int agent, int k, float *out) {
    const int l = threadIdx.x;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (2 * l < P.T) {
        const bool a1 = 2 * l + 1 < P.T;
        v[2] = NAN;
        v[3] = NAN;
        noise_pair(P, philox != 0, iter, agent, k, l, a1, v[0], v[1], v[2], v[3]);
        noise_at(P, philox != 0, iter, agent, k, 2 * l, v[4], v[5]);
        if (a1) noise_at(P, philox != 0, iter, agent, k, 2 * l + 1, v[6], v[7]);
    }
    for (int q = 0; q < 8; ++q) out[8 * l + q] = v[q];
}

// ------------------------------------------------------------------------------------------ look-back pieces
// lb_scan: thread i owns positions NP i .. NP i + NP - 1 (one past n: idle, x = NaN); every block stages the 32 candidates in
// sh_c as the rollout kernels do (thread j writes its candidate into its pair).  m[n]; bad[n]: the lane's flag (NP = 2: the OR
// over its pair, stored at both positions)
template <int NP, typename R> __global__ __launch_bounds__(64) void k_lb_scan(const R *cand, const R *pos, int n, int *m_out, int *bad_out) {
    __shared__ RefPair<R> sh_c[LB_CAND / 2];
    if (threadIdx.x < LB_CAND) {
        const int j = threadIdx.x;
        R *pair = reinterpret_cast<R *>(&sh_c[j >> 1]);  // {x_2q, x_2q+1, y_2q, y_2q+1}
        pair[j & 1] = cand[2 * j];
        pair[2 + (j & 1)] = cand[2 * j + 1];
    }
    __syncthreads();
    const int first = NP * (blockIdx.x * 64 + threadIdx.x);
    R xs[NP], ys[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool have = first + i < n;
        xs[i] = have ? pos[2 * (first + i)] : R(NAN);
        ys[i] = have ? pos[2 * (first + i) + 1] : R(0);
    }
    int m[NP];
    bool bad;
    lb_scan<NP, R>(sh_c, xs, ys, m, bad);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (first + i < n) {
            m_out[first + i] = m[i];
            bad_out[first + i] = bad ? 1 : 0;
        }
    }
}

template <typename R> int run_lb_scan(int np, const R *cand, const R *pos, int n, int *m, int *bad) {
    if ((np != 1 && np != 2) || n < 1 || n > (1 << 20) || n % np) return (int)hipErrorInvalidValue;
    Scope sc;
    R *dc, *dp;
    int *dm, *db;
    CK(sc.in(dc, cand, (size_t)LB_CAND * 2));
    CK(sc.in(dp, pos, (size_t)n * 2));
    CK(sc.out(dm, n));
    CK(sc.out(db, n));
    const int blocks = (n / np + 63) / 64;
    if (np == 1) k_lb_scan<1, R><<<blocks, 64>>>(dc, dp, n, dm, db);
    else k_lb_scan<2, R><<<blocks, 64>>>(dc, dp, n, dm, db);
    CK(finish(m, dm, n));
    return (int)hipMemcpy(bad, db, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
}

__global__ __launch_bounds__(256) void k_lb_reach(const int *tab, int n, int *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = lb_reach(tab[4 * i], tab[4 * i + 1], tab[4 * i + 2], tab[4 * i + 3]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_lb_tag(const unsigned *seq, int n, unsigned *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = lb_tag(seq[i]);
}

// Workgroup b (one wave) publishes word[b] unless skip[b], then waits for the words of [0, b) under `tag` for at most `limit`
// ticks: out[b] = {ok, E, bad, every lane returned the same}.  Every wait ends by its own clock (lb_wait).
__global__ __launch_bounds__(64) void k_lb_exchange(unsigned *slots, const unsigned *word, const int *skip, unsigned tag, int limit,
                                                    int *out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!skip[b]) lb_publish(slots, b, word[b], lane);
    int E = -1;
    bool bad = true;
    const bool ok = lb_wait(slots, b, tag, lane, E, bad, limit);
    const int mine = (ok ? 1 : 0) | (bad ? 2 : 0) | (E << 2);
    const int same = __all(mine == wv::read_lane(mine, 0));
    if (lane == 0) {
        out[4 * b] = ok ? 1 : 0;
        out[4 * b + 1] = E;
        out[4 * b + 2] = bad ? 1 : 0;
        out[4 * b + 3] = same;
    }
}

constexpr int LB_SLOT_WORDS = LB_COPIES * LB_COPY_STRIDE;
constexpr int LB_LIMIT_MAX = 1000000;  // 10 ms at 100 MHz: what a launch of this harness may wait at the most

// ------------------------------------------------------------------------------------------ mppi_merge.h
// merge_combine<A, 256, NWIN> as k_merge / k_finalize call it: every load first, then the merge.  out = {rho, eta, eta2, n_hit,
// w_eps[2T]}; want_hits 0 leaves the count out (n_hit stays -1)
template <typename A, int NWIN>
__global__ __launch_bounds__(MERGE_THREADS) void k_harness_combine(const A *__restrict__ recs, const A *__restrict__ heads, int n,
                                                                   int T, A beta, int want_hits, A *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MergeLds<A> L(smem, T, 0);
    MergeRegs<A, MERGE_THREADS, NWIN> mr;
    merge_load_heads<A, MERGE_THREADS, NWIN>(heads, mr);
    merge_load_tile<A, MERGE_THREADS, NWIN>(recs, T, 0, mr);
    A rho, eta, eta2, n_hit = want_hits ? A(0) : A(-1);
    merge_combine<A, MERGE_THREADS, NWIN>(recs, n, T, beta, mr, L.s, L.part, rho, eta, eta2, [&](int i, A v) { out[4 + i] = v; },
                                          &n_hit);
    if (threadIdx.x == 0) { out[0] = rho; out[1] = eta; out[2] = eta2; out[3] = n_hit; }
}

// merge_abi<A> over n records {rho, eta, eta2, W[2T]} in doubles.  out = {rho, eta, eta2, w_eps[2T]}
template <typename A>
__global__ __launch_bounds__(MERGE_THREADS) void k_harness_abi(const double *__restrict__ recs, int n, int T, A beta,
                                                               A *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MergeLds<A> L(smem, T, 0);
    A rho, eta, eta2;
    merge_abi<A>(recs, n, T, beta, L.s, L.red, rho, eta, eta2, [&](int i, A v) { out[3 + i] = v; });
    if (threadIdx.x == 0) { out[0] = rho; out[1] = eta; out[2] = eta2; }
}

constexpr int MERGE_T_MAX = 512;  // (merge_lds_elems(512, 0, 8) doubles: 22 KiB of LDS)

// heads [slots][4], recs [slots][record_len(T)]: the first `slots` slots of buffers of nwin * 256 + 256 zero-filled slots -- what
// the product allocates whatever n is (merge_load_* read whole windows unconditionally); n <= slots: the slots past n are the
// caller's "absent" ones
template <typename A> int run_merge_combine(int nwin, const A *heads, const A *recs, int slots, int n, int T, A beta, int want_hits, A *out) {
    const int cap = nwin * MERGE_MAX_RECORDS + MERGE_MAX_RECORDS;
    if (nwin < 1 || nwin > MERGE_MAX_WINDOWS || n < 1 || n > nwin * MERGE_MAX_RECORDS || slots < n || slots > cap || T < 1 ||
        T > MERGE_T_MAX)
        return (int)hipErrorInvalidValue;
    const size_t rl = (size_t)record_len(T, (int)sizeof(A));
    Scope sc;
    A *dh, *dr, *dout;
    CK(sc.alloc((void **)&dh, (size_t)cap * 4 * sizeof(A)));
    CK(sc.alloc((void **)&dr, (size_t)cap * rl * sizeof(A)));
    CK(hipMemset(dh, 0, (size_t)cap * 4 * sizeof(A)));
    CK(hipMemset(dr, 0, (size_t)cap * rl * sizeof(A)));
    CK(hipMemcpy(dh, heads, (size_t)slots * 4 * sizeof(A), hipMemcpyHostToDevice));
    CK(hipMemcpy(dr, recs, (size_t)slots * rl * sizeof(A), hipMemcpyHostToDevice));
    CK(sc.out(dout, (size_t)4 + 2 * T));
    const size_t lds = sizeof(A) * merge_lds_elems(T, 0, sizeof(A));
    if (nwin == 1) k_harness_combine<A, 1><<<1, MERGE_THREADS, lds>>>(dr, dh, n, T, beta, want_hits, dout);
    else k_harness_combine<A, 2><<<1, MERGE_THREADS, lds>>>(dr, dh, n, T, beta, want_hits, dout);
    return (int)finish(out, dout, (size_t)4 + 2 * T);
}

template <typename A> int run_merge_abi(const double *recs, int n, int T, A beta, A *out) {
    if (n < 1 || n > MERGE_MAX_RECORDS || T < 1 || T > MERGE_T_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    double *dr;
    A *dout;
    CK(sc.in(dr, recs, (size_t)n * partial_len(T)));
    CK(sc.out(dout, (size_t)3 + 2 * T));
    k_harness_abi<A><<<1, MERGE_THREADS, sizeof(A) * merge_lds_elems(T, 0, sizeof(A))>>>(dr, n, T, beta, dout);
    return (int)finish(out, dout, (size_t)3 + 2 * T);
}

}  // namespace

extern "C" {

int prims_sincos_f32(const float *x, float *s, float *c, int n) { return run_map<float>(M_SINCOS, x, 0.f, s, c, n); }
int prims_tan_f32(const float *x, float *y, int n) { return run_map<float>(M_TAN, x, 0.f, y, nullptr, n); }
int prims_pymod_f32(const float *a, float m, float *r, int n) { return run_map<float>(M_PYMOD, a, m, r, nullptr, n); }
int prims_exp_f32(const float *x, float *y, int n) { return run_map<float>(M_EXP, x, 0.f, y, nullptr, n); }
int prims_clamp_f32(const float *v, float lim, float *r, int n) { return run_map<float>(M_CLAMP, v, lim, r, nullptr, n); }
int prims_clamp_f64(const double *v, double lim, double *r, int n) { return run_map<double>(M_CLAMP, v, lim, r, nullptr, n); }

int prims_scan_f32(int op, int variant, const float *in, float *out) { return run_scan(op, variant, in, out); }
int prims_scan_f64(int op, int variant, const double *in, double *out) { return run_scan(op, variant, in, out); }
int prims_scan_i32(int op, int variant, const int *in, int *out) { return run_scan(op, variant, in, out); }
int prims_shift_f32(int variant, const float *in, float carry, float *out) { return run_shift(variant, in, carry, out); }
int prims_shift_f64(int variant, const double *in, double carry, double *out) { return run_shift(variant, in, carry, out); }
int prims_read_lane_f32(const float *in, float *out) { return run_read_lane(in, out); }
int prims_read_lane_f64(const double *in, double *out) { return run_read_lane(in, out); }
int prims_shfl_xor_f32(int m, const float *in, float *out) { return run_shfl_xor(m, in, out); }
int prims_shfl_xor_f64(int m, const double *in, double *out) { return run_shfl_xor(m, in, out); }
int prims_argmin_f32(const float *d, const int *j, float *d_out, int *j_out) { return run_argmin(d, j, d_out, j_out); }
int prims_argmin_f64(const double *d, const int *j, double *d_out, int *j_out) { return run_argmin(d, j, d_out, j_out); }
int prims_ordered_sum_f32(float acc, const float *v, int first, int n, float *out) { return run_ordered_sum(acc, v, first, n, out); }
int prims_ordered_sum_f64(double acc, const double *v, int first, int n, double *out) { return run_ordered_sum(acc, v, first, n, out); }

int prims_search_rows(void) { return SEARCH_ROWS; }
int prims_search_f32(const float *ref, int n_ref, int c, int wlen, const float *qx, const float *qy, int *out) {
    return run_search(ref, n_ref, c, wlen, qx, qy, out);
}
int prims_search_f64(const double *ref, int n_ref, int c, int wlen, const double *qx, const double *qy, int *out) {
    return run_search(ref, n_ref, c, wlen, qx, qy, out);
}

// shape: shape_x[9] then shape_y[9]; poses [n][3] {x, y, yaw}; out [3][n]
int prims_collide_f32(int n_obs, const float *obs, const float *shape, const float *poses, int n, int *out) {
    return run_collide(n_obs, obs, shape, poses, n, out);
}
int prims_collide_f64(int n_obs, const double *obs, const double *shape, const double *poses, int n, int *out) {
    return run_collide(n_obs, obs, shape, poses, n, out);
}

int prims_philox(const unsigned *ctr, const unsigned *key, unsigned *out, int n) {
    if (n < 0 || n > SAMPLER_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *dc, *dk, *dout;
    CK(sc.in(dc, ctr, (size_t)n * 4));
    CK(sc.in(dk, key, (size_t)n * 2));
    CK(sc.out(dout, (size_t)n * 4));
    if (n) k_philox<<<(n + 255) / 256, 256>>>(dc, dk, dout, n);
    return (int)finish(out, dout, (size_t)n * 4);
}

int prims_uniform_open(const unsigned *r, float *out, int n) {
    if (n < 0 || n > SAMPLER_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *dr;
    float *dout;
    CK(sc.in(dr, r, n));
    CK(sc.out(dout, n));
    if (n) k_uniform_open<<<(n + 255) / 256, 256>>>(dr, dout, n);
    return (int)finish(out, dout, n);
}

int prims_box_muller(const unsigned *ra, const unsigned *rb, const float *chol, float *e, int n) {
    if (n < 0 || n > SAMPLER_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *da, *db;
    float *dout;
    CK(sc.in(da, ra, n));
    CK(sc.in(db, rb, n));
    CK(sc.out(dout, (size_t)n * 2));
    const Chol ch = {{chol[0], chol[1], chol[2]}};
    if (n) k_box_muller<<<(n + 255) / 256, 256>>>(da, db, ch, dout, n);
    return (int)finish(e, dout, (size_t)n * 2);
}

int prims_sample(unsigned seed_lo, unsigned seed_hi, unsigned iter, const unsigned *k, const int *t, unsigned stream,
                 const float *chol, float *e, int n) {
    if (n < 0 || n > SAMPLER_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *dk;
    int *dt;
    float *dout;
    CK(sc.in(dk, k, n));
    CK(sc.in(dt, t, n));
    CK(sc.out(dout, (size_t)n * 2));
    const Chol ch = {{chol[0], chol[1], chol[2]}};
    if (n) k_sample<<<(n + 255) / 256, 256>>>(seed_lo, seed_hi, iter, dk, dt, stream, ch, dout, n);
    return (int)finish(e, dout, (size_t)n * 2);
}

// row [T][2]: sample k's row of agent `agent`'s noise tensor [K = k + 1][T][2] (the tensor branch reads nothing else, so
// only the row exists: P.eps points where the whole tensor would start); out [64][8], see k_noise_pair
int prims_noise_pair(int philox, unsigned seed_lo, unsigned seed_hi, unsigned iter, int T, int k_offset, int noise_stream,
                     int agent, int k, const float *chol, const float *row, float *out) {
    if (T < 1 || T > 128 || k < 0 || agent < 0 || agent > 7) return (int)hipErrorInvalidValue;
    Scope sc;
    float *drow, *dout;
    CK(sc.in(drow, row, (size_t)T * 2));
    CK(sc.out(dout, 64 * 8));
    KParams<float> P{};
    P.K = k + 1; P.T = T; P.k_offset = k_offset; P.noise_stream = noise_stream;
    P.seed_lo = seed_lo; P.seed_hi = seed_hi; P.n_agents = 8; P.eps_slots = 0;
    for (int q = 0; q < 3; ++q) P.chol[q] = chol[q];
    const size_t before = (((size_t)agent * P.K + (size_t)k) * T) * 2 * sizeof(float);  // bytes of the tensors before the row
    P.eps = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(drow) - before);
    k_noise_pair<<<1, 64>>>(P, philox, iter, agent, k, dout);
    return (int)finish(out, dout, 64 * 8);
}

// candidates [32][2], positions [n][2] (n a multiple of np, np 1 or 2: positions per lane) -> m[n], bad[n]
int prims_lb_scan_f32(int np, const float *cand, const float *pos, int n, int *m, int *bad) { return run_lb_scan(np, cand, pos, n, m, bad); }
int prims_lb_scan_f64(int np, const double *cand, const double *pos, int n, int *m, int *bad) { return run_lb_scan(np, cand, pos, n, m, bad); }

// tab [n][4] = {leave, window, n_ref, c} -> out[n] = 0 / 1
int prims_lb_reach(const int *tab, int n, int *out) {
    if (n < 1 || n > (1 << 20)) return (int)hipErrorInvalidValue;
    Scope sc;
    int *dt, *dout;
    CK(sc.in(dt, tab, (size_t)n * 4));
    CK(sc.out(dout, n));
    k_lb_reach<<<(n + 255) / 256, 256>>>(dt, n, dout);
    return (int)finish(out, dout, n);
}

int prims_lb_tag(const unsigned *seq, int n, unsigned *out) {
    if (n < 1 || n > (1 << 20)) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *ds, *dout;
    CK(sc.in(ds, seq, n));
    CK(sc.out(dout, n));
    k_lb_tag<<<(n + 255) / 256, 256>>>(ds, n, dout);
    return (int)finish(out, dout, n);
}

int prims_lb_slot_words(void) { return LB_SLOT_WORDS; }
int prims_lb_default_limit(void) { return (int)LB_TIMEOUT_TICKS; }
// word[B], skip[B]; slots [LB_COPIES * LB_COPY_STRIDE]: what the buffer holds before the launch, returned whole after it;
// out [B][4] = {ok, E, bad, lanes agree}
int prims_lb_exchange(int B, const unsigned *word, const int *skip, unsigned tag, int limit, unsigned *slots, int *out) {
    if (B < 1 || B > HYP_MAX_BLOCKS || limit < 0 || limit > LB_LIMIT_MAX) return (int)hipErrorInvalidValue;
    Scope sc;
    unsigned *dw, *dslots;
    int *dskip, *dout;
    CK(sc.in(dw, word, B));
    CK(sc.in(dskip, skip, B));
    CK(sc.in(dslots, slots, LB_SLOT_WORDS));
    CK(sc.out(dout, (size_t)B * 4));
    k_lb_exchange<<<B, 64>>>(dslots, dw, dskip, tag, limit, dout);
    CK(finish(out, dout, (size_t)B * 4));
    return (int)hipMemcpy(slots, dslots, (size_t)LB_SLOT_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost);
}

int prims_merge_record_len_f32(int T) { return record_len(T, 4); }
int prims_merge_record_len_f64(int T) { return record_len(T, 8); }
int prims_merge_combine_f32(int nwin, const float *heads, const float *recs, int slots, int n, int T, float beta, int want_hits,
                            float *out) {
    return run_merge_combine(nwin, heads, recs, slots, n, T, beta, want_hits, out);
}
int prims_merge_combine_f64(int nwin, const double *heads, const double *recs, int slots, int n, int T, double beta, int want_hits,
                            double *out) {
    return run_merge_combine(nwin, heads, recs, slots, n, T, beta, want_hits, out);
}
int prims_merge_abi_f32(const double *recs, int n, int T, float beta, float *out) { return run_merge_abi(recs, n, T, beta, out); }
int prims_merge_abi_f64(const double *recs, int n, int T, double beta, double *out) { return run_merge_abi(recs, n, T, beta, out); }

}  // extern "C"
