// The serial tail's device code, shared by k_merge / k_finalize / k_eval_filter (mppi_kernels.hip) and the test harness
// (tests/device/prims_harness.hip): the rescale merge of softmin records in the internal layout (merge_load_*, merge_combine)
// and in the ABI layout (merge_abi), the moving average (filter_store / filter_at) and the block reductions.
//
// Contract of the record buffers: n records in slots 0 .. n-1; merge_load_* read whole windows of MERGE_MAX_RECORDS slots
// (heads and W) unconditionally, so the buffers hold windows * 256 + 256 slots whatever n is.  A slot >= n ("absent") enters
// with a zero scale: whatever FINITE values it holds leave the result unchanged bit for bit.  Non-finite values there
// (0 x NaN) are outside the contract -- the product zero-fills the buffers at creation and no producer writes past n.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mppi_device.h"

#ifndef STAMP  // (phase stamps of the diagnostic build, defined by mppi_kernels.hip before this header)
#define STAMP(n) \
    do {         \
    } while (0)
#endif

namespace mppi {

// Block records (written by k_rollout_fused / k_reduce / k_merge) use the INTERNAL layout
// {rho, eta, eta2, pad, W[2T] padded to a 16-byte multiple}, so W is read as aligned 16-byte vectors;
// the per-rank record of the split step uses the ABI layout {rho, eta, eta2, W[2T]} in doubles.
// ------------------------------------------------------------------------------------------
// NT threads merge 256 records: thread = (16-byte column vc = tid % 32, group grp = tid / 32), NT/32 groups of
// 256/(NT/32) consecutive records.  NT = 256: the merge kernels' own launches; NT = 1024: the prologue of k_iter.
template <int NT> struct MergeShape {
    static constexpr int GROUPS = NT / 32, MAXJ = MERGE_MAX_RECORDS / GROUPS, WAVES = NT / 64;
};

template <typename A> struct alignas(16) VecT { A v[16 / sizeof(A)]; };

// LDS of the merge code.  w: the weighted noise in the filter's padded layout, [2 (T + W + 1)] (k_merge: W = 0,
// plain); u: the updated controls [2T]; s: 64 record scales per wave; red: block reductions; part: per-group
// partial sums.  Every region starts on a 16-byte boundary.
template <typename A, int NT = MERGE_THREADS> struct MergeLds {
    A *w, *u, *s, *red, *part;
    __device__ __forceinline__ MergeLds(char *smem, int T, int W) {
        w = reinterpret_cast<A *>(smem);
        u = w + ((2 * (T + W + 1) + 3) & ~3);
        s = u + ((2 * T + 3) & ~3);
        red = s + MERGE_MAX_WINDOWS * NT;
        part = red + 64;
    }
};

__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ double fast_exp(double x) { return exp(x); }
__device__ __forceinline__ float fast_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }  // 1 ulp
__device__ __forceinline__ double fast_div(double a, double b) { return a / b; }

// ---- the moving average of the weighted noise (`_moving_average_filter`), shared by k_finalize and k_eval_filter ----
// Sample t of channel d sits at sh_w[2 (t + H) + d], H = W / 2: H leading and W - H trailing slots hold zeros
// (np.convolve 'same', mppi_differential_drive.py:257-263) or copies of the first H / last W - H samples
// (mppi_race_car.py:211-222: the padded signal is xx[:W//2] + xx + xx[-W//2:], and -W//2 is -(H + 1) at an odd W)
template <typename A> __device__ __forceinline__ void filter_store(A *sh_w, int i, A v, int T, int W, bool pad_copy) {
    const int t = i >> 1, d = i & 1, H = W / 2;
    const A pv = pad_copy ? v : A(0);
    sh_w[2 * (t + H) + d] = v;
    if (t < H) sh_w[2 * t + d] = pv;
    if (t >= T - (W - H)) sh_w[2 * (t + W) + d] = pv;
}
// filtered sample t of channel d (window W): taps padded[t + W - 1 - q], q = 0 .. W-1, in that order
template <typename A> __device__ __forceinline__ A filter_at(const A *sh_w, int t, int d, int T, int W, int f_filter) {
    const int H = W / 2;
    const A inv_w = fast_div(A(1), (A)W);
    if (f_filter == FILTER_NONE) return sh_w[2 * (t + H) + d];
    if (f_filter == FILTER_TORCH) {
        // conv1d(padding = H) over the padded signal, first T outputs (mppi_race_car_torch.py:211-222):
        // output t = padded rows t-H .. t-H+W-1, rows before the start are the convolution's zero padding
        A sacc = 0;
        for (int q = 0; q < W; ++q) {
            const int m = t - H + q;
            if (m >= 0) sacc += sh_w[2 * m + d] * inv_w;
        }
        return sacc;
    }
    const A *tap = sh_w + 2 * t + d;
    A sacc = 0;
    if (W == 10) {  // every reference variant; static LDS offsets, reads issue back to back
#pragma unroll
        for (int q = 0; q < 10; ++q) sacc += tap[2 * (9 - q)] * inv_w;
    } else {
        for (int q = 0; q < W; ++q) sacc += tap[2 * (W - 1 - q)] * inv_w;
    }
    if (f_filter == FILTER_DIFF) {  // the edge factors of mppi_differential_drive.py:265-269
        const int n_conv = (W + 1) / 2;
        if (t == 0) sacc *= fast_div((A)W, (A)n_conv);
        else if (t < n_conv) sacc *= fast_div((A)W, (A)(t + n_conv));
        if (t == T - 1)
            for (int q = 1; q < n_conv; ++q) sacc *= fast_div((A)W, (A)(q + n_conv - (W % 2)));
    }
    return sacc;
}

template <typename A> struct BlockRed {  // block-wide reductions through one LDS exchange each (256 threads)
    static __device__ __forceinline__ A min1(A v, A *sh, int tid) {
        v = wv::reduce<wv::OpMin>(v);
        __syncthreads();
        if ((tid & 63) == 0) sh[tid >> 6] = v;
        __syncthreads();
        A r = sh[0];
#pragma unroll
        for (int w = 1; w < MERGE_THREADS / 64; ++w) r = fmin(r, sh[w]);
        return r;
    }
    static __device__ __forceinline__ void add2(A &a, A &b, A *sh, int tid) {
        a = wv::reduce<wv::OpAdd>(a);
        b = wv::reduce<wv::OpAdd>(b);
        __syncthreads();
        if ((tid & 63) == 0) { sh[tid >> 6] = a; sh[32 + (tid >> 6)] = b; }
        __syncthreads();
        a = 0;
        b = 0;
#pragma unroll
        for (int w = 0; w < MERGE_THREADS / 64; ++w) { a += sh[w]; b += sh[32 + w]; }
    }
};

// Merge n <= 256 NWIN records with the rescale trick: rho = min rho_b,
// s_b = exp(-beta (rho_b - rho)), eta = sum s_b eta_b, W = sum s_b W_b.  Records come from a PREVIOUS
// launch: ordinary loads are coherent.  Written for latency -- the caller issues every load first thing
// (merge_load_*), before it touches anything else, so that one memory round trip covers them all; the
// heads are reduced per wave (each wave reads all 256 heads, DPP reductions, no block barrier).
// Record b lives in slot b; slots >= n are never written by a producer and the buffers are zero-filled and
// padded by 256 records at creation, so every load is unconditional and in bounds, and an absent slot enters
// with a zero scale.
// NWIN windows of 256 records: the same thread mapping in every window, all windows' loads in flight at once.
template <typename A, int NT = MERGE_THREADS, int NWIN = 1> struct MergeRegs {
    VecT<A> w[NWIN][MergeShape<NT>::MAXJ];
    A hr[4 * NWIN], he[4 * NWIN], he2[4 * NWIN];  // heads of records 256 win + lane + {0, 64, 128, 192}
    A hc[4 * NWIN];                                // their fourth word: samples that carry a collision penalty
};

template <typename A, int NT, int NWIN>
__device__ __forceinline__ void merge_load_heads(const A *__restrict__ heads, MergeRegs<A, NT, NWIN> &m) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 4 * NWIN; ++i) {  // the compact copy: consecutive lanes read consecutive 16 / 32 bytes
        const int b = lane + 64 * i;
        const size_t r = (size_t)b;
        const VecT4<A> hd = *reinterpret_cast<const VecT4<A> *>(heads + 4 * r);
        m.hr[i] = hd.x;
        m.he[i] = hd.y;
        m.he2[i] = hd.z;
        m.hc[i] = hd.w;
    }
}

template <typename A, int NT, int NWIN>
__device__ __forceinline__ void merge_load_tile(const A *__restrict__ recs, int T, int vt, MergeRegs<A, NT, NWIN> &m) {
    constexpr int VW = 16 / sizeof(A), MAXJ = MergeShape<NT>::MAXJ;
    const int tid = threadIdx.x, vc = tid & 31, grp = tid >> 5;
    const unsigned rbytes = (unsigned)record_len(T, (int)sizeof(A)) * (unsigned)sizeof(A);
    const int nvc = (2 * T + VW - 1) / VW;  // 16-byte columns of W
    const char *base = reinterpret_cast<const char *>(recs);
    const unsigned col = (unsigned)(4 + min(vt * 32 + vc, nvc - 1) * VW) * (unsigned)sizeof(A);
    const unsigned off0 = (unsigned)(grp * MAXJ) * rbytes + col;
#pragma unroll
    for (int win = 0; win < NWIN; ++win)
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            m.w[win][j] = *reinterpret_cast<const VecT<A> *>(base + (off0 + (unsigned)(win * MERGE_MAX_RECORDS + j) * rbytes));
}

// `store(i, v)` receives w_eps[i] = W[i] / eta for i in [0, 2T); rho/eta/eta2 end up in every thread.
template <typename A, int NT, int NWIN, typename Store>
__device__ __forceinline__ void merge_combine(const A *__restrict__ recs, int n, int T, A beta,
                                              MergeRegs<A, NT, NWIN> &m, A *sh_s, A *sh_part, A &rho, A &eta, A &eta2,
                                              Store store, A *n_hit = nullptr) {
    constexpr int VW = 16 / sizeof(A), MAXJ = MergeShape<NT>::MAXJ, GROUPS = MergeShape<NT>::GROUPS;
    using V = VecT<A>;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int vc = tid & 31, grp = tid >> 5;
    const int nvc = (2 * T + VW - 1) / VW;
    A lr = A(INFINITY);
#pragma unroll
    for (int i = 0; i < 4 * NWIN; ++i) {
        if (lane + 64 * i >= n) m.hr[i] = A(INFINITY);
        lr = fmin(lr, m.hr[i]);
    }
    rho = wv::reduce<wv::OpMin>(lr);
    STAMP(25);
    A sc[4 * NWIN];
    eta = 0;
    eta2 = 0;
#pragma unroll
    for (int i = 0; i < 4 * NWIN; ++i) {
        sc[i] = lane + 64 * i < n ? fast_exp(-beta * (m.hr[i] - rho)) : A(0);
        eta += sc[i] * m.he[i];
        eta2 += sc[i] * sc[i] * m.he2[i];
    }
    eta = wv::reduce<wv::OpAdd>(eta);
    eta2 = wv::reduce<wv::OpAdd>(eta2);
    if (n_hit && *n_hit >= A(0)) {  // (the caller asks for the count by passing 0, and leaves it out with -1: no obstacles)
        A cnt = 0;
#pragma unroll
        for (int i = 0; i < 4 * NWIN; ++i) cnt += lane + 64 * i < n ? m.hc[i] : A(0);
        *n_hit = wv::reduce<wv::OpAdd>(cnt);
    }
    // this wave's two groups use the scales of records r0 .. r0 + 2 MAXJ - 1 only (a run inside one of the four
    // 64-record slots every lane holds): a wave-local exchange through 64 private LDS words, no block barrier
    // (per window)
    const int r0 = wid * 2 * MAXJ, slot = r0 >> 6;
    A *my_s = sh_s + wid * 64;  // window win at + win * NT
#pragma unroll
    for (int win = 0; win < NWIN; ++win)
        my_s[win * NT + lane] = slot == 0 ? sc[4 * win] : slot == 1 ? sc[4 * win + 1] : slot == 2 ? sc[4 * win + 2] : sc[4 * win + 3];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    STAMP(26);
    const A *sj_base = my_s + (r0 & 63) + (grp & 1) * MAXJ;
    const A inv_eta = fast_div(A(1), eta);
    const int n_tiles = (nvc + 31) / 32;
    for (int vt = 0; vt < n_tiles; ++vt) {
        V acc;
#pragma unroll
        for (int q = 0; q < VW; ++q) acc.v[q] = 0;
#pragma unroll
        for (int win = 0; win < NWIN; ++win)
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                const A sj = sj_base[win * NT + j];
#pragma unroll
                for (int q = 0; q < VW; ++q) acc.v[q] += sj * m.w[win][j].v[q];
            }
        if (vt > 0) __syncthreads();  // the previous tile's readers of sh_part are done
        *reinterpret_cast<V *>(sh_part + (grp * 32 + vc) * VW) = acc;
        __syncthreads();
        if (__builtin_expect(vt + 1 < n_tiles, 0)) merge_load_tile<A, NT, NWIN>(recs, T, vt + 1, m);  // T > 64 (f64: 32) only
        for (int e = tid; e < 32 * VW; e += NT) {
            const int i = vt * 32 * VW + e;
            if (i < 2 * T) {
                A t = 0;
#pragma unroll
                for (int g = 0; g < GROUPS; ++g) t += sh_part[g * 32 * VW + e];
                store(i, t * inv_eta);  // w_eps = W / eta, :132-135
            }
        }
    }
    __syncthreads();
}

// ABI layout (doubles, {rho, eta, eta2, W[2T]}), n = number of ranks: few records, plain loops.
template <typename A, typename Store>
__device__ __forceinline__ void merge_abi(const double *recs, int n, int T, A beta, A *sh_s, A *sh_red, A &rho, A &eta,
                                          A &eta2, Store store, int stride = 0) {
    const int tid = threadIdx.x, plen = stride ? stride : partial_len(T);
    A hr = A(INFINITY), he = 0, he2 = 0;
    if (tid < n) {
        const double *pb = recs + tid * plen;
        hr = (A)pb[0];
        he = (A)pb[1];
        he2 = (A)pb[2];
    }
    rho = BlockRed<A>::min1(hr, sh_red, tid);
    const A sc = tid < n ? fast_exp(-beta * (hr - rho)) : A(0);
    if (tid < n) sh_s[tid] = sc;
    eta = sc * he;
    eta2 = sc * sc * he2;
    BlockRed<A>::add2(eta, eta2, sh_red, tid);
    const A inv_eta = fast_div(A(1), eta);
    for (int i = tid; i < 2 * T; i += MERGE_THREADS) {
        A t = 0;
        for (int b = 0; b < n; ++b) t += sh_s[b] * (A)recs[b * plen + 3 + i];
        store(i, t * inv_eta);  // w_eps = W / eta, :132-135
    }
    __syncthreads();
}

}  // namespace mppi
