// `pytorch_mppi`-style MPPI with BUILT-IN dynamics / running-cost models: what the reference's
// test/test_mppi.py, test/test_mppi_diff.py, test/test_mppi_diff_dyna.py and train/bullet_mppi_differential_drive.py
// hand to `pytorch_mppi.MPPI` as Python callbacks, as selectable device functions, so that those callers need neither
// the library nor a callback per step.
//
//   dynamics      UNICYCLE     x' = x + v cos(th) dt, y' = y + v sin(th) dt, th' = th + w dt   (test/test_mppi.py:12-26)
//                 SKID_STEER   5 states [x, y, th, v, w], 4 wheel forces                       (test/test_mppi_diff_dyna.py:13-40)
//                 RACECAR      kinematic bicycle [x, y, th, v], u = [steer, accel]             (test/test_mppi_racecar.py:13-30)
//                 RACECAR_DYNAMIC  bicycle with tyre forces, u = [acc, steer]                  (test/test_torch_mppi_race_car.py:7-39)
//                 DOUBLE_INTEGRATOR  p' = p + dt v, v' = v + dt u                              (test/test_torch_mppi.py:5-15)
//   running cost  (s - goal)^T diag(Q) (s - goal) + u^T diag(R) u + obstacle_weight * sum_m o_m(d_m)
//                 INVERSE      o = 1 / (d + 1e-6) inside the safety distance, 0 outside         (test/test_mppi.py:40-50)
//                 EXPONENTIAL  o = exp(-(d - safety)), obstacles moving: p_m(t) = p_m + vel_m t  (test/test_mppi_diff.py:25-52)
//   terminal cost (s_T - goal)^T diag(q) (s_T - goal) on the state after the last step, once per sample (test/test_torch_mppi.py:23-25)
//   options       noise_mu, u_scale, noise_abs_cost of the library's constructor; each is behind a flag of its own, so that a
//                 handle that sets none of them runs the arithmetic it ran before they existed, bit for bit
//
// The loop around them is the published information-theoretic MPPI (Williams et al. 2017) the way `pytorch_mppi`
// arranges it: shift U, sample noise, clamp the perturbed action and recompute the noise from it, roll out, add
// lambda * U^T Sigma^-1 noise, softmin weights with rate 1/lambda, U += sum_k w_k noise_k, return U[0].
// `pytorch_mppi` itself is absent from the build container and un-pinned by the reference (no version anywhere): the
// loop is PARITY UNPINNED; tests check it against oracle/mppi_cb_oracle.py, a NumPy restatement of the same algorithm.
//
// Small problems (K ~ 1000, T ~ 25): one THREAD per sample, serial in t -- nothing here is tuned; the tuned path is
// mppi_kernels.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mppi_hip.h"
#include "mppi_owner.h"
#include "philox.h"

namespace {

constexpr int CB_NX = 5, CB_NU = 4, CB_OBS = 16;

struct CbParams {
    int K, T, nx, nu, dynamics, obstacle_kind, n_obs, sample_null_action;
    float dt, lambda_, safety, obstacle_weight;
    float goal[CB_NX], q[CB_NX], r[CB_NU], u_min[CB_NU], u_max[CB_NU];
    float sinv[CB_NU * CB_NU], chol[CB_NU * CB_NU];  // Sigma^-1 and the lower Cholesky factor of Sigma (row-major)
    float obs[CB_OBS][4];                            // x, y, vx, vy
    float skid[5];                                   // m, I, r, L, damping (test/test_mppi_diff_dyna.py:15-19, 29-30)
    unsigned seed_lo, seed_hi;
    float model[8];                                  // RACECAR: L; RACECAR_DYNAMIC: l_r, l_f, m, C_f, C_r
    int terminal, has_mu, scaled, abs_cost;          // the flags of the terms below: 0 leaves the term out of the arithmetic
    float tgoal[CB_NX], tq[CB_NX], mu[CB_NU], u_scale;
};

__device__ __forceinline__ void cb_dynamics(const CbParams &P, float *s, const float *u) {
    if (P.dynamics == MPPI_CB_DYN_UNICYCLE) {  // test/test_mppi.py:12-26
        const float th = s[2];
        s[0] += u[0] * cosf(th) * P.dt;
        s[1] += u[0] * sinf(th) * P.dt;
        s[2] += u[1] * P.dt;
    } else if (P.dynamics == MPPI_CB_DYN_RACECAR) {  // test/test_mppi_racecar.py:13-30: u = [steer, accel]
        const float th = s[2], v = s[3];
        s[0] += v * cosf(th) * P.dt;
        s[1] += v * sinf(th) * P.dt;
        s[2] += v / P.model[0] * tanf(u[0]) * P.dt;
        s[3] += u[1] * P.dt;
    } else if (P.dynamics == MPPI_CB_DYN_RACECAR_DYNAMIC) {  // test/test_torch_mppi_race_car.py:7-39: u = [acc, steer]
        const float lr = P.model[0], lf = P.model[1], m = P.model[2], Cf = P.model[3], Cr = P.model[4];
        const float th = s[2], v = s[3], sd = sinf(u[1]), cd = cosf(u[1]);
        // the script's slip angles: the yaw stands where a yaw rate would be expected (:25-26), restated as it is
        const float af = atan2f(v * sd + lf * th, v * cd) - u[1];
        const float ar = atan2f(v * sd - lr * th, v * cd);
        s[0] += v * cosf(th) * P.dt;
        s[1] += v * sinf(th) * P.dt;
        s[2] += (v / lr) * sd * P.dt;
        s[3] += (u[0] - (Cf * af * sd + Cr * ar) / m) * P.dt;
    } else if (P.dynamics == MPPI_CB_DYN_DOUBLE_INTEGRATOR) {  // test/test_torch_mppi.py:5-15: A = [[1, dt], [0, 1]], B = [0, dt]
        const float v = s[1];
        s[0] += P.dt * v;
        s[1] += P.dt * u[0];
    } else {  // test/test_mppi_diff_dyna.py:13-40: F_fr, F_fl, F_rr, F_rl
        const float m = P.skid[0], I = P.skid[1], r = P.skid[2], L = P.skid[3], damp = P.skid[4];
        const float th = s[2], v = s[3], om = s[4];
        const float dv = (r / (4.f * m)) * (u[0] + u[1] + u[2] + u[3]) - damp * v;
        const float dom = (r / (L * I)) * ((u[0] + u[2]) - (u[1] + u[3])) / 2.f - damp * om;
        s[0] += v * cosf(th) * P.dt;
        s[1] += v * sinf(th) * P.dt;
        s[2] += om * P.dt;
        s[3] += dv * P.dt;
        s[4] += dom * P.dt;
    }
}

__device__ __forceinline__ float cb_running_cost(const CbParams &P, const float *s, const float *u, int t) {
    float c = 0.f;
    for (int i = 0; i < P.nx; ++i) {
        const float e = s[i] - P.goal[i];
        c += P.q[i] * e * e;
    }
    for (int i = 0; i < P.nu; ++i) c += P.r[i] * u[i] * u[i];
    float oc = 0.f;
    for (int m = 0; m < P.n_obs; ++m) {
        const float ox = P.obs[m][0] + P.obs[m][2] * (float)t, oy = P.obs[m][1] + P.obs[m][3] * (float)t;
        const float d = sqrtf((s[0] - ox) * (s[0] - ox) + (s[1] - oy) * (s[1] - oy));
        if (P.obstacle_kind == MPPI_CB_OBS_INVERSE) oc += d < P.safety ? 1.f / (d + 1e-6f) : 0.f;  // test_mppi.py:46-48
        else oc += expf(-(d - P.safety));                                                          // test_mppi_diff.py:42-44
    }
    return c + P.obstacle_weight * oc;
}

__device__ __forceinline__ float cb_terminal_cost(const CbParams &P, const float *s) {
    float c = 0.f;
    for (int i = 0; i < P.nx; ++i) {
        const float e = s[i] - P.tgoal[i];
        c += P.tq[i] * e * e;
    }
    return c;
}

// noise[k, t, :] ~ N(mu, Sigma): injected tensor, or Philox4x32-10 keyed by (k, t, iteration) -> two Box-Muller pairs
__device__ __forceinline__ void cb_noise(const CbParams &P, const float *eps, unsigned iter, int k, int t, float *n) {
    if (eps) {
        for (int i = 0; i < P.nu; ++i) n[i] = eps[((size_t)k * P.T + t) * P.nu + i];
        return;
    }
    unsigned r[4];
    px::philox4x32_10((unsigned)k, (unsigned)t, iter, 0x6362u, P.seed_lo, P.seed_hi, r);
    const float id[3] = {1.f, 0.f, 1.f};
    float z[4];
    px::box_muller(r[0], r[1], id, z[0], z[1]);
    px::box_muller(r[2], r[3], id, z[2], z[3]);
    for (int i = 0; i < P.nu; ++i) {
        float a = 0.f;
        for (int j = 0; j <= i; ++j) a += P.chol[i * CB_NU + j] * z[j];
        n[i] = P.has_mu ? P.mu[i] + a : a;
    }
}

// the action sample k applies at step t and the noise that stands for it after clamping
__device__ __forceinline__ void cb_action(const CbParams &P, const float *U, const float *eps, unsigned iter, int k, int t,
                                          float *act, float *noise) {
    float n[CB_NU];
    cb_noise(P, eps, iter, k, t, n);
    for (int i = 0; i < P.nu; ++i) {
        float a = U[t * P.nu + i] + n[i];
        if (P.sample_null_action && k == P.K - 1) a = 0.f;
        a = fminf(fmaxf(a, P.u_min[i]), P.u_max[i]);
        act[i] = a;
        noise[i] = a - U[t * P.nu + i];
    }
}

// u_scale: dynamics and running cost see u_scale * the clamped action; bounds, perturbation term and update do not
__device__ __forceinline__ void cb_scale(const CbParams &P, float *act) {
    if (P.scaled)
        for (int i = 0; i < P.nu; ++i) act[i] *= P.u_scale;
}

__global__ void k_cb_rollout(const CbParams P, const float *__restrict__ U, const float *__restrict__ state,
                             const float *__restrict__ eps, unsigned iter, float *__restrict__ cost_total) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.K) return;
    float s[CB_NX];
    for (int i = 0; i < P.nx; ++i) s[i] = state[i];
    float cost = 0.f, pert = 0.f;
    for (int t = 0; t < P.T; ++t) {
        float act[CB_NU], noise[CB_NU];
        cb_action(P, U, eps, iter, k, t, act, noise);
        if (P.abs_cost)  // noise_abs_cost: |noise| after clamping in the perturbation term; the update keeps the sign
            for (int i = 0; i < P.nu; ++i) noise[i] = fabsf(noise[i]);
        cb_scale(P, act);
        cb_dynamics(P, s, act);
        cost += cb_running_cost(P, s, act, t);
        for (int i = 0; i < P.nu; ++i) {  // lambda * U^T Sigma^-1 noise
            float a = 0.f;
            for (int j = 0; j < P.nu; ++j) a += noise[j] * P.sinv[j * CB_NU + i];
            pert += U[t * P.nu + i] * P.lambda_ * a;
        }
    }
    if (P.terminal) cost += cb_terminal_cost(P, s);  // s is the state after the last step
    cost_total[k] = cost + pert;
}

// the clamped, unscaled actions of the last command: one thread per (k, t)
__global__ void k_cb_perturbed(const CbParams P, const float *__restrict__ U, const float *__restrict__ eps, unsigned iter,
                               float *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.K * P.T) return;
    float act[CB_NU], noise[CB_NU];
    cb_action(P, U, eps, iter, e / P.T, e % P.T, act, noise);
    for (int i = 0; i < P.nu; ++i) out[(size_t)e * P.nu + i] = act[i];
}

// c_j sorts before c_k: a NaN is larger than every number, equal costs (and NaNs among themselves) go by index
__device__ __forceinline__ bool cb_before(float cj, int j, float ck, int k) {
    const bool jn = cj != cj, kn = ck != ck;
    if (jn || kn) return jn && kn ? j < k : kn;
    return cj < ck || (cj == ck && j < k);
}

// The n cheapest samples of the last command and their trajectories from `state`: one thread per sample; the costs pass
// through LDS in tiles of a workgroup while every thread counts the samples that sort before its own.  The ranks are a
// permutation of 0 .. K - 1 whatever the costs hold, so a thread with rank < n owns row `rank` of both outputs.
__global__ __launch_bounds__(256) void k_cb_top(const CbParams P, const float *__restrict__ U, const float *__restrict__ state,
                                                const float *__restrict__ eps, unsigned iter,
                                                const float *__restrict__ cost_total, int n, float *__restrict__ traj,
                                                int *__restrict__ index_out) {
    __shared__ float sh[256];
    const int k = blockIdx.x * 256 + threadIdx.x;
    const float ck = k < P.K ? cost_total[k] : 0.f;
    int rank = 0;
    for (int base = 0; base < P.K; base += 256) {  // (every thread of the workgroup takes every barrier)
        const int j0 = base + threadIdx.x;
        sh[threadIdx.x] = j0 < P.K ? cost_total[j0] : 0.f;
        __syncthreads();
        const int m = min(256, P.K - base);
        if (k < P.K)
            for (int j = 0; j < m; ++j) rank += cb_before(sh[j], base + j, ck, k) ? 1 : 0;
        __syncthreads();
    }
    if (k >= P.K || rank >= n) return;
    index_out[rank] = k;
    float s[CB_NX];
    for (int i = 0; i < P.nx; ++i) s[i] = state[i];
    for (int t = 0; t < P.T; ++t) {
        float act[CB_NU], noise[CB_NU];
        cb_action(P, U, eps, iter, k, t, act, noise);
        cb_scale(P, act);
        cb_dynamics(P, s, act);
        for (int i = 0; i < P.nx; ++i) traj[((size_t)rank * P.T + t) * P.nx + i] = s[i];
    }
}

// softmin weights with rate 1/lambda, U += sum_k w_k noise_k; one workgroup
__global__ __launch_bounds__(256) void k_cb_update(const CbParams P, float *__restrict__ U, const float *__restrict__ eps,
                                                   unsigned iter, const float *__restrict__ cost_total,
                                                   float *__restrict__ omega, float *__restrict__ action_out,
                                                   float *__restrict__ U_drawn) {
    __shared__ float sh[256];
    __shared__ float sh_unew[256];
    const int tid = threadIdx.x;
    float m = INFINITY;
    for (int k = tid; k < P.K; k += 256) m = fminf(m, cost_total[k]);
    sh[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = fminf(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    const float beta = sh[0];
    __syncthreads();
    float a = 0.f;
    for (int k = tid; k < P.K; k += 256) a += expf(-(cost_total[k] - beta) / P.lambda_);
    sh[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const float eta = sh[0];
    for (int k = tid; k < P.K; k += 256) omega[k] = expf(-(cost_total[k] - beta) / P.lambda_) / eta;
    __syncthreads();
    for (int e = tid; e < P.T * P.nu; e += 256) {  // (T * nu <= 256, checked at create)
        const int t = e / P.nu, i = e % P.nu;
        float acc = 0.f;
        for (int k = 0; k < P.K; ++k) {
            float act[CB_NU], noise[CB_NU];
            cb_action(P, U, eps, iter, k, t, act, noise);
            acc += omega[k] * noise[i];
        }
        sh_unew[e] = U[e] + acc;
        U_drawn[e] = U[e];  // the sequence this command's samples were drawn around (mppi_cb_get_perturbed_actions)
    }
    __syncthreads();
    for (int e = tid; e < P.T * P.nu; e += 256) U[e] = sh_unew[e];
    if (tid < P.nu) action_out[tid] = sh_unew[tid];
}

__global__ void k_cb_shift(const CbParams P, float *__restrict__ U, const float *__restrict__ u_init) {  // roll(-1), last = u_init
    __shared__ float sh[256];
    const int n = P.T * P.nu, e = threadIdx.x;
    if (e < n) sh[e] = e + P.nu < n ? U[e + P.nu] : u_init[e - (n - P.nu)];
    __syncthreads();
    if (e < n) U[e] = sh[e];
}

__global__ void k_cb_eval(const CbParams P, int what, const float *__restrict__ s_in, const float *__restrict__ u_in, int t,
                          int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s[CB_NX], u[CB_NU];
    for (int q = 0; q < P.nx; ++q) s[q] = s_in[(size_t)i * P.nx + q];
    for (int q = 0; q < P.nu; ++q) u[q] = what == 2 ? 0.f : u_in[(size_t)i * P.nu + q];
    if (what == 2) {
        out[i] = cb_terminal_cost(P, s);
    } else if (what == 0) {
        cb_dynamics(P, s, u);
        for (int q = 0; q < P.nx; ++q) out[(size_t)i * P.nx + q] = s[q];
    } else {
        out[i] = cb_running_cost(P, s, u, t);
    }
}

// the trajectory the nominal sequence U drives from `state` (what the reference's get_trajectories rolls out)
__global__ void k_cb_nominal(const CbParams P, const float *__restrict__ U, const float *__restrict__ state, float *__restrict__ traj) {
    if (threadIdx.x != 0) return;
    float s[CB_NX];
    for (int i = 0; i < P.nx; ++i) s[i] = state[i];
    for (int t = 0; t < P.T; ++t) {
        float act[CB_NU];
        for (int i = 0; i < P.nu; ++i) act[i] = U[t * P.nu + i];
        cb_scale(P, act);  // the callers' self.u_scale * self.U[t]
        cb_dynamics(P, s, act);
        for (int i = 0; i < P.nx; ++i) traj[t * P.nx + i] = s[i];
    }
}

}  // namespace

struct mppi_cb_handle {
    mppi_cb_config cfg;
    CbParams P;
    mppi::DevBuf<float> d_U, d_state, d_cost, d_omega, d_action, d_uinit;  // (released by `delete h`)
    mppi::DevBuf<float> d_Udrawn;  // the nominal sequence the last command's samples were drawn around (after shift, before update)
    long long iter = 0;
    long long drawn_iter = -1;     // that command's iteration number; -1: no command yet
    bool drawn_injected = false;   // ... and whether its noise was an injected tensor
    std::string err;
};

static thread_local std::string g_cb_error;
#define CB_FAIL(h, code, ...)                                   \
    do {                                                        \
        char _b[400];                                           \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                  \
        if (h) (h)->err = _b; else g_cb_error = _b;             \
        return (code);                                          \
    } while (0)
#define CB_HIP(h, call)                                                                              \
    do {                                                                                             \
        hipError_t _e = (call);                                                                      \
        if (_e != hipSuccess) CB_FAIL(h, MPPI_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
    } while (0)

extern "C" const char *mppi_cb_last_error(const mppi_cb_handle *h) { return h ? h->err.c_str() : g_cb_error.c_str(); }

extern "C" int mppi_cb_create(const mppi_cb_config *c, mppi_cb_handle **out) {
    mppi_cb_handle *none = nullptr;
    if (!c || !out) CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: null argument");
    if (c->struct_size != (int32_t)sizeof(mppi_cb_config)) CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: struct_size mismatch");
    if (c->dynamics < MPPI_CB_DYN_UNICYCLE || c->dynamics > MPPI_CB_DYN_DOUBLE_INTEGRATOR)
        CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: unknown dynamics %d", c->dynamics);
    static const int NX_OF[5] = {3, 5, 4, 4, 2}, NU_OF[5] = {2, 4, 2, 2, 1};
    const int nx = NX_OF[c->dynamics], nu = NU_OF[c->dynamics];
    if (c->dynamics == MPPI_CB_DYN_RACECAR && !(c->model_params[0] > 0))
        CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: racecar wheelbase L = %g must be positive", c->model_params[0]);
    if (c->dynamics == MPPI_CB_DYN_RACECAR_DYNAMIC && !(c->model_params[0] > 0 && c->model_params[2] > 0))
        CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: racecar_dynamic l_r = %g and m = %g must be positive", c->model_params[0],
                c->model_params[2]);
    if (!std::isfinite(c->u_scale) || c->u_scale == 0)
        CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: u_scale = %g must be finite and not 0", c->u_scale);
    if (c->obstacle_kind != MPPI_CB_OBS_INVERSE && c->obstacle_kind != MPPI_CB_OBS_EXPONENTIAL)
        CB_FAIL(none, MPPI_ERR_BAD_ARG, "mppi_cb_create: unknown obstacle cost %d", c->obstacle_kind);
    if (c->K < 1 || c->T < 1 || c->T * nu > 256 || c->n_obs < 0 || c->n_obs > CB_OBS || !(c->lambda_ > 0) || !(c->dt > 0))
        CB_FAIL(none, MPPI_ERR_SHAPE, "mppi_cb_create: K=%d T=%d (T*nu <= 256) n_obs=%d (<= %d) lambda=%g dt=%g", c->K, c->T, c->n_obs,
                CB_OBS, c->lambda_, c->dt);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || c->device < 0 || c->device >= ndev)
        CB_FAIL(none, MPPI_ERR_NO_DEVICE, "mppi_cb_create: no such HIP device %d", c->device);
    // the factorisation reads the lower triangle only: the upper one has to say the same, within rounding of the caller's own
    // arithmetic relative to the diagonal (|S_ij - S_ji| <= 1e-9 sqrt(S_ii S_jj); NaN fails either test)
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < i; ++j) {
            const double scale = sqrt(fabs(c->noise_sigma[i * 4 + i] * c->noise_sigma[j * 4 + j]));
            if (!(fabs(c->noise_sigma[i * 4 + j] - c->noise_sigma[j * 4 + i]) <= 1e-9 * scale))
                CB_FAIL(none, MPPI_ERR_BAD_ARG, "noise_sigma must be symmetric positive definite: [%d][%d] = %g, [%d][%d] = %g", i, j,
                        c->noise_sigma[i * 4 + j], j, i, c->noise_sigma[j * 4 + i]);
        }
    // Cholesky factor and inverse of the nu x nu noise covariance (f64 on the host)
    double L[16] = {0}, Li[16] = {0}, Sinv[16] = {0};
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j <= i; ++j) {
            double a = c->noise_sigma[i * 4 + j];
            for (int k = 0; k < j; ++k) a -= L[i * 4 + k] * L[j * 4 + k];
            if (i == j) {
                if (!(a > 0)) CB_FAIL(none, MPPI_ERR_BAD_ARG, "noise_sigma must be symmetric positive definite");
                L[i * 4 + i] = sqrt(a);
            } else {
                L[i * 4 + j] = a / L[j * 4 + j];
            }
        }
    for (int i = 0; i < nu; ++i) {  // L^-1 by forward substitution
        Li[i * 4 + i] = 1.0 / L[i * 4 + i];
        for (int j = 0; j < i; ++j) {
            double a = 0;
            for (int k = j; k < i; ++k) a -= L[i * 4 + k] * Li[k * 4 + j];
            Li[i * 4 + j] = a / L[i * 4 + i];
        }
    }
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nu; ++j) {
            double a = 0;
            for (int k = 0; k < nu; ++k) a += Li[k * 4 + i] * Li[k * 4 + j];
            Sinv[i * 4 + j] = a;
        }
    mppi_cb_handle *h = new mppi_cb_handle();
    h->cfg = *c;
    CbParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.K = c->K; P.T = c->T; P.nx = nx; P.nu = nu; P.dynamics = c->dynamics; P.obstacle_kind = c->obstacle_kind;
    P.n_obs = c->n_obs; P.sample_null_action = c->sample_null_action;
    P.dt = (float)c->dt; P.lambda_ = (float)c->lambda_; P.safety = (float)c->safety_distance; P.obstacle_weight = (float)c->obstacle_weight;
    for (int i = 0; i < nx; ++i) { P.goal[i] = (float)c->goal[i]; P.q[i] = (float)c->q_diag[i]; }
    for (int i = 0; i < nu; ++i) { P.r[i] = (float)c->r_diag[i]; P.u_min[i] = (float)c->u_min[i]; P.u_max[i] = (float)c->u_max[i]; }
    for (int i = 0; i < 16; ++i) { P.sinv[i] = (float)Sinv[i]; P.chol[i] = (float)L[i]; }
    for (int m = 0; m < c->n_obs; ++m)
        for (int q = 0; q < 4; ++q) P.obs[m][q] = (float)c->obstacles[m * 4 + q];
    for (int i = 0; i < 5; ++i) P.skid[i] = (float)c->skid_params[i];
    P.seed_lo = (unsigned)(c->seed & 0xffffffffu);
    P.seed_hi = (unsigned)(c->seed >> 32);
    for (int i = 0; i < 8; ++i) P.model[i] = (float)c->model_params[i];
    P.terminal = c->terminal_cost != 0;
    P.abs_cost = c->noise_abs_cost != 0;
    P.u_scale = (float)c->u_scale;
    P.scaled = P.u_scale != 1.f;
    for (int i = 0; i < nx; ++i) { P.tgoal[i] = (float)c->terminal_goal[i]; P.tq[i] = (float)c->terminal_q[i]; }
    for (int i = 0; i < nu; ++i) {
        P.mu[i] = (float)c->noise_mu[i];
        P.has_mu |= P.mu[i] != 0.f;
    }
    auto fail = [&](const char *what, hipError_t e) {
        g_cb_error = std::string(what) + " failed: " + hipGetErrorString(e);
        mppi_cb_destroy(h);
        return (int)MPPI_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = h->d_U.alloc(sizeof(float) * c->T * nu)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_Udrawn.alloc(sizeof(float) * c->T * nu)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_state.alloc(sizeof(float) * CB_NX)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_cost.alloc(sizeof(float) * c->K)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_omega.alloc(sizeof(float) * c->K)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_action.alloc(sizeof(float) * CB_NU)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = h->d_uinit.alloc(sizeof(float) * CB_NU)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMemset(h->d_U, 0, sizeof(float) * c->T * nu)) != hipSuccess) return fail("hipMemset", e);
    float ui[CB_NU];
    for (int i = 0; i < CB_NU; ++i) ui[i] = (float)c->u_init[i];
    if ((e = hipMemcpy(h->d_uinit, ui, sizeof(ui), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
    *out = h;
    return MPPI_OK;
}

extern "C" int mppi_cb_destroy(mppi_cb_handle *h) {
    if (!h) return MPPI_OK;
    hipSetDevice(h->cfg.device);
    delete h;
    return MPPI_OK;
}

static int cb_io(mppi_cb_handle *h, float *dev, double *host_out, const double *host_in, size_t n) {
    std::vector<float> tmp(n);
    if (host_in) {
        for (size_t i = 0; i < n; ++i) tmp[i] = (float)host_in[i];
        CB_HIP(h, hipMemcpy(dev, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    } else {
        CB_HIP(h, hipMemcpy(tmp.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) host_out[i] = (double)tmp[i];
    }
    return MPPI_OK;
}

extern "C" int mppi_cb_set_nominal(mppi_cb_handle *h, const double *U) {
    if (!h || !U) return MPPI_ERR_BAD_ARG;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    CB_HIP(h, hipDeviceSynchronize());
    return cb_io(h, h->d_U, nullptr, U, (size_t)h->P.T * h->P.nu);
}
extern "C" int mppi_cb_get_nominal(mppi_cb_handle *h, double *U) {
    if (!h || !U) return MPPI_ERR_BAD_ARG;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    CB_HIP(h, hipDeviceSynchronize());
    return cb_io(h, h->d_U, U, nullptr, (size_t)h->P.T * h->P.nu);
}
extern "C" int mppi_cb_get_costs(mppi_cb_handle *h, double *cost_total, double *omega) {
    if (!h) return MPPI_ERR_BAD_ARG;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    CB_HIP(h, hipDeviceSynchronize());
    if (cost_total)
        if (int rc = cb_io(h, h->d_cost, cost_total, nullptr, (size_t)h->P.K)) return rc;
    if (omega)
        if (int rc = cb_io(h, h->d_omega, omega, nullptr, (size_t)h->P.K)) return rc;
    return MPPI_OK;
}

extern "C" int mppi_cb_command(mppi_cb_handle *h, const double *state, const float *eps, int32_t shift_nominal_trajectory,
                               double *action_out, void *stream) {
    if (!h || !state || !action_out) return MPPI_ERR_BAD_ARG;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    float st[CB_NX] = {0, 0, 0, 0, 0};
    for (int i = 0; i < h->P.nx; ++i) st[i] = (float)state[i];
    CB_HIP(h, hipMemcpyAsync(h->d_state, st, sizeof(st), hipMemcpyHostToDevice, s));
    if (shift_nominal_trajectory) hipLaunchKernelGGL(k_cb_shift, dim3(1), dim3(256), 0, s, h->P, h->d_U, h->d_uinit);
    hipLaunchKernelGGL(k_cb_rollout, dim3((h->P.K + 255) / 256), dim3(256), 0, s, h->P, h->d_U, h->d_state, eps,
                       (unsigned)h->iter, h->d_cost);
    hipLaunchKernelGGL(k_cb_update, dim3(1), dim3(256), 0, s, h->P, h->d_U, eps, (unsigned)h->iter, h->d_cost, h->d_omega,
                       h->d_action, h->d_Udrawn);
    CB_HIP(h, hipGetLastError());
    float act[CB_NU];
    CB_HIP(h, hipMemcpyAsync(act, h->d_action, sizeof(act), hipMemcpyDeviceToHost, s));
    CB_HIP(h, hipStreamSynchronize(s));
    for (int i = 0; i < h->P.nu; ++i) action_out[i] = (double)act[i];
    h->drawn_iter = h->iter;
    h->drawn_injected = eps != nullptr;
    ++h->iter;
    return MPPI_OK;
}

extern "C" int mppi_cb_eval(mppi_cb_handle *h, int32_t what, const double *states, const double *actions, int32_t t, int32_t n,
                            double *out) {
    if (!h || !states || (!actions && what != 2) || !out || n < 1 || what < 0 || what > 2) return MPPI_ERR_BAD_ARG;
    if (what == 2 && !h->P.terminal) CB_FAIL(h, MPPI_ERR_STATE, "mppi_cb_eval: the handle has no terminal cost");
    CB_HIP(h, hipSetDevice(h->cfg.device));
    const int nx = h->P.nx, nu = h->P.nu, n_out = what == 0 ? nx : 1;
    mppi::DevBuf<float> ds, du, dout;  // released on every exit, the early ones of CB_HIP included
    CB_HIP(h, ds.alloc(sizeof(float) * (size_t)n * nx));
    CB_HIP(h, du.alloc(sizeof(float) * (size_t)n * nu));
    CB_HIP(h, dout.alloc(sizeof(float) * (size_t)n * n_out));
    int rc = cb_io(h, ds, nullptr, states, (size_t)n * nx);
    if (!rc && what != 2) rc = cb_io(h, du, nullptr, actions, (size_t)n * nu);
    if (!rc) {
        hipLaunchKernelGGL(k_cb_eval, dim3((n + 255) / 256), dim3(256), 0, nullptr, h->P, what, ds, du, t, n, dout);
        if (hipDeviceSynchronize() != hipSuccess) rc = MPPI_ERR_HIP;
    }
    if (!rc) rc = cb_io(h, dout, out, nullptr, (size_t)n * n_out);
    return rc;
}

extern "C" int mppi_cb_nominal_trajectory(mppi_cb_handle *h, const double *state, double *traj) {
    if (!h || !state || !traj) return MPPI_ERR_BAD_ARG;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    float st[CB_NX] = {0, 0, 0, 0, 0};
    for (int i = 0; i < h->P.nx; ++i) st[i] = (float)state[i];
    mppi::DevBuf<float> dt;
    CB_HIP(h, dt.alloc(sizeof(float) * (size_t)h->P.T * h->P.nx));
    CB_HIP(h, hipMemcpy(h->d_state, st, sizeof(st), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cb_nominal, dim3(1), dim3(64), 0, nullptr, h->P, h->d_U, h->d_state, dt);
    int rc = hipDeviceSynchronize() == hipSuccess ? MPPI_OK : MPPI_ERR_HIP;
    if (!rc) rc = cb_io(h, dt, traj, nullptr, (size_t)h->P.T * h->P.nx);
    return rc;
}

// the last command's draw can be made again from (drawn_iter, d_Udrawn) and Philox, or from the injected tensor handed in again
static int cb_check_drawn(mppi_cb_handle *h, const float *eps, const char *who) {
    if (h->drawn_iter < 0) CB_FAIL(h, MPPI_ERR_STATE, "%s: no command has run on this handle", who);
    if (h->drawn_injected != (eps != nullptr))
        CB_FAIL(h, MPPI_ERR_STATE, "%s: the last command's noise was %s", who,
                h->drawn_injected ? "injected: hand the same tensor in again" : "drawn in the kernel: eps must be NULL");
    return MPPI_OK;
}

extern "C" int mppi_cb_get_perturbed_actions(mppi_cb_handle *h, const float *eps, double *out) {
    if (!h || !out) return MPPI_ERR_BAD_ARG;
    if (int rc = cb_check_drawn(h, eps, "mppi_cb_get_perturbed_actions")) return rc;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)h->P.K * h->P.T;
    mppi::DevBuf<float> dout;
    CB_HIP(h, dout.alloc(sizeof(float) * rows * h->P.nu));
    hipLaunchKernelGGL(k_cb_perturbed, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, nullptr, h->P, h->d_Udrawn, eps,
                       (unsigned)h->drawn_iter, dout);
    CB_HIP(h, hipGetLastError());
    CB_HIP(h, hipDeviceSynchronize());
    return cb_io(h, dout, out, nullptr, rows * h->P.nu);
}

extern "C" int mppi_cb_top_trajectories(mppi_cb_handle *h, const double *state, const float *eps, int32_t n, double *traj_out,
                                        int32_t *index_out) {
    if (!h || !state || !traj_out || !index_out) return MPPI_ERR_BAD_ARG;
    if (n < 1 || n > h->P.K) CB_FAIL(h, MPPI_ERR_SHAPE, "mppi_cb_top_trajectories: n = %d outside [1, K = %d]", n, h->P.K);
    if (int rc = cb_check_drawn(h, eps, "mppi_cb_top_trajectories")) return rc;
    CB_HIP(h, hipSetDevice(h->cfg.device));
    float st[CB_NX] = {0, 0, 0, 0, 0};
    for (int i = 0; i < h->P.nx; ++i) st[i] = (float)state[i];
    const size_t n_traj = (size_t)n * h->P.T * h->P.nx;
    mppi::DevBuf<float> dtraj;
    mppi::DevBuf<int> didx;
    CB_HIP(h, dtraj.alloc(sizeof(float) * n_traj));
    CB_HIP(h, didx.alloc(sizeof(int) * (size_t)n));
    CB_HIP(h, hipMemcpy(h->d_state, st, sizeof(st), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cb_top, dim3((h->P.K + 255) / 256), dim3(256), 0, nullptr, h->P, h->d_Udrawn, h->d_state, eps,
                       (unsigned)h->drawn_iter, h->d_cost, n, dtraj, didx);
    CB_HIP(h, hipGetLastError());
    CB_HIP(h, hipDeviceSynchronize());
    if (int rc = cb_io(h, dtraj, traj_out, nullptr, n_traj)) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "index_out is read back as it is");
    CB_HIP(h, hipMemcpy(index_out, didx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return MPPI_OK;
}
