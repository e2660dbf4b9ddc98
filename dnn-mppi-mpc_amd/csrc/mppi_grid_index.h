/* Cost grids (mppi_set_cost_grid): the index arithmetic of the bilinear lookup along one axis, one definition for the kernels,
 * the host and a plain C caller (examples/asan_host_check.c drives it with NaN, +-inf and 1e30).  mppi_kernels.h includes it.
 *   g = fmin(fmax((x - o) inv, 0), n - 1);   i = min((int)g, n - 2);   f = g - i
 * fmax / fmin return their other operand for a NaN, so a NaN coordinate lands on node 0 and +-inf on an edge node; the
 * conversion to int sees a value inside [0, n - 1] whatever x is.  For n >= 2 the result lies in [0, n - 2]: both i and i + 1
 * are nodes of the axis, and f lies in [0, 1]. */
#ifndef MPPI_GRID_INDEX_H
#define MPPI_GRID_INDEX_H
#include <math.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPPI_GRID_HD __host__ __device__
#else
#define MPPI_GRID_HD
#endif
static inline MPPI_GRID_HD int mppi_grid_index_f32(float x, float o, float inv, int n, float *f) {
    const float g = fminf(fmaxf((x - o) * inv, 0.0f), (float)(n - 1));
    const int t = (int)g, i = t < n - 2 ? t : n - 2;
    *f = g - (float)i;
    return i;
}
static inline MPPI_GRID_HD int mppi_grid_index_f64(double x, double o, double inv, int n, double *f) {
    const double g = fmin(fmax((x - o) * inv, 0.0), (double)(n - 1));
    const int t = (int)g, i = t < n - 2 ? t : n - 2;
    *f = g - (double)i;
    return i;
}
#endif
