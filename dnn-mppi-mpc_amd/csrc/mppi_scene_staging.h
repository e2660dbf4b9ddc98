/* Composed scenes (mppi_set_scene_mode): what a launch that carries fleet plans AND obstacle tracks stages into dynamic LDS,
 * one definition for the planner (which sizes the launch by it), the kernels (which decide by it where they read) and a
 * plain C caller (examples/asan_host_check.c and tests/test_scene_cases.py drive it at its budget edges).  mppi_kernels.h
 * includes it.
 *   budget: 40000 bytes for 4-byte elements, 16384 for 8-byte ones -- what fits beside the rollout forms' own LDS within the
 *           64 KB a workgroup gets without raising a limit (fleet_plan_lds_bytes / track_lds_bytes: the same limits)
 *   plans:  n_plan_agents (T + 1) points of two elements (0 agents: the handle has no plans); staged if they fit the budget
 *   tracks: the window of the largest set, n_max tracks of (T + 1) points and one threshold each; staged 16-byte aligned
 *           behind the plans if they fit what remains
 * Whatever does not fit is read from memory: plans too large on their own leave the tracks the whole budget. */
#ifndef MPPI_SCENE_STAGING_H
#define MPPI_SCENE_STAGING_H
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPPI_SCENE_HD __host__ __device__
#else
#define MPPI_SCENE_HD
#endif
typedef struct mppi_scene_staging {
    int plans, tracks; /* bytes staged (0: read from memory, or absent) */
} mppi_scene_staging;
/* where the tracks' window starts behind `plans` staged bytes */
static inline MPPI_SCENE_HD int mppi_scene_track_offset(int plans) { return (plans + 15) & ~15; }
/* the dynamic LDS a launch with this staging needs */
static inline MPPI_SCENE_HD int mppi_scene_lds_total(mppi_scene_staging s) {
    return s.tracks > 0 ? mppi_scene_track_offset(s.plans) + s.tracks : s.plans;
}
static inline MPPI_SCENE_HD mppi_scene_staging mppi_scene_lds_bytes(int elem_bytes, int n_plan_agents, int n_max, int T) {
    const long long budget = elem_bytes == 4 ? 40000 : 16384;
    const long long pb = (long long)n_plan_agents * (T + 1) * 2 * elem_bytes;
    const long long tb = (long long)n_max * ((T + 1) * 2 + 1) * elem_bytes;
    mppi_scene_staging s = {0, 0};
    if (pb > 0 && pb <= budget) s.plans = (int)pb;
    if (tb > 0 && mppi_scene_track_offset(s.plans) + tb <= budget) s.tracks = (int)tb;
    return s;
}
#endif
