/* Host-side check of libmppi_hip.so under AddressSanitizer (make -C dnn-mppi-mpc_amd/csrc asan_check; no GPU needed):
 * the entry points that run on the host before any device work -- argument validation, error strings, create on a box
 * without a device -- are driven with good and bad arguments; ASan reports any out-of-bounds access or leak. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mppi_hip.h"
#include "mppi_grid_index.h" /* the cost grids' index arithmetic, as the kernels and the host compile it */
#include "mppi_scene_staging.h" /* what a composed launch stages into LDS, likewise */

static int fails = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

int main(void) {
    EXPECT(mppi_abi_version() == MPPI_ABI_VERSION);
    mppi_config c;
    memset(&c, 0, sizeof(c));
    mppi_handle *h = NULL;
    EXPECT(mppi_create(NULL, &h) == MPPI_ERR_BAD_ARG);
    EXPECT(mppi_create(&c, NULL) == MPPI_ERR_BAD_ARG);
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG); /* struct_size 0 */
    EXPECT(strlen(mppi_last_error(NULL)) > 0);
    c.struct_size = (int32_t)sizeof(c);
    c.K = 0;
    c.T = 10;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_SHAPE);
    c.K = 256;
    c.model = 7;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG);
    c.model = MPPI_MODEL_DIFFDRIVE;
    c.search_window = 20;
    c.filter_window = 10;
    c.sigma[0] = 0.1; c.sigma[3] = 0.01;
    c.param_exploration = 0.05; c.param_lambda = 1.0; c.param_alpha = 0.2;
    c.delta_t = 0.1;
    c.sigma[1] = c.sigma[2] = 1.0; /* not positive definite */
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG);
    c.sigma[1] = c.sigma[2] = 0.0;
    /* moving obstacles: the create-time refusals come before any device work, each with its reason as text */
    c.obstacle_motion = 1; /* (obstacle_model is MPPI_OBSTACLE_NONE) */
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "MPPI_OBSTACLE_NONE") != NULL);
    c.obstacle_model = MPPI_OBSTACLE_CIRCLE;
    c.model = MPPI_MODEL_DIFFDRIVE_MLP;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_UNSUPPORTED && strstr(mppi_last_error(NULL), "MPPI_MODEL_DIFFDRIVE_MLP") != NULL);
    EXPECT(strstr(mppi_last_error(NULL), "obstacle_motion = 2") != NULL); /* (the refusal points to the learned scene handle) */
    /* the learned model's scene handle, value 2: its create paths up to the device check */
    c.obstacle_motion = MPPI_OBSTACLE_MOTION_LEARNED;
    c.model = MPPI_MODEL_DIFFDRIVE;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "MPPI_MODEL_DIFFDRIVE_MLP") != NULL);
    c.model = MPPI_MODEL_RACECAR;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG);
    c.model = MPPI_MODEL_DIFFDRIVE_MLP;
    c.obstacle_model = MPPI_OBSTACLE_NONE;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "MPPI_OBSTACLE_NONE") != NULL);
    c.obstacle_model = MPPI_OBSTACLE_CIRCLE;
    c.waypoint_mode = MPPI_WAYPOINT_FROZEN;
    c.n_agents = 3;
    c.fleet_radius = 0.4;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_UNSUPPORTED && strstr(mppi_last_error(NULL), "fleet") != NULL);
    c.fleet_radius = 0.0;
    c.n_agents = 0;
    c.K_global = 512;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_UNSUPPORTED && strstr(mppi_last_error(NULL), "shard") != NULL);
    c.K_global = 0;
    c.precision = MPPI_PREC_F64;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_UNSUPPORTED);
    c.precision = MPPI_PREC_F32;
    {   /* past every refusal: the handle, or -- without an MI355X -- the device check */
        const int rc2 = mppi_create(&c, &h);
        EXPECT(rc2 == MPPI_OK || rc2 == MPPI_ERR_NO_DEVICE);
        if (rc2 == MPPI_OK) EXPECT(mppi_destroy(h) == MPPI_OK);
        h = NULL;
    }
    c.waypoint_mode = MPPI_WAYPOINT_SEQUENTIAL;
    c.model = MPPI_MODEL_DIFFDRIVE;
    /* fleet avoidance: likewise refused before any device work (obstacle_model is MPPI_OBSTACLE_CIRCLE here) */
    c.obstacle_motion = 1;
    c.waypoint_mode = MPPI_WAYPOINT_FROZEN;
    c.n_agents = 3;
    c.fleet_radius = -0.5;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "fleet_radius") != NULL);
    c.fleet_radius = NAN;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG);
    c.fleet_radius = INFINITY;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG);
    c.fleet_radius = 0.4;
    c.n_agents = 1;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "n_agents >= 2") != NULL);
    c.n_agents = 3;
    c.obstacle_motion = 0;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_BAD_ARG && strstr(mppi_last_error(NULL), "obstacle_motion = 1") != NULL);
    c.obstacle_motion = 1;
    c.n_agents = 257;
    EXPECT(mppi_create(&c, &h) == MPPI_ERR_UNSUPPORTED && strstr(mppi_last_error(NULL), "256") != NULL);
    c.n_agents = 0;
    c.fleet_radius = 0.0;
    c.waypoint_mode = MPPI_WAYPOINT_SEQUENTIAL;
    {   /* the two entry points that came with it refuse a NULL handle before anything is read or written */
        int32_t m = -7;
        double d = -1.0;
        int64_t n = -1;
        EXPECT(mppi_get_agent_circles(NULL, 0, &d, &d, 1, &m) == MPPI_ERR_BAD_ARG && m == -7);
        EXPECT(mppi_get_fleet_clearance(NULL, &d, &n, 1) == MPPI_ERR_BAD_ARG && n == -1);
        /* and so do the two of the fleet's plan mode */
        EXPECT(mppi_set_fleet_prediction(NULL, MPPI_FLEET_PLAN) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_fleet_plans(NULL, &d) == MPPI_ERR_BAD_ARG && d == -1.0);
        /* and the three of the obstacle tracks */
        EXPECT(mppi_set_obstacle_tracks(NULL, &d, &d, 1, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_obstacle_tracks(NULL, 0, &d, &d, 1, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_obstacle_tracks_at(NULL, 0, 0, &d, 1, &m) == MPPI_ERR_BAD_ARG && m == -7 && d == -1.0);
        /* and the three of the cost grids */
        EXPECT(mppi_set_cost_grid(NULL, &d, 2, 2, 0.0, 0.0, 1.0, 1.0, 0.5) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_cost_grid(NULL, 0, &d, 2, 2, 0.0, 0.0, 1.0, 1.0, 0.5) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_eval_cost_grid(NULL, 0, &d, 1, &d) == MPPI_ERR_BAD_ARG && d == -1.0);
        /* and the two of the composed scenes: NULL comes first, a good or a bad mode alike */
        EXPECT(mppi_set_scene_mode(NULL, MPPI_SCENE_COMPOSED) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_scene_mode(NULL, 2) == MPPI_ERR_BAD_ARG && mppi_set_scene_mode(NULL, -1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_scene_mode(NULL, &m) == MPPI_ERR_BAD_ARG && m == -7);
        /* and the three of the cost-grid footprint: NULL comes first, a good or a bad mode alike; nothing is written */
        EXPECT(mppi_set_cost_grid_footprint(NULL, MPPI_GRID_FOOTPRINT_OUTLINE) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_cost_grid_footprint(NULL, 2) == MPPI_ERR_BAD_ARG && mppi_set_cost_grid_footprint(NULL, -1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_cost_grid_footprint(NULL, &m) == MPPI_ERR_BAD_ARG && m == -7);
        EXPECT(mppi_get_cost_grid_footprint(NULL, NULL) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_eval_cost_grid_footprint(NULL, 0, &d, 1, &d, &d) == MPPI_ERR_BAD_ARG && d == -1.0);
        EXPECT(mppi_eval_cost_grid_footprint(NULL, -1, NULL, 0, NULL, NULL) == MPPI_ERR_BAD_ARG);
    }
    {   /* the composed launches' staging at its budget edges (T = 128: 2064 bytes of plans per agent and 2072 per track in
         * f64, half of each in f32): plans first, the tracks 16-byte aligned behind them, each only if it fits; a buffer of the
         * total is written at both regions' last bytes, so a wrong size or offset is an out-of-bounds write for ASan */
        static const int cases[][6] = {/* elem, plan agents, tracks, T -> plans, tracks */
            {8, 3, 4, 128, 6192, 8288}, {8, 3, 5, 128, 6192, 0}, {8, 7, 1, 128, 14448, 0}, {8, 8, 7, 128, 0, 14504},
            {8, 8, 8, 128, 0, 0}, {8, 0, 7, 128, 0, 14504}, {8, 0, 8, 128, 0, 0}, {4, 38, 0, 128, 39216, 0}, {4, 39, 0, 128, 0, 0},
            {4, 3, 35, 128, 3096, 36260}, {4, 3, 36, 128, 3096, 0}, {4, 39, 38, 128, 0, 39368}, {4, 39, 39, 128, 0, 0},
            {4, 1, 1, 2, 24, 28}, {4, 0, 0, 50, 0, 0}};
        for (size_t q = 0; q < sizeof(cases) / sizeof(cases[0]); ++q) {
            const int *c = cases[q];
            const mppi_scene_staging s = mppi_scene_lds_bytes(c[0], c[1], c[2], c[3]);
            const int off = mppi_scene_track_offset(s.plans), total = mppi_scene_lds_total(s);
            EXPECT(s.plans == c[4] && s.tracks == c[5]);
            EXPECT(off % 16 == 0 && off >= s.plans && off < s.plans + 16 && total <= (c[0] == 4 ? 40000 : 16384));
            char *lds = (char *)calloc((size_t)total + 1, 1);
            if (s.plans > 0) lds[s.plans - 1] = 1;
            if (s.tracks > 0) { lds[off] = 2; lds[off + s.tracks - 1] = 3; }
            EXPECT(total == (s.tracks > 0 ? off + s.tracks : s.plans));
            free(lds);
        }
        EXPECT(mppi_scene_track_offset(24) == 32 && mppi_scene_track_offset(32) == 32 && mppi_scene_track_offset(0) == 0);
    }
    {   /* the grids' index function stays inside [0, n - 2] and its fraction inside [0, 1] whatever the coordinate is; the
         * table below is read at both nodes it names, so a wrong index is an out-of-bounds read for ASan */
        static const double xs[] = {NAN, INFINITY, -INFINITY, 1e30, -1e30, 0.0, -0.0, 1e-30, 0.999999, 1.0, 2.5, 4094.5, 4095.0, 4096.0};
        static const int ns[] = {2, 3, 7, 4096};
        for (size_t q = 0; q < sizeof(ns) / sizeof(ns[0]); ++q) {
            const int n = ns[q];
            float *row32 = (float *)calloc((size_t)n, sizeof(float));
            double *row64 = (double *)calloc((size_t)n, sizeof(double));
            for (size_t i = 0; i < sizeof(xs) / sizeof(xs[0]); ++i) {
                float f32 = -1.0f;
                double f64 = -1.0;
                const int i32 = mppi_grid_index_f32((float)xs[i], 0.0f, 1.0f, n, &f32);
                const int i64 = mppi_grid_index_f64(xs[i], 0.0, 1.0, n, &f64);
                EXPECT(i32 >= 0 && i32 <= n - 2 && f32 >= 0.0f && f32 <= 1.0f);
                EXPECT(i64 >= 0 && i64 <= n - 2 && f64 >= 0.0 && f64 <= 1.0);
                EXPECT(row32[i32] + row32[i32 + 1] == 0.0f && row64[i64] + row64[i64 + 1] == 0.0);
            }
            /* a shifted and scaled axis: o = -3, resolution 0.5 */
            float f = -1.0f;
            EXPECT(mppi_grid_index_f32(-2.25f, -3.0f, 2.0f, n, &f) == (n > 2 ? 1 : 0) && f == (n > 2 ? 0.5f : 1.0f));
            free(row32);
            free(row64);
        }
    }
    c.obstacle_model = MPPI_OBSTACLE_NONE;
    c.obstacle_motion = 0;
    {   /* and the setters refuse a NULL handle before anything is read */
        double circle[3] = {0.5, 0.5, 0.1}, vel[2] = {0.1, 0.0};
        int32_t step = 0;
        double out = 0.0;
        EXPECT(mppi_set_obstacles_moving(NULL, circle, vel, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_obstacles_moving(NULL, 0, circle, vel, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_eval_is_collided_at(NULL, circle, 1, &step, &out) == MPPI_ERR_BAD_ARG);
    }
    const int rc = mppi_create(&c, &h); /* a box without an MI355X: MPPI_ERR_NO_DEVICE, with the reason as text */
    if (rc == MPPI_OK) {
        double path[6] = {0, 0, 0, 1, 1, 0};
        EXPECT(mppi_set_ref_path(h, path, 2, 3) == MPPI_OK);
        EXPECT(mppi_set_ref_path(h, path, 0, 3) == MPPI_ERR_SHAPE);
        EXPECT(mppi_set_waypoint_idx(h, 5) == MPPI_ERR_BAD_ARG);
        /* the per-agent setters on a single-agent handle: agent 0 is the plain setter, any other agent is refused */
        double circle[3] = {0.5, 0.5, 0.1};
        int32_t idx = -1, end = -1;
        EXPECT(mppi_set_agent_ref_path(h, 0, path, 2, 3) == MPPI_OK);
        EXPECT(mppi_set_agent_ref_path(h, 0, path, 2, 2) == MPPI_ERR_SHAPE);
        EXPECT(mppi_set_agent_ref_path(h, 0, NULL, 2, 3) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_ref_path(h, -1, path, 2, 3) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_ref_path(h, 1, path, 2, 3) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_obstacles(h, 0, circle, 1) == MPPI_OK);
        EXPECT(mppi_set_agent_obstacles(h, 0, NULL, 0) == MPPI_OK);
        EXPECT(mppi_set_agent_obstacles(h, 0, NULL, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_obstacles(h, 0, circle, -1) == MPPI_ERR_SHAPE);
        EXPECT(mppi_set_agent_obstacles(h, 1, circle, 1) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_agent_status(h, &idx, NULL) == MPPI_OK && idx == 0);
        EXPECT(mppi_get_agent_status(h, NULL, &end) == MPPI_OK);
        EXPECT(mppi_destroy(h) == MPPI_OK);
    } else {
        EXPECT(rc == MPPI_ERR_NO_DEVICE);
        EXPECT(strstr(mppi_last_error(NULL), "HIP device") != NULL || strstr(mppi_last_error(NULL), "gfx950") != NULL);
    }
    EXPECT(mppi_destroy(NULL) == MPPI_OK);
    {
        double path[6] = {0, 0, 0, 1, 1, 0};
        EXPECT(mppi_set_agent_ref_path(NULL, 0, path, 2, 3) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_obstacles(NULL, 0, path, 2) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_get_agent_status(NULL, NULL, NULL) == MPPI_ERR_BAD_ARG);
    }
    {   /* the per-agent model setters: a NULL handle is refused before anything is read */
        static float w_in[64 * 5], b_in[64], w_h[64 * 64], b_h[64], w_out[3 * 64], b_out[3];
        const float *wh[1] = {w_h}, *bh[1] = {b_h};
        const double m5[5] = {0, 0, 0, 0, 0}, s5[5] = {1, 1, 1, 1, 1};
        EXPECT(mppi_set_agent_mlp(NULL, 0, 64, 1, w_in, b_in, wh, bh, w_out, b_out) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_agent_mlp_scaled(NULL, 0, 64, 1, w_in, b_in, wh, bh, w_out, b_out, m5, s5, m5, s5) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_mlp(NULL, 64, 1, w_in, b_in, wh, bh, w_out, b_out) == MPPI_ERR_BAD_ARG);
        EXPECT(mppi_set_mlp_scaled(NULL, 64, 1, w_in, b_in, wh, bh, w_out, b_out, NULL, NULL, NULL, NULL) == MPPI_ERR_BAD_ARG);
    }
    EXPECT(mppi_comm_unique_id(NULL) == MPPI_ERR_BAD_ARG);
    EXPECT(mppi_get_rollout_kernel(NULL, NULL, 0) == MPPI_ERR_BAD_ARG);
    mppi_cb_config cb;
    memset(&cb, 0, sizeof(cb));
    mppi_cb_handle *hc = NULL;
    EXPECT(mppi_cb_create(&cb, &hc) != MPPI_OK);
    printf(fails ? "asan_host_check: %d expectation(s) failed\n" : "asan_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
