/*
 * mppi_hip.h -- C ABI of libmppi_hip.so, the MI355X (gfx950) MPPI rollout engine.
 *
 * The reference (SokhengDin/DNN-MPPI-MPC) has no FFI: its boundary for this path is the
 * Python class surface of controllers/mppi_differential_drive*.py and
 * controllers/mppi_race_car*.py.  This header is the C ABI placed underneath that surface
 * (SURVEY.md section 8b); every entry point cites the reference code it stands in for.
 * `file:line` citations are relative to the reference repository root.
 *
 * Conventions
 *   - every function returns 0 on success or a negative mppi_status; text via
 *     mppi_last_error().  No exception crosses the ABI.
 *   - "host" pointers are ordinary CPU memory; "device" pointers are HIP device memory on
 *     the handle's GPU (e.g. torch.Tensor.data_ptr() of a contiguous CUDA tensor --
 *     accepted zero-copy).  The caller owns every buffer it passes.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - a handle is not thread-safe: one handle per host thread / GPU.
 */
#ifndef MPPI_HIP_H
#define MPPI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: mppi_config.fleet_radius.  mppi_config.obstacle_motion = 2 (MPPI_OBSTACLE_MOTION_LEARNED, the learned model's scene handle)
 * arrived WITHOUT a bump -- no symbol, field or layout changed -- so a caller that needs it probes by the answer of mppi_create:
 * a library without it refuses value 2 with MPPI_ERR_BAD_ARG whatever the model. */
#define MPPI_ABI_VERSION 8

typedef enum {
    MPPI_OK = 0,
    MPPI_ERR_BAD_ARG = -1,    /* null pointer, bad enum, inconsistent sizes */
    MPPI_ERR_SHAPE = -2,      /* T below the filter window, K < 1, path not set ... */
    MPPI_ERR_NO_DEVICE = -3,  /* no HIP device / wrong architecture */
    MPPI_ERR_HIP = -4,        /* a HIP runtime call failed */
    MPPI_ERR_PATH_END = -5,   /* race car: nearest waypoint is the last one (mppi_race_car.py:63-65) */
    MPPI_ERR_UNSUPPORTED = -6,/* e.g. sequential waypoint mode with K sharded over ranks */
    MPPI_ERR_STATE = -7,      /* call sequence error (step_end without step_begin ...) */
    MPPI_ERR_COMM = -8        /* peer-to-peer exchange: a rank did not arrive within the timeout */
} mppi_status;

/* dynamics: controllers/mppi_differential_drive.py:182-198 / controllers/mppi_race_car.py:183-197 */
typedef enum {
    MPPI_MODEL_DIFFDRIVE = 0,
    MPPI_MODEL_RACECAR = 1,
    /* unicycle + learned residual, x' = x + dt (f(x,v) + MLP([x,v])) (test/bullet_differential_drive_dnn.py:79-92);
     * needs mppi_set_mlp; fp32 only (MFMA) */
    MPPI_MODEL_DIFFDRIVE_MLP = 2
} mppi_model;
/* arithmetic type of the rollout/cost kernels (the noise tensor is always f32) */
typedef enum { MPPI_PREC_F32 = 0, MPPI_PREC_F64 = 1 } mppi_precision;
/* waypoint search state, SURVEY.md App. A.3:
 *  SEQUENTIAL = one index threaded through all K*(T+1) cost calls in k-major order
 *               (mppi_differential_drive.py:228,:244, update_prev_idx=True)
 *  FROZEN     = index fixed at the nearest waypoint of x0 during rollouts
 *               (mppi_race_car.py:143,:152, default update_prev_idx=False)
 *  PER_ROLLOUT = the index threads through a sample's OWN T stage calls and its terminal call exactly as the reference
 *               threads it (:228, :244: every call searches from where the previous one ended) but starts again from the
 *               x0 call's index at every sample -- the part of the reference's bookkeeping that survives when samples
 *               must be independent (K sharded over GPUs, several agents per handle, all host cores in the CPU baseline);
 *               prev_way_point_idx after the iteration = the x0 call's index, as in FROZEN.  Diff-drive models only (the
 *               race-car files have no such bookkeeping: MPPI_ERR_UNSUPPORTED) */
typedef enum { MPPI_WAYPOINT_SEQUENTIAL = 0, MPPI_WAYPOINT_FROZEN = 1, MPPI_WAYPOINT_PER_ROLLOUT = 2 } mppi_waypoint_mode;
/* softmin rate beta in w = exp(-beta (S - rho)):
 *  INV_EXPLORATION 1/param_exploration (mppi_differential_drive.py:175)
 *  INV_LAMBDA      1/param_lambda      (mppi_race_car.py:205)
 *  LAMBDA          param_lambda        (mppi_differential_drive_torch.py:187) */
typedef enum { MPPI_BETA_INV_EXPLORATION = 0, MPPI_BETA_INV_LAMBDA = 1, MPPI_BETA_LAMBDA = 2 } mppi_beta_mode;
/* smoothing of the weighted noise:
 *  DIFFDRIVE  np.convolve 'same' + edge factors incl. the repeated last-row factor
 *             (mppi_differential_drive.py:257-271)
 *  RACECAR    pad with first/last window/2 rows, convolve, unpad (mppi_race_car.py:211-222)
 *  TORCH      the torch files' variant of RACECAR: same padding, `conv1d(padding=window/2)` and the FIRST T
 *             outputs, i.e. output n averages padded rows n-5 .. n+4 with zeros before the start
 *             (mppi_differential_drive_torch.py:252-263, mppi_race_car_torch.py:211-222) */
typedef enum {
    MPPI_FILTER_DIFFDRIVE = 0, MPPI_FILTER_RACECAR = 1, MPPI_FILTER_NONE = 2, MPPI_FILTER_TORCH = 3
} mppi_filter_mode;
/* collision term (adds collision_penalty per colliding stage/terminal state):
 *  CIRCLE   robot disc of radius 0.5*margin vs circles (mppi_differential_drive_obs.py:301-313)
 *  OUTLINE  9 outline points of the (l*m) x (w*m) box vs circles (mppi_race_car_obstacle.py:241-274) */
typedef enum { MPPI_OBSTACLE_NONE = 0, MPPI_OBSTACLE_CIRCLE = 1, MPPI_OBSTACLE_OUTLINE = 2 } mppi_obstacle_model;

/* mppi_config.obstacle_motion = 2: the learned model's scene handle (documented at the field) */
#define MPPI_OBSTACLE_MOTION_LEARNED 2
/* mppi_config.obstacle_motion = 3: the learned model's fleet handle -- a scene handle with fleet_radius > 0 (likewise) */
#define MPPI_OBSTACLE_MOTION_LEARNED_FLEET 3

/*
 * Mirrors the constructor keywords of MPPIAlgorithms (mppi_differential_drive.py:44-60,
 * _obs.py:44-62) and MPPIRacecarController (mppi_race_car.py:10-27, _obstacle.py:11-30),
 * plus one switch per behavioural difference between the reference's variants
 * (SURVEY.md App. B).  Zero-initialise, set struct_size = sizeof(mppi_config).
 */
typedef struct {
    int32_t struct_size;
    int32_t device;              /* HIP device ordinal */
    int32_t model;               /* mppi_model */
    int32_t precision;           /* mppi_precision */
    int32_t K;                   /* samples evaluated by THIS handle (num_samples_K / number_of_samples_K) */
    int32_t T;                   /* horizon (num_horizons_T / horizon_step_T) */
    int32_t K_global;            /* total samples over all ranks (0 => K) */
    int32_t k_offset;            /* global index of this handle's first sample */
    double delta_t;
    double u_max[2];             /* diff: max_speed, max_omega; race: max_steer_abs, max_accel_abs */
    double wheel_base;           /* race car only */
    double param_exploration, param_lambda, param_alpha;
    double sigma[4];             /* row-major 2x2 */
    double stage_cost_weight[4]; /* diff: x,y,yaw; race: x,y,yaw,v */
    double terminal_cost_weight[4];
    int32_t beta_mode;           /* mppi_beta_mode */
    int32_t accumulate_stage_cost; /* 0: S[k] = ... (mppi_differential_drive.py:124); 1: S[k] += ... (mppi_race_car.py:84) */
    int32_t waypoint_mode;       /* mppi_waypoint_mode */
    int32_t search_window;       /* 20 (:204), 200 (mppi_race_car.py:158), 10 (_cuda.py:201) */
    int32_t wrap_yaw_stage;      /* (yaw + 2pi) % 2pi before the stage cost (mppi_race_car.py:141) */
    int32_t wrap_yaw_terminal;   /* same for the terminal cost (mppi_race_car.py:150, _cuda.py:239) */
    int32_t clamp_rollout;       /* `_g` inside the rollout (off only in mppi_differential_drive_torch.py:128) */
    int32_t clamp_u_after_update;/* in-place clamp of u by the visualisation loop (mppi_differential_drive.py:145-149) */
    int32_t filter_mode;         /* mppi_filter_mode */
    int32_t filter_window;       /* 10 in every reference file; any window >= 1 is served (< 1 => 10).  DIFFDRIVE needs
                                    T >= window, RACECAR and TORCH T >= (window + 1) / 2 (they pad with the last
                                    -(-window // 2) rows: one more than window / 2 at an odd window); shorter horizons, at
                                    which the reference's own filter raises, are MPPI_ERR_SHAPE */
    int32_t obstacle_model;      /* mppi_obstacle_model */
    int32_t raise_at_path_end;   /* 1: mppi_step returns MPPI_ERR_PATH_END (mppi_race_car.py:63-65) */
    double safety_margin;        /* diff: safety_margin_rate; race: collision_safety_margin_rate */
    double vehicle_w, vehicle_l; /* race outline, 3.0 / 4.0 (mppi_race_car_obstacle.py:53-54) */
    double collision_penalty;    /* 1.0e10 */
    uint64_t seed;               /* Philox key for the on-device sampler */
    /* Several independent MPPI problems ("agents") in one handle and one launch per stage:
     * same parameters; separate state, nominal controls, waypoint index and noise; one scene -- reference path and obstacle
     * set -- for all of them (mppi_set_ref_path / mppi_set_obstacles) or one per agent (mppi_set_agent_ref_path /
     * mppi_set_agent_obstacles: a fleet, or one planner weighing several routes).
     * 0/1 = one agent (every entry point).  > 1: needs MPPI_WAYPOINT_FROZEN or _PER_ROLLOUT and no sharding; the analytic
     * models T <= 128 and K <= 8192; MPPI_MODEL_DIFFDRIVE_MLP K <= 32768, with one mppi_set_mlp serving every agent or one
     * model per agent (mppi_set_agent_mlp: a fleet whose robots carry their own fine-tuned residuals, an ensemble of
     * checkpoints planning side by side; all of one shape), on the f16-split kernels only: MPPI_MLP_F32 and weights beyond
     * the f16 range are MPPI_ERR_UNSUPPORTED there;
     * mppi_set_state / mppi_get_state / mppi_set_u_prev / mppi_get_u_prev / mppi_get_costs then take [n_agents][...]
     * arrays and mppi_run_closed_loop advances all agents (stats: agent 0; an agent that reaches the end of its path
     * stops the call with MPPI_ERR_PATH_END: mppi_get_agent_status says which); mppi_set_waypoint_idx /
     * mppi_set_iteration apply to every agent; the host-in-the-loop and split steps, the visualisation rollouts and the
     * exchange are single-agent; the mppi_eval_* stage methods see agent 0's scene and agent 0's model. */
    int32_t n_agents;
    /* fourth word of the sampler's Philox counter (agent a of a batched handle draws with noise_stream + a, so a
     * single-agent handle with noise_stream = a reproduces its noise) */
    int32_t noise_stream;
    /* Moving obstacles.  0: every circle stands still (zero-initialised configs: as before).  1: a circle is {x, y, r, vx, vy},
     * constant velocity in world coordinates, metres per second (mppi_set_obstacles_moving, mppi_set_agent_obstacles_moving).
     * A create-time field: the rollout layout and the record buffers are decided here -- such a handle runs the one-sample-
     * per-wave kernels for every K (several agents: T <= 128 and K <= 8192, as documented above).
     * THE OBSTACLE CLOCK IS THE HANDLE'S ITERATION COUNTER, the one the sampler reads (mppi_stats.iteration): with iter0 its
     * value when the set was uploaded, n = iteration - iter0 control steps have passed since, and the state a rollout reaches
     * after j steps is tested against the centres c + v * (delta_t * (n + j)): j = 1 .. T for the stage calls, j = T for the
     * terminal call (it prices the same state as the last stage call), j = 0 for whatever prices "now" (mppi_eval_is_collided,
     * mppi_eval_cost).  delta_t * (n + j) is evaluated in the handle's precision with the integer n + j converted exactly,
     * then one fused multiply-add per coordinate; zero velocities give the static centres exactly.  An f32 handle loses centre
     * precision as |v| * delta_t * n grows (half an ulp of that product): a caller to whom that matters uploads fresh
     * positions, which re-bases iter0.
     * One iteration is one tick: all speculation rounds of an iteration see the same clock, mppi_run_closed_loop advances
     * the obstacles with the plant without the host, and a replayed graph (MPPI_GRAPH=1) reads the clock afresh from the
     * device.  mppi_set_iteration replays noise and must not move obstacles: it shifts iter0 by the same amount.
     * Needs an obstacle model (MPPI_OBSTACLE_NONE: MPPI_ERR_BAD_ARG); MPPI_MODEL_DIFFDRIVE_MLP: MPPI_ERR_UNSUPPORTED (the
     * message points to value 2).
     * 2 (MPPI_OBSTACLE_MOTION_LEARNED): THE LEARNED MODEL'S SCENE HANDLE.  Accepted with MPPI_MODEL_DIFFDRIVE_MLP only (an
     * analytic model: MPPI_ERR_BAD_ARG, as any unknown value) and, like 1, only with an obstacle model.  A value of its own
     * because value 1 with the learned model has always been refused with MPPI_ERR_UNSUPPORTED and callers probe for that
     * answer: the refusal stays, and a caller that wants the scene says so.  Everything documented for value 1 holds on such
     * a handle with the learned transition in place of the analytic one: the clock and its re-basing, mppi_set_obstacles_moving,
     * mppi_set_obstacle_tracks, mppi_set_cost_grid, mppi_set_cost_grid_footprint, mppi_set_scene_mode and their per-agent forms
     * with their exclusivity rules and their T <= 128 limit, j = t + 1 for the state after step t + 1 of a rollout and j = T
     * for the terminal call, the stage methods (agent 0's scene), mppi_stats.n_collided.  Batched agents keep their own scenes
     * and their own models (mppi_set_agent_mlp).  Limits, each MPPI_ERR_UNSUPPORTED: fleet_radius > 0 (the mates' plans are
     * rolled out with analytic dynamics), K_global > K (sharding), and on such a handle the f32-input model cases of
     * mppi_set_mlp (MPPI_MLP_F32=1, weights beyond the f16 range): the scene is priced by the f16-split kernels only, and
     * MPPI_MLP_FORM / MPPI_MLP_TERMS do not apply.  f64 is refused for the learned model as before.  The fleet_radius refusal
     * keeps its answer (callers probe for it) and points to value 3.
     * 3 (MPPI_OBSTACLE_MOTION_LEARNED_FLEET): THE LEARNED MODEL'S FLEET HANDLE, a value-2 handle whose agents see each other.
     * Accepted with MPPI_MODEL_DIFFDRIVE_MLP, n_agents from 2 to 256, fleet_radius > 0, an obstacle model, f32 and K_global = K.
     * Refused before the device is looked for: an analytic model, fleet_radius = 0 or n_agents < 2 (MPPI_ERR_BAD_ARG);
     * n_agents > 256, sharding, f64 (MPPI_ERR_UNSUPPORTED); and whatever a learned batch refuses (the sequential index, the
     * f32-input model cases, more than 512 records per agent).  Everything a value-2 batch takes keeps working: a model per agent
     * or one for all, own circles with velocities, tracks and a grid under the exclusivity rules of the analytic fleet handles
     * (with the mates' plans: mppi_set_scene_mode(MPPI_SCENE_COMPOSED)), mppi_set_fleet_prediction, mppi_get_fleet_plans,
     * mppi_get_agent_circles, mppi_get_fleet_clearance, mppi_run_closed_loop, graph capture, mppi_set_iteration.
     *   MPPI_FLEET_VELOCITY (the default): the mate rows documented at fleet_radius, word for word -- the speed is row 0 of the
     *   mate's nominal sequence, clamped; THE RESIDUAL DOES NOT ENTER the constant-velocity prediction.
     *   MPPI_FLEET_PLAN: point 0 of agent a's plan is its (x, y), point j its position after Euler steps of f + ITS OWN MLP with
     *   rows 0 .. j - 1 of its nominal sequence (control t at step t), clamped where the rollout clamps, in the learned rollout's
     *   own arithmetic -- one launch of one workgroup per agent in front of the rollout launch, inside a captured graph.
     * A library without value 3 refuses it with MPPI_ERR_BAD_ARG whatever the model; MPPI_ABI_VERSION stays 8. */
    int32_t obstacle_motion;
    int32_t reserved0;
    /* Fleet avoidance.  0: off (zero-initialised configs: as before).  > 0: every agent of the handle sees every other agent
     * (its "mates") as a moving circle of this radius, written on the device at the start of every iteration -- no host round
     * trip, no re-upload.  Needs n_agents >= 2 and obstacle_motion = 1 (else MPPI_ERR_BAD_ARG), and with obstacle_motion an
     * obstacle model, an analytic dynamics model (the learned model: obstacle_motion = 3, documented there), T <= 128 and
     * K <= 8192; n_agents <= 256 (more: MPPI_ERR_UNSUPPORTED);
     * negative or non-finite: MPPI_ERR_BAD_ARG.  All of it is refused before the device is looked for.
     * THE MATE ROWS.  At the start of every iteration mppi_run_closed_loop runs, before that iteration's rollout launch, agent
     * b's obstacle table is its own circles (mppi_set_obstacles[_moving] / mppi_set_agent_obstacles[_moving], unchanged, in
     * their order) followed by one circle per mate a = 0 .. n_agents - 1, a != b, ascending: n_obs = m_b + n_agents - 1.  Mate a:
     *   centre     p_a = (x, y) of a's state at the start of the iteration;
     *   threshold  packed as a circle of radius fleet_radius is: (0.5 safety_margin + fleet_radius)^2 for MPPI_OBSTACLE_CIRCLE,
     *              fleet_radius^2 for MPPI_OBSTACLE_OUTLINE;
     *   velocity   v_a = s_a (cos yaw_a, sin yaw_a); diff-drive: s_a = component 0 of row 0 of a's nominal sequence as it
     *              stands at the start of the iteration (what mppi_get_u_prev returns for a), clamped to +-u_max[0]; race car:
     *              s_a = the state's v (x[3]);
     *   prediction the state b reaches after j rollout steps is tested against p_a + v_a (delta_t j), j as for obstacle_motion
     *              (1 .. T stage calls, T terminal call): constant velocity from NOW, not from an upload time.
     * p_a, s_a, cos and sin are evaluated in f64 (the state is stored as doubles, u in the handle's precision) and the results
     * rounded to the handle's precision.  A table has one clock -- iter0, the upload time of b's own set -- so the mate row is
     * stored back-dated: with n = iteration_b - iter0_b it holds c = fma(-v, delta_t n, p), and the test's
     * fma(v, delta_t (n + j), c) lands on p + v delta_t j up to the rounding documented for moving circles above (an f32 handle:
     * half an ulp of |v| delta_t n twice; fresh own circles, even an empty set, re-base iter0).
     * b's own circles are priced exactly as on a handle without fleet_radius: own rows, iter0 and the rollout kernel are the
     * same.  Every agent of a fleet handle owns its table (m_b + n_agents - 1 circle rows and as many velocity rows), also
     * where the shared setters gave all agents the same circles: the host writes the own part at a setter, the device the mate
     * part every iteration (k_fleet_rows: one launch in front of the rollout launch, inside a captured graph and inside the
     * first timing bracket of mppi_last_kernel_ms; counted by mppi_get_counters under neither launch class).
     * mppi_eval_is_collided[_at] and mppi_eval_cost see agent 0's scene, its mate rows as of the current states included: the
     * library refreshes the rows before such a call.  mppi_set_state, mppi_set_u_prev and mppi_set_iteration need nothing
     * special: the rows are a pure function of states, nominal controls and clocks, made afresh at the start of an iteration. */
    double fleet_radius;
} mppi_config;

/* per-iteration diagnostics (the reference only prints) */
typedef struct {
    double rho;           /* min_k S */
    double eta;           /* sum_k exp(-beta (S_k - rho)) */
    double ess;           /* effective sample size (sum w)^2 / sum w^2 */
    int32_t idx_start;    /* waypoint index after the x0 call (mppi_differential_drive.py:96) */
    int32_t idx_after;    /* prev_way_point_idx after the iteration */
    int32_t path_end;     /* idx_start reached the last waypoint (:97-99) */
    int32_t rounds;       /* speculation rounds the sequential waypoint mode needed (>= 1) */
    int64_t iteration;    /* iterations completed by this handle */
    int32_t n_collided;   /* samples of the last iteration whose cost carries a collision penalty (`_is_collided`,
                             _obs.py:301-313 / mppi_race_car_obstacle.py:255-274); 0 without obstacles; -1 when the records of
                             other ranks were merged (K sharded: they carry no count) */
    int32_t reserved;
    double iter_us;       /* host wall time per iteration of the call that filled this struct (mppi_step: the call;
                             mppi_run_closed_loop: the call divided by its iterations), microseconds */
    double kernel_us;     /* rollout + merge + finalize kernel time per iteration by HIP events on the launch stream: the
                             average over the window since mppi_enable_timing(h, 1), as of this call; 0 while timing is off */
} mppi_stats;

typedef struct mppi_handle mppi_handle;

/* library level */
int mppi_abi_version(void);
const char *mppi_last_error(const mppi_handle *h); /* h may be NULL: last create() failure */
int mppi_device_count(void);

/* MPPIAlgorithms.__init__ / MPPIRacecarController.__init__ (mppi_differential_drive.py:44-85,
 * mppi_race_car.py:10-52): validates, allocates the workspaces, u_prev = 0, waypoint idx = 0 */
int mppi_create(const mppi_config *cfg, mppi_handle **out);
int mppi_destroy(mppi_handle *h);

/* `self.ref_path` (host, row-major [n, ncols], ncols = 3 (x,y,yaw) or 4 (x,y,yaw,v));
 * re-settable like the attribute (mppi_race_car.py:267) */
int mppi_set_ref_path(mppi_handle *h, const double *path, int32_t n, int32_t ncols);
/* `self.obstacle_circles` (host, [m,3] = x,y,r) */
int mppi_set_obstacles(mppi_handle *h, const double *xyr, int32_t m);
/* The same for ONE agent of a batched handle (mppi_config.n_agents > 1): agent `agent` in [0, n_agents) -- else
 * MPPI_ERR_BAD_ARG -- follows its own `self.ref_path` (mppi_race_car.py:267) / sees its own `self.obstacle_circles`
 * (mppi_differential_drive_obs.py:301-313, mppi_race_car_obstacle.py:255-274); validation and packing are those of the two
 * calls above.  On a batched handle the two calls above set EVERY agent, so a later one returns the batch to a shared scene;
 * an agent with m = 0 beside agents with obstacles collides with nothing.  Every agent needs a path before a run
 * (MPPI_ERR_STATE).  On a single-agent handle agent = 0 is the plain setter. */
int mppi_set_agent_ref_path(mppi_handle *h, int32_t agent, const double *path, int32_t n, int32_t ncols);
int mppi_set_agent_obstacles(mppi_handle *h, int32_t agent, const double *xyr, int32_t m);
/* The two obstacle setters for a handle with mppi_config.obstacle_motion = 1 (on any other handle: MPPI_ERR_STATE): xyr as
 * above and vel (host, [m,2] = vx,vy; metres per second) as the circles stand and move AT THIS CALL -- it sets iter0 to the
 * current iteration counter (see mppi_config.obstacle_motion).  Otherwise the semantics of mppi_set_obstacles /
 * mppi_set_agent_obstacles: the shared set or one agent's own, m = 0 collides with nothing.  Non-finite velocities are
 * MPPI_ERR_BAD_ARG, and a refused call leaves the scene as it was.  On such a handle the static setters above stay valid
 * and mean velocity 0. */
int mppi_set_obstacles_moving(mppi_handle *h, const double *xyr, const double *vel, int32_t m);
int mppi_set_agent_obstacles_moving(mppi_handle *h, int32_t agent, const double *xyr, const double *vel, int32_t m);
/* Per agent: `prev_way_point_idx` / `prev_waypoints_idx` (mppi_differential_drive.py:85) and whether its last x0 call found
 * the last waypoint of ITS path (:97-99, mppi_race_car.py:62-65) -- with paths of different lengths, which agent stopped a
 * call that returned MPPI_ERR_PATH_END.  Host int32_t[n_agents] each, either may be NULL. */
int mppi_get_agent_status(mppi_handle *h, int32_t *idx_out, int32_t *path_end_out);
/*
 * Weights of the residual model `MultiLayerPerceptron` (train/train_diff_mlp.py:13-36), host float arrays in the
 * checkpoint's own layout (saved_models/mlp_diff_300x100_3l.pth): input_layer.weight [H,5], .bias [H];
 * hidden_layer.{0..n_hidden-1}.weight [H,H], .bias [H]; out_layer.weight [3,H], .bias [3].
 * Supported: hidden H in {64, 128, 256, 512} x n_hidden in {1, 2, 3, 4}; anything else is MPPI_ERR_SHAPE, and
 * mppi_last_error names the set.  512 x 3 (the architecture the reference trains, mlp_diff_300x100_3l*.pth) and 512 x 2 (its
 * older checkpoints mlp_diff.pth, mlp_diff_300x100.pth, mlp_diff_300x100_v2.pth) run k_rollout_mlp_h3 (MPPI_MLP_FORM,
 * MPPI_MLP_TERMS, MPPI_MLP_F32 apply); every other shape runs k_rollout_mlp_w<H, ...> (the same arithmetic, H / 64 waves).
 * Numeric range: the default kernels carry weights, inputs and activations as pairs of f16 numbers.  Inputs [x, y, yaw, v, w]
 * and first-layer pre-activations of ANY finite magnitude are handled (per-sample power-of-two scales inside the kernel); a
 * WEIGHT beyond +-65504 cannot be: at 512 x 3 / 512 x 2 such a model is served by the f32-input MFMA kernel instead (about 3x
 * slower, same results to the tolerance of the tests; mppi_last_error then says so and mppi_get_rollout_kernel returns
 * "k_rollout_mlp("); the other shapes have no f32-input kernel and return MPPI_ERR_UNSUPPORTED, as they do with MPPI_MLP_F32=1.
 */
int mppi_set_mlp(mppi_handle *h, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                 const float *const *w_hidden, const float *const *b_hidden, const float *w_out, const float *b_out);
/*
 * The same with the `StandardScaler` statistics the model was trained with (train/train_diff_mlp.py:72-86; values in
 * SURVEY.md App. C): the network then sees (z - in_mean) / in_scale, z = [x, y, yaw, v, w], and its output is taken as
 * y * out_scale + out_mean.  The two affine maps are folded into the first and the last Linear in f64 on the host
 * (W_in / in_scale, b_in - (W_in / in_scale) in_mean; out_scale W_out, out_scale b_out + out_mean), so the kernels are
 * the same.  in_mean / in_scale: 5 doubles, out_mean / out_scale: 3 doubles; a NULL pair means identity.
 */
int mppi_set_mlp_scaled(mppi_handle *h, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                        const float *const *w_hidden, const float *const *b_hidden, const float *w_out, const float *b_out,
                        const double *in_mean, const double *in_scale, const double *out_mean, const double *out_scale);
/*
 * The same two calls for ONE agent of a batched handle (mppi_config.n_agents > 1), with the semantics of the per-agent scene
 * setters: agent `agent` in [0, n_agents) -- else MPPI_ERR_BAD_ARG -- plans with its own residual model, held in buffers the
 * handle owns for it; validation, packing and (mppi_set_agent_mlp_scaled) folding are those of the calls above.  On a
 * batched handle the two calls above set EVERY agent, so a later one returns the batch to one shared model and releases the
 * agents' own copies.  On a single-agent handle agent = 0 is the plain setter.
 * One shape per batch: a launch is one kernel instantiation, so a per-agent model whose (hidden, n_hidden) differs from the
 * shape held by any OTHER agent that has a model is MPPI_ERR_SHAPE (mppi_last_error names both shapes); on a handle where
 * no agent has a model yet the first call fixes the shape; mppi_set_mlp changes the shape of the whole batch.
 * Also refused: a handle of another dynamics model (MPPI_ERR_STATE); a shape outside the supported set (MPPI_ERR_SHAPE);
 * weights beyond the f16 range or MPPI_MLP_F32=1 (MPPI_ERR_UNSUPPORTED: batched handles run the f16-split kernels only).  A
 * call that fails leaves the agent on the model it had.  Every agent needs a model before a run: MPPI_ERR_STATE names the
 * first one without.  Replacing an agent's weights between two mppi_run_closed_loop calls needs no re-capture of a cached
 * graph (MPPI_GRAPH=1): the kernels read the agents' models from a table in device memory.
 * The single-agent entry points a batched handle serves -- mppi_eval_state_transition, and the visualisation rollouts'
 * kernels -- use agent 0's model, as they use agent 0's scene.
 */
int mppi_set_agent_mlp(mppi_handle *h, int32_t agent, int32_t hidden, int32_t n_hidden, const float *w_in, const float *b_in,
                       const float *const *w_hidden, const float *const *b_hidden, const float *w_out, const float *b_out);
int mppi_set_agent_mlp_scaled(mppi_handle *h, int32_t agent, int32_t hidden, int32_t n_hidden, const float *w_in,
                              const float *b_in, const float *const *w_hidden, const float *const *b_hidden, const float *w_out,
                              const float *b_out, const double *in_mean, const double *in_scale, const double *out_mean,
                              const double *out_scale);
/* mutable controller state: `u_prev[T,2]` and `prev_way_point_idx` / `prev_waypoints_idx`
 * (mppi_differential_drive.py:82,:85); host pointers */
int mppi_set_u_prev(mppi_handle *h, const double *u);
int mppi_get_u_prev(mppi_handle *h, double *u);
int mppi_set_waypoint_idx(mppi_handle *h, int32_t idx); /* every agent: idx must lie on every agent's path */
int mppi_get_waypoint_idx(mppi_handle *h, int32_t *idx);

/*
 * One `_calc_input_control` / `_calc_control_input` (mppi_differential_drive.py:87-165,
 * mppi_race_car.py:55-121): sample -> rollout -> cost -> softmin weight -> reduce ->
 * filter -> update -> shift.
 *   x0      host, nx doubles (3 diff / 4 race)                                  [observed_x]
 *   eps     device, float[K,T,2] C-order, or NULL => Philox(seed, iteration)    [`_calc_epsilon`]
 *   u_out   host, double[T,2]: the returned (shifted) sequence                  [`u`, :165]
 *   u0_out  host, double[2]:  the returned first control (pre-shift u[1])       [`u[0]`, :165]
 *   stats   host, nullable
 * Synchronises `stream` before returning (the outputs are host memory).
 */
int mppi_step(mppi_handle *h, const double *x0, const float *eps, double *u_out, double *u0_out,
              mppi_stats *stats, void *stream);

/* The same with the observed state in DEVICE memory (nx doubles, e.g. a float64 CUDA tensor's data_ptr()): a state
 * estimator that already lives on the GPU hands it over without a host round trip. */
int mppi_step_device_x0(mppi_handle *h, const double *x0_device, const float *eps, double *u_out, double *u0_out,
                        mppi_stats *stats, void *stream);

/*
 * Split form for K sharded over ranks.  `begin` runs sample ->
 * rollout -> cost -> local softmin partial and writes this rank's record
 * {rho_g, eta_g, eta2_g, W_g[T,2]} (3 + 2T doubles, mppi_partial_len) to `partial` (device).
 * The caller all-gathers the records over its communicator (RCCL); `end` merges `nranks`
 * records (device, double[nranks, 3+2T]) and finishes the iteration identically on every
 * rank.  x0 == NULL in `begin` takes the state already on the device (closed loop);
 * `end_async` then advances it with the plant and returns without synchronising, and
 * `mppi_sync_result` fetches the outputs of the last finished iteration.
 */
int mppi_partial_len(const mppi_handle *h, int32_t *n_doubles);
int mppi_step_begin(mppi_handle *h, const double *x0, const float *eps, double *partial, void *stream);
int mppi_step_end(mppi_handle *h, const double *partials, int32_t nranks, double *u_out, double *u0_out,
                  mppi_stats *stats, void *stream);
int mppi_step_end_async(mppi_handle *h, const double *partials, int32_t nranks, void *stream);
int mppi_sync_result(mppi_handle *h, double *u_out, double *u0_out, mppi_stats *stats, void *stream);

/*
 * Peer-to-peer form of the same exchange ("direct P2P stores into peers' buffers +
 * flag polling over xGMI" when the collective's latency dominates an iteration).  Every rank owns one
 * exchange buffer in fine-grained device memory; `export` creates it and returns its IPC handle
 * (mppi_comm_handle_bytes() bytes), the caller passes the handles of all ranks around once (any host
 * channel, e.g. torch.distributed.all_gather_object) and `connect` maps them (entries of `local_ptrs`
 * that are non-NULL are used as they are: peers living in the same process, see `mppi_comm_buffer`; such a
 * pointer must be device memory, and when it lives on another GPU `connect` enables peer access to that GPU --
 * MPPI_ERR_UNSUPPORTED when it is not device memory or the two GPUs cannot reach each other).
 * From then on mppi_step and mppi_run_closed_loop exchange the per-rank record inside the finalize
 * kernel: store into every peer's buffer, raise a flag, wait for all flags -- no host call and no
 * collective launch per iteration.  Every rank must make the same sequence of step / closed-loop /
 * probe calls.  A rank that does not arrive within MPPI_EXCHANGE_TIMEOUT_MS (default 3000) makes the
 * call fail with MPPI_ERR_COMM on every rank; `probe` runs one flag round to check the wiring.
 * Needs MPPI_WAYPOINT_FROZEN (as the split form does).
 */
int mppi_comm_handle_bytes(void);
int mppi_comm_export(mppi_handle *h, int32_t nranks, void *handle_out);
int mppi_comm_buffer(mppi_handle *h, void **device_ptr);
int mppi_comm_connect(mppi_handle *h, int32_t rank, int32_t nranks, const void *handles /* [nranks][handle_bytes] */,
                      void *const *local_ptrs /* nullable [nranks] */);
int mppi_comm_probe(mppi_handle *h, void *stream);
int mppi_comm_close(mppi_handle *h);

/*
 * The same exchange carried by RCCL INSIDE the library (`mppi_comm_init(h, ncclUniqueId, rank,
 * nranks)`): rank 0 obtains an id with `mppi_comm_unique_id` (= ncclGetUniqueId, mppi_comm_unique_id_bytes() = 128 bytes),
 * passes it to every rank over any host channel, and every rank calls `mppi_comm_init` (= ncclCommInitRank on the handle's
 * device; collective, blocks until all ranks have called).  From then on mppi_step and mppi_run_closed_loop on that handle
 * enqueue ONE ncclAllGather of the per-rank record (3 + 2T doubles) per iteration between the rollout and the finalize
 * launches, on the caller's stream: a C caller needs no torch.distributed.  A peer-to-peer connection (mppi_comm_connect)
 * takes precedence over it when both exist.  librccl.so.1 is loaded on first use (dlopen), not linked.  Needs
 * MPPI_WAYPOINT_FROZEN; every rank must make the same sequence of calls; `mppi_comm_close` releases the communicator.
 */
int mppi_comm_unique_id_bytes(void);
int mppi_comm_unique_id(void *id_out);
int mppi_comm_init(mppi_handle *h, const void *unique_id, int32_t rank, int32_t nranks);

/* S[K] of the last iteration (`S`, :103) and its weights (`_compute_weight`, :167-180); host doubles */
int mppi_get_costs(mppi_handle *h, double *S);
int mppi_get_weights(mppi_handle *h, double *w);
/* the noise the sampler produces for `iteration` (`_calc_epsilon`, :273-283): device float[K,T,2]
 * ([n_agents,K,T,2] for a batched handle: agent a's tensor follows agent a-1's) */
int mppi_sample_epsilon(mppi_handle *h, int64_t iteration, float *eps_out, void *stream);
/*
 * `_calc_epsilon` materialised for the calls that take no tensor of their own (mppi_run_closed_loop, and mppi_step /
 * mppi_step_begin with eps == NULL): a ring of `n_slots` noise tensors in DEVICE memory, float[n_slots][n_agents][K][T][2];
 * iteration i (the handle's iteration counter, see mppi_set_iteration) reads slot i mod n_slots, picked inside the kernels,
 * so a closed loop on the device replays a recorded noise sequence -- and the rollout reads its noise as coalesced rows from
 * HBM (the reference's second pass over eps, :132-135, stays in registers).  n_slots must be a power of two; the caller owns
 * the ring and keeps it alive; eps_ring == NULL or n_slots == 0 returns to the in-kernel Philox sampler.  A ring filled by
 * mppi_sample_epsilon(h, i, ring + i * n_agents * K * T * 2) for i = 0 .. n_slots-1 reproduces the sampler's run over those
 * iterations bit for bit.
 */
int mppi_set_noise_ring(mppi_handle *h, const float *eps_ring, int32_t n_slots);
/* iteration counter that keys the sampler (checkpoint / resume).  Moving obstacles stay where they are: the clock's origin
 * moves with the counter (see mppi_config.obstacle_motion). */
int mppi_set_iteration(mppi_handle *h, int64_t iteration);

/*
 * The visualisation rollouts of the last iteration (mppi_differential_drive.py:144-159):
 * optimal_traj[T,nx] from the updated u and sampled_traj[K,T,nx] from the clamped v, both
 * with the reference's `[t-1]` control indexing.  Device float buffers, either nullable.
 * MPPI_MODEL_DIFFDRIVE_MLP: the same loop with the learned transition (the rollout kernel's network code, states stored
 * instead of costs).
 */
int mppi_rollout_viz(mppi_handle *h, float *optimal_traj, float *sampled_traj, void *stream);

/*
 * Closed loop on the device: the plant of the reference's driver
 * (DifferentialDrive.update_state mppi_differential_drive.py:33-40 / Vehicle.update
 * models/vehicle.py:85-114) advances the state with the returned control after every
 * iteration, with no host round trip.  `mppi_set_state` seeds it; `mppi_run_closed_loop`
 * runs `n_iters` complete iterations (eps from the sampler) and synchronises once.
 */
int mppi_set_state(mppi_handle *h, const double *x);
int mppi_get_state(mppi_handle *h, double *x);
int mppi_run_closed_loop(mppi_handle *h, int32_t n_iters, double *u0_trace /* host, nullable [n_iters,2] */,
                         mppi_stats *stats, void *stream);

/*
 * The stage methods of the controller classes as batched entry points, evaluated by the device
 * code the rollout kernels use, in the handle's precision.  Host arrays of n items in and out.
 *   mppi_eval_state_transition  `_state_transition` (mppi_differential_drive.py:182-198) / `_F` (mppi_race_car.py:183-197):
 *                               x[n,nx], v[n,2] -> x_next[n,nx]   (no clamping: that is `_g`, mppi_eval_clamp)
 *   mppi_eval_clamp             `_g` (:285-289 / mppi_race_car.py:176-181): v[n,2] -> clamped [n,2]
 *   mppi_eval_is_collided       `_is_collided` (_obs.py:301-313 / mppi_race_car_obstacle.py:255-274): x[n,nx] -> {0,1}[n]
 *   mppi_eval_nearest_waypoint  `_get_nearest_waypoint` (:201-220) / `get_nearest_waypoint` (mppi_race_car.py:157-174)
 *                               for the positions x[n,nx] (columns 0,1), searched from *prev_idx.  update_prev_idx = 1:
 *                               the index threads through the n calls in order, as n successive calls of the reference
 *                               method would, and *prev_idx is left at the last one; 0: every call starts at *prev_idx
 *   mppi_eval_cost              `_compute_cost` / `_c` (terminal = 0), `_terminal_cost` / `_phi` (terminal = 1): the
 *                               weighted tracking error against the nearest waypoint (searched as above) + the
 *                               collision penalty; idx_out (nullable) receives the waypoint index of every call
 *   mppi_eval_moving_average    `_moving_average_filter` in the handle's filter mode: xx[T,2] -> [T,2]
 *   mppi_eval_weights           `_compute_weight` of a given cost vector S[n] with the handle's softmin rate
 */
int mppi_eval_state_transition(mppi_handle *h, const double *x, const double *v, int32_t n, double *x_next);
int mppi_eval_clamp(mppi_handle *h, const double *v, int32_t n, double *out);
int mppi_eval_is_collided(mppi_handle *h, const double *x, int32_t n, double *out);
/* `_is_collided` of pose i against the circles steps[i] >= 0 rollout steps ahead of the current obstacle clock (host
 * int32_t[n]; see mppi_config.obstacle_motion: steps[i] = j of the rollout).  mppi_eval_is_collided and mppi_eval_cost price
 * at step 0 of the current clock.  On a handle without obstacle motion the steps change nothing. */
int mppi_eval_is_collided_at(mppi_handle *h, const double *x, int32_t n, const int32_t *steps, double *out);
/* The circles agent `agent`'s next iteration will test, own set first, then its mates: host xyr_out [cap][3] = centre as of
 * rollout step 0 of the current clock and the RADIUS r (threshold unpacked), vel_out [cap][2]; *m_out = the number the agent
 * has (written even when cap is too small: MPPI_ERR_SHAPE then).  Any handle with an obstacle model (none: MPPI_ERR_STATE;
 * agent outside [0, n_agents): MPPI_ERR_BAD_ARG); what a planner's visualisation draws, and what the tests read.  The values
 * are the table's own, in the handle's precision: centre = fma(v, delta_t n, c) as the kernels form it at j = 0. */
int mppi_get_agent_circles(mppi_handle *h, int32_t agent, double *xyr_out, double *vel_out, int32_t cap, int32_t *m_out);
/* Fleet handles (else MPPI_ERR_STATE): per agent, over the iterations run since mppi_create or the last call with reset != 0,
 * min_dist[a] = the smallest centre distance to any mate among the states those iterations started from (f64; +inf: none ran),
 * contact_iters[a] = how many of them started with that distance < 2 * fleet_radius.  Host arrays [n_agents], either nullable.
 * (A closed-loop call of many iterations returns only the last state: this says whether two robots touched in between.  The
 * refreshes in front of mppi_eval_* and mppi_get_agent_circles are not counted.) */
int mppi_get_fleet_clearance(mppi_handle *h, double *min_dist, int64_t *contact_iters, int32_t reset);
/* How a fleet handle (mppi_config.fleet_radius > 0) predicts an agent's mates along the horizon, switched at run time.
 * MPPI_FLEET_VELOCITY (the default): constant velocity from the mate rows, as documented at mppi_config.fleet_radius, bit for
 * bit what a handle gives that never called this.  MPPI_FLEET_PLAN: every mate is predicted along its own planned trajectory.
 * THE PLANS.  At the start of every iteration mppi_run_closed_loop runs -- the moment the mate rows are written in velocity mode
 * -- the plan of agent a is
 *   P_a[0] = (x, y) of a's state;
 *   P_a[j], j = 1 .. T: the position after the model's Euler steps with rows 0 .. j - 1 of a's nominal sequence as it stands then
 *           (what mppi_get_u_prev returns for a), clamped to +-u_max exactly where the rollout clamps (mppi_config.clamp_rollout).
 * Both models (unicycle, bicycle), in the handle's precision R from the state rounded to R: the arithmetic of the rollout itself
 * at zero noise for an exploiting sample (prefix sums over the horizon in R), so P_a is the trajectory a's own iteration prices
 * as its nominal one.  The state agent b reaches after j rollout steps is tested against P_a[j] for every a != b, with the
 * threshold a mate has in velocity mode ((0.5 safety_margin + fleet_radius)^2 for MPPI_OBSTACLE_CIRCLE, fleet_radius^2 for
 * MPPI_OBSTACLE_OUTLINE -- there against the nearest of the outline points as the race-car kernels fold them, for both
 * models); j = 1 .. T for the stage calls, T for the terminal call, 0 for what prices "now".  A plan has no clock and is not
 * back-dated: it is made from now.  b's own circles (static or moving) are priced exactly as on the same handle in velocity
 * mode: own rows, iter0, the same arithmetic.  In plan mode an agent's table is its own rows alone (n_obs = m_b:
 * mppi_get_agent_circles returns the own circles only); an agent without circles of its own still prices its mates and counts
 * them in mppi_stats.n_collided.  One launch (k_fleet_plan) takes the place of k_fleet_rows at the front of every slot, inside a
 * captured graph and inside the first timing bracket, and keeps the clearance record (mppi_get_fleet_clearance: unchanged in
 * meaning).  mppi_eval_is_collided[_at] and mppi_eval_cost see agent 0's own circles and its mates' plans, refreshed first;
 * mppi_eval_is_collided_at refuses a step outside [0, T] (MPPI_ERR_BAD_ARG).
 * Like every setter this synchronises, re-uploads the scenes and drops a cached graph.  NULL handle or unknown mode:
 * MPPI_ERR_BAD_ARG; a handle without fleet_radius > 0: MPPI_ERR_STATE.  Limits: those of fleet handles. */
#define MPPI_FLEET_VELOCITY 0
#define MPPI_FLEET_PLAN 1
int mppi_set_fleet_prediction(mppi_handle *h, int32_t mode);
/* Plan mode (else MPPI_ERR_STATE): every agent's plan, host xy [n_agents][T + 1][2], made afresh from the current states and
 * nominal controls before it is read back (the values are the table's own, in the handle's precision; the refresh does not
 * count for the clearance record). */
int mppi_get_fleet_plans(mppi_handle *h, double *xy);
/* OBSTACLE TRACKS: obstacles that an outside predictor delivers as a list of positions, one per control step, instead of
 * {centre, velocity}.  The setters work on a handle created with obstacle_motion = 1 (any other: MPPI_ERR_STATE).
 * THE TRACKS.  xy is [n][L][2]: point i of track m, xy[m][i], is the centre of obstacle m i control steps (delta_t each) after
 * this call; radius[m] is its radius.  The points are stored rounded to the handle's precision R with no other arithmetic, so
 * what the device tests is R(xy) exactly.
 * THE CLOCK is that of the moving circles: the setter records iter0 = the handle's iteration counter in a word of the set's own
 * (the circles' iter0 is untouched), and with c = iteration - iter0 the state a rollout reaches after j steps is tested against
 * point min(c + j, L - 1) of every track; j = 1 .. T for the stage calls, T for the terminal call, 0 for what prices "now".  A
 * track holds its last point once it runs out; a track of L = 1 is a static circle.  One iteration is one tick, speculation
 * rounds share it, mppi_run_closed_loop and a replayed graph read the clock on the device.  mppi_set_iteration shifts the
 * tracks' iter0 with the circles' (the clock does not move); a fresh upload re-bases it.
 * THE TEST.  Every track has a threshold of its own, packed from radius[m] exactly as a circle of that radius is packed:
 * (0.5 safety_margin + r)^2 for MPPI_OBSTACLE_CIRCLE, r^2 for MPPI_OBSTACLE_OUTLINE -- there against the nearest of the outline
 * points as the race-car kernels fold them, for both models.  The handle's own circles, static or moving, are priced exactly as
 * before, beside the tracks; a handle may have tracks and no circles.  A sample that hits a track counts in
 * mppi_stats.n_collided.  mppi_eval_is_collided[_at] and mppi_eval_cost see agent 0's tracks; any step >= 0 is valid there.
 * n = 0 removes the set: the handle is then bit for bit the handle that never called the setter.
 * BATCHES.  mppi_set_obstacle_tracks gives every agent the same set (and takes back what the agent setter gave);
 * mppi_set_agent_obstacle_tracks gives one agent a set of its own.  Sets may differ in n and L, and an agent may have none: the
 * semantics of mppi_set_obstacles / mppi_set_agent_obstacles.
 * REFUSALS leave the scene as it was.  NULL handle, NULL xy or radius with n > 0, a non-finite point, a non-finite or negative
 * radius, an agent outside [0, n_agents): MPPI_ERR_BAD_ARG.  n outside [0, 256], L outside [1, 65536] (n > 0): MPPI_ERR_SHAPE.
 * A fleet handle (fleet_radius > 0: its plan mode uses the same parameter words) or a horizon T > 128 (the unfused rollout):
 * MPPI_ERR_UNSUPPORTED.  Like every setter this synchronises and drops a cached graph. */
int mppi_set_obstacle_tracks(mppi_handle *h, const double *xy, const double *radius, int32_t n, int32_t L);
int mppi_set_agent_obstacle_tracks(mppi_handle *h, int32_t agent, const double *xy, const double *radius, int32_t n, int32_t L);
/* The centres and radii agent `agent` tests at rollout step `step` >= 0 of the current clock: xyr_out [cap][3] receives
 * {R(xy)[m][min(c + step, L - 1)], radius[m]} for its n tracks (for visualisation and tests).  *n_out is written even when cap
 * is too small (MPPI_ERR_SHAPE then). */
int mppi_get_obstacle_tracks_at(mppi_handle *h, int32_t agent, int32_t step, double *xyr_out, int32_t cap, int32_t *n_out);
/* COST GRIDS: a costmap -- a lidar or occupancy grid, inflated -- priced along every rollout by bilinear lookup, whatever the
 * scene holds.  The setters work on a handle created with obstacle_motion = 1 (any other: MPPI_ERR_STATE).
 * STORAGE.  cells is a host array [ny][nx], row-major: cells[iy][ix] is the value at the world point (origin_x + ix resolution,
 * origin_y + iy resolution).  Cells, origin, inv = 1 / resolution (divided in double), weight and lethal are stored rounded once
 * to the handle's precision R; nothing else is kept.
 * THE VALUE at a state's position (x, y), all in R:
 *     gx = fmin(fmax((x - ox) inv, 0), nx - 1);   ix = min((int)gx, nx - 2);   fx = gx - ix;        (the same for y)
 *     c0 = fma(fx, G[iy][ix+1]   - G[iy][ix],   G[iy][ix]);
 *     c1 = fma(fx, G[iy+1][ix+1] - G[iy+1][ix], G[iy+1][ix]);
 *     g  = fma(fy, c1 - c0, c0)
 * A node returns its cell exactly (the last node of an axis, where ix = nx - 2 and fx = 1: a + (b - a), the cell to one rounding
 * of the difference); outside the grid the edge value continues; a non-finite coordinate lands on an edge node (NaN: node 0 of
 * its axis); every read stays inside the table whatever the state is.
 * PRICING.  Wherever the handle adds the collision penalty -- every stage call it prices, and the terminal call -- the state's
 * cost also gains weight g, and the state counts as hit when g >= lethal or a circle says so.  With accumulate_stage_cost = 0
 * the last state is therefore priced twice, as the penalty is.  lethal = +inf: soft cost only.  mppi_stats.n_collided keeps its
 * definition (S >= collision_penalty); an agent with a grid and no circles counts its hits.  Both dynamics models sample the
 * state's (x, y) only (no footprint; mppi_set_cost_grid_footprint below adds the outline).  The handle's circles, static or moving, are priced exactly as before, beside the grid.
 * The grid has no clock: it stands until replaced.  cells == NULL or nx == 0 removes it: the handle is then bit for bit the
 * handle that never called the setter.  A re-upload of the same nx x ny reuses the buffers and keeps a cached graph
 * (MPPI_GRAPH=1): the rolling-costmap loop; origin, resolution, weight and lethal may change with it.
 * BATCHES.  mppi_set_cost_grid gives every agent the same grid (and takes back what the agent setter gave);
 * mppi_set_agent_cost_grid gives one agent a grid of its own, of any shape, or (cells == NULL) none.
 * mppi_eval_cost, mppi_eval_is_collided and mppi_eval_is_collided_at include agent 0's grid.
 * REFUSALS leave the scene as it was.  A handle that has obstacle tracks: MPPI_ERR_STATE (and the track setters refuse a
 * handle that has a grid: both use the same parameter words).  A fleet handle (fleet_radius > 0) or a horizon T > 128 (the
 * unfused rollout): MPPI_ERR_UNSUPPORTED.  nx or ny outside [2, 4096], a non-finite cell or origin, resolution not finite
 * or not > 0, weight not finite or < 0, lethal NaN or <= 0, an agent outside [0, n_agents), a NULL handle: MPPI_ERR_BAD_ARG.
 * Like every setter this synchronises. */
int mppi_set_cost_grid(mppi_handle *h, const double *cells, int32_t nx, int32_t ny, double origin_x, double origin_y,
                       double resolution, double weight, double lethal);
int mppi_set_agent_cost_grid(mppi_handle *h, int32_t agent, const double *cells, int32_t nx, int32_t ny, double origin_x,
                             double origin_y, double resolution, double weight, double lethal);
/* The raw value g of agent `agent`'s grid at n points xy [n][2], from the device function the rollout prices with (for
 * visualisation and tests).  An agent without a grid: MPPI_ERR_STATE. */
int mppi_eval_cost_grid(mppi_handle *h, int32_t agent, const double *xy, int32_t n, double *value);
/* COST GRID FOOTPRINT: price the vehicle's outline against the grid, not only its centre.
 * THE MODE belongs to the handle: one for every agent, kept across grid uploads and removals; it may be set before any grid
 * exists.  A handle that never calls the setter, or sets MPPI_GRID_FOOTPRINT_CENTRE, is bit for bit the handle described
 * above: the same launches, the same answer of mppi_get_rollout_kernel, the same outputs.
 * THE POINTS.  In MPPI_GRID_FOOTPRINT_OUTLINE nine body-frame points q = 0 .. 8 are sampled wherever the handle prices a grid:
 * q = 0 the centre (0, 0), q = 1 .. 8 the outline the collision test uses -- with a = 0.5 vehicle_l safety_margin and
 * b = 0.5 vehicle_w safety_margin: (-a, 0), (-a, b), (0, b), (a, b), (a, 0), (a, -b), (0, -b), (-a, -b), each rounded once to
 * the handle's precision R.  The world point of (qx, qy), all in R, with {sn, cs} the kernels' own sincos of the state's yaw --
 * the yaw the collision test uses, unwrapped --:
 *     px = fma(qx, cs, fma(-qy, sn, x));        py = fma(qx, sn, fma(qy, cs, y))
 * (two roundings per coordinate; the offset joins the first product).  The centre is the state's (x, y) itself.
 * THE VALUE.  g_foot = fmax over q of g(p_q), g the bilinear formula above, folded in the order q = 0, 1, .. 8.
 * PRICING.  Everything said above about pricing holds with g replaced by g_foot: the cost gains weight g_foot wherever the
 * penalty is added (the terminal call too, so twice with accumulate_stage_cost = 0), the state is hit when g_foot >= lethal or
 * any other ingredient says so, mppi_stats.n_collided keeps its definition, and every read stays inside the table whatever the
 * state is (a NaN or infinite yaw or position lands on edge nodes).  Composed scenes price their grid the same way.
 * mppi_eval_is_collided[_at] and mppi_eval_cost follow the mode, using the pose's yaw column; mppi_eval_cost_grid stays the raw
 * centre value.  Both dynamics models: MPPI_OBSTACLE_OUTLINE with the diff-drive model is a rectangular AGV.
 * REFUSALS name their limit in mppi_last_error and change nothing.  NULL handle (or NULL mode of the getter): MPPI_ERR_BAD_ARG,
 * before anything else.  An unknown mode: MPPI_ERR_BAD_ARG.  A handle created with obstacle_motion = 0: MPPI_ERR_STATE.
 * MPPI_GRID_FOOTPRINT_OUTLINE on a handle whose obstacle_model is not MPPI_OBSTACLE_OUTLINE: MPPI_ERR_UNSUPPORTED (a disc is
 * served by inflating the map by its radius), and on a horizon T > 128: MPPI_ERR_UNSUPPORTED.  MPPI_GRID_FOOTPRINT_CENTRE is
 * accepted on any handle that has obstacle_motion.  The setter synchronises; a call that changes the mode drops a cached graph,
 * one that does not changes nothing.  In either mode a re-upload of a grid of the same shape keeps a cached graph. */
#define MPPI_GRID_FOOTPRINT_CENTRE  0   /* default: the state's (x, y), as documented at mppi_set_cost_grid */
#define MPPI_GRID_FOOTPRINT_OUTLINE 1
int mppi_set_cost_grid_footprint(mppi_handle *h, int32_t mode);
int mppi_get_cost_grid_footprint(const mppi_handle *h, int32_t *mode);
/* g_foot of agent `agent`'s grid at n poses pose [n][3] = x, y, yaw, and -- points not NULL -- the nine world points
 * points [n][9][2], from the device function the rollout prices with, in either mode (for visualisation and tests).  An agent
 * without a grid: MPPI_ERR_STATE. */
int mppi_eval_cost_grid_footprint(mppi_handle *h, int32_t agent, const double *pose, int32_t n, double *value, double *points);
/* ---- composed scenes: fleet plans, obstacle tracks and a cost grid on one handle ----
 * By default (MPPI_SCENE_EXCLUSIVE) the mates' plans, the obstacle tracks and the cost grid exclude each other on a handle, as
 * the three setters document: a handle that never calls this behaves bit for bit as before, refusals and messages included.
 * MPPI_SCENE_COMPOSED lifts exactly those cross-refusals: a grid beside tracks, and tracks or a grid on a fleet handle (in
 * either prediction mode).  Every other refusal of mppi_set[_agent]_cost_grid, mppi_set[_agent]_obstacle_tracks and
 * mppi_set_fleet_prediction stays, with its code and text.
 * SEMANTICS.  Nothing new is defined: every ingredient keeps what its setter documents -- the tracks their own clock and their
 * last point, the grid its formula and `lethal`, the plans their thresholds, the handle's circles their pricing -- and a state
 * counts as hit when ANY of them says so; its cost gains weight g wherever the penalty is added.  mppi_stats.n_collided keeps
 * its definition.  mppi_eval_is_collided[_at] and mppi_eval_cost see all of agent 0's ingredients; mppi_eval_is_collided_at
 * refuses a step outside [0, T] only when the mates' plans are among them.  The getters answer as on the exclusive handles.
 * COST.  A composed handle that holds at most one of {plan mode, tracks on some agent, a grid on some agent} runs the very
 * launch the exclusive handle runs (bit for bit); with two or more it runs the composed rollout form, which carries all of
 * them.  Removing ingredients returns the handle to the single-ingredient forms.
 * ACCEPTED on a handle created with obstacle_motion = 1 (any other: MPPI_ERR_STATE) whose horizon is T <= 128 (longer:
 * MPPI_ERR_UNSUPPORTED).  A NULL handle or an unknown mode: MPPI_ERR_BAD_ARG.  Switching back to MPPI_SCENE_EXCLUSIVE while
 * the handle holds more than one of the three: MPPI_ERR_STATE, the message names what is held, nothing changes.  In
 * MPPI_SCENE_EXCLUSIVE mppi_set_fleet_prediction(MPPI_FLEET_PLAN) refuses (MPPI_ERR_STATE) a handle that holds tracks or a
 * grid -- which only a handle that was composed before can.  Like every setter this synchronises; a switch drops a cached
 * graph. */
#define MPPI_SCENE_EXCLUSIVE 0   /* default: plans, tracks and a grid exclude each other, as documented */
#define MPPI_SCENE_COMPOSED  1
int mppi_set_scene_mode(mppi_handle *h, int32_t mode);
int mppi_get_scene_mode(const mppi_handle *h, int32_t *mode);
int mppi_eval_nearest_waypoint(mppi_handle *h, const double *x, int32_t n, int32_t *prev_idx, int32_t update_prev_idx,
                               int32_t *idx_out);
int mppi_eval_cost(mppi_handle *h, int32_t terminal, const double *x, int32_t n, int32_t *prev_idx, int32_t update_prev_idx,
                   double *cost, int32_t *idx_out);
int mppi_eval_moving_average(mppi_handle *h, const double *xx, double *out);
int mppi_eval_weights(mppi_handle *h, const double *S, int32_t n, double *w);

/* Kernel durations by HIP events on the launch stream.  While enabled, every launch group of every
 * iteration is bracketed by an event pair, plus one empty pair that calibrates the cost of the
 * bracketing itself.  mppi_last_kernel_ms: averages (ms) over the window since timing was enabled,
 * calibration subtracted: out[0] rollout+cost(+fused softmin partial; a fleet handle: + its k_fleet_rows launch), out[1] separate reduce / merge
 * launches (0 when fused), out[2] finalise, out[3] the empty-pair calibration itself. */
int mppi_last_kernel_ms(mppi_handle *h, float *out4);
int mppi_enable_timing(mppi_handle *h, int32_t on);
/* Measurement aid: launch the rollout kernel `n` >= 1 times per iteration (it is idempotent -- same
 * state in, same S / partial records out).  The growth of the iteration period per extra launch is that
 * kernel's launch-to-launch duration on the stream, free of any event overhead (bench.py). */
int mppi_set_rollout_repeats(mppi_handle *h, int32_t n);
/* Launch bookkeeping since mppi_create (host side): out3 = {iterations completed, rollout-class kernel launches
 * (the repeats of mppi_set_rollout_repeats included), finalize launches}.  An iteration of the sequential waypoint
 * mode may take several of each (speculation rounds); bench.py divides a measured time by these. */
int mppi_get_counters(mppi_handle *h, int64_t *out3);

/* Host side of mppi_run_closed_loop since mppi_create (seconds, cumulative): out2 = {time spent ENQUEUEING the launches,
 * time inside the calls}.  A loop the host cannot feed fast enough shows enqueue ~ whole call; bench.py reports the ratio
 * (`host_enqueue_share`), because the iteration's 9 us leave a host that needs ~3 us per launch little slack. */
int mppi_get_host_timing(const mppi_handle *h, double *out2);

/* Launch-to-launch duration of the rollout kernel on the GPU with the host out of the loop (bench.py's `roofline.kernel_us`):
 * `n_slots` closed-loop iterations are captured into a HIP graph as they are and with the (idempotent) rollout kernel
 * launched 1 + `extra` times per iteration, each replayed four times between two events; us_out2 = {microseconds one more
 * launch of the kernel costs, microseconds per iteration of the plain graph}.  The iterations are real ones (the state
 * advances).  Needs a waypoint index that cannot move (frozen mode, or the end of the path) and no rank exchange. */
int mppi_time_rollout_launch(mppi_handle *h, int32_t n_slots, int32_t extra, void *stream, double *us_out2);

/* Which fused rollout kernel serves the handle (fixed at mppi_create from K x n_agents and T; diagnostic, for tests and
 * profiles): low two bits 0 = one sample per wave, lanes over the horizon; 1 = two samples per wave, two steps per lane
 * (T <= 64 and >= 8192 samples per launch); 2 = one sample per wave, two steps per lane (64 < T <= 128); 3 = two samples per
 * wave, three steps per lane (the race car as the reference runs it, f32, 64 < T <= 96);
 * +4 = every (half-)wave rolls out two samples in sequence.  -1: the handle does not use the fused kernels. */
int mppi_get_rollout_layout(const mppi_handle *h, int32_t *layout);
/* The kernel instantiation the handle's last rollout-class launch took, spelled as rocprofv3 prints it (e.g.
 * "k_rollout_fused<float, 0, 1, false, 2, false>", "k_rollout_dual<float, 1, 1, false, 2, true>"): bench.py looks the
 * launch's counter figures up under this name in profiles/.  A learned-dynamics handle answers as soon as mppi_set_mlp has
 * run: "k_rollout_mlp_h3<false, 8, 2, 3>" (operands as two f16 halves, the default) or "k_rollout_mlp(" (f32-input MFMA: chosen by
 * MPPI_MLP_F32=1, or by mppi_set_mlp itself when a weight exceeds the f16 range) for 512 x 3 and 512 x 2;
 * "k_rollout_mlp_w<H, false>" for every other shape. */
int mppi_get_rollout_kernel(const mppi_handle *h, char *buf, int32_t n);

/*
 * `pytorch_mppi`-style MPPI with built-in dynamics / running-cost models: the callbacks the
 * reference's test/test_mppi.py, test/test_mppi_diff.py, test/test_mppi_diff_dyna.py,
 * train/bullet_mppi_differential_drive.py, test/test_mppi_racecar.py, test/test_torch_mppi_race_car.py and
 * test/test_torch_mppi.py hand to `pytorch_mppi.MPPI`, as selectable device functions.  `mppi_cb_command`
 * is `MPPI.command(state)`: shift the nominal sequence, sample, roll out, weigh, update, return the first action.
 * The library itself is absent from the build container and un-pinned by the reference: the loop follows the
 * published algorithm and is PARITY UNPINNED (csrc/mppi_cb.hip, oracle/mppi_cb_oracle.py).  fp32 like the callers.
 */
typedef enum {
    MPPI_CB_DYN_UNICYCLE = 0,   /* test/test_mppi.py:12-26: [x, y, theta], [v, omega] */
    MPPI_CB_DYN_SKID_STEER = 1, /* test/test_mppi_diff_dyna.py:13-40: [x, y, theta, v, omega], 4 wheel forces */
    /* The three below step every component by Euler from the OLD state, in the order written, dt from the config.
     * test/test_mppi_racecar.py:13-30, [x, y, theta, v], u = [steer delta, accel a], default dt 0.05:
     *   x += v cos(theta) dt; y += v sin(theta) dt; theta += v / L * tan(delta) * dt; v += a dt;   model_params = {L = 0.3} */
    MPPI_CB_DYN_RACECAR = 2,
    /* test/test_torch_mppi_race_car.py:7-39, [x, y, theta, v], u = [acc, steer delta] -- the other order --, default dt 0.05:
     *   alpha_f = atan2(v sin(delta) + l_f theta, v cos(delta)) - delta;  alpha_r = atan2(v sin(delta) - l_r theta, v cos(delta));
     *   x, y as above; theta += (v / l_r) sin(delta) dt; v += (acc - (C_f alpha_f sin(delta) + C_r alpha_r) / m) dt;
     * model_params = {l_r = 1.5, l_f = 1.0, m = 1000, C_f = 1000, C_r = 1000}.  The script puts the yaw theta where a yaw rate
     * would be expected (:25-26); that is the caller's model and it is restated as it stands. */
    MPPI_CB_DYN_RACECAR_DYNAMIC = 3,
    /* test/test_torch_mppi.py:5-15, [p, v], u = [force], default dt 0.1: p += dt v; v += dt u (the script's A and B) */
    MPPI_CB_DYN_DOUBLE_INTEGRATOR = 4
} mppi_cb_dynamics;
typedef enum {
    MPPI_CB_OBS_INVERSE = 0,     /* 1 / (d + 1e-6) inside the safety distance (test/test_mppi.py:40-50) */
    MPPI_CB_OBS_EXPONENTIAL = 1  /* exp(-(d - safety)), obstacles moving with the step index (test/test_mppi_diff.py:25-52) */
} mppi_cb_obstacle_cost;
typedef struct {
    int32_t struct_size, device;
    int32_t dynamics;            /* mppi_cb_dynamics: fixes nx (3 / 5 / 4 / 4 / 2) and nu (2 / 4 / 2 / 2 / 1) */
    int32_t obstacle_kind;       /* mppi_cb_obstacle_cost */
    int32_t K, T;                /* num_samples, horizon (T * nu <= 256) */
    int32_t n_obs;               /* <= 16 */
    int32_t sample_null_action;  /* the last sample applies the zero action (test_mppi_diff_dyna.py:338) */
    double dt, lambda_;
    double noise_sigma[16];      /* row-major, leading nu x nu block of a 4 x 4; symmetric (both triangles are compared) positive definite */
    double u_min[4], u_max[4], u_init[4];
    double goal[5], q_diag[5], r_diag[4];
    double obstacles[64];        /* [n_obs][4] = x, y, vx, vy (per step of the horizon) */
    double safety_distance, obstacle_weight;
    double skid_params[5];       /* m, I, r, L, damping (2.0, 0.05, 0.1, 0.4, 0.1 in the reference) */
    uint64_t seed;
    /* --- grown at the end; struct_size tells a library that knows these fields from one that does not --- */
    double model_params[8];      /* constants of the model chosen by `dynamics` (see the enum); a non-positive L, l_r or m:
                                    MPPI_ERR_BAD_ARG */
    /* `terminal_state_cost` (test/test_torch_mppi.py:23-25): terminal_cost != 0 adds (s_T - terminal_goal)^T diag(terminal_q)
     * (s_T - terminal_goal), s_T the state after the last step, once per sample, to the sum of its running costs before the
     * perturbation term; 0 leaves the rollout as it was. */
    int32_t terminal_cost;
    /* `noise_abs_cost`: the perturbation term is lambda sum_t sum_i U[t,i] sum_j |noise[t,j]| Sigma^-1[j,i], the absolute
     * value taken of the noise after clamping; the update keeps the signed noise. */
    int32_t noise_abs_cost;
    double terminal_goal[5], terminal_q[5];
    double noise_mu[4];          /* `noise_mu`: the in-kernel draw is mu + L z; an injected eps stands for the whole draw */
    /* `u_scale`, finite and not 0 (else MPPI_ERR_BAD_ARG; 1 is the neutral value): dynamics and running cost see u_scale * the
     * clamped perturbed action; bounds, perturbation term, update and returned action are in unscaled units;
     * mppi_cb_nominal_trajectory and mppi_cb_top_trajectories apply it, as the callers' `self.u_scale * self.U[t]` does
     * (test/test_mppi_racecar.py:73, :83). */
    double u_scale;
} mppi_cb_config;
typedef struct mppi_cb_handle mppi_cb_handle;
const char *mppi_cb_last_error(const mppi_cb_handle *h);
int mppi_cb_create(const mppi_cb_config *cfg, mppi_cb_handle **out);
int mppi_cb_destroy(mppi_cb_handle *h);
/* the nominal control sequence `U` [T, nu] (host) */
int mppi_cb_set_nominal(mppi_cb_handle *h, const double *U);
int mppi_cb_get_nominal(mppi_cb_handle *h, double *U);
/* state: host [nx]; eps: device float [K, T, nu] or NULL (Philox); action_out: host [nu] */
int mppi_cb_command(mppi_cb_handle *h, const double *state, const float *eps, int32_t shift_nominal_trajectory,
                    double *action_out, void *stream);
/* `cost_total` [K] and the weights `omega` [K] of the last command (either nullable) */
int mppi_cb_get_costs(mppi_cb_handle *h, double *cost_total, double *omega);
/* the callbacks themselves, batched: what = 0 `dynamics(states, actions, t)` -> [n, nx]; 1 `running_cost` -> [n];
 * 2 `terminal_state_cost(states)` -> [n] (actions ignored and may be NULL; a handle without one: MPPI_ERR_STATE) */
int mppi_cb_eval(mppi_cb_handle *h, int32_t what, const double *states, const double *actions, int32_t t, int32_t n,
                 double *out);
/* the trajectory U drives from `state`: [T, nx] (the optimal trajectory of the callers' get_trajectories) */
int mppi_cb_nominal_trajectory(mppi_cb_handle *h, const double *state, double *traj);
/* The handle keeps the nominal sequence the last command's samples were drawn around (after the shift, before the update) and
 * that command's iteration number, so the two calls below make its draw again: from Philox (eps NULL), or from the injected
 * tensor handed in again (eps, device float [K, T, nu]).  Before the first command, or with eps where the last command drew
 * in the kernel and the other way round: MPPI_ERR_STATE.
 * `perturbed_action` (test/test_mppi_racecar.py:83): the clamped, unscaled actions of the last command, host [K][T][nu]. */
int mppi_cb_get_perturbed_actions(mppi_cb_handle *h, const float *eps, double *out);
/* The callers' sampled fan (test/test_mppi_racecar.py:76-84, test/test_mppi.py:60-80): the trajectories from `state` of the n
 * samples with the lowest `cost_total` of the last command, in ascending order -- host traj_out [n][T][nx] -- and their
 * sample indices, host index_out [n].  The rank of sample k is the number of samples j with c_j < c_k, or c_j == c_k and
 * j < k; a NaN cost counts as larger than every number and NaNs are ordered among themselves by index, so the ranks are a
 * permutation of 0 .. K - 1 whatever the costs hold (a stable ascending argsort).  n outside [1, K]: MPPI_ERR_SHAPE. */
int mppi_cb_top_trajectories(mppi_cb_handle *h, const double *state, const float *eps, int32_t n, double *traj_out,
                             int32_t *index_out);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_HIP_H */
