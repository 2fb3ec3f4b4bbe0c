/*
 * topay.h — C-ABI of the MI355X-native batched (s,theta) trajectory optimizer.
 *
 * Drop-in boundary for ONE hot path of TopAY-Planner/TopAY: `MomaTrajOpt::optimizeTraj`
 * (reference: src/planner/src/moma_traj_opt.cpp:142-498) and what it calls per L-BFGS
 * iteration.  The reference exposes an in-process C++ class, one instance per candidate
 * thread (src/planner/include/planner/moma_traj_opt.h:613-674); this ABI is the same surface,
 * batch-first: one context optimises `batch` independent candidate trajectories at once,
 * one 64-lane wavefront per trajectory, on one GPU.
 *
 *   reference member                                   replaced by
 *   -------------------------------------------------  ------------------------------------
 *   MomaTrajOpt(GridMap::Ptr)        moma_traj_opt.h:651   topay_create + topay_set_map
 *   init(ros::NodeHandle&)           moma_traj_opt.h:845   topay_default_params / topay_create
 *   optimizeTraj(...) lines 146-357  moma_traj_opt.cpp     topay_set_init_traj
 *   optimizeTraj(...) lines 359-497  moma_traj_opt.cpp     topay_optimize
 *   getTraj(), traj_cost             moma_traj_opt.h:943   topay_get_result
 *   first/secondStageCostCallback    moma_traj_opt.cpp:817,885   topay_eval (test hook)
 *   printConstraintsSituations       moma_traj_opt.h:1052  topay_check_feasible
 *
 * Conventions: plain pointers and sizes, no C++/torch types, never throws.  Every call
 * returns a topay_status (0 = ok).  A context is single-caller (like one MomaTrajOpt); several
 * contexts may coexist (one per GPU / process).  All host buffers are caller-owned and copied;
 * the context owns its device memory.  Arithmetic is IEEE double throughout.
 */
#ifndef TOPAY_H
#define TOPAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int topay_status;
enum {
  TOPAY_OK = 0,
  TOPAY_ERR_INVALID_ARG = -1,
  TOPAY_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error; see topay_last_error() */
  TOPAY_ERR_NO_MAP = -3,
  TOPAY_ERR_NO_TRAJ = -4,
  TOPAY_ERR_TOO_MANY_PIECES = -5,
  TOPAY_ERR_UNSUPPORTED = -6
};

/* Per-trajectory solver status (reported by topay_get_result / topay_get_stats).  Values >= -1024
 * are the reference's L-BFGS codes (src/planner/include/utils/lbfgs.hpp:135-184). */
enum {
  TOPAY_LBFGS_CONVERGENCE = 0,
  TOPAY_LBFGS_STOP = 1,
  TOPAY_LBFGS_CANCELED = 2,
  TOPAY_LBFGSERR_INVALID_FUNCVAL = -1012,
  TOPAY_LBFGSERR_MINIMUMSTEP = -1011,
  TOPAY_LBFGSERR_MAXIMUMSTEP = -1010,
  TOPAY_LBFGSERR_MAXIMUMLINESEARCH = -1009,
  TOPAY_LBFGSERR_MAXIMUMITERATION = -1008,
  TOPAY_LBFGSERR_WIDTHTOOSMALL = -1007,
  TOPAY_LBFGSERR_INVALIDPARAMETERS = -1006,
  TOPAY_LBFGSERR_INCREASEGRADIENT = -1005
};

/* L-BFGS parameter block — mirrors lbfgs::lbfgs_parameter_t (lbfgs.hpp:15-129). */
typedef struct {
  int mem_size;
  int past;
  int max_iterations;
  int max_linesearch;
  double g_epsilon;
  double delta;
  double min_step;
  double max_step;
  double f_dec_coeff;
  double s_curv_coeff;
  double cautious_factor;
  double machine_prec;
} topay_lbfgs_params_t;

/* Optimizer parameters — mirror MomaTrajOptParam (moma_traj_opt.h:441-564) with the values of
 * src/planner/params/optimizer.yaml as defaults, plus the MomaParam constants the path reads
 * (src/simulator/fake_moma/include/fake_moma/moma_param.h:36-126). */
typedef struct {
  int int_K;            /* Simpson panels per piece; this build supports 12 only */
  int min_piece_num;
  double relu_mu;
  double sample_interval;
  double energy_weights[9];
  /* first stage */
  double s1_time_weight, s1_moment_weight, s1_acc_weight, s1_domega_weight, s1_path_pos_weight;
  int s1_normal_past, s1_shot_path_past;
  double s1_shot_path_horizon;
  topay_lbfgs_params_t s1_lbfgs;
  /* second stage */
  double s2_time_weight, s2_moment_weight, s2_acc_weight, s2_domega_weight;
  double s2_collision_weight, s2_mani_colli_weight, s2_self_colli_weight;
  double s2_mani_pos_weight, s2_mani_vel_weight, s2_mani_acc_weight, s2_mean_time_weight;
  topay_lbfgs_params_t s2_lbfgs;
  /* ALM on the end-point constraint (only entries [0],[1] of the reference's vectors are used) */
  double alm_init_lambda[2], alm_init_rho[2], alm_rho_max[2], alm_gamma[2];
  double alm_tolerance;
  /* Deterministic replacement of the reference's 1.0 s wall-clock cap on the ALM loop
   * (moma_traj_opt.cpp:403-407): maximum number of outer iterations. */
  int alm_max_outer;
  /* Second part of that replacement: the reference checks its 1.0 s clock only before starting another ALM round;
   * here no further round is started once the stage-2 work done so far -- evaluations x pieces, the unit the
   * cost of an evaluation is proportional to -- reaches this budget.  Default 24000 piece-evaluations: one second
   * of the CPU path at the ~42 us per piece-evaluation measured for the oracle.  0 = unlimited. */
  int alm_work_budget;
  /* robot (MomaParam) */
  double chassis_height, chassis_colli_radius;
  double max_v, max_a, max_w, max_dw;
  double colli_length[8];
  double colli_points[16];
  double colli_point_radius[16];
  double joint_pos_limit_max[7];
  double joint_vel_limit[7];
  double joint_acc_limit[7];
  double relative_R[9]; /* row-major */
  double relative_t[3];
} topay_params_t;

/* ESDF description — GridMap (src/map/include/map/grid_map.h) dense buffers:
 *   esdf2d[x*dims[1] + y]                        (grid_map.h:798-806)
 *   esdf3d[x*dims[1]*dims[2] + y*dims[2] + z]    (grid_map.h:808-816) */
typedef struct {
  double origin[3];
  double resolution;
  int dims[3];
  double min_boundary[3];
  double max_boundary[3];
} topay_map_desc_t;

typedef struct topay_ctx topay_ctx;

/* Fill `p` with the reference defaults (optimizer.yaml + MomaParam). */
topay_status topay_default_params(topay_params_t* p);

/* == MomaTrajOpt::init (src/planner/include/planner/moma_traj_opt.h:845-941) for a caller without a ROS parameter server:
 * the optimiser parameters from the reference's parameter file (src/planner/params/optimizer.yaml, under
 * `planner_node: moma_traj_opt:` or at top level).  path_or_text: a file name, or the YAML text itself.  Keys that are
 * absent keep the value *params has on entry (call topay_default_params first).  ignored (optional, NUL-terminated,
 * newline-separated): the keys init() reads but this path has no use for -- mean_time_lowb / mean_time_uppb (the
 * reference's penalty uses the literals 0.5 and 2.0, moma_traj_opt.cpp:1752-1769), first_stage/mean_time_weight,
 * second_stage/alm_data/... -- and any key init() does not know. */
topay_status topay_params_from_yaml(const char* path_or_text, topay_params_t* params, char* ignored, int ignored_cap);

/* Create a context on HIP device `device` (use LOCAL_RANK for one process per GPU). */
topay_status topay_create(const topay_params_t* params, int device, topay_ctx** out);
void topay_destroy(topay_ctx* ctx);

/* == assigning MomaTrajOpt::opt_param (a public member the planner may change between calls, moma_traj_opt.h:616):
 * replace the context's parameters.  Weights, L-BFGS and ALM settings take effect with the next solve / evaluation of
 * the resident batch; a change of sample_interval, min_piece_num, the velocity / acceleration limits or the history
 * depth invalidates the resident batch (call topay_set_init_traj again).  Waits for a solve in flight. */
topay_status topay_set_params(topay_ctx* ctx, const topay_params_t* params);
const char* topay_last_error(void);

/* Upload a map; the context keeps a device copy.  Up to TOPAY_MAX_MAPS maps may be resident (the
 * reference's benchmark loop uses a fresh map per episode); `map_id` selects the slot (0 for the
 * single-map case). */
#define TOPAY_MAX_MAPS 4096
topay_status topay_set_map(topay_ctx* ctx, int map_id, const topay_map_desc_t* desc, const double* esdf2d,
                           const double* esdf3d);

/* == GridMap::updateESDF (src/map/src/grid_map.cpp:125-521): build the 2-D and 3-D signed distance fields of map slot
 * `map_id` ON THE DEVICE from the occupancy grids the reference fills from its point cloud (grid_map.cpp:733-747):
 *   occ2d[x*dims[1] + y] (1 = a point below the chassis height), occ3d[x*dims[1]*dims[2] + y*dims[2] + z].
 * Afterwards the slot is as if topay_set_map had been called with the CPU-built fields (bit-identical values).
 * topay_get_map copies a resident map back and reports the duration of the last build in milliseconds. */
topay_status topay_build_esdf(topay_ctx* ctx, int map_id, const topay_map_desc_t* desc, const signed char* occ2d,
                              const signed char* occ3d);
/* n_maps maps of equal dimensions in one set of launches (the benchmark loop regenerates the map every episode): the
 * occupancy grids are concatenated map after map; slots first_map_id .. first_map_id + n_maps - 1 are filled. */
topay_status topay_build_esdf_batch(topay_ctx* ctx, int n_maps, int first_map_id, const topay_map_desc_t* desc,
                                    const signed char* occ2d, const signed char* occ3d);
topay_status topay_get_map(topay_ctx* ctx, int map_id, double* esdf2d, double* esdf3d, double* build_ms);

/* Map slots first_map_id .. first_map_id + n_maps - 1 of `ctx` become references to the resident maps of `owner` (same
 * device), without a copy: the maps are read-only for every entry point but the three that fill a slot.  The reference
 * hands one GridMap::Ptr to all of its optimisers (planner.cpp:59-75: every MomaTrajOpt gets the planner's grid_map);
 * here the contexts of the batches in flight share one set of fields the same way.  The library tracks the sharing:
 * when `owner` refills one of the slots (topay_set_map, topay_build_esdf*), or is destroyed, every context that shares
 * the slot first finishes its pending solve and then loses it -- its next use of the slot returns TOPAY_ERR_NO_MAP until
 * it is shared or filled again; nothing is left pointing at freed or half-written fields. */
topay_status topay_share_maps(topay_ctx* ctx, topay_ctx* owner, int first_map_id, int n_maps);

/* All five fields of GridMap::updateESDF (src/map/src/grid_map.cpp:125-521).  Besides esdf2d and esdf3d (above) the
 * reference builds two more 2-D fields for its front-end:
 *   esdf_buffer_2d_inflate   (355-423): the signed field of the cells where esdf2d < chassis_colli_radius;
 *   esdf_buffer_2d_critical  (211-351): the signed field of occ_buffer_2d_critical (any cloud point above the cell,
 *                            whatever its height, grid_map.cpp:733-747), then -- into the same buffer, as the reference
 *                            does at line 348 -- the field of the cells where that one is < chassis_colli_radius.
 * occ2d_critical may be NULL: the projection of occ3d onto the plane is used (what the reference's fill produces for a
 * cloud inside the map's height).  topay_build_esdf / _batch are this call with occ2d_critical = NULL.
 * topay_get_map_fields copies the two extra fields of a built map back (either pointer may be NULL). */
topay_status topay_build_esdf_fields(topay_ctx* ctx, int n_maps, int first_map_id, const topay_map_desc_t* desc,
                                     const signed char* occ2d, const signed char* occ2d_critical, const signed char* occ3d);
topay_status topay_get_map_fields(topay_ctx* ctx, int map_id, double* esdf2d_inflate, double* esdf2d_critical);

/* ---- Benchmark episodes on the device: worlds, occupancy, scenarios -------------------------------------------------------
 * The first half of a turn of the reference's benchmark loop (Planner::benchmarkCallback, planner.cpp:491-548): the random
 * world (random_map_generator.cpp: "tables" 207-325, "cuboids" 342-443), its occupancy grids (GridMap::regenerateDesk /
 * regenerateMap, grid_map.cpp:716-798), updateESDF, and the rejection sampling of start, goal and the two arm
 * configurations.  The reference seeds all of it from std::random_device; here every generator is a mt19937_64 with an explicit
 * seed and the three draws of the CPU harness (harness/workload.hpp), which is the checker: equal seeds give equal bytes.
 *
 * topay_world_params_t: the generator's parameters (params/map_tables.yaml, map_cuboids.yaml).  obs_num are used as given:
 * a caller that wants the harness's World::build scales them with the area, obs_num * size_xy^2 / 400, rounded
 * (topay_amd.api.world_params does).  The map is GridMap::init's: min = -size / 2 (z from 0), dims = ceil(size / resolution).
 * Caps (TOPAY_ERR_INVALID_ARG above): a map holds at most 2048 accepted obstacle boxes, obs_num[0] + obs_num[1] + 2 keep-outs;
 * desk_arrangement_range is 1 <= [0] <= [1] <= 8 (a group of at most 8 x 8 desks: the primitive list of a map is sized for it). */
typedef struct {
  int kind;            /* 0 tables, 1 cuboids */
  int obs_num[2];      /* desks, boxes (40, 80) / standing, floating cuboids (80, 80) at 20 x 20 m */
  double size_xy, size_z, resolution, cloud_resolution;   /* 20, 1.6, 0.1, 0.05 */
  double wall_size_range[2], wall_height_range[2], float_size_range[2], float_height_range[2],
         desk_length_range[2], desk_width_range[2], desk_height_range[2];
  int desk_arrangement_range[2];
  int reserved;
} topay_world_params_t;
topay_status topay_world_default_params(int kind, topay_world_params_t* p);

/* World::build(kind, seed[i], ..., keepouts, nthreads = -1) for n maps followed by the construction of the five fields: slots
 * first_map_id .. first_map_id + n - 1 then hold what topay_build_esdf_fields gives for the harness's occupancy grids, bit for bit.
 *   seed         [n]
 *   keepouts_xy  [n][2][2]: centres of the two 1 x 1 x 1 m keep-out boxes of the tables world (start, goal; grid_map.cpp:766-770);
 *                NULL = none; ignored by the cuboids world
 *   status       [n], may be NULL: 1 built; -1 the generator's guard of 2 000 000 tries ended a loop early (the world is built
 *                with the obstacles placed so far, as the harness builds it)
 * The cloud is never materialised: every box is axis aligned, so a box marks (x, y) cells times a set of z cells.  Maps with at
 * most 32 layers whose column masks fit the LDS of a compute unit are rasterised there and written with 16-byte stores (path 1);
 * any other map by byte stores into cleared grids (path 2).  Both give the same bytes.
 * topay_get_occupancy copies the grids of a slot of the last topay_generate_worlds / _episodes back (any pointer may be NULL;
 * TOPAY_ERR_NO_MAP for a slot that call did not fill, or that has been refilled by another entry since). */
topay_status topay_generate_worlds(topay_ctx* ctx, int n, int first_map_id, const topay_world_params_t* params,
                                   const unsigned long long* seed, const double* keepouts_xy, int* status);
topay_status topay_get_occupancy(topay_ctx* ctx, int map_id, signed char* occ2d, signed char* occ2d_critical, signed char* occ3d);

/* World::sampleStartGoalXY for n seeds on a size_xy map (host only: the keep-outs of a tables world are needed before the world
 * exists): goal, then start, each (x, y) in [-size_xy / 2 + 2, size_xy / 2 - 2] and theta in [-pi, pi), accepted when
 * 3 <= distance <= 8.  start3 / goal3: [n][3].  TOPAY_ERR_INVALID_ARG for a map too small to hold such a pair. */
topay_status topay_sample_start_goal_xy(int n, const unsigned long long* seed, double size_xy, double* start3, double* goal3);
/* World::sampleArm for n states on resident maps: joints U[-max, max] until GridMap::isWholeBodyCollision is false, at most
 * max_tries times (<= 0: 2000, the harness's stand-in for the reference's 1 s clock).  states [n][10]: in x, y, theta; out the
 * joints of the last try.  ok [n]: 1 / 0; tries [n] (may be NULL).  map_ids NULL = slot 0. */
topay_status topay_sample_arm(topay_ctx* ctx, int n, const int* map_ids, const unsigned long long* seed, int max_tries,
                              double* states, int* ok, int* tries);
/* World::sampleScenario for n seeds on resident maps (the cuboids flow): start / goal pairs as above whose ends are 0.5 m clear in
 * the 2-D field, then the goal arm, then the start arm, up to 10000 attempts.  start, goal [n][10]; ok [n]. */
topay_status topay_sample_scenarios(topay_ctx* ctx, int n, const int* map_ids, const unsigned long long* seed, double* start,
                                    double* goal, int* ok);
/* One attempt of an episode per seed: the map into slot first_map_id + i, start and goal into start / goal [n][10].
 *   kind 0 (the tables flow of the harness's wl_tables_batch_create, without its init-path stand-in): with sd = seed * 1000 +
 *          attempt, start and goal (x, y, theta) from sd, the world from sd with keep-outs at both, the goal arm from
 *          seed * 7919 + 2 * attempt, the start arm from seed * 7919 + 2 * attempt + 1 (64-bit wrap-around arithmetic);
 *   kind 1: the world from seed, topay_sample_scenarios with the same seed.
 *   attempt  [n] or NULL = 0;  status [n]: 1 ok, 0 an arm or the scenario could not be sampled.
 * Nothing is retried inside: a caller repeats a failed episode on its own slot with attempt + 1. */
topay_status topay_generate_episodes(topay_ctx* ctx, int n, int first_map_id, const topay_world_params_t* params,
                                     const unsigned long long* seed, const int* attempt, double* start, double* goal, int* status);

/* Diagnostics of the last topay_generate_worlds / _episodes of a context (read only):
 *   topay_world_last_path  which rasteriser path ran, 1 or 2;
 *   topay_world_stage_ms   device time by stage from events: generation, rasterisation, fields, and the sampler's launch
 *                          (0 after topay_generate_worlds), in ms. */
topay_status topay_world_last_path(topay_ctx* ctx, int* path);
topay_status topay_world_stage_ms(topay_ctx* ctx, double ms[4]);
/* TEST HOOKS -- for the test suite only, not part of the product interface.  The two setters stay in force on the context until
 * they are set back to 0:
 *   topay_world_test_path       2 forces rasteriser path 2 whatever the map; 0 = the rule;
 *   topay_world_test_max_tries  tries per arm of topay_generate_episodes' tables flow; 0 = the harness's 2000;
 *   topay_test_mt64             runs on the device: outputs skip .. skip + n - 1 of mt19937_64(seed). */
topay_status topay_world_test_path(topay_ctx* ctx, int path);
topay_status topay_world_test_max_tries(topay_ctx* ctx, int max_tries);
topay_status topay_test_mt64(unsigned long long seed, int skip, int n, unsigned long long* out);

/* == optimizeTraj lines 146-357 for every batch member.
 *   path_len[b]      number of 10-d states of candidate b
 *   init_paths       ragged, sum(path_len) x 10, row-major (x, y, theta, q1..q7)
 *   boundary_vel/acc batch x 20, each a 10 x 2 column-major matrix as in the reference
 *                    (row 0 = v, row 1 = omega, rows 3-9 = joints; col 0 = start, col 1 = end); NULL = zeros
 *   map_ids          map slot per candidate, NULL = all slot 0
 * Uploads the raw paths (they stay resident), runs the init kernel, sizes the workspace.
 * The reference puts no bound on the number of pieces (moma_traj_opt.cpp:245, 300-321); this build solves up to 170
 * (a 255 s trajectory at the reference's 1.5 s sample_interval: what a four-wave workgroup holds in a compute unit's LDS).  A
 * candidate that needs more is reported as failed (success 0, cost NaN, n_pieces 0) without being launched and the
 * rest of the batch is solved normally; topay_get_batch's n_pieces lets the caller count such candidates. */
topay_status topay_set_init_traj(topay_ctx* ctx, int batch, const int* path_len, const double* init_paths,
                                 const double* boundary_vel, const double* boundary_acc, const int* map_ids);

/* Re-run the init kernel from the resident raw paths (restores x0 so the same batch can be
 * optimised again without uploading the paths a second time). */
topay_status topay_reset(topay_ctx* ctx);

/* == optimizeTraj lines 359-497 for every batch member (stage-1 L-BFGS, stage-2 ALM loop). */
topay_status topay_optimize(topay_ctx* ctx);

/* The same in two halves, so that a caller can keep several contexts (batches) in flight on one GPU: the tail of one
 * batch -- a few long candidates, most of the device idle -- then overlaps the bulk of the next.  topay_optimize ==
 * topay_optimize_async + topay_synchronize.  Results may be read after topay_synchronize.  The asynchronous call may
 * block until every candidate of the batch issued before it (by any context of the process on this device) has started:
 * the library hands the device over oldest batch first.  All contexts of a process share one parameter block in constant
 * memory: a solve whose parameters differ from those of a solve still in flight waits for that one to finish. */
topay_status topay_optimize_async(topay_ctx* ctx);
topay_status topay_synchronize(topay_ctx* ctx);

/* Batch-level results after topay_optimize: success[b] (0/1), cost[b] (traj_cost), n_pieces[b].
 * Any pointer may be NULL. */
topay_status topay_get_batch(topay_ctx* ctx, int* success, double* cost, int* n_pieces);

/* getTraj() of candidate i: durations[N]; coeffs[N][9][6] highest order first (minco.hpp:908-921);
 * knots_xy[(N+1)][2] Simpson-integrated piece end points.  Any output pointer may be NULL. */
topay_status topay_get_result(topay_ctx* ctx, int i, int* success, double* cost, int* n_pieces, double* durations,
                              double* coeffs, double* knots_xy);

/* getTraj() for a selection of candidates in ONE call and one device-to-host copy -- what a planner does with the
 * winners it has picked from topay_get_batch / topay_check_feasible / topay_get_total_durations (planner.cpp:999-1016:
 * the shortest feasible candidate of a scenario is the one that gets published).  Results are packed by pieces:
 *   idx[n]              candidate indices (a candidate that was never launched contributes zero pieces)
 *   piece_off[n + 1]    OUT: candidate k owns pieces [piece_off[k], piece_off[k+1]) of durations / coeffs
 *   durations[pieces]   coeffs[pieces][9][6] highest order first (minco.hpp:908-921)
 *   knots_xy            candidate k's N_k + 1 piece end points start at knots_xy[2 * (piece_off[k] + k)]
 *   cap_pieces          capacity of the output arrays in pieces; TOPAY_ERR_INVALID_ARG when the selection needs more */
topay_status topay_get_results(topay_ctx* ctx, int n, const int* idx, int cap_pieces, int* piece_off, double* durations,
                               double* coeffs, double* knots_xy);

/* Candidate i in the layout of src/planner/msg/PolyTraj.msg (uint8 order; std_msgs/Float32MultiArray[] coeff;
 * float32[] durations; int8[] directions -- the reference defines the message but never fills it, so the field
 * meanings are the obvious ones): *order = 5; coeff[N][9][6] = getTraj()'s coefficients as float32, one 9 x 6 array per
 * piece, highest order first; durations[N]; directions[N] = sign of the arc-length rate at the middle of the piece
 * (+1 forward, -1 reverse).  Capacity cap_pieces; *n_pieces receives N. */
topay_status topay_get_polytraj_msg(topay_ctx* ctx, int i, int cap_pieces, unsigned char* order, float* coeff,
                                    float* durations, signed char* directions, int* n_pieces);

/* Per-candidate solver counters, 8 ints each:
 * {stage1_ret, stage1_iters, stage1_evals, stage2_last_ret, stage2_iters, stage2_evals, alm_outer, sum_bound}
 * sum_bound = sum over stage-2 iterations of the two-loop history length (roofline accounting). */
topay_status topay_get_stats(topay_ctx* ctx, int* stats /* batch x 8 */);

/* Per-candidate optimisation time in microseconds, measured on the device (the reference logs the same quantity per
 * candidate, planner.cpp:893-905 "optimization time").  start_us (optional): when each solve started, on the same
 * device clock (only differences are meaningful); hw_id (optional): the hardware slot it ran on,
 * xcc << 16 | se << 12 | cu << 4 | simd (scheduling diagnostics).  Any pointer may be NULL. */
topay_status topay_get_elapsed_us(topay_ctx* ctx, double* us /* batch */, double* start_us /* batch */, int* hw_id /* batch */);

/* == GridMap::isWholeBodyCollision (src/map/include/map/grid_map.h:613-650) for n states (x, y, theta, q1..q7) against
 * map slot map_id: collide[i] = 1 when state i violates a joint limit, lies outside the map or collides (chassis, the 12
 * arm spheres against the environment, the chassis top and each other).  The check the front-end applies to every state
 * it samples or interpolates (mcrrts.cpp, planner.cpp:529-548). */
topay_status topay_whole_body_collision(topay_ctx* ctx, int map_id, int n, const double* states, int* collide);

/* First slice of the front-end that produces optimizeTraj's init paths.
 * topay_dense_path == GraphSearch::getDensePath (src/planner/src/graph_search.cpp:119-176) for n_paths raw 2-D paths:
 *   raw_len[p] points of path p, raw_xy ragged (sum x 2); out[p][cap_per_path][4] = (x, y, theta, dt) of the entries the
 *   reference keeps (dt > 1e-3, plus the final pose); out_len[p] = their number (entries beyond cap_per_path are counted,
 *   not written).
 * topay_connect_check_num / topay_connect_collision == MCRRTs::connectCollision (src/planner/include/planner/mcrrts.h:
 *   310-348) for n_edges edges of the joint-space tree.  The car poses along an edge come from OMPL's
 *   ReedsSheppStateSpace (distance, interpolate: mcrrts.h:318-324, 336) -- a third-party dependency of the reference,
 *   not part of it -- so the caller supplies rs_distance[e] and, for the piece_num[e] checks of edge e, the interpolated
 *   car poses car_poses[sum piece_num][3] at fractions i / piece_num[e]; the library interpolates the joints, builds the
 *   states and runs GridMap::isWholeBodyCollision on every one: collide[e] = 1 when any state of the edge collides. */
topay_status topay_dense_path(topay_ctx* ctx, int n_paths, const int* raw_len, const double* raw_xy, double step_size,
                              const double* start_yaw, const double* end_yaw, double v_max, double w_max, int cap_per_path,
                              int* out_len, double* out);
topay_status topay_connect_check_num(int n_edges, const double* rs_distance, const double* q_from /* n x 7 */,
                                     const double* q_to /* n x 7 */, double check_res, int* piece_num);
topay_status topay_connect_collision(topay_ctx* ctx, int map_id, int n_edges, const int* piece_num, const double* car_poses,
                                     const double* q_from, const double* q_to, int* collide);

/* == GraphSearch::plan2dJPS (src/planner/src/graph_search.cpp:53-117, with plan / getJpsSucc / jump / hasForced 178-475 and the
 * JPS2DNeib neighbour rules 583-669): the planner's direct chassis path (planner.cpp:816: threshold = chassis radius + 0.1)
 * for n (start, goal) pairs -- jump-point search on the 2-D distance field of each pair's map slot, then the zigzag cut
 * with GridMap::isLineCollisionGrid2d (grid_map.h:565-610).  out_len[p] = points of path p (0: no path; counts beyond
 * cap_points are reported, not written), out_xy + p * cap_points * 2 = its points, first = start, last = goal: the raw
 * path topay_dense_path takes.  stats (n x 2, optional): expanded nodes, jump points before the cut.  The open list
 * follows boost::heap::d_ary_heap<arity<2>> with the reference's compare_state (graph_search.h:20-38; boost is not part of
 * the reference's sources, its sift rules are restated), which is what decides between equal-cost paths.  One wavefront per
 * search (lane 0 runs the heap, the wave scans the jumps); the search state (21 bytes per map cell and search) is allocated
 * for the call. */
topay_status topay_plan2d_jps(topay_ctx* ctx, int n, const int* map_ids /* n, NULL = slot 0 */, const double* start_xy /* n x 2 */,
                              const double* end_xy /* n x 2 */, double threshold, int cap_points, int* out_len, double* out_xy, int* stats);

/* == MCRRTs::plan (src/planner/src/mcrrts.cpp:5-231; steer / rewire 336-400; the inline members of
 * src/planner/include/planner/mcrrts.h:153-348), the layered bidirectional search over the arm joints along a fixed chassis
 * path that produces optimizeTraj's init path -- n instances (candidate chassis paths) per call, one wavefront each.
 *   path_len[p], car_paths    chassis path of instance p: path_len[p] entries (x, y, theta, dt) as topay_dense_path /
 *                             GraphSearch::getDensePath return them (ragged, sum x 4); 2..min(cap_per_path, 255) entries
 *   start, end                n x 10 full states (x, y, theta, q1..q7); the joints seed the two trees
 *   wb_len[p], wb_path        the whole-body path: wb_len[p] states of 10 doubles (one per layer) at wb_path + p *
 *                             cap_per_path * 10; wb_len[p] = 0 when no path was found
 *   stats (n x 8, optional)   status (1 path, 0 none, -1 node pool full, -2 bad input), nodes, iterations, tree nodes,
 *                             anti-tree nodes, the two nodes that joined the trees, whole-body collision checks
 *   c_max (n, optional)       cost of the connection (mcrrts.cpp:74-79)
 * The chassis poses along a tree edge are ompl::base::ReedsSheppStateSpace(1e-2)'s (mcrrts.h:134, 318-324, 336); OMPL is a
 * third-party dependency that is not part of the reference's sources, its published algorithm (Reeds & Shepp 1990) is
 * implemented in the library (topay_reeds_shepp exposes it).  Where the reference is not reproducible the library is
 * deterministic (topay_mcrrt_params_t): every random draw is a pure function of (seed, first_instance + p, iteration,
 * slot) instead of a std::mt19937 seeded from std::random_device (mcrrts.h:89), and the 0.2 s wall-clock limits
 * (params/mcrrts.yaml, mcrrts.cpp:43, 143, mcrrts.h:225) are counts. */
typedef struct {
  double goal_sample_rate;     /* mcrrts/goal_sample_rate (0.4) */
  double check_colli_res;      /* mcrrts/check_colli_res (0.01): spacing of the collision checks along an edge */
  double rs_turning_radius;    /* ReedsSheppStateSpace(1.0e-2), mcrrts.h:134 */
  int max_iter;                /* iterations of the main loop (stands in for mcrrts/max_time) */
  int max_sample_tries;        /* resamplings of sampleState while the sample is in collision (mcrrts.h:225) */
  int node_cap;                /* nodes per instance; the search fails with status -1 when it needs more */
  int reserved;
  unsigned long long seed;
} topay_mcrrt_params_t;
void topay_mcrrt_default_params(topay_mcrrt_params_t* p);
topay_status topay_mcrrt_plan(topay_ctx* ctx, int n, const int* map_ids /* n, NULL = slot 0 */, const int* path_len, const double* car_paths,
                              const double* start, const double* end, const topay_mcrrt_params_t* params /* NULL = defaults */,
                              unsigned long long first_instance, int cap_per_path, int* wb_len, double* wb_path, int* stats, double* c_max);
/* Node table of instance `instance` of the last topay_mcrrt_plan, in creation order (diagnostics, parity tests): layer
 * (robo_state.first), state (MCRRTNode::NodeState: 1 EXPANDED, 2 IN_TREE, 3 IN_ANTI_TREE), parent (index, -1 none),
 * cost, q (7 per node).  Up to cap rows; any pointer may be NULL. */
topay_status topay_mcrrt_nodes(topay_ctx* ctx, int instance, int cap, int* layer, int* state, int* parent, double* cost, double* q);
/* == TopologyPRM::findTopoPaths (src/planner/src/topo_prm.cpp:60-122 with createGraph 124-212, findVisibGuard 214-233,
 * needConnection 235-263, getSample 265-276, lineVisib 278-315, pruneGraph 317-344, pruneEquivalent 346-382, selectShortPaths
 * 384-422, sameTopoPath 424-448, discretizePath 472-506, 599-616, shortcutPath(s) 512-582, discretizeLine 584-597, searchPaths /
 * depthFirstSearch 656-734; RayCaster::setInput / step, src/planner/src/utils/raycast.cpp:31-48, 253-346; parameters
 * src/planner/params/topo_prm.yaml): the topological roadmap that gives a planning call its up to reserve_num candidate
 * chassis paths (planner.cpp:813), for n (start, goal) queries, one wavefront each.  The roadmap reads the two front-end
 * fields of the query's map slot (getDistCoarse2d / 2i: esdf_buffer_2d_inflate, or esdf_buffer_2d_critical where
 * critical[p] != 0 -- the planner's second try, planner.cpp:961-963) and, for the push of a collision point, the plain 2-D
 * field (the critical one when critical): the slot must have been filled by topay_build_esdf* (TOPAY_ERR_NO_MAP after
 * topay_set_map, which has no front-end fields).
 *   n_paths[p], path_len, path_xy   select_paths of query p in the reference's order (shortest first): path k has
 *                             path_len[p * cap_paths + k] points at path_xy + (p * cap_paths + k) * cap_points * 2, first = start,
 *                             last = goal: the raw path topay_dense_path takes.  Counts beyond cap_points are reported, not
 *                             written.  cap_paths >= reserve_num.
 *   stats (n x 8, optional)   status (1 at least one path, 0 none, -1 a pool of the query is full: node_cap nodes,
 *                             TOPAY_TOPO_MAX_NB neighbours of a node, or the points of a discretised path -- twice the map's
 *                             diagonal in cells + 512; -2 undefined in the reference: a raw path of 100 nodes or more
 *                             (path_list(100), line 666), discretizePath without an interval or on an interval of zero length
 *                             (lines 491-500), a depth-first search past 2 000 000 nodes), samples drawn, samples that passed the
 *                             clearance test, graph nodes before / after pruneGraph, raw paths the search found, paths after the
 *                             first pruneEquivalent, selected paths.  With a negative status the other seven are 0.
 * Device memory: the graphs, raw paths and point buffers of the call stay in the context for topay_topo_graph /
 * topay_topo_raw_paths until the next call or topay_destroy -- per query node_cap x 156 bytes, max_raw_path x 200 bytes and
 * (2 max_raw_path2 + 2 reserve_num) point buffers of 16 bytes x the point cap of the largest map of the call: 1.1 MB per
 * query with the defaults on a 200 x 200 map, i.e. 1.1 GB for 1024 queries.  Split a larger sweep into several calls.  The
 * point cap of a query (status -1) is that of its own map.
 * Where the reference is not reproducible the library is deterministic: every draw of rand_pos_(eng_)
 * (default_random_engine(rd_()), topo_prm.cpp:36-37, 268-269) is a pure function of (seed, first_instance + p, sample index,
 * axis) -- the generator of topay_mcrrt_plan, mapped to [-1, 1) -- and the 0.01 s of accumulated wall time (max_sample_time) is
 * part of the count max_sample_num: default 2368 = the median number of samples the CPU restatement draws in 10 ms on one
 * host core over 64 tables scenarios (2340, docs/EXPERIMENTS.md "Sampling budget of the roadmap"), rounded up to whole
 * waves of 64; the reference's other bound, 5000, does not bind there.  A ray that has not reached its end cell after
 * |dx| + |dy| steps (the reference would not terminate) counts as visible.  sample_inflate_z is read by the reference and
 * never used (z = 0); short_cut_num likewise (parallel_shortcut: true runs one iteration per raw path, selectShortPaths five). */
#define TOPAY_TOPO_MAX_NB 32   /* neighbours per graph node */
typedef struct {
  double sample_inflate_x, sample_inflate_y;  /* topo_prm/sample_inflate_x, _y (1.5, 4.0) */
  double clearance;                           /* topo_prm/clearance (0.1) */
  double ratio_to_short;                      /* topo_prm/ratio_to_short (2.0) */
  int max_sample_num;                         /* samples per query (2368, see above; topo_prm.yaml: 5000 and 0.01 s) */
  int max_raw_path, max_raw_path2;            /* 300, 25 (at most 4096, 64) */
  int reserve_num;                            /* 6 (at most 16) */
  int node_cap;                               /* graph nodes per query (512); status -1 when it needs more */
  int reserved;
  unsigned long long seed;
} topay_topo_params_t;
void topay_topo_default_params(topay_topo_params_t* p);
topay_status topay_topo_paths(topay_ctx* ctx, int n, const int* map_ids /* n, NULL = slot 0 */, const double* start_xy /* n x 2 */,
                              const double* end_xy /* n x 2 */, const int* critical /* n, NULL = all 0 */,
                              const topay_topo_params_t* params /* NULL = defaults */, unsigned long long first_instance,
                              int cap_paths, int cap_points, int* n_paths /* n */, int* path_len /* n x cap_paths */,
                              double* path_xy /* n x cap_paths x cap_points x 2 */, int* stats /* n x 8, optional */);
/* The graph of query `instance` of the last topay_topo_paths after pruneGraph, in list order (diagnostics, parity tests):
 * id, type (1 guard, 2 connector), position, number of neighbours and their ids (TOPAY_TOPO_MAX_NB per node).  Up to cap
 * nodes are written, *n_nodes is their number in the graph; any output pointer may be NULL. */
topay_status topay_topo_graph(topay_ctx* ctx, int instance, int cap, int* id, int* type, double* pos_xy, int* n_neighbors,
                              int* neighbors /* cap x TOPAY_TOPO_MAX_NB */, int* n_nodes);
/* Parity tooling: the <= max_raw_path2 raw paths searchPaths kept for `instance` (which = 0) or their versions after
 * shortcutPaths (which = 1), laid out as topay_topo_paths lays out one query. */
topay_status topay_topo_raw_paths(topay_ctx* ctx, int instance, int which, int cap_paths, int cap_points, int* n_paths,
                                  int* path_len /* cap_paths */, double* path_xy /* cap_paths x cap_points x 2 */);

/* == Planner::planMomaParallel (src/planner/src/planner.cpp:792-1061), the whole planning call, for n calls at once: start
 * state, goal state and map slot in, the winning trajectory out.  Every stage is the kernel of its own entry point above and
 * every intermediate result stays on the device; only per-candidate counts, lengths and statuses come back between the
 * stages (they size the next launch and the solver's workspace).  Per call p, try t = 0 (plain fields), then t = 1 (the
 * critical field, planner.cpp:961-963) for the calls that have no winner yet:
 *   candidates   select_paths of topay_topo_paths (critical = t) in its order; for t = 0 the topay_plan2d_jps path
 *                (threshold chassis_colli_radius + jps_margin) is appended when it is not empty (a JPS path of more than
 *                512 points is a candidate that fails with search status -2: it is not kept).  No candidate: the try
 *                fails.  More than max_candidates: the reference throws "Too many paths to optimize" (planner.cpp:829):
 *                status -3 for that call, nothing more is run for it, the other calls are not affected.
 *   candidate k  getDensePath(path, dense_step, start[2], end[2], max_v, max_w), then MCRRTs::plan(start, end, dense) with
 *                `end` as given; a search without a path (or with fewer than 2 states, or a dense path outside 2..255
 *                entries: search status -2) fails the candidate.
 *   solve        the survivors of all calls of the try are ONE batch: init paths = the whole-body paths, column 0 of
 *                boundary_vel = start_v and zeros elsewhere (planner.cpp:873-875), map slot = the call's, group = the call
 *                with cancel_budget (topay_set_groups); topay_optimize, then the gate.  A candidate counts iff success, gate
 *                passed and not interrupted.  One that needs more than 170 pieces fails as topay_set_init_traj reports it.
 *   winner       the first candidate, in candidate order, whose total duration is strictly the smallest (planner.cpp:999-1010;
 *                rule and summation order of topay_scenario_records / topay_get_total_durations).
 * A call that fails both tries has status 0: the reference would now try OMPL's planners (planner.cpp:974-993), which are
 * outside this library.
 * The result of a call depends on nothing but the call: with c = first_call + p the roadmap draws with instance 2 c + t and
 * the search of candidate k with instance 16 c + 8 t + k, so a call may be batched with any others, in any order.
 *   result[p][8]             (columns TOPAY_PLAN_RES_*, TOPAY_PLAN_RES_LEN of them)
 *                            status (1 winner, 0 none, -3 too many candidates), try that decided the call (the winner's, else
 *                            the last one attempted; -1 none), candidates of try 0, of try 1, winner k or -1, the winner's
 *                            pieces, roadmap status of the last try attempted, the winner's index in the batch of its try
 *                            or -1 (what the per-candidate getters take while that batch is the resident one; a
 *                            position in the batch, hence the one entry that depends on what the call is batched with)
 *   candidates[p][2][8][4]   (optional; per try TOPAY_PLAN_MAX_CAND entries of columns TOPAY_PLAN_CAND_*, TOPAY_PLAN_CAND_ROW_LEN
 *                            ints per call) stage, n_pieces, search status, solver stage-2 status; stage (TOPAY_PLAN_STAGE_*):
 *                            0 absent, 1 search failed, 2 too many pieces, 3 solver failed, 4 gate failed, 5 interrupted, 6 counts
 *   winner_cost_duration[p][2]  (optional) the winner's traj_cost and total duration (NaN without a winner)
 * The winners' durations, coefficients, knots and whole-body init paths are gathered on the device into a store of the
 * context (the second try reuses the workspace); it stays valid until the next topay_plan_calls or topay_destroy and is what
 * topay_plan_get_trajs (layout of topay_get_results, per call instead of per candidate) and topay_plan_get_front_path read;
 * a call without a winner contributes zero pieces / zero states.  Afterwards the context's resident batch is the last
 * try's that had a candidate to solve: the getters above keep working on it.
 * Errors: TOPAY_ERR_NO_MAP when a call's slot has no front-end fields (topay_set_map); TOPAY_ERR_INVALID_ARG for n <= 0, NULL
 * start / end / result, max_candidates outside 1..8 or a stage's parameters out of range.  A solve in flight is waited for.
 * Device memory: per call of a front-end launch 1.1 MB of roadmap state (defaults, 200 x 200 map), 0.1 MB of raw paths and
 * 64 KB of dense paths; per candidate 0.27 MB of search state (node_cap 2048) and the solver's workspace (topay_workspace_bytes:
 * 0.4 MB at 11 pieces); the 21 bytes per map cell and JPS search are chunked to 2 GB.  The front-end runs in launches of at
 * most 1024 calls (a constant: results do not depend on it), so n calls need about min(n, 1024) x 2.2 MB + n x 3 x 0.4 MB.
 * topay_plan_test_chunk (test hook): another number of calls per front-end launch for this context, 0 = the constant.
 * topay_plan_stage_ms: device time of the last topay_plan_calls by stage, from pairs of HIP events around the stage's
 * launches on the context's stream (uploads, allocations and the host's waits between the stages are outside), 8 doubles
 * (TOPAY_PLAN_MS_*): roadmap, JPS, candidate table + dense paths, search (with its hand-off), init (hand-off + k_init), solve,
 * gate + winner, store gather. */
#define TOPAY_PLAN_MAX_CAND 8   /* candidates per call and try: traj_opters.size(), planner.cpp:59 */
enum { TOPAY_PLAN_RES_STATUS, TOPAY_PLAN_RES_TRY, TOPAY_PLAN_RES_CANDIDATES0, TOPAY_PLAN_RES_CANDIDATES1, TOPAY_PLAN_RES_WINNER,
       TOPAY_PLAN_RES_N_PIECES, TOPAY_PLAN_RES_TOPO_STATUS, TOPAY_PLAN_RES_WINNER_BATCH_INDEX, TOPAY_PLAN_RES_LEN };
enum { TOPAY_PLAN_CAND_STAGE, TOPAY_PLAN_CAND_N_PIECES, TOPAY_PLAN_CAND_SEARCH_STATUS, TOPAY_PLAN_CAND_SOLVER_STATUS, TOPAY_PLAN_CAND_LEN };
#define TOPAY_PLAN_CAND_ROW_LEN (2 * TOPAY_PLAN_MAX_CAND * TOPAY_PLAN_CAND_LEN)   /* 64 */
enum { TOPAY_PLAN_STAGE_ABSENT, TOPAY_PLAN_STAGE_SEARCH_FAILED, TOPAY_PLAN_STAGE_TOO_MANY_PIECES, TOPAY_PLAN_STAGE_SOLVER_FAILED,
       TOPAY_PLAN_STAGE_GATE_FAILED, TOPAY_PLAN_STAGE_INTERRUPTED, TOPAY_PLAN_STAGE_COUNTS, TOPAY_PLAN_STAGE_LEN };
enum { TOPAY_PLAN_MS_ROADMAP, TOPAY_PLAN_MS_JPS, TOPAY_PLAN_MS_DENSE, TOPAY_PLAN_MS_SEARCH, TOPAY_PLAN_MS_INIT, TOPAY_PLAN_MS_SOLVE,
       TOPAY_PLAN_MS_GATE_WINNER, TOPAY_PLAN_MS_STORE, TOPAY_PLAN_MS_LEN };
typedef struct {
  topay_topo_params_t topo;      /* topay_topo_default_params */
  topay_mcrrt_params_t mcrrt;    /* topay_mcrrt_default_params */
  double dense_step;             /* 1.414  (planner.cpp:858) */
  double jps_margin;             /* 0.1: plan2dJPS threshold = chassis_colli_radius + jps_margin (planner.cpp:816) */
  int cancel_budget;             /* 2400 piece-evaluations = the 100 ms of planner.cpp:946; 0 = no cancellation */
  int max_candidates;            /* 8 = traj_opters.size() (planner.cpp:59, 829); at most 8 */
  int critical_retry;            /* 1: second try on the critical field for calls without a success (961-963) */
  int reserved;
} topay_plan_params_t;
void topay_plan_default_params(topay_plan_params_t* p);
topay_status topay_plan_calls(topay_ctx* ctx, int n, const int* map_ids /* n, NULL = slot 0 */, const double* start /* n x 10 */,
                              const double* end /* n x 10 */, const double* start_v /* n x 10, NULL = zeros */,
                              const topay_plan_params_t* params /* NULL = defaults */, unsigned long long first_call,
                              int* result /* n x 8 */, int* candidates /* n x 2 x 8 x 4, optional */,
                              double* winner_cost_duration /* n x 2, optional */);
topay_status topay_plan_get_trajs(topay_ctx* ctx, int n, const int* call_idx, int cap_pieces, int* piece_off, double* durations,
                                  double* coeffs, double* knots_xy);
topay_status topay_plan_get_front_path(topay_ctx* ctx, int call, int cap_states, int* n_states, double* states /* x 10 */);
topay_status topay_plan_stage_ms(topay_ctx* ctx, double* ms /* 8 */);
topay_status topay_plan_test_chunk(topay_ctx* ctx, int calls);

/* ---- the replanning cycle: what runs around planMomaParallel while the robot moves.
 * Tracked trajectories.  A context keeps, per robot slot (0 .. TOPAY_TRACK_SLOTS - 1 = 4095), up to two committed trajectories
 * that outlive planning calls: 1 = end_traj, the one the robot follows and the planner replaces (planner.cpp:1010), and
 * 2 = global_traj, the one local goals are taken from.  A trajectory is a MomaTraj (moma_traj_opt.h:26-110): start state
 * (x, y, theta), up to 170 pieces -- durations and coefficients in the layout of topay_get_results, per piece 9 x 6, highest
 * order first -- and car_seq, which is computed once when the trajectory is committed, as MomaTraj's constructor does.
 *   topay_track_set          MomaTraj::setTraj (moma_traj_opt.h:96-110) from host data; which: 1, 2 or 3 = both
 *   topay_track_commit_plan  the winners of calls call_idx[k] of the last topay_plan_calls into slots robots[k], device to
 *                            device; committed[k] (may be NULL) = 1, or 0 when the call has no winner: the slot stays as it was
 *   topay_track_get          *n_pieces = pieces of the slot's trajectory (0: none; which: 1 or 2); the other outputs may be NULL
 *   topay_track_clear        both trajectories of the slot
 * TOPAY_ERR_INVALID_ARG: a robot slot out of range, which out of range, n_pieces outside 1..170, a total duration that is
 * not in (0, 1e4) (the gate's "no trajectory" rule; a NaN among the durations is such a one); a robot slot named twice in
 * one topay_track_commit_plan.
 * Memory: the trajectories lie in one device arena that grows and gives nothing back before topay_destroy.  A slot's block is
 * sized to the next power of two above what its trajectory needs (55 doubles per piece and 2 per 0.025 s of duration; at least
 * 1024 doubles) and is
 * reused by every later trajectory that fits, topay_track_clear included; one that does not fit gets a new block and the old
 * one is lost.  The lost blocks of a slot sum to less than its last one, so the arena stays below four times what the largest
 * trajectory of every (slot, which) ever committed needs (16 KiB where that is more), however long the loop runs. */
#define TOPAY_TRACK_SLOTS 4096
topay_status topay_track_set(topay_ctx* ctx, int robot, int which, const double* start3, int n_pieces, const double* durations,
                             const double* coeffs /* n_pieces x 9 x 6 */);
topay_status topay_track_commit_plan(topay_ctx* ctx, int n, const int* robots, const int* call_idx, int which, int* committed);
topay_status topay_track_get(topay_ctx* ctx, int robot, int which, int cap_pieces, int* n_pieces, double* start3, double* durations,
                             double* coeffs);
topay_status topay_track_clear(topay_ctx* ctx, int robot);
/* == Planner::safeCallback (planner.cpp:597-638) for n robots: end_traj of slot robots[k] sampled every 0.01 s (t = 0; t < T;
 * t += 0.01, the running sum) through getState against map slot map_ids[k] AS IT IS NOW -- not the map the trajectory was
 * planned on: getDistance2d of the chassis against 0.99 chassis_colli_radius, then getDistance3d of the 12 collision spheres
 * against 0.99 radius, in that order; the sweep of a robot ends at its first violation.  A point outside the map is 1e10 away.
 *   safe[k]          1 / 0
 *   first_hit[k][2]  index of the first violating sample and the first body in the reference's loop order at that sample
 *                    (0 chassis, 1..12 spheres); -1, -1 when safe
 *   hit[k][2]        time and distance of that hit; NaN when safe
 * Output pointers may be NULL.  TOPAY_ERR_NO_TRAJ: a slot without an end_traj; TOPAY_ERR_NO_MAP: a map slot that is not set.
 * topay_track_safe_ms: device time (HIP events around the launch) of the last sweep. */
topay_status topay_track_safe(topay_ctx* ctx, int n, const int* robots, const int* map_ids, int* safe, int* first_hit, double* hit);
topay_status topay_track_safe_ms(topay_ctx* ctx, double* ms);
/* Tracked trajectories sampled on the device: where n robots are at many times each, how they move there and how much room
 * they have.  Slot robots[k]'s trajectory `which` (1 end_traj, 2 global_traj) at M samples in all; row s of an output belongs
 * to sample s, and `what` (a sum of TOPAY_SAMPLE_*) says which outputs are computed.  At a sample's time t:
 *   state      [M][10]     MomaTraj::getState(t) (moma_traj_opt.h:113-137): x, y, theta, q1..q7; t clamped to [0, T]
 *   dstate     [M][10]     getDState(t) (moma_traj_opt.h:149-158): ds/dt, dtheta/dt, 0, the seven joint rates; t clamped
 *   ee_pose    [M][9]      MomaParam::getFKPose of that state (moma_param.h:339-373), the 9-vector of topay_ee_pose
 *   centres    [M][12][3]  the collision spheres' centres in the world frame (MomaParam::getColliPts, moma_param.h:203-247), as
 *                          the safety sweep forms them (planner.cpp:619)
 *   distance   [M][13]     what the sweep compares (planner.cpp:613-624): column 0 GridMap::getDistance2d of the chassis xy,
 *                          columns 1..12 getDistance3d of sphere i (grid_map.h:256-362), on map slot map_ids[k] AS IT IS NOW; a
 *                          point outside the map is 1e10 away
 *   clearance  [M][13]     distance minus the body's full radius: chassis_colli_radius, colli_point_radius of sphere i (not the
 *                          sweep's 0.99 of it); outside the map 1e10 - r
 *   duration   [n]         getTotalDuration (minco.hpp:304-313) of robot k's trajectory; needs no bit of `what`
 * clearance + r is the distance again only while r / 2 <= distance <= 2 r, where the subtraction is exact; closer or further it
 * rounds.  So `distance` is there beside `clearance`: hit[k][1] of topay_track_safe IS distance[first_hit[k][0]][first_hit[k][1]] of
 * the grid t0 = 0, step = 0.01, and the sweep's test is distance < 0.99 r.
 * topay_track_sample takes ragged times: robot k's are times[time_off[k] .. time_off[k + 1] - 1], time_off[0] = 0, M =
 * time_off[n]; a robot may have none.  topay_track_sample_grid takes a grid per robot: sample j of robot k (row k m + j) is the
 * running sum t0[k], += step (j additions, the `for (t = t0; ..; t += step)` of the reference's loops, planner.cpp:608, 719); m
 * samples always, no cut at T.
 * Every output pointer may be NULL, and an output whose bit is clear or whose pointer is NULL is neither computed nor written.
 * An output may be host memory or memory of the context's device (a torch tensor's data_ptr(), 8-byte aligned): the pointer
 * is asked (hipPointerGetAttributes); device memory is written by the kernel where it lies, and the entry returns once that is
 * done.  A robot may be named more than once.  The entries only read: trajectories, the resident batch, the plan store and the
 * maps stay as they are.
 * TOPAY_ERR_NO_TRAJ: a slot without the trajectory `which` names.  TOPAY_ERR_NO_MAP: TOPAY_SAMPLE_CLEARANCE or _DISTANCE and a map
 * slot that is not set (TOPAY_SAMPLE_CENTRES needs no map, and map_ids may be NULL without those two bits).
 * TOPAY_ERR_INVALID_ARG: n <= 0, which outside 1..2, what without a bit or with an unknown one, a robot slot out of range,
 * TOPAY_SAMPLE_CLEARANCE or _DISTANCE with map_ids NULL, time_off that decreases or does not start at 0, a time, t0 or step
 * that is not finite and below 1e9 in magnitude (checked before any launch), m < 0, n m of 2^31 or more, an output on another
 * device.  topay_track_sample_ms: device time (HIP events around the launch) of the last sampling kernel. */
enum { TOPAY_SAMPLE_STATE = 1, TOPAY_SAMPLE_DSTATE = 2, TOPAY_SAMPLE_EE_POSE = 4, TOPAY_SAMPLE_CLEARANCE = 8, TOPAY_SAMPLE_CENTRES = 16,
       TOPAY_SAMPLE_DISTANCE = 32 };
topay_status topay_track_sample(topay_ctx* ctx, int n, const int* robots, int which, const int* map_ids /* n */,
                                const int* time_off /* n + 1 */, const double* times, int what, double* state, double* dstate,
                                double* ee_pose, double* clearance, double* centres, double* duration, double* distance);
topay_status topay_track_sample_grid(topay_ctx* ctx, int n, const int* robots, int which, const int* map_ids /* n */,
                                     const double* t0 /* n */, double step, int m, int what, double* state, double* dstate,
                                     double* ee_pose, double* clearance, double* centres, double* duration, double* distance);
topay_status topay_track_sample_ms(topay_ctx* ctx, double* ms);
/* The endpoints of a replan, Planner::replanCallback (planner.cpp:708-731), for n robots:
 *   start[k]    end_traj.getState(t_s), t_s = t_since_replan[k] + planning_budget
 *   start_v[k]  end_traj.getDState(t_s) (moma_traj_opt.h:149-158): ds/dt, dtheta/dt, 0, the seven joint rates; t clamped to [0, T]
 *   goal[k]     the first state of global_traj on the grid t = t_since_begin[k], += 0.1, while t < T_g, whose xy is more than
 *               planning_horizon from start's xy; else global_goal[k] (also when the slot has no global_traj)
 *   goal_source[k]  the index of that step, -1 when global_goal was used
 * The clocks must be finite and t_since_begin not negative.  TOPAY_ERR_NO_TRAJ: a slot without an end_traj. */
topay_status topay_replan_inputs(topay_ctx* ctx, int n, const int* robots, const double* t_since_replan, const double* t_since_begin,
                                 const double* global_goal /* n x 10 */, double planning_budget, double planning_horizon,
                                 double* start /* n x 10 */, double* start_v /* n x 10 */, double* goal /* n x 10 */, int* goal_source);
/* One round of Planner::replanCallback (planner.cpp:640-750) for n robots: the safety sweep of every robot against
 * map_ids[k]; the trigger t_since_replan > replan_interval || !safe, unless now_xy (n x 2, may be NULL) is within 0.5 m of
 * global_goal's xy (planner.cpp:649: arrived); the endpoints of the triggered robots; ONE planning call for all of them, as
 * topay_plan_calls runs it, robot k's call numbered first_call + k -- k its position among the n given, so that its result does
 * not depend on which others triggered; the winners committed as end_traj (global_traj stays).  The three 10-vectors per
 * triggered robot pass through the host between the stages; trajectories, fields and sweeps stay on the device.  A robot
 * slot may be named only once among the n (TOPAY_ERR_INVALID_ARG).
 *   status[k][4]     (columns TOPAY_REPLAN_ST_*) outcome (0 not due, 1 replanned and committed, 2 due but no winner: the old trajectory is kept, 3 arrived),
 *                    safe, the robot's row in the plan store (what topay_plan_get_trajs takes) or -1, goal_source
 *   endpoints[k][30] (optional) start, start_v, goal of the triggered robots, NaN for the others
 *   plan_result[k][8], plan_candidates[k][2][8][4]  (optional) the tables of topay_plan_calls for the triggered robots, zeros
 *                    for the others */
enum { TOPAY_REPLAN_ST_OUTCOME, TOPAY_REPLAN_ST_SAFE, TOPAY_REPLAN_ST_STORE_ROW, TOPAY_REPLAN_ST_GOAL_SOURCE, TOPAY_REPLAN_ST_LEN };
topay_status topay_replan_calls(topay_ctx* ctx, int n, const int* robots, const int* map_ids, const double* t_since_replan,
                                const double* t_since_begin, const double* now_xy, const double* global_goal, double replan_interval,
                                double planning_budget, double planning_horizon, const topay_plan_params_t* params,
                                unsigned long long first_call, int* status, double* endpoints, int* plan_result, int* plan_candidates);

/* ---- End-effector goals: MomaTrajOpt::optimizeEE (moma_traj_opt.cpp:5-140) for n independent problems -----------------------
 * A goal state (x, y, theta, q1..q7) from an end-effector pose: what Planner::planCallBack is written around for "target"
 * goals (planner.cpp:188-199).  A pose is getFKPose's 9-vector (moma_param.h:339-373): position, row 0, row 1 of the rotation.
 * One problem per GPU lane, so the natural call is seeds x targets: many seeds per target, topay_ee_select picks.
 * What the reference leaves undefined is decided like this:
 *   - eeCostCallback adds into a gradient that lbfgs_optimize never clears (moma_traj_opt.cpp:135-137; lbfgs.hpp:504, 523,
 *     318); here the gradient is ASSIGNED.  (The reference's only call of optimizeEE is commented out.)
 *   - success is the reference's set of codes (moma_traj_opt.cpp:30-31): TOPAY_LBFGS_CONVERGENCE, _STOP, _CANCELED and
 *     TOPAY_LBFGSERR_MAXIMUMITERATION; the raw code is returned as well.
 *   - a sphere outside the 3-D field has distance 0 and gradient 0 (getDisWithGradI3d); reparameterisations, penalty and
 *     sin / cos are those of the trajectory solver (sigmoidC2, invSigmoidC2, getQtoVqGrad, smoothL1Penalty with relu_mu of
 *     topay_params_t, deterministic sin / cos). */
typedef struct {
  topay_lbfgs_params_t lbfgs;     /* mem_size 64 (1..64 accepted), past 3 (0..8), g_epsilon 1e-5, delta 1e-4, max_iterations 10000;
                                   * the other fields: lbfgs_parameter_t's defaults (lbfgs.hpp:15-129) */
  double cost_scale;              /* 10   (moma_traj_opt.cpp:68) */
  double mani_colli_weight;       /* 100  (69) */
  double self_colli_weight;       /* 100  (70) */
  double clearance_factor;        /* 1.1  (78) */
  double pose_tol;                /* topay_ee_select: largest |getFKPose(state) - ee_ref| (9-vector, 2-norm) of a goal; 1e-2 */
  int require_collision_free;     /* topay_ee_select: 1 = the goal must not be in isWholeBodyCollision on its map; 1 */
  int reserved;
} topay_ee_params_t;
void topay_ee_default_params(topay_ee_params_t* p);
/* getFKPose of n states: pose[n][9]. */
topay_status topay_ee_pose(topay_ctx* ctx, int n, const double* states /* n x 10 */, double* pose /* n x 9 */);
/* One eeCostCallback per problem at the UNCONSTRAINED x (x, y, theta, invSigmoidC2 of the joints), with the default weights:
 * f[n], g[n][10].  map_ids NULL = slot 0.  The per-evaluation parity hook, as topay_eval is for the trajectory problem. */
topay_status topay_ee_eval(topay_ctx* ctx, int n, const int* map_ids, const double* x /* n x 10 */, const double* ee_ref /* n x 9 */,
                           double* f, double* g /* n x 10 */);
/* optimizeEE of n problems.  seed_states[k] is the reference's moma_pos on entry; a seed joint at or beyond
 * +-joint_pos_limit_max has no unconstrained image: TOPAY_ERR_INVALID_ARG, checked before any launch.  states[k] is the
 * solution for a success code, else the seed; cost[k] the last evaluated cost; code[k] the raw L-BFGS code; iters[k], evals[k]
 * the iterations and cost evaluations taken.  Outputs other than states may be NULL.  A problem's result does not depend on
 * the others in the call or on its position among them.  topay_ee_ms: device time of the last call (HIP events). */
topay_status topay_ee_goals(topay_ctx* ctx, int n, const int* map_ids, const double* seed_states /* n x 10 */, const double* ee_ref /* n x 9 */,
                            const topay_ee_params_t* params, double* states /* n x 10 */, double* cost, int* code, int* iters, int* evals);
topay_status topay_ee_ms(topay_ctx* ctx, double* ms);
/* Seeds x targets into goals: per group g < n_groups the FIRST problem of smallest cost among those k with group_of[k] == g,
 * a success code, |getFKPose(states[k]) - ee_ref[k]| <= pose_tol and, when require_collision_free, not isWholeBodyCollision
 * on map_ids[k] (the check of topay_whole_body_collision).  winner[g] = its index and goal[g] = its state; winner[g] = -1 and
 * goal[g] untouched where none qualifies.  goal is the array topay_plan_calls takes. */
topay_status topay_ee_select(topay_ctx* ctx, int n, const int* map_ids, const int* group_of, int n_groups, const double* states /* n x 10 */,
                             const double* cost, const int* code, const double* ee_ref /* n x 9 */, const topay_ee_params_t* params,
                             int* winner, double* goal /* n_groups x 10 */);

/* ---- Sensor clouds into the map: rog_map's ProbMap on the grid of a map slot ------------------------------------------------
 * ProbMap::updateProbMap (src/rog_map/src/rog_map/prob_map.cpp:302-373) with raycastProcess (666-779), probabilisticMapFromCache
 * (544-568), hitPointUpdate / missPointUpdate (570-664), insertUpdateCandidate / updateLocalBox (781-822), RayCaster
 * (src/rog_map/include/utils/raycaster.cpp:65-192) and lineBoxIntersectPoint (include/utils/common_lib.hpp:148-170): the map
 * real-robot mode plans on (grid_map.cpp:20-26), as a per-slot occupancy belief.  Clouds are inserted on the device, occupancy
 * grids are derived from the belief and the slot's five fields rebuilt from them, so that the map can change under a committed
 * trajectory (topay_track_safe) without the host touching a voxel.
 * Configuration restated: raycasting/enable true, esdf/enable false, frontier_extraction_en false, no inflation map, no kd-tree;
 * map_sliding is a step of its own (topay_sense_slide, below): the insert never moves the grid.  Left out: re-addressing the
 * window through its hash (a slide moves the belief); the InfMap / CounterMap counters; ESDFMap::updateESDF3D
 * (the slot's fields come from the exact builder of topay_build_esdf_fields); the first-frame block that clears a sphere of
 * raycast_range_min around the robot (prob_map.cpp:356-372), a no-op at the shipped ray_range [0.0, 5]: ray_range[0] > 0 is
 * refused with TOPAY_ERR_UNSUPPORTED.
 * Grid: the slot's topay_map_desc_t, i.e. GridMap::init's origin, dims and resolution; points are in the map's world frame.  A
 * position is moved into the grid's frame first, u = p - origin, and the reference's code runs on u: voxel floor(u / resolution),
 * centre at + 0.5.  That is the reference's ORIGIN_AT_CORNER branch, the one its CMakeLists.txt:14 selects; its local map is the
 * voxels 0 .. dims - 1 and its local-map bounds the centres of the first and last voxel (sliding_map.cpp:93-95).
 * Belief: one float of log-odds per voxel.  A fresh voxel holds 0 (occupancy_buffer_.resize(map_size, 0), prob_map.cpp:78), which
 * is unknown: l_free <= 0 < l_occ for p_free < 0.5 < p_occ.  isOccupied: l >= l_occ; isKnownFree: l < l_free; unknown between
 * (prob_map.h:125-135).  l_x = logit(p_x) as config.hpp:229-235 computes it from the float p_x: the quotient x / (1 - x) in float,
 * the logarithm of that float in double, rounded to float.
 * Counts: per voxel and batch an operation count and a hit count (16 bits each); the flush adds l_hit * hits where there are hits
 * ("hit wins", prob_map.cpp:558-564), else l_miss * operations, once, and clamps: the belief does not depend on the order of the
 * points beyond what point_filt_num makes of it.  A batch may count at most 32767 rays per slot (a ray counts a voxel at most
 * twice; ceil(points / point_filt_num) per cloud is what is added up): TOPAY_ERR_INVALID_ARG for a cloud that could exceed it.
 * The intensity filter is the reference's: applied only when intensity_thresh > 0 (prob_map.cpp:688), and point_filt_num counts
 * the points that passed it.  point_filt_num and batch_update_size below 1 are 1 (config.hpp:180-194).  A point with a NaN or an
 * infinite coordinate is counted by the filters and casts no ray. */
typedef struct {
  float p_min, p_miss, p_free, p_occ, p_hit, p_max;            /* .12 .49 .499 .85 .9 .98  (params/rog_map.yaml, raycasting/) */
  double ray_range[2];                                         /* 0, 5 */
  int point_filt_num, batch_update_size, intensity_thresh;     /* 15, 1, -10 */
  int reserved;
  double virtual_ceil_height, virtual_ground_height;           /* 9999, -9999 */
  double local_update_box[3];                                  /* 50, 50, 5 */
  double chassis_height;                                       /* 0.155 (MomaParam): the 2-D rule of topay_sense_commit */
} topay_sense_params_t;
topay_status topay_sense_default_params(topay_sense_params_t* p);
/* The six log-odds of a parameter block, as the library computes them: l_hit, l_miss, l_min, l_max, l_occ, l_free. */
topay_status topay_sense_logodds(const topay_sense_params_t* p, float* l6);
/* Allocates or clears the beliefs of the n slots map_ids[k] on the grid `desc`: every voxel unknown, counts zero, batch counter
 * zero.  The slot's fields (if any) are not touched: a belief is state beside the map until topay_sense_commit. */
topay_status topay_sense_reset(topay_ctx* ctx, int n, const int* map_ids, const topay_map_desc_t* desc);
/* One updateProbMap per slot, all clouds of the call in one set of launches.  Slot k's cloud is points cloud_off[k] ..
 * cloud_off[k + 1] - 1 of points_xyzi (x, y, z, intensity as four floats per point; empty clouds are legal), seen from
 * sensor_pos[k] (3 doubles).  points_xyzi may be TOPAY_SENSE_LAST_SCAN: the points of the context's last topay_sense_scan, which
 * are on the device already (cloud_off then indexes that call's output).
 *   status[k] (may be NULL)  1 inserted and flushed, 0 inserted, the batch is still open (batch_update_size), -1 / -2 the sensor is
 *                            above the virtual ceiling / below the virtual ground: nothing changes (prob_map.cpp:313-322)
 * TOPAY_ERR_INVALID_ARG: a slot named twice (the batch counter is per slot), offsets that decrease, parameters out of range, a
 * sensor that is not finite or more than 1e6 m from the map's origin; TOPAY_ERR_NO_MAP: a slot without a belief. */
#define TOPAY_SENSE_LAST_SCAN ((const float*)(uintptr_t)1)
topay_status topay_sense_insert(topay_ctx* ctx, int n, const int* map_ids, const int* cloud_off /* n + 1 */, const float* points_xyzi,
                                const double* sensor_pos /* n x 3 */, const topay_sense_params_t* params, int* status /* n, optional */);
/* The belief into the map: occ3d = isOccupied (unknown counts as free, as ProbMap's own query does), occ2d_critical its
 * projection over z, occ2d = 1 where an occupied voxel's centre is below chassis_height (GridMap::cloudCallback, grid_map.cpp:
 * 554-568, with the voxel centre as the point); l_occ and chassis_height are those of the slot's last insert (the defaults before
 * the first).  Then the five fields through the code of topay_build_esdf_fields, device to device: the slot reads as if that
 * entry had been called with these grids, sharers of the slot are invalidated as for any refill (topay_share_maps), and
 * topay_get_occupancy serves the slots of the last topay_sense_commit.  A slot may be named once. */
topay_status topay_sense_commit(topay_ctx* ctx, int n, const int* map_ids);
/* The parity hook: the belief of a slot as it is, [nx][ny][nz] each.  Any pointer may be NULL. */
topay_status topay_sense_get(topay_ctx* ctx, int map_id, float* logodds, int* op_cnt, int* hit_cnt, int* batch_counter);
/* A range sensor on the device, so that an episode can be driven without the host: NOT a restatement (the reference's
 * pointcloud_render_node needs PCL).  Per pose (x, y, z, yaw) n_az x n_el rays through the resident occ3d of truth_map_ids[k] (a
 * slot topay_get_occupancy serves): ray i * n_el + j has azimuth 2 pi i / n_az + yaw and elevation fov ((j + 0.5) / n_el - 0.5)
 * (the library's deterministic sin / cos) and is traversed over `range` with the inserter's RayCaster.  Its point is the centre of
 * the first occupied voxel, the pose's own included; a ray that leaves the map or ends without one gives the point at 1.5 range
 * along it, so that an inserter with ray_range[1] <= range clamps it and records misses only.  Intensity 0.  Point k of pose p is
 * written at p * n_az * n_el + k, without compaction: cloud_off[p] = p * n_az * n_el (n + 1 entries, may be NULL).  The points
 * stay on the device for topay_sense_insert (TOPAY_SENSE_LAST_SCAN); points (cloud_cap points of 4 floats, may be NULL) receives
 * a copy. */
topay_status topay_sense_scan(topay_ctx* ctx, int n, const int* truth_map_ids, const double* poses /* n x 4 */, int n_az, int n_el, double fov,
                              double range, int cloud_cap, int* cloud_off, float* points);
/* Device time (HIP events) of the last scan, insert (selection and rays), flush, and commit with its fields, in ms. */
topay_status topay_sense_ms(topay_ctx* ctx, double ms[4]);

/* ---- Sliding sensor map: a slot's belief moves with the robot ---------------------------------------------------------------
 * params/rog_map.yaml ships map_sliding: {enable: true, threshold: 0.3}: ProbMap::updateProbMap re-centres the local map on the
 * sensor before it inserts a cloud (prob_map.cpp:306-311, 324-328), and SlidingMap::mapSliding forgets what leaves the window and
 * keeps what stays (sliding_map.cpp:113-166).  topay_sense_slide is that step for n slots; the cycle of a moving robot is
 * scan -> slide -> insert (skipped on status 2) -> commit.  A caller who never calls it sees nothing change.
 * Frame.  The belief's descriptor stays the one statement of the grid.  A slide by s voxels replaces origin[a] by
 * origin[a] + (double)s[a] * resolution (one multiply and one add per axis), and min_boundary / max_boundary move by the same
 * amount.  After that every sense entry runs unchanged on the new descriptor: the reference's code on u = p - origin.
 * Centre.  c[a] = dims[a] / 2 (integer division; for the reference's odd sizes 2h + 1 its centre voxel).
 *   v[a] = floor((sensor[a] - origin[a]) * (1 / resolution))    the inserter's expression (posToGlobalIndex, sliding_map.cpp:181-183)
 *   s[a] = v[a] - c[a] on the sliding axes, 0 elsewhere          shift_num (sliding_map.cpp:120)
 * Trigger (prob_map.cpp:324-326).  local_map_origin_d_ is origin_i * resolution, the LOW CORNER of the centre voxel and not its
 * centre (sliding_map.cpp:118); restated as it stands: d[a] = (sensor[a] - origin[a]) - (double)c[a] * resolution, and the slot
 * slides iff sqrt(d0 d0 + d1 d1 (+ d2 d2)), summed left to right over the sliding axes, is > threshold.  threshold = 0 re-centres
 * unconditionally.  The reference's implicit first-frame slide (map_empty_, !init_; prob_map.cpp:325, 329-332) has no counterpart:
 * topay_sense_reset places the grid explicitly.
 *   status[k]   0  within the threshold: nothing changes, shift 0 0 0
 *               1  slid by shift[3k ..]
 *               2  the sensor's voxel lay outside 0 .. dims - 1 on a sliding axis: slid as in 1, whatever the threshold.  The
 *                  reference drops that frame's cloud (prob_map.cpp:306-311), so the caller should skip the insert too
 *              -1  a batch is open (batch counter != 0, the reference's condition for both slides): nothing changes, shift 0 0 0
 * Effect.  The log-odds of local voxel l afterwards are those of local voxel l + s before, where l + s lies in 0 .. dims - 1 on
 * every axis; every other voxel holds 0 = unknown, what resetCell and resetLocalMap leave (prob_map.cpp:511-, 823-831).  A shift of
 * dims[a] or more on an axis therefore clears everything (resetLocalMap, sliding_map.cpp:121-128; the slab clearing of a shift of
 * exactly dims[a] gives the same).  Counts are zero whenever a slide is legal (no count outlives a flush, and a slide needs a
 * closed batch): they stay zero and do not move.  The batch counter stays 0.
 * Fields.  A slide touches the belief only.  The slot's five fields and the slot's own descriptor stay those of the last
 * topay_sense_commit, so a planning call between slide and commit reads a consistent map; the next topay_sense_commit builds the
 * fields on the slid descriptor and installs it with them.
 * Memory.  The shifted image is written into one scratch buffer of the context and copied back on the context's stream.  The
 * scratch holds 4 bytes per voxel of the slots that moved in one call and grows to the largest such call: at most the log-odds
 * of all beliefs named in one call, never a second copy per slot.
 * Deviations.  slide_z defaults to 0: a ground robot's slot spans z from the floor, and topay_sense_commit's chassis rule and the
 * 16-layer columns assume it; with slide_z = 0 the z axis takes no part in the shift, the trigger or status 2.  slide_z = 1 is
 * the reference.  The window is moved physically and not re-addressed through getLocalIndexHash (sliding_map.cpp:168-173),
 * because every kernel that reads a belief or a field indexes a dense grid.  Left out as for the insert: InfMap, FreeCntMap and
 * ESDFMap::mapSliding.
 * TOPAY_ERR_NO_MAP: a slot without a belief.  TOPAY_ERR_INVALID_ARG: a slot named twice or out of range, n <= 0, NULL map_ids or
 * sensor_pos, a negative or non-finite threshold, a sensor that is not finite or more than 1e6 m from the origin (the inserter's
 * rule) or whose voxel index exceeds 1e9. */
typedef struct {
  double threshold;   /* 0.3   rog_map.yaml map_sliding/threshold */
  int slide_z;        /* 0: x and y only (see Deviations); 1: all three axes, as the reference */
  int reserved;
} topay_sense_slide_params_t;
topay_status topay_sense_slide_default_params(topay_sense_slide_params_t* p);
topay_status topay_sense_slide(topay_ctx* ctx, int n, const int* map_ids, const double* sensor_pos /* n x 3 */,
                               const topay_sense_slide_params_t* params /* NULL = defaults */,
                               int* status /* n, optional */, int* shift /* n x 3, optional */);
topay_status topay_sense_slide_ms(topay_ctx* ctx, double* ms);   /* device time of the last call's launches */
/* The parity hook beside topay_sense_get: the descriptor of a slot's belief as it is (the slot's own follows at the commit). */
topay_status topay_sense_get_desc(topay_ctx* ctx, int map_id, topay_map_desc_t* desc);

/* ---------------------------------------------------------------------------------------------------------------------
 * The tracking controller and the fake robot: what Planner::cmdCallback (planner.cpp:158-178) runs between two replans.
 * topay_mpc_*: OMPC (planner/src/ompc.cpp, include/planner/ompc.h), the chassis tracking MPC around a slot's end_traj;
 * topay_sim_*: moma_sim (simulator/fake_moma/src/moma_sim.cpp:208-229, 251-308); topay_track_follow: both, period after period,
 * without the host.  Robot slots are those of topay_track_*.  One wave per robot.
 * Clock: the library keeps none.  Every call takes t_cur[k] = the reference's now - begin_time; after a replan that is the
 * wait_time of setTraj(end_traj, wait_time).  at_goal is therefore a function of the call, t_cur >= T_total + 1.0 (1.0 s after
 * topay_mpc_set_direct in direct mode, whose begin_time is the clock's zero too), not a flag that stays set.
 * Restated as it stands: the arm command getState / getDState(t_cur + 1 / ctrl_freq); the reference rows by the running sum
 * t = t_cur + dt, t += dt; smooth_yaw with its >= pi / 2 loops; predictMotion with stateTrans's clamps; du summed as the
 * reference sums it; the QP of solveMPCDiff entry for entry, in both of its branches (delay_num_v == delay_num_w, delay_num_v >
 * delay_num_w); output left as it was when the QP is not solved; predictMotion(xopt); the command output(0, delay_num_v),
 * output(1, delay_num_w) and the FIFO shift.  The controller state survives a new end_traj (setTraj clears nothing).
 * Deviations:
 *   - The wall-clock break of the outer loop (ompc.cpp:630, 1 / ctrl_freq) is not restated: max_iter is the only cap.
 *   - OSQP is not restated.  The QP has one minimiser (its Hessian's diagonal is positive); the solver returns x, y, z that meet
 *     OSQP's termination criterion on the unscaled problem at qp_eps_abs = qp_eps_rel = 1e-6:
 *       |A x - z|_inf <= eps_abs + eps_rel max(|A x|, |z|),   |P x + q + A' y|_inf <= eps_abs + eps_rel max(|P x|, |A' y|, |q|),
 *     l <= z <= u, and y in the normal cone of [l, u] at z (y_i > 0 only where z_i = u_i, y_i < 0 only where z_i = l_i), exactly.
 *     Method: OSQP's ADMM step with a fixed rho (no adaptation: that depends on timings; 10, not OSQP's initial 0.1, at which the
 *     shipped QP does not reach the criterion in 30000 steps, docs/EXPERIMENTS.md), equality rows at 1e3 rho, variables
 *     ordered by stage (v_j, w_j, x_j, y_j, theta_j) so that P + sigma I + A' R A has half-bandwidth 5; it is factored (L D L') once
 *     per QP in LDS, every step is one banded solve plus stage-local products.  The criterion is tested every 10th step and at
 *     qp_max_iter.  The first QP of a command starts from zero, every later one from the x, y of the one before.  Every sum has one
 *     fixed order: device, emulator and harness/ompc.hpp agree bit for bit.
 *   - sin / cos are the library's deterministic ones.
 * Left out: the CasADi MPC class of mpc.h, the drawing functions, gripper_state, the lidar pose, normlize_theta (unused).
 * Refused before any launch: TOPAY_ERR_UNSUPPORTED for delay_num_v < delay_num_w (the reference's code for it is commented out,
 * its matrix would be incomplete) and for max(delay_num_v, delay_num_w) == 0 (the reference reads output_buff.back() of an empty
 * vector); TOPAY_ERR_INVALID_ARG for predict_steps - delay_num_v < 2 (the dQ corrections and mz assume two inputs of each kind),
 * more than 64 stages (predict_steps - delay_num_w), predict_steps > 128, max_iter < 1, clocks, states or positions that are not
 * finite or reach 1e9 in magnitude (parameters: 1e12), a slot named twice, a slot that was never reset.
 * A new end_traj does not change the slot's mode (the library does not tie the two stores together): where the reference's setTraj
 * sets control_state = 0, a caller in direct mode calls topay_mpc_set_direct(..., NULL). */
#define TOPAY_MPC_MAX_STEPS 128
#define TOPAY_MPC_MAX_STAGES 64
typedef struct {
  double du_threshold, dt, ctrl_freq;                 /* 0.001, 0.02, 50   (params/mpc.yaml, ompc/) */
  int max_iter, predict_steps, delay_num_v, delay_num_w;   /* 150, 50, 20, 20 */
  double max_omega, max_domega, max_speed, min_speed, max_accel;   /* 0.9, 1.0, 1.0, -1.0, 0.8 */
  double matrix_q[3], matrix_r[2], matrix_rd[2];      /* 10 10 3, 0.01 0.01, 15 1.5 */
  double qp_eps_abs, qp_eps_rel;                      /* 1e-6, 1e-6 */
  double qp_rho, qp_sigma, qp_alpha;                  /* 10, 1e-6, 1.6 */
  int qp_max_iter, reserved;                          /* 30000 */
} topay_mpc_params_t;
topay_status topay_mpc_default_params(topay_mpc_params_t* p);
/* Variables and constraint rows of the QP at these parameters (the reference's nx and nc); the checks above. */
topay_status topay_mpc_qp_dims(const topay_mpc_params_t* p, int* nx, int* nc);
/* What OMPC::init creates, for the n slots robots[k]: output (2 x predict_steps) zero, the command FIFO output_buff of
 * max(delay_num_v, delay_num_w) zero entries, mode 0.  The parameters hold for the slot until its next reset. */
topay_status topay_mpc_reset(topay_ctx* ctx, int n, const int* robots, const topay_mpc_params_t* params);
/* OMPC::setDirect: control_state 1 with the constant reference direct_pos[k] (x, y, theta), arm held at now_state, at goal after
 * 1.0 s.  direct_pos NULL: back to trajectory mode. */
topay_status topay_mpc_set_direct(topay_ctx* ctx, int n, const int* robots, const double* direct_pos /* n x 3 or NULL */);
/* One OMPC::getCmd per robot.  cmd[k][16] = speed, angular_velocity, q[7], dq[7].  status[k][TOPAY_MPC_ST_LEN]: outcome (0
 * command, 1 at goal: zero chassis command, nothing else changes, 2 no trajectory: zero command, arm held at now_state, 3 a
 * command, but the QP was not solved in some outer iteration), outer iterations taken, QP steps summed, mode.  xopt (may be NULL):
 * [k][TOPAY_MPC_MAX_STEPS + 1][3], rows 0 .. predict_steps of predictMotion(xopt), the others zero. */
enum { TOPAY_MPC_ST_OUTCOME, TOPAY_MPC_ST_OUTER, TOPAY_MPC_ST_QP_ITERS, TOPAY_MPC_ST_MODE, TOPAY_MPC_ST_LEN };
topay_status topay_mpc_cmds(topay_ctx* ctx, int n, const int* robots, const double* t_cur, const double* now_state /* n x 10 */,
                            double* cmd /* n x 16 */, int* status /* n x 4, optional */, double* xopt /* optional */);
/* The parity hook: the first outer iteration of topay_mpc_cmds for one robot, the slot's state untouched.  The QP dense and in the
 * reference's order (variables: states, v, w; rows: box v, box w, dynamics, rate v, rate w): P [nx][nx], q [nx], A [nc][nx], l, u
 * [nc]; its solution x [nx], y, z [nc]; info[2] = QP steps, solved.  Any output may be NULL.  TOPAY_ERR_NO_TRAJ when the call does
 * not reach the QP (no trajectory, at goal): the kernel decides that, as for topay_mpc_cmds, and the outputs are left alone. */
topay_status topay_mpc_probe(topay_ctx* ctx, int robot, double t_cur, const double* now_state, double* P, double* q, double* A, double* l,
                             double* u, double* x, double* y, double* z, int* info);
/* The slot's state: output [2][TOPAY_MPC_MAX_STEPS], fifo [TOPAY_MPC_MAX_STEPS][2] (the first max(delay_num_v, delay_num_w) rows
 * are output_buff, oldest first), mode.  Any pointer may be NULL. */
topay_status topay_mpc_get_state(topay_ctx* ctx, int robot, double* output, double* fifo, int* mode);
/* Device time (HIP events) of the last topay_mpc_cmds or topay_track_follow, in ms. */
topay_status topay_mpc_ms(topay_ctx* ctx, double* ms);

/* moma_sim with the clock made explicit.  topay_sim_reset: the robot at state0[k] (x, y, theta, q[7]), no command received, an empty
 * actuator FIFO of delay_cmds commands (1 .. 128; 20 = the reference's time_delay 0.4 s at 50 Hz).  The reference's test "ROS time
 * since the first command > time_delay" is restated as a count: the chassis command is zero until delay_cmds commands have been
 * received, after that the oldest entry is taken, so command k acts from the receipt of command k + delay_cmds.
 * topay_sim_step: cmd[k] (may be NULL: no command this step) through rcvVelCmdCallBack, then `ticks` ticks of simCallBack at 0.01 s
 * (x += v 0.01 cos(theta), y likewise, theta += w 0.01, normyaw's single wrap, the arm set to cmd.q); nothing moves before the
 * first command.  state (n x 10, may be NULL) receives the robots' states. */
topay_status topay_sim_reset(topay_ctx* ctx, int n, const int* robots, const double* state0 /* n x 10 */, int delay_cmds);
topay_status topay_sim_step(topay_ctx* ctx, int n, const int* robots, const double* cmd /* n x 16 or NULL */, int ticks, double* state);
/* `periods` control periods in one launch: per period one topay_mpc_cmds from the simulator's own state at t, one topay_sim_step
 * of ticks_per_period ticks, t = t + 1 / ctrl_freq (t starts at t0[k]).  Equal bit for bit to that sequence of single calls.
 * states_out [n][periods][10] (after the step), cmds_out [n][periods][16], status_out [n][periods][TOPAY_MPC_ST_LEN]: optional. */
topay_status topay_track_follow(topay_ctx* ctx, int n, const int* robots, const double* t0, int periods, int ticks_per_period,
                                double* states_out, double* cmds_out, int* status_out);

/* ompl::base::ReedsSheppStateSpace(rho) for n pose pairs (x, y, theta): distance[i] = distance(from_i, to_i), word[i] /
 * lengths[i][5] = the shortest path's segment word (0..17, OMPL's reedsSheppPathType numbering) and signed segment lengths
 * in units of rho, pose[i] = interpolate(from_i, to_i, t[i]) when t is given.  Output pointers may be NULL. */
topay_status topay_reeds_shepp(topay_ctx* ctx, int n, const double* from, const double* to, const double* t /* n or NULL */, double rho,
                               double* distance, int* word, double* lengths, double* pose);

/* MomaTraj playback of candidate i (moma_traj_opt.h:26-137): car_seq -- (x, y, theta, t) every 0.1 s from Simpson
 * panels of 0.025 s, what the reference stores in the trajectory object and publishes -- and getState(t) at caller-given
 * times, states[n_times][10] = (x, y, theta, q1..q7).  seq (seq_cap rows of 4 doubles) may be NULL; *n_seq receives the
 * number of car_seq entries. */
topay_status topay_playback(topay_ctx* ctx, int i, int n_times, const double* times, double* states, int seq_cap,
                            double* seq, int* n_seq);

/* Mesh kinematics of MomaParam that only getMeshPose uses (moma_param.h:60-67, 77-90, 114-115). */
typedef struct topay_mesh_params_t {
  double link_length[7];
  double joint_pos_limit_min[7];
  double joint_offset[21];   /* 7 x 3 row-major: roll, pitch, yaw of the fixed rotation before joint i */
  double joint_dof_axis[21]; /* 7 x 3 row-major: the joint angle multiplies this (roll, pitch, yaw) triple */
} topay_mesh_params_t;
topay_status topay_default_mesh_params(topay_mesh_params_t* p);

/* == MomaParam::getMeshPose (moma_param.h:724-790) for n states (x, y, theta, q1..q7): parts[n][11][7], rows = chassis,
 * stump, link 1..7, end effector (a copy of link 7), end-effector collision point (position only, orientation zero);
 * columns = x, y, z, qw, qx, qy, qz as in MeshPart.msg. */
topay_status topay_mesh_poses(topay_ctx* ctx, const topay_mesh_params_t* mesh, int n, const double* states, double* parts);

/* == Planner::toMeshMsg (planner.cpp:2003-2056) of candidate i, the MeshTraj message the planner publishes for the winner
 * (planner.cpp:1014-1016): the trajectory sampled through MomaTraj::getState every T / res (res = 1000 in the
 * reference; t accumulated and compared `t < T` as there, so *n_states is res or res + 1), per sample the 11 mesh
 * poses, the yaw and the accumulated chassis arc length.  cap_states >= res + 1. */
topay_status topay_mesh_traj(topay_ctx* ctx, int i, const topay_mesh_params_t* mesh, int res, int cap_states, double* parts,
                             double* yaws, double* arc_lengths, int* n_states);

/* Total duration of every candidate's returned trajectory (MomaTraj::getTotalDuration): the quantity the planner ranks
 * the successful candidates of a scenario by (planner.cpp:999-1010). */
topay_status topay_get_total_durations(topay_ctx* ctx, double* total /* batch */);

/* ALM state (alm_lambda[2], alm_rho[2]) every candidate finished with; traj_cost is the stage-2 cost at the returned x
 * with this state (moma_traj_opt.cpp:398-401, 456-459). */
topay_status topay_get_alm(topay_ctx* ctx, double* alm /* batch x 4: lambda0, lambda1, rho0, rho1 */);

/* Number of decision variables of candidate i (n = 10N - 8) and the packed vector
 * x = [tau(N) | theta(N-1) | s(N) | Vq(7 x (N-1), column = knot)] (moma_traj_opt.cpp:324-344). */
topay_status topay_get_x(topay_ctx* ctx, int i, int* n, double* x);

/* Test hook == first/secondStageCostCallback (moma_traj_opt.cpp:817-955): evaluate stage `stage`
 * (1 or 2) of candidate i at x with ALM state (lambda, rho); returns f, g[n] and, for stage 2,
 * final_xy_error[2] (NULL allowed). */
topay_status topay_eval(topay_ctx* ctx, int stage, int i, const double* x, const double* alm_lambda,
                        const double* alm_rho, double* f, double* g, double* final_xy_error);

/* Test hook: topay_eval by the kernel with `waves` wavefronts per trajectory (1: N <= 64, 2: N <= 64, 4: N <= 170)
 * instead of the candidate's class default.  The evaluation is order-identical for any number of waves: f, g and the
 * end-point error must come out bit for bit equal. */
topay_status topay_eval_waves(topay_ctx* ctx, int stage, int i, int waves, const double* x, const double* alm_lambda,
                              const double* alm_rho, double* f, double* g, double* final_xy_error);

/* The spline of a given decision vector as candidate i's result.  MomaTrajOpt keeps the MINCO state of its last cost
 * evaluation and getTraj() returns it (moma_traj_opt.h:943-946; secondStageCostCallback, moma_traj_opt.cpp:885-955):
 * one stage-2 evaluation at x with the ALM state (lambda, rho), after which topay_get_result(s), topay_playback,
 * topay_mesh_traj, topay_get_polytraj_msg and the feasibility gate serve x's trajectory (replay / warm-start entry;
 * the stored cost is the stage-2 cost at x, success is set). */
topay_status topay_load_solution(topay_ctx* ctx, int i, const double* x, const double* alm_lambda, const double* alm_rho);

/* Batched form of the hook over candidates [0, batch): x is batch x nmax (row stride nmax from
 * topay_get_nmax), g likewise; used by bench.py to time the cost/gradient kernel on its own. */
topay_status topay_eval_batch(topay_ctx* ctx, int stage, int repeats, double* f /* batch */);
topay_status topay_get_nmax(topay_ctx* ctx, int* nmax, int* Nmax);

/* == printConstraintsSituations (moma_traj_opt.h:1052-1204), the gate the planner applies to every optimised candidate
 * (planner.cpp:878-880), for every candidate of the batch after topay_optimize: feasible[b] 0/1.  The trajectory is
 * sampled every 0.01 s through MomaTraj::getState (moma_traj_opt.h:26-137).
 * topay_feasibility_report also returns checkFeasible's verdict (948-1050: additionally requires the sphere clearances)
 * and the extreme values the verdicts are made from, 38 doubles per candidate:
 *   |v| |a| |omega| |domega| maxima, |q| max[7], |dq| max[7], |d2q| max[7], chassis min distance, sphere min distance[12].
 * Any output pointer may be NULL. */
topay_status topay_check_feasible(topay_ctx* ctx, int* feasible);
topay_status topay_feasibility_report(topay_ctx* ctx, int* feasible, int* strict, double* report /* batch x 38 */);

/* Debug / parity tooling: record the cost f of every evaluation made by the next topay_optimize
 * (at most `cap` per candidate, 0 switches it off); topay_get_trace copies candidate i's `cap` values. */
topay_status topay_set_trace(topay_ctx* ctx, int cap);
topay_status topay_get_trace(topay_ctx* ctx, int i, double* out);

/* Test hook for the deterministic elementary functions of the solver (topay_amd/csrc/topay_math.h):
 * out[4i..] = sin(a_i), cos(a_i), atan2(a_i, b_i), sqrt(|a_i|)/(1+|b_i|). */
topay_status topay_test_math(topay_ctx* ctx, int n, const double* a, const double* b, double* out4n);

/* == the planner's thread group and its cancellation (planner.cpp:829-952): the candidates of one planning call run
 * concurrently, and 100 ms after the first of them has succeeded (optimizeTraj true AND printConstraintsSituations
 * passed) the ones still running are interrupted (threads.interrupt_all(); interruption points: top of the ALM loop and
 * every second-stage cost evaluation, moma_traj_opt.cpp:402, 887) and count as failed.
 *   group_id[b]    planning call of candidate b, -1 = none (NULL: no groups)
 *   cancel_budget  the 100 ms in the deterministic unit of alm_work_budget: piece-evaluations (stage-1 + stage-2
 *                  evaluations x pieces; 24 000 = 1 s, so 2400 = 100 ms); 0 = no cancellation (the default)
 * The rule is applied on the candidates' own work clocks -- a candidate counts iff its clock at the end is within
 * cancel_budget of the smallest clock of a feasible success of its call -- so the outcome does not depend on how the
 * device happened to schedule the candidates; the solve stops a candidate as soon as it can see that it is past the limit.
 * Interrupted candidates: success 0, stage-2 status TOPAY_INTERRUPTED, topay_get_interrupted 1.
 * Call after topay_set_init_traj (a new batch starts without groups). */
#define TOPAY_INTERRUPTED (-2000)
topay_status topay_set_groups(topay_ctx* ctx, const int* group_id /* batch */, int cancel_budget);
/* threads.interrupt_all() (planner.cpp:952) for the solve in flight: every candidate stops at one of its next interruption
 * points (the flag lives in host memory; a running candidate looks at it ahead of every eighth stage-2 evaluation -- every
 * fourth / every one with more than 16 / 32 pieces -- i.e. within a millisecond or two; a workgroup before it takes another
 * candidate).  Returns at once (callable from another thread than the one in topay_synchronize). */
topay_status topay_cancel(topay_ctx* ctx);
topay_status topay_get_interrupted(topay_ctx* ctx, int* interrupted /* batch */);
/* The wall-clock knob of a planning call (max_replan_time, agent_benchmark_tables.yaml:6; the 1.0 s cap of the ALM loop,
 * moma_traj_opt.cpp:403-407, is of the same kind): topay_optimize_async, then topay_cancel if the batch has not finished
 * within budget_ms of wall time, then topay_synchronize.  Candidates that finished in time keep their results; the rest
 * return TOPAY_INTERRUPTED.  *timed_out (may be NULL) tells whether the cancel was needed.  Unlike the deterministic
 * budgets (alm_max_outer, alm_work_budget, topay_set_groups) the outcome depends on the machine and its load. */
topay_status topay_optimize_within(topay_ctx* ctx, double budget_ms, int* timed_out);

/* A planning call on an otherwise idle device (BASELINE configs[1]: 64 candidates of one scenario; planner.cpp:930-958 runs its
 * handful of candidates one after the other).  mode 1: a batch with at most one candidate per SIMD of the device (1024 on an MI355X: up
 * to there the longest candidate decides the time of the batch, measured) runs its candidates of up to 32 pieces on workgroups of
 * four waves -- the one-wave solver on the first, all four in every cost / gradient evaluation
 * (the sample passes of the two sweeps side by side).  Results are those of the default kernels bit for bit (the evaluation is
 * order-identical for any number of waves, the solver is the one-wave solver); what changes is the time of a solve.  mode 2: for
 * every batch (tests); mode 0 (the default): never.  Takes effect at the next topay_optimize / topay_optimize_async. */
topay_status topay_set_latency_mode(topay_ctx* ctx, int mode);

/* ---- multi-GPU: scenarios shard over the GPUs of a node (one process per GPU, nothing of the solve is shared); the one
 * exchange is the all-gather of a 32-byte record per scenario over RCCL (the reference's selection of
 * a scenario's winner, planner.cpp:999-1010, stays local).  A C++ planner shards with these four calls and no torch:
 *   rank 0: topay_comm_unique_id(&id), hands the 128 bytes to the other processes (file, pipe, ROS parameter ...);
 *   every rank: topay_comm_init(ctx, &id, world, rank); per step topay_scenario_records + topay_gather_records.
 * RCCL is bound at run time (librccl.so.1; TOPAY_RCCL_LIB overrides): TOPAY_ERR_UNSUPPORTED when it is not there. */
typedef struct { char internal[128]; } topay_comm_id_t;          /* == ncclUniqueId */
typedef struct {
  int scenario_id;      /* caller's id of the scenario (planning call) */
  int best_candidate;   /* index of the winner among the scenario's candidates, -1: none */
  int status;           /* 1: a candidate succeeded and passed the gate */
  int n_pieces;         /* pieces of the winner */
  double cost;          /* traj_cost of the winner */
  double duration;      /* total duration of the winner: what the planner ranks by */
} topay_record_t;
topay_status topay_comm_unique_id(topay_comm_id_t* id);
topay_status topay_comm_init(topay_ctx* ctx, const topay_comm_id_t* id, int world, int rank);
topay_status topay_comm_destroy(topay_ctx* ctx);
/* One record per scenario of the solved batch resident in ctx, in order of first appearance of its id in scenario_of
 * (batch entries); winner_index (may be NULL) receives the batch index of each scenario's winner or -1. */
topay_status topay_scenario_records(topay_ctx* ctx, const int* scenario_of, int cap_records, topay_record_t* records, int* n_records,
                                    int* winner_index);
/* ncclAllGather of per_rank records from every rank (n_mine <= per_rank valid ones); all[world x per_rank] receives them
 * in rank order with the valid ones compacted to the front, *n_valid their number.  Runs on a stream of its own. */
topay_status topay_gather_records(topay_ctx* ctx, const topay_record_t* mine, int n_mine, int per_rank, topay_record_t* all, int* n_valid);
/* The two halves of that exchange for a caller with a transport of its own (MPI, gloo, a ROS topic): the block a rank
 * contributes -- its n_mine records padded to per_rank entries with scenario_id = INT32_MIN -- and the reading of the
 * world x per_rank gathered entries: valid records compacted to the front of `all` in rank order, *n_valid their number,
 * the rest of `all` padding.  topay_gather_records is pack, ncclAllGather, unpack.  No device is touched. */
topay_status topay_pack_records(const topay_record_t* mine, int n_mine, int per_rank, topay_record_t* block);
topay_status topay_unpack_records(const topay_record_t* gathered, int world, int per_rank, topay_record_t* all, int* n_valid);

/* Launch class of a candidate with n_pieces pieces: the waves its SOLVER's vectors are divided over and the decision-vector
 * elements per thread of that solver.  For parity tooling: the rounding of the solver's dot products depends on how the
 * vectors are divided over the threads (an evaluation does not: it is order-identical for any number of waves).  Since
 * round 5 every class solves on one wave -- the long classes (more than 32 pieces) run their evaluations on four waves and
 * the solver on the first of them -- so *waves is 1 for every n_pieces.  Any output pointer may be NULL. */
topay_status topay_class_of(int n_pieces, int* waves, int* elements_per_thread, int* class_index);

/* topay_edt_test_plan (test hook): what the distance-field build (topay_build_esdf*) decides from the shape of n_maps maps of
 * dims = (nx, ny, nz) alone, as the 19 numbers out[0 .. 19).  No context and no device, like topay_class_of.
 *   out[0]       1: every dimension <= 512 cells, the exhaustive-search kernels; 0: the envelope kernel
 *   out[1]       first pass of the 3-D field: 16 / 32 / 64 = the ballot kernel of that line length, 0 = the direct kernel
 *   out[2..5)    lines per tile wy, wx, w2 of the y pass, the x pass and the 2-D x pass
 *   out[5..8)    dynamic LDS bytes of those tiles
 *   out[8..13)   per envelope pass (3-D z, y, x; 2-D y, x): 1 = stacks in LDS, 0 = in the HBM workspace
 *   out[13..18)  per envelope pass: LDS bytes of a block's stacks
 *   out[18]      workspace elements per map
 * out[1..8) describe the launches when out[0] is 1, out[8..19) when it is 0. */
topay_status topay_edt_test_plan(const int dims[3], int n_maps, long long* out);

/* Device memory (bytes) of the batch resident in the context: every block topay_set_init_traj sized.  The variable-length
 * blocks (L-BFGS history first of all) are packed by each candidate's own size, not strided by the longest member. */
topay_status topay_workspace_bytes(topay_ctx* ctx, unsigned long long* bytes);

/* Scheduling diagnostics: how often topay_optimize_async gave up waiting (120 s) for the previously issued batch to
 * become resident before issuing this context's batch (the dispatch gate only orders batches; results never depend on
 * it).  Non-zero means the device was stalled by something else; topay_last_error() then holds the message. */
topay_status topay_gate_timeouts(topay_ctx* ctx, int* n);

/* Device time (HIP events on the context's stream) of the last topay_optimize / topay_eval_batch
 * solve kernel(s), in milliseconds, and the number of launches it covered. */
topay_status topay_last_kernel_ms(topay_ctx* ctx, double* ms, int* launches);
/* How many of those launches ran on the helper-wave kernels (topay_set_latency_mode). */
topay_status topay_last_helper_launches(topay_ctx* ctx, int* n);

#ifdef __cplusplus
}
#endif
#endif /* TOPAY_H */
