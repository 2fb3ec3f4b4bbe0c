"""Host-side mirror of the reference's `MomaTrajOpt` surface over the C-ABI (include/topay.h).

The reference interface (src/planner/include/planner/moma_traj_opt.h:646-674) is one C++ object per
candidate thread: `optimizeTraj(init_path, boundary_vel, boundary_acc) -> bool`, then `getTraj()` and the
public `traj_cost`.  `MomaTrajOptBatch` keeps those names and argument meanings but takes a *batch* of
candidates (one 64-lane wavefront each on the GPU).

This module only binds `topay_amd/lib/libtopay_hip.so` (built by hipcc for gfx950).  There is no CPU
path: if the library is missing, or no HIP device is usable, it raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libtopay_hip.so")

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)


class LbfgsParams(C.Structure):
    _fields_ = [("mem_size", C.c_int), ("past", C.c_int), ("max_iterations", C.c_int), ("max_linesearch", C.c_int),
                ("g_epsilon", C.c_double), ("delta", C.c_double), ("min_step", C.c_double), ("max_step", C.c_double),
                ("f_dec_coeff", C.c_double), ("s_curv_coeff", C.c_double), ("cautious_factor", C.c_double),
                ("machine_prec", C.c_double)]


class Params(C.Structure):
    """topay_params_t — mirrors MomaTrajOptParam (moma_traj_opt.h:441-564) + MomaParam constants."""
    _fields_ = [
        ("int_K", C.c_int), ("min_piece_num", C.c_int), ("relu_mu", C.c_double), ("sample_interval", C.c_double),
        ("energy_weights", C.c_double * 9),
        ("s1_time_weight", C.c_double), ("s1_moment_weight", C.c_double), ("s1_acc_weight", C.c_double),
        ("s1_domega_weight", C.c_double), ("s1_path_pos_weight", C.c_double),
        ("s1_normal_past", C.c_int), ("s1_shot_path_past", C.c_int), ("s1_shot_path_horizon", C.c_double),
        ("s1_lbfgs", LbfgsParams),
        ("s2_time_weight", C.c_double), ("s2_moment_weight", C.c_double), ("s2_acc_weight", C.c_double),
        ("s2_domega_weight", C.c_double), ("s2_collision_weight", C.c_double), ("s2_mani_colli_weight", C.c_double),
        ("s2_self_colli_weight", C.c_double), ("s2_mani_pos_weight", C.c_double), ("s2_mani_vel_weight", C.c_double),
        ("s2_mani_acc_weight", C.c_double), ("s2_mean_time_weight", C.c_double),
        ("s2_lbfgs", LbfgsParams),
        ("alm_init_lambda", C.c_double * 2), ("alm_init_rho", C.c_double * 2), ("alm_rho_max", C.c_double * 2),
        ("alm_gamma", C.c_double * 2), ("alm_tolerance", C.c_double), ("alm_max_outer", C.c_int),
        ("alm_work_budget", C.c_int),
        ("chassis_height", C.c_double), ("chassis_colli_radius", C.c_double),
        ("max_v", C.c_double), ("max_a", C.c_double), ("max_w", C.c_double), ("max_dw", C.c_double),
        ("colli_length", C.c_double * 8), ("colli_points", C.c_double * 16), ("colli_point_radius", C.c_double * 16),
        ("joint_pos_limit_max", C.c_double * 7), ("joint_vel_limit", C.c_double * 7), ("joint_acc_limit", C.c_double * 7),
        ("relative_R", C.c_double * 9), ("relative_t", C.c_double * 3),
    ]


class MeshParams(C.Structure):
    """topay_mesh_params_t — the mesh kinematics of MomaParam (moma_param.h:60-67, 77-90, 114-115)."""
    _fields_ = [("link_length", C.c_double * 7), ("joint_pos_limit_min", C.c_double * 7), ("joint_offset", C.c_double * 21),
                ("joint_dof_axis", C.c_double * 21)]


class CommId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


class McrrtParams(C.Structure):
    """topay_mcrrt_params_t (include/topay.h): the search's parameters, deterministic caps and seed."""
    _fields_ = [("goal_sample_rate", C.c_double), ("check_colli_res", C.c_double), ("rs_turning_radius", C.c_double),
                ("max_iter", C.c_int), ("max_sample_tries", C.c_int), ("node_cap", C.c_int), ("reserved", C.c_int),
                ("seed", C.c_ulonglong)]


class TopoParams(C.Structure):
    """topay_topo_params_t (include/topay.h): the roadmap's parameters, deterministic caps and seed."""
    _fields_ = [("sample_inflate_x", C.c_double), ("sample_inflate_y", C.c_double), ("clearance", C.c_double),
                ("ratio_to_short", C.c_double), ("max_sample_num", C.c_int), ("max_raw_path", C.c_int), ("max_raw_path2", C.c_int),
                ("reserve_num", C.c_int), ("node_cap", C.c_int), ("reserved", C.c_int), ("seed", C.c_ulonglong)]


TOPO_MAX_NB = 32   # TOPAY_TOPO_MAX_NB


class PlanParams(C.Structure):
    """topay_plan_params_t (include/topay.h): the stages' parameters and the planner's constants of a planning call."""
    _fields_ = [("topo", TopoParams), ("mcrrt", McrrtParams), ("dense_step", C.c_double), ("jps_margin", C.c_double),
                ("cancel_budget", C.c_int), ("max_candidates", C.c_int), ("critical_retry", C.c_int), ("reserved", C.c_int)]


# The rows of plan_calls' tables by name: the enums TOPAY_PLAN_RES_*, TOPAY_PLAN_STAGE_* and TOPAY_PLAN_MS_* of include/topay.h
# (tests/test_plan.py holds the lists to them).
PLAN_RESULT_KEYS = ["status", "try", "candidates0", "candidates1", "winner", "n_pieces", "topo_status", "winner_batch_index"]
PLAN_STAGES = ["absent", "search_failed", "too_many_pieces", "solver_failed", "gate_failed", "interrupted", "counts"]
PLAN_STAGE_MS_KEYS = ["roadmap", "jps", "dense", "search", "init", "solve", "gate_winner", "store"]


class WorldParams(C.Structure):
    """topay_world_params_t (include/topay.h): the world generator's parameters (params/map_tables.yaml, map_cuboids.yaml)."""
    _fields_ = [("kind", C.c_int), ("obs_num", C.c_int * 2), ("size_xy", C.c_double), ("size_z", C.c_double), ("resolution", C.c_double),
                ("cloud_resolution", C.c_double), ("wall_size_range", C.c_double * 2), ("wall_height_range", C.c_double * 2),
                ("float_size_range", C.c_double * 2), ("float_height_range", C.c_double * 2), ("desk_length_range", C.c_double * 2),
                ("desk_width_range", C.c_double * 2), ("desk_height_range", C.c_double * 2), ("desk_arrangement_range", C.c_int * 2),
                ("reserved", C.c_int)]


class EeParams(C.Structure):
    """topay_ee_params_t (include/topay.h): L-BFGS block, weights of eeCostCallback, what topay_ee_select asks of a goal."""
    _fields_ = [("lbfgs", LbfgsParams), ("cost_scale", C.c_double), ("mani_colli_weight", C.c_double), ("self_colli_weight", C.c_double),
                ("clearance_factor", C.c_double), ("pose_tol", C.c_double), ("require_collision_free", C.c_int), ("reserved", C.c_int)]


class SenseParams(C.Structure):
    """topay_sense_params_t (include/topay.h): ProbMap's parameters (params/rog_map.yaml) and the chassis height of the 2-D rule."""
    _fields_ = [("p_min", C.c_float), ("p_miss", C.c_float), ("p_free", C.c_float), ("p_occ", C.c_float), ("p_hit", C.c_float),
                ("p_max", C.c_float), ("ray_range", C.c_double * 2), ("point_filt_num", C.c_int), ("batch_update_size", C.c_int),
                ("intensity_thresh", C.c_int), ("reserved", C.c_int), ("virtual_ceil_height", C.c_double),
                ("virtual_ground_height", C.c_double), ("local_update_box", C.c_double * 3), ("chassis_height", C.c_double)]


class SenseSlideParams(C.Structure):
    """topay_sense_slide_params_t (include/topay.h): map_sliding/threshold of params/rog_map.yaml and whether z slides."""
    _fields_ = [("threshold", C.c_double), ("slide_z", C.c_int), ("reserved", C.c_int)]


class MpcParams(C.Structure):
    """topay_mpc_params_t (include/topay.h): the ompc/ keys of params/mpc.yaml and the QP solver's knobs."""
    _fields_ = [("du_threshold", C.c_double), ("dt", C.c_double), ("ctrl_freq", C.c_double), ("max_iter", C.c_int),
                ("predict_steps", C.c_int), ("delay_num_v", C.c_int), ("delay_num_w", C.c_int), ("max_omega", C.c_double),
                ("max_domega", C.c_double), ("max_speed", C.c_double), ("min_speed", C.c_double), ("max_accel", C.c_double),
                ("matrix_q", C.c_double * 3), ("matrix_r", C.c_double * 2), ("matrix_rd", C.c_double * 2), ("qp_eps_abs", C.c_double),
                ("qp_eps_rel", C.c_double), ("qp_rho", C.c_double), ("qp_sigma", C.c_double), ("qp_alpha", C.c_double),
                ("qp_max_iter", C.c_int), ("reserved", C.c_int)]


MPC_MAX_STEPS = 128          # TOPAY_MPC_MAX_STEPS
MPC_ST_KEYS = ["outcome", "outer", "qp_iters", "mode"]   # TOPAY_MPC_ST_*
c_fp = C.POINTER(C.c_float)
SENSE_LAST_SCAN = "last_scan"   # sense_insert: the points of the last sense_scan, on the device (TOPAY_SENSE_LAST_SCAN)
SENSE_MS_KEYS = ["scan", "insert", "flush", "commit"]
c_u64p = C.POINTER(C.c_ulonglong)
c_i8p = C.POINTER(C.c_int8)
WORLD_STAGE_MS_KEYS = ["generation", "rasterisation", "fields", "sampling"]


class Record(C.Structure):
    """topay_record_t: the 32-byte per-scenario record of the multi-GPU exchange."""
    _fields_ = [("scenario_id", C.c_int), ("best_candidate", C.c_int), ("status", C.c_int), ("n_pieces", C.c_int),
                ("cost", C.c_double), ("duration", C.c_double)]


class MapDesc(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("resolution", C.c_double), ("dims", C.c_int * 3),
                ("min_boundary", C.c_double * 3), ("max_boundary", C.c_double * 3)]


class TopayError(RuntimeError):
    pass


_libs = {}


def load(path=None):
    """Load the C-ABI library.  Default: the hipcc-built product library; raises if it is missing."""
    path = os.path.abspath(path or os.environ.get("TOPAY_LIB") or DEFAULT_LIB)   # TOPAY_LIB: diagnostic A/B of two builds
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise TopayError(
            f"{path} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
            "topay_amd has no CPU fallback.")
    L = C.CDLL(path)
    L.topay_last_error.restype = C.c_char_p
    L.topay_default_params.argtypes = [C.POINTER(Params)]
    L.topay_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
    L.topay_destroy.argtypes = [C.c_void_p]
    L.topay_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
    L.topay_default_mesh_params.argtypes = [C.POINTER(MeshParams)]
    L.topay_mesh_poses.argtypes = [C.c_void_p, C.POINTER(MeshParams), C.c_int, c_dp, c_dp]
    L.topay_mesh_traj.argtypes = [C.c_void_p, C.c_int, C.POINTER(MeshParams), C.c_int, C.c_int, c_dp, c_dp, c_dp, c_ip]
    L.topay_set_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapDesc), c_dp, c_dp]
    L.topay_set_init_traj.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_dp, c_ip]
    L.topay_reset.argtypes = [C.c_void_p]
    L.topay_optimize.argtypes = [C.c_void_p]
    L.topay_optimize_async.argtypes = [C.c_void_p]
    L.topay_synchronize.argtypes = [C.c_void_p]
    L.topay_get_batch.argtypes = [C.c_void_p, c_ip, c_dp, c_ip]
    L.topay_get_result.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_ip, c_dp, c_dp, c_dp]
    L.topay_get_results.argtypes = [C.c_void_p, C.c_int, c_ip, C.c_int, c_ip, c_dp, c_dp, c_dp]
    L.topay_get_polytraj_msg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.POINTER(C.c_int8), c_ip]
    L.topay_mcrrt_default_params.argtypes = [C.POINTER(McrrtParams)]
    L.topay_mcrrt_default_params.restype = None
    L.topay_mcrrt_plan.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, C.POINTER(McrrtParams), C.c_ulonglong, C.c_int, c_ip, c_dp,
                                   c_ip, c_dp]
    L.topay_mcrrt_nodes.argtypes = [C.c_void_p, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_dp, c_dp]
    L.topay_topo_default_params.argtypes = [C.POINTER(TopoParams)]
    L.topay_topo_default_params.restype = None
    L.topay_topo_paths.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_ip, C.POINTER(TopoParams), C.c_ulonglong, C.c_int, C.c_int, c_ip, c_ip,
                                   c_dp, c_ip]
    L.topay_topo_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, c_ip, c_ip, c_dp, c_ip, c_ip, c_ip]
    L.topay_topo_raw_paths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, c_ip, c_dp]
    if hasattr(L, "topay_plan_calls"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_plan_default_params.argtypes = [C.POINTER(PlanParams)]
        L.topay_plan_default_params.restype = None
        L.topay_plan_calls.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_dp, C.POINTER(PlanParams), C.c_ulonglong, c_ip, c_ip, c_dp]
        L.topay_plan_get_trajs.argtypes = [C.c_void_p, C.c_int, c_ip, C.c_int, c_ip, c_dp, c_dp, c_dp]
        L.topay_plan_get_front_path.argtypes = [C.c_void_p, C.c_int, C.c_int, c_ip, c_dp]
        L.topay_plan_stage_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_plan_test_chunk.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "topay_replan_calls"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_track_set.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp, C.c_int, c_dp, c_dp]
        L.topay_track_commit_plan.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, C.c_int, c_ip]
        L.topay_track_get.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_ip, c_dp, c_dp, c_dp]
        L.topay_track_clear.argtypes = [C.c_void_p, C.c_int]
        L.topay_track_safe.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, c_ip, c_ip, c_dp]
        L.topay_track_safe_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_replan_inputs.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_dp, C.c_double, C.c_double, c_dp, c_dp, c_dp, c_ip]
        L.topay_replan_calls.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp, C.c_double, C.c_double, C.c_double,
                                         C.POINTER(PlanParams), C.c_ulonglong, c_ip, c_dp, c_ip, c_ip]
    if hasattr(L, "topay_track_sample"):   # (older builds of the library under tools/libs, A/B runs)
        # the outputs as addresses: a numpy array's or a device tensor's
        outs = [C.c_void_p] * 7
        L.topay_track_sample.argtypes = [C.c_void_p, C.c_int, c_ip, C.c_int, c_ip, c_ip, c_dp, C.c_int] + outs
        L.topay_track_sample_grid.argtypes = [C.c_void_p, C.c_int, c_ip, C.c_int, c_ip, c_dp, C.c_double, C.c_int, C.c_int] + outs
        L.topay_track_sample_ms.argtypes = [C.c_void_p, c_dp]
    if hasattr(L, "topay_ee_goals"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_ee_default_params.argtypes = [C.POINTER(EeParams)]
        L.topay_ee_default_params.restype = None
        L.topay_ee_pose.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp]
        L.topay_ee_eval.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_dp, c_dp]
        L.topay_ee_goals.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, C.POINTER(EeParams), c_dp, c_dp, c_ip, c_ip, c_ip]
        L.topay_ee_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_ee_select.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, C.c_int, c_dp, c_dp, c_ip, c_dp, C.POINTER(EeParams), c_ip, c_dp]
    L.topay_reeds_shepp.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp, c_dp, C.c_double, c_dp, c_ip, c_dp, c_dp]
    L.topay_dense_path.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.c_double, c_dp, c_dp, C.c_double, C.c_double, C.c_int, c_ip, c_dp]
    L.topay_connect_check_num.argtypes = [C.c_int, c_dp, c_dp, c_dp, C.c_double, c_ip]
    L.topay_connect_collision.argtypes = [C.c_void_p, C.c_int, C.c_int, c_ip, c_dp, c_dp, c_dp, c_ip]
    L.topay_get_stats.argtypes = [C.c_void_p, c_ip]
    L.topay_get_alm.argtypes = [C.c_void_p, c_dp]
    L.topay_whole_body_collision.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp, c_ip]
    L.topay_playback.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp, c_dp, C.c_int, c_dp, c_ip]
    L.topay_build_esdf.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapDesc), C.POINTER(C.c_int8), C.POINTER(C.c_int8)]
    L.topay_get_map.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp, c_dp]
    L.topay_build_esdf_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MapDesc), C.POINTER(C.c_int8),
                                         C.POINTER(C.c_int8)]
    L.topay_build_esdf_fields.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MapDesc), C.POINTER(C.c_int8), C.POINTER(C.c_int8),
                                          C.POINTER(C.c_int8)]
    L.topay_get_map_fields.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp]
    if hasattr(L, "topay_edt_test_plan"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_edt_test_plan.argtypes = [c_ip, C.c_int, C.POINTER(C.c_longlong)]
    if hasattr(L, "topay_generate_worlds"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_world_default_params.argtypes = [C.c_int, C.POINTER(WorldParams)]
        L.topay_generate_worlds.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(WorldParams), c_u64p, c_dp, c_ip]
        L.topay_get_occupancy.argtypes = [C.c_void_p, C.c_int, c_i8p, c_i8p, c_i8p]
        L.topay_world_last_path.argtypes = [C.c_void_p, c_ip]
        L.topay_world_test_path.argtypes = [C.c_void_p, C.c_int]
        L.topay_world_test_max_tries.argtypes = [C.c_void_p, C.c_int]
        L.topay_world_stage_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_sample_start_goal_xy.argtypes = [C.c_int, c_u64p, C.c_double, c_dp, c_dp]
        L.topay_sample_arm.argtypes = [C.c_void_p, C.c_int, c_ip, c_u64p, C.c_int, c_dp, c_ip, c_ip]
        L.topay_sample_scenarios.argtypes = [C.c_void_p, C.c_int, c_ip, c_u64p, c_dp, c_dp, c_ip]
        L.topay_generate_episodes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(WorldParams), c_u64p, c_ip, c_dp, c_dp, c_ip]
        L.topay_test_mt64.argtypes = [C.c_ulonglong, C.c_int, C.c_int, c_u64p]
    if hasattr(L, "topay_sense_insert"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_sense_default_params.argtypes = [C.POINTER(SenseParams)]
        L.topay_sense_logodds.argtypes = [C.POINTER(SenseParams), c_fp]
        L.topay_sense_reset.argtypes = [C.c_void_p, C.c_int, c_ip, C.POINTER(MapDesc)]
        L.topay_sense_insert.argtypes = [C.c_void_p, C.c_int, c_ip, c_ip, C.c_void_p, c_dp, C.POINTER(SenseParams), c_ip]
        L.topay_sense_commit.argtypes = [C.c_void_p, C.c_int, c_ip]
        L.topay_sense_get.argtypes = [C.c_void_p, C.c_int, c_fp, c_ip, c_ip, c_ip]
        L.topay_sense_scan.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, c_ip, c_fp]
        L.topay_sense_ms.argtypes = [C.c_void_p, c_dp]
    if hasattr(L, "topay_sense_slide"):
        L.topay_sense_slide_default_params.argtypes = [C.POINTER(SenseSlideParams)]
        L.topay_sense_slide.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.POINTER(SenseSlideParams), c_ip, c_ip]
        L.topay_sense_slide_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_sense_get_desc.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapDesc)]
    if hasattr(L, "topay_mpc_cmds"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_mpc_default_params.argtypes = [C.POINTER(MpcParams)]
        L.topay_mpc_qp_dims.argtypes = [C.POINTER(MpcParams), c_ip, c_ip]
        L.topay_mpc_reset.argtypes = [C.c_void_p, C.c_int, c_ip, C.POINTER(MpcParams)]
        L.topay_mpc_set_direct.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp]
        L.topay_mpc_cmds.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, c_dp, c_ip, c_dp]
        L.topay_mpc_probe.argtypes = [C.c_void_p, C.c_int, C.c_double, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip]
        L.topay_mpc_get_state.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp, c_ip]
        L.topay_mpc_ms.argtypes = [C.c_void_p, c_dp]
        L.topay_sim_reset.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.c_int]
        L.topay_sim_step.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.c_int, c_dp]
        L.topay_track_follow.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, C.c_int, C.c_int, c_dp, c_dp, c_ip]
    L.topay_get_total_durations.argtypes = [C.c_void_p, c_dp]
    L.topay_check_feasible.argtypes = [C.c_void_p, c_ip]
    L.topay_feasibility_report.argtypes = [C.c_void_p, c_ip, c_ip, c_dp]
    L.topay_get_elapsed_us.argtypes = [C.c_void_p, c_dp, c_dp, c_ip]
    L.topay_get_x.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp]
    L.topay_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]
    L.topay_load_solution.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp, c_dp]
    L.topay_gate_timeouts.argtypes = [C.c_void_p, c_ip]
    L.topay_class_of.argtypes = [C.c_int, c_ip, c_ip, c_ip]
    L.topay_set_groups.argtypes = [C.c_void_p, c_ip, C.c_int]
    if hasattr(L, "topay_set_latency_mode"):   # (older builds of the library under tools/libs, A/B runs)
        L.topay_set_latency_mode.argtypes = [C.c_void_p, C.c_int]
    L.topay_comm_unique_id.argtypes = [C.POINTER(CommId)]
    L.topay_comm_init.argtypes = [C.c_void_p, C.POINTER(CommId), C.c_int, C.c_int]
    L.topay_comm_destroy.argtypes = [C.c_void_p]
    L.topay_scenario_records.argtypes = [C.c_void_p, c_ip, C.c_int, C.POINTER(Record), c_ip, c_ip]
    L.topay_gather_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_int, C.c_int, C.POINTER(Record), c_ip]
    L.topay_cancel.argtypes = [C.c_void_p]
    L.topay_get_interrupted.argtypes = [C.c_void_p, c_ip]
    L.topay_workspace_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.topay_eval_waves.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]
    L.topay_eval_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp]
    L.topay_get_nmax.argtypes = [C.c_void_p, c_ip, c_ip]
    L.topay_check_feasible.argtypes = [C.c_void_p, c_ip]
    L.topay_last_kernel_ms.argtypes = [C.c_void_p, c_dp, c_ip]
    if hasattr(L, "topay_last_helper_launches"):
        L.topay_last_helper_launches.argtypes = [C.c_void_p, c_ip]
    L.topay_test_math.argtypes = [C.c_void_p, C.c_int, c_dp, c_dp, c_dp]
    L.topay_set_trace.argtypes = [C.c_void_p, C.c_int]
    L.topay_get_trace.argtypes = [C.c_void_p, C.c_int, c_dp]
    _libs[path] = L
    return L


def default_params(lib=None):
    L = lib or load()
    p = Params()
    _chk(L, L.topay_default_params(C.byref(p)))
    return p


def _u64(a):
    """Seeds as 64-bit words (Python integers of any size wrap around like the harness's uint64_t arithmetic)."""
    if isinstance(a, np.ndarray):
        a = a.tolist()                        # (a list of mixed magnitudes would become float64 in numpy: convert item by item)
    if not isinstance(a, (list, tuple)):
        a = [a]
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in a], dtype=np.uint64)


def world_params(kind, size_xy=20.0, size_z=1.6, resolution=0.1, cloud_resolution=0.05, lib=None, **kw):
    """WorldParams of the tables (0) / cuboids (1) world with the obstacle counts scaled by the area as World::build does
    (workload.hpp:689-691): round(40 | 80 x size_xy^2 / 400), round(80 x ...).  kw: any other field, set last."""
    L = lib or load()
    p = WorldParams()
    _chk(L, L.topay_world_default_params(int(kind), C.byref(p)))
    p.size_xy, p.size_z, p.resolution, p.cloud_resolution = float(size_xy), float(size_z), float(resolution), float(cloud_resolution)
    area_scale = (p.size_xy * p.size_xy) / (20.0 * 20.0)
    for k in range(2):
        v = p.obs_num[k] * area_scale
        p.obs_num[k] = int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))   # lround: halves away from zero
    for k, v in kw.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            for i, x in enumerate(v):
                getattr(p, k)[i] = x
        else:
            setattr(p, k, v)
    return p


def sample_start_goal_xy(seeds, size_xy=20.0, lib=None):
    """World::sampleStartGoalXY for every seed (host only): (start [n, 3], goal [n, 3])."""
    L = lib or load()
    sd = _u64(seeds)
    s3, g3 = np.zeros((len(sd), 3)), np.zeros((len(sd), 3))
    _chk(L, L.topay_sample_start_goal_xy(len(sd), sd.ctypes.data_as(c_u64p), float(size_xy), _dp(s3), _dp(g3)))
    return s3, g3


def edt_plan(dims, n_maps=1, lib=None):
    """What the distance-field build decides from the shape of n_maps maps of dims = (nx, ny, nz) alone (edt_plan of topay_edt.h through
    the test hook topay_edt_test_plan; host arithmetic, no device).  family "small": the first pass ("ballot16" / "ballot32" /
    "ballot64" / "direct"), the tile widths wy, wx, w2 and the LDS bytes lds_y, lds_x, lds_2 of their tiles.  family "envelope": the
    k_edt_pass instance <SRC,FIN,WS> of the passes z, y, x (3-D) and y2, x2 (2-D) -- WS 1: stacks in LDS -- and lds_y, the stack bytes
    of the 3-D y pass."""
    L = lib or load()
    out = (C.c_longlong * 19)()
    _chk(L, L.topay_edt_test_plan((C.c_int * 3)(*[int(d) for d in dims]), int(n_maps), out))
    if out[0]:
        return dict(family="small", first=f"ballot{out[1]}" if out[1] else "direct", wy=out[2], wx=out[3], w2=out[4],
                    lds_y=out[5], lds_x=out[6], lds_2=out[7])
    ws = out[8:13]
    return dict(family="envelope", z=f"<0,0,{ws[0]}>", y=f"<1,0,{ws[1]}>", x=f"<1,1,{ws[2]}>", y2=f"<0,0,{ws[3]}>", x2=f"<1,1,{ws[4]}>",
                lds_y=out[14])


def test_mt64(seed, skip, n, lib=None):
    """Outputs skip .. skip + n - 1 of mt19937_64(seed), generated on the device (test hook)."""
    L = lib or load()
    out = np.zeros(n, dtype=np.uint64)
    _chk(L, L.topay_test_mt64(int(seed) & 0xFFFFFFFFFFFFFFFF, int(skip), int(n), out.ctypes.data_as(c_u64p)))
    return out


def params_from_yaml(source, base=None, lib=None):
    """== MomaTrajOpt::init (moma_traj_opt.h:845-941): the optimiser parameters from the reference's parameter file
    (src/planner/params/optimizer.yaml: `planner_node: moma_traj_opt: ...`, the keys init() reads from the parameter
    server).  `source` is a path, a YAML text or an already parsed mapping; keys that are absent keep the value of
    `base` (default: topay_default_params).  Returns (Params, ignored): `ignored` lists the keys the reference reads
    but this path has no use for -- mean_time_lowb / mean_time_uppb (the reference's penalty uses the literals 0.5 and
    2.0, moma_traj_opt.cpp:1752-1769), first_stage/mean_time_weight (stage 1 has no mean-time term), alm_data/* (read
    into a struct optimizeTraj never consults) -- and any key init() does not know."""
    import yaml

    if isinstance(source, dict):
        doc = source
    else:
        text = open(source).read() if os.path.exists(str(source)) else str(source)
        doc = yaml.safe_load(text) or {}
    for k in ("planner_node", "moma_traj_opt"):
        if isinstance(doc, dict) and k in doc:
            doc = doc[k]
    p = Params()
    if base is not None:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(Params))
    else:
        _chk(lib or load(), (lib or load()).topay_default_params(C.byref(p)))
    ignored = []

    def vec(dst, src, n):
        for i in range(min(n, len(src))):
            dst[i] = float(src[i])

    def lbfgs(dst, m, prefix):
        for k, v in m.items():
            if k in ("mem_size", "past", "max_iterations"):
                setattr(dst, k, int(v))
            elif k in ("g_epsilon", "min_step", "delta"):
                setattr(dst, k, float(v))
            else:
                ignored.append(prefix + k)

    for k, v in (doc or {}).items():
        if k in ("int_K", "min_piece_num"):
            setattr(p, k, int(v))
        elif k in ("relu_mu", "sample_interval"):
            setattr(p, k, float(v))
        elif k == "energy_weights":
            vec(p.energy_weights, v, 9)
        elif k == "first_stage":
            for kk, vv in v.items():
                if kk in ("time_weight", "moment_weight", "acc_weight", "domega_weight", "path_pos_weight"):
                    setattr(p, "s1_" + kk, float(vv))
                elif kk == "lbgfs_normal_past":          # (sic) also becomes the stage-1 `past`, moma_traj_opt.h:873
                    p.s1_normal_past = int(vv)
                    p.s1_lbfgs.past = int(vv)
                elif kk == "lbgfs_shot_path_past":
                    p.s1_shot_path_past = int(vv)
                elif kk == "shot_path_horizon":
                    p.s1_shot_path_horizon = float(vv)
                elif kk == "lbfgs":
                    lbfgs(p.s1_lbfgs, {a: b for a, b in vv.items() if a != "past"}, "first_stage/lbfgs/")
                    if "past" in vv:
                        ignored.append("first_stage/lbfgs/past")
                else:
                    ignored.append("first_stage/" + kk)
        elif k == "second_stage":
            for kk, vv in v.items():
                if kk in ("time_weight", "moment_weight", "acc_weight", "domega_weight", "collision_weight", "mani_colli_weight",
                          "self_colli_weight", "mani_pos_weight", "mani_vel_weight", "mani_acc_weight", "mean_time_weight"):
                    setattr(p, "s2_" + kk, float(vv))
                elif kk == "lbfgs":
                    lbfgs(p.s2_lbfgs, vv, "second_stage/lbfgs/")
                elif kk == "alm_param":
                    for a, b in vv.items():       # the reference sizes these vectors 9 and uses entries 0 and 1 (end-point x, y)
                        if a in ("init_lambda", "init_rho", "rho_max", "gamma"):
                            vec(getattr(p, "alm_" + a), b, 2)
                        elif a == "tolerance":
                            p.alm_tolerance = float(b[0])
                        else:
                            ignored.append("second_stage/alm_param/" + a)
                else:
                    ignored.extend(f"second_stage/{kk}/{a}" for a in vv) if isinstance(vv, dict) else ignored.append("second_stage/" + kk)
        else:
            ignored.append(k)
    return p, ignored


def params_from_yaml_c(source, base=None, lib=None):
    """The library's own loader (topay_params_from_yaml, for C / C++ callers): same mapping as params_from_yaml."""
    L = lib or load()
    p = Params()
    if base is not None:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(Params))
    else:
        _chk(L, L.topay_default_params(C.byref(p)))
    buf = C.create_string_buffer(4096)
    L.topay_params_from_yaml.argtypes = [C.c_char_p, C.POINTER(Params), C.c_char_p, C.c_int]
    _chk(L, L.topay_params_from_yaml(str(source).encode(), C.byref(p), buf, 4096))
    ign = buf.value.decode()
    return p, ([x for x in ign.split("\n") if x] if ign else [])


def pack_records(records, per_rank, lib=None):
    """A rank's block of the record exchange (topay_pack_records): its records padded to per_rank entries whose
    scenario_id is INT32_MIN.  No device involved."""
    L = load(lib)
    rec = np.ascontiguousarray(records)
    out = (Record * per_rank)()
    L.topay_pack_records.argtypes = [C.POINTER(Record), C.c_int, C.c_int, C.POINTER(Record)]
    _chk(L, L.topay_pack_records(rec.ctypes.data_as(C.POINTER(Record)), len(rec), per_rank, out))
    return np.ctypeslib.as_array(out).copy()


def unpack_records(gathered, world, per_rank, lib=None):
    """The valid records of world x per_rank gathered entries, in rank order (topay_unpack_records)."""
    L = load(lib)
    g = np.ascontiguousarray(gathered)
    out = (Record * (per_rank * world))()
    nv = C.c_int(0)
    L.topay_unpack_records.argtypes = [C.POINTER(Record), C.c_int, C.c_int, C.POINTER(Record), C.POINTER(C.c_int)]
    _chk(L, L.topay_unpack_records(g.ctypes.data_as(C.POINTER(Record)), world, per_rank, out, C.byref(nv)))
    return np.ctypeslib.as_array(out)[:nv.value].copy()


def _chk(L, status):
    if status != 0:
        raise TopayError(f"topay status {status}: {L.topay_last_error().decode()}")


def _dp(a):
    return a.ctypes.data_as(c_dp) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(c_ip) if a is not None else None


# TOPAY_SAMPLE_* of include/topay.h; the outputs of track_sample as (name, bit, shape of a row)
SAMPLE_STATE, SAMPLE_DSTATE, SAMPLE_EE_POSE, SAMPLE_CLEARANCE, SAMPLE_CENTRES, SAMPLE_DISTANCE = 1, 2, 4, 8, 16, 32
SAMPLE_OUTPUTS = (("state", SAMPLE_STATE, (10,)), ("dstate", SAMPLE_DSTATE, (10,)), ("ee_pose", SAMPLE_EE_POSE, (9,)),
                  ("clearance", SAMPLE_CLEARANCE, (13,)), ("centres", SAMPLE_CENTRES, (12, 3)), ("distance", SAMPLE_DISTANCE, (13,)))

STAT_KEYS = ["stage1_ret", "stage1_iters", "stage1_evals", "stage2_last_ret", "stage2_iters", "stage2_evals",
             "alm_outer", "sum_bound"]


class MomaTrajOptBatch:
    """Batched stand-in for `MomaTrajOpt` (reference: moma_traj_opt.h:613-674)."""

    def __init__(self, params=None, device=0, lib_path=None):
        self.L = load(lib_path)
        self.opt_param = params if params is not None else default_params(self.L)
        h = C.c_void_p()
        _chk(self.L, self.L.topay_create(C.byref(self.opt_param), device, C.byref(h)))
        self.h = h
        self.batch = 0
        self.traj_cost = None
        self._map_dims = {}
        self._plan_pieces = None

    def close(self):
        if getattr(self, "h", None):
            self.L.topay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- MomaTrajOpt(GridMap::Ptr): the shared read-only map
    def set_map(self, origin, resolution, dims, min_boundary, max_boundary, esdf2d, esdf3d, map_id=0):
        d = MapDesc()
        for i in range(3):
            d.origin[i] = origin[i]
            d.dims[i] = int(dims[i])
            d.min_boundary[i] = min_boundary[i]
            d.max_boundary[i] = max_boundary[i]
        d.resolution = resolution
        e2 = np.ascontiguousarray(esdf2d, dtype=np.float64)
        e3 = np.ascontiguousarray(esdf3d, dtype=np.float64)
        _chk(self.L, self.L.topay_set_map(self.h, map_id, C.byref(d), _dp(e2), _dp(e3)))
        self._map_dims[map_id] = tuple(int(x) for x in dims)

    # -- optimizeTraj lines 146-357
    def set_init_traj(self, path_len, init_paths, boundary_vel=None, boundary_acc=None, map_ids=None):
        pl = np.ascontiguousarray(path_len, dtype=np.int32)
        ip = np.ascontiguousarray(init_paths, dtype=np.float64)
        bv = None if boundary_vel is None else np.ascontiguousarray(boundary_vel, dtype=np.float64)
        ba = None if boundary_acc is None else np.ascontiguousarray(boundary_acc, dtype=np.float64)
        mi = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        self.batch = len(pl)
        _chk(self.L, self.L.topay_set_init_traj(self.h, self.batch, _ip(pl), _dp(ip), _dp(bv), _dp(ba), _ip(mi)))

    def reset(self):
        _chk(self.L, self.L.topay_reset(self.h))

    # -- optimizeTraj lines 359-497; returns the per-candidate bool of the reference
    def optimize(self):
        _chk(self.L, self.L.topay_optimize(self.h))
        succ = np.zeros(self.batch, dtype=np.int32)
        cost = np.zeros(self.batch)
        _chk(self.L, self.L.topay_get_batch(self.h, _ip(succ), _dp(cost), None))
        self.traj_cost = cost
        return succ.astype(bool)

    def optimize_within(self, budget_ms):
        """optimize with a wall-clock budget (topay_optimize_within): (success flags, timed_out)."""
        to = C.c_int(0)
        self.L.topay_optimize_within.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int)]
        _chk(self.L, self.L.topay_optimize_within(self.h, float(budget_ms), C.byref(to)))
        return self.finish(), bool(to.value)

    def optimize_async(self):
        """Issue the solve without waiting (several contexts may be in flight on one GPU); pair with finish()."""
        _chk(self.L, self.L.topay_optimize_async(self.h))

    def finish(self):
        """Wait for optimize_async and fetch the per-candidate results, like optimize()."""
        _chk(self.L, self.L.topay_synchronize(self.h))
        succ = np.zeros(self.batch, dtype=np.int32)
        cost = np.zeros(self.batch)
        _chk(self.L, self.L.topay_get_batch(self.h, _ip(succ), _dp(cost), None))
        self.traj_cost = cost
        return succ.astype(bool)

    def optimizeTraj(self, path_len, init_paths, boundary_vel=None, boundary_acc=None, map_ids=None):
        self.set_init_traj(path_len, init_paths, boundary_vel, boundary_acc, map_ids)
        return self.optimize()

    def n_pieces(self):
        n = np.zeros(self.batch, dtype=np.int32)
        _chk(self.L, self.L.topay_get_batch(self.h, None, None, _ip(n)))
        return n

    # -- getTraj()
    def getTraj(self, i):
        n = C.c_int(0)
        _chk(self.L, self.L.topay_get_result(self.h, i, None, None, C.byref(n), None, None, None))
        N = n.value
        dur = np.zeros(N)
        coef = np.zeros(N * 54)
        knots = np.zeros((N + 1) * 2)
        succ = C.c_int(0)
        cost = C.c_double(0)
        _chk(self.L, self.L.topay_get_result(self.h, i, C.byref(succ), C.byref(cost), None, _dp(dur), _dp(coef), _dp(knots)))
        return dict(success=bool(succ.value), cost=cost.value, durations=dur, coeffs=coef.reshape(N, 9, 6),
                    knots_xy=knots.reshape(N + 1, 2))

    def getTrajs(self, idx, n_pieces=None):
        """getTraj() of a selection of candidates in one call / one copy (the planner's winners): dict of packed arrays
        piece_off[n+1], durations[P], coeffs[P, 9, 6], knots_xy[P + n, 2] (candidate k's knots start at piece_off[k] + k)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        n = len(idx)
        npc = self.n_pieces() if n_pieces is None else n_pieces
        cap = int(npc[idx].sum()) if n else 0
        off = np.zeros(n + 1, dtype=np.int32)
        dur = np.zeros(cap)
        coef = np.zeros(cap * 54)
        kn = np.zeros(2 * (cap + n))
        _chk(self.L, self.L.topay_get_results(self.h, n, _ip(idx), cap, _ip(off), _dp(dur), _dp(coef), _dp(kn)))
        return dict(piece_off=off, durations=dur, coeffs=coef.reshape(cap, 9, 6), knots_xy=kn.reshape(cap + n, 2))

    def polytraj_msg(self, i):
        """Candidate i in the field layout of planner/msg/PolyTraj.msg: (order, coeff[N, 9, 6] f32, durations[N] f32, directions[N] i8)."""
        N = int(self.n_pieces()[i])
        order = C.c_ubyte(0)
        coef = np.zeros(max(N, 1) * 54, dtype=np.float32)
        dur = np.zeros(max(N, 1), dtype=np.float32)
        dirs = np.zeros(max(N, 1), dtype=np.int8)
        n = C.c_int(0)
        _chk(self.L, self.L.topay_get_polytraj_msg(self.h, i, max(N, 1), C.byref(order), coef.ctypes.data_as(C.POINTER(C.c_float)),
                                                   dur.ctypes.data_as(C.POINTER(C.c_float)), dirs.ctypes.data_as(C.POINTER(C.c_int8)),
                                                   C.byref(n)))
        return order.value, coef[:N * 54].reshape(N, 9, 6), dur[:N], dirs[:N]

    def stats(self):
        s = np.zeros(self.batch * 8, dtype=np.int32)
        _chk(self.L, self.L.topay_get_stats(self.h, _ip(s)))
        return s.reshape(self.batch, 8)

    def check_feasible(self, report=False):
        """printConstraintsSituations for every candidate (bool array); with report=True also checkFeasible's verdict
        and the 38 extreme values per candidate."""
        f = np.zeros(self.batch, dtype=np.int32)
        if not report:
            _chk(self.L, self.L.topay_check_feasible(self.h, _ip(f)))
            return f.astype(bool)
        st = np.zeros(self.batch, dtype=np.int32)
        rep = np.zeros(self.batch * 38)
        _chk(self.L, self.L.topay_feasibility_report(self.h, _ip(f), _ip(st), _dp(rep)))
        return f.astype(bool), st.astype(bool), rep.reshape(self.batch, 38)

    def total_durations(self):
        """Total duration of every candidate's trajectory (what the planner ranks successful candidates by)."""
        t = np.zeros(self.batch)
        _chk(self.L, self.L.topay_get_total_durations(self.h, _dp(t)))
        return t

    def build_esdf(self, origin, res, dims, min_b, max_b, occ2d, occ3d, map_id=0):
        """GridMap::updateESDF on the device from the occupancy grids; the slot is then usable like after set_map."""
        d = MapDesc()
        for k in range(3):
            d.origin[k] = origin[k]; d.dims[k] = int(dims[k]); d.min_boundary[k] = min_b[k]; d.max_boundary[k] = max_b[k]
        d.resolution = res
        o2 = np.ascontiguousarray(occ2d, dtype=np.int8)
        o3 = np.ascontiguousarray(occ3d, dtype=np.int8)
        _chk(self.L, self.L.topay_build_esdf(self.h, map_id, C.byref(d), o2.ctypes.data_as(C.POINTER(C.c_int8)),
                                             o3.ctypes.data_as(C.POINTER(C.c_int8))))
        self._map_dims[map_id] = tuple(int(x) for x in dims)

    def build_esdf_batch(self, origin, res, dims, min_b, max_b, occ2d_all, occ3d_all, first_map_id=0):
        """Same for a batch of equally sized maps: occ*_all are [n_maps, cells] arrays."""
        d = MapDesc()
        for k in range(3):
            d.origin[k] = origin[k]; d.dims[k] = int(dims[k]); d.min_boundary[k] = min_b[k]; d.max_boundary[k] = max_b[k]
        d.resolution = res
        o2 = np.ascontiguousarray(occ2d_all, dtype=np.int8)
        o3 = np.ascontiguousarray(occ3d_all, dtype=np.int8)
        n_maps = o2.shape[0]
        _chk(self.L, self.L.topay_build_esdf_batch(self.h, n_maps, first_map_id, C.byref(d), o2.ctypes.data_as(C.POINTER(C.c_int8)),
                                                   o3.ctypes.data_as(C.POINTER(C.c_int8))))
        for k in range(n_maps):
            self._map_dims[first_map_id + k] = tuple(int(x) for x in dims)

    def build_esdf_fields(self, origin, res, dims, min_b, max_b, occ2d, occ2d_critical, occ3d, map_id=0):
        """GridMap::updateESDF in full (also the inflate / critical 2-D fields); occ2d_critical may be None."""
        d = MapDesc()
        for k in range(3):
            d.origin[k] = origin[k]; d.dims[k] = int(dims[k]); d.min_boundary[k] = min_b[k]; d.max_boundary[k] = max_b[k]
        d.resolution = res
        o2 = np.ascontiguousarray(occ2d, dtype=np.int8)
        o3 = np.ascontiguousarray(occ3d, dtype=np.int8)
        oc = None if occ2d_critical is None else np.ascontiguousarray(occ2d_critical, dtype=np.int8)
        P8 = C.POINTER(C.c_int8)
        _chk(self.L, self.L.topay_build_esdf_fields(self.h, 1, map_id, C.byref(d), o2.ctypes.data_as(P8),
                                                    None if oc is None else oc.ctypes.data_as(P8), o3.ctypes.data_as(P8)))
        self._map_dims[map_id] = tuple(int(x) for x in dims)

    def get_map_fields(self, map_id=0):
        """(esdf2d_inflate, esdf2d_critical) of a map built on the device."""
        nx, ny, nz = self._map_dims[map_id]
        a = np.zeros(nx * ny)
        b = np.zeros(nx * ny)
        _chk(self.L, self.L.topay_get_map_fields(self.h, map_id, _dp(a), _dp(b)))
        return a, b

    def get_map(self, map_id=0):
        """(esdf2d, esdf3d, build_ms) of a resident map."""
        nx, ny, nz = self._map_dims[map_id]
        e2 = np.zeros(nx * ny)
        e3 = np.zeros(nx * ny * nz)
        ms = C.c_double(0)
        _chk(self.L, self.L.topay_get_map(self.h, map_id, _dp(e2), _dp(e3), C.byref(ms)))
        return e2, e3, ms.value

    # -- the first half of a benchmark episode (planner.cpp:491-548) on the device
    def _world_dims(self, prm, first_map_id, n):
        dims = tuple(int(np.ceil(v / prm.resolution)) for v in (prm.size_xy, prm.size_xy, prm.size_z))
        for k in range(n):
            self._map_dims[first_map_id + k] = dims

    def generate_worlds(self, prm, seeds, keepouts=None, first_map_id=0):
        """World::build for every seed into slots first_map_id ... (topay_generate_worlds), fields included.  keepouts: [n, 2, 2]
        (tables: start and goal xy) or None.  Returns the status array (1 built, -1 the generator's guard ended a loop)."""
        sd = _u64(seeds)
        n = len(sd)
        ko = None if keepouts is None else np.ascontiguousarray(keepouts, dtype=np.float64).reshape(n, 4)
        st = np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_generate_worlds(self.h, n, int(first_map_id), C.byref(prm), sd.ctypes.data_as(c_u64p), _dp(ko), _ip(st)))
        self._world_dims(prm, first_map_id, n)
        return st

    def get_occupancy(self, map_id=0):
        """(occ2d, occ2d_critical, occ3d) of a slot of the last generate_worlds / generate_episodes."""
        if map_id not in self._map_dims:
            raise TopayError(f"topay status -3: slot {map_id} holds no map")
        nx, ny, nz = self._map_dims[map_id]
        o2, oc, o3 = np.zeros(nx * ny, dtype=np.int8), np.zeros(nx * ny, dtype=np.int8), np.zeros(nx * ny * nz, dtype=np.int8)
        _chk(self.L, self.L.topay_get_occupancy(self.h, int(map_id), o2.ctypes.data_as(c_i8p), oc.ctypes.data_as(c_i8p), o3.ctypes.data_as(c_i8p)))
        return o2, oc, o3

    def world_last_path(self):
        """Rasteriser path of the last generate_worlds / generate_episodes: 1 masks in LDS, 2 byte stores."""
        v = C.c_int(0)
        _chk(self.L, self.L.topay_world_last_path(self.h, C.byref(v)))
        return v.value

    def world_test_path(self, path):
        """Test hook: 2 = byte stores whatever the map, 0 = the rule."""
        _chk(self.L, self.L.topay_world_test_path(self.h, int(path)))

    def world_test_max_tries(self, max_tries):
        """Test hook: tries per arm of generate_episodes' tables flow (0 = 2000)."""
        _chk(self.L, self.L.topay_world_test_max_tries(self.h, int(max_tries)))

    def world_stage_ms(self):
        """Device time of the last generate_worlds / generate_episodes by stage (WORLD_STAGE_MS_KEYS), milliseconds."""
        ms = np.zeros(4)
        _chk(self.L, self.L.topay_world_stage_ms(self.h, _dp(ms)))
        return dict(zip(WORLD_STAGE_MS_KEYS, ms.tolist()))

    def sample_arm(self, states, seeds, map_ids=None, max_tries=0):
        """World::sampleArm for [n, 10] states (x, y, theta given) -> (states with joints, ok, tries)."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10).copy()
        n = len(st)
        sd = _u64(seeds)
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        ok, tr = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_sample_arm(self.h, n, _ip(mid), sd.ctypes.data_as(c_u64p), int(max_tries), _dp(st), _ip(ok), _ip(tr)))
        return st, ok.astype(bool), tr

    def sample_scenarios(self, seeds, map_ids=None):
        """World::sampleScenario for every seed -> (start [n, 10], goal [n, 10], ok)."""
        sd = _u64(seeds)
        n = len(sd)
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        s, g, ok = np.zeros((n, 10)), np.zeros((n, 10)), np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_sample_scenarios(self.h, n, _ip(mid), sd.ctypes.data_as(c_u64p), _dp(s), _dp(g), _ip(ok)))
        return s, g, ok.astype(bool)

    def generate_episodes(self, prm, seeds, first_map_id=0, max_attempts=1, attempts=None):
        """One episode per seed into slots first_map_id ... (topay_generate_episodes): map, start, goal.  A failed episode is
        repeated on its own slot with attempt + 1, up to max_attempts attempts (the retry the library leaves to its caller).
        attempts: the first attempt of every episode (default 0).  Returns (start [n, 10], goal [n, 10], status [n], attempt [n] --
        the attempt that gave the episode, or the last one tried).

        A retry round calls the library on the failed slots only, and every call replaces the grids that get_occupancy reads:
        after a retry, get_occupancy serves the slots of the last call alone (TopayError NO_MAP for an episode that succeeded
        in an earlier round; the fields of every slot stay resident).  Each distinct run of retried slots also keeps a field
        arena of its own until its slots are rebuilt in one call or the context is destroyed."""
        sd = _u64(seeds)
        n = len(sd)
        att = np.zeros(n, dtype=np.int32) if attempts is None else np.ascontiguousarray(attempts, dtype=np.int32).copy()
        start, goal, status = np.zeros((n, 10)), np.zeros((n, 10)), np.zeros(n, dtype=np.int32)
        todo = np.arange(n)
        for rnd in range(max(1, int(max_attempts))):
            runs = np.split(todo, np.nonzero(np.diff(todo) != 1)[0] + 1)    # consecutive slots go in one call
            for run in runs:
                k = len(run)
                s, g, st = np.zeros((k, 10)), np.zeros((k, 10)), np.zeros(k, dtype=np.int32)
                sdr, atr = np.ascontiguousarray(sd[run]), np.ascontiguousarray(att[run])
                _chk(self.L, self.L.topay_generate_episodes(self.h, k, int(first_map_id + run[0]), C.byref(prm), sdr.ctypes.data_as(c_u64p), _ip(atr),
                                                            _dp(s), _dp(g), _ip(st)))
                start[run], goal[run], status[run] = s, g, st
            self._world_dims(prm, first_map_id, n)
            todo = np.nonzero(status != 1)[0]
            if len(todo) == 0 or rnd + 1 == max(1, int(max_attempts)):
                break
            att[todo] += 1
        return start, goal, status, att

    # ---- sensor clouds into the map (topay_sense_*: rog_map's ProbMap on a slot's grid) -------------------------------
    def sense_params(self, **kw):
        """topay_sense_default_params (params/rog_map.yaml) with the given fields replaced."""
        p = SenseParams()
        _chk(self.L, self.L.topay_sense_default_params(C.byref(p)))
        for k, v in kw.items():
            if isinstance(v, (list, tuple, np.ndarray)):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = x
            else:
                setattr(p, k, v)
        return p

    def sense_logodds(self, params=None):
        """l_hit, l_miss, l_min, l_max, l_occ, l_free of a parameter block as the library computes them (float32[6])."""
        out = np.zeros(6, dtype=np.float32)
        _chk(self.L, self.L.topay_sense_logodds(C.byref(params or self.sense_params()), out.ctypes.data_as(c_fp)))
        return out

    def sense_reset(self, map_ids, origin, res, dims, min_b, max_b):
        """topay_sense_reset: the beliefs of the slots map_ids on one grid, all unknown."""
        d = MapDesc()
        for i in range(3):
            d.origin[i], d.dims[i], d.min_boundary[i], d.max_boundary[i] = origin[i], int(dims[i]), min_b[i], max_b[i]
        d.resolution = res
        ids = np.ascontiguousarray(map_ids, dtype=np.int32).reshape(-1)
        _chk(self.L, self.L.topay_sense_reset(self.h, len(ids), _ip(ids), C.byref(d)))
        if not hasattr(self, "_sense_dims"):
            self._sense_dims = {}
        for m in ids:
            self._sense_dims[int(m)] = tuple(int(v) for v in dims)

    def sense_insert(self, map_ids, clouds, sensor_pos, params=None, cloud_off=None):
        """topay_sense_insert: one updateProbMap per slot.  clouds: a list of [k, 4] float32 arrays (x, y, z, intensity), one per
        slot, or SENSE_LAST_SCAN with the cloud_off sense_scan returned.  Returns status[n]: 1 flushed, 0 batch open, -1 / -2 the
        sensor is above the ceiling / below the ground."""
        ids = np.ascontiguousarray(map_ids, dtype=np.int32).reshape(-1)
        n = len(ids)
        sp = np.ascontiguousarray(sensor_pos, dtype=np.float64).reshape(n, 3)
        if isinstance(clouds, str) and clouds == SENSE_LAST_SCAN:
            off = np.ascontiguousarray(cloud_off, dtype=np.int32)
            ptr = C.c_void_p(1)
        else:
            cl = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in clouds]
            off = np.concatenate([[0], np.cumsum([len(c) for c in cl])]).astype(np.int32)
            pts = np.ascontiguousarray(np.concatenate(cl) if cl else np.zeros((0, 4)), dtype=np.float32)
            ptr = C.c_void_p(pts.ctypes.data) if len(pts) else C.c_void_p(None)
        assert len(off) == n + 1
        st = np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_sense_insert(self.h, n, _ip(ids), _ip(off), ptr, _dp(sp), C.byref(params or self.sense_params()), _ip(st)))
        return st

    def sense_commit(self, map_ids):
        """topay_sense_commit: occupancy grids from the beliefs, then the five fields of each slot, on the device."""
        ids = np.ascontiguousarray(map_ids, dtype=np.int32).reshape(-1)
        _chk(self.L, self.L.topay_sense_commit(self.h, len(ids), _ip(ids)))
        for m in ids:
            self._map_dims[int(m)] = self._sense_dims[int(m)]

    def sense_get(self, map_id):
        """The belief of a slot: (logodds float32, op_cnt, hit_cnt int32, each [nx, ny, nz], batch_counter)."""
        dims = self._sense_dims[int(map_id)]
        lo = np.zeros(dims, dtype=np.float32)
        op, hit = np.zeros(dims, dtype=np.int32), np.zeros(dims, dtype=np.int32)
        bc = C.c_int(0)
        _chk(self.L, self.L.topay_sense_get(self.h, int(map_id), lo.ctypes.data_as(c_fp), _ip(op), _ip(hit), C.byref(bc)))
        return lo, op, hit, bc.value

    def sense_scan(self, truth_map_ids, poses, n_az, n_el, fov, rng, copy_back=True):
        """topay_sense_scan: n_az x n_el rays per pose (x, y, z, yaw) through the resident occ3d of the truth slots.  Returns
        (cloud_off int32[n + 1], points float32[n, n_az * n_el, 4] or None); the points stay on the device for
        sense_insert(..., SENSE_LAST_SCAN, cloud_off=cloud_off)."""
        ids = np.ascontiguousarray(truth_map_ids, dtype=np.int32).reshape(-1)
        n = len(ids)
        ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 4)
        off = np.zeros(n + 1, dtype=np.int32)
        pts = np.zeros((n, n_az * n_el, 4), dtype=np.float32) if copy_back else None
        _chk(self.L, self.L.topay_sense_scan(self.h, n, _ip(ids), _dp(ps), int(n_az), int(n_el), float(fov), float(rng), n * n_az * n_el, _ip(off),
                                             pts.ctypes.data_as(c_fp) if copy_back else None))
        return off, pts

    def sense_ms(self):
        """Device time of the last scan, insert, flush and commit (with its fields) in ms."""
        ms = np.zeros(4)
        _chk(self.L, self.L.topay_sense_ms(self.h, _dp(ms)))
        return dict(zip(SENSE_MS_KEYS, ms.tolist()))

    def sense_slide_params(self, **kw):
        """topay_sense_slide_default_params (threshold 0.3, slide_z 0) with the given fields replaced."""
        p = SenseSlideParams()
        _chk(self.L, self.L.topay_sense_slide_default_params(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def sense_slide(self, map_ids, sensor_pos, params=None):
        """topay_sense_slide: the beliefs of the slots re-centred on their sensors where the trigger says so.  Returns
        (status int32[n], shift int32[n, 3]): 0 within the threshold, 1 slid, 2 slid from outside the window (skip this frame's
        insert), -1 a batch is open."""
        ids = np.ascontiguousarray(map_ids, dtype=np.int32).reshape(-1)
        n = len(ids)
        sp = np.ascontiguousarray(sensor_pos, dtype=np.float64).reshape(n, 3)
        st, sh = np.zeros(n, dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        _chk(self.L, self.L.topay_sense_slide(self.h, n, _ip(ids), _dp(sp), C.byref(params) if params is not None else None, _ip(st), _ip(sh)))
        return st, sh

    def sense_slide_ms(self):
        """Device time of the last sense_slide's launches in ms."""
        ms = C.c_double(0.0)
        _chk(self.L, self.L.topay_sense_slide_ms(self.h, C.byref(ms)))
        return ms.value

    def sense_desc(self, map_id):
        """topay_sense_get_desc: (origin, min_boundary, max_boundary) of a slot's belief, float64[3] each."""
        d = MapDesc()
        _chk(self.L, self.L.topay_sense_get_desc(self.h, int(map_id), C.byref(d)))
        return np.array(d.origin[:]), np.array(d.min_boundary[:]), np.array(d.max_boundary[:])

    def playback(self, i, times):
        """MomaTraj playback of candidate i: (states[len(times), 10], car_seq[n, 4])."""
        t = np.ascontiguousarray(times, dtype=np.float64)
        st = np.zeros((len(t), 10))
        cap = 4096
        seq = np.zeros((cap, 4))
        n = C.c_int(0)
        _chk(self.L, self.L.topay_playback(self.h, i, len(t), _dp(t), _dp(st), cap, _dp(seq), C.byref(n)))
        return st, seq[:min(n.value, cap)].copy()

    def whole_body_collision(self, states, map_id=0):
        """GridMap::isWholeBodyCollision for an [n, 10] array of states -> bool array."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        out = np.zeros(len(st), dtype=np.int32)
        _chk(self.L, self.L.topay_whole_body_collision(self.h, map_id, len(st), _dp(st), _ip(out)))
        return out.astype(bool)

    def dense_path(self, raw_paths, start_yaw, end_yaw, step_size=1.414, v_max=1.0, w_max=1.25, cap=None):
        """GraphSearch::getDensePath for a list of raw 2-D paths ([k_p, 2] arrays) -> list of [m_p, 4] arrays (x, y, theta, dt)."""
        lens = np.array([len(p) for p in raw_paths], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in raw_paths]))
        sy = np.ascontiguousarray(start_yaw, dtype=np.float64)
        ey = np.ascontiguousarray(end_yaw, dtype=np.float64)
        if cap is None:
            seg = [np.linalg.norm(np.diff(np.asarray(p, dtype=np.float64).reshape(-1, 2), axis=0), axis=1) for p in raw_paths]
            cap = int(max(2 * (np.ceil(s_ / step_size).clip(1).sum() + 1) + 4 for s_ in seg))
        out = np.zeros((len(lens), cap, 4))
        n = np.zeros(len(lens), dtype=np.int32)
        _chk(self.L, self.L.topay_dense_path(self.h, len(lens), _ip(lens), _dp(flat), step_size, _dp(sy), _dp(ey), v_max, w_max, cap, _ip(n), _dp(out)))
        return [out[p, :min(n[p], cap)].copy() for p in range(len(lens))], n

    def connect_collision(self, rs_distance, car_pose_fn, q_from, q_to, check_res, map_id=0):
        """MCRRTs::connectCollision for a batch of edges.  car_pose_fn(e, fractions) -> [len(fractions), 3] car poses of
        edge e (the caller's Reeds-Shepp interpolation).  Returns (collide[n] bool, piece_num[n])."""
        rs = np.ascontiguousarray(rs_distance, dtype=np.float64)
        qf = np.ascontiguousarray(q_from, dtype=np.float64).reshape(-1, 7)
        qt = np.ascontiguousarray(q_to, dtype=np.float64).reshape(-1, 7)
        n = len(rs)
        pn = np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_connect_check_num(n, _dp(rs), _dp(qf), _dp(qt), check_res, _ip(pn)))
        car = np.ascontiguousarray(np.concatenate([car_pose_fn(e, np.arange(pn[e]) / float(pn[e])) for e in range(n)]), dtype=np.float64)
        col = np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_connect_collision(self.h, map_id, n, _ip(pn), _dp(car), _dp(qf), _dp(qt), _ip(col)))
        return col.astype(bool), pn

    def share_maps(self, owner, first_map_id=0, n_maps=1):
        """Use `owner`'s resident maps (same device) for these slots instead of a copy of the fields."""
        self.L.topay_share_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _chk(self.L, self.L.topay_share_maps(self.h, owner.h, int(first_map_id), int(n_maps)))
        self._map_owner = owner      # keeps the owner alive

    def plan2d_jps(self, start_xy, end_xy, threshold=0.5, map_ids=None, cap=512):
        """GraphSearch::plan2dJPS for a batch of (start, goal) pairs -> (list of [m, 2] paths (empty: none), stats [n, 2])."""
        a = np.ascontiguousarray(start_xy, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(end_xy, dtype=np.float64).reshape(-1, 2)
        n = len(a)
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        ln, st, out = np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32), np.zeros((n, cap, 2))
        self.L.topay_plan2d_jps.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp, c_dp, C.c_double, C.c_int, c_ip, c_dp, c_ip]
        _chk(self.L, self.L.topay_plan2d_jps(self.h, n, None if mid is None else _ip(mid), _dp(a), _dp(b), float(threshold), int(cap), _ip(ln), _dp(out),
                                             _ip(st)))
        return [out[p, :min(ln[p], cap)].copy() for p in range(n)], st, ln

    def topo_params(self, **kw):
        p = TopoParams()
        self.L.topay_topo_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def topo_paths(self, start_xy, end_xy, prm=None, map_ids=None, critical=None, first_instance=0, cap_paths=None, cap_points=256):
        """TopologyPRM::findTopoPaths for a batch of (start, goal) pairs on maps built with build_esdf* -> (list per query of
        lists of [m, 2] paths, shortest first; stats [n, 8]: status, samples, samples past the clearance test, nodes before /
        after pruning, raw paths, paths after the first prune, selected paths)."""
        a = np.ascontiguousarray(start_xy, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(end_xy, dtype=np.float64).reshape(-1, 2)
        n = len(a)
        prm = prm if prm is not None else self.topo_params()
        cap_paths = int(cap_paths or prm.reserve_num)
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        cr = None if critical is None else np.ascontiguousarray(np.broadcast_to(np.asarray(critical), (n,)), dtype=np.int32)
        while True:
            npth, ln = np.zeros(n, dtype=np.int32), np.zeros((n, cap_paths), dtype=np.int32)
            out, st = np.zeros((n, cap_paths, cap_points, 2)), np.zeros((n, 8), dtype=np.int32)
            _chk(self.L, self.L.topay_topo_paths(self.h, n, _ip(mid), _dp(a), _dp(b), _ip(cr), C.byref(prm), int(first_instance), cap_paths,
                                                 int(cap_points), _ip(npth), _ip(ln), _dp(out), _ip(st)))
            if n == 0 or ln.max() <= cap_points:
                break
            cap_points = int(ln.max())   # (a path longer than the buffer: its length was reported, ask again with room for it)
        return [[out[p, k, :ln[p, k]].copy() for k in range(npth[p])] for p in range(n)], st

    def topo_graph(self, k, cap=None):
        """Graph of query k of the last topo_paths after pruneGraph, in list order: dict of id, type, pos, n_nb, nb."""
        cap = int(cap or 65535)
        n = C.c_int(0)
        _chk(self.L, self.L.topay_topo_graph(self.h, int(k), 0, None, None, None, None, None, C.byref(n)))
        m = min(n.value, cap)
        g = dict(id=np.zeros(m, dtype=np.int32), type=np.zeros(m, dtype=np.int32), pos=np.zeros((m, 2)), n_nb=np.zeros(m, dtype=np.int32),
                 nb=np.zeros((m, TOPO_MAX_NB), dtype=np.int32))
        _chk(self.L, self.L.topay_topo_graph(self.h, int(k), m, _ip(g["id"]), _ip(g["type"]), _dp(g["pos"]), _ip(g["n_nb"]), _ip(g["nb"]), C.byref(n)))
        return g

    def topo_raw_paths(self, k, which=0, cap_paths=64, cap_points=None):
        """The raw paths searchPaths kept for query k of the last topo_paths (which = 0) or their shortcut versions (1)."""
        cap_points = int(cap_points or (100 if which == 0 else 1024))
        while True:
            n, ln, out = C.c_int(0), np.zeros(cap_paths, dtype=np.int32), np.zeros((cap_paths, cap_points, 2))
            _chk(self.L, self.L.topay_topo_raw_paths(self.h, int(k), int(which), cap_paths, cap_points, C.byref(n), _ip(ln), _dp(out)))
            if ln.max() <= cap_points:
                break
            cap_points = int(ln.max())
        return [out[i, :ln[i]].copy() for i in range(min(n.value, cap_paths))]

    def candidate_paths(self, start_xy, end_xy, map_ids=None, critical=False, prm=None, first_instance=0):
        """The candidates of a planning call (planner.cpp:813-829): the roadmap's paths, plus -- when not critical and not empty --
        the plan2d_jps path (threshold chassis_colli_radius + 0.1); at most 8 per query (ValueError above: the reference throws
        "Too many paths to optimize").  Returns a list per query of [m, 2] raw paths, the layout dense_path takes."""
        a = np.ascontiguousarray(start_xy, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(end_xy, dtype=np.float64).reshape(-1, 2)
        paths, _ = self.topo_paths(a, b, prm, map_ids=map_ids, critical=1 if critical else None, first_instance=first_instance)
        if not critical:
            jps, _, _ = self.plan2d_jps(a, b, float(self.opt_param.chassis_colli_radius) + 0.1, map_ids=map_ids)
            for p in range(len(a)):
                if len(jps[p]):
                    paths[p].append(jps[p])
        for p in range(len(a)):
            if len(paths[p]) > 8:
                raise ValueError(f"query {p}: {len(paths[p])} candidate paths (at most 8: too many paths to optimize)")
        return paths

    def plan_params(self, topo=None, mcrrt=None, **kw):
        """PlanParams with the defaults of topay_plan_default_params; topo / mcrrt: dicts of fields of the two stages' blocks."""
        p = PlanParams()
        self.L.topay_plan_default_params(C.byref(p))
        for k, v in (topo or {}).items():
            setattr(p.topo, k, v)
        for k, v in (mcrrt or {}).items():
            setattr(p.mcrrt, k, v)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def plan_calls(self, start, end, map_ids=None, start_v=None, params=None, first_call=0):
        """Planner::planMomaParallel for n calls (topay_plan_calls): start / end [n, 10] states.  Returns (result [n, 8] --
        PLAN_RESULT_KEYS --, candidates [n, 2, 8, 4] = (stage, n_pieces, search status, solver stage-2 status) per try and
        candidate, winner_cost_duration [n, 2]).  The winners stay in the context's store: plan_trajs / plan_front_path."""
        st = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 10)
        en = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 10)
        n = len(st)
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        sv = None if start_v is None else np.ascontiguousarray(start_v, dtype=np.float64).reshape(n, 10)
        res, cand, wcd = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 2, 8, 4), dtype=np.int32), np.zeros((n, 2))
        _chk(self.L, self.L.topay_plan_calls(self.h, n, _ip(mid), _dp(st), _dp(en), _dp(sv), None if params is None else C.byref(params),
                                             int(first_call), _ip(res), _ip(cand), _dp(wcd)))
        self._note_plan_store(np.arange(n), res)
        return res, cand, wcd

    def _note_plan_store(self, rows, res):
        """What plan_trajs needs to size its buffers: the pieces of the winner in every row of the plan store, from the result
        table of the call that filled it (rows[k] = the store row of res[k], -1: none).  plan_calls and replan_calls share it."""
        rows = np.asarray(rows)
        pieces = np.zeros(int(rows.max()) + 1 if (rows >= 0).any() else 0, dtype=np.int32)
        has = rows >= 0
        pieces[rows[has]] = np.where(res[has, 0] == 1, res[has, 5], 0)
        self._plan_pieces = pieces

    def plan_trajs(self, calls):
        """The winners of a selection of calls of the last plan_calls, packed like getTrajs: piece_off[n+1], durations[P],
        coeffs[P, 9, 6], knots_xy[P + n, 2] (a call without a winner has no pieces)."""
        if self._plan_pieces is None:
            raise TopayError("plan_trajs: no plan_calls has been run on this context")
        idx = np.ascontiguousarray(calls, dtype=np.int32)
        n = len(idx)
        cap = int(self._plan_pieces[idx].sum()) if n else 0
        off = np.zeros(n + 1, dtype=np.int32)
        dur, coef, kn = np.zeros(cap), np.zeros(cap * 54), np.zeros(2 * (cap + n))
        _chk(self.L, self.L.topay_plan_get_trajs(self.h, n, _ip(idx), cap, _ip(off), _dp(dur), _dp(coef), _dp(kn)))
        return dict(piece_off=off, durations=dur, coeffs=coef.reshape(cap, 9, 6), knots_xy=kn.reshape(cap + n, 2))

    def plan_front_path(self, call):
        """The whole-body init path ([m, 10]) the winner of `call` was optimised from; empty without a winner."""
        n = C.c_int(0)
        _chk(self.L, self.L.topay_plan_get_front_path(self.h, int(call), 0, C.byref(n), None))
        out = np.zeros((n.value, 10))
        if n.value:
            _chk(self.L, self.L.topay_plan_get_front_path(self.h, int(call), n.value, C.byref(n), _dp(out)))
        return out

    def plan_test_chunk(self, calls):
        """Test hook: calls per front-end launch of plan_calls on this context (0 = the library's constant, 1024)."""
        _chk(self.L, self.L.topay_plan_test_chunk(self.h, int(calls)))

    def plan_stage_ms(self):
        """Device time of the last plan_calls by stage (PLAN_STAGE_MS_KEYS), milliseconds."""
        ms = np.zeros(8)
        _chk(self.L, self.L.topay_plan_stage_ms(self.h, _dp(ms)))
        return dict(zip(PLAN_STAGE_MS_KEYS, ms.tolist()))

    # ---- tracked trajectories and the replanning cycle (topay_host_track.h)
    def track_set(self, robot, which, start3, durations, coeffs):
        """MomaTraj::setTraj into robot slot `robot`: which 1 = end_traj, 2 = global_traj, 3 = both; coeffs [N, 9, 6] in the
        layout of getTrajs (highest order first)."""
        s3 = np.ascontiguousarray(start3, dtype=np.float64).reshape(-1)[:3].copy()
        dur = np.ascontiguousarray(durations, dtype=np.float64).reshape(-1)
        co = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1)
        if len(co) != 54 * len(dur):
            raise ValueError("coeffs must hold 9 x 6 values per piece")
        _chk(self.L, self.L.topay_track_set(self.h, int(robot), int(which), _dp(s3), len(dur), _dp(dur), _dp(co)))

    def track_commit_plan(self, robots, calls, which=1):
        """The winners of `calls` of the last plan_calls into the robot slots, on the device.  Returns committed [n] (0: the call
        had no winner, the slot is as it was)."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        ci = np.ascontiguousarray(calls, dtype=np.int32)
        done = np.zeros(len(rb), dtype=np.int32)
        _chk(self.L, self.L.topay_track_commit_plan(self.h, len(rb), _ip(rb), _ip(ci), int(which), _ip(done)))
        return done

    def track_get(self, robot, which=1):
        """(start3, durations [N], coeffs [N, 9, 6]) of the slot's trajectory, or None when it holds none."""
        n = C.c_int(0)
        _chk(self.L, self.L.topay_track_get(self.h, int(robot), int(which), 0, C.byref(n), None, None, None))
        if n.value == 0:
            return None
        s3, dur, co = np.zeros(3), np.zeros(n.value), np.zeros(n.value * 54)
        _chk(self.L, self.L.topay_track_get(self.h, int(robot), int(which), n.value, C.byref(n), _dp(s3), _dp(dur), _dp(co)))
        return s3, dur, co.reshape(-1, 9, 6)

    def track_clear(self, robot):
        _chk(self.L, self.L.topay_track_clear(self.h, int(robot)))

    def track_safe(self, robots, map_ids):
        """Planner::safeCallback of the robots' end_traj against the map slots as they are now.  Returns (safe [n] bool,
        first_hit [n, 2] = (sample, body), hit [n, 2] = (time, distance))."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        mid = np.ascontiguousarray(map_ids, dtype=np.int32)
        n = len(rb)
        safe, fh, hit = np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32), np.zeros((n, 2))
        _chk(self.L, self.L.topay_track_safe(self.h, n, _ip(rb), _ip(mid), _ip(safe), _ip(fh), _dp(hit)))
        return safe.astype(bool), fh, hit

    def track_safe_ms(self):
        """Device time of the last track_safe (or of the sweep of the last replan_calls), milliseconds."""
        ms = np.zeros(1)
        _chk(self.L, self.L.topay_track_safe_ms(self.h, _dp(ms)))
        return float(ms[0])

    def _sample_outs(self, what, n, rows, out):
        """The seven output addresses of topay_track_sample / _grid in the order of the C entry, and the dict the call returns:
        a new numpy array per selected output, or the caller's tensor of `out` (float64, contiguous, of the output's shape)."""
        if what <= 0 or what >= 64:
            raise ValueError("what must be a sum of SAMPLE_* bits")
        out = dict(out or {})
        res, ptr = {}, {}
        for name, bit, tail in SAMPLE_OUTPUTS + (("duration", 0, ()),):
            if bit and not what & bit:
                ptr[name] = None
                continue
            shape = ((n,) if name == "duration" else (rows,)) + tail
            t = out.pop(name, None)
            if t is None:
                res[name] = np.zeros(shape)
                ptr[name] = res[name].ctypes.data
            else:   # a torch tensor, by its methods: torch is not imported here
                if str(t.dtype) != "torch.float64" or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"out[{name!r}] must be a contiguous float64 tensor of shape {shape}")
                res[name] = t
                ptr[name] = t.data_ptr()
        if out:
            raise ValueError(f"out has entries that `what` does not select: {sorted(out)}")
        return [ptr[k] for k in ("state", "dstate", "ee_pose", "clearance", "centres", "duration", "distance")], res

    def track_sample(self, robots, times, which=1, map_ids=None, what=SAMPLE_STATE | SAMPLE_DSTATE, out=None):
        """The robots' tracked trajectories (which: 1 end_traj, 2 global_traj) at ragged times: times[k] is the sequence of
        robot k's times (it may be empty), row sum(len(times[:k])) + j of an output is its sample j.  what: a sum of SAMPLE_*;
        CLEARANCE and DISTANCE need map_ids.  Returns a dict of the selected outputs (SAMPLE_OUTPUTS: state [M, 10], dstate
        [M, 10], ee_pose [M, 9], clearance [M, 13], centres [M, 12, 3], distance [M, 13]) and "duration" [n], numpy arrays.
        out: a dict of torch tensors on the context's device under the same names (float64, contiguous, of those shapes): the
        kernel writes into them, they are returned in place of arrays, and the work on them is done when the call returns."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        n = len(rb)
        if len(times) != n:
            raise ValueError("times must hold one sequence per robot")
        ts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in times]
        off = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(ts)) if n else np.zeros(0)
        mid = None if map_ids is None else np.ascontiguousarray(np.broadcast_to(np.asarray(map_ids, dtype=np.int32), (n,)))
        ptrs, res = self._sample_outs(int(what), n, int(off[-1]), out)
        _chk(self.L, self.L.topay_track_sample(self.h, n, _ip(rb), int(which), _ip(mid), _ip(off), _dp(flat), int(what), *ptrs))
        return res

    def track_sample_grid(self, robots, t0, step, m, which=1, map_ids=None, what=SAMPLE_STATE | SAMPLE_DSTATE, out=None):
        """As track_sample on a grid per robot: sample j of robot k (row k m + j) at the running sum t0[k], += step; m samples
        always, beyond the trajectory's end the clamped state."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        n = len(rb)
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
        mid = None if map_ids is None else np.ascontiguousarray(np.broadcast_to(np.asarray(map_ids, dtype=np.int32), (n,)))
        ptrs, res = self._sample_outs(int(what), n, n * int(m), out)
        _chk(self.L, self.L.topay_track_sample_grid(self.h, n, _ip(rb), int(which), _ip(mid), _dp(t0), float(step), int(m), int(what), *ptrs))
        return res

    def track_sample_ms(self):
        """Device time of the last track_sample / track_sample_grid kernel, milliseconds."""
        ms = np.zeros(1)
        _chk(self.L, self.L.topay_track_sample_ms(self.h, _dp(ms)))
        return float(ms[0])

    # ---- the tracking controller and the fake robot (topay_host_mpc.h)
    def mpc_params(self, **kw):
        """topay_mpc_default_params with the given fields replaced (arrays as sequences)."""
        p = MpcParams()
        _chk(self.L, self.L.topay_mpc_default_params(C.byref(p)))
        for k, v in kw.items():
            if k in ("matrix_q", "matrix_r", "matrix_rd"):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = float(x)
            else:
                setattr(p, k, v)
        return p

    def mpc_qp_dims(self, params):
        nx, nc = C.c_int(0), C.c_int(0)
        _chk(self.L, self.L.topay_mpc_qp_dims(C.byref(params), C.byref(nx), C.byref(nc)))
        return nx.value, nc.value

    def mpc_reset(self, robots, params=None):
        """OMPC::init for the robot slots: output and FIFO zero, trajectory mode; the parameters hold until the next reset."""
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        p = params if params is not None else self.mpc_params()
        _chk(self.L, self.L.topay_mpc_reset(self.h, len(rb), _ip(rb), C.byref(p)))

    def mpc_set_direct(self, robots, direct_pos=None):
        """OMPC::setDirect with direct_pos [n, 3]; None: back to trajectory mode."""
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        dp = None if direct_pos is None else np.ascontiguousarray(direct_pos, dtype=np.float64).reshape(len(rb), 3)
        _chk(self.L, self.L.topay_mpc_set_direct(self.h, len(rb), _ip(rb), None if dp is None else _dp(dp)))

    def mpc_cmds(self, robots, t_cur, now_state, want_xopt=False):
        """One OMPC::getCmd per robot.  Returns (cmd [n, 16] = speed, angular_velocity, q[7], dq[7]; status [n, 4], columns
        MPC_ST_KEYS; xopt [n, 129, 3] or None)."""
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        n = len(rb)
        tc = np.ascontiguousarray(np.broadcast_to(np.asarray(t_cur, dtype=np.float64), (n,)))
        ns = np.ascontiguousarray(now_state, dtype=np.float64).reshape(n, 10)
        cmd, st = np.zeros((n, 16)), np.zeros((n, 4), dtype=np.int32)
        xo = np.zeros((n, MPC_MAX_STEPS + 1, 3)) if want_xopt else None
        _chk(self.L, self.L.topay_mpc_cmds(self.h, n, _ip(rb), _dp(tc), _dp(ns), _dp(cmd), _ip(st), None if xo is None else _dp(xo)))
        return cmd, st, xo

    def mpc_probe(self, robot, t_cur, now_state, params):
        """The first QP of mpc_cmds for one robot, the slot untouched: dict with P, q, A, l, u (dense, the reference's order), x, y,
        z, iters, solved."""
        nx, nc = self.mpc_qp_dims(params)
        ns = np.ascontiguousarray(now_state, dtype=np.float64).reshape(10)
        o = dict(P=np.zeros((nx, nx)), q=np.zeros(nx), A=np.zeros((nc, nx)), l=np.zeros(nc), u=np.zeros(nc), x=np.zeros(nx), y=np.zeros(nc),
                 z=np.zeros(nc))
        info = np.zeros(2, dtype=np.int32)
        _chk(self.L, self.L.topay_mpc_probe(self.h, int(robot), float(t_cur), _dp(ns), _dp(o["P"]), _dp(o["q"]), _dp(o["A"]), _dp(o["l"]),
                                            _dp(o["u"]), _dp(o["x"]), _dp(o["y"]), _dp(o["z"]), _ip(info)))
        o["iters"], o["solved"] = int(info[0]), int(info[1])
        return o

    def mpc_get_state(self, robot):
        """(output [2, 128], fifo [128, 2], mode) of the slot."""
        out, ff, mode = np.zeros((2, MPC_MAX_STEPS)), np.zeros((MPC_MAX_STEPS, 2)), C.c_int(0)
        _chk(self.L, self.L.topay_mpc_get_state(self.h, int(robot), _dp(out), _dp(ff), C.byref(mode)))
        return out, ff, mode.value

    def mpc_ms(self):
        """Device time of the last mpc_cmds / track_follow, milliseconds."""
        ms = np.zeros(1)
        _chk(self.L, self.L.topay_mpc_ms(self.h, _dp(ms)))
        return float(ms[0])

    def sim_reset(self, robots, state0, delay_cmds=20):
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        s0 = np.ascontiguousarray(state0, dtype=np.float64).reshape(len(rb), 10)
        _chk(self.L, self.L.topay_sim_reset(self.h, len(rb), _ip(rb), _dp(s0), int(delay_cmds)))

    def sim_step(self, robots, cmd, ticks):
        """One command (cmd [n, 16] or None) into every robot's actuator FIFO, then `ticks` ticks of 0.01 s.  Returns states [n, 10]."""
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        n = len(rb)
        cm = None if cmd is None else np.ascontiguousarray(cmd, dtype=np.float64).reshape(n, 16)
        st = np.zeros((n, 10))
        _chk(self.L, self.L.topay_sim_step(self.h, n, _ip(rb), None if cm is None else _dp(cm), int(ticks), _dp(st)))
        return st

    def track_follow(self, robots, t0, periods, ticks_per_period=2):
        """`periods` control periods on the device: command, simulator step, t += 1 / ctrl_freq.  Returns (states [n, periods, 10],
        cmds [n, periods, 16], status [n, periods, 4])."""
        rb = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        n = len(rb)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
        st, cm, ss = np.zeros((n, periods, 10)), np.zeros((n, periods, 16)), np.zeros((n, periods, 4), dtype=np.int32)
        _chk(self.L, self.L.topay_track_follow(self.h, n, _ip(rb), _dp(t), int(periods), int(ticks_per_period), _dp(st), _dp(cm), _ip(ss)))
        return st, cm, ss

    def replan_inputs(self, robots, t_since_replan, t_since_begin, global_goal, planning_budget, planning_horizon):
        """The endpoints of Planner::replanCallback: (start [n, 10], start_v [n, 10], goal [n, 10], goal_source [n])."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        n = len(rb)
        tr = np.ascontiguousarray(np.broadcast_to(np.asarray(t_since_replan, dtype=np.float64), (n,)))
        tb = np.ascontiguousarray(np.broadcast_to(np.asarray(t_since_begin, dtype=np.float64), (n,)))
        gg = np.ascontiguousarray(global_goal, dtype=np.float64).reshape(n, 10)
        st, sv, go, src = np.zeros((n, 10)), np.zeros((n, 10)), np.zeros((n, 10)), np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_replan_inputs(self.h, n, _ip(rb), _dp(tr), _dp(tb), _dp(gg), float(planning_budget), float(planning_horizon),
                                                _dp(st), _dp(sv), _dp(go), _ip(src)))
        return st, sv, go, src

    def replan_calls(self, robots, map_ids, t_since_replan, t_since_begin, global_goal, replan_interval, planning_budget, planning_horizon,
                     now_xy=None, params=None, first_call=0):
        """One round of Planner::replanCallback for n robots (topay_replan_calls).  Returns (status [n, 4] = (outcome, safe, row
        in the plan store, goal_source), endpoints [n, 3, 10] = (start, start_v, goal), result [n, 8], candidates [n, 2, 8, 4])."""
        rb = np.ascontiguousarray(robots, dtype=np.int32)
        n = len(rb)
        mid = np.ascontiguousarray(map_ids, dtype=np.int32)
        tr = np.ascontiguousarray(np.broadcast_to(np.asarray(t_since_replan, dtype=np.float64), (n,)))
        tb = np.ascontiguousarray(np.broadcast_to(np.asarray(t_since_begin, dtype=np.float64), (n,)))
        gg = np.ascontiguousarray(global_goal, dtype=np.float64).reshape(n, 10)
        xy = None if now_xy is None else np.ascontiguousarray(now_xy, dtype=np.float64).reshape(n, 2)
        status, ends = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 3, 10))
        res, cand = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 2, 8, 4), dtype=np.int32)
        _chk(self.L, self.L.topay_replan_calls(self.h, n, _ip(rb), _ip(mid), _dp(tr), _dp(tb), _dp(xy), _dp(gg), float(replan_interval),
                                               float(planning_budget), float(planning_horizon), None if params is None else C.byref(params),
                                               int(first_call), _ip(status), _dp(ends), _ip(res), _ip(cand)))
        self._note_plan_store(status[:, 2], res)
        return status, ends, res, cand

    # ---- end-effector goals (MomaTrajOpt::optimizeEE) ----
    def ee_params(self, **kw):
        """EeParams with the defaults of topay_ee_default_params; lbfgs: a dict of fields of its L-BFGS block."""
        p = EeParams()
        self.L.topay_ee_default_params(C.byref(p))
        for k, v in kw.items():
            if k == "lbfgs":
                for kk, vv in v.items():
                    setattr(p.lbfgs, kk, vv)
            else:
                setattr(p, k, v)
        return p

    def ee_pose(self, states):
        """getFKPose of [n, 10] states: [n, 9] = position, row 0, row 1 of the end effector's rotation."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        out = np.zeros((len(st), 9))
        _chk(self.L, self.L.topay_ee_pose(self.h, len(st), _dp(st), _dp(out)))
        return out

    @staticmethod
    def _ee_mid(map_ids, n):
        return None if map_ids is None else np.ascontiguousarray(np.broadcast_to(np.asarray(map_ids, dtype=np.int32), (n,)))

    def ee_eval(self, x, ee_ref, map_ids=None):
        """One eeCostCallback per problem at the unconstrained x [n, 10]: (f [n], g [n, 10])."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 10)
        n = len(x)
        ref = np.ascontiguousarray(ee_ref, dtype=np.float64).reshape(n, 9)
        mid = self._ee_mid(map_ids, n)
        f, g = np.zeros(n), np.zeros((n, 10))
        _chk(self.L, self.L.topay_ee_eval(self.h, n, _ip(mid), _dp(x), _dp(ref), _dp(f), _dp(g)))
        return f, g

    def ee_goals(self, seed_states, ee_ref, map_ids=None, params=None):
        """optimizeEE of n problems: (states [n, 10], cost [n], code [n], iters [n], evals [n])."""
        seed = np.ascontiguousarray(seed_states, dtype=np.float64).reshape(-1, 10)
        n = len(seed)
        ref = np.ascontiguousarray(ee_ref, dtype=np.float64).reshape(n, 9)
        mid = self._ee_mid(map_ids, n)
        st, cost = np.zeros((n, 10)), np.zeros(n)
        code, it, ev = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.topay_ee_goals(self.h, n, _ip(mid), _dp(seed), _dp(ref), None if params is None else C.byref(params), _dp(st), _dp(cost),
                                           _ip(code), _ip(it), _ip(ev)))
        return st, cost, code, it, ev

    def ee_ms(self):
        """Device time of the last ee_goals, milliseconds."""
        ms = np.zeros(1)
        _chk(self.L, self.L.topay_ee_ms(self.h, _dp(ms)))
        return float(ms[0])

    def ee_select(self, group_of, n_groups, states, cost, code, ee_ref, map_ids=None, params=None, goal=None):
        """Per group the first qualified problem of smallest cost: (winner [n_groups], goal [n_groups, 10]); goal rows of groups
        without a winner keep what `goal` held (zeros when not given)."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        n = len(st)
        grp = np.ascontiguousarray(group_of, dtype=np.int32)
        co = np.ascontiguousarray(cost, dtype=np.float64)
        cd = np.ascontiguousarray(code, dtype=np.int32)
        ref = np.ascontiguousarray(ee_ref, dtype=np.float64).reshape(n, 9)
        mid = self._ee_mid(map_ids, n)
        win = np.zeros(n_groups, dtype=np.int32)
        go = np.zeros((n_groups, 10)) if goal is None else np.array(goal, dtype=np.float64).reshape(n_groups, 10)
        _chk(self.L, self.L.topay_ee_select(self.h, n, _ip(mid), _ip(grp), int(n_groups), _dp(st), _dp(co), _ip(cd), _dp(ref),
                                            None if params is None else C.byref(params), _ip(win), _dp(go)))
        return win, go

    def mcrrt_params(self, **kw):
        p = McrrtParams()
        self.L.topay_mcrrt_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def mcrrt_plan(self, lens, car_paths, start, end, params=None, map_ids=None, first_instance=0, cap=None):
        """MCRRTs::plan for a batch of chassis paths (ragged car_paths [sum lens, 4] = (x, y, theta, dt); start / end [n, 10]).
        Returns (wb_paths: list of [m, 10] arrays (empty when no path), stats [n, 8], c_max [n])."""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = len(lens)
        car = np.ascontiguousarray(car_paths, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(start, dtype=np.float64).reshape(n, 10)
        en = np.ascontiguousarray(end, dtype=np.float64).reshape(n, 10)
        cap = int(cap or max(2, int(lens.max()) if n else 2))
        mid = None if map_ids is None else np.ascontiguousarray(map_ids, dtype=np.int32)
        wl_ = np.zeros(n, dtype=np.int32)
        wb = np.zeros((n, cap, 10))
        stats = np.zeros((n, 8), dtype=np.int32)
        cmax = np.zeros(n)
        _chk(self.L, self.L.topay_mcrrt_plan(self.h, n, None if mid is None else _ip(mid), _ip(lens), _dp(car), _dp(st), _dp(en),
                                             None if params is None else C.byref(params), int(first_instance), cap, _ip(wl_), _dp(wb),
                                             _ip(stats), _dp(cmax)))
        return [wb[p, :wl_[p]].copy() for p in range(n)], stats, cmax

    def mcrrt_nodes(self, instance, n_nodes):
        """Node table of one instance of the last mcrrt_plan: dict of layer, state, parent, cost, q ([n_nodes, 7])."""
        m = int(n_nodes)
        layer, state, parent = (np.zeros(m, dtype=np.int32) for _ in range(3))
        cost, q = np.zeros(m), np.zeros((m, 7))
        _chk(self.L, self.L.topay_mcrrt_nodes(self.h, int(instance), m, _ip(layer), _ip(state), _ip(parent), _dp(cost), _dp(q)))
        return dict(layer=layer, state=state, parent=parent, cost=cost, q=q)

    def reeds_shepp(self, from_poses, to_poses, t=None, rho=1.0e-2):
        """ompl ReedsSheppStateSpace(rho): (distance [n], word [n], lengths [n, 5], pose [n, 3] or None)."""
        a = np.ascontiguousarray(from_poses, dtype=np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(to_poses, dtype=np.float64).reshape(-1, 3)
        n = len(a)
        tt = None if t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
        d, w, ln, po = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros((n, 5)), np.zeros((n, 3))
        _chk(self.L, self.L.topay_reeds_shepp(self.h, n, _dp(a), _dp(b), None if tt is None else _dp(tt), float(rho), _dp(d), _ip(w), _dp(ln),
                                              _dp(po)))
        return d, w, ln, (po if tt is not None else None)

    def alm_state(self):
        """(lambda0, lambda1, rho0, rho1) every candidate finished with."""
        a = np.zeros(self.batch * 4)
        _chk(self.L, self.L.topay_get_alm(self.h, _dp(a)))
        return a.reshape(self.batch, 4)

    def elapsed_us(self):
        """Device-measured optimisation time of every candidate (microseconds)."""
        t = np.zeros(self.batch)
        _chk(self.L, self.L.topay_get_elapsed_us(self.h, _dp(t), None, None))
        return t

    def start_us(self, raw=False):
        """When every candidate's solve began, on the device's constant clock (raw=True: comparable between contexts of
        one device; default: relative to the first start of this batch)."""
        t = np.zeros(self.batch)
        _chk(self.L, self.L.topay_get_elapsed_us(self.h, None, _dp(t), None))
        return t if raw else t - t.min()

    def hw_ids(self):
        h = np.zeros(self.batch, dtype=np.int32)
        _chk(self.L, self.L.topay_get_elapsed_us(self.h, None, None, _ip(h)))
        return h

    def get_x(self, i):
        n = C.c_int(0)
        _chk(self.L, self.L.topay_get_x(self.h, i, C.byref(n), None))
        x = np.zeros(n.value)
        _chk(self.L, self.L.topay_get_x(self.h, i, C.byref(n), _dp(x)))
        return x

    # -- firstStageCostCallback / secondStageCostCallback (test hook)
    def eval(self, stage, i, x, alm_lambda=None, alm_rho=None, waves=None):
        """(f, g, final_xy_error) of candidate i at x.  waves=1/2/4: by the kernel with that many wavefronts per trajectory
        (test hook topay_eval_waves) instead of the candidate's class default."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros_like(x)
        f = C.c_double(0)
        e = np.zeros(2)
        lam = None if alm_lambda is None else np.ascontiguousarray(alm_lambda, dtype=np.float64)
        rho = None if alm_rho is None else np.ascontiguousarray(alm_rho, dtype=np.float64)
        if waves is None:
            _chk(self.L, self.L.topay_eval(self.h, stage, i, _dp(x), _dp(lam), _dp(rho), C.byref(f), _dp(g), _dp(e)))
        else:
            _chk(self.L, self.L.topay_eval_waves(self.h, stage, i, int(waves), _dp(x), _dp(lam), _dp(rho), C.byref(f), _dp(g), _dp(e)))
        return f.value, g, e

    def load_solution(self, i, x, alm_lambda=None, alm_rho=None):
        """Make the spline of the decision vector x candidate i's result (getTraj() after an evaluation at x)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        lam = None if alm_lambda is None else np.ascontiguousarray(alm_lambda, dtype=np.float64)
        rho = None if alm_rho is None else np.ascontiguousarray(alm_rho, dtype=np.float64)
        _chk(self.L, self.L.topay_load_solution(self.h, i, _dp(x), _dp(lam), _dp(rho)))

    def class_of(self, n_pieces):
        """(waves the solver's vectors are divided over, vector elements per thread of the solver, launch class index) of a candidate of
        n_pieces pieces: what the bits of its solve depend on (since round 5 one wave for every class; the classes from index 4 up
        -- more than 32 pieces -- evaluate on four waves)."""
        w, e, k = C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(self.L, self.L.topay_class_of(int(n_pieces), C.byref(w), C.byref(e), C.byref(k)))
        return w.value, e.value, k.value

    def workspace_bytes(self):
        b = C.c_ulonglong(0)
        _chk(self.L, self.L.topay_workspace_bytes(self.h, C.byref(b)))
        return int(b.value)

    def set_groups(self, group_id, cancel_budget=2400):
        """Planning call (scenario) of every candidate and the cancellation window after a call's first feasible success, in
        piece-evaluations (2400 = the reference's 100 ms); None / 0 switches cancellation off."""
        g = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.int32)
        _chk(self.L, self.L.topay_set_groups(self.h, _ip(g), int(cancel_budget) if g is not None else 0))

    def set_latency_mode(self, mode):
        """0: never (default); 1: batches with at most one candidate per SIMD (1024 on an MI355X) run on four-wave workgroups whose extra
        waves join the evaluations only (same bits, shorter solves); 2: every batch."""
        _chk(self.L, self.L.topay_set_latency_mode(self.h, int(mode)))

    def cancel(self):
        _chk(self.L, self.L.topay_cancel(self.h))

    def interrupted(self):
        out = np.zeros(self.batch, dtype=np.int32)
        _chk(self.L, self.L.topay_get_interrupted(self.h, _ip(out)))
        return out.astype(bool)

    # -- the multi-GPU exchange through the C-ABI (a C++ planner's path; bench.py uses torch.distributed for the same records)
    def comm_unique_id(self):
        cid = CommId()
        _chk(self.L, self.L.topay_comm_unique_id(C.byref(cid)))
        return cid

    def comm_init(self, cid, world, rank):
        _chk(self.L, self.L.topay_comm_init(self.h, C.byref(cid), world, rank))

    def comm_destroy(self):
        _chk(self.L, self.L.topay_comm_destroy(self.h))

    def scenario_records(self, scenario_of):
        """(records structured array, winner batch indices) of the solved batch: one 32-byte record per scenario."""
        so = np.ascontiguousarray(scenario_of, dtype=np.int32)
        cap = len(set(so.tolist()))
        recs = (Record * max(cap, 1))()
        n = C.c_int(0)
        win = np.zeros(max(cap, 1), dtype=np.int32)
        _chk(self.L, self.L.topay_scenario_records(self.h, _ip(so), cap, recs, C.byref(n), _ip(win)))
        return np.ctypeslib.as_array(recs)[:n.value].copy() if n.value else np.zeros(0, dtype=np.dtype(Record)), win[:n.value]

    def gather_records(self, records, per_rank, world):
        rec = np.ascontiguousarray(records)
        out = (Record * (per_rank * world))()
        nv = C.c_int(0)
        _chk(self.L, self.L.topay_gather_records(self.h, rec.ctypes.data_as(C.POINTER(Record)), len(rec), per_rank, out, C.byref(nv)))
        return np.ctypeslib.as_array(out)[:nv.value].copy()

    def gate_timeouts(self):
        n = C.c_int(0)
        _chk(self.L, self.L.topay_gate_timeouts(self.h, C.byref(n)))
        return n.value

    def _mesh_params(self):
        m = MeshParams()
        _chk(self.L, self.L.topay_default_mesh_params(C.byref(m)))
        return m

    def mesh_poses(self, states, mesh=None):
        """MomaParam::getMeshPose for n states: (n, 11, 7) = (x, y, z, qw, qx, qy, qz) of chassis, stump, 7 links, ee, ee point."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        out = np.zeros((len(st), 11, 7))
        m = mesh or self._mesh_params()
        _chk(self.L, self.L.topay_mesh_poses(self.h, C.byref(m), len(st), _dp(st), _dp(out)))
        return out

    def mesh_traj(self, i, res=1000, mesh=None):
        """Planner::toMeshMsg of candidate i: (parts (n, 11, 7), yaws (n), arc_lengths (n))."""
        cap = res + 1
        parts, yaws, arcs = np.zeros((cap, 11, 7)), np.zeros(cap), np.zeros(cap)
        n = np.zeros(1, dtype=np.int32)
        m = mesh or self._mesh_params()
        _chk(self.L, self.L.topay_mesh_traj(self.h, i, C.byref(m), res, cap, _dp(parts), _dp(yaws), _dp(arcs), _ip(n)))
        return parts[:n[0]], yaws[:n[0]], arcs[:n[0]]

    def set_params(self, params=None):
        """Push `opt_param` (or `params`) to the context: the reference's `opt_param` is a public member the planner may
        change between calls (moma_traj_opt.h:616)."""
        if params is not None:
            self.opt_param = params
        _chk(self.L, self.L.topay_set_params(self.h, C.byref(self.opt_param)))

    COST_TERMS = ("jerk", "time", "chassis_colli", "moment", "acc", "domega", "mani_colli", "self_colli", "mani_pos",
                  "mani_vel", "mani_acc", "mean_time", "endp")

    def cost_terms(self, i, x, alm_lambda, alm_rho):
        """Per-term breakdown of the stage-2 cost at x -- what the reference's DebugManager publishes under
        /debug_cost/<name> (moma_traj_opt.h:566-611, names as in 930-941).  Every term carries its own weight, so term k
        is the cost evaluated with every other weight at zero (the ALM term switched off by lambda = 0, rho = 1e-300):
        13 evaluations through topay_eval with topay_set_params in between; a debugging aid, not a hot path."""
        own = {"jerk": "energy_weights", "time": "s2_time_weight", "chassis_colli": "s2_collision_weight",
               "moment": "s2_moment_weight", "acc": "s2_acc_weight", "domega": "s2_domega_weight",
               "mani_colli": "s2_mani_colli_weight", "self_colli": "s2_self_colli_weight", "mani_pos": "s2_mani_pos_weight",
               "mani_vel": "s2_mani_vel_weight", "mani_acc": "s2_mani_acc_weight", "mean_time": "s2_mean_time_weight"}
        keep = Params()
        C.memmove(C.byref(keep), C.byref(self.opt_param), C.sizeof(Params))
        out = {}
        try:
            for name in self.COST_TERMS:
                q = Params()
                C.memmove(C.byref(q), C.byref(keep), C.sizeof(Params))
                for term, field in own.items():
                    if term == name:
                        continue
                    if field == "energy_weights":
                        for k in range(9):
                            q.energy_weights[k] = 0.0
                    else:
                        setattr(q, field, 0.0)
                _chk(self.L, self.L.topay_set_params(self.h, C.byref(q)))
                if name == "endp":
                    out[name] = self.eval(2, i, x, alm_lambda, alm_rho)[0]
                else:
                    out[name] = self.eval(2, i, x, [0.0, 0.0], [1e-300, 1e-300])[0]
        finally:
            _chk(self.L, self.L.topay_set_params(self.h, C.byref(keep)))
        return out

    def eval_batch(self, stage, repeats=1):
        f = np.zeros(self.batch)
        _chk(self.L, self.L.topay_eval_batch(self.h, stage, repeats, _dp(f)))
        return f

    def set_trace(self, cap):
        self._trace_cap = cap
        _chk(self.L, self.L.topay_set_trace(self.h, cap))

    def get_trace(self, i):
        out = np.zeros(self._trace_cap)
        _chk(self.L, self.L.topay_get_trace(self.h, i, _dp(out)))
        return out

    def test_math(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.zeros(4 * len(a))
        _chk(self.L, self.L.topay_test_math(self.h, len(a), _dp(a), _dp(b), _dp(out)))
        return out.reshape(-1, 4)

    def last_helper_launches(self):
        n = C.c_int(0)
        _chk(self.L, self.L.topay_last_helper_launches(self.h, C.byref(n)))
        return n.value

    def last_kernel_ms(self):
        ms = C.c_double(0)
        n = C.c_int(0)
        _chk(self.L, self.L.topay_last_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
