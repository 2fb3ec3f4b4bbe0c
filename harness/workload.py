"""ctypes front-end of the synthetic workload generator (libtopay_workload.so).

Builds the BASELINE.json configurations: seeded "tables"/"cuboids" worlds with their 2-D/3-D ESDF,
start/goal scenarios, and front-end stand-in init paths (ragged P x 10 states per candidate).
Harness only: runs on the CPU, once per map/scenario, outside every timed region.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)

TABLES, CUBOIDS = 0, 1


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libtopay_workload.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.wl_world_create.restype = C.c_void_p
        L.wl_world_create.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                      c_dp, C.c_int]
        L.wl_world_esdf2d.restype = c_dp
        L.wl_world_esdf3d.restype = c_dp
        L.wl_world_esdf2d.argtypes = [C.c_void_p]
        L.wl_world_occ2d.restype = C.POINTER(C.c_int8)
        L.wl_world_occ3d.restype = C.POINTER(C.c_int8)
        L.wl_world_occ2d.argtypes = [C.c_void_p]
        L.wl_world_occ3d.argtypes = [C.c_void_p]
        L.wl_world_esdf3d.argtypes = [C.c_void_p]
        L.wl_world_esdf3d_size.argtypes = [C.c_void_p]
        L.wl_world_esdf3d_size.restype = C.c_longlong
        L.wl_set_keep_esdf3d.argtypes = [C.c_int]
        L.wl_world_destroy.argtypes = [C.c_void_p]
        L.wl_world_desc.argtypes = [C.c_void_p, c_ip, c_dp, c_dp, c_dp, c_dp]
        L.wl_sample_start_goal_xy.argtypes = [C.c_uint64, C.c_double, c_dp, c_dp]
        L.wl_sample_arm.argtypes = [C.c_void_p, C.c_uint64, c_dp]
        L.wl_sample_scenario.argtypes = [C.c_void_p, C.c_uint64, c_dp, c_dp]
        L.wl_whole_body_collision.argtypes = [C.c_void_p, c_dp]
        L.wl_whole_body_tie_slack.argtypes = [C.c_void_p, c_dp]
        L.wl_whole_body_tie_slack.restype = C.c_double
        L.wl_init_paths.argtypes = [C.c_void_p, c_dp, c_dp, C.c_int, C.c_uint64, c_dp, C.c_int, c_ip]
        L.wl_tables_batch_create.restype = C.c_void_p
        L.wl_tables_batch_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double,
                                             C.c_int]
        L.wl_tables_batch_destroy.argtypes = [C.c_void_p]
        L.wl_tables_batch_ntraj.argtypes = [C.c_void_p]
        L.wl_tables_batch_nstates.argtypes = [C.c_void_p]
        L.wl_tables_batch_nstates.restype = C.c_longlong
        L.wl_tables_batch_get.argtypes = [C.c_void_p, c_ip, c_ip, c_dp]
        L.wl_tables_batch_world.argtypes = [C.c_void_p, C.c_int]
        L.wl_tables_batch_world.restype = C.c_void_p
        _LIB = L
    return _LIB


def _dp(a):
    return a.ctypes.data_as(c_dp) if a is not None else None


class World:
    def __init__(self, kind, seed=42, size_xy=20.0, size_z=1.6, res=0.1, cloud_res=0.05, keepouts=None, nthreads=0,
                 _borrowed=None):
        L = lib()
        if _borrowed is not None:
            self.h = C.c_void_p(_borrowed)
            self._owned = False
        else:
            ko = np.zeros((0, 2)) if keepouts is None else np.ascontiguousarray(keepouts, dtype=np.float64).reshape(-1, 2)
            self.h = C.c_void_p(L.wl_world_create(kind, seed, size_xy, size_z, res, cloud_res, ko.shape[0], _dp(ko), nthreads))
            self._owned = True
        self.kind = kind
        self.size_xy = size_xy
        dims = np.zeros(3, dtype=np.int32)
        origin = np.zeros(3)
        mn = np.zeros(3)
        mx = np.zeros(3)
        r = C.c_double(0)
        L.wl_world_desc(self.h, dims.ctypes.data_as(c_ip), _dp(origin), C.byref(r), _dp(mn), _dp(mx))
        self.dims, self.origin, self.res, self.min_b, self.max_b = dims, origin, r.value, mn, mx
        n2 = int(dims[0]) * int(dims[1])
        n3 = n2 * int(dims[2])
        # nthreads < 0: occupancy grids only (no CPU distance fields; scenario sampling and init paths need them)
        self.esdf2d = np.ctypeslib.as_array(L.wl_world_esdf2d(self.h), shape=(n2,)) if nthreads >= 0 or _borrowed is not None else None
        # None when the batch generator was told to drop it (TablesBatch(keep_esdf3d=...))
        self.esdf3d = np.ctypeslib.as_array(L.wl_world_esdf3d(self.h), shape=(n3,)) if L.wl_world_esdf3d_size(self.h) == n3 else None
        self.occ2d = np.ctypeslib.as_array(L.wl_world_occ2d(self.h), shape=(n2,))
        self.occ3d = np.ctypeslib.as_array(L.wl_world_occ3d(self.h), shape=(n3,))

    def close(self):
        if self.h:
            if self._owned:
                lib().wl_world_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample_scenario(self, seed):
        s = np.zeros(10)
        g = np.zeros(10)
        ok = lib().wl_sample_scenario(self.h, seed, _dp(s), _dp(g))
        return bool(ok), s, g

    def sample_arm(self, seed, state):
        st = np.ascontiguousarray(state, dtype=np.float64).copy()
        ok = lib().wl_sample_arm(self.h, seed, _dp(st))
        return bool(ok), st

    def collision(self, state):
        st = np.ascontiguousarray(state, dtype=np.float64)
        return bool(lib().wl_whole_body_collision(self.h, _dp(st)))

    def collision_tie_slack(self, state):
        """Smallest |lhs - rhs| over all threshold comparisons of isWholeBodyCollision for this state."""
        st = np.ascontiguousarray(state, dtype=np.float64)
        return float(lib().wl_whole_body_tie_slack(self.h, _dp(st)))

    def init_paths(self, start, goal, n_cand, seed, max_states=20000):
        start = np.ascontiguousarray(start, dtype=np.float64)
        goal = np.ascontiguousarray(goal, dtype=np.float64)
        out = np.zeros(max_states * 10)
        lens = np.zeros(n_cand, dtype=np.int32)
        made = lib().wl_init_paths(self.h, _dp(start), _dp(goal), n_cand, seed, _dp(out), max_states,
                                   lens.ctypes.data_as(c_ip))
        if made < 0:
            raise RuntimeError("init path buffer too small")
        lens = lens[:made]
        tot = int(lens.sum())
        return lens.copy(), out[: tot * 10].reshape(tot, 10).copy()


def sample_start_goal_xy(seed, size_xy=20.0):
    s = np.zeros(3)
    g = np.zeros(3)
    lib().wl_sample_start_goal_xy(seed, size_xy, _dp(s), _dp(g))
    return s, g


def tables_scenario(scenario_id, n_cand, base_seed=42, **world_kw):
    """Reference flow for the 'tables' scene (planner.cpp:498-548): sample start/goal, build the map with 1x1 m
    keep-outs at both, then rejection-sample the arm joints.  Returns (world, start, goal, lens, paths)."""
    seed = base_seed + scenario_id
    for attempt in range(50):
        s3, g3 = sample_start_goal_xy(seed * 1000 + attempt, world_kw.get("size_xy", 20.0))
        w = World(TABLES, seed=seed * 1000 + attempt, keepouts=[s3[:2], g3[:2]], **world_kw)
        start = np.zeros(10)
        goal = np.zeros(10)
        start[:3] = s3
        goal[:3] = g3
        ok1, goal = w.sample_arm(seed * 7919 + 2 * attempt, goal)
        ok2, start = w.sample_arm(seed * 7919 + 2 * attempt + 1, start)
        if not (ok1 and ok2):
            w.close()
            continue
        lens, paths = w.init_paths(start, goal, n_cand, seed * 104729 + attempt)
        if len(lens) == 0:
            w.close()
            continue
        return w, start, goal, lens, paths
    raise RuntimeError("could not build a tables scenario")


def cuboids_batch(n_scenarios, n_cand, map_seed=42, base_seed=42, first_scenario=0, **world_kw):
    """n_scenarios random start/goal pairs x n_cand candidates on ONE cuboids map (BASELINE config 3).
    Returns (world, lens, paths, scenario_of_traj)."""
    w = World(CUBOIDS, seed=map_seed, **world_kw)
    all_lens, all_paths, scen = [], [], []
    sid = first_scenario
    made = 0
    while made < n_scenarios:
        ok, s, g = w.sample_scenario(base_seed + sid)
        sid += 1
        if not ok:
            continue
        lens, paths = w.init_paths(s, g, n_cand, (base_seed + sid) * 104729)
        if len(lens) < n_cand:
            continue
        all_lens.append(lens)
        all_paths.append(paths)
        scen += [made] * len(lens)
        made += 1
    return w, np.concatenate(all_lens), np.concatenate(all_paths), np.asarray(scen, dtype=np.int32)


class TablesBatch:
    """S 'tables' scenarios, one map each, n_cand candidates per scenario (benchmark_tables batch)."""

    def __init__(self, n_scenarios, n_cand, base_seed=42, size_xy=20.0, size_z=1.6, res=0.1, cloud_res=0.05, nthreads=0,
                 keep_esdf3d=None):
        """keep_esdf3d = k: only the first k scenarios keep their CPU-built 3-D distance field (World.esdf3d is None for
        the others); the occupancy grids and the 2-D field are always kept."""
        L = lib()
        L.wl_set_keep_esdf3d(-1 if keep_esdf3d is None else int(keep_esdf3d))
        try:
            self.h = C.c_void_p(L.wl_tables_batch_create(n_scenarios, n_cand, base_seed, size_xy, size_z, res, cloud_res, nthreads))
        finally:
            L.wl_set_keep_esdf3d(-1)
        nt = L.wl_tables_batch_ntraj(self.h)
        ns = L.wl_tables_batch_nstates(self.h)
        self.lens = np.zeros(nt, dtype=np.int32)
        self.scen = np.zeros(nt, dtype=np.int32)
        paths = np.zeros(ns * 10)
        L.wl_tables_batch_get(self.h, self.lens.ctypes.data_as(c_ip), self.scen.ctypes.data_as(c_ip), _dp(paths))
        self.paths = paths.reshape(ns, 10)
        self.dts = np.zeros(ns)             # getDensePath's dt per state: (x, y, theta, dt) is MCRRTs::plan's car path
        L.wl_tables_batch_get_dt.argtypes = [C.c_void_p, c_dp]
        L.wl_tables_batch_get_dt(self.h, _dp(self.dts))
        self.scenarios = sorted(set(self.scen.tolist()))
        self._worlds = {}

    def world(self, sidx):
        if sidx not in self._worlds:
            wp = lib().wl_tables_batch_world(self.h, sidx)
            self._worlds[sidx] = World(TABLES, _borrowed=wp)
        return self._worlds[sidx]

    def close(self):
        if self.h:
            for w in self._worlds.values():
                w.close()
            lib().wl_tables_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def front_end_fields(occ2d, occ3d, dims, res, chassis_radius=0.4, occ2d_critical=None):
    """CPU construction of GridMap's esdf_buffer_2d_inflate and esdf_buffer_2d_critical (grid_map.cpp:211-423) from the
    occupancy grids -- the checker of topay_build_esdf_fields.  Returns (inflate, critical)."""
    L = lib()
    nx, ny, nz = (int(x) for x in dims)
    o2 = np.ascontiguousarray(occ2d, dtype=np.int8)
    o3 = np.ascontiguousarray(occ3d, dtype=np.int8)
    oc = None if occ2d_critical is None else np.ascontiguousarray(occ2d_critical, dtype=np.int8)
    inf = np.zeros(nx * ny)
    cr = np.zeros(nx * ny)
    P8 = C.POINTER(C.c_int8)
    L.wl_edt_front_end_fields.argtypes = [P8, P8, P8, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, c_dp, c_dp]
    L.wl_edt_front_end_fields.restype = None
    L.wl_edt_front_end_fields(o2.ctypes.data_as(P8), None if oc is None else oc.ctypes.data_as(P8), o3.ctypes.data_as(P8), nx, ny, nz,
                              float(res), float(chassis_radius), inf.ctypes.data_as(c_dp), cr.ctypes.data_as(c_dp))
    return inf, cr


def dense_path(raw_xy, start_yaw, end_yaw, step_size=1.414, v_max=1.0, w_max=1.25):
    """CPU restatement of GraphSearch::getDensePath (graph_search.cpp:119-176) -> [m, 4] array (x, y, theta, dt)."""
    L = lib()
    raw = np.ascontiguousarray(raw_xy, dtype=np.float64).reshape(-1, 2)
    cap = 4 * (int(np.ceil(np.linalg.norm(np.diff(raw, axis=0), axis=1) / step_size).clip(1).sum()) + 4)
    out = np.zeros((cap, 4))
    L.wl_dense_path.argtypes = [c_dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, c_dp, C.c_int]
    L.wl_dense_path.restype = C.c_int
    n = L.wl_dense_path(raw.ctypes.data_as(c_dp), len(raw), step_size, start_yaw, end_yaw, v_max, w_max, out.ctypes.data_as(c_dp), cap)
    return out[:n].copy()


# ---- layered joint-space search (MCRRTs::plan) and Reeds-Shepp restatements: libtopay_mcrrt.so --------------------------
_MLIB = None


class McrrtParams(C.Structure):
    """== topay_mcrrt_params_t (include/topay.h), == topay_wl::McrrtParams (harness/mcrrt.hpp)"""
    _fields_ = [("goal_sample_rate", C.c_double), ("check_colli_res", C.c_double), ("rs_turning_radius", C.c_double),
                ("max_iter", C.c_int), ("max_sample_tries", C.c_int), ("node_cap", C.c_int), ("reserved", C.c_int),
                ("seed", C.c_uint64)]

    def __init__(self, **kw):
        super().__init__(0.4, 0.01, 1.0e-2, 1000, 64, 2048, 0, 42)
        for k, v in kw.items():
            setattr(self, k, v)


class McrrtNodeRec(C.Structure):
    _fields_ = [("layer", C.c_int), ("state", C.c_int), ("parent", C.c_int), ("cost", C.c_double), ("q", C.c_double * 7)]


def mlib():
    global _MLIB
    if _MLIB is None:
        path = os.path.join(_HERE, "libtopay_mcrrt.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.wl_mcrrt_plan.argtypes = [C.c_void_p, c_dp, c_dp, C.c_int, c_dp, C.POINTER(McrrtParams), C.c_uint64, C.c_int, c_dp, c_ip, c_ip,
                                    c_dp, c_dp, C.c_int, C.POINTER(McrrtNodeRec)]
        L.wl_rs_path.argtypes = [C.c_double, c_dp, c_dp, c_ip, c_dp]
        L.wl_rs_path.restype = C.c_double
        L.wl_rs_interpolate.argtypes = [C.c_double, c_dp, c_dp, C.c_double, c_dp]
        L.wl_rs_interpolate.restype = None
        L.wl_mcrrt_u01.argtypes = [C.c_uint64] * 4
        L.wl_mcrrt_u01.restype = C.c_double
        L.wl_replan_traj_create.argtypes = [c_dp, C.c_int, c_dp, c_dp]
        L.wl_replan_traj_create.restype = C.c_void_p
        L.wl_replan_traj_destroy.argtypes = [C.c_void_p]
        L.wl_replan_traj_destroy.restype = None
        L.wl_replan_car_seq_len.argtypes = [C.c_void_p]
        L.wl_replan_state.argtypes = [C.c_void_p, C.c_double, c_dp, c_dp]
        L.wl_replan_state.restype = None
        L.wl_replan_safe.argtypes = [C.c_void_p, c_dp, C.c_double, c_ip, c_dp, c_dp, c_dp, c_dp, c_ip, c_dp, c_dp]
        L.wl_replan_endpoints.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, c_dp, C.c_double, C.c_double, c_dp, c_dp, c_dp]
        map_args = [c_dp, C.c_double, c_ip, c_dp, c_dp, c_dp, c_dp]
        L.wl_ee_pose.argtypes = [C.c_int, c_dp, c_dp]
        L.wl_ee_pose.restype = None
        L.wl_ee_eval.argtypes = map_args + [c_dp, c_dp, c_dp, c_dp, c_ip, c_dp]
        L.wl_ee_eval.restype = C.c_double
        L.wl_ee_optimize.argtypes = map_args + [c_dp, c_dp, c_ip, C.c_double, C.c_double, c_dp, c_ip]
        L.wl_pm_create.argtypes = [c_dp, C.c_double, c_ip]
        L.wl_pm_create.restype = C.c_void_p
        L.wl_pm_destroy.argtypes = [C.c_void_p]
        L.wl_pm_destroy.restype = None
        L.wl_pm_update.argtypes = [C.c_void_p, C.c_int, C.c_void_p, c_dp, C.c_void_p]
        L.wl_pm_get.argtypes = [C.c_void_p, C.c_void_p, c_ip, c_ip, c_ip]
        L.wl_pm_get.restype = None
        L.wl_pm_slide.argtypes = [C.c_void_p, c_dp, C.c_double, C.c_int, c_ip, c_dp]
        L.wl_pm_occupancy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wl_pm_occupancy.restype = None
        L.wl_pm_logodds.argtypes = [C.c_void_p, C.c_void_p]
        L.wl_pm_logodds.restype = None
        L.wl_pm_scan.argtypes = [C.c_void_p, c_dp, C.c_double, c_ip, c_dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
        L.wl_pm_scan.restype = None
        L.wl_ompc_create.argtypes = [C.c_void_p]
        L.wl_ompc_create.restype = C.c_void_p
        L.wl_ompc_destroy.argtypes = [C.c_void_p]
        L.wl_ompc_destroy.restype = None
        L.wl_ompc_set_direct.argtypes = [C.c_void_p, C.c_int, c_dp]
        L.wl_ompc_set_direct.restype = None
        L.wl_ompc_cmd.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_dp]
        L.wl_ompc_cmd.restype = None
        L.wl_ompc_get.argtypes = [C.c_void_p, c_dp, c_dp]
        L.wl_ompc_get.restype = None
        L.wl_ompc_probe.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double] + [c_dp] * 10 + [c_ip]
        L.wl_sim_create.argtypes = [c_dp, C.c_int]
        L.wl_sim_create.restype = C.c_void_p
        L.wl_sim_destroy.argtypes = [C.c_void_p]
        L.wl_sim_destroy.restype = None
        L.wl_sim_step.argtypes = [C.c_void_p, c_dp, C.c_int, c_dp]
        L.wl_sim_step.restype = None
        _MLIB = L
    return _MLIB


class ProbMapCheck:
    """The CPU checker of the sensor-cloud entries (harness/prob_map.hpp): one ProbMap on a grid.  params: a ctypes structure with
    the layout of topay_sense_params_t (topay_amd.api.SenseParams)."""

    def __init__(self, origin, res, dims):
        self.origin = np.ascontiguousarray(origin, dtype=np.float64)
        self.dims = np.ascontiguousarray(dims, dtype=np.int32)
        self.res = float(res)
        self.h = mlib().wl_pm_create(_dp(self.origin), self.res, self.dims.ctypes.data_as(c_ip))

    def __del__(self):
        if getattr(self, "h", None):
            mlib().wl_pm_destroy(self.h)
            self.h = None

    def update(self, cloud, sensor, params):
        pts = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
        sp = np.ascontiguousarray(sensor, dtype=np.float64)
        return mlib().wl_pm_update(self.h, len(pts), pts.ctypes.data, _dp(sp), C.addressof(params))

    def get(self):
        d = tuple(int(v) for v in self.dims)
        lo, op, hit = np.zeros(d, dtype=np.float32), np.zeros(d, dtype=np.int32), np.zeros(d, dtype=np.int32)
        bc = C.c_int(0)
        mlib().wl_pm_get(self.h, lo.ctypes.data, op.ctypes.data_as(c_ip), hit.ctypes.data_as(c_ip), C.byref(bc))
        return lo, op, hit, bc.value

    def slide(self, sensor, params):
        """ProbMap::slide for one sensor position.  params: threshold and slide_z (topay_amd.api.SenseSlideParams).  Returns
        (status, shift int32[3]); self.origin is the grid's origin after it."""
        sp = np.ascontiguousarray(sensor, dtype=np.float64)
        shift = np.zeros(3, dtype=np.int32)
        st = mlib().wl_pm_slide(self.h, _dp(sp), float(params.threshold), int(params.slide_z), shift.ctypes.data_as(c_ip), _dp(self.origin))
        return st, shift

    def occupancy(self, params):
        nx, ny, nz = (int(v) for v in self.dims)
        o2, oc, o3 = np.zeros((nx, ny), dtype=np.int8), np.zeros((nx, ny), dtype=np.int8), np.zeros((nx, ny, nz), dtype=np.int8)
        mlib().wl_pm_occupancy(self.h, C.addressof(params), o2.ctypes.data, oc.ctypes.data, o3.ctypes.data)
        return o2, oc, o3


def pm_logodds(params):
    out = np.zeros(6, dtype=np.float32)
    mlib().wl_pm_logodds(C.addressof(params), out.ctypes.data)
    return out


def pm_scan(occ3d, origin, res, dims, pose, n_az, n_el, fov, rng):
    """The checker's range sensor for one pose (x, y, z, yaw): points float32[n_az * n_el, 4]."""
    o3 = np.ascontiguousarray(occ3d, dtype=np.int8)
    org, dm, ps = np.ascontiguousarray(origin, dtype=np.float64), np.ascontiguousarray(dims, dtype=np.int32), np.ascontiguousarray(pose, dtype=np.float64)
    out = np.zeros((n_az * n_el, 4), dtype=np.float32)
    mlib().wl_pm_scan(o3.ctypes.data, _dp(org), float(res), dm.ctypes.data_as(c_ip), _dp(ps), n_az, n_el, float(fov), float(rng), out.ctypes.data)
    return out


class EeGoal:
    """CPU restatement of getFKPose, eeCostCallback (gradient assigned) and optimizeEE on one map (harness/ee_goal.hpp)."""

    def __init__(self, origin, res, dims, min_b, max_b, esdf2d, esdf3d):
        self.L = mlib()
        self.org = np.ascontiguousarray(origin, dtype=np.float64)
        self.res = float(res)
        self.dm = np.ascontiguousarray(dims, dtype=np.int32)
        self.mn, self.mx = np.ascontiguousarray(min_b, dtype=np.float64), np.ascontiguousarray(max_b, dtype=np.float64)
        self.e2, self.e3 = np.ascontiguousarray(esdf2d, dtype=np.float64), np.ascontiguousarray(esdf3d, dtype=np.float64)

    def _map(self):
        return (_dp(self.org), self.res, self.dm.ctypes.data_as(c_ip), _dp(self.mn), _dp(self.mx), _dp(self.e2), _dp(self.e3))

    @staticmethod
    def pose(states):
        """getFKPose of [n, 10] states: [n, 9]."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        out = np.zeros((len(st), 9))
        mlib().wl_ee_pose(len(st), _dp(st), _dp(out))
        return out

    def eval(self, x, ee_ref):
        """eeCostCallback at the unconstrained x: (f, g [10], dict(terms = ee / mani / chassis / pairs, n_mani, n_chassis, n_pairs,
        n_outside, kink_penalty, kink_cell, kink_sigmoid))."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        ref = np.ascontiguousarray(ee_ref, dtype=np.float64)
        g, terms, counts, kinks = np.zeros(10), np.zeros(4), np.zeros(4, dtype=np.int32), np.zeros(3)
        f = self.L.wl_ee_eval(*self._map(), _dp(x), _dp(ref), _dp(g), _dp(terms), counts.ctypes.data_as(c_ip), _dp(kinks))
        return float(f), g, dict(terms=dict(zip(("ee", "mani", "chassis", "pairs"), terms)), n_mani=int(counts[0]), n_chassis=int(counts[1]),
                                 n_pairs=int(counts[2]), n_outside=int(counts[3]), kink_penalty=float(kinks[0]), kink_cell=float(kinks[1]),
                                 kink_sigmoid=float(kinks[2]))

    def optimize(self, seed_state, ee_ref, mem_size=64, past=3, max_iterations=10000, max_linesearch=64, g_epsilon=1e-5, delta=1e-4):
        """optimizeEE: (state [10], cost, code, iters, evals); the seed comes back for a code outside the reference's success set."""
        st = np.array(seed_state, dtype=np.float64)
        ref = np.ascontiguousarray(ee_ref, dtype=np.float64)
        lb = np.array([mem_size, past, max_iterations, max_linesearch], dtype=np.int32)
        cost, oi = np.zeros(1), np.zeros(2, dtype=np.int32)
        code = self.L.wl_ee_optimize(*self._map(), _dp(st), _dp(ref), lb.ctypes.data_as(c_ip), float(g_epsilon), float(delta), _dp(cost),
                                     oi.ctypes.data_as(c_ip))
        return st, float(cost[0]), int(code), int(oi[0]), int(oi[1])


class ReplanTraj:
    """CPU restatement of MomaTraj with Planner::safeCallback and the endpoints of Planner::replanCallback (harness/replan.hpp).
    start3 = (x, y, theta), durations [N], coeffs [N, 9, 6] with the highest order first, as setTraj takes them."""

    def __init__(self, start3, durations, coeffs):
        self.L = mlib()
        s3 = np.ascontiguousarray(start3, dtype=np.float64).reshape(-1)[:3].copy()
        dur = np.ascontiguousarray(durations, dtype=np.float64).reshape(-1)
        co = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1)
        assert len(co) == 54 * len(dur)
        self.T = float(np.add.accumulate(dur)[-1])
        self.h = self.L.wl_replan_traj_create(_dp(s3), len(dur), _dp(dur), _dp(co))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.wl_replan_traj_destroy(self.h)
            self.h = None

    def state(self, t):
        """(getState(t), getDState(t))"""
        s, d = np.zeros(10), np.zeros(10)
        self.L.wl_replan_state(self.h, float(t), _dp(s), _dp(d))
        return s, d

    def safe(self, origin, res, dims, min_b, max_b, esdf2d, esdf3d):
        """safeCallback against the given fields: dict(safe, sample, body, t, d, min_margin) -- min_margin = the smallest
        |d - 0.99 r| over every body of every sample up to and including the first hit."""
        org = np.ascontiguousarray(origin, dtype=np.float64)
        dm = np.ascontiguousarray(dims, dtype=np.int32)
        mn, mx = np.ascontiguousarray(min_b, dtype=np.float64), np.ascontiguousarray(max_b, dtype=np.float64)
        e2, e3 = np.ascontiguousarray(esdf2d, dtype=np.float64), np.ascontiguousarray(esdf3d, dtype=np.float64)
        fh, hit, mm = np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(1)
        ok = self.L.wl_replan_safe(self.h, _dp(org), float(res), dm.ctypes.data_as(c_ip), _dp(mn), _dp(mx), _dp(e2), _dp(e3), fh.ctypes.data_as(c_ip),
                                   _dp(hit), _dp(mm))
        return dict(safe=bool(ok), sample=int(fh[0]), body=int(fh[1]), t=float(hit[0]), d=float(hit[1]), min_margin=float(mm[0]))

    def endpoints(self, global_traj, t_since_replan, t_since_begin, global_goal, planning_budget, planning_horizon):
        """replanCallback:708-731 with this trajectory as end_traj: (start, start_v, goal, goal_source)."""
        gg = np.ascontiguousarray(global_goal, dtype=np.float64)
        st, sv, go = np.zeros(10), np.zeros(10), np.zeros(10)
        src = self.L.wl_replan_endpoints(self.h, global_traj.h if global_traj is not None else None, float(t_since_replan), float(t_since_begin),
                                         _dp(gg), float(planning_budget), float(planning_horizon), _dp(st), _dp(sv), _dp(go))
        return st, sv, go, int(src)


def mcrrt_plan(world, start, end, car_path, params=None, inst=0, track_slack=False, want_nodes=True):
    """CPU restatement of MCRRTs::plan (mcrrts.cpp:5-231) on `world`.  car_path: [L, 4] (x, y, theta, dt).  Returns a dict:
    status (1 path / 0 none / -1 node pool full), wb_path [m, 10], stats (8 ints), c_max, min_slack, nodes (structured array:
    layer, state, parent, cost, q -- in creation order)."""
    L = mlib()
    prm = params or McrrtParams()
    cp = np.ascontiguousarray(car_path, dtype=np.float64).reshape(-1, 4)
    st = np.ascontiguousarray(start, dtype=np.float64)
    en = np.ascontiguousarray(end, dtype=np.float64)
    wb = np.zeros((len(cp), 10))
    wl_, stats = C.c_int(0), np.zeros(8, dtype=np.int32)
    cmax, slack = C.c_double(0), C.c_double(0)
    nodes = (McrrtNodeRec * prm.node_cap)() if want_nodes else None
    s = L.wl_mcrrt_plan(world.h, _dp(st), _dp(en), len(cp), _dp(cp), C.byref(prm), int(inst), int(track_slack), _dp(wb), C.byref(wl_),
                        stats.ctypes.data_as(c_ip), C.byref(cmax), C.byref(slack), prm.node_cap, nodes)
    out = dict(status=int(s), wb_path=wb[:wl_.value].copy(), stats=stats, c_max=cmax.value, min_slack=slack.value, nodes=None)
    if want_nodes:
        rec = np.dtype([("layer", "<i4"), ("state", "<i4"), ("parent", "<i4"), ("pad", "<i4"), ("cost", "<f8"), ("q", "<f8", (7,))])
        assert rec.itemsize == C.sizeof(McrrtNodeRec)
        out["nodes"] = np.frombuffer(nodes, dtype=rec, count=prm.node_cap)[:stats[1]].copy()
    return out


def plan2d_jps(world, start_xy, end_xy, threshold=0.5, cap=4096):
    """CPU restatement of GraphSearch::plan2dJPS (graph_search.cpp:53-117) -> ([m, 2] path, empty when none; (expanded nodes,
    jump points of the raw path))."""
    L = mlib()
    L.wl_plan2d_jps.argtypes = [C.c_void_p, c_dp, c_dp, C.c_double, C.c_int, c_dp, c_ip]
    a = np.ascontiguousarray(start_xy, dtype=np.float64)
    b = np.ascontiguousarray(end_xy, dtype=np.float64)
    out = np.zeros((cap, 2))
    st = np.zeros(2, dtype=np.int32)
    n = L.wl_plan2d_jps(world.h, _dp(a), _dp(b), float(threshold), cap, _dp(out), st.ctypes.data_as(c_ip))
    return out[:min(n, cap)].copy(), (int(st[0]), int(st[1]))


def rs_path(from_pose, to_pose, rho=1.0e-2):
    """ompl::base::ReedsSheppStateSpace(rho).reedsShepp(from, to) restated: (word 0..17, five signed lengths, distance)."""
    L = mlib()
    a = np.ascontiguousarray(from_pose, dtype=np.float64)
    b = np.ascontiguousarray(to_pose, dtype=np.float64)
    t, ln = C.c_int(0), np.zeros(5)
    d = L.wl_rs_path(rho, _dp(a), _dp(b), C.byref(t), _dp(ln))
    return t.value, ln, d


def rs_interpolate(from_pose, to_pose, t, rho=1.0e-2):
    L = mlib()
    a = np.ascontiguousarray(from_pose, dtype=np.float64)
    b = np.ascontiguousarray(to_pose, dtype=np.float64)
    out = np.zeros(3)
    L.wl_rs_interpolate(rho, _dp(a), _dp(b), float(t), _dp(out))
    return out


# ---- topological roadmap (TopologyPRM::findTopoPaths) restatement: harness/topo_prm.hpp ---------------------------------
TOPO_MAX_NB = 32


class TopoParams(C.Structure):
    """== topay_topo_params_t (include/topay.h), == topay_wl::TopoParams (harness/topo_prm.hpp)"""
    _fields_ = [("sample_inflate_x", C.c_double), ("sample_inflate_y", C.c_double), ("clearance", C.c_double),
                ("ratio_to_short", C.c_double), ("max_sample_num", C.c_int), ("max_raw_path", C.c_int), ("max_raw_path2", C.c_int),
                ("reserve_num", C.c_int), ("node_cap", C.c_int), ("reserved", C.c_int), ("seed", C.c_uint64)]

    def __init__(self, **kw):
        super().__init__(1.5, 4.0, 0.1, 2.0, TOPO_DEFAULT_SAMPLES, 300, 25, 6, 512, 0, 42)
        for k, v in kw.items():
            setattr(self, k, v)


TOPO_DEFAULT_SAMPLES = 2368   # == topay_topo_default_params (docs/EXPERIMENTS.md, "Sampling budget of the roadmap")


def world_front_end_fields(world, chassis_radius=0.4):
    """(inflate, critical) of a World, built once with the CPU construction and kept on the object."""
    f = getattr(world, "_front_end_fields", None)
    if f is None:
        f = front_end_fields(world.occ2d, world.occ3d, world.dims, world.res, chassis_radius)
        world._front_end_fields = f
    return f


def _topo_lib():
    L = mlib()
    if not getattr(L, "_topo_ready", False):
        L.wl_topo_run.restype = C.c_void_p
        L.wl_topo_run.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, c_dp, C.POINTER(TopoParams), C.c_uint64, C.c_int, C.c_int, c_ip, c_ip, c_dp]
        L.wl_topo_free.argtypes = [C.c_void_p]
        L.wl_topo_free.restype = None
        L.wl_topo_graph_size.argtypes = [C.c_void_p]
        L.wl_topo_graph.argtypes = [C.c_void_p, c_ip, c_ip, c_dp, c_ip, c_ip]
        L.wl_topo_graph.restype = None
        L.wl_topo_get_paths.argtypes = [C.c_void_p, C.c_int, c_ip, c_dp]
        L.wl_topo_ray_cells.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, C.c_int, c_ip]
        L.wl_topo_samples_in.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, c_dp, C.POINTER(TopoParams), C.c_uint64, C.c_double]
        L._topo_ready = True
    return L


def topo_paths(world, start, goal, params=None, inst=0, critical=False, track_slack=True, fields=None):
    """CPU restatement of TopologyPRM::findTopoPaths on `world` (fields = (inflate, critical) arrays; default: the CPU
    construction for a 0.4 m chassis).  Returns a dict: status, paths (select_paths: list of [m, 2]), stats (8 ints as
    topay_topo_paths), graph (id, type, pos, n_nb, nb in list order), raw_paths, short_paths, min_slack, moves, pushes."""
    L = _topo_lib()
    prm = params or TopoParams()
    inf, cr = fields if fields is not None else world_front_end_fields(world)
    inf = np.ascontiguousarray(inf, dtype=np.float64)
    cr = np.ascontiguousarray(cr, dtype=np.float64)
    a = np.ascontiguousarray(np.asarray(start, dtype=np.float64)[:2])
    b = np.ascontiguousarray(np.asarray(goal, dtype=np.float64)[:2])
    stats, cnt, slack = np.zeros(8, dtype=np.int32), np.zeros(2, dtype=np.int32), C.c_double(0)
    h = C.c_void_p(L.wl_topo_run(world.h, _dp(inf), _dp(cr), _dp(a), _dp(b), C.byref(prm), int(inst), int(bool(critical)), int(bool(track_slack)),
                                 stats.ctypes.data_as(c_ip), cnt.ctypes.data_as(c_ip), C.byref(slack)))
    try:
        n = L.wl_topo_graph_size(h)
        g = dict(id=np.zeros(n, dtype=np.int32), type=np.zeros(n, dtype=np.int32), pos=np.zeros((n, 2)), n_nb=np.zeros(n, dtype=np.int32),
                 nb=np.zeros((n, TOPO_MAX_NB), dtype=np.int32))
        L.wl_topo_graph(h, g["id"].ctypes.data_as(c_ip), g["type"].ctypes.data_as(c_ip), _dp(g["pos"]), g["n_nb"].ctypes.data_as(c_ip),
                        g["nb"].ctypes.data_as(c_ip))

        def paths(which):
            m = L.wl_topo_get_paths(h, which, None, None)
            lens = np.zeros(max(m, 1), dtype=np.int32)
            L.wl_topo_get_paths(h, which, lens.ctypes.data_as(c_ip), None)
            xy = np.zeros((max(int(lens[:m].sum()), 1), 2))
            L.wl_topo_get_paths(h, which, lens.ctypes.data_as(c_ip), _dp(xy))
            o = np.concatenate([[0], np.cumsum(lens[:m])])
            return [xy[o[i]:o[i + 1]].copy() for i in range(m)]

        ok = stats[0] >= 0
        return dict(status=int(stats[0]), paths=paths(2), stats=stats, graph=g, raw_paths=paths(0) if ok else [], short_paths=paths(1) if ok else [],
                    min_slack=slack.value, moves=int(cnt[0]), pushes=int(cnt[1]))
    finally:
        L.wl_topo_free(h)


def topo_ray_cells(world, p1, p2, cap=4096):
    """The cells TopologyPRM::lineVisib tests for the ray p1 -> p2, in order (before boundIndex2d clamps them)."""
    L = _topo_lib()
    inf = np.ascontiguousarray(world_front_end_fields(world)[0])
    a = np.ascontiguousarray(p1, dtype=np.float64)
    b = np.ascontiguousarray(p2, dtype=np.float64)
    cells = np.zeros((cap, 2), dtype=np.int32)
    n = L.wl_topo_ray_cells(world.h, _dp(inf), _dp(a), _dp(b), cap, cells.ctypes.data_as(c_ip))
    return cells[:min(n, cap)].copy()


def topo_samples_in(world, start, goal, seconds=0.01, params=None, inst=0):
    """Samples createGraph draws in `seconds` of loop time on this host, one thread (the reference's max_sample_time rule)."""
    L = _topo_lib()
    inf, cr = world_front_end_fields(world)
    prm = params or TopoParams()
    a = np.ascontiguousarray(np.asarray(start, dtype=np.float64)[:2])
    b = np.ascontiguousarray(np.asarray(goal, dtype=np.float64)[:2])
    return int(L.wl_topo_samples_in(world.h, _dp(np.ascontiguousarray(inf)), _dp(np.ascontiguousarray(cr)), _dp(a), _dp(b), C.byref(prm), int(inst), float(seconds)))


class OmpcCheck:
    """The CPU checker of the tracking controller (harness/ompc.hpp): one OMPC.  params: a ctypes structure with the layout of
    topay_mpc_params_t (topay_amd.api.MpcParams).  The trajectory is the caller's: rows [T, 3] = getState(t)[:3] at t = t_cur + dt,
    += dt; arm_q / arm_dq [7] = getState / getDState(t_cur + 1 / ctrl_freq)[3:]."""

    def __init__(self, params):
        self.T = int(params.predict_steps)
        self.maxd = max(int(params.delay_num_v), int(params.delay_num_w))
        self.nx = 3 * (self.T - params.delay_num_w) + (self.T - params.delay_num_v) + (self.T - params.delay_num_w)
        self.nc = self.nx + (self.T - params.delay_num_v) + (self.T - params.delay_num_w) - 2
        self.h = mlib().wl_ompc_create(C.addressof(params))

    def __del__(self):
        if getattr(self, "h", None):
            mlib().wl_ompc_destroy(self.h)
            self.h = None

    def set_direct(self, pos3=None):
        p = np.zeros(3) if pos3 is None else np.ascontiguousarray(pos3, dtype=np.float64)
        mlib().wl_ompc_set_direct(self.h, 0 if pos3 is None else 1, _dp(p))

    def cmd(self, t_cur, now_state, rows=None, arm_q=None, arm_dq=None, T_total=0.0, has_traj=True):
        """(cmd [16], status [4], xopt [T + 1, 3])"""
        ns = np.ascontiguousarray(now_state, dtype=np.float64)
        rw = np.zeros((self.T, 3)) if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
        q = np.zeros(7) if arm_q is None else np.ascontiguousarray(arm_q, dtype=np.float64)
        dq = np.zeros(7) if arm_dq is None else np.ascontiguousarray(arm_dq, dtype=np.float64)
        cmd, st, xo = np.zeros(16), np.zeros(4, dtype=np.int32), np.zeros((self.T + 1, 3))
        mlib().wl_ompc_cmd(self.h, 1 if has_traj else 0, float(t_cur), float(T_total), _dp(ns), _dp(rw), _dp(q), _dp(dq), _dp(cmd),
                           st.ctypes.data_as(c_ip), _dp(xo))
        return cmd, st, xo

    def get(self):
        out, ff = np.zeros((2, self.T)), np.zeros((self.maxd, 2))
        mlib().wl_ompc_get(self.h, _dp(out), _dp(ff))
        return out, ff

    def probe(self, t_cur, now_state, rows=None, T_total=0.0, has_traj=True):
        ns = np.ascontiguousarray(now_state, dtype=np.float64)
        rw = np.zeros((self.T, 3)) if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
        nx, nc = self.nx, self.nc
        o = dict(P=np.zeros((nx, nx)), q=np.zeros(nx), A=np.zeros((nc, nx)), l=np.zeros(nc), u=np.zeros(nc), x=np.zeros(nx), y=np.zeros(nc),
                 z=np.zeros(nc))
        info = np.zeros(2, dtype=np.int32)
        ok = mlib().wl_ompc_probe(self.h, 1 if has_traj else 0, float(t_cur), float(T_total), _dp(ns), _dp(rw), _dp(o["P"]), _dp(o["q"]),
                                  _dp(o["A"]), _dp(o["l"]), _dp(o["u"]), _dp(o["x"]), _dp(o["y"]), _dp(o["z"]), info.ctypes.data_as(c_ip))
        if not ok:
            return None
        o["iters"], o["solved"] = int(info[0]), int(info[1])
        return o


class SimCheck:
    """The CPU checker of the fake robot (harness/ompc.hpp)."""

    def __init__(self, state0, delay_cmds=20):
        s0 = np.ascontiguousarray(state0, dtype=np.float64)
        self.h = mlib().wl_sim_create(_dp(s0), int(delay_cmds))

    def __del__(self):
        if getattr(self, "h", None):
            mlib().wl_sim_destroy(self.h)
            self.h = None

    def step(self, cmd, ticks):
        st = np.zeros(10)
        cm = None if cmd is None else np.ascontiguousarray(cmd, dtype=np.float64)
        mlib().wl_sim_step(self.h, None if cm is None else _dp(cm), int(ticks), _dp(st))
        return st
