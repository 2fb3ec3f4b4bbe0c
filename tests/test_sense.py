"""Sensor clouds into the map (topay_amd/csrc/topay_sense.h, include/topay.h topay_sense_*): rog_map's ProbMap on the grid of a
map slot, the grids and fields derived from the belief, and the range sensor.

Without a device the CPU lane emulator of the kernel sources is compared with the sequential checker (harness/prob_map.hpp);
marked gpu, the device is compared with the emulator.  Everything is compared bit for bit: log-odds, both count arrays, the batch
counter, the occupancy grids, the five fields, the scan's points.

Shapes: 24 x 24 x 12 voxels.  Most cases use 0.1 m voxels with the origin at (-1.2, -1.2, 0); the cases that need a point exactly
on a voxel face or corner use 0.125 m voxels with the origin at (-1.5, -1.5, 0), where every boundary is a binary fraction.  The
commit and scan cases use a 2.4 x 2.4 x 1.6 m tables world (24 x 24 x 16: the 16-layer columns take the 16-byte stores).

The end-to-end episode (two robots, a 10 x 10 x 1.6 m tables world) runs the planning call with capped solver iterations on both
sides; its emulator run takes about 20 s and is shared by the CPU and the GPU test.
"""
import functools
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB, ROOT
from harness import workload as wl
from topay_amd import api

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
GRID = dict(origin=(-1.2, -1.2, 0.0), res=0.1, dims=(24, 24, 12), min_b=(-1.2, -1.2, 0.0), max_b=(1.2, 1.2, 1.2))
GRID8 = dict(origin=(-1.5, -1.5, 0.0), res=0.125, dims=(24, 24, 12), min_b=(-1.5, -1.5, 0.0), max_b=(1.5, 1.5, 1.5))
SENSOR = (0.05, 0.05, 0.55)   # the centre of voxel (12, 12, 5) of GRID
NEW_ENTRIES = ["topay_sense_default_params", "topay_sense_logodds", "topay_sense_reset", "topay_sense_insert", "topay_sense_commit",
               "topay_sense_get", "topay_sense_scan", "topay_sense_ms"]


@functools.lru_cache(maxsize=None)
def _opt(backend):
    return api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB if backend == "emu" else None)


def _pts(xyz, intensity=0.0):
    a = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([a, np.full((len(a), 1), intensity, dtype=np.float32)], axis=1)


def _same(a, b):
    return a[3] == b[3] and all(x.dtype == y.dtype and x.shape == y.shape and (x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a[:3], b[:3]))


def _run_lib(backend, grid, steps, slot=7):
    """steps: (cloud, sensor, params) per insert.  The belief and the status after every insert."""
    opt = _opt(backend)
    opt.sense_reset([slot], **grid)
    out = []
    for cloud, sensor, prm in steps:
        st = int(opt.sense_insert([slot], [cloud], [sensor], prm)[0])
        out.append(opt.sense_get(slot) + (st,))
    return out


def _run_checker(grid, steps):
    pm = wl.ProbMapCheck(grid["origin"], grid["res"], grid["dims"])
    out = []
    for cloud, sensor, prm in steps:
        st = pm.update(cloud, sensor, prm)
        out.append(pm.get() + (st,))
    return out


@functools.lru_cache(maxsize=None)
def _emu_cached(key):
    return _run_lib("emu", *_CASES[key])


_CASES = {}


def _check(backend, key, grid, steps):
    """emu: the emulator against the checker; gpu: the device against the emulator.  Returns the backend's states."""
    _CASES[key] = (grid, steps)
    want = _run_checker(grid, steps) if backend == "emu" else _emu_cached(key)
    got = _emu_cached(key) if backend == "emu" else _run_lib("gpu", grid, steps)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[4] == w[4], (key, i, g[4], w[4])
        assert _same(g, w), (key, i, int((g[0] != w[0]).sum()), int((g[1] != w[1]).sum()), int((g[2] != w[2]).sum()), g[3], w[3])
    return got


def _prm(**kw):
    kw.setdefault("point_filt_num", 1)
    return _opt("emu").sense_params(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. symbols and defaults
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_default_parameters():
    import __graft_entry__ as entry
    entry.build_hip()
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    declared = set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M))
    hip, em = api.load(), api.load(EMU_LIB)
    for n in NEW_ENTRIES:
        assert n in declared, n
        assert hasattr(hip, n), f"{n} not exported by the HIP library"
        assert hasattr(em, n), f"{n} not exported by the emulator library"
    for n in ("sense_params", "sense_reset", "sense_insert", "sense_commit", "sense_get", "sense_scan", "sense_ms", "sense_logodds"):
        assert hasattr(api.MomaTrajOptBatch, n), n
    p = _opt("emu").sense_params()
    f32 = np.float32
    assert (f32(p.p_min), f32(p.p_miss), f32(p.p_free), f32(p.p_occ), f32(p.p_hit), f32(p.p_max)) == (f32(.12), f32(.49), f32(.499), f32(.85), f32(.9), f32(.98))
    assert list(p.ray_range) == [0.0, 5.0] and p.point_filt_num == 15 and p.batch_update_size == 1 and p.intensity_thresh == -10
    assert p.virtual_ceil_height == 9999.0 and p.virtual_ground_height == -9999.0 and list(p.local_update_box) == [50.0, 50.0, 5.0]
    assert p.chassis_height == 0.155
    # the log-odds: library, checker and config.hpp:229-235 restated here (float quotient, double logarithm, rounded to float)
    want = np.array([f32(np.log(np.float64(f32(x) / (f32(1) - f32(x))))) for x in (.9, .49, .12, .98, .85, .499)], dtype=f32)
    assert (_opt("emu").sense_logodds(p) == want).all() and (wl.pm_logodds(p) == want).all()
    assert want[5] < 0 < want[4]   # a fresh voxel (0, prob_map.cpp:78) is unknown


# ---------------------------------------------------------------------------------------------------------------------
# 2. traversal and clamp edge cases
# ---------------------------------------------------------------------------------------------------------------------
S8, C8 = (0.0625, 0.125, 0.5625), (0.0, 0.0, 0.5)   # GRID8: y exactly on a voxel face; a voxel corner
EDGE = {
    "axis_aligned": (GRID, SENSOR, [(0.85, 0.05, 0.55)], {}),
    "own_voxel": (GRID, SENSOR, [(0.07, 0.06, 0.56)], {}),
    "two_in_one_voxel": (GRID, SENSOR, [(0.51, 0.32, 0.55), (0.53, 0.33, 0.57)], {}),
    "hit_and_crossed": (GRID, SENSOR, [(0.55, 0.05, 0.55), (0.95, 0.05, 0.55)], {}),
    "beyond_range_max": (GRID, SENSOR, [(1.0, 0.3, 0.7), (-0.2, 0.1, 0.5)], dict(ray_range=[0.0, 0.6])),
    "outside_map": (GRID, SENSOR, [(3.0, 0.5, 0.6), (-0.4, -2.5, 0.3), (0.2, 0.3, 1.7)], {}),
    "ceil_and_ground": (GRID, SENSOR, [(0.5, 0.2, 1.1), (0.4, -0.3, 0.05), (0.3, 0.3, 0.5)], dict(virtual_ceil_height=0.9, virtual_ground_height=0.2)),
    "along_a_face": (GRID8, S8, [(1.0625, 0.125, 0.5625), (1.0625, 1.125, 0.5625), (-0.9375, 0.125, 0.5625)], {}),
    # the sensor outside updateLocalBox's box (clipped to voxel centres): the box intersection can move a point BEYOND the range
    "sensor_in_outer_half_voxel": (GRID, (-1.19, -1.0, 0.55), [(-1.18, -0.5, 0.55), (0.3, 0.2, 0.6)], dict(ray_range=[0.0, 0.6])),
    "sensor_outside_map": (GRID, (-1.3, 0.1, 0.5), [(-0.5, 0.1, 0.5), (-1.25, 0.4, 0.5), (0.4, -0.3, 0.7)], dict(ray_range=[0.0, 0.6])),
    # the sensor exactly ON a face of that box (the centre plane of a border voxel), a point just beyond the face: the intersection's
    # t on that axis is -0, which `t > 0` rejects, and the other axes move the point beyond the range as well
    "sensor_on_box_face_z": (GRID8, (0.0625, 0.0625, 0.0625), [(0.3625, 0.0625, 0.0625 - 1e-6)], dict(ray_range=[0.0, 0.6])),
    "sensor_on_box_face_x": (GRID8, (-1.4375, 0.0625, 0.5625), [(-1.4375 - 1e-6, 0.3625, 0.5625), (1.4375, 0.0625, 0.5625)], dict(ray_range=[0.0, 0.6])),
    "sensor_on_box_face_max": (GRID8, (1.4375, 1.4375, 1.4375), [(1.4375 + 1e-6, 1.1, 1.4375), (1.2, 1.4375 + 1e-6, 1.4375)], dict(ray_range=[0.0, 0.6])),
    # a diagonal ray whose end lies on a voxel edge: on the last tie `step` moves the axis that has arrived, passes the end voxel
    # and runs on to the map's edge, far beyond the point and the range (RayCaster::step ends on equality only, raycaster.cpp:149-156)
    "overshoot_on_a_tie": (GRID8, (-0.9375, 1.0625, 0.5625), [(-0.625, 0.75, 0.5625)], dict(ray_range=[0.0, 0.6])),
    "sensor_on_corner": (GRID8, C8, [(-0.8, -0.8, 0.2), (0.9, 0.9, 1.0), (0.75, -0.75, 0.5), (0.0, 1.0, 0.5), (0.5, 0.25, 0.75)], dict(ray_range=[0.0, 5.0])),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(EDGE))
def test_traversal_and_clamp_edge_cases(backend, case):
    grid, sensor, pts, kw = EDGE[case]
    prm = _prm(**kw)
    two = _prm(batch_update_size=2, **kw)   # then twice into an open batch: the counts are visible after the first of them
    got = _check(backend, "edge_" + case, grid, [(_pts(pts), sensor, prm), (_pts(pts), sensor, two), (_pts(pts), sensor, two)])
    no_hit = case in ("outside_map", "sensor_in_outer_half_voxel", "sensor_outside_map") or case.startswith("sensor_on_box_face")
    assert got[1][4] == 0 and got[1][1].sum() >= got[1][2].sum() > (-1 if no_hit else 0) and got[2][4] == 1
    lo, op, hit, bc, st = got[0]
    assert st == 1 and bc == 0 and op.sum() == 0 and hit.sum() == 0 and ((lo != 0).any() or case == "sensor_outside_map")
    assert got[2][1].sum() == 0 and got[2][2].sum() == 0   # a flush leaves no count behind, wherever the rays went
    l = _opt("emu").sense_logodds(prm)
    if case == "own_voxel":        # setInput returns false: no miss anywhere, the hit is recorded
        assert (lo != 0).sum() == 1 and lo[12, 12, 5] == l[0]
    if case == "two_in_one_voxel":  # hit_cnt 2 in the open batch; 2 l_hit is above l_max, so the flushed voxel holds l_max
        assert got[1][2][17, 15, 5] == 2 and got[1][1][17, 15, 5] == 2 and lo[17, 15, 5] == l[3] and l[0] * np.float32(2) > l[3]
    if case == "hit_and_crossed":   # hit wins: the voxel of the first point takes l_hit although the second ray crosses it
        assert lo[17, 12, 5] == l[0] and lo[21, 12, 5] == l[0] and lo[18, 12, 5] == l[1]
    if case in ("beyond_range_max", "outside_map"):
        assert (lo > 0).sum() == (1 if case == "beyond_range_max" else 0)   # clamped points record misses only
    if case.startswith("sensor_on_box_face"):   # the point was moved beyond the range: voxels further than 0.6 m + a voxel's diagonal counted
        idx = np.argwhere(got[1][1] > 0)
        s_idx = np.floor((np.array(sensor) - np.array(grid["origin"])) / grid["res"])
        assert len(idx) and np.abs(idx - s_idx).max() * grid["res"] > 0.6 + 2 * grid["res"]
    if case == "overshoot_on_a_tie":   # sensor voxel (4, 20, 4), end voxel (7, 18, 4); the ray goes on to x = 23
        assert got[1][2][7, 18, 4] == 1 and got[1][1][23, :, 4].sum() > 0 and (lo[8:, :, 4] < 0).any()
    if case == "ceil_and_ground":   # (the reference scales the UNIT ray by pc / dz, prob_map.cpp:720, 726: not the plane's point; restated as it is)
        assert (lo > 0).sum() == 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. filters and batching
# ---------------------------------------------------------------------------------------------------------------------
def _cloud(n, seed, spread=1.6):
    r = np.random.default_rng(seed)
    xyz = np.stack([r.uniform(-spread, spread, n), r.uniform(-spread, spread, n), r.uniform(-0.2, 1.5, n)], axis=1)
    return _pts(xyz)


@pytest.mark.parametrize("backend", BACKENDS)
def test_point_filter_counts_only_points_that_passed_the_intensity_filter(backend):
    cl = _cloud(41, 3)
    cl[:, 3] = np.where(np.arange(41) % 2 == 0, 0.0, 10.0)   # threshold 5 drops every other point
    prm = _prm(point_filt_num=3, intensity_thresh=5)
    got = _check(backend, "filter", GRID, [(cl, SENSOR, prm)])
    passed = cl[cl[:, 3] >= 5]
    by_hand = _run_lib(backend, GRID, [(passed[::3], SENSOR, _prm())], slot=8)   # every third of the points that passed
    assert _same(got[0], by_hand[0])
    wrong = _run_lib(backend, GRID, [(cl[::3][cl[::3, 3] >= 5], SENSOR, _prm())], slot=8)   # every third point, then the filter
    assert not _same(got[0], wrong[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_batch_update_size_two(backend):
    prm = _prm(batch_update_size=2)
    got = _check(backend, "batch2", GRID, [(_cloud(50, 4), SENSOR, prm), (_cloud(50, 5), (0.3, -0.2, 0.4), prm), (_cloud(20, 6), SENSOR, prm)])
    assert got[0][4] == 0 and got[0][3] == 1 and (got[0][0] == 0).all() and got[0][1].sum() > 0 and got[0][2].sum() > 0   # counted, no belief yet
    assert got[1][4] == 1 and got[1][3] == 0 and (got[1][0] != 0).any() and got[1][1].sum() == 0 and got[1][2].sum() == 0   # one flush
    assert got[2][4] == 0 and got[2][3] == 1 and (got[2][0].view(np.int32) == got[1][0].view(np.int32)).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("thresh", [-10, 5], ids=["plain", "intensity"])
def test_cloud_sizes(backend, thresh):
    """0, 1, 63, 64, 65, 130 points (whole waves and tails) and 600 (the selection walks a cloud in tiles of 256), filter 1 and 4."""
    steps = []
    for i, n in enumerate([0, 1, 63, 64, 65, 130, 600]):
        cl = _cloud(n, 10 + i)
        cl[:, 3] = (np.arange(n) * 7 % 5) * 3.0
        steps.append((cl, SENSOR, _prm(point_filt_num=1 + 3 * (i % 2), intensity_thresh=thresh)))
    got = _check(backend, f"sizes{thresh}", GRID, steps)
    assert (got[0][0] == 0).all() and got[0][4] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. saturation
# ---------------------------------------------------------------------------------------------------------------------
def test_saturation_and_class_transitions():
    f32 = np.float32
    l_hit, l_miss, l_min, l_max, l_occ, l_free = [f32(np.log(np.float64(f32(x) / (f32(1) - f32(x))))) for x in (.9, .49, .12, .98, .85, .499)]
    prm = _prm()
    hit, cross = _pts([(0.55, 0.05, 0.55)]), _pts([(0.95, 0.05, 0.55)] * 30)
    steps = [(hit, SENSOR, prm)] * 3 + [(cross, SENSOR, prm)] * 7
    got = _check("emu", "saturation", GRID, steps)
    vals = [f32(0)] + [g[0][17, 12, 5] for g in got]
    assert vals[1] == l_hit and vals[2] == l_max and vals[3] == l_max and vals[-1] == l_min and vals[-2] == l_min
    cls = ["occupied" if v >= l_occ else ("free" if v < l_free else "unknown") for v in vals]
    assert [c for i, c in enumerate(cls) if i == 0 or c != cls[i - 1]] == ["unknown", "occupied", "unknown", "free"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. order independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_order_independence(backend):
    cl = _cloud(500, 21)
    perm = np.random.default_rng(22).permutation(500)
    prm = _prm()
    a = _check(backend, "order_a", GRID, [(cl, SENSOR, prm)] * 2)
    b = _check(backend, "order_b", GRID, [(cl[perm], SENSOR, prm), (cl[perm[::-1]], SENSOR, prm)])
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    ca, cb = _run_checker(*_CASES["order_a"]), _run_checker(*_CASES["order_b"])
    assert _same(ca[1], cb[1])   # the checker shows it too


# ---------------------------------------------------------------------------------------------------------------------
# 6. commit, 7. scan
# ---------------------------------------------------------------------------------------------------------------------
WORLD_SEED, TRUTH, BELIEF, PLAIN = 3, 2, 0, 5
POSES = np.array([[0.0, 0.0, 0.4, 0.3], [-0.6, 0.5, 0.8, 2.0], [0.7, -0.6, 0.2, -1.0]])


def _world(opt):
    prm = api.world_params(0, size_xy=2.4, size_z=1.6, lib=opt.L)
    assert (opt.generate_worlds(prm, [WORLD_SEED], first_map_id=TRUTH) != 0).all()
    o2, oc, o3 = opt.get_occupancy(TRUTH)
    nx, ny, nz = opt._map_dims[TRUTH]
    assert (nx, ny, nz) == (24, 24, 16) and 0 < o3.sum() < o3.size
    grid = dict(origin=(-1.2, -1.2, 0.0), res=0.1, dims=(24, 24, 16), min_b=(-1.2, -1.2, 0.0), max_b=(1.2, 1.2, 1.6))
    return grid, o3.reshape(24, 24, 16)


@functools.lru_cache(maxsize=None)
def _committed(backend):
    """Three scans of the tables world from three poses into the belief slot, committed.  Everything the commit tests compare."""
    opt = _opt(backend)
    grid, truth = _world(opt)
    opt.sense_reset([BELIEF], **grid)
    prm = opt.sense_params(point_filt_num=1, ray_range=[0.0, 2.0])
    clouds = []
    for pose in POSES:
        off, pts = opt.sense_scan([TRUTH], [pose], 64, 16, 1.2, 2.0)
        assert list(off) == [0, 1024]
        assert int(opt.sense_insert([BELIEF], api.SENSE_LAST_SCAN, [pose[:3]], prm, cloud_off=off)[0]) == 1
        clouds.append(pts[0].copy())
    opt.sense_commit([BELIEF])
    occ = opt.get_occupancy(BELIEF)
    e2, e3, _ = opt.get_map(BELIEF)
    inf, crit = opt.get_map_fields(BELIEF)
    states = np.zeros((200, 10))
    r = np.random.default_rng(5)
    states[:, 0], states[:, 1], states[:, 2] = r.uniform(-1.0, 1.0, 200), r.uniform(-1.0, 1.0, 200), r.uniform(-3, 3, 200)
    states[:, 3:] = r.uniform(-1.5, 1.5, (200, 7))
    col = opt.whole_body_collision(states, BELIEF)
    return dict(grid=grid, truth=truth, prm=prm, clouds=clouds, belief=opt.sense_get(BELIEF), occ=occ, fields=(e2, e3, inf, crit), states=states, col=col)


@pytest.mark.parametrize("backend", BACKENDS)
def test_commit(backend):
    R = _committed(backend)
    opt, grid = _opt(backend), R["grid"]
    if backend == "emu":   # the grids against the checker's derivation from the same clouds
        pm = wl.ProbMapCheck(grid["origin"], grid["res"], grid["dims"])
        for cl, pose in zip(R["clouds"], POSES):
            assert pm.update(cl, pose[:3], R["prm"]) == 1
        assert _same(pm.get(), R["belief"])
        want = pm.occupancy(R["prm"])
    else:
        E = _committed("emu")
        assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(R["clouds"], E["clouds"])) and _same(R["belief"], E["belief"])
        want = [np.asarray(g) for g in E["occ"]]
    o2, oc, o3 = [np.asarray(g) for g in R["occ"]]
    assert (o2.reshape(-1) == want[0].reshape(-1)).all() and (oc.reshape(-1) == want[1].reshape(-1)).all() and (o3.reshape(-1) == want[2].reshape(-1)).all()
    assert o3.sum() > 20 and oc.sum() >= o2.sum() > 0 and (o3.reshape(24, 24, 16) <= R["truth"]).all()   # sees part of the world, nothing else
    # the five fields: topay_build_esdf_fields with these grids, bit for bit
    opt.build_esdf_fields(grid["origin"], grid["res"], grid["dims"], grid["min_b"], grid["max_b"], o2, oc, o3, map_id=PLAIN)
    e2, e3, _ = opt.get_map(PLAIN)
    inf, crit = opt.get_map_fields(PLAIN)
    for got, ref in zip(R["fields"], (e2, e3, inf, crit)):
        assert (np.asarray(got).view(np.int64) == np.asarray(ref).view(np.int64)).all()
    assert (opt.whole_body_collision(R["states"], PLAIN) == R["col"]).all() and 0 < R["col"].sum() < len(R["col"])
    if backend == "gpu":
        assert (R["col"] == _committed("emu")["col"]).all()


def test_scan_against_the_checker():
    opt = _opt("emu")
    grid, truth = _world(opt)
    pose = np.array([0.05, -0.15, 0.45, 0.7])
    assert truth[12, 10, 4] == 0
    _, pts = opt.sense_scan([TRUTH], [pose], 64, 4, 1.0, 2.0)
    want = wl.pm_scan(truth, grid["origin"], grid["res"], grid["dims"], pose, 64, 4, 1.0, 2.0)
    assert (pts[0].view(np.int32) == want.view(np.int32)).all()
    # a short range: the rays without a hit sit at 1.5 range along the ray
    rng = 0.3
    _, near = opt.sense_scan([TRUTH], [pose], 64, 4, 1.0, rng)
    assert (near[0].view(np.int32) == wl.pm_scan(truth, grid["origin"], grid["res"], grid["dims"], pose, 64, 4, 1.0, rng).view(np.int32)).all()
    i, j = np.divmod(np.arange(256), 4)
    az, el = 2 * np.pi * i / 64 + pose[3], 1.0 * ((j + 0.5) / 4 - 0.5)
    far = pose[:3] + 1.5 * rng * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    dist = np.linalg.norm(near[0][:, :3] - pose[:3], axis=1)
    miss = dist > rng + 0.1
    assert miss.any() and np.abs(near[0][miss, :3] - far[miss]).max() < 1e-6 and (near[0][:, 3] == 0).all()
    # a pose inside an occupied voxel: every ray returns that voxel
    x, y, z = [int(v[0]) for v in np.nonzero(truth)]
    centre = np.array(grid["origin"]) + (np.array([x, y, z]) + 0.5) * grid["res"]
    _, own = opt.sense_scan([TRUTH], [list(centre + 0.01) + [0.0]], 64, 4, 1.0, 2.0)
    assert (own[0][:, :3] == centre.astype(np.float32)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    opt = _opt("emu")
    L, prm = opt.L, _prm()
    one = _pts([(0.5, 0.2, 0.6)])
    opt.sense_reset([20, 21], **GRID)
    ids = np.array([20, 20], dtype=np.int32)
    off = np.array([0, 1, 1], dtype=np.int32)
    sp = np.array([SENSOR, SENSOR], dtype=np.float64)
    args = (api._ip(off), one.ctypes.data, api._dp(sp), prm, None)
    assert L.topay_sense_insert(opt.h, 2, api._ip(ids), *args) == -1                          # a slot twice: TOPAY_ERR_INVALID_ARG
    ids[:] = [20, 22]
    assert L.topay_sense_insert(opt.h, 2, api._ip(ids), *args) == -3                          # before reset: TOPAY_ERR_NO_MAP
    assert L.topay_sense_commit(opt.h, 1, api._ip(np.array([22], dtype=np.int32))) == -3
    assert L.topay_sense_insert(opt.h, 1, api._ip(ids), api._ip(off), one.ctypes.data, api._dp(sp), _prm(ray_range=[0.3, 5.0]), None) == -6   # range_min > 0
    before = opt.sense_get(20)
    low = _prm(virtual_ceil_height=0.5, virtual_ground_height=0.1)
    st = opt.sense_insert([20, 21], [one, one], [(0.0, 0.0, 0.55), (0.0, 0.0, 0.3)], low)      # slot 20: the sensor is above the ceiling
    assert list(st) == [-1, 1] and _same(opt.sense_get(20), before) and (opt.sense_get(21)[0] != 0).any()
    assert int(opt.sense_insert([20], [one], [(0.0, 0.0, 0.05)], low)[0]) == -2 and _same(opt.sense_get(20), before)
    big = _pts(np.zeros((40000, 3)))                                                           # more rays than a 16-bit count holds
    with pytest.raises(api.TopayError, match="16-bit"):
        opt.sense_insert([20], [big], [SENSOR], prm)
    assert _same(opt.sense_get(20), before)



# ---------------------------------------------------------------------------------------------------------------------
# commit of several consecutive slots in one call (on the device: one batched field construction) against one call per slot
# ---------------------------------------------------------------------------------------------------------------------
GRID_ODD = dict(origin=(-1.15, -1.15, 0.0), res=0.1, dims=(23, 23, 12), min_b=(-1.15, -1.15, 0.0), max_b=(1.15, 1.15, 1.2))


def _slot_maps(opt, slots):
    return [opt.get_occupancy(m) + opt.get_map(m)[:2] + opt.get_map_fields(m) for m in slots]


@pytest.mark.parametrize("backend", BACKENDS)
def test_commit_of_consecutive_slots(backend):
    """23 x 23 x 12: neither grid of a run of 3 ends on a 16-byte boundary.

    What this compares is one backend with itself: one commit of three slots against three commits of one.  On the device the first
    goes through the field construction as ONE batch of three maps; under the emulator topay_sense_commit hands a run over slot by
    slot, so there both sides take the same path.  The independent check of that batched construction is in tests/test_edt_exact.py
    (test_sense_commit_of_consecutive_slots_against_the_definition): the same three slots, every field against the brute-force
    definition computed from the slot's own occupancy grids, on the device as well."""
    opt, slots = _opt(backend), [10, 11, 12]
    opt.sense_reset(slots, **GRID_ODD)
    clouds = [_cloud(300, 40 + k, spread=1.1) for k in range(3)]
    assert (opt.sense_insert(slots, clouds, [SENSOR, (0.4, -0.3, 0.4), (-0.5, 0.5, 0.8)], _prm()) == 1).all()
    opt.sense_commit(slots)
    together = _slot_maps(opt, slots)
    alone = []
    for m in slots:
        opt.sense_commit([m])
        alone += _slot_maps(opt, [m])
    for a, b in zip(together, alone):
        assert a[2].sum() > 5
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and (np.asarray(x).view(np.int8) == np.asarray(y).view(np.int8)).all()
    assert not (together[0][2] == together[1][2]).all()
    with pytest.raises(api.TopayError):     # the grids of an earlier commit are gone: only the last commit's are served
        opt.get_occupancy(10)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: two robots, the map changes under a committed trajectory
# ---------------------------------------------------------------------------------------------------------------------
# Chosen on the CPU (emulator) beforehand, as the loop `for seed in range(50)` at the full first range of 5 m: seed 0 is the first
# world in which the second scan flips a robot (robot 0) from safe to unsafe; the range did not have to be shrunk.
E2E_SEED, E2E_RANGE1, E2E_SIZE = 0, 5.0, 10.0
# second scan: robot 0 from the state of its committed trajectory 1 s before that trajectory first violates the TRUTH map (an
# obstacle the first scan could not see: the belief's sweep was safe); robot 1, whose trajectory is safe in the truth, from its start
E2E_POSES2 = np.array([[-0.5827918833456173, 1.428973817528711, 0.5, -4.086212862315743],
                       [-2.0412398197772355, 2.9528712577789724, 0.5, -2.892973131781924]])


@functools.lru_cache(maxsize=None)
def _episode(backend):
    lib = EMU_LIB if backend == "emu" else None
    p = api.default_params(api.load(lib))
    p.s1_lbfgs.max_iterations = 40
    p.s2_lbfgs.max_iterations = 40
    p.alm_max_outer = 2
    opt = api.MomaTrajOptBatch(params=p, device=0, lib_path=lib)
    prm = api.world_params(0, size_xy=E2E_SIZE, lib=opt.L)
    start, goal, st, _ = opt.generate_episodes(prm, [E2E_SEED], first_map_id=2)      # 1. the truth world in slot 2
    assert st[0] == 1
    S, G = np.array([start[0], goal[0]]), np.array([goal[0], start[0]])             # two robots, opposite ways
    org = np.array([-E2E_SIZE / 2, -E2E_SIZE / 2, 0.0])
    opt.sense_reset([0, 1], origin=org, res=0.1, dims=(100, 100, 16), min_b=org, max_b=org + np.array([10.0, 10.0, 1.6]))
    poses = np.array([[s_[0], s_[1], 0.5, s_[2]] for s_ in S])
    off, _ = opt.sense_scan([2, 2], poses, 64, 16, 1.0, E2E_RANGE1, copy_back=False)  # 2. scan, insert, commit from the start poses
    sp = opt.sense_params(point_filt_num=1, ray_range=[0.0, E2E_RANGE1])
    assert (opt.sense_insert([0, 1], api.SENSE_LAST_SCAN, poses[:, :3], sp, cloud_off=off) == 1).all()
    opt.sense_commit([0, 1])
    res, _, _ = opt.plan_calls(S, G, map_ids=[0, 1])                                 # 3. plan on the beliefs
    done = opt.track_commit_plan([0, 1], [0, 1])                                     # 4. commit the winners
    safe1 = opt.track_safe([0, 1], [0, 1])
    truth = opt.track_safe([0, 1], [2, 2])
    off, _ = opt.sense_scan([2, 2], E2E_POSES2, 64, 16, 1.0, 5.0, copy_back=False)    # 5., 6. second scan, insert, commit
    assert (opt.sense_insert([0, 1], api.SENSE_LAST_SCAN, E2E_POSES2[:, :3], opt.sense_params(point_filt_num=1), cloud_off=off) == 1).all()
    opt.sense_commit([0, 1])
    safe2 = opt.track_safe([0, 1], [0, 1])                                           # 7.
    return dict(res=res, done=done, safe1=safe1, truth=truth, safe2=safe2, occ=int(opt.get_occupancy(0)[2].sum()))


def test_episode_second_scan_makes_a_committed_trajectory_unsafe():
    E = _episode("emu")
    assert E["done"].all() and E["safe1"][0].all()
    assert list(E["truth"][0]) == [False, True]                 # robot 0's trajectory runs into something its first scan did not show
    assert list(E["safe2"][0]) == [False, True]                 # ... and the second scan shows it: safe -> unsafe
    assert E["safe2"][1][0, 0] >= 0 and np.isfinite(E["safe2"][2][0]).all()


@pytest.mark.gpu
def test_episode_on_the_device_matches_the_emulator():
    E, D = _episode("emu"), _episode("gpu")
    assert (D["res"][:, :7] == E["res"][:, :7]).all() and (D["done"] == E["done"]).all() and D["occ"] == E["occ"]
    for key in ("safe1", "truth", "safe2"):
        for d, e in zip(D[key], E[key]):
            # (every value equal; "NaN when safe" is any NaN: its sign and payload are not part of the result)
            assert d.shape == e.shape and d.dtype == e.dtype and np.array_equal(d, e, equal_nan=d.dtype == np.float64), (key, d, e)
    assert list(D["safe1"][0]) == [True, True] and list(D["safe2"][0]) == [False, True]
