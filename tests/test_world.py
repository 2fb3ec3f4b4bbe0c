"""Benchmark episodes on the device (topay_amd/csrc/topay_world.h): the mt19937_64 stream, the world generators, the
rasteriser's occupancy grids, the fields built from them, the scenario samplers and whole episodes, each against the CPU
harness (harness/workload.hpp) with equal seeds.  Everything is compared bit for bit; a sampler instance may differ only at a
tie of a collision threshold (the rule of tests/test_collision.py), at most one per test.

Every case runs twice: through the CPU lane emulator of the kernel sources and, marked gpu, on the device.  Cases that need
the fields of several maps build them one call per map on the emulator and in one call on the device (they were written when
the emulator ran the blocks of a launch along x only; the batched construction, blockIdx.y = map, is checked on both in
tests/test_edt_exact.py).

Shapes: the default 20 x 20 x 1.6 m map where the issue names it, otherwise 10 x 10 m (100 x 100 cells, the obstacle counts
scaled as World::build scales them) -- the smallest map on which a start and a goal 3 m apart fit.
"""
import functools
import os

import numpy as np
import pytest

from conftest import EMU_LIB
from harness import workload as wl
from topay_amd import api

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
MASK = 0xFFFFFFFFFFFFFFFF


def _opt(backend):
    return api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB if backend == "emu" else None)


@functools.lru_cache(maxsize=None)
def _world(kind, seed, size_xy=20.0, size_z=1.6, res=0.1, cloud_res=0.05, keepouts=None, fields=False):
    """The harness's world (occupancy only unless fields), built once per test session."""
    ko = None if keepouts is None else np.array(keepouts).reshape(-1, 2)
    return wl.World(kind, seed=seed & MASK, size_xy=size_xy, size_z=size_z, res=res, cloud_res=cloud_res, keepouts=ko, nthreads=4 if fields else -1)


def _prm(opt, kind, **kw):
    return api.world_params(kind, lib=opt.L, **kw)


def _harness_of(prm, kind, seed, keepouts=None, fields=False):
    ko = None if keepouts is None else tuple(float(v) for v in np.asarray(keepouts).reshape(-1))
    return _world(kind, int(seed), prm.size_xy, prm.size_z, prm.resolution, prm.cloud_resolution, ko, fields)


def _check_occupancy(opt, prm, kind, seeds, keepouts=None):
    st = opt.generate_worlds(prm, seeds, keepouts)
    assert (st == 1).all()
    for i, sd in enumerate(seeds):
        w = _harness_of(prm, kind, sd, None if keepouts is None else keepouts[i])
        o2, oc, o3 = opt.get_occupancy(i)
        assert tuple(opt._map_dims[i]) == tuple(int(v) for v in w.dims)
        assert (o2 == w.occ2d).all() and (o3 == w.occ3d).all(), (kind, sd, int((o2 != w.occ2d).sum()), int((o3 != w.occ3d).sum()))
        assert o3.sum() > 1000 and o2.sum() > 100
        if prm.size_z >= 1.5:   # walls and cuboids are at most 1.5 m high: the cloud stays inside the map's height
            assert (oc == o3.reshape(len(oc), -1).max(axis=1)).all()
    return st


KEEP3 = np.array([[[1.0, 2.0], [-3.0, 4.0]], [[-6.5, 0.25], [0.0, 0.0]], [[5.0, 5.0], [7.0, 1.0]]])


# ---------------------------------------------------------------------------------------------------------------------
# generator stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_mt64_stream(backend):
    """The C++ library's stream: the 10000th output of mt19937_64(5489), and the first 1000 outputs of three seeds (one with the
    top bit set; 1000 outputs cross three twists) against tests/golden/mt64_stream.npz, which make_mt64_stream.py beside it
    writes from std::mt19937_64 -- all 64 bits equal.  A window that starts inside the stream (skip > 0) against the same values."""
    L = _opt(backend).L
    assert int(api.test_mt64(5489, 9999, 1, lib=L)[0]) == 9981545732273789042
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt64_stream.npz"))
    seeds, want = [int(v) for v in ref["seeds"]], ref["out"]
    assert seeds == [1, 42, 2 ** 63 + 12345] and want.shape == (3, 1000) and want.dtype == np.uint64
    for k, seed in enumerate(seeds):
        out = api.test_mt64(seed, 0, 1000, lib=L)
        assert out.dtype == np.uint64 and (out == want[k]).all(), (seed, int(np.argmax(out != want[k])))
    assert (api.test_mt64(seeds[2], 300, 400, lib=L) == want[2, 300:700]).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_start_goal_xy_bit_identical(backend):
    L = _opt(backend).L
    seeds = [s * 1000 + a for s in range(40, 72) for a in (0, 1)] + [MASK, 2 ** 63]
    for size in (20.0, 10.0):
        s3, g3 = api.sample_start_goal_xy(seeds, size, lib=L)
        for i, sd in enumerate(seeds):
            hs, hg = wl.sample_start_goal_xy(sd, size)
            assert (s3[i] == hs).all() and (g3[i] == hg).all(), (sd, size)


# ---------------------------------------------------------------------------------------------------------------------
# occupancy, byte for byte
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", [wl.TABLES, wl.CUBOIDS])
def test_occupancy_default_map(backend, kind):
    """a. The default 20 x 20 x 1.6 m map: three seeds in one call (tables with keep-outs), then n = 1."""
    opt = _opt(backend)
    prm = _prm(opt, kind)
    assert list(prm.obs_num) == ([40, 80] if kind == wl.TABLES else [80, 80])
    ko = KEEP3 if kind == wl.TABLES else None
    _check_occupancy(opt, prm, kind, [101, 102, 103], ko)
    assert opt.world_last_path() == 1
    _check_occupancy(opt, prm, kind, [104], None if ko is None else ko[:1])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind,case", [(k, c) for k in (wl.TABLES, wl.CUBOIDS) for c in ("b_small", "c_cloud_eq_cell", "d_cloud_003")])
def test_occupancy_cases(backend, kind, case):
    """b. 100 x 100 cells with the scaled obstacle counts; c. cloud resolution = cell size (points on cell boundaries: the float
    roundings decide); d. a cloud resolution that does not divide the cell."""
    opt = _opt(backend)
    kw = dict(b_small=dict(size_xy=10.0), c_cloud_eq_cell=dict(size_xy=10.0, cloud_resolution=0.1), d_cloud_003=dict(size_xy=10.0, cloud_resolution=0.03))[case]
    prm = _prm(opt, kind, **kw)
    assert list(prm.obs_num) == ([10, 20] if kind == wl.TABLES else [20, 20])
    ko = KEEP3[:2] * 0.4 if kind == wl.TABLES else None
    _check_occupancy(opt, prm, kind, [7, 8], ko)
    assert opt.world_last_path() == 1


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", [wl.TABLES, wl.CUBOIDS])
def test_occupancy_second_path(backend, kind):
    """e. 66 layers (res 0.05, size_z 3.3) cannot take the masks in LDS: the byte-store path runs, and it gives the same bytes.
    The same path forced on a map that takes the first one by the rule: identical grids from both."""
    opt = _opt(backend)
    prm = _prm(opt, kind, size_xy=6.0, resolution=0.05, size_z=3.3)
    _check_occupancy(opt, prm, kind, [7, 8], KEEP3[:2] * 0.2 if kind == wl.TABLES else None)
    assert opt.world_last_path() == 2
    prm = _prm(opt, kind, size_xy=10.0)
    opt.generate_worlds(prm, [21, 22])
    assert opt.world_last_path() == 1
    first = [opt.get_occupancy(i) for i in range(2)]
    opt.world_test_path(2)
    opt.generate_worlds(prm, [21, 22])
    assert opt.world_last_path() == 2
    for i in range(2):
        for a, b in zip(first[i], opt.get_occupancy(i)):
            assert (a == b).all()
    opt.world_test_path(0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_occupancy_keepout_at_edge_and_32_layers(backend):
    """f. Keep-outs at the map's edge and corner (desks beside them hang over the boundary: their points are clipped), and a map
    of 32 layers (size_z 3.2: the 32-bit masks of the first path)."""
    opt = _opt(backend)
    prm = _prm(opt, wl.TABLES, size_xy=10.0)
    _check_occupancy(opt, prm, wl.TABLES, [31, 32], np.array([[[4.9, 0.0], [-5.0, -5.0]], [[0.0, 5.2], [4.6, 4.6]]]))
    for kind in (wl.TABLES, wl.CUBOIDS):
        prm = _prm(opt, kind, size_xy=10.0, size_z=3.2)
        _check_occupancy(opt, prm, kind, [33])
        assert opt.world_last_path() == 1 and opt._map_dims[0][2] == 32


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", [wl.TABLES, wl.CUBOIDS])
def test_critical_grid(backend, kind):
    """occ2d_critical marks a column whatever the height of the point: the projection of occ3d while the cloud stays inside the
    map's height; with size_z = 1.0 (walls of up to 1.5 m rise above it) the projection of the occ3d of the same seed at
    size_z = 3.2 -- the height does not enter the generator."""
    opt = _opt(backend)
    # the default 20 x 20 x 1.6 m worlds (the seeds of test_occupancy_default_map: the harness's worlds are shared)
    _check_occupancy(opt, _prm(opt, kind), kind, [101, 102], KEEP3[:2] if kind == wl.TABLES else None)
    # size_z = 1.0: occ2d and occ3d against the harness, the critical grid against the 32-layer map of the same seed
    _check_occupancy(opt, _prm(opt, kind, size_xy=10.0, size_z=1.0), kind, [51])
    _, oc_low, o3_low = opt.get_occupancy(0)
    _check_occupancy(opt, _prm(opt, kind, size_xy=10.0, size_z=3.2), kind, [51])
    _, _, o3_high = opt.get_occupancy(0)
    proj = o3_high.reshape(len(oc_low), -1).max(axis=1)
    assert (oc_low == proj).all()
    assert (proj >= o3_low.reshape(len(oc_low), -1).max(axis=1)).all()


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
def _generate(opt, backend, prm, seeds, keepouts=None, first=0):
    """Worlds with their fields: one call on the device, one call per map on the emulator (see the module's docstring)."""
    if backend == "gpu":
        return opt.generate_worlds(prm, seeds, keepouts, first_map_id=first)
    return np.concatenate([opt.generate_worlds(prm, [sd], None if keepouts is None else keepouts[i:i + 1], first_map_id=first + i) for i, sd in enumerate(seeds)])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", [wl.TABLES, wl.CUBOIDS])
def test_fields_equal_upload_path(backend, kind):
    """The five fields after topay_generate_worlds == topay_build_esdf_fields fed the harness's occupancy, two maps per kind."""
    opt, ref = _opt(backend), _opt(backend)
    prm = _prm(opt, kind, size_xy=10.0)
    seeds, ko = [61, 62], (KEEP3[:2] * 0.4 if kind == wl.TABLES else None)
    _generate(opt, backend, prm, seeds, ko)
    for i, sd in enumerate(seeds):
        w = _harness_of(prm, kind, sd, None if ko is None else ko[i])
        ref.build_esdf_fields(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, None, w.occ3d, map_id=0)
        e2, e3, _ = opt.get_map(i)
        r2, r3, _ = ref.get_map(0)
        inf, cr = opt.get_map_fields(i)
        rinf, rcr = ref.get_map_fields(0)
        assert (e2 == r2).all() and (e3 == r3).all() and (inf == rinf).all() and (cr == rcr).all()
        assert np.isfinite(e3).all() and e2.min() < 0 < e2.max()


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_SEEDS = list(range(500, 564))


def _two_maps(opt, backend):
    """Slot 0: a tables world, slot 1: a cuboids world, 10 x 10 m; the harness's twins with their CPU fields."""
    pt, pc = _prm(opt, wl.TABLES, size_xy=10.0), _prm(opt, wl.CUBOIDS, size_xy=10.0)
    opt.generate_worlds(pt, [71], first_map_id=0)
    opt.generate_worlds(pc, [72], first_map_id=1)
    return [_harness_of(pt, wl.TABLES, 71, fields=True), _harness_of(pc, wl.CUBOIDS, 72, fields=True)]


def _excuse(w, dev_states, ref_states):
    """The tie rule: the harness says a state the device accepted collides -> that state is within 1e-12 of a threshold;
    otherwise the harness accepted its own state earlier than the device did -> the harness's state is."""
    for st in dev_states:
        if w.collision(st):
            assert w.collision_tie_slack(st) < 1e-12
            return
    assert min(w.collision_tie_slack(st) for st in ref_states) < 1e-12


@pytest.mark.parametrize("backend", BACKENDS)
def test_sample_arm(backend):
    opt = _opt(backend)
    worlds = _two_maps(opt, backend)
    s3, _ = api.sample_start_goal_xy(SAMPLER_SEEDS, 10.0, lib=opt.L)
    excused = 0
    for m, w in enumerate(worlds):
        st0 = np.zeros((len(SAMPLER_SEEDS), 10))
        st0[:, :3] = s3
        st, ok, tries = opt.sample_arm(st0, [sd * 7919 + m for sd in SAMPLER_SEEDS], map_ids=[m] * len(SAMPLER_SEEDS))
        assert ok.any() and (tries[ok] >= 1).all() and (tries[~ok] == 2000).all()
        for i, sd in enumerate(SAMPLER_SEEDS):
            hok, hst = w.sample_arm(sd * 7919 + m, st0[i])
            if hok == ok[i] and (hst == st[i]).all():
                continue
            excused += 1
            _excuse(w, [st[i]] if ok[i] else [], [hst])
    assert excused <= 1
    # one try on a state deep inside an obstacle
    w = worlds[0]
    cell = int(np.argmin(w.esdf2d))
    ny = int(w.dims[1])
    deep = np.zeros((1, 10))
    deep[0, 0] = (cell // ny + 0.5) * w.res + w.origin[0]
    deep[0, 1] = (cell % ny + 0.5) * w.res + w.origin[1]
    assert w.esdf2d[cell] < -0.05
    st, ok, tries = opt.sample_arm(deep, [9], map_ids=[0], max_tries=1)
    assert not ok[0] and tries[0] == 1 and w.collision(st[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_sample_scenarios(backend):
    opt = _opt(backend)
    worlds = _two_maps(opt, backend)
    excused = 0
    for m, w in enumerate(worlds):
        s, g, ok = opt.sample_scenarios(SAMPLER_SEEDS, map_ids=[m] * len(SAMPLER_SEEDS))
        assert ok.all()
        for i, sd in enumerate(SAMPLER_SEEDS):
            hok, hs, hg = w.sample_scenario(sd)
            if hok == ok[i] and (hs == s[i]).all() and (hg == g[i]).all():
                continue
            excused += 1
            _excuse(w, [g[i], s[i]], [hg, hs])
    assert excused <= 1


# ---------------------------------------------------------------------------------------------------------------------
# episodes
# ---------------------------------------------------------------------------------------------------------------------
def _harness_episode(prm, kind, seed, attempt):
    """The flow of wl_tables_batch_create / wl.tables_scenario (without init paths), and the cuboids flow, from harness primitives."""
    if kind == wl.CUBOIDS:
        w = _harness_of(prm, kind, seed, fields=True)
        ok, s, g = w.sample_scenario(seed)
        return w, int(ok), s, g
    sd = (seed * 1000 + attempt) & MASK
    s3, g3 = wl.sample_start_goal_xy(sd, prm.size_xy)
    w = _harness_of(prm, kind, sd, [s3[:2], g3[:2]], fields=True)
    start, goal = np.zeros(10), np.zeros(10)
    start[:3], goal[:3] = s3, g3
    ok1, goal = w.sample_arm((seed * 7919 + 2 * attempt) & MASK, goal)
    ok2, start = w.sample_arm((seed * 7919 + 2 * attempt + 1) & MASK, start)
    return w, int(ok1 and ok2), start, goal


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind,seeds", [(wl.TABLES, [42, 43, 44, 45, 46, 47, 48, 49]), (wl.CUBOIDS, [42, 43, 44, 45])])
def test_episodes(backend, kind, seeds):
    opt = _opt(backend)
    prm = _prm(opt, kind, size_xy=10.0)
    attempts = [0, 1, 0, 2, 0, 0, 3, 0][:len(seeds)]
    chunks = [list(range(len(seeds)))] if backend == "gpu" else [[i] for i in range(len(seeds))]
    excused = 0
    for ch in chunks:
        s, g, st, att = opt.generate_episodes(prm, [seeds[i] for i in ch], first_map_id=ch[0], attempts=[attempts[i] for i in ch])
        assert (att == [attempts[i] for i in ch]).all()
        for k, i in enumerate(ch):
            w, hst, hs, hg = _harness_episode(prm, kind, seeds[i], attempts[i])
            o2, oc, o3 = opt.get_occupancy(i)
            assert (o2 == w.occ2d).all() and (o3 == w.occ3d).all()
            if kind == wl.TABLES:
                assert (s[k, :3] == hs[:3]).all() and (g[k, :3] == hg[:3]).all()
            if st[k] == hst and (st[k] == 0 or ((s[k] == hs).all() and (g[k] == hg).all())):
                continue
            excused += 1
            _excuse(w, [g[k], s[k]] if st[k] else [], [hg, hs])
    assert excused <= 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_episode_retry_helper(backend):
    """generate_episodes(max_attempts): with one try per arm most first attempts fail; the helper repeats the episode with
    attempt + 1 on its slot, and the attempt that succeeds is the harness's episode of that attempt (its arms accepted at
    the first try there too)."""
    opt = _opt(backend)
    prm = _prm(opt, wl.TABLES, size_xy=10.0)
    opt.world_test_max_tries(1)
    retried = 0
    for seed in (42, 43):
        _, _, st1, att1 = opt.generate_episodes(prm, [seed], max_attempts=1)
        s, g, st, att = opt.generate_episodes(prm, [seed], max_attempts=12)
        assert att1[0] == 0 and (st1[0] == 1) == (att[0] == 0)
        assert st[0] == 1, "no attempt of 12 accepted both arms at the first try"
        retried += int(att[0] > 0)
        w, hst, hs, hg = _harness_episode(prm, wl.TABLES, seed, int(att[0]))
        assert hst == 1 and (hs == s[0]).all() and (hg == g[0]).all()
        o2, _, o3 = opt.get_occupancy(0)
        assert (o2 == w.occ2d).all() and (o3 == w.occ3d).all()
    assert retried >= 1
    opt.world_test_max_tries(0)


# ---------------------------------------------------------------------------------------------------------------------
# hand-over to the planning call (device only)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plan_calls_on_generated_episodes():
    """topay_plan_calls on two episodes generated on the device == on the same episodes with the maps uploaded from the harness."""
    dev, ref = _opt("gpu"), _opt("gpu")
    prm = _prm(dev, wl.TABLES)
    s, g, st, att = dev.generate_episodes(prm, [42, 43], max_attempts=8)
    assert (st == 1).all()
    for i in range(2):
        w, hst, hs, hg = _harness_episode(prm, wl.TABLES, [42, 43][i], int(att[i]))
        ref.build_esdf_fields(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, None, w.occ3d, map_id=i)
    out_d = dev.plan_calls(s, g, map_ids=[0, 1])
    out_r = ref.plan_calls(s, g, map_ids=[0, 1])
    assert (out_d[0] == out_r[0]).all() and (out_d[1] == out_r[1]).all()
    assert (out_d[0][:, 0] == 1).any(), "no planning call found a trajectory: nothing would be compared below"
    td, tr = dev.plan_trajs([0, 1]), ref.plan_trajs([0, 1])
    for k in ("piece_off", "durations", "coeffs", "knots_xy"):
        assert td[k].shape == tr[k].shape and (td[k] == tr[k]).all(), k


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_world_errors(backend):
    import ctypes as C

    opt = _opt(backend)
    L, prm = opt.L, _prm(opt, wl.CUBOIDS, size_xy=10.0)
    sd = np.array([1, 2], dtype=np.uint64)
    sp = sd.ctypes.data_as(api.c_u64p)
    INVALID, NO_MAP = -1, -3
    assert L.topay_generate_worlds(opt.h, 0, 0, C.byref(prm), sp, None, None) == INVALID
    assert L.topay_generate_worlds(opt.h, -1, 0, C.byref(prm), sp, None, None) == INVALID
    assert L.topay_generate_worlds(opt.h, 2, 4095, C.byref(prm), sp, None, None) == INVALID
    bad = _prm(opt, wl.CUBOIDS, size_xy=10.0)
    bad.kind = 2
    assert L.topay_generate_worlds(opt.h, 1, 0, C.byref(bad), sp, None, None) == INVALID
    many = _prm(opt, wl.CUBOIDS, size_xy=10.0, obs_num=[2000, 47])     # 2047 + 2 keep-outs > the pool of 2048
    assert L.topay_generate_worlds(opt.h, 1, 0, C.byref(many), sp, None, None) == INVALID
    p = api.WorldParams()
    assert L.topay_world_default_params(2, C.byref(p)) == INVALID
    s10, st = np.zeros((2, 10)), np.zeros(2, dtype=np.int32)
    assert L.topay_generate_episodes(opt.h, 0, 0, C.byref(prm), sp, None, api._dp(s10), api._dp(s10), api._ip(st)) == INVALID
    tiny = _prm(opt, wl.CUBOIDS, size_xy=6.0)                          # no start / goal pair 3 m apart fits
    assert L.topay_generate_episodes(opt.h, 1, 0, C.byref(tiny), sp, None, api._dp(s10), api._dp(s10), api._ip(st)) == INVALID
    assert L.topay_sample_arm(opt.h, 1, None, sp, 0, api._dp(s10), api._ip(st), None) == NO_MAP
    o2 = np.zeros(100 * 100, dtype=np.int8)
    assert L.topay_get_occupancy(opt.h, 0, o2.ctypes.data_as(api.c_i8p), None, None) == NO_MAP
    opt.generate_worlds(prm, [5], first_map_id=3)
    assert L.topay_get_occupancy(opt.h, 3, o2.ctypes.data_as(api.c_i8p), None, None) == 0 and o2.sum() > 0
    assert L.topay_get_occupancy(opt.h, 3, None, None, None) == 0
    assert L.topay_get_occupancy(opt.h, 2, o2.ctypes.data_as(api.c_i8p), None, None) == NO_MAP
    assert L.topay_get_occupancy(opt.h, 4, o2.ctypes.data_as(api.c_i8p), None, None) == NO_MAP
    # a slot refilled through the upload entry no longer has generated grids
    w = _harness_of(prm, wl.CUBOIDS, 5)
    opt.build_esdf_fields(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, None, w.occ3d, map_id=3)
    assert L.topay_get_occupancy(opt.h, 3, o2.ctypes.data_as(api.c_i8p), None, None) == NO_MAP
