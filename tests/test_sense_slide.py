"""Sliding sensor map (include/topay.h topay_sense_slide, topay_amd/csrc/topay_sense.h k_sense_slide): a slot's belief re-centred on
the sensor, what leaves the window forgotten, what stays kept (rog_map's SlidingMap::mapSliding and the two triggers of
ProbMap::updateProbMap).

Without a device the CPU lane emulator of the kernel sources is compared with the sequential checker (harness/prob_map.hpp, which
slides as the reference does: it clears the slabs that leave and re-addresses a ring, no voxel moves); marked gpu, the device is
compared with the emulator.  Everything is compared bit for bit: log-odds, both count arrays, the batch counter, status, shift and
the descriptor's origin and bounds as doubles (the checker keeps an origin only: its bounds are the reset's plus shift x resolution).

Grid: 24 x 24 x 12 voxels of 0.125 m, origin (-1.5, -1.5, 0), where every boundary and every slid origin is a binary fraction and
therefore exact; 24 x 24 x 10 where a column is no multiple of four floats.  The commit and the roaming cases use 0.1 m tables worlds
with 16 layers.  The centre voxel is (12, 12, nz / 2): its low corner, from which the trigger measures, is (0, 0) in x and y.
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
GRID8 = dict(origin=(-1.5, -1.5, 0.0), res=0.125, dims=(24, 24, 12), min_b=(-1.5, -1.5, 0.0), max_b=(1.5, 1.5, 1.5))
GRID8_Z10 = dict(origin=(-1.5, -1.5, 0.0), res=0.125, dims=(24, 24, 10), min_b=(-1.5, -1.5, 0.0), max_b=(1.5, 1.5, 1.25))
NEW_ENTRIES = ["topay_sense_slide_default_params", "topay_sense_slide", "topay_sense_slide_ms"]


@functools.lru_cache(maxsize=None)
def _opt(backend):
    return api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB if backend == "emu" else None)


def _pts(xyz, intensity=0.0):
    a = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([a, np.full((len(a), 1), intensity, dtype=np.float32)], axis=1)


def _prm(**kw):
    kw.setdefault("point_filt_num", 1)
    return _opt("emu").sense_params(**kw)


def _sp(**kw):
    return _opt("emu").sense_slide_params(**kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    """Two states (log-odds, op_cnt, hit_cnt, batch counter, status, shift, descriptor): every bit."""
    return (all(x.dtype == y.dtype and x.shape == y.shape and (_bits(x) == _bits(y)).all() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
            and a[4] == b[4] and tuple(a[5]) == tuple(b[5]) and (_bits(a[6]) == _bits(b[6])).all())


def _apply(opt, slot, step):
    """One step on a slot: ("ins", cloud, sensor, params) or ("sl", sensor, slide params).  (status, shift)."""
    if step[0] == "ins":
        return int(opt.sense_insert([slot], [step[1]], [step[2]], step[3])[0]), (0, 0, 0)
    st, sh = opt.sense_slide([slot], [step[1]], step[2])
    return int(st[0]), tuple(int(v) for v in sh[0])


def _run_lib(backend, grid, steps, slot=7):
    """The state after every step: log-odds, op_cnt, hit_cnt, batch counter, status, shift, (origin, min, max) as nine doubles."""
    opt = _opt(backend)
    opt.sense_reset([slot], **grid)
    out = []
    for step in steps:
        st, sh = _apply(opt, slot, step)
        out.append(opt.sense_get(slot) + (st, sh, np.concatenate(opt.sense_desc(slot))))
    return out


def _run_checker(grid, steps):
    pm = wl.ProbMapCheck(grid["origin"], grid["res"], grid["dims"])
    mn, mx = np.array(grid["min_b"], dtype=np.float64), np.array(grid["max_b"], dtype=np.float64)
    out = []
    for step in steps:
        if step[0] == "ins":
            st, sh = pm.update(step[1], step[2], step[3]), (0, 0, 0)
        else:
            st, shift = pm.slide(step[1], step[2])
            sh = tuple(int(v) for v in shift)
            by = shift.astype(np.float64) * np.float64(grid["res"])   # the descriptor's rule: one multiply, one add per axis
            mn, mx = mn + by, mx + by
        out.append(pm.get() + (st, sh, np.concatenate([pm.origin, mn, mx])))
    return out


_CASES = {}


@functools.lru_cache(maxsize=None)
def _emu_cached(key):
    return _run_lib("emu", *_CASES[key])


def _check(backend, key, grid, steps):
    """emu: the emulator against the checker; gpu: the device against the emulator.  Returns the backend's states."""
    _CASES[key] = (grid, steps)
    want = _run_checker(grid, steps) if backend == "emu" else _emu_cached(key)
    got = _emu_cached(key) if backend == "emu" else _run_lib("gpu", grid, steps)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (key, i, g[3:], w[3:], [int((_bits(x) != _bits(y)).sum()) for x, y in zip(g[:3], w[:3])])
    return got


def _np_shift(lo, s):
    """new[l] = old[l + s] where l + s is a voxel of the grid, else 0."""
    out = np.zeros_like(lo)
    dst, src = [], []
    for n, k in zip(lo.shape, s):
        a, b = max(0, -k), min(n, n - k)
        if a >= b:
            return out
        dst.append(slice(a, b))
        src.append(slice(a + k, b + k))
    out[tuple(dst)] = lo[tuple(src)]
    return out


def _sensor_at(grid, shift, z=0.5625, slide_z=False):
    """The centre of the voxel that lies `shift` voxels from the grid's centre voxel (in z only when z slides)."""
    o, r, d = np.array(grid["origin"]), grid["res"], np.array(grid["dims"])
    p = o + (d // 2 + np.array(shift) + 0.5) * r
    if not slide_z:
        p[2] = z
    return tuple(float(v) for v in p)


def _cloud(n, seed, spread=1.6):
    r = np.random.default_rng(seed)
    xyz = np.stack([r.uniform(-spread, spread, n), r.uniform(-spread, spread, n), r.uniform(-0.2, 1.5, n)], axis=1)
    return _pts(xyz)


def _structured():
    """Three inserts from three sensors: occupied, free and unknown voxels; a voxel hit twice in one batch is at l_max, and the
    sensors' own voxels, which every ray of an insert leaves through, at l_min."""
    prm = _prm()
    twice = _pts([(0.7, 0.4, 0.6), (0.7, 0.4, 0.6), (-0.9, -0.8, 0.3), (-0.9, -0.8, 0.3)])
    return [("ins", np.concatenate([_cloud(150, 31), twice]), (0.05, 0.05, 0.55), prm), ("ins", _cloud(150, 32), (0.4, -0.3, 0.4), prm),
            ("ins", np.concatenate([_cloud(150, 33), twice]), (-0.5, 0.5, 0.8), prm)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. symbols and defaults
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_default_parameters():
    import __graft_entry__ as entry
    entry.build_hip()
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    declared = set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M))
    hip, em = api.load(), api.load(EMU_LIB)
    for n in NEW_ENTRIES + ["topay_sense_get_desc"]:
        assert n in declared, n
        assert hasattr(hip, n), f"{n} not exported by the HIP library"
        assert hasattr(em, n), f"{n} not exported by the emulator library"
    for n in ("sense_slide_params", "sense_slide", "sense_slide_ms", "sense_desc"):
        assert hasattr(api.MomaTrajOptBatch, n), n
    p = _opt("emu").sense_slide_params()
    assert p.threshold == 0.3 and p.slide_z == 0 and p.reserved == 0
    assert hasattr(wl.ProbMapCheck, "slide")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the shift table
# ---------------------------------------------------------------------------------------------------------------------
SHIFTS = [((1, 0, 0), 0), ((-1, 0, 0), 0), ((0, 23, 0), 0), ((0, -23, 0), 0), ((3, -5, 0), 0), ((24, 0, 0), 0), ((0, -30, 0), 0),
          ((0, 0, 2), 1), ((1, 1, -3), 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("grid_name", ["nz12", "nz10"])
@pytest.mark.parametrize("shift,slide_z", SHIFTS, ids=[f"{s[0]}_{s[1]}_{s[2]}" for s, _ in SHIFTS])
def test_shift_table(backend, grid_name, shift, slide_z):
    """x, y and z shifts of both signs, by one voxel, by all but one, by the whole grid and beyond it.  nz = 12 with no z shift goes
    in 16-byte pieces; nz = 10 and every z shift go float by float."""
    grid = GRID8 if grid_name == "nz12" else GRID8_Z10
    steps = _structured() + [("sl", _sensor_at(grid, shift, slide_z=bool(slide_z)), _sp(threshold=0.0, slide_z=slide_z))]
    got = _check(backend, f"shift_{grid_name}_{shift}", grid, steps)
    before, after = got[2], got[3]
    l = _opt("emu").sense_logodds(steps[0][3])
    lo = before[0]
    assert (lo >= l[4]).sum() > 20 and (lo < l[5]).sum() > 200 and (lo == 0).sum() > 200 and (lo == l[3]).any() and (lo == l[2]).any()
    outside = any(abs(s) >= n for s, n in zip(shift, grid["dims"]))   # the sensor's voxel is then outside the window as well
    far = any(not 0 <= n // 2 + s < n for s, n in zip(shift, grid["dims"]))
    assert after[4] == (2 if far else 1) and after[5] == tuple(shift)
    assert (_bits(after[0]) == _bits(_np_shift(lo, shift))).all()
    assert (after[0] == 0).all() == outside and not after[1].any() and not after[2].any() and after[3] == 0
    want = np.array(grid["origin"] + grid["min_b"] + grid["max_b"]) + np.tile(np.array(shift) * grid["res"], 3)
    assert (after[6] == want).all()   # (exact: binary fractions)


# ---------------------------------------------------------------------------------------------------------------------
# 3. trigger and status
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_trigger_and_status(backend):
    ins = _structured()
    # 0.29 m from the low corner of the centre voxel: inside the threshold of 0.3; 0.31 m: outside it (voxel 14 in x)
    got = _check(backend, "trigger", GRID8, ins + [("sl", (0.29, 0.0, 0.5625), _sp()), ("sl", (0.31, 0.0, 0.5625), _sp())])
    assert got[3][4] == 0 and got[3][5] == (0, 0, 0) and _same(got[3][:4] + (0, (0, 0, 0), got[3][6]), got[2][:4] + (0, (0, 0, 0), got[2][6]))
    assert got[4][4] == 1 and got[4][5] == (2, 0, 0) and (_bits(got[4][0]) == _bits(_np_shift(got[2][0], (2, 0, 0)))).all()
    assert got[4][6][0] == -1.25 and got[4][6][3] == -1.25 and got[4][6][6] == 1.75
    # an open batch: nothing changes; once it is closed the same call slides
    two = _prm(batch_update_size=2)
    far = _sensor_at(GRID8, (3, -5, 0))
    steps = [("ins", _cloud(100, 41), (0.05, 0.05, 0.55), two), ("sl", far, _sp(threshold=0.0)), ("ins", _cloud(100, 42), (0.05, 0.05, 0.55), two),
             ("sl", far, _sp(threshold=0.0))]
    got = _check(backend, "open_batch", GRID8, steps)
    assert got[0][3] == 1 and got[0][1].sum() > 0
    assert got[1][4] == -1 and got[1][5] == (0, 0, 0) and got[1][3] == 1 and all((_bits(x) == _bits(y)).all() for x, y in zip(got[1][:3], got[0][:3]))
    assert (got[1][6] == got[0][6]).all()
    assert got[2][4] == 1 and got[2][3] == 0 and got[3][4] == 1 and got[3][5] == (3, -5, 0)
    assert (_bits(got[3][0]) == _bits(_np_shift(got[2][0], (3, -5, 0)))).all() and (got[3][0] != 0).any()
    # a sensor outside the window slides whatever the threshold says, and reports 2
    got = _check(backend, "outside", GRID8, ins + [("sl", (2.0, 0.0625, 0.5625), _sp(threshold=100.0))])
    assert got[3][4] == 2 and got[3][5] == (16, 0, 0) and (_bits(got[3][0]) == _bits(_np_shift(got[2][0], (16, 0, 0)))).all()
    assert (got[3][0] != 0).any()
    # slide_z = 0: a sensor far above the window neither triggers nor shifts z
    high = (0.0625, 0.0625, 50.0)
    got = _check(backend, "high", GRID8, ins + [("sl", high, _sp()), ("sl", high, _sp(threshold=0.0)), ("sl", high, _sp(threshold=0.0, slide_z=1))])
    assert got[3][4] == 0 and got[4][4] == 1 and got[4][5] == (0, 0, 0) and (_bits(got[4][0]) == _bits(got[2][0])).all()
    assert (got[4][6] == got[2][6]).all()
    assert got[5][4] == 2 and got[5][5] == (0, 0, 394) and (got[5][0] == 0).all()   # as the reference: z slides, everything leaves


# ---------------------------------------------------------------------------------------------------------------------
# 4. a slid window is a crop of a fixed map
# ---------------------------------------------------------------------------------------------------------------------
BIG = dict(origin=(-1.5, -1.5, 0.0), res=0.125, dims=(48, 24, 12), min_b=(-1.5, -1.5, 0.0), max_b=(4.5, 1.5, 1.5))


def _near(sensor, n, seed):
    """n points within 0.55 m of the sensor on a lattice of 1/4096 m: float32 holds them exactly, no point is beyond the range of
    0.6 m, so every coordinate, difference and quotient of the traversal is the same number in the frame of either grid.  (A
    coarse lattice would put ray ends on voxel edges, where the traversal overshoots to the map's border: test_sense's tie case.)"""
    r = np.random.default_rng(seed)
    d = r.integers(-2252, 2253, size=(4 * n, 3)) / 4096.0
    d = d[(np.linalg.norm(d, axis=1) < 0.55) & (np.linalg.norm(d, axis=1) > 0.05)][:n]
    assert len(d) == n
    return _pts(np.array(sensor) + d)


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_slid_window_is_a_crop_of_a_fixed_map(backend):
    prm = _prm(ray_range=[0.0, 0.6])
    sensors = [(-0.125, 0.125, 0.5625), (0.125, -0.0625, 0.6875), (0.9375, 0.125, 0.5625), (1.125, -0.125, 0.6875)]
    ins = [("ins", _near(s, 120, 50 + i), s, prm) for i, s in enumerate(sensors)]
    slide = ("sl", _sensor_at(GRID8, (8, 0, 0)), _sp(threshold=0.0))
    # The condition (not a tolerance): no ray comes within 0.7 m of a border in x or y of either grid, so neither grid ever clips a
    # ray or the update box there.  Shown on the checker with the batch left open, so that the counts of every insert stay visible:
    # the outermost six layers (0.75 m) in x and y hold none.  (In z both grids have the same extent and clip alike.)
    open_ = _prm(ray_range=[0.0, 0.6], batch_update_size=100)
    for grid, which in ((BIG, ins), (GRID8, ins[:2]), (dict(GRID8, origin=(-0.5, -1.5, 0.0)), ins[2:])):
        pm = wl.ProbMapCheck(grid["origin"], grid["res"], grid["dims"])
        for _, cloud, sensor, _ in which:
            assert pm.update(cloud, sensor, open_) == 0
        op = pm.get()[1]
        assert op.sum() > 0 and not op[:6].any() and not op[-6:].any() and not op[:, :6].any() and not op[:, -6:].any()
    win = _check(backend, "crop_window", GRID8, ins[:2] + [slide] + ins[2:])
    big = _check(backend, "crop_big", BIG, ins)
    assert win[2][4] == 1 and win[2][5] == (8, 0, 0) and win[2][6][0] == -0.5
    for i, j in ((0, 0), (1, 1)):   # before the slide the window is big[0:24] ...
        assert (_bits(win[i][0]) == _bits(big[j][0][:24])).all()
    for i, j in ((2, 1), (3, 2), (4, 3)):   # ... and from the slide on big[8:32], bit for bit
        assert (_bits(win[i][0]) == _bits(big[j][0][8:32])).all(), (i, j)
    kept = win[2][0][:16]
    assert (kept != 0).sum() > 100 and (_bits(kept) == _bits(win[1][0][8:])).all()   # what stayed is what the window knew
    entered = win[4][0][16:]
    assert not win[2][0][16:].any() and (entered != 0).sum() > 5   # what entered was unknown until the later inserts touched it
    assert (big[3][0][:8] != 0).any()   # (the fixed map still holds what the window has forgotten)


# ---------------------------------------------------------------------------------------------------------------------
# 6. several slots, one call
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _several(backend):
    """Three slots with three different beliefs slid in one call, and three slots with the same beliefs slid one by one."""
    opt = _opt(backend)
    slots, alone = [30, 31, 33], [40, 41, 42]
    sensors = [_sensor_at(GRID8, (2, 0, 0)), _sensor_at(GRID8, (0, 0, 0)), _sensor_at(GRID8, (-24, 1, 0))]
    ins = _structured()
    opt.sense_reset(slots + alone, **GRID8)
    for k, m in enumerate(slots + alone):
        for step in ins[:1 + k % 3]:   # one, two and three inserts
            _apply(opt, m, step)
    before = [opt.sense_get(m)[0] for m in slots]
    st, sh = opt.sense_slide(slots, sensors)
    one = [opt.sense_slide([a], [sensors[k]]) for k, a in enumerate(alone)]
    state = lambda m: opt.sense_get(m) + (np.concatenate(opt.sense_desc(m)),)
    return dict(before=before, st=st, sh=sh, one=one, together=[state(m) for m in slots], alone=[state(m) for m in alone])


@pytest.mark.parametrize("backend", BACKENDS)
def test_several_slots_in_one_call(backend):
    """Shifts (2, 0, 0), none and (-24, 1, 0) in one call at the default threshold: each slot ends as it does alone."""
    R = _several(backend)
    assert list(R["st"]) == [1, 0, 2] and R["sh"].tolist() == [[2, 0, 0], [0, 0, 0], [-24, 1, 0]]
    for k, (got, want) in enumerate(zip(R["together"], R["alone"])):
        assert R["one"][k][0][0] == R["st"][k] and (R["one"][k][1][0] == R["sh"][k]).all()
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[:3], want[:3])) and got[3] == want[3] == 0
        assert (_bits(got[0]) == _bits(_np_shift(R["before"][k], R["sh"][k]))).all() and (got[4] == want[4]).all()
    assert (R["together"][0][0] != 0).any() and (_bits(R["together"][1][0]) == _bits(R["before"][1])).all() and (R["before"][1] != 0).any()
    assert not R["together"][2][0].any() and (R["before"][2] != 0).any()
    if backend == "gpu":
        E = _several("emu")
        assert (R["st"] == E["st"]).all() and (R["sh"] == E["sh"]).all()
        for got, want in zip(R["together"], E["together"]):
            assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[:3], want[:3])) and (_bits(got[4]) == _bits(want[4])).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    opt = _opt("emu")
    L = opt.L
    opt.sense_reset([20, 21], **GRID8)
    _apply(opt, 20, _structured()[0])
    before = opt.sense_get(20), opt.sense_desc(20)
    sp = np.array([_sensor_at(GRID8, (3, 0, 0))] * 2, dtype=np.float64)
    st, sh = np.zeros(2, dtype=np.int32), np.zeros((2, 3), dtype=np.int32)

    def call(ids, n=None, pos=sp, prm=None, ids_null=False):
        ids = np.array(ids, dtype=np.int32)
        return L.topay_sense_slide(opt.h, len(ids) if n is None else n, None if ids_null else api._ip(ids), None if pos is None else api._dp(pos),
                                   None if prm is None else prm, api._ip(st), api._ip(sh))

    assert call([22]) == -3                                    # a slot without a belief: TOPAY_ERR_NO_MAP
    assert call([20, 20]) == -1                                # a slot named twice: TOPAY_ERR_INVALID_ARG from here on
    assert call([-1]) == -1 and call([10 ** 6]) == -1          # a slot out of range
    assert call([20], n=0) == -1 and call([20], n=-2) == -1    # n <= 0
    assert call([20], ids_null=True) == -1                     # NULL map_ids
    assert call([20], pos=None) == -1                          # NULL sensor_pos
    assert call([20], prm=_sp(threshold=-0.1)) == -1           # a negative threshold
    assert call([20], prm=_sp(threshold=float("nan"))) == -1 and call([20], prm=_sp(threshold=float("inf"))) == -1   # not finite
    for bad in (float("nan"), float("inf"), 1.0e6 + 2.0):      # a sensor that is not finite, or more than 1e6 m from the origin
        for a in range(3):
            pos = sp.copy()
            pos[1, a] = bad
            assert call([21, 20], pos=pos) == -1, (bad, a)
    after = opt.sense_get(20), opt.sense_desc(20)
    assert all((_bits(x) == _bits(y)).all() for x, y in zip(before[0][:3], after[0][:3])) and all((x == y).all() for x, y in zip(before[1], after[1]))
    assert call([20, 21], prm=_sp(threshold=0.0)) == 0 and list(st) == [1, 1] and sh.tolist() == [[3, 0, 0], [3, 0, 0]]   # (the same call, legal)
    assert L.topay_sense_slide(opt.h, 1, api._ip(np.array([20], dtype=np.int32)), api._dp(sp), None, None, None) == 0      # defaults, no outputs


# ---------------------------------------------------------------------------------------------------------------------
# 5. commit after a slide
# ---------------------------------------------------------------------------------------------------------------------
WORLD_SEED, TRUTH, BELIEF, PLAIN = 3, 2, 0, 5
POSES = np.array([[0.0, 0.0, 0.4, 0.3], [-0.6, 0.5, 0.8, 2.0], [0.7, -0.6, 0.2, -1.0]])
GRID_W = dict(origin=(-1.2, -1.2, 0.0), res=0.1, dims=(24, 24, 16), min_b=(-1.2, -1.2, 0.0), max_b=(1.2, 1.2, 1.6))


@functools.lru_cache(maxsize=None)
def _committed_after_a_slide(backend):
    """A 2.4 x 2.4 x 1.6 m tables world scanned from two poses into the belief slot and committed; then the belief slid by
    (4, -3, 0), a third scan inserted, and committed again.  The states: chassis at x in 1.2 .. 1.55, beyond the first window."""
    opt = _opt(backend)
    prm = api.world_params(0, size_xy=2.4, size_z=1.6, lib=opt.L)
    assert (opt.generate_worlds(prm, [WORLD_SEED], first_map_id=TRUTH) != 0).all()
    opt.sense_reset([BELIEF], **GRID_W)
    sp = opt.sense_params(point_filt_num=1, ray_range=[0.0, 2.0])
    clouds = []

    def frame(pose):
        off, pts = opt.sense_scan([TRUTH], [pose], 64, 16, 1.2, 2.0)
        assert int(opt.sense_insert([BELIEF], api.SENSE_LAST_SCAN, [pose[:3]], sp, cloud_off=off)[0]) == 1
        clouds.append(pts[0].copy())

    frame(POSES[0])
    frame(POSES[1])
    opt.sense_commit([BELIEF])
    r = np.random.default_rng(7)
    states = np.zeros((400, 10))
    states[:, 0], states[:, 1], states[:, 2] = r.uniform(1.2, 1.55, 400), r.uniform(-1.4, 0.8, 400), r.uniform(-3, 3, 400)
    col_old = opt.whole_body_collision(states, BELIEF)
    sensor = _sensor_at(GRID_W, (4, -3, 0))
    slide = opt.sense_slide([BELIEF], [sensor], opt.sense_slide_params(threshold=0.0))
    frame(POSES[2])
    col_between = opt.whole_body_collision(states, BELIEF)   # the slot still holds the fields and the descriptor of the first commit
    desc = opt.sense_desc(BELIEF)
    opt.sense_commit([BELIEF])
    occ = opt.get_occupancy(BELIEF)
    e2, e3, _ = opt.get_map(BELIEF)
    inf, crit = opt.get_map_fields(BELIEF)
    return dict(sp=sp, clouds=clouds, sensor=sensor, slide=slide, desc=desc, belief=opt.sense_get(BELIEF), occ=occ, fields=(e2, e3, inf, crit), states=states,
                col_old=col_old, col_between=col_between, col_new=opt.whole_body_collision(states, BELIEF))


@pytest.mark.parametrize("backend", BACKENDS)
def test_commit_after_a_slide(backend):
    R = _committed_after_a_slide(backend)
    opt = _opt(backend)
    assert int(R["slide"][0][0]) == 1 and R["slide"][1].tolist() == [[4, -3, 0]]
    res = np.float64(0.1)
    by = np.array([4, -3, 0], dtype=np.float64) * res
    origin, mn, mx = np.array(GRID_W["origin"]) + by, np.array(GRID_W["min_b"]) + by, np.array(GRID_W["max_b"]) + by
    assert all((_bits(g) == _bits(w)).all() for g, w in zip(R["desc"], (origin, mn, mx)))
    if backend == "emu":   # the belief and the grids against the checker's derivation from the same clouds
        pm = wl.ProbMapCheck(GRID_W["origin"], GRID_W["res"], GRID_W["dims"])
        for k, (cl, pose) in enumerate(zip(R["clouds"], POSES)):
            if k == 2:
                st, sh = pm.slide(R["sensor"], opt.sense_slide_params(threshold=0.0))
                assert st == 1 and sh.tolist() == [4, -3, 0] and (_bits(pm.origin) == _bits(origin)).all()
            assert pm.update(cl, pose[:3], R["sp"]) == 1
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(pm.get()[:3], R["belief"][:3]))
        want = pm.occupancy(R["sp"])
    else:
        E = _committed_after_a_slide("emu")
        assert all((_bits(a) == _bits(b)).all() for a, b in zip(R["clouds"], E["clouds"]))
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(R["belief"][:3], E["belief"][:3]))
        assert (R["col_new"] == E["col_new"]).all() and (R["col_old"] == E["col_old"]).all()
        want = [np.asarray(g) for g in E["occ"]]
    o2, oc, o3 = [np.asarray(g) for g in R["occ"]]
    assert (o2.reshape(-1) == want[0].reshape(-1)).all() and (oc.reshape(-1) == want[1].reshape(-1)).all() and (o3.reshape(-1) == want[2].reshape(-1)).all()
    assert o3.sum() > 20 and not o3.reshape(24, 24, 16)[20:].any()   # the four x layers that entered lie beyond the world: nothing there
    # the five fields: topay_build_esdf_fields with these grids on the slid descriptor, bit for bit
    opt.build_esdf_fields(origin, GRID_W["res"], GRID_W["dims"], mn, mx, o2, oc, o3, map_id=PLAIN)
    e2, e3, _ = opt.get_map(PLAIN)
    inf, crit = opt.get_map_fields(PLAIN)
    for got, ref in zip(R["fields"], (e2, e3, inf, crit)):
        assert (np.asarray(got).view(np.int64) == np.asarray(ref).view(np.int64)).all()
    # a chassis beyond the first window: outside the map (in collision) for the fields of the first commit, which a slide leaves in
    # place; after the second commit the slot answers on the slid grid, where some of these states are free
    assert R["col_old"].all() and (R["col_between"] == R["col_old"]).all()
    assert (opt.whole_body_collision(R["states"], PLAIN) == R["col_new"]).all() and 0 < (~R["col_new"]).sum() < len(R["col_new"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. a roaming episode
# ---------------------------------------------------------------------------------------------------------------------
ROAM_SEED, ROAM_X = 11, [-1.2, -0.7, -0.2, 0.3, 0.8]
ROAM_W = dict(origin=(-2.4, -1.2, 0.0), res=0.1, dims=(24, 24, 16), min_b=(-2.4, -1.2, 0.0), max_b=(0.0, 1.2, 1.6))


@functools.lru_cache(maxsize=None)
def _roam(backend):
    """The truth is a 4.8 x 4.8 x 1.6 m tables world (48 x 48 x 16: the generator makes square worlds only, so the 48 x 24 the issue
    names is its middle half), the belief a 24 x 24 x 16 window that starts on its left.  Five poses 0.5 m apart along x: scan
    (8 x 4 rays, range 1.0), slide at the default threshold, insert unless the status is 2, commit.  Then the sweep of a one-piece
    trajectory near the last pose, outside the first window.  No planning call."""
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB if backend == "emu" else None)
    prm = api.world_params(0, size_xy=4.8, size_z=1.6, lib=opt.L)
    assert (opt.generate_worlds(prm, [ROAM_SEED], first_map_id=TRUTH) != 0).all()
    assert opt._map_dims[TRUTH] == (48, 48, 16)
    opt.sense_reset([BELIEF], **ROAM_W)
    sp = opt.sense_params(point_filt_num=1, ray_range=[0.0, 1.0])
    steps = []
    for x in ROAM_X:
        pose = np.array([x, 0.0, 0.4, 0.0])
        off, pts = opt.sense_scan([TRUTH], [pose], 8, 4, 1.0, 1.0)
        st, sh = opt.sense_slide([BELIEF], [pose[:3]])
        ins = int(opt.sense_insert([BELIEF], api.SENSE_LAST_SCAN, [pose[:3]], sp, cloud_off=off)[0]) if st[0] != 2 else None
        opt.sense_commit([BELIEF])
        steps.append(dict(pose=pose, cloud=pts[0].copy(), st=int(st[0]), sh=sh[0].tolist(), ins=ins, belief=opt.sense_get(BELIEF),
                          desc=np.concatenate(opt.sense_desc(BELIEF)), occ=opt.get_occupancy(BELIEF), e2=opt.get_map(BELIEF)[0]))
    co = np.zeros((1, 9, 6))
    co[0, 1, 4] = 0.3   # arc length 0.3 t along yaw 0, for 0.5 s
    opt.track_set(3, 1, [0.7, 0.0, 0.0], [0.5], co)
    safe = opt.track_safe([3], [BELIEF])
    return dict(sp=sp, steps=steps, safe=safe)


def test_roaming_episode_on_the_emulator_matches_the_checker():
    E = _roam("emu")
    assert [s["st"] for s in E["steps"]] == [0, 1, 1, 1, 1] and [s["sh"] for s in E["steps"]] == [[0, 0, 0]] + [[5, 0, 0]] * 4
    assert all(s["ins"] == 1 for s in E["steps"])
    pm = wl.ProbMapCheck(ROAM_W["origin"], ROAM_W["res"], ROAM_W["dims"])
    for s in E["steps"]:
        st, sh = pm.slide(s["pose"][:3], _sp())
        assert st == s["st"] and sh.tolist() == s["sh"] and (_bits(pm.origin) == _bits(s["desc"][:3])).all()
        assert pm.update(s["cloud"], s["pose"][:3], E["sp"]) == 1
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(pm.get()[:3], s["belief"][:3]))
        want = pm.occupancy(E["sp"])
        assert all((np.asarray(g).reshape(-1) == w.reshape(-1)).all() for g, w in zip(s["occ"], want))
    last = E["steps"][-1]
    assert abs(last["desc"][0] - (-0.4)) < 1e-12 and (last["belief"][0] != 0).sum() > 50
    safe, first_hit, hit = E["safe"]   # the sweep answered from the slid map: the trajectory lies outside the first window
    assert safe.shape == (1,) and (first_hit[0] >= 0).all() != bool(safe[0])


@pytest.mark.gpu
def test_roaming_episode_on_the_device_matches_the_emulator():
    E, D = _roam("emu"), _roam("gpu")
    for d, e in zip(D["steps"], E["steps"]):
        assert d["st"] == e["st"] and d["sh"] == e["sh"] and d["ins"] == e["ins"] and (_bits(d["desc"]) == _bits(e["desc"])).all()
        assert (_bits(d["cloud"]) == _bits(e["cloud"])).all()
        assert all((_bits(x) == _bits(y)).all() for x, y in zip(d["belief"][:3], e["belief"][:3])) and d["belief"][3] == e["belief"][3]
        assert all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(d["occ"], e["occ"]))
        assert (_bits(d["e2"]) == _bits(e["e2"])).all()
    for d, e in zip(D["safe"], E["safe"]):
        assert d.shape == e.shape and np.array_equal(d, e, equal_nan=d.dtype == np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the scratch image is the context's: it grows to the largest call, is reused, and goes with the context
# ---------------------------------------------------------------------------------------------------------------------
def test_the_scratch_is_reused_and_given_back():
    import ctypes as C
    import gc

    L = api.load(EMU_LIB)
    for f in (L.topay_emu_live_allocations, L.topay_emu_live_events):
        f.restype = C.c_long
    gc.collect()
    before = L.topay_emu_live_allocations(), L.topay_emu_live_events()
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    opt.sense_reset([0, 1, 2], **GRID8)
    for m in (0, 1, 2):
        _apply(opt, m, _structured()[0])
    sp = opt.sense_slide_params(threshold=0.0)
    opt.sense_slide([0, 1], [_sensor_at(GRID8, (1, 0, 0))] * 2, sp)       # the largest call: two slots move
    grown = L.topay_emu_live_allocations()
    for ids in ([2], [0, 1], [1, 2]):                                      # no larger one: nothing is allocated
        opt.sense_slide(ids, [_sensor_at(GRID8, (0, 1, 0))] * len(ids), sp)
        assert L.topay_emu_live_allocations() == grown
    assert (opt.sense_get(2)[0] != 0).any() and opt.sense_slide_ms() >= 0.0
    opt.close()
    del opt
    gc.collect()
    assert (L.topay_emu_live_allocations(), L.topay_emu_live_events()) == before
