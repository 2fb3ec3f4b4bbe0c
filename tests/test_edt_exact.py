"""The distance-field kernels (topay_amd/csrc/topay_edt.h, dispatched by topay_host_maps.h) against the brute-force
definition of tests/edt_reference.py, bit for bit, one named case per dispatch path.

Every comparison views the doubles as int64: there is no tolerance.  The emulator (CPU suite) and the device (gpu) are
each compared with the reference directly, never with each other.  Four of the five fields can be read back (esdf3d,
esdf2d, inflate, critical-inflate); the plain critical field is scratch on the device (its buffer is released at the end
of the build) and enters through its threshold grid, the seeds of critical-inflate.

Case -> path.  The dispatch is stated once in the library (edt_plan of topay_edt.h, which the launchers of
topay_host_maps.h read) and restated independently in `plan` below; every case asserts its selections against both --
the library under test is asked through api.edt_plan -- and test_plan_is_the_restatement compares the two statements
field by field on both sides of every decision:

 lines <= 512 cells in every dimension ("small"): z pass k_edt_first_ballot<nz> for nz in 16/32/64, else
 k_edt_direct; y pass k_edt_tile with wy = largest divisor of nz up to 64; x pass k_edt_tile_signed with
 wx = largest divisor of ny nz up to 32; each 2-D field k_edt_direct twice and k_edt_tile_signed with w2 = largest
 divisor of ny up to 32.  k_edt_threshold twice per build, k_edt_project when no critical grid is handed over.

   ballot16      9 x 7 x 16     k_edt_first_ballot<16>, 1008 cells: the last wave is partly dead; wy 16, wx 28, w2 7
   ballot32      5 x 7 x 32     k_edt_first_ballot<32>; wy 32, wx 32, w2 7
   ballot64      3 x 5 x 64     k_edt_first_ballot<64> (the q == 63 mask); wy 64, wx 32, w2 5
   direct_odd    23 x 19 x 12   k_edt_direct z pass; wy 12, wx 19, w2 19: widths that do not divide the 256-thread block
   wy1           6 x 5 x 67     nz prime above 64: wy 1; wx 5
   w2_1          8 x 37 x 3     ny prime above 32: w2 1 (k_edt_tile_signed with one line per tile); wy 3, wx 3
   tiny          4 x 3 x 5      tiles smaller than the block (cells < 256)
   ytile128k     2 x 512 x 64   k_edt_tile tile of 512 x 64 x 4 B = 128 KB, the LDS maximum
   xtile128k     512 x 4 x 8    k_edt_tile_signed tiles of 2 x 512 x 32 x 4 B = 128 KB
   x1 / y1       1 x 7 x 5, 6 x 1 x 5   a dimension of one cell in x or y (accepted); z = 1 is refused (pinned below)

 a dimension above 512 cells: the serial envelope k_edt_pass<SRC,FIN,WS>, stacks in LDS (WS 1) when
 (n + 2) x 640 B <= 56 KB, or <= 150 KB and maps x lines <= 65536; else in HBM (WS 0).

   env_x         513 x 5 x 3    3-D z <0,0,1>, y <1,0,1>, x <1,1,0>; 2-D y <0,0,1>, x <1,1,0>
   env_y         5 x 513 x 3    3-D z <0,0,1>, y <1,0,0>, x <1,1,1>; 2-D y <0,0,0>, x <1,1,1>
   env_z         3 x 5 x 513    3-D z <0,0,0>, y <1,0,1>, x <1,1,1>
   env_n1        513 x 1 x 2    a line of one cell through the envelope (y pass, 2-D y pass)
   env_lds100    513 x 100 x 3  y pass: 102 x 640 = 65280 B of LDS stacks (conditional: above 56 KB)
   env_lds101    513 x 101 x 3  y pass: 65920 B, above the 64 KB a kernel gets without hipFuncSetAttribute
   env_lds238    513 x 238 x 2  y pass: 153600 B = 150 KB, the longest line that still takes LDS stacks
   env_batch2    2 maps of 513 x 5 x 3 into slots 8, 9 (blockIdx.y = map in k_edt_pass, both stack placements)
   env_batch43   43 maps of 513 x 100 x 3: 43 x 1539 y lines > 65536, the same lines now take HBM stacks <1,0,0> (device only)
   batch3        3 maps of 23 x 19 x 13 into slots 5..7 (blockIdx.y = map in every small-line kernel)
   sense_commit  3 consecutive slots of 23 x 23 x 12 through topay_sense_commit: one batched construction
"""
import functools
import os
import re

import numpy as np
import pytest

import edt_reference as ref
from conftest import EMU_LIB, ROOT
from topay_amd import api

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
FIELDS = ("esdf3d", "esdf2d", "inflate", "critical_inflate")


@functools.lru_cache(maxsize=None)
def _opt(backend):
    return api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB if backend == "emu" else None)


def _radius():
    return float(api.default_params(api.load(EMU_LIB)).chassis_colli_radius)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch (edt_plan of topay_edt.h), restated
# ---------------------------------------------------------------------------------------------------------------------
def pick_w(lines, cap):
    return max(d for d in range(1, cap + 1) if lines % d == 0)


def env_lds_bytes(n):
    return (n + 2) * 64 * 10


def env_stacks(n, nlines, n_maps):
    lb = env_lds_bytes(n)
    return "lds" if lb <= 56 * 1024 or (lb <= 150 * 1024 and n_maps * nlines <= 65536) else "hbm"


def plan(dims, n_maps=1):
    nx, ny, nz = dims
    if max(dims) <= 512:
        wy, wx, w2 = pick_w(nz, 64), pick_w(ny * nz, 32), pick_w(ny, 32)
        return dict(family="small", first=f"ballot{nz}" if nz in (16, 32, 64) else "direct", wy=wy, wx=wx, w2=w2,
                    lds_y=ny * wy * 4, lds_x=nx * wx * 8, lds_2=nx * w2 * 8)
    ws = {"lds": 1, "hbm": 0}
    return dict(family="envelope",
                z=f"<0,0,{ws[env_stacks(nz, nx * ny, n_maps)]}>", y=f"<1,0,{ws[env_stacks(ny, nx * nz, n_maps)]}>",
                x=f"<1,1,{ws[env_stacks(nx, ny * nz, n_maps)]}>", y2=f"<0,0,{ws[env_stacks(ny, nx, n_maps)]}>",
                x2=f"<1,1,{ws[env_stacks(nx, ny, n_maps)]}>", lds_y=env_lds_bytes(ny))


def _lib(backend):
    """The library under test: the emulator build in the CPU cases, the product library in the gpu cases."""
    return api.load(EMU_LIB if backend == "emu" else None)


# Shapes on both sides of every decision of the dispatch (n_maps 1 unless a pair says otherwise).
SWEEP = ([(512, 7, 5), (513, 7, 5), (7, 512, 5), (7, 513, 5), (7, 5, 512), (7, 5, 513)]            # small / envelope, per axis
         + [(5, 7, nz) for nz in (15, 16, 17, 31, 32, 33, 63, 64, 65, 67)]                          # ballot widths, wy up to its cap
         + [(5, ny, 3) for ny in (31, 32, 33, 37)]                                                  # w2 up to its cap, prime above it
         + [(513, n, 3) for n in (87, 88, 100, 101, 238, 239)]                                      # y stacks: 56 KB, 64 KB, 150 KB
         + [(3, 513, n) for n in (87, 88, 238, 239)] + [(n, 513, 3) for n in (87, 88, 238, 239)]    # ... the same for z and for x, x2
         + [(513, 1, 2), (1, 513, 3), (1, 7, 5), (6, 1, 5)])                                        # one cell in x and in y
# 65536 lines in all and one map more: 513 x 100 x 3 has 1539 y lines of 65280 B of stacks (42 maps: 64638, 43: 66177);
# 1024 x 97 x 2 has 2048 y lines of 97 cells, 63360 B (32 maps: 65536 exactly, 33: 67584) and 1024 lines in its 2-D y pass
# (64 maps: 65536 exactly); 513 x 1 x 97 has 513 z lines of 97 cells (127 maps: 65151, 128: 65664)
SWEEP_MAPS = [((513, 100, 3), 42), ((513, 100, 3), 43), ((1024, 97, 2), 32), ((1024, 97, 2), 33), ((1024, 97, 2), 64), ((1024, 97, 2), 65),
              ((513, 1, 97), 127), ((513, 1, 97), 128), ((513, 1, 97), 129)]


def test_plan_is_the_restatement():
    """The library's own statement of the dispatch (edt_plan of topay_edt.h, which the construction reads) equals the restatement
    `plan`, field by field, on both sides of every decision: a change of the dispatch fails here instead of silently moving a
    case to another path."""
    lib = _lib("emu")
    shapes = [(d, 1) for d in SWEEP] + [(d, 1) for d, _, _ in list(SMALL.values()) + list(LARGE.values())] + SWEEP_MAPS
    for dims, n_maps in shapes:
        assert api.edt_plan(dims, n_maps, lib=lib) == plan(dims, n_maps), (dims, n_maps)
    # the sweep does sit on both sides of each threshold
    assert env_lds_bytes(87) <= 56 * 1024 < env_lds_bytes(88) and env_lds_bytes(238) == 150 * 1024 < env_lds_bytes(239)
    assert [plan((1024, 97, 2), m)["y"] for m in (32, 33)] == ["<1,0,1>", "<1,0,0>"] and 32 * 1024 * 2 == 65536
    assert [plan((1024, 97, 2), m)["y2"] for m in (64, 65)] == ["<0,0,1>", "<0,0,0>"] and 64 * 1024 == 65536
    assert [plan((513, 1, 97), m)["z"] for m in (127, 128)] == ["<0,0,1>", "<0,0,0>"]
    assert {plan(d)["family"] for d in SWEEP[:6]} == {"small", "envelope"}
    assert {plan(d)["first"] for d in SWEEP[6:16]} == {"ballot16", "ballot32", "ballot64", "direct"}
    # every kernel the construction launches is one that a case below is named after
    src = open(os.path.join(ROOT, "topay_amd", "csrc", "topay_host_maps.h")).read()
    launched = set(re.findall(r"k_edt_[a-z_]+(?:<[0-9, ]+>)?", src))
    # Gone from this set because they were never launched: k_edt_tile<1, 1> (only its LDS attribute was set), and the template
    # arguments of k_edt_direct<0, 0> / k_edt_tile<1, 0> (the only instances ever launched: the kernels are plain functions now).
    assert launched == {"k_edt_first_ballot<16>", "k_edt_first_ballot<32>", "k_edt_first_ballot<64>", "k_edt_direct", "k_edt_tile",
                        "k_edt_tile_signed", "k_edt_pass<0, 0, 0>", "k_edt_pass<0, 0, 1>", "k_edt_pass<1, 0, 0>",
                        "k_edt_pass<1, 0, 1>", "k_edt_pass<1, 1, 0>", "k_edt_pass<1, 1, 1>", "k_edt_threshold", "k_edt_project"}, launched


# name -> (dims, res, expected selections)
SMALL = {
    "ballot16": ((9, 7, 16), 0.1, dict(first="ballot16", wy=16, wx=28, w2=7)),
    "ballot32": ((5, 7, 32), 0.1, dict(first="ballot32", wy=32, wx=32, w2=7)),
    "ballot64": ((3, 5, 64), 0.1, dict(first="ballot64", wy=64, wx=32, w2=5)),
    "direct_odd": ((23, 19, 12), 0.1, dict(first="direct", wy=12, wx=19, w2=19)),
    "wy1": ((6, 5, 67), 0.05, dict(first="direct", wy=1, wx=5, w2=5)),
    "w2_1": ((8, 37, 3), 0.1, dict(first="direct", wy=3, wx=3, w2=1)),
    "tiny": ((4, 3, 5), 0.1, dict(first="direct", wy=5, wx=15, w2=3, lds_y=60, lds_x=480)),
    "x1": ((1, 7, 5), 0.1, dict(first="direct", wy=5, wx=7, w2=7)),
    "y1": ((6, 1, 5), 0.1, dict(first="direct", wy=5, wx=5, w2=1)),
    "env_x": ((513, 5, 3), 0.1, dict(z="<0,0,1>", y="<1,0,1>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>")),
    "env_y": ((5, 513, 3), 0.1, dict(z="<0,0,1>", y="<1,0,0>", x="<1,1,1>", y2="<0,0,0>", x2="<1,1,1>")),
    "env_z": ((3, 5, 513), 0.1, dict(z="<0,0,0>", y="<1,0,1>", x="<1,1,1>", y2="<0,0,1>", x2="<1,1,1>")),
    "env_n1": ((513, 1, 2), 0.1, dict(z="<0,0,1>", y="<1,0,1>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>")),
}
LARGE = {
    "ytile128k": ((2, 512, 64), 0.2, dict(first="ballot64", wy=64, wx=32, w2=32, lds_y=128 * 1024)),
    "xtile128k": ((512, 4, 8), 0.2, dict(first="direct", wy=8, wx=32, w2=4, lds_x=128 * 1024)),
    "env_lds100": ((513, 100, 3), 0.2, dict(z="<0,0,1>", y="<1,0,1>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>", lds_y=65280)),
    "env_lds101": ((513, 101, 3), 0.2, dict(z="<0,0,1>", y="<1,0,1>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>", lds_y=65920)),
    "env_lds238": ((513, 238, 2), 0.2, dict(z="<0,0,1>", y="<1,0,1>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>", lds_y=150 * 1024)),
}


def _assert_plan(backend, dims, expect, n_maps=1):
    """The expected selections of a case, against the restatement and against what the library under test decides."""
    for who, got in (("restatement", plan(dims, n_maps)), ("library", api.edt_plan(dims, n_maps, lib=_lib(backend)))):
        for k, v in expect.items():
            assert got[k] == v, (who, dims, k, got[k], v)


def test_plan_of_every_case():
    for dims, _, expect in list(SMALL.values()) + list(LARGE.values()):
        _assert_plan("emu", dims, expect)
    assert env_lds_bytes(101) > 64 * 1024 >= env_lds_bytes(100) > 56 * 1024       # 101: above the default; both conditional
    assert env_stacks(238, 513 * 2, 1) == "lds" and env_stacks(239, 513 * 2, 1) == "hbm"
    _assert_plan("emu", (513, 100, 3), dict(y="<1,0,1>"), n_maps=42)              # 42 x 1539 = 64638 lines
    _assert_plan("emu", (513, 100, 3), dict(z="<0,0,1>", y="<1,0,0>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>"), n_maps=43)   # 66177
    _assert_plan("emu", (23, 19, 13), dict(first="direct", wy=13, wx=19, w2=19))
    _assert_plan("emu", (23, 23, 12), dict(first="direct", wy=12, wx=23, w2=23))


# ---------------------------------------------------------------------------------------------------------------------
# occupancy patterns: name -> (occ3d [nx, ny, nz], occ2d [nx, ny], critical grid or None), all int8 of 0 / 1
# ---------------------------------------------------------------------------------------------------------------------
def _low(o3):
    """occ2d as the reference fills it: the points below the chassis height (here: the lower half of the layers)."""
    return o3[:, :, :max(1, o3.shape[2] // 2)].any(axis=2).astype(np.int8)


def _other_critical(o2, rng):
    """An explicit critical grid that is not the projection: occ2d and a few cells of its own."""
    c = o2.copy()
    c.ravel()[rng.integers(0, c.size, size=3)] = 1
    return c


def dense_patterns(dims, seed):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z3 = lambda: np.zeros(dims, dtype=np.int8)
    out = {}
    out["empty"] = (z3(), np.zeros((nx, ny), np.int8), None)
    out["full"] = (np.ones(dims, np.int8), np.ones((nx, ny), np.int8), None)
    o = z3()
    for i in (0, nx - 1):
        for j in (0, ny - 1):
            for k in (0, nz - 1):
                o[i, j, k] = 1
    o2 = _low(o)
    out["corners"] = (o, o2, _other_critical(o2, rng))
    o = z3()
    o[nx - 1, ny - 1, nz - 1] = 1                    # the last cell of its x, y and z line (and of the map)
    o2 = np.zeros((nx, ny), np.int8)
    o2[nx - 1, ny - 1] = 1
    out["last_cell"] = (o, o2, None)
    for ax in range(3):
        o = z3()
        idx = [slice(None)] * 3
        idx[ax] = dims[ax] // 3
        o[tuple(idx)] = 1
        o2 = np.zeros((nx, ny), np.int8)
        if ax < 2:
            o2[tuple(idx[:2])] = 1
        else:
            o2[nx // 2, :] = 1                        # (a z plane projects onto everything: a line instead)
        out[f"plane_{'xyz'[ax]}"] = (o, o2, None)
    i, j, k = np.indices(dims)
    out["checkerboard"] = ((((i + j + k) & 1) == 0).astype(np.int8), (((i[:, :, 0] + j[:, :, 0]) & 1) == 0).astype(np.int8), None)
    out["random50"] = ((rng.random(dims) < 0.5).astype(np.int8), (rng.random((nx, ny)) < 0.5).astype(np.int8), None)
    o = (rng.random(dims) < 0.02).astype(np.int8)
    o2 = (rng.random((nx, ny)) < 0.02).astype(np.int8)
    out["random2"] = (o, o2, _other_critical(o2, rng))
    o = z3()                                          # solid boxes that touch the faces
    o[:max(1, nx // 4), :max(1, ny // 3), :] = 1
    o[nx - max(1, nx // 5):, ny // 2:, nz - max(1, nz // 3):] = 1
    o[nx // 2:nx // 2 + 2, ny - 1:, :max(1, nz // 2)] = 1
    out["boxes"] = (o, _low(o), None)
    return out


def sparse_patterns(dims, seed):
    """For the shapes whose dense brute force would take minutes: isolated voxels and small boxes, some of them on the far
    faces of every axis, about a hundred occupied cells."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    out = {}
    o = np.zeros(dims, np.int8)
    o[nx - 1, ny - 1, nz - 1] = 1
    o2 = np.zeros((nx, ny), np.int8)
    o2[nx - 1, ny - 1] = 1
    out["last_cell"] = (o, o2, None)
    o = np.zeros(dims, np.int8)
    for _ in range(40):
        o[rng.integers(nx), rng.integers(ny), rng.integers(nz)] = 1
    o[0, 0, 0] = o[nx - 1, 0, nz - 1] = o[0, ny - 1, 0] = o[nx - 1, ny - 1, nz - 1] = o[nx - 1, ny // 2, 0] = o[nx // 2, ny - 1, nz - 1] = 1
    o2 = _low(o)
    out["voxels"] = (o, o2, _other_critical(o2, rng))
    o = np.zeros(dims, np.int8)
    o[nx - min(nx, 3):, ny - min(ny, 4):, nz - min(nz, 2):] = 1     # on the far faces
    o[:min(nx, 2), ny // 2:ny // 2 + 3, :] = 1
    o[nx // 2:nx // 2 + 3, :min(ny, 2), :min(nz, 3)] = 1
    for _ in range(12):
        o[rng.integers(nx), rng.integers(ny), rng.integers(nz)] = 1
    out["boxes"] = (o, _low(o), None)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# build and compare
# ---------------------------------------------------------------------------------------------------------------------
def _desc(dims, res):
    return (0.0, 0.0, 0.0), res, dims, (0.0, 0.0, 0.0), tuple(d * res for d in dims)


def _read(opt, slot):
    e2, e3, _ = opt.get_map(slot)
    inf, crit = opt.get_map_fields(slot)
    return dict(esdf3d=e3, esdf2d=e2, inflate=inf, critical_inflate=crit)


def _same_bits(got, want, what):
    for f in FIELDS:
        g, w = got[f], want[f]
        assert g.dtype == np.float64 and g.shape == w.shape, (what, f)
        bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
        assert bad.size == 0, (what, f, int(bad.size), int(bad[0]), float(g[bad[0]]), float(w[bad[0]]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(dims, res, [(pattern, occ3, occ2, critical, reference fields)]): computed once, shared by the backends."""
    dims, res, _ = (SMALL.get(name) or LARGE[name])
    pats = dense_patterns(dims, 1234) if name in SMALL else sparse_patterns(dims, 4321)
    return dims, res, [(p, o3, o2, oc, ref.fields(o2, o3, dims, res, _radius(), oc)) for p, (o3, o2, oc) in pats.items()]


def _run_case(backend, name):
    dims, res, pats = _case(name)
    _assert_plan(backend, dims, (SMALL.get(name) or LARGE[name])[2])
    opt = _opt(backend)
    explicit = 0
    for p, o3, o2, oc, want in pats:
        assert o3.dtype == np.int8 and set(np.unique(o3)) <= {0, 1}
        opt.build_esdf_fields(*_desc(dims, res), o2, oc, o3, map_id=3)
        _same_bits(_read(opt, 3), want, (name, p))
        explicit += oc is not None and not (oc == o3.any(axis=2)).all()
    assert explicit >= 1    # an explicit critical grid that differs from the projection went through this path


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(SMALL))
def test_small_shape_every_pattern(name, backend):
    _run_case(backend, name)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(LARGE))
def test_large_shape_sparse_patterns(name, backend):
    _run_case(backend, name)


def test_reference_on_hand_computed_maps():
    """The reference itself, on maps small enough to do by hand (res 0.5, radius 0.4: the inflate grids are the occupancy)."""
    d2 = ref.sq_dist(np.array([[0, 0, 0, 0], [0, 0, 0, 1]], dtype=bool))
    assert d2.tolist() == [[10, 5, 2, 1], [9, 4, 1, 0]]
    assert (ref.sq_dist(np.zeros((2, 3, 2), dtype=bool)) == ref.NONE).all()
    o = np.zeros((3, 1, 2), np.int8)
    o[0, 0, 0] = 1
    f = ref.fields(o[:, :, 0], o, (3, 1, 2), 0.5, 0.4)
    far = 0.5 * np.sqrt(np.finfo(np.float64).max)
    assert f["esdf3d"].tolist() == [0.0, 0.5, 0.5, 0.5 * np.sqrt(2.0), 1.0, 0.5 * np.sqrt(5.0)]     # occupied: 0 + (-0.5 + 0.5)
    assert f["esdf2d"].tolist() == [0.0, 0.5, 1.0] and f["inflate"].tolist() == [0.0, 0.5, 1.0]
    full = ref.fields(np.ones((2, 2), np.int8), np.ones((2, 2, 2), np.int8), (2, 2, 2), 0.5, 0.4)
    assert (full["esdf3d"] == 0.0 + (-far + 0.5)).all() and (full["critical_inflate"] == -far + 0.5).all()
    empty = ref.fields(np.zeros((2, 2), np.int8), np.zeros((2, 2, 2), np.int8), (2, 2, 2), 0.5, 0.4)
    assert (empty["esdf3d"] == far).all() and (empty["inflate"] == far).all()
    # a line of 9 cells, the first occupied, res 0.1, radius 0.4: the cell at 0.1 * 4 = 0.4 is NOT below the radius, so the inflate
    # grid is cells 0..3; inside it the distance to the first free cell (4) less one cell, negative
    o2 = np.zeros((9, 1), np.int8)
    o2[0, 0] = 1
    g = ref.fields(o2, np.zeros((9, 1, 2), np.int8), (9, 1, 2), 0.1, 0.4)
    assert g["esdf2d"].tolist() == [0.0 + (-0.1 + 0.1)] + [0.1 * k for k in range(1, 9)] and 0.1 * 4.0 == 0.4
    assert g["inflate"].tolist() == [0.0 + (-(0.1 * k) + 0.1) for k in (4.0, 3.0, 2.0, 1.0)] + [0.1 * k for k in range(1, 6)]
    none = 0.1 * np.sqrt(np.finfo(np.float64).max)
    assert (g["critical"] == none).all() and (g["critical_inflate"] == none).all()            # no voxel in any column
    # a 3 x 3 block in a 7 x 7 map: centre -(2 - 1) cells, the block's rim 0, outside the distance to the block
    o2 = np.zeros((7, 7), np.int8)
    o2[2:5, 2:5] = 1
    e2 = ref.fields(o2, np.zeros((7, 7, 2), np.int8), (7, 7, 2), 0.1, 0.4)["esdf2d"].reshape(7, 7)
    assert e2[3, 3] == 0.0 + (-(0.1 * 2.0) + 0.1) and e2[2, 2] == 0.0 and e2[0, 3] == 0.1 * 2.0 and e2[0, 0] == 0.1 * np.sqrt(8.0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_single_layer_is_refused(backend):
    """nz = 1: the lookups fetch z-neighbours in pairs, so the entry refuses the map (TOPAY_ERR_UNSUPPORTED = -6) before any launch."""
    with pytest.raises(api.TopayError, match=r"topay status -6: .*single layer"):
        _opt(backend).build_esdf_fields(*_desc((5, 4, 1), 0.1), np.zeros(20, np.int8), None, np.zeros(20, np.int8), map_id=3)


@functools.lru_cache(maxsize=None)
def _batch_maps(dims, n_maps, kind, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    maps = []
    for m in range(n_maps):
        if kind == "mixed":
            dens = (0.3, 0.02, 0.0)[m % 3]
            o3 = (rng.random(dims) < dens).astype(np.int8)
            if dens == 0.0:
                o3[:nx // 4, ny // 2:, :] = 1
                o3[nx - 2:, :3, nz - 4:] = 1
            o2 = (rng.random((nx, ny)) < dens).astype(np.int8) if dens else _low(o3)
        else:   # a handful of voxels, two of them on the far faces of the long axis, different in every map
            o3 = np.zeros(dims, np.int8)
            for _ in range(6):
                o3[rng.integers(nx), rng.integers(ny), rng.integers(nz)] = 1
            o3[nx - 1, rng.integers(ny), rng.integers(nz)] = 1
            o3[rng.integers(nx), ny - 1, nz - 1] = 1
            o2 = _low(o3)
        maps.append((o3, o2))
    return maps


@functools.lru_cache(maxsize=None)
def _batch_ref(dims, res, n_maps, kind, seed):
    return [ref.fields(o2, o3, dims, res, _radius()) for o3, o2 in _batch_maps(dims, n_maps, kind, seed)]


def _run_batch(backend, dims, res, n_maps, kind, seed, first):
    maps = _batch_maps(dims, n_maps, kind, seed)
    assert len({o3.tobytes() for o3, _ in maps}) == n_maps            # every map is different
    want = _batch_ref(dims, res, n_maps, kind, seed)
    opt = _opt(backend)
    opt.build_esdf_batch(*_desc(dims, res), np.stack([o2.ravel() for _, o2 in maps]), np.stack([o3.ravel() for o3, _ in maps]), first_map_id=first)
    for m in range(n_maps):
        _same_bits(_read(opt, first + m), want[m], (kind, "map", m))


@pytest.mark.parametrize("backend", BACKENDS)
def test_batch_of_three_maps_into_later_slots(backend):
    """build_esdf_batch of 3 different maps of 23 x 19 x 13 into slots 5, 6, 7: blockIdx.y = map in every kernel."""
    _run_batch(backend, (23, 19, 13), 0.1, 3, "mixed", 77, first=5)


@pytest.mark.parametrize("backend", BACKENDS)
def test_envelope_batch_of_two(backend):
    """2 maps of 513 x 5 x 3 into slots 8, 9: blockIdx.y = map in k_edt_pass, LDS stacks (z, y) and HBM stacks per map (x)."""
    _assert_plan(backend, (513, 5, 3), SMALL["env_x"][2], n_maps=2)
    _run_batch(backend, (513, 5, 3), 0.1, 2, "voxels", 98, first=8)


@pytest.mark.parametrize("backend", BACKENDS[1:])
def test_envelope_batch_of_43_takes_hbm_stacks(backend):
    """43 maps of 513 x 100 x 3: 43 x 1539 = 66177 y lines > 65536, so the 100-cell lines that took LDS stacks in env_lds100
    take HBM stacks (k_edt_pass<1,0,0>, one stack set per map: blockIdx.y x ws_stride).  res 0.5 > the chassis radius keeps the
    inflate grids as sparse as the occupancy, so the brute force of 43 maps stays under a second.

    Device only: the emulator needs 12 s for the 6.6 million cells.  It runs k_edt_pass<1,0,0> in env_y and the map dimension of
    a k_edt_pass launch in test_envelope_batch_of_two."""
    _assert_plan(backend, (513, 100, 3), dict(z="<0,0,1>", y="<1,0,0>", x="<1,1,0>", y2="<0,0,1>", x2="<1,1,0>"), n_maps=43)
    _run_batch(backend, (513, 100, 3), 0.5, 43, "voxels", 99, first=2)


# the grid, clouds and sensors of tests/test_sense.py::test_commit_of_consecutive_slots
GRID_ODD = dict(origin=(-1.15, -1.15, 0.0), res=0.1, dims=(23, 23, 12), min_b=(-1.15, -1.15, 0.0), max_b=(1.15, 1.15, 1.2))


def _cloud(n, seed, spread):
    r = np.random.default_rng(seed)
    xyz = np.stack([r.uniform(-spread, spread, n), r.uniform(-spread, spread, n), r.uniform(-0.2, 1.5, n)], axis=1).astype(np.float32)
    return np.concatenate([xyz, np.zeros((n, 1), np.float32)], axis=1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_sense_commit_of_consecutive_slots_against_the_definition(backend):
    """One topay_sense_commit of slots 10, 11, 12 (23 x 23 x 12) builds the fields of the three slots as ONE batch of three maps on
    the device (under the emulator the commit hands the run over slot by slot; a batch of three under the emulator is
    test_batch_of_three_maps_into_later_slots).  Every slot's fields are the definition's, from the occupancy grids that slot's
    commit produced (critical grid included)."""
    opt, slots = _opt(backend), [10, 11, 12]
    opt.sense_reset(slots, **GRID_ODD)
    clouds = [_cloud(300, 40 + k, 1.1) for k in range(3)]
    prm = opt.sense_params(point_filt_num=1)
    assert (opt.sense_insert(slots, clouds, [(0.05, 0.05, 0.55), (0.4, -0.3, 0.4), (-0.5, 0.5, 0.8)], prm) == 1).all()
    opt.sense_commit(slots)
    seen = set()
    for m in slots:
        o2, oc, o3 = opt.get_occupancy(m)
        assert o3.sum() > 5
        seen.add(o3.tobytes())
        want = ref.fields(o2, o3, GRID_ODD["dims"], GRID_ODD["res"], _radius(), occ2d_critical=oc)
        _same_bits(_read(opt, m), want, ("sense_commit", m))
    assert len(seen) == 3
