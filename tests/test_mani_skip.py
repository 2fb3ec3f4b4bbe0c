"""The manipulator block's skips of work whose result is exactly zero (TOPAY_MANI_SKIP_IDLE, topay_amd/csrc/topay_mani.h) change
no value: the lane-emulator build of the sources as they are is compared, bit for bit, with a second emulator library built
with -DTOPAY_MANI_SKIP_IDLE=0 (the code paths of before), and the device is compared with the oracle on the same inputs.

The inputs are the cuboids_small candidates (N = 4 ... 11: 13 N samples, every candidate ends in a partly filled pass) on the
fixture's map, in a free field, under a descending ceiling, over a rising floor, and in free fields with ONE voxel lowered so
that exactly one sample is pushed on sphere 0, respectively sphere 11.  Which samples and spheres a field touches is computed
here (sphere_centres / violations below: the block's forward kinematics and trilinear lookup restated in numpy, the sample
positions checked against the oracle's piece end points) and asserted; the oracle's per-term costs confirm which source of
force is on (it books the chassis top and the sphere pairs under one term).

What a bit comparison cannot see: a padding lane that votes although it must not only sends the wave down the full path, which
gives the same bits.  That the vote is over active lanes is a matter of speed, not of values, and is not tested here."""
import os
import shlex
import subprocess

import numpy as np
import pytest

from conftest import EMU_LIB, ROOT, serpentine_path, set_map
from oracle import oracle as orc
from topay_amd import api

EMU_DIR = os.path.join(ROOT, "tests", "emu")
LAM, RHO = [0.3, -0.2], [1e4, 2e4]


@pytest.fixture(scope="module")
def noskip_lib(tmp_path_factory, built_libs):
    """The emulator Makefile's own compiler line (as `make -n` prints it) plus -DTOPAY_MANI_SKIP_IDLE=0, into a temporary directory."""
    out = subprocess.check_output(["make", "-n", "-B", "-C", EMU_DIR, "libtopay_emu.so"], text=True)
    line = [l for l in out.splitlines() if " -shared " in l]
    assert len(line) == 1, out
    cmd = shlex.split(line[0])
    lib = str(tmp_path_factory.mktemp("emu_noskip") / "libtopay_emu_noskip.so")
    cmd[cmd.index("-o") + 1] = lib
    cmd.insert(1, "-DTOPAY_MANI_SKIP_IDLE=0")
    subprocess.check_call(cmd, cwd=EMU_DIR)
    return lib


class Field:
    """A map of the fixture's geometry with distance fields of its own."""

    def __init__(self, w, esdf2d, esdf3d):
        self.origin, self.res, self.dims, self.min_b, self.max_b = w.origin, w.res, w.dims, w.min_b, w.max_b
        self.esdf2d = np.ascontiguousarray(esdf2d, dtype=np.float64)
        self.esdf3d = np.ascontiguousarray(esdf3d, dtype=np.float64)
        self.view = orc.MapView(w.origin, w.res, w.dims, w.min_b, w.max_b, self.esdf2d, self.esdf3d)


def plane_field(w, z0, sign):
    """Distance to a horizontal plane at height z0: below it (sign +1, a ceiling) or above it (sign -1, a floor) is free."""
    nx, ny, nz = (int(v) for v in w.dims)
    zc = w.origin[2] + (np.arange(nz) + 0.5) * w.res
    e3 = np.broadcast_to(sign * (z0 - zc), (nx, ny, nz)).reshape(-1)
    return Field(w, np.full(nx * ny, 5.0), e3)


def free_field(w):
    n2, n3 = int(w.dims[0] * w.dims[1]), int(np.prod(w.dims))
    return Field(w, np.full(n2, 5.0), np.full(n3, 5.0))


K = 12   # Simpson intervals per piece: the even samples m = 0 ... K of a piece are the penalty samples


def sphere_centres(o, prm):
    """World centres [13 N, 12, 3] of the arm's spheres at every penalty sample of the trajectory the oracle last evaluated
    (sample e = 13 i + m), as manipulator_block forms them; the XY positions by the evaluation's Simpson prefix."""
    c, T = o.coeffs()
    N = o.N
    knots = o.get_traj()[2]
    relR = np.array(prm.relative_R[:9]).reshape(3, 3)
    relT = np.array(prm.relative_t[:3])
    L = np.array(prm.colli_length[:8])
    cp, cr = np.array(prm.colli_points[:16]), np.array(prm.colli_point_radius[:16])
    off, rad = cp[cp != 0.0][:12], cr[cp != 0.0][:12]
    poly = lambda row, i, s: sum(c[row, 6 * i + k] * s ** k for k in range(6))
    out = np.zeros((13 * N, 12, 3))
    pos = knots[0].copy()
    for i in range(N):
        h = T[i] / K / 2
        assert np.abs(pos - knots[i]).max() < 1e-9      # the prefix reproduces the oracle's piece end points
        vel = lambda j: sum(k * c[1, 6 * i + k] * (j * h) ** (k - 1) for k in range(1, 6)) * np.array(
            [np.cos(poly(0, i, j * h)), np.sin(poly(0, i, j * h))])
        for m in range(K + 1):
            s = 2 * m * h
            th = poly(0, i, s)
            q = [poly(2 + a, i, s) for a in range(7)]
            Rz = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
            A = Rz @ relR
            p0 = np.array([pos[0], pos[1], prm.chassis_height + relT[2]]) + np.append(Rz[:2, :2] @ relT[:2], 0.0)
            R, org, k = np.eye(3), np.zeros(3), 0
            for link in range(8):
                for _ in range(2 if link % 2 == 0 else 1):
                    out[13 * i + m, k] = p0 + A @ (org + R[:, 2] * off[k])
                    k += 1
                org = org + R[:, 2] * L[link]
                if link < 7:
                    cq, sq = np.cos(q[link]), np.sin(q[link])
                    R = R @ (np.array([[cq, -sq, 0], [sq, cq, 0], [0, 0, 1]]) if link % 2 == 0
                             else np.array([[cq, 0, sq], [0, 1, 0], [-sq, 0, cq]]))
            if m < K:
                pos = pos + (2 * h) / 6 * (vel(2 * m) + 4 * vel(2 * m + 1) + vel(2 * m + 2))
    return out, rad


def violations(field, P, rad):
    """ESDF violation sph_viol[k] - 10 d of every (sample, sphere): esdf3d_query restated (trilinear, clamped neighbours,
    d = 0 outside the map)."""
    r, org, dims = field.res, np.asarray(field.origin), np.asarray(field.dims)
    e3 = field.esdf3d.reshape(dims)
    idx = np.floor((P - 0.5 * r - org) / r).astype(int)
    fr = (P - ((idx + 0.5) * r + org)) / r
    lo, hi = np.clip(idx, 0, dims - 1), np.clip(idx + 1, 0, dims - 1)
    d = np.zeros(P.shape[:2])
    for bx, by, bz in np.ndindex(2, 2, 2):
        ix = (hi if bx else lo)[..., 0]
        iy = (hi if by else lo)[..., 1]
        iz = (hi if bz else lo)[..., 2]
        wgt = (fr[..., 0] if bx else 1 - fr[..., 0]) * (fr[..., 1] if by else 1 - fr[..., 1]) * (fr[..., 2] if bz else 1 - fr[..., 2])
        d += wgt * e3[ix, iy, iz]
    inside = np.all((P >= np.asarray(field.min_b) + 1e-4) & (P <= np.asarray(field.max_b) - 1e-4), axis=-1)
    return rad * 10.0 * 1.1 - np.where(inside, d, 0.0) * 10.0


def one_voxel_field(w, P, rad, sphere):
    """A free field with one voxel lowered so that exactly one sample violates, on `sphere` only, every other (sample, sphere)
    staying clear by a margin: the first sample for which that can be arranged.  Returns (field, sample)."""
    free = free_field(w)
    dims = np.asarray(w.dims)
    for e in range(P.shape[0]):
        cell = np.clip(np.round((P[e, sphere] - np.asarray(w.origin)) / w.res - 0.5).astype(int), 0, dims - 1)
        fr = np.abs((P[e, sphere] - ((cell + 0.5) * w.res + np.asarray(w.origin))) / w.res)
        wgt = np.prod(1.0 - fr)                                   # weight of the voxel at the sphere's centre
        e3 = free.esdf3d.copy().reshape(dims)
        e3[tuple(cell)] = 5.0 - (5.0 - 1.1 * rad[sphere]) / (0.8 * wgt)   # violation from 0.8 of that weight on
        f = Field(w, free.esdf2d, e3.reshape(-1))
        v = violations(f, P, rad)
        hit = v > -1e-3
        if hit.sum() == 1 and v[e, sphere] > 1e-3:
            return f, e
    raise AssertionError("no sample can be singled out on sphere %d" % sphere)


def terms_at(field, path, x):
    o = orc.Oracle(field.view)
    o.set_init_traj(path)
    o.set_alm(LAM, RHO)
    f, g = o.eval(2, x)
    return f, g, o.debug_terms()


@pytest.fixture(scope="module")
def crafted(cuboids_small):
    """[(name, field, candidate, x, f, g)] with the oracle's cost and gradient; every case is confirmed by the oracle's terms."""
    cs = cuboids_small
    w = cs["world"]
    prm = api.default_params(api.load(EMU_LIB))
    lim = np.array(prm.joint_pos_limit_max[:7])

    def centres(b, x):
        o = orc.Oracle(free_field(w).view)
        o.set_init_traj(path(b))
        o.set_alm(LAM, RHO)
        o.eval(2, x)
        return sphere_centres(o, prm)
    path = lambda b: cs["paths"][cs["offs"][b]:cs["offs"][b + 1]]
    world = Field(w, w.esdf2d, w.esdf3d)
    free = free_field(w)
    cases = []

    def x0_of(b):
        o = orc.Oracle(free.view)
        o.set_init_traj(path(b))
        return o.get_x(), o.N

    def add(name, field, b, x, want):
        f, g, t = terms_at(field, path(b), x)
        for k in ("mani_colli", "self_colli", "mani_pos"):
            assert (t[k] > 0) == (k in want), (name, b, k, t)
        cases.append((name, field, b, x, f, g))

    for b in range(len(cs["lens"])):
        x0, N = x0_of(b)
        cases.append(("world", world, b, x0) + terms_at(world, path(b), x0)[:2])
        # free space: no force on any sphere of any sample, the skip fires in every pass
        add("free", free, b, x0, ())
    for b in (0, 3):
        x0, N = x0_of(b)
        # one plane each, moved to the first 2 mm step at which it touches: ceiling -> the highest sphere of the fewest samples,
        # floor -> the base spheres of every sample
        for name, sign, zs in (("ceiling", 1.0, np.arange(3.0, -0.5, -0.002)), ("floor", -1.0, np.arange(-1.5, 1.6, 0.002))):
            lo, hi = 0, len(zs) - 1   # (the term is monotone in the plane's position: bisection)
            assert terms_at(plane_field(w, zs[hi], sign), path(b), x0)[2]["mani_colli"] > 0
            assert terms_at(plane_field(w, zs[lo], sign), path(b), x0)[2]["mani_colli"] == 0
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if terms_at(plane_field(w, zs[mid], sign), path(b), x0)[2]["mani_colli"] > 0:
                    hi = mid
                else:
                    lo = mid
            field = plane_field(w, zs[hi], sign)
            add(name, field, b, x0, ("mani_colli",))
            P, rad = centres(b, x0)
            hit = violations(field, P, rad) > 0
            assert hit.any()
            if name == "floor":      # link 0 does not move with the joints: its spheres at every sample, nothing above them
                assert not hit[:, 2:].any() and hit[:, :2].any(axis=1).all()
            else:                    # the tip sphere, in the few samples whose tip lies within 2 mm of the highest
                assert set(np.nonzero(hit.any(axis=0))[0]) == {11} and hit.any(axis=1).sum() <= 4
                assert P[hit][:, 2].min() > P[..., 2].max() - 0.002
        # one sample pushed on sphere 0 only, one on sphere 11 only (one active lane of one pass votes, for one sphere)
        P, rad = centres(b, x0)
        for sphere in (0, 11):
            field, e = one_voxel_field(w, P, rad, sphere)
            add("one_lane_sphere%d" % sphere, field, b, x0, ("mani_colli",))
        # joint position limit with no force on any sphere: the read-modify-write onto the +0.0 words (the last joint turns
        # the last link about its own axis: no sphere moves)
        x = x0.copy()
        x[3 * N - 1:].reshape(N - 1, 7)[:, 6] = lim[6] + 0.3
        add("joint_limit", free, b, x, ("mani_pos",))
        # the second joint leans the straightened arm over until its upper spheres come down to the chassis top (the oracle
        # books the chassis top and the sphere pairs under one term; a straight arm keeps its non-adjacent spheres apart)
        for lean in np.arange(0.8, 3.2, 0.1):
            x = x0.copy()
            q = x[3 * N - 1:].reshape(N - 1, 7)
            q[:] = 0.0
            q[:, 1] = lean
            t = terms_at(free, path(b), x)[2]
            if t["self_colli"] > 0:
                break
        add("chassis_top", free, b, x, ("self_colli",) + (("mani_pos",) if t["mani_pos"] > 0 else ()))
        # folded joints: sphere pairs collide (as in test_eval_rare_paths_match_oracle), no ESDF force
        x = x0.copy()
        x[3 * N - 1:] += np.tile([0.0, 1.5, 0.0, 2.4, 0.0, 1.9, 0.0], N - 1)
        t = terms_at(free, path(b), x)[2]
        add("pairs", free, b, x, ("self_colli",) + (("mani_pos",) if t["mani_pos"] > 0 else ()))
    return cases


def batch_of(crafted, cuboids_small, **kw):
    """One context holding every crafted case's candidate on its map: the fields in map slots, one candidate per case."""
    cs = cuboids_small
    opt = api.MomaTrajOptBatch(**kw)
    fields = []
    for c in crafted:
        if not any(c[1] is f for f in fields):
            fields.append(c[1])
    for k, f in enumerate(fields):
        opt.set_map(f.origin, f.res, f.dims, f.min_b, f.max_b, f.esdf2d, f.esdf3d, k)
    lens = np.array([cs["lens"][c[2]] for c in crafted], dtype=np.int32)
    paths = np.concatenate([cs["paths"][cs["offs"][c[2]]:cs["offs"][c[2] + 1]] for c in crafted])
    mid = np.array([[c[1] is f for f in fields].index(True) for c in crafted], dtype=np.int32)
    opt.set_init_traj(lens, paths, map_ids=mid)
    return opt


def test_skip_and_no_skip_builds_evaluate_to_the_same_bits(crafted, cuboids_small, noskip_lib):
    a = batch_of(crafted, cuboids_small, lib_path=EMU_LIB)
    b = batch_of(crafted, cuboids_small, lib_path=noskip_lib)
    for k, (name, field, cand, x, f, g) in enumerate(crafted):
        fa, ga, ea = a.eval(2, k, x, LAM, RHO)
        fb, gb, eb = b.eval(2, k, x, LAM, RHO)
        assert fa == fb and (ga == gb).all() and (ea == eb).all(), (name, cand)
        assert abs(f - fa) <= 1e-11 * abs(f) and np.abs(g - ga).max() <= 1e-10 * np.abs(g).max(), (name, cand)
    a.close()
    b.close()


def test_skip_and_no_skip_builds_solve_to_the_same_bytes(cuboids_small, noskip_lib):
    """Capped solve (12 stage-2 iterations) of four candidates: byte-identical iterates, equal statistics."""
    cs = cuboids_small
    sel = [0, 1, 3, 5]
    lens = cs["lens"][sel]
    paths = np.concatenate([cs["paths"][cs["offs"][i]:cs["offs"][i + 1]] for i in sel])
    res = []
    for lib in (EMU_LIB, noskip_lib):
        p = api.default_params(api.load(lib))
        p.s2_lbfgs.max_iterations = 12
        p.alm_max_outer = 1
        opt = api.MomaTrajOptBatch(params=p, lib_path=lib)
        set_map(opt, cs["world"])
        opt.optimizeTraj(lens, paths)
        res.append(([opt.get_x(k).tobytes() for k in range(len(sel))], opt.stats().copy()))
        opt.close()
    assert res[0][0] == res[1][0]
    assert (res[0][1] == res[1][1]).all()


@pytest.mark.gpu
def test_crafted_cases_on_the_device_match_the_oracle(crafted, cuboids_small):
    """eval(2, ...) of the crafted cases (N = 4 ... 11) and of one long-class candidate (N > 32) against the oracle."""
    gpu = batch_of(crafted, cuboids_small, device=0)
    for k, (name, field, cand, x, f, g) in enumerate(crafted):
        fg, gg, _ = gpu.eval(2, k, x, LAM, RHO)
        assert abs(f - fg) <= 1e-11 * abs(f), (name, cand)
        assert np.abs(g - gg).max() <= 1e-10 * np.abs(g).max(), (name, cand)
    gpu.close()
    # the long-class kernel (four waves): a 40 m serpentine on the fixture's map and in free space
    w = cuboids_small["world"]
    path = serpentine_path(40.0)
    for field in (Field(w, w.esdf2d, w.esdf3d), free_field(w)):
        o = orc.Oracle(field.view)
        o.set_init_traj(path)
        assert o.N > 32
        x = o.get_x()
        o.set_alm(LAM, RHO)
        f, g = o.eval(2, x)
        opt = api.MomaTrajOptBatch(device=0)
        opt.set_map(field.origin, field.res, field.dims, field.min_b, field.max_b, field.esdf2d, field.esdf3d, 0)
        opt.set_init_traj(np.array([len(path)], dtype=np.int32), path)
        fg, gg, _ = opt.eval(2, 0, x, LAM, RHO)
        assert abs(f - fg) <= 1e-11 * abs(f)
        assert np.abs(g - gg).max() <= 1e-10 * np.abs(g).max()
        opt.close()
