"""The replanning cycle around the planning call: tracked trajectories (MomaTraj::setTraj / getState / getDState,
moma_traj_opt.h:40-158), topay_track_safe == Planner::safeCallback (planner.cpp:597-638), topay_replan_inputs == the endpoints
of Planner::replanCallback (708-731), topay_replan_calls == one round of that callback for n robots.

Checker: harness/replan.hpp (wl.ReplanTraj), a serial CPU restatement with libm.  Tolerance of a state, a time or a distance
against it: 1e-11 absolute, the one tests/test_feasibility.py uses for the playback against the oracle (libm against the
deterministic sin / cos, scan against running sum in car_seq).  Verdict, sample index and body are compared exactly, under a
precondition asserted on the restatement alone: up to and including the first hit no body is closer than 1e-6 to its
threshold, four orders above the tolerance.
"""
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB
from harness import workload as wl
from topay_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
MARGIN = 1e-6
NEW_ENTRIES = ["topay_track_set", "topay_track_commit_plan", "topay_track_get", "topay_track_clear", "topay_track_safe", "topay_track_safe_ms",
               "topay_replan_inputs", "topay_replan_calls"]

# ---------------------------------------------------------------------------------------------------------------------
# hand-made trajectories and maps
# ---------------------------------------------------------------------------------------------------------------------
ORIGIN, RES, DIMS = np.array([-4.0, -4.0, 0.0]), 0.1, np.array([80, 80, 20], dtype=np.int32)
MIN_B, MAX_B = ORIGIN.copy(), ORIGIN + DIMS * RES


def _quintic(durs, v=1.0, omega=0.0, theta0=0.0, qrate=0.0):
    """Pieces in the layout of setTraj ([N, 9, 6], coefficient of t^5 first): arc-length rate v (+ a small t^2 term so that the
    higher orders are exercised), yaw theta0 + omega t, joint k = 0.1 k + qrate t, continuous across the pieces."""
    co = np.zeros((len(durs), 9, 6))
    t0 = 0.0
    for i, T in enumerate(durs):
        co[i, 0, 5], co[i, 0, 4] = theta0 + omega * t0, omega
        co[i, 1, 5], co[i, 1, 4], co[i, 1, 2] = v * t0, v, 0.01 * (i + 1)
        for k in range(7):
            co[i, 2 + k, 5], co[i, 2 + k, 4] = 0.1 * k * (k % 2) + qrate * t0, qrate
        t0 += T
    return np.array(durs, dtype=np.float64), co


def _occ(block2d=None, block3d=None):
    """Occupancy of the 80 x 80 x 20 grid: one far corner cell (so that no field is empty) plus boxes given in metres as
    (x0, x1, y0, y1) / (x0, x1, y0, y1, z0, z1)."""
    o2 = np.zeros((80, 80), dtype=np.int8)
    o3 = np.zeros((80, 80, 20), dtype=np.int8)
    o2[79, 79] = 1
    o3[79, 79, :] = 1
    c = lambda a, org: int(round((a - org) / RES))
    if block2d is not None:
        x0, x1, y0, y1 = block2d
        o2[c(x0, -4):c(x1, -4), c(y0, -4):c(y1, -4)] = 1
    if block3d is not None:
        x0, x1, y0, y1, z0, z1 = block3d
        o3[c(x0, -4):c(x1, -4), c(y0, -4):c(y1, -4), c(z0, 0):c(z1, 0)] = 1
    return o2.reshape(-1), o3.reshape(-1)


def _build(opt, slot, block2d=None, block3d=None):
    o2, o3 = _occ(block2d, block3d)
    opt.build_esdf(ORIGIN, RES, DIMS, MIN_B, MAX_B, o2, o3, map_id=slot)
    e2, e3, _ = opt.get_map(slot)
    return e2, e3


def _ref_safe(ref, fields):
    return ref.safe(ORIGIN, RES, DIMS, MIN_B, MAX_B, fields[0], fields[1])


# the shapes of issue section 2: (name, start3, durations, coeffs)
def _shapes():
    out = []
    d, c = _quintic([0.05])
    out.append(("5 samples", [0.62, 0.0, 0.0], d, c))
    d, c = _quintic([0.635])
    out.append(("64 samples", [0.03, 0.0, 0.0], d, c))
    d, c = _quintic([0.675])
    out.append(("68 samples", [0.0, 0.0, 0.0], d, c))
    d, c = _quintic([0.5, 0.5, 0.5])
    out.append(("3 pieces", [-0.75, 0.0, 0.0], d, c))
    return out


BLOCK2D = (1.0, 1.3, -0.5, 0.5)
BLOCK3D = (1.0, 1.3, -0.5, 0.5, 0.6, 1.0)


def _sweep_cases(opt):
    """Runs every shape against the free map, the 2-D block, the 3-D-only block, and one trajectory that leaves the map.
    Returns a list of (name, device outputs, restatement outputs)."""
    maps = {"free": _build(opt, 10), "block2d": _build(opt, 11, block2d=BLOCK2D), "block3d": _build(opt, 12, block3d=BLOCK3D)}
    slots = {"free": 10, "block2d": 11, "block3d": 12}
    shapes = _shapes()
    d, c = _quintic([1.0])
    shapes.append(("arm into the block", [0.2, 0.0, 0.0], d, c))
    d, c = _quintic([1.0, 1.0])
    shapes.append(("leaves the map", [3.0, 0.0, 0.0], d, c))
    out = []
    for r, (name, s3, dur, co) in enumerate(shapes):
        opt.track_set(r, 1, s3, dur, co)
        ref = wl.ReplanTraj(s3, dur, co)
        for mname in ("free", "block2d", "block3d"):
            safe, fh, hit = opt.track_safe([r], [slots[mname]])
            out.append((f"{name} / {mname}", (bool(safe[0]), int(fh[0, 0]), int(fh[0, 1]), float(hit[0, 0]), float(hit[0, 1])), _ref_safe(ref, maps[mname])))
    return out


def _check_sweeps(cases):
    by = {}
    for name, dev, ref in cases:
        print(name, dev, ref)
        assert ref["min_margin"] >= MARGIN, (name, ref)            # the precondition, on the restatement
        assert dev[0] == ref["safe"] and dev[1] == ref["sample"] and dev[2] == ref["body"], (name, dev, ref)
        if ref["safe"]:
            assert np.isnan(dev[3]) and np.isnan(dev[4])
        else:
            assert abs(dev[3] - ref["t"]) <= TOL and abs(dev[4] - ref["d"]) <= TOL, (name, dev, ref)
        by[name] = ref
    # the cases are what they are meant to be (conditions on the restatement)
    assert all(by[f"{s} / free"]["safe"] for s in ("5 samples", "64 samples", "68 samples", "3 pieces", "arm into the block", "leaves the map"))
    assert by["5 samples / block2d"]["body"] == 0 and by["5 samples / block2d"]["sample"] < 5
    assert by["64 samples / block2d"]["body"] == 0 and by["64 samples / block2d"]["sample"] == 63     # the last sample of the only pass
    assert by["68 samples / block2d"]["body"] == 0 and 64 <= by["68 samples / block2d"]["sample"] <= 67   # second pass, carry of the scan
    assert by["3 pieces / block2d"]["body"] == 0 and by["3 pieces / block2d"]["t"] > 1.0                 # in the last piece
    assert by["arm into the block / block3d"]["body"] >= 1 and by["arm into the block / block2d"]["body"] == 0
    assert by["leaves the map / block2d"]["safe"] and by["leaves the map / block3d"]["safe"]
    return True


def _endpoint_cases(opt):
    """Issue section 4 on one robot: end_traj = 3 pieces turning, global_traj = a longer one.  Returns (name, device, restatement)."""
    de, ce = _quintic([0.8, 0.7, 0.9], v=0.7, omega=0.4, qrate=0.05)
    dg, cg = _quintic([2.0, 2.5, 2.5], v=0.9, omega=-0.2, qrate=-0.03)
    s3 = [-1.0, 0.5, 0.3]
    opt.track_set(40, 1, s3, de, ce)
    opt.track_set(40, 2, s3, dg, cg)
    E, G = wl.ReplanTraj(s3, de, ce), wl.ReplanTraj(s3, dg, cg)
    gg = np.linspace(1.0, 2.0, 10)
    out = []
    for name, tr, tb, budget, horizon in (("horizon inside", 0.3, 0.45, 0.2, 1.5), ("second pass of the walk", 0.0, 0.0, 0.0, 6.0),
                                          ("horizon beyond", 0.3, 0.45, 0.2, 50.0), ("past the global trajectory", 0.3, 7.5, 0.2, 0.1),
                                          ("t_s beyond T", 2.3, 1.0, 0.5, 1.0)):
        st, sv, go, src = opt.replan_inputs([40], tr, tb, gg[None], budget, horizon)
        out.append((name, (st[0], sv[0], go[0], int(src[0])), E.endpoints(G, tr, tb, gg, budget, horizon)))
    return out, E, gg


def _check_endpoints(cases, E, gg):
    by = {}
    for name, dev, ref in cases:
        print(name, dev[3], ref[3])
        for k in range(3):
            assert np.abs(dev[k] - ref[k]).max() <= TOL, (name, k, dev[k], ref[k])
        assert dev[3] == ref[3], name
        by[name] = (dev, ref)
    assert by["horizon inside"][1][3] >= 0
    assert by["second pass of the walk"][1][3] >= 64                 # found by the second pass of 64 steps
    assert by["horizon beyond"][1][3] == -1 and (by["horizon beyond"][0][2] == gg).all()
    assert by["past the global trajectory"][1][3] == -1 and (by["past the global trajectory"][0][2] == gg).all()
    sT, vT = E.state(E.T)
    assert np.abs(by["t_s beyond T"][0][0] - sT).max() <= TOL and np.abs(by["t_s beyond T"][0][1] - vT).max() <= TOL
    return True


@pytest.fixture(scope="module")
def emu():
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    yield opt
    opt.close()


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite (lane emulator)
# ---------------------------------------------------------------------------------------------------------------------
def test_tracked_playback_matches_restatement(emu):
    """getState / getDState of a tracked trajectory (through topay_replan_inputs with t_s = t) for 1 and 3 hand-made pieces at
    t < 0, 0, a piece boundary, T, t > T and in between; track_get returns what track_set was given."""
    for robot, (durs, kw) in enumerate((([1.3], dict(v=0.8, omega=0.5, qrate=0.1)), ([0.4, 0.55, 0.37], dict(v=0.6, omega=-0.7, theta0=0.2, qrate=-0.2)))):
        d, c = _quintic(durs, **kw)
        s3 = [0.3, -0.2, kw.get("theta0", 0.0)]
        emu.track_set(robot, 3, s3, d, c)
        for which in (1, 2):
            g3, gd, gc = emu.track_get(robot, which)
            assert (g3 == s3).all() and (gd == d).all() and (gc == c).all()
        ref = wl.ReplanTraj(s3, d, c)
        T = ref.T
        for t in [-0.5, 0.0, durs[0], T, T + 1.0, 0.05, 0.1, 0.25 * T, 0.731 * T, T - 1e-9]:
            st, sv, _, src = emu.replan_inputs([robot], t, 0.0, np.zeros((1, 10)), 0.0, 1e9)
            rs, rv = ref.state(t)
            assert np.abs(st[0] - rs).max() <= TOL and np.abs(sv[0] - rv).max() <= TOL, (robot, t, st[0] - rs, sv[0] - rv)
            assert sv[0, 2] == 0.0 and src[0] == -1
    emu.track_clear(1)
    assert emu.track_get(1, 1) is None and emu.track_get(1, 2) is None and emu.track_get(0, 1) is not None


def test_tracked_playback_equals_batch_playback(cuboids_small):
    """The same coefficients as a solved candidate of a batch and as a tracked trajectory: getState bit for bit equal to
    topay_playback.  A capped emulator solve supplies the coefficients: a batch takes them only from a solve, and a solve
    has three pieces or more (two path states give three), so the hand-made 1-piece trajectory has no batch to compare with;
    its getState is held to the restatement in test_tracked_playback_matches_restatement."""
    cs = cuboids_small
    from conftest import set_map
    p = api.default_params(api.load(EMU_LIB))
    p.s1_lbfgs.max_iterations = 20
    p.s2_lbfgs.max_iterations = 20
    p.alm_max_outer = 1
    opt = api.MomaTrajOptBatch(params=p, device=0, lib_path=EMU_LIB)
    set_map(opt, cs["world"])
    opt.optimizeTraj(cs["lens"][:1], cs["paths"][:cs["offs"][1]])
    tr = opt.getTrajs([0])
    dur, co = tr["durations"], tr["coeffs"]
    assert len(dur) >= 3 and np.isfinite(co).all()
    s3 = cs["paths"][0][:3]
    assert (tr["knots_xy"][0] == s3[:2]).all()
    opt.track_set(7, 1, s3, dur, co)
    T = opt.total_durations()[0]
    times = np.concatenate([[-0.3, 0.0, dur[0], T, T + 2.0], np.linspace(0, T, 41)])
    pb, _ = opt.playback(0, times)
    for k, t in enumerate(times):
        st, _, _, _ = opt.replan_inputs([7], t, 0.0, np.zeros((1, 10)), 0.0, 1e9)
        assert (st[0] == pb[k]).all(), (t, st[0] - pb[k])
    opt.close()


def test_safety_sweep_shapes(emu):
    assert _check_sweeps(_sweep_cases(emu))


def _map_change_case(opt):
    """Issue section 3: one tracked trajectory against slots A = 20 and B = 21, before and after A is rebuilt with an obstacle
    on the path.  Checks against the restatement; returns the two sweeps' outputs."""
    d, c = _quintic([0.675])
    s3 = [0.0, 0.0, 0.0]
    opt.track_set(30, 1, s3, d, c)
    ref = wl.ReplanTraj(s3, d, c)
    _build(opt, 20)
    _build(opt, 21)
    first = opt.track_safe([30, 30], [20, 21])
    assert first[0].all()
    fields = _build(opt, 20, block2d=BLOCK2D)                # slot A rebuilt with an obstacle on the path
    r = _ref_safe(ref, fields)
    assert not r["safe"] and r["min_margin"] >= MARGIN
    safe, fh, hit = second = opt.track_safe([30, 30], [20, 21])
    assert not safe[0] and fh[0, 0] == r["sample"] and fh[0, 1] == r["body"] == 0
    assert abs(hit[0, 0] - r["t"]) <= TOL and abs(hit[0, 1] - r["d"]) <= TOL
    assert safe[1] and (fh[1] == -1).all()                   # the untouched slot B
    return first + second


def test_map_changes_under_the_trajectory(emu):
    _map_change_case(emu)


def test_replan_endpoints(emu):
    cases, E, gg = _endpoint_cases(emu)
    assert _check_endpoints(cases, E, gg)


def test_refusals(emu):
    L = emu.L
    d, c = _quintic([0.5, 0.5])
    s3 = np.zeros(3)
    _build(emu, 25)
    emu.track_set(50, 1, s3, d, c)
    one = np.array([50], dtype=np.int32)
    m25 = np.array([25], dtype=np.int32)
    for bad in (-1, 4096):                                    # a robot slot out of range
        assert L.topay_track_set(emu.h, bad, 1, api._dp(s3), 2, api._dp(d), api._dp(c.reshape(-1))) == -1
        b = np.array([bad], dtype=np.int32)
        assert L.topay_track_safe(emu.h, 1, api._ip(b), api._ip(m25), None, None, None) == -1
        assert L.topay_track_clear(emu.h, bad) == -1
    for which in (0, 4):                                      # which outside 1..3
        assert L.topay_track_set(emu.h, 51, which, api._dp(s3), 2, api._dp(d), api._dp(c.reshape(-1))) == -1
    empty = np.array([52], dtype=np.int32)                    # a sweep of an empty slot
    assert L.topay_track_safe(emu.h, 1, api._ip(empty), api._ip(m25), None, None, None) == -4            # TOPAY_ERR_NO_TRAJ
    with pytest.raises(api.TopayError, match="no end_traj"):
        emu.track_safe([52], [25])
    for durs in ([0.0, 0.0], [0.5, np.nan], [6000.0, 6000.0]):   # durations that sum to 0, to a NaN, beyond 1e4
        dd = np.array(durs)
        assert L.topay_track_set(emu.h, 51, 1, api._dp(s3), 2, api._dp(dd), api._dp(c.reshape(-1))) == -1
    assert emu.track_get(51, 1) is None                       # nothing of the refused calls was stored
    big_d, big_c = _quintic([0.1] * 171)                      # more than 170 pieces
    assert L.topay_track_set(emu.h, 51, 1, api._dp(s3), 171, api._dp(big_d), api._dp(big_c.reshape(-1))) == -1
    ok_d, ok_c = _quintic([0.1] * 170)
    emu.track_set(51, 1, s3, ok_d, ok_c)
    assert emu.track_safe([51], [25])[0][0]
    with pytest.raises(api.TopayError, match="named twice"):  # one robot slot twice in a cycle: two commits into one block
        emu.replan_calls([50, 50], [25, 25], 0.1, 0.1, np.zeros((2, 10)), 1e9, 0.1, 3.0)
    nomap = np.array([230], dtype=np.int32)                   # a map slot without fields
    assert L.topay_track_safe(emu.h, 1, api._ip(one), api._ip(nomap), None, None, None) == -3            # TOPAY_ERR_NO_MAP
    assert L.topay_track_safe(emu.h, 1, api._ip(one), api._ip(m25), None, None, None) == 0


def _lib_exports(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\sT\s+(topay_[a-z0-9_]+)", out))


def test_new_entries_are_declared_and_exported():
    import __graft_entry__ as entry
    entry.build_hip()
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    declared = set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M))
    hip, em = api.load(), api.load(EMU_LIB)
    for n in NEW_ENTRIES:
        assert n in declared, n
        assert hasattr(hip, n), f"{n} not exported by the HIP library"
        assert hasattr(em, n), f"{n} not exported by the emulator library"


# ---------------------------------------------------------------------------------------------------------------------
# the cycle
# ---------------------------------------------------------------------------------------------------------------------
def _capped(lib_path=None, s1=40, s2=40, outer=2):
    L = api.load(lib_path)
    p = api.default_params(L)
    p.s1_lbfgs.max_iterations = s1
    p.s2_lbfgs.max_iterations = s2
    p.alm_max_outer = outer
    return api.MomaTrajOptBatch(params=p, device=0, lib_path=lib_path)


def _tracks(opt, robots):
    out = []
    for r in robots:
        out.append(tuple(opt.track_get(int(r), w) for w in (1, 2)))
    return out


def _same_track(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _blocked_world(w, ref_traj, frac=0.4):
    """The occupancy of world w with a 0.4 m box put on the tracked trajectory at the fraction frac of its duration (2-D and 3-D)."""
    st, _ = ref_traj.state(frac * ref_traj.T)
    nx, ny, nz = (int(v) for v in w.dims)
    o2 = np.array(w.occ2d, dtype=np.int8).reshape(nx, ny).copy()
    o3 = np.array(w.occ3d, dtype=np.int8).reshape(nx, ny, nz).copy()
    ix, iy = int((st[0] - w.origin[0]) / w.res), int((st[1] - w.origin[1]) / w.res)
    o2[max(ix - 2, 0):ix + 2, max(iy - 2, 0):iy + 2] = 1
    o3[max(ix - 2, 0):ix + 2, max(iy - 2, 0):iy + 2, :] = 1
    return o2.reshape(-1), o3.reshape(-1)


CYCLE_FRAC, CYCLE_HORIZON = 0.6, 3.0


def _cycle_setup(opt, n):
    """n robots on the maps of TablesBatch(4, 1, base_seed=2024): a capped plan_calls, winners committed as end_traj and
    global_traj; then an obstacle on robot 1's trajectory, in robot 1's map only."""
    tb = wl.TablesBatch(4, 1, base_seed=2024, nthreads=8)
    worlds = [tb.world(s_) for s_ in tb.scenarios]
    for k, w in enumerate(worlds):
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, w.occ3d, map_id=k)
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]
    start = np.array([tb.paths[offs[b]] for b in first])[:n]
    goal = np.array([tb.paths[offs[b + 1] - 1] for b in first])[:n]
    mid = np.arange(n, dtype=np.int32)
    robots = np.arange(100, 100 + n, dtype=np.int32)
    res, _, _ = opt.plan_calls(start, goal, map_ids=mid, first_call=40)
    done = opt.track_commit_plan(robots, np.arange(n), which=3)
    assert (done == (res[:, 0] == 1)).all()
    return dict(tb=tb, worlds=worlds, start=start, goal=goal, mid=mid, robots=robots, res=res, done=done)


def _block_robot(opt, S, r, frac=CYCLE_FRAC):
    w = S["worlds"][r]
    s3, d, c = opt.track_get(int(S["robots"][r]), 1)
    o2, o3 = _blocked_world(w, wl.ReplanTraj(s3, d, c), frac)
    opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, o2, o3, map_id=int(S["mid"][r]))


def _cycle_unsafe_robot(opt, S, base=500):
    """replan_calls with a long interval after robot 1's map got an obstacle: (status, endpoints, result, candidates, tracks)."""
    n = len(S["robots"])
    out = opt.replan_calls(S["robots"], S["mid"], np.full(n, 0.2), np.full(n, 0.2), S["goal"], 1e9, 0.1, CYCLE_HORIZON, first_call=base)
    return out + (_tracks(opt, S["robots"]),)


def test_replan_cycle():
    opt = _capped(EMU_LIB)
    S = _cycle_setup(opt, 3)
    n, robots, mid, goal = 3, S["robots"], S["mid"], S["goal"]
    assert S["done"].all(), "the capped planning call of the setup must give every robot a trajectory"
    before = _tracks(opt, robots)
    assert opt.track_safe(robots, mid)[0].all()
    _block_robot(opt, S, 1)
    assert list(opt.track_safe(robots, mid)[0]) == [True, False, True]
    ends1 = opt.replan_inputs(robots[1:2], 0.2, 0.2, goal[1:2], 0.1, CYCLE_HORIZON)
    status, ends, res, cand, after = _cycle_unsafe_robot(opt, S, base=500)
    print("status", status.tolist(), "result", res.tolist())
    assert (status[[0, 2], 0] == 0).all() and (status[[0, 2], 1] == 1).all() and (status[[0, 2], 2] == -1).all()
    for r in (0, 2):
        assert _same_track(after[r][0], before[r][0]) and _same_track(after[r][1], before[r][1])
        assert np.isnan(ends[r]).all()
    assert status[1, 0] == 1 and status[1, 1] == 0 and status[1, 2] == 0 and status[1, 3] == ends1[3][0]
    for k in range(3):
        assert (ends[1, k] == ends1[k][0]).all()
    assert _same_track(after[1][1], before[1][1])                                   # global_traj stays
    assert not _same_track(after[1][0], before[1][0])
    tr = opt.plan_trajs([status[1, 2]])                                             # the plan store after replan_calls
    assert (after[1][0][1] == tr["durations"]).all() and (after[1][0][2] == tr["coeffs"]).all()
    # the same call alone, numbered base + 1
    r1, c1, _ = opt.plan_calls(ends1[0], ends1[2], map_ids=mid[1:2], start_v=ends1[1], first_call=501)
    assert r1[0, 0] == 1 and (r1[0, :7] == res[1, :7]).all() and (c1[0] == cand[1]).all()
    tr = opt.plan_trajs([0])
    assert (after[1][0][1] == tr["durations"]).all() and (after[1][0][2] == tr["coeffs"]).all()
    assert (after[1][0][0] == opt.plan_front_path(0)[0, :3]).all()
    with pytest.raises(api.TopayError, match="named twice"):                        # one robot slot twice in a commit
        opt.track_commit_plan([robots[0], robots[0]], [0, 0], which=1)
    # a short interval: all three trigger, each equals its single call
    now = _tracks(opt, robots)
    endsA = opt.replan_inputs(robots, 0.2, 0.2, goal, 0.1, 3.0)
    st2, en2, res2, cand2 = opt.replan_calls(robots, mid, np.full(n, 0.2), np.full(n, 0.2), goal, 0.1, 0.1, 3.0, first_call=700)
    assert (st2[:, 0] == 1).all() and (st2[:, 2] == np.arange(n)).all()
    after2 = _tracks(opt, robots)
    for r in range(n):
        rr, cc, _ = opt.plan_calls(endsA[0][r:r + 1], endsA[2][r:r + 1], map_ids=mid[r:r + 1], start_v=endsA[1][r:r + 1], first_call=700 + r)
        assert rr[0, 0] == 1 and (rr[0, :7] == res2[r, :7]).all() and (cc[0] == cand2[r]).all(), r
        tr = opt.plan_trajs([0])
        assert (after2[r][0][1] == tr["durations"]).all() and (after2[r][0][2] == tr["coeffs"]).all() and not _same_track(after2[r][0], now[r][0])
    # a replan without a winner (the goal enclosed, as in tests/test_plan.py) keeps the old trajectory: status 2
    w = S["worlds"][0]
    e2d = np.asarray(w.esdf2d).reshape(int(w.dims[0]), int(w.dims[1]))
    ix, iy = np.unravel_index(int(np.argmin(e2d)), e2d.shape)
    bad = goal[:1].copy()
    bad[0, 0], bad[0, 1] = w.origin[0] + (ix + 0.5) * w.res, w.origin[1] + (iy + 0.5) * w.res
    opt.track_set(int(robots[0]), 2, *_short_global())       # a global_traj that ends before t_since_begin: the goal is global_goal
    keep = opt.track_get(int(robots[0]), 1)
    st3, _, res3, _ = opt.replan_calls(robots[:1], mid[:1], [0.2], [5.0], bad, 0.1, 0.1, 3.0, first_call=900)
    assert st3[0, 0] == 2 and st3[0, 3] == -1 and res3[0, 0] == 0 and _same_track(opt.track_get(int(robots[0]), 1), keep)
    # arrived: within 0.5 m of the global goal nothing is run
    st4, en4, res4, _ = opt.replan_calls(robots[:1], mid[:1], [0.2], [0.2], goal[:1], 0.1, 0.1, 3.0, now_xy=goal[:1, :2] + [[0.3, 0.0]], first_call=950)
    assert st4[0, 0] == 3 and st4[0, 2] == -1 and (res4 == 0).all() and np.isnan(en4).all()
    assert _same_track(opt.track_get(int(robots[0]), 1), keep)
    S["tb"].close()
    opt.close()


def _short_global():
    d, c = _quintic([0.5])
    return [0.0, 0.0, 0.0], d, c


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    opt = api.MomaTrajOptBatch(device=0)
    yield opt
    opt.close()


@pytest.mark.gpu
def test_sweeps_and_endpoints_on_gpu_equal_emulator(dev, emu):
    """Issue sections 2 to 4 on the device: every output equals the emulator's bit for bit (and so passes the checks against the
    restatement that the emulator passes)."""
    a, b = _sweep_cases(dev), _sweep_cases(emu)
    assert _check_sweeps(a)
    for (na, da, _), (nb, db, _) in zip(a, b):
        assert na == nb and np.array_equal(np.array(da, dtype=np.float64), np.array(db, dtype=np.float64), equal_nan=True), (na, da, db)
    (ca, E, gg), (cb, _, _) = _endpoint_cases(dev), _endpoint_cases(emu)
    assert _check_endpoints(ca, E, gg)
    for (na, da, _), (nb, db, _) in zip(ca, cb):
        assert all((x == y).all() for x, y in zip(da[:3], db[:3])) and da[3] == db[3], na
    for x, y in zip(_map_change_case(dev), _map_change_case(emu)):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.gpu
def test_replan_cycle_gpu_equals_emulator():
    """The unsafe-robot case with 4 robots, capped solves: status, endpoints, plan tables and every tracked trajectory after the
    cycle are the emulator's bit for bit."""
    out = []
    for lib in (None, EMU_LIB):
        opt = _capped(lib)
        S = _cycle_setup(opt, 4)
        _block_robot(opt, S, 1)
        out.append(_cycle_unsafe_robot(opt, S, base=500))
        S["tb"].close()
        opt.close()
    a, b = out
    print("device status", a[0].tolist())
    assert a[0][1, 1] == 0 and a[0][1, 0] == 1 and (a[0][[0, 2, 3], 0] == 0).all()
    assert (a[0] == b[0]).all() and np.array_equal(a[1], b[1], equal_nan=True) and (a[2] == b[2]).all() and (a[3] == b[3]).all()
    for ta, tb_ in zip(a[4], b[4]):
        assert _same_track(ta[0], tb_[0]) and _same_track(ta[1], tb_[1])


# 256 trajectories of the planner against maps they were not planned on
MANY_SEED = 2024      # TablesBatch(64, 1, base_seed=2024), the scenarios of tests/test_plan.py


def _many_sweeps(opt):
    """Issue test 10.  One capped plan_calls over the 64 maps of TablesBatch(64, 1, base_seed=MANY_SEED); robot i of 256 tracks
    winner i % W (W winners: every winner on four slots or more).  Then the winners' maps are rebuilt, every second one with a
    box on its own winner's path, and robot i is swept against the rebuilt map of scenario (its own + 13 (i // W)) % 64: its
    own map with or without the box, or another scenario's tables.  Returns (W, device outputs [256], restatement outputs [256])."""
    tb = wl.TablesBatch(64, 1, base_seed=MANY_SEED, nthreads=8, keep_esdf3d=0)
    worlds = [tb.world(s_) for s_ in tb.scenarios]
    w0 = worlds[0]
    for k, w in enumerate(worlds):
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, w.occ3d, map_id=k)
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]
    start = np.array([tb.paths[offs[b]] for b in first])
    goal = np.array([tb.paths[offs[b + 1] - 1] for b in first])
    res, _, _ = opt.plan_calls(start, goal, map_ids=np.arange(64, dtype=np.int32), first_call=0)
    win = np.nonzero(res[:, 0] == 1)[0]
    W = len(win)
    assert W >= 32, "the capped planning call must give at least half of the scenarios a trajectory"
    robots = np.arange(1000, 1256, dtype=np.int32)
    call = win[np.arange(256) % W]
    assert opt.track_commit_plan(robots, call, which=1).all()
    refs = {int(c): wl.ReplanTraj(*opt.track_get(int(robots[k]), 1)) for k, c in enumerate(win)}
    for k, c in enumerate(win):                              # every second winner's map gets the box, the others stay: safe robots
        w = worlds[c]
        o2, o3 = _blocked_world(w, refs[int(c)]) if k % 2 else (w.occ2d, w.occ3d)
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, o2, o3, map_id=int(c))
    mid = ((call + 13 * (np.arange(256) // W)) % 64).astype(np.int32)
    safe, fh, hit = opt.track_safe(robots, mid)
    fields = {}
    for m in set(mid.tolist()):
        e2, e3, _ = opt.get_map(m)
        fields[m] = (e2, e3)
    dev, ref = [], []
    for i in range(256):
        dev.append((bool(safe[i]), int(fh[i, 0]), int(fh[i, 1]), float(hit[i, 0]), float(hit[i, 1])))
        ref.append(refs[int(call[i])].safe(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, *fields[int(mid[i])]))
    tb.close()
    return W, dev, ref


def _check_many(W, dev, ref):
    inside = [i for i in range(256) if ref[i]["min_margin"] >= MARGIN]
    unsafe = [i for i in inside if not ref[i]["safe"]]
    print(f"{W} winners; {256 - len(inside)} of 256 robots outside the precondition; unsafe {len(unsafe)}, "
          f"bodies {sorted(set(ref[i]['body'] for i in unsafe))}, samples {min(ref[i]['sample'] for i in unsafe)} .. {max(ref[i]['sample'] for i in unsafe)}")
    assert 256 - len(inside) <= 5, "more than 2 % of the robots outside the precondition: not a case for this seed"     # 5 / 256 < 2 %
    # the cases are what they are meant to be (conditions on the restatement): both verdicts, chassis and arm as first body,
    # first hits beyond the first pass of 64 samples
    assert len(unsafe) >= 64 and len(inside) - len(unsafe) >= 8
    assert any(ref[i]["body"] == 0 for i in unsafe) and any(ref[i]["body"] >= 1 for i in unsafe) and any(ref[i]["sample"] >= 64 for i in unsafe)
    for i in inside:
        d, r = dev[i], ref[i]
        assert d[0] == r["safe"] and d[1] == r["sample"] and d[2] == r["body"], (i, d, r)
        if not r["safe"]:
            assert abs(d[3] - r["t"]) <= TOL and abs(d[4] - r["d"]) <= TOL, (i, d, r)
    return True


@pytest.mark.gpu
def test_256_planned_trajectories_swept_on_gpu():
    """256 tracked trajectories of the planner (many pieces, many passes of 64 samples) against rebuilt maps: verdict, sample
    and body equal the restatement's for every robot whose restatement margin is 1e-6 or more; time and distance to 1e-11.
    Seed: MANY_SEED = 2024.  For it the restatement finds 57 winners and 0 of the 256 robots outside the precondition (227
    unsafe with the chassis and spheres 5 to 12 as first bodies, first hits at samples 0 to 1086, and 29 safe);
    _check_many allows 5 (below 2 %) and asserts the share on the restatement."""
    opt = _capped(None)
    W, dev, ref = _many_sweeps(opt)
    opt.close()
    assert _check_many(W, dev, ref)
