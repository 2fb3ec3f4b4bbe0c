"""topay_track_sample / topay_track_sample_grid: tracked trajectories sampled on the device (states, rates, end-effector
poses, sphere centres, distances and clearances of n robots at many times each).

Every yardstick is an entry that existed before these: topay_replan_inputs (getState / getDState), topay_playback, topay_ee_pose,
topay_track_safe, topay_get_map.  All comparisons are bit for bit, except the one restatement on the host in
test_centres_reproduce_the_distances, whose bound is derived there.  One set of case builders runs on the lane emulator in the
CPU suite and through the HIP library under -m gpu.
"""
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB
from topay_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["topay_track_sample", "topay_track_sample_grid", "topay_track_sample_ms"]
S, D, E, CL, CE, DI = api.SAMPLE_STATE, api.SAMPLE_DSTATE, api.SAMPLE_EE_POSE, api.SAMPLE_CLEARANCE, api.SAMPLE_CENTRES, api.SAMPLE_DISTANCE
ALL = S | D | E | CL | CE | DI

# ---------------------------------------------------------------------------------------------------------------------
# hand-made trajectories and maps (the helpers of tests/test_replan.py, copied)
# ---------------------------------------------------------------------------------------------------------------------
ORIGIN, RES, DIMS = np.array([-4.0, -4.0, 0.0]), 0.1, np.array([80, 80, 20], dtype=np.int32)
MIN_B, MAX_B = ORIGIN.copy(), ORIGIN + DIMS * RES
BLOCK2D = (1.0, 1.3, -0.5, 0.5)
BLOCK3D = (1.0, 1.3, -0.5, 0.5, 0.6, 1.0)


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


def _total(durs):
    T = 0.0
    for d in durs:      # getTotalDuration's order
        T += d
    return T


# The issue's three trajectories: (robot slot, start3, durations, keywords of _quintic)
TRAJS = ((60, [0.3, -0.2, 0.0], [0.35], dict(v=0.8)),                                              # ends inside a panel, T < 4 steps of car_seq
         (61, [-0.5, 0.1, 0.2], [0.4, 0.27], dict(v=0.6, theta0=0.2)),                           # the boundary on a car_seq step
         (62, [-1.0, 0.5, 0.3], [0.7, 0.7, 0.7], dict(v=0.7, omega=0.4, theta0=0.3, qrate=0.05)))  # > 64 samples at 0.025 s
OTHER = ([0.8, 0.6], dict(v=0.9, omega=-0.2, qrate=-0.03))    # a different quintic, for the slot that holds two trajectories


def _set_trajs(opt):
    """Slots 60..62: the three trajectories as end_traj.  Slot 63: OTHER as end_traj and the third as global_traj."""
    for r, s3, durs, kw in TRAJS:
        d, c = _quintic(durs, **kw)
        opt.track_set(r, 1, s3, d, c)
    d, c = _quintic(OTHER[0], **OTHER[1])
    opt.track_set(63, 1, TRAJS[2][1], d, c)
    d, c = _quintic(TRAJS[2][2], **TRAJS[2][3])
    opt.track_set(63, 2, TRAJS[2][1], d, c)


def _case_times(durs):
    T, b = _total(durs), durs[0]
    return np.array([-0.5, 0.0, 1e-300, 0.025, 0.1, b, np.nextafter(b, 0.0), np.nextafter(b, np.inf), T, np.nextafter(T, 0.0), T + 3.0])


def _by_replan_inputs(opt, robots, times):
    """getState / getDState of robot robots[k] at times[k] through the existing entry: t_since_replan = t, planning_budget = 0.
    (The entry takes a slot any number of times, one wave each.)"""
    n = len(robots)
    st, sv, _, _ = opt.replan_inputs(robots, np.asarray(times, dtype=np.float64), 0.0, np.zeros((n, 10)), 0.0, 1e9)
    return st, sv


def _flat(robots, times):
    return np.concatenate([np.full(len(t), r, dtype=np.int32) for r, t in zip(robots, times)]), np.concatenate(times)


# ---------------------------------------------------------------------------------------------------------------------
# case builders: what the sampling entries return, and the yardstick beside it
# ---------------------------------------------------------------------------------------------------------------------
def _case_states(opt):
    """Test 1.  (name, sampled, yardstick) triples of arrays that must be equal."""
    _set_trajs(opt)
    out = []
    robots = [r for r, _, _, _ in TRAJS]
    times = [_case_times(durs) for _, _, durs, _ in TRAJS]
    got = opt.track_sample(robots, times, what=S | D)
    fr, ft = _flat(robots, times)
    st, sv = _by_replan_inputs(opt, fr, ft)
    out += [("case times: state", got["state"], st), ("case times: dstate", got["dstate"], sv)]
    out.append(("duration", got["duration"], np.array([_total(durs) for _, _, durs, _ in TRAJS])))
    # 1, 63, 64, 65, 130 samples and a robot without any between two with samples: the work table
    T3 = _total(TRAJS[2][2])
    robots = [62, 61, 62, 60, 62, 61, 62]
    times = [np.array([0.3]), np.linspace(-0.1, 0.8, 63), np.linspace(0.0, T3, 64), np.zeros(0), np.linspace(-0.2, T3 + 0.2, 65), np.linspace(0.0, 0.67, 130),
             np.array([1.0, 2.0])]
    got = opt.track_sample(robots, times, what=S | D)
    fr, ft = _flat(robots, times)
    st, sv = _by_replan_inputs(opt, fr, ft)
    out += [("block counts: state", got["state"], st), ("block counts: dstate", got["dstate"], sv)]
    # which = 2: global_traj of slot 63 is the quintic that slot 62 holds as end_traj; its end_traj is another one
    t = [np.linspace(-0.1, T3 + 0.1, 70)]
    g2, e62, e63 = (opt.track_sample([r], t, which=w, what=S | D) for r, w in ((63, 2), (62, 1), (63, 1)))
    out += [("which = 2: state", g2["state"], e62["state"]), ("which = 2: dstate", g2["dstate"], e62["dstate"]), ("which = 2: duration", g2["duration"], e62["duration"])]
    assert not (e63["state"] == e62["state"]).all() and e63["duration"][0] != e62["duration"][0]   # (the slot's end_traj really is another one)
    st, sv = _by_replan_inputs(opt, np.full(70, 63, dtype=np.int32), t[0])
    out += [("slot 63 end_traj: state", e63["state"], st), ("slot 63 end_traj: dstate", e63["dstate"], sv)]
    return out


def _case_ee(opt):
    """Test 3: ee_pose against topay_ee_pose of the returned states."""
    _set_trajs(opt)
    robots = [60, 61, 62]
    times = [_case_times(durs) for _, _, durs, _ in TRAJS]
    times[2] = np.concatenate([times[2], np.linspace(0.0, 2.1, 66)])
    got = opt.track_sample(robots, times, what=S | E)
    only = opt.track_sample(robots, times, what=E)               # without the state output: the same poses
    return [("ee_pose", got["ee_pose"], opt.ee_pose(got["state"])), ("ee_pose alone", only["ee_pose"], got["ee_pose"])]


def _radii(opt):
    """r_body: the chassis radius, then the radii of the 12 spheres (the entries of colli_points that are not zero)."""
    p = opt.opt_param
    r = [p.chassis_colli_radius] + [p.colli_point_radius[i] for i in range(16) if p.colli_points[i] != 0.0]
    assert len(r) == 13
    return np.array(r)


def _grid_times(t0, step, m):
    out, t = np.zeros(m), np.float64(t0)
    for j in range(m):      # the running sum of the reference's loops
        out[j] = t
        t = t + np.float64(step)
    return out


# (name, robot slot, start3, durations, map slot): the shapes and maps of test_replan._sweep_cases
SWEEPS = (("5 samples / free", 70, [0.62, 0.0, 0.0], [0.05], 10),
          ("68 samples / block2d", 71, [0.0, 0.0, 0.0], [0.675], 11),
          ("3 pieces / block2d", 72, [-0.75, 0.0, 0.0], [0.5, 0.5, 0.5], 11),
          ("arm into the block / block3d", 73, [0.2, 0.0, 0.0], [1.0], 12),
          ("arm into the block / block2d", 73, [0.2, 0.0, 0.0], [1.0], 11),
          ("leaves the map / block3d", 74, [3.0, 0.0, 0.0], [1.0, 1.0], 12))


def _case_clearance(opt):
    """Test 4: per sweep case (name, sweep outputs, T, grid outputs)."""
    fields = {10: _build(opt, 10), 11: _build(opt, 11, block2d=BLOCK2D), 12: _build(opt, 12, block3d=BLOCK3D)}
    out = []
    for name, r, s3, durs, slot in SWEEPS:
        d, c = _quintic(durs)
        opt.track_set(r, 1, s3, d, c)
        T = _total(durs)
        m = int(np.ceil(T / 0.01)) + 2
        safe, fh, hit = opt.track_safe([r], [slot])
        got = opt.track_sample_grid([r], 0.0, 0.01, m, map_ids=[slot], what=S | CL | CE | DI)
        out.append((name, (bool(safe[0]), fh[0].copy(), hit[0].copy()), T, got))
    return out, fields


def _check_clearance(opt, cases):
    rb = _radii(opt)
    seen = {}
    for name, (safe, fh, hit), T, got in cases:
        m = len(got["distance"])
        t = _grid_times(0.0, 0.01, m)
        keep = t < T                                              # the sweep's samples
        assert keep[0] and not keep[-1], name                     # (m reaches past T)
        dist, cl = got["distance"], got["clearance"]
        # the sweep's comparison as k_track_safe states it: d < r * 0.99 ...
        viol = (dist < rb[None, :] * 0.99) & keep[:, None]
        # ... and as the issue states it on the margins: the same verdicts (the subtraction is exact near the threshold)
        assert (((cl + rb[None, :]) < 0.99 * rb[None, :]) & keep[:, None] == viol).all(), name
        assert safe == (not viol.any()), name
        if safe:
            assert (fh == -1).all() and np.isnan(hit).all(), name
        else:
            s = int(np.argmax(viol.any(axis=1)))
            b = int(np.argmax(viol[s]))                           # chassis, then the spheres in order
            assert fh[0] == s and fh[1] == b, (name, fh, s, b)
            assert hit[0] == t[s] and hit[1] == dist[s, b], (name, hit, t[s], dist[s, b])
            if 0.5 * rb[b] <= hit[1] <= 2.0 * rb[b]:              # d - r exact (Sterbenz): the addition undoes it
                assert cl[s, b] + rb[b] == hit[1], name
        out_of_map = dist == 1e10
        assert (cl == dist - rb[None, :]).all(), name               # the one expression
        assert (cl[out_of_map] == (1e10 - np.broadcast_to(rb, cl.shape))[out_of_map]).all(), name
        seen[name] = (safe, None if safe else int(fh[1]), int(fh[0]), out_of_map)
    # the cases are what they are meant to be
    assert seen["5 samples / free"][0] and seen["leaves the map / block3d"][0]
    assert seen["68 samples / block2d"][1] == 0 and seen["68 samples / block2d"][2] >= 64        # the chassis, in the second block
    assert seen["3 pieces / block2d"][1] == 0 and seen["arm into the block / block2d"][1] == 0
    assert seen["arm into the block / block3d"][1] >= 1                                           # a sphere only
    oom = seen["leaves the map / block3d"][3]
    assert oom[:, 0].any() and oom[:, 1:].any() and not oom.all()                                 # leaves it on the way
    return True


def _case_grid(opt):
    """Test 6: the grid entry against the ragged entry at the numpy running sums."""
    _set_trajs(opt)
    robots, t0, step = [60, 61, 62], np.array([-0.05, 0.0, 0.3]), 0.025
    out = []
    for m in (1, 64, 65):
        g = opt.track_sample_grid(robots, t0, step, m, what=S | D | E | CE)
        r = opt.track_sample(robots, [_grid_times(a, step, m) for a in t0], what=S | D | E | CE)
        out += [(f"m = {m}: {k}", g[k], r[k]) for k in ("state", "dstate", "ee_pose", "centres", "duration")]
    return out


def _equal(pairs):
    for name, a, b in pairs:
        assert a.shape == b.shape and (a == b).all(), (name, np.argwhere(a != b)[:4])
    return True


@pytest.fixture(scope="module")
def emu():
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    yield opt
    opt.close()


@pytest.fixture(scope="module")
def solved(cuboids_small):
    """The construction of test_replan.test_tracked_playback_equals_batch_playback: a capped emulator solve, candidate 0 set
    into slot 7.  (opt, durations, T)"""
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
    opt.track_set(7, 1, cs["paths"][0][:3], dur, co)
    yield opt, dur, opt.total_durations()[0]
    opt.close()


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite (lane emulator)
# ---------------------------------------------------------------------------------------------------------------------
def test_state_and_rate_equal_replan_inputs(emu):
    """Test 1: state / dstate equal start / start_v of topay_replan_inputs at every case time (clamps included), for 1, 63,
    64, 65 and 130 samples and an empty range, for which = 1 and which = 2."""
    assert _equal(_case_states(emu))


def test_states_equal_batch_playback(solved):
    """Test 2: the states of a solved candidate set into a slot equal topay_playback of the candidate."""
    opt, dur, T = solved
    times = np.concatenate([[-0.3, 0.0, dur[0], T, T + 2.0], np.linspace(0, T, 41)])
    pb, _ = opt.playback(0, times)
    got = opt.track_sample([7], [times], what=S)
    assert (got["state"] == pb).all() and got["duration"][0] == T


def test_ee_pose_equals_ee_pose_of_the_states(emu):
    assert _equal(_case_ee(emu))


def test_clearance_against_the_sweep(emu):
    """Test 4: the sweep's verdict, first hit and distance follow from the grid t0 = 0, step = 0.01 of distances / clearances."""
    cases, _ = _case_clearance(emu)
    assert _check_clearance(emu, cases)


def _host_distance3d(e3, p):
    """GridMap::getDistance3d as harness/workload.hpp states it (trilinear, the clamped neighbours, no fused operations) at
    points p [n, 3] inside the map."""
    e = e3.reshape(DIMS)
    idx, diff = np.zeros((len(p), 3), dtype=np.int64), np.zeros((len(p), 3))
    for a in range(3):
        pm = p[:, a] - 0.5 * RES
        idx[:, a] = np.floor((pm - ORIGIN[a]) * (1.0 / RES)).astype(np.int64)
        diff[:, a] = (p[:, a] - ((idx[:, a] + 0.5) * RES + ORIGIN[a])) * (1.0 / RES)
    bnd = lambda i, a: np.clip(i, 0, DIMS[a] - 1)
    v = lambda x, y, z: e[bnd(idx[:, 0] + x, 0), bnd(idx[:, 1] + y, 1), bnd(idx[:, 2] + z, 2)]
    dx, dy, dz = diff.T
    v00, v01 = v(0, 0, 0) * (1 - dx) + v(1, 0, 0) * dx, v(0, 0, 1) * (1 - dx) + v(1, 0, 1) * dx
    v10, v11 = v(0, 1, 0) * (1 - dx) + v(1, 1, 0) * dx, v(0, 1, 1) * (1 - dx) + v(1, 1, 1) * dx
    v0, v1 = v00 * (1 - dy) + v10 * dy, v01 * (1 - dy) + v11 * dy
    return v0 * (1.0 - dz) + v1 * dz


def test_centres_reproduce_the_distances(emu):
    """Test 5.  No existing entry returns sphere centres, so the issue's second yardstick: getDistance3d lookups of `centres` on
    the fields of topay_get_map reproduce distance[:, 1:] (and clearance[:, 1:] + r).  The lookup on the host is the harness's
    (harness/workload.hpp, GridMap::getDistance3d): trilinear, plain products and sums, where the device's esdf3d_query fuses
    each interpolation step into one fma.  Bound: the result is a convex combination of 8 field values |v| <= V through 3
    nested steps a (1 - d) + b d with d in [0, 1); a step of either form rounds at most 4 times (1 - d, two products, the sum),
    each by at most 2^-53 of a quantity <= V, and the steps above pass an error on with weights that sum to 1.  So either form
    is within 3 x 4 x 2^-53 V of the exact value and the two within 24 x 2^-53 V < 2^-48 V of each other.  Used: 2^-48 max|field|.
    clearance + r rounds twice more, by at most 2^-53 (V + r) each, r < 1."""
    cases, fields = _case_clearance(emu)
    rb = _radii(emu)
    checked = 0
    for (name, _, _, got), (_, _, _, _, slot) in zip(cases, SWEEPS):
        ce, dist = got["centres"], got["distance"]
        assert ce.shape == (len(dist), 12, 3)
        e3 = fields[slot][1]
        V = np.abs(e3).max()
        bound = 2.0 ** -48 * V
        inside = dist[:, 1:] != 1e10
        pts = ce[inside]
        lo, hi = MIN_B + 1e-4, MAX_B - 1e-4
        assert ((pts >= lo) & (pts <= hi)).all(), name            # 1e10 exactly where a centre is outside, and only there
        assert not ((ce[~inside] >= lo) & (ce[~inside] <= hi)).all(axis=1).any(), name
        ref = _host_distance3d(e3, pts)
        err = np.abs(dist[:, 1:][inside] - ref).max()
        print(name, "largest difference to the host lookup", err, "bound", bound)
        assert err <= bound, name
        assert np.abs(got["clearance"][:, 1:][inside] + np.broadcast_to(rb[1:], inside.shape)[inside] - ref).max() <= bound + 2.0 ** -52 * (V + 1.0), name
        # the first sphere sits on the arm's first link: a centre is a point of the robot, in the world frame
        assert np.abs(ce[:, 0, :2] - got["state"][:, :2]).max() < 0.5, name
        checked += len(pts)
    assert checked > 1000


def test_grid_equals_ragged(emu):
    assert _equal(_case_grid(emu))


def _raw_sample(opt, robots, times, what, bufs, which=1, map_ids=None):
    """topay_track_sample with the caller's seven buffers (state, dstate, ee_pose, clearance, centres, duration, distance)."""
    rb = np.array(robots, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in times])]).astype(np.int32)
    flat = np.ascontiguousarray(np.concatenate(times), dtype=np.float64)
    mid = None if map_ids is None else np.array(map_ids, dtype=np.int32)
    return opt.L.topay_track_sample(opt.h, len(rb), api._ip(rb), which, api._ip(mid), api._ip(off), api._dp(flat), what,
                                    *[None if b is None else b.ctypes.data for b in bufs])


def test_selection_and_independence(emu, solved):
    _set_trajs(emu)
    _build(emu, 10)
    times = [np.linspace(-0.1, 2.3, 70)]
    M, SENT = 70, 777.0
    shapes = ((M, 10), (M, 10), (M, 9), (M, 13), (M, 12, 3), (1,), (M, 13))
    # what = STATE alone: nothing else is written, although every pointer is given
    bufs = [np.full(s, SENT) for s in shapes]
    assert _raw_sample(emu, [62], times, S, bufs, map_ids=[10]) == 0
    assert (bufs[0] != SENT).all() and bufs[5][0] == _total(TRAJS[2][2])
    assert all((bufs[k] == SENT).all() for k in (1, 2, 3, 4, 6))
    # a NULL pointer with its bit set: the others are written as before
    full = emu.track_sample([62], times, map_ids=[10], what=ALL)
    assert (full["state"] == bufs[0]).all()
    some = [np.full(s, SENT) for s in shapes]
    some[0] = some[3] = None
    assert _raw_sample(emu, [62], times, ALL, some, map_ids=[10]) == 0
    for k, name in ((1, "dstate"), (2, "ee_pose"), (4, "centres"), (6, "distance")):
        assert (some[k] == full[name]).all(), name
    # robot A alone, beside B and C, named twice
    tb, tc = np.linspace(0.0, 0.7, 9), np.linspace(0.0, 0.4, 130)
    abc = emu.track_sample([61, 62, 60], [tb, times[0], tc], map_ids=[10, 10, 10], what=ALL)
    twice = emu.track_sample([62, 61, 62], [times[0], tb, times[0]], map_ids=[10, 10, 10], what=ALL)
    for name, _, _ in api.SAMPLE_OUTPUTS:
        assert (abc[name][9:9 + M] == full[name]).all(), name
        assert (twice[name][:M] == full[name]).all() and (twice[name][M + 9:] == full[name]).all(), name
    assert abc["duration"][1] == twice["duration"][0] == twice["duration"][2] == full["duration"][0]
    # the context is as it was: tracked trajectories, the sweep, the resident batch
    opt, dur, T = solved
    _build(opt, 10)
    n = opt.batch
    def snapshot():
        succ, cost, npc = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n, dtype=np.int32)
        assert opt.L.topay_get_batch(opt.h, api._ip(succ), api._dp(cost), api._ip(npc)) == 0
        return opt.track_get(7, 1) + opt.track_safe([7], [10]) + (succ, cost, npc, opt.get_x(0))
    before = snapshot()
    opt.track_sample([7, 7], [np.linspace(0, T, 130), np.array([0.5])], map_ids=[10, 10], what=ALL)
    opt.track_sample_grid([7], 0.0, 0.01, 70, map_ids=[10], what=ALL)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b, equal_nan=True)
    assert opt.track_sample_ms() >= 0.0


def test_refusals(emu):
    _set_trajs(emu)
    _build(emu, 10)
    t = [np.array([0.1, 0.2])]
    none = [None] * 7
    st = [np.zeros((2, 10))] + [None] * 6
    L, h = emu.L, emu.h
    ok = lambda **kw: _raw_sample(emu, kw.pop("robots", [62]), kw.pop("times", t), kw.pop("what", S), kw.pop("bufs", st), **kw)
    assert ok() == 0
    assert ok(robots=[65]) == -4                                                     # TOPAY_ERR_NO_TRAJ: an empty slot
    assert ok(robots=[62], which=2) == -4                                            # ... a slot without a global_traj
    with pytest.raises(api.TopayError, match="no global_traj"):
        emu.track_sample([62], t, which=2)
    assert ok(what=CL, map_ids=[230]) == -3                                          # TOPAY_ERR_NO_MAP: CLEARANCE, the slot is not set
    assert ok(what=S | CE, map_ids=[230]) == 0                                       # centres need no map
    assert ok(what=S | CE) == 0
    assert ok(what=CL) == -1                                                         # CLEARANCE with map_ids = NULL
    with pytest.raises(api.TopayError, match="need map_ids"):
        emu.track_sample([62], t, what=CL)
    one, off, tt = np.array([62], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([0.1, 0.2])
    call = lambda n=1, which=1, off=off, tt=tt, what=S: L.topay_track_sample(h, n, api._ip(one), which, None, api._ip(off), api._dp(tt), what, st[0].ctypes.data, *none[1:])
    assert call() == 0
    assert call(n=0) == -1 and call(n=-1) == -1                                      # n <= 0
    assert call(which=0) == -1 and call(which=3) == -1                               # which outside 1..2
    assert call(what=0) == -1 and call(what=64) == -1                                # what == 0 (and a bit that does not exist)
    two, off3 = np.array([62, 61], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32)
    assert L.topay_track_sample(h, 2, api._ip(two), 1, None, api._ip(off3), api._dp(tt), S, st[0].ctypes.data, *none[1:]) == -1   # offsets that decrease
    for bad in (np.nan, np.inf, -np.inf):                                            # a time that is not finite
        assert call(tt=np.array([0.1, bad])) == -1
    t0 = np.array([0.0])
    grid = lambda t0=t0, step=0.01, m=2, what=S: L.topay_track_sample_grid(h, 1, api._ip(one), 1, None, api._dp(t0), step, m, what, st[0].ctypes.data, *none[1:])
    assert grid() == 0 and grid(m=0) == 0
    assert grid(step=np.nan) == -1 and grid(step=np.inf) == -1                       # step not finite
    assert grid(m=-1) == -1                                                          # m < 0
    assert grid(t0=np.array([np.nan])) == -1
    assert grid(what=0) == -1 and grid(what=CL) == -1
    out_of_range = np.array([4096], dtype=np.int32)
    assert L.topay_track_sample(h, 1, api._ip(out_of_range), 1, None, api._ip(off), api._dp(tt), S, st[0].ctypes.data, *none[1:]) == -1


def _lib_exports(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\sT\s+(topay_[a-z0-9_]+)", out))


def test_sampling_entries_are_declared_and_exported():
    import __graft_entry__ as entry
    entry.build_hip()
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    declared = set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M))
    hip, em = _lib_exports(api.DEFAULT_LIB), _lib_exports(EMU_LIB)
    for n in NEW_ENTRIES:
        assert n in declared, n
        assert n in hip, f"{n} not exported by the HIP library"
        assert n in em, f"{n} not exported by the emulator library"
    for name in ("STATE", "DSTATE", "EE_POSE", "CLEARANCE", "CENTRES", "DISTANCE"):
        m = re.search(rf"TOPAY_SAMPLE_{name} = (\d+)", text)
        assert m and int(m.group(1)) == getattr(api, "SAMPLE_" + name), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    opt = api.MomaTrajOptBatch(device=0)
    yield opt
    opt.close()


@pytest.mark.gpu
def test_cases_on_gpu_equal_emulator(dev, emu):
    """The case builders of tests 1, 3, 4 and 6 through the HIP library: they pass their checks, and every array equals the
    emulator's bit for bit."""
    for build in (_case_states, _case_ee, _case_grid):
        a, b = build(dev), build(emu)
        assert _equal(a)
        for (na, xa, _), (nb, xb, _) in zip(a, b):
            assert na == nb and xa.shape == xb.shape and (xa == xb).all(), na
    (ca, _), (cb, _) = _case_clearance(dev), _case_clearance(emu)
    assert _check_clearance(dev, ca)
    for (na, sa, _, ga), (nb, sb, _, gb) in zip(ca, cb):
        assert sa[0] == sb[0] and (sa[1] == sb[1]).all() and np.array_equal(sa[2], sb[2], equal_nan=True), na
        for k in ga:
            assert (ga[k] == gb[k]).all(), (na, k)


_TENSOR_CHILD = r"""
import sys
import numpy as np
import torch                              # first: the library then binds to the HIP runtime that torch has loaded
cuda = torch.device("cuda", 0)
torch.zeros(1, device=cuda)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_track_sample as T
from topay_amd import api
ALL, S, CL = T.ALL, T.S, T.CL
dev = api.MomaTrajOptBatch(device=0)
T._set_trajs(dev)
T._build(dev, 10)
robots, times = [62, 60, 61], [np.linspace(-0.1, 2.3, 130), np.zeros(0), np.linspace(0.0, 0.7, 65)]
host = dev.track_sample(robots, times, map_ids=[10, 10, 10], what=ALL)
M = 195
out = {name: torch.full((M,) + tail, 777.0, dtype=torch.float64, device=cuda) for name, _, tail in api.SAMPLE_OUTPUTS}
out["duration"] = torch.full((3,), 777.0, dtype=torch.float64, device=cuda)
got = dev.track_sample(robots, times, map_ids=[10, 10, 10], what=ALL, out=out)
for name in host:
    assert got[name] is out[name]
    assert (out[name].cpu().numpy() == host[name]).all(), name
# some outputs on the device, the others returned as arrays; the grid entry; a tensor that starts 8 bytes into its storage
hg = dev.track_sample_grid(robots, [0.0, 0.1, 0.2], 0.01, 65, map_ids=[10, 10, 10], what=S | CL)
part = {"clearance": torch.full((M * 13 + 1,), 777.0, dtype=torch.float64, device=cuda)[1:].view(M, 13)}
gg = dev.track_sample_grid(robots, [0.0, 0.1, 0.2], 0.01, 65, map_ids=[10, 10, 10], what=S | CL, out=part)
assert isinstance(gg["state"], np.ndarray) and (gg["state"] == hg["state"]).all()
assert (part["clearance"].cpu().numpy() == hg["clearance"]).all()
for bad in (torch.zeros((M, 13), dtype=torch.float32, device=cuda), torch.zeros((M + 1, 13), dtype=torch.float64, device=cuda),
            torch.zeros((M, 26), dtype=torch.float64, device=cuda)[:, ::2]):
    try:
        dev.track_sample_grid(robots, 0.0, 0.01, 65, map_ids=[10, 10, 10], what=CL, out={"clearance": bad})
    except ValueError:
        continue
    raise AssertionError("a tensor of the wrong type, shape or layout was accepted")
try:
    dev.track_sample_grid(robots, 0.0, 0.01, 65, what=S, out=part)               # an output that `what` does not select
except ValueError:
    pass
else:
    raise AssertionError("an output that what does not select was accepted")
dev.close()
print("TENSORS_OK")
"""


@pytest.mark.gpu
def test_device_tensors_as_outputs():
    """out=: torch tensors on the device are filled by the kernel and equal the host-pointer call; a wrong tensor is refused.
    In a process of its own, which is what the test is about: the tensors and the library must share one HIP runtime, so torch is
    imported before the library is loaded, and this process has loaded the library long ago."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "TENSORS_OK" in r.stdout


def _many(opt, robots_checked=None):
    """96 robots x 257 samples, every output: robot i tracks the quintic i % 3 of TRAJS from a start of its own, on the block3d
    map.  robots_checked: only these (the emulator's side)."""
    _build(opt, 12, block3d=BLOCK3D)
    idx = list(range(96)) if robots_checked is None else list(robots_checked)
    for i in idx:
        _, s3, durs, kw = TRAJS[i % 3]
        d, c = _quintic(durs, **kw)
        opt.track_set(200 + i, 1, [s3[0] + 0.02 * i, s3[1] - 0.01 * i, s3[2] + 0.01 * i], d, c)
    robots = [200 + i for i in idx]
    t0 = np.array([-0.05 + 0.001 * i for i in idx])
    return opt.track_sample_grid(robots, t0, 0.01, 257, map_ids=[12] * len(idx), what=ALL)


@pytest.mark.gpu
def test_many_robots_on_gpu(dev, emu):
    """The work table at 96 robots x 257 samples (5 items per robot, the last with one sample), every output; three of the robots
    against the emulator."""
    pick = (0, 47, 95)
    got, ref = _many(dev), _many(emu, pick)
    assert got["state"].shape == (96 * 257, 10) and np.isfinite(got["clearance"]).all()
    for name in ref:
        g = got[name].reshape((96, -1) + got[name].shape[1:]) if name != "duration" else got[name]
        r = ref[name].reshape((3, -1) + ref[name].shape[1:]) if name != "duration" else ref[name]
        for j, i in enumerate(pick):
            assert (g[i] == r[j]).all(), (name, i)
