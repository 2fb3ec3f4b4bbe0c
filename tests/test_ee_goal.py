"""End-effector goals: topay_ee_pose == MomaParam::getFKPose (moma_param.h:339-373), topay_ee_eval == one
MomaTrajOpt::eeCostCallback (moma_traj_opt.cpp:48-140, gradient assigned), topay_ee_goals == optimizeEE (5-46) for a batch,
topay_ee_select == seeds x targets into goals.

Checker: harness/ee_goal.hpp (wl.EeGoal), a serial CPU restatement with libm; getEEGrads in the reference's triple-loop form,
optimizeEE through the oracle's lbfgs_optimize.  The reference ships no vectors, so the restatement's gradient is pinned here
by central differences of its own cost.  CPU tests run the lane emulator; GPU tests compare the device with it bit for bit.
"""
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB
from harness import workload as wl
from topay_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["topay_ee_default_params", "topay_ee_pose", "topay_ee_eval", "topay_ee_goals", "topay_ee_ms", "topay_ee_select"]

# the 80 x 80 x 20 hand-made map of tests/test_replan.py
ORIGIN, RES, DIMS = np.array([-4.0, -4.0, 0.0]), 0.1, np.array([80, 80, 20], dtype=np.int32)
MIN_B, MAX_B = ORIGIN.copy(), ORIGIN + DIMS * RES
BLOCK_A = (0.2, 0.5, -0.2, 0.5, 0.5, 1.2)      # slot 1: a block the arm of a robot near the origin reaches
BLOCK_B = (-0.6, -0.3, -0.2, 0.5, 0.4, 1.0)    # slot 2: another block, on the other side
JMAX = np.array([3.1, 2.26, 3.1, 2.355, 3.1, 2.23, 6.28])   # moma_param.h:116
A = 0.7071068                                                # relative_R's literal (moma_param.h:123-125)
TOL_POSE = 1e-11
SUCCESS = (0, 1, 2, -1008)


def _occ(block3d=None):
    o2 = np.zeros((80, 80), dtype=np.int8)
    o3 = np.zeros((80, 80, 20), dtype=np.int8)
    o2[79, 79] = 1
    o3[79, 79, :] = 1
    c = lambda a, org: int(round((a - org) / RES))
    if block3d is not None:
        x0, x1, y0, y1, z0, z1 = block3d
        o3[c(x0, -4):c(x1, -4), c(y0, -4):c(y1, -4), c(z0, 0):c(z1, 0)] = 1
    return o2.reshape(-1), o3.reshape(-1)


def _maps(opt):
    """Slots 0 free, 1 block A, 2 block B; returns the restatements on the same fields."""
    refs = []
    for slot, blk in enumerate((None, BLOCK_A, BLOCK_B)):
        o2, o3 = _occ(blk)
        opt.build_esdf(ORIGIN, RES, DIMS, MIN_B, MAX_B, o2, o3, map_id=slot)
        e2, e3, _ = opt.get_map(slot)
        refs.append(wl.EeGoal(ORIGIN, RES, DIMS, MIN_B, MAX_B, e2, e3))
    return refs


def _inv_sigmoid(q):
    """invSigmoidC2 (moma_traj_opt.h:745-807) of the seven joints."""
    b = 0.5 * (JMAX + q) / JMAX
    T = b / (1 - b)
    return np.where(T > 1, np.sqrt(np.maximum(2 * T - 1, 0)) - 1, 1 - np.sqrt(np.maximum(2 / np.maximum(T, 1e-300) - 1, 0)))


def _unconstrained(state):
    s = np.asarray(state, dtype=np.float64)
    return np.concatenate([s[:3], _inv_sigmoid(s[3:])])


@pytest.fixture(scope="module")
def emu():
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    opt.ee_refs = _maps(opt)
    yield opt
    opt.close()


@pytest.fixture(scope="module")
def gpu():
    opt = api.MomaTrajOptBatch(device=0)
    opt.ee_refs = _maps(opt)
    yield opt
    opt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. getFKPose
# ---------------------------------------------------------------------------------------------------------------------
def test_ee_pose(emu):
    """Hand-worked from moma_param.h's constants (a = 0.7071068, h = chassis_height + relative_t.z = 0.171, the seven
    colli_length sum to 0.8505):
      zero state: the arm stands on (0, 0.115, h): position (0, 0.115, 1.0215), rotation relative_R: rows (a, a, 0), (-a, a, 0).
      q1 = pi/2 (even joint, about z): position unchanged, rotation relative_R Rz(pi/2): rows (a, -a, 0), (a, a, 0).
      q2 = pi/2 (odd joint, about y): links 0, 1 (0.139 + 0.1015) stay vertical, z = 0.171 + 0.2405 = 0.4115; the other five
        (0.61 m) lie along relative_R (1, 0, 0) = (a, -a, 0): position (0.61 a, 0.115 - 0.61 a, 0.4115); rotation
        relative_R Ry(pi/2): rows (0, a, a), (0, a, -a).
    Then 16 random states against the restatement to 1e-11 absolute (libm against the deterministic sin / cos, as
    tests/test_replan.py and tests/test_feasibility.py)."""
    st = np.zeros((3, 10))
    st[1, 3] = np.pi / 2
    st[2, 4] = np.pi / 2
    want = np.array([[0, 0.115, 1.0215, A, A, 0, -A, A, 0],
                     [0, 0.115, 1.0215, A, -A, 0, A, A, 0],
                     [0.61 * A, 0.115 - 0.61 * A, 0.4115, 0, A, A, 0, A, -A]])
    got = emu.ee_pose(st)
    assert np.abs(got - want).max() <= TOL_POSE, got - want
    rng = np.random.default_rng(11)
    rs = np.concatenate([rng.uniform(-3, 3, (16, 3)), rng.uniform(-1, 1, (16, 7)) * JMAX * 0.95], axis=1)
    err = np.abs(emu.ee_pose(rs) - wl.EeGoal.pose(rs)).max()
    print("pose against the restatement:", err)
    assert err <= TOL_POSE


# ---------------------------------------------------------------------------------------------------------------------
# 2. eeCostCallback
# ---------------------------------------------------------------------------------------------------------------------
# name -> (slot, state); ee_ref = getFKPose(state + 0.03)
EVAL_CASES = {
    "free": (0, [0, 0, 0, 0.3, 0.4, -0.2, 0.5, 0.1, -0.3, 0.2]),
    "near the block": (1, [0.1, 0, 0, 0.3, 0.4, -0.2, 0.5, 0.1, -0.3, 0.2]),
    "folded": (0, [0, 0, 0, 0.1, 2.2, 0.1, 2.3, 0.1, 0.3, 0.2]),
    "bent down": (0, [0, 0, 0, 0.1, 1.75, 0.1, 0.3, 0.1, 0.3, 0.2]),
    "outside": (0, [3.6, 0, 0.785, 0.05, 1.5, 0.05, 0.2, 0.1, 0.1, 0.2]),
}
KINK_PENALTY, KINK_CELL, KINK_SIGMOID = 2e-5, 2e-5, 1e-3   # see test_restatement_gradient_by_differences
FD_BOUND = 5e-7


def _eval_inputs():
    names = list(EVAL_CASES)
    slots = np.array([EVAL_CASES[k][0] for k in names], dtype=np.int32)
    st = np.array([EVAL_CASES[k][1] for k in names], dtype=np.float64)
    x = np.array([_unconstrained(s) for s in st])
    ref = wl.EeGoal.pose(st + 0.03)
    return names, slots, x, ref


def test_ee_eval_matches_restatement(emu):
    """f to 1e-11 relative, g to 1e-10 max|g| (the project's per-evaluation bar); every term active in one case and inactive
    in another, asserted on the restatement's breakdown."""
    names, slots, x, ref = _eval_inputs()
    f, g = emu.ee_eval(x, ref, slots)
    by = {}
    for k, name in enumerate(names):
        fr, gr, bd = emu.ee_refs[slots[k]].eval(x[k], ref[k])
        print(name, fr, abs(f[k] - fr) / abs(fr), np.abs(g[k] - gr).max() / np.abs(gr).max(), bd)
        assert abs(f[k] - fr) <= 1e-11 * abs(fr), name
        assert np.abs(g[k] - gr).max() <= 1e-10 * np.abs(gr).max(), name
        by[name] = bd
    assert by["free"]["n_mani"] == by["free"]["n_chassis"] == by["free"]["n_pairs"] == by["free"]["n_outside"] == 0
    assert by["near the block"]["n_mani"] > 0 and by["near the block"]["n_outside"] == 0 and by["near the block"]["n_pairs"] == 0
    assert by["folded"]["n_pairs"] > 0 and by["folded"]["n_mani"] == 0
    assert by["bent down"]["n_chassis"] > 0 and by["free"]["n_chassis"] == 0
    assert by["outside"]["n_outside"] >= 1 and by["outside"]["n_pairs"] == 0 and by["outside"]["n_chassis"] == 0


def test_restatement_gradient_by_differences(emu):
    """The pin of the restatement itself (CPU only): central differences of its f, h = 1e-6, against its g on the cases above.
    The cost is C2 across the penalty's joins (0 and relu_mu) but only C0 across the faces of the interpolation cells and
    of the in-map test, so each case is first moved (small deterministic steps) to a point whose distance from every such
    place is asserted: penalty arguments >= 2e-5 from 0 and relu_mu (h times the largest |d argument / dx| ~ 15), sphere centres
    >= 2e-5 m from a cell face (h times the largest |d centre / dx| ~ 1.2, with 10 x room), |Vq| >= 1e-3.
    Measured |fd - g| / max|g|: 1e-10 .. 3e-10 on four cases, 5.0e-8 on "outside", where f carries the constant ~90 of a sphere
    outside the map (d = 0) beside a gradient of ~0.2: the cancellation eps f / h ~ 1e-8 of the difference quotient, not the
    gradient.  The bound is 10 x the largest, 5e-7; a missing or mis-signed gradient term shows at 1e-2 and above."""
    names, slots, x, ref = _eval_inputs()
    h = 1e-6
    worst = 0.0
    for k, name in enumerate(names):
        R = emu.ee_refs[slots[k]]
        xk = None
        for t in range(200):   # move off the kinks
            cand = x[k] + 1.7e-4 * t * np.cos(np.arange(10) + 0.3 * t)
            bd = R.eval(cand, ref[k])[2]
            if bd["kink_penalty"] >= KINK_PENALTY and bd["kink_cell"] >= KINK_CELL and bd["kink_sigmoid"] >= KINK_SIGMOID:
                xk = cand
                break
        assert xk is not None, name
        f0, g0, bd = R.eval(xk, ref[k])
        assert bd["kink_penalty"] >= KINK_PENALTY and bd["kink_cell"] >= KINK_CELL and bd["kink_sigmoid"] >= KINK_SIGMOID
        fd = np.zeros(10)
        for i in range(10):
            e = np.zeros(10)
            e[i] = h
            fd[i] = (R.eval(xk + e, ref[k])[0] - R.eval(xk - e, ref[k])[0]) / (2 * h)
        rel = np.abs(fd - g0).max() / np.abs(g0).max()
        print(name, "fd rel", rel, bd)
        worst = max(worst, rel)
        assert rel <= FD_BOUND, (name, rel)
    print("largest central-difference deviation:", worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. solves
# ---------------------------------------------------------------------------------------------------------------------
N_SOLVE = 65
STATE_FLOOR, STATE_TOL = 6.1e-12, 6.1e-10   # measured in test_seed_offsets_keep_restatement_stable; 100 x the floor


def _problems():
    """65 problems ee_ref = getFKPose(s*), seed = s* + delta, |delta| <= 0.05.  In the first wave: problem 3 starts at s* (stop
    test met at iteration 0), odd problems sit on slot 1, problem 7 (slot 1) starts inside block A's clearance.
    Problem 7's offset is 0.03, not 0.05: from inside the penalty (f ~ 600, |g| ~ 1e3) the 0.05 seed is a solve the restatement
    cannot reproduce against ITSELF -- one ulp on seed coordinates other than the one test_solves_match_restatement probes moves
    its converged state by 0.036, into another minimum -- so it says nothing about an implementation.  The offsets are checked
    on the restatement alone in test_seed_offsets_keep_restatement_stable."""
    rng = np.random.default_rng(5)
    base = np.array([0, 0, 0, 0.3, 0.4, -0.2, 0.5, 0.1, -0.3, 0.2])
    star = base + np.concatenate([rng.uniform(-0.8, -0.3, (N_SOLVE, 1)), rng.uniform(-0.3, 0.3, (N_SOLVE, 9))], axis=1)
    slots = (np.arange(N_SOLVE) % 2).astype(np.int32)
    star[7, :3] = [0.1, 0.0, 0.0]
    star[7, 3:] = base[3:]
    seed = star + 0.05 * rng.uniform(-1, 1, (N_SOLVE, 10))
    seed[3] = star[3]
    seed[7] = star[7] + 0.6 * (seed[7] - star[7])
    return slots, seed, wl.EeGoal.pose(star)


def _solve_variants(opt, params=None):
    """The batch of 65, its prefixes of 63 and 64, and every problem alone: asserts bit equality, returns the batch."""
    slots, seed, ref = _problems()
    full = opt.ee_goals(seed, ref, slots, params)
    for n in (63, 64):
        part = opt.ee_goals(seed[:n], ref[:n], slots[:n], params)
        for a, b in zip(part, full):
            assert (a == b[:n]).all(), n
    for k in range(N_SOLVE):
        one = opt.ee_goals(seed[k:k + 1], ref[k:k + 1], slots[k:k + 1], params)
        for a, b in zip(one, full):
            assert (a[0] == b[k]).all(), k
    # a problem at another position of another wave
    perm = np.roll(np.arange(N_SOLVE), 9)
    moved = opt.ee_goals(seed[perm], ref[perm], slots[perm], params)
    for a, b in zip(moved, full):
        assert (a == b[perm]).all()
    return full


def test_solves_alone_equal_batch(emu):
    """3(a): n = 1, 63, 64, 65; a problem's bits do not depend on the batch or on its lane."""
    st, cost, code, it, ev = _solve_variants(emu)
    assert np.isin(code, SUCCESS).all() and code[3] == 0 and it[3] == 0 and ev[3] == 1
    assert it.max() > it.min() + 3          # lanes of one wave in different phases
    slots, seed, ref = _problems()
    assert emu.ee_refs[1].eval(_unconstrained(seed[7]), ref[7])[2]["n_mani"] > 0   # starts inside the block's clearance


def test_solves_short_ring(emu):
    """3(b): mem_size = 4, the history ring wraps inside these solves."""
    p = emu.ee_params(lbfgs=dict(mem_size=4))
    st, cost, code, it, ev = _solve_variants(emu, p)
    assert np.isin(code, SUCCESS).all() and it.max() > 6


def test_seed_offsets_keep_restatement_stable(emu):
    """The choice of delta, checked on the restatement alone (CPU only): every problem of _problems() solved again with one ulp
    added to and taken from each seed coordinate in turn (20 runs) takes the same code, iters and evals and ends within
    STATE_FLOOR of the unperturbed run.  A problem that fails this is too sensitive to compare two implementations on.
    This is also where the floor of a converged state is measured (the iteration amplifies rounding, so two
    correct implementations differ by about this much): the largest deviation over the 65 x 20 perturbed runs is 6.08e-12
    (problem 7; 6.7e-13 without it); STATE_FLOOR = 6.1e-12 is asserted and STATE_TOL = 100 x that = 6.1e-10."""
    slots, seed, ref = _problems()
    floor = 0.0
    for k in range(N_SOLVE):
        R = emu.ee_refs[slots[k]]
        a = R.optimize(seed[k], ref[k])
        for c in range(10):
            for toward in (np.inf, -np.inf):
                s2 = seed[k].copy()
                s2[c] = np.nextafter(s2[c], toward)
                b = R.optimize(s2, ref[k])
                assert b[2:] == a[2:], (k, c, a[2:], b[2:])
                floor = max(floor, np.abs(a[0] - b[0]).max())
                assert np.abs(a[0] - b[0]).max() <= STATE_FLOOR, (k, c)
    print("floor over 65 x 20 perturbed restatement runs:", floor)


def test_solves_match_restatement(emu):
    """3(c): code, iters, evals equal the restatement's; states within STATE_TOL = 6.1e-10, 100 x the floor the restatement shows
    against itself when one ulp is added to a seed coordinate (measured over every coordinate in
    test_seed_offsets_keep_restatement_stable: 6.08e-12; the single probe of coordinate 4 used here gives 4.9e-15).
    Precondition, on the restatement alone: the run with one ulp added to seed coordinate 4 takes equal iters and evals; at most
    one problem in eight may be dropped for failing it.  Measured: 65 problems used, device - restatement 1.6e-11."""
    slots, seed, ref = _problems()
    st, cost, code, it, ev = emu.ee_goals(seed, ref, slots)
    used, floor, worst = 0, 0.0, 0.0
    for k in range(N_SOLVE):
        R = emu.ee_refs[slots[k]]
        a = R.optimize(seed[k], ref[k])
        s2 = seed[k].copy()
        s2[4] = np.nextafter(s2[4], np.inf)
        b = R.optimize(s2, ref[k])
        if a[3:] != b[3:] or a[2] != b[2]:
            continue
        used += 1
        floor = max(floor, np.abs(a[0] - b[0]).max())
        assert (code[k], it[k], ev[k]) == a[2:], (k, code[k], it[k], ev[k], a[2:])
        worst = max(worst, np.abs(st[k] - a[0]).max())
        assert abs(cost[k] - a[1]) <= 1e-9 + 1e-6 * abs(a[1]), k
    print("problems used", used, "floor", floor, "device - restatement", worst)
    assert used >= N_SOLVE - N_SOLVE // 8
    assert floor <= STATE_FLOOR
    assert worst <= STATE_TOL


def test_iteration_cap_and_seed_at_limit(emu):
    slots, seed, ref = _problems()
    p = emu.ee_params(lbfgs=dict(max_iterations=3))
    st, cost, code, it, ev = emu.ee_goals(seed[:8], ref[:8], slots[:8], p)
    capped = code == -1008
    assert capped.sum() >= 4 and (it[capped] == 3).all()
    assert (st[capped] != seed[:8][capped]).any(axis=1).all()          # LBFGSERR_MAXIMUMITERATION is a success: the state is written
    for k in np.nonzero(capped)[0]:
        a = emu.ee_refs[slots[k]].optimize(seed[k], ref[k], max_iterations=3)
        assert a[2] == -1008 and np.abs(a[0] - st[k]).max() <= STATE_TOL
    bad = seed[:2].copy()
    bad[1, 4] = JMAX[1]
    out = np.zeros((2, 10))
    assert emu.L.topay_ee_goals(emu.h, 2, None, api._dp(bad), api._dp(ref[:2].copy()), None, api._dp(out), None, None, None, None) == -1
    with pytest.raises(api.TopayError, match="limit"):
        emu.ee_goals(bad, ref[:2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the deviation: no carried gradient
# ---------------------------------------------------------------------------------------------------------------------
def _deviation(opt):
    slots, seed, ref = _problems()
    k = 5
    two = opt.ee_goals(np.stack([seed[k], seed[k]]), np.stack([ref[k], ref[k]]), [slots[k]] * 2)
    for a in two:
        assert (a[0] == a[1]).all()
    names, es, x, eref = _eval_inputs()
    f1, g1 = opt.ee_eval(x, eref, es)
    f2, g2 = opt.ee_eval(x, eref, es)
    assert (f1 == f2).all() and (g1 == g2).all()
    return two, f1, g1


def test_gradient_is_assigned(emu):
    _deviation(emu)


# ---------------------------------------------------------------------------------------------------------------------
# 5. selection
# ---------------------------------------------------------------------------------------------------------------------
def test_ee_select_hand_made(emu):
    """3 groups.  Group 0: a failed code with the smallest cost, a residual over pose_tol, then a tie in cost (first wins).
    Group 1: the cheapest member in whole-body collision (arm through block A), the other wins.  Group 2: empty."""
    good = np.array([-0.6, 0, 0, 0.3, 0.4, -0.2, 0.5, 0.1, -0.3, 0.2])
    hit = np.array([0.3, 0, 0, 0.0, 0.2, 0.0, 0.2, 0.0, 0.0, 0.0])          # base under block A, arm up through it
    assert emu.whole_body_collision(hit[None], 1)[0] and not emu.whole_body_collision(good[None], 1)[0]
    states = np.stack([good, good, good, good + 1e-3, hit, good])
    ref = wl.EeGoal.pose(states)
    ref[1] = wl.EeGoal.pose(good + 0.05)                                  # residual over pose_tol
    group = np.array([0, 0, 0, 0, 1, 1], dtype=np.int32)
    cost = np.array([0.1, 0.2, 0.5, 0.5, 0.1, 0.9])
    code = np.array([-1001, 0, 1, 0, 0, -1008], dtype=np.int32)
    before = np.full((3, 10), 7.0)
    win, goal = emu.ee_select(group, 3, states, cost, code, ref, map_ids=[1] * 6, goal=before)
    assert list(win) == [2, 5, -1], win
    assert (goal[0] == states[2]).all() and (goal[1] == states[5]).all() and (goal[2] == 7.0).all()
    p = emu.ee_params(require_collision_free=0)
    win, _ = emu.ee_select(group, 3, states, cost, code, ref, map_ids=[1] * 6, params=p)
    assert list(win) == [2, 4, -1]


def _end_to_end(opt):
    """8 seeds x 2 targets on slot 1 through ee_goals and ee_select."""
    rng = np.random.default_rng(9)
    targets = np.array([[-0.6, 0.2, 0.1, 0.3, 0.4, -0.2, 0.5, 0.1, -0.3, 0.2], [-0.9, -0.4, -0.3, -0.2, 0.6, 0.3, 0.4, -0.1, 0.2, 0.0]])
    ref = np.repeat(wl.EeGoal.pose(targets), 8, axis=0)
    seed = np.repeat(targets, 8, axis=0) + 0.05 * rng.uniform(-1, 1, (16, 10))
    group = np.repeat(np.arange(2, dtype=np.int32), 8)
    mid = np.ones(16, dtype=np.int32)
    st, cost, code, it, ev = opt.ee_goals(seed, ref, mid)
    win, goal = opt.ee_select(group, 2, st, cost, code, ref, map_ids=mid)
    p = opt.ee_params()
    for gidx in range(2):
        w = win[gidx]
        assert w >= 0 and group[w] == gidx and code[w] in SUCCESS
        assert (goal[gidx] == st[w]).all()
        assert np.linalg.norm(wl.EeGoal.pose(goal[gidx][None])[0] - ref[w]) <= p.pose_tol
        assert not opt.whole_body_collision(goal[gidx][None], 1)[0]
    return st, cost, code, it, ev, win, goal


def test_ee_select_end_to_end(emu):
    _end_to_end(emu)


def _lib_exports(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\sT\s+(topay_[a-z0-9_]+)", out))


def test_new_entries_are_declared_and_exported():
    import __graft_entry__ as entry
    entry.build_hip()
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    declared = set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M))
    hip, em = _lib_exports(api.DEFAULT_LIB), _lib_exports(EMU_LIB)
    for n in NEW_ENTRIES:
        assert n in declared, n
        assert n in hip, f"{n} not exported by the HIP library"
        assert n in em, f"{n} not exported by the emulator library"


# ---------------------------------------------------------------------------------------------------------------------
# 6. the device against the emulator, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


@pytest.mark.gpu
def test_gpu_eval_bits(gpu, emu):
    names, slots, x, ref = _eval_inputs()
    assert _same(gpu.ee_eval(x, ref, slots), emu.ee_eval(x, ref, slots))
    assert _same(gpu.ee_eval(x[:1], ref[:1], slots[:1]), emu.ee_eval(x[:1], ref[:1], slots[:1]))
    rng = np.random.default_rng(11)
    rs = np.concatenate([rng.uniform(-3, 3, (65, 3)), rng.uniform(-1, 1, (65, 7)) * JMAX * 0.95], axis=1)
    assert (gpu.ee_pose(rs) == emu.ee_pose(rs)).all()
    # 65 evaluations over the three slots: the tail wave
    xs = np.array([_unconstrained(s) for s in rs * np.r_[0.1, 0.1, 1, np.ones(7)]])
    refs = wl.EeGoal.pose(rs * np.r_[0.1, 0.1, 1, np.ones(7)] + 0.02)
    mid = (np.arange(65) % 3).astype(np.int32)
    assert _same(gpu.ee_eval(xs, refs, mid), emu.ee_eval(xs, refs, mid))


@pytest.mark.gpu
def test_gpu_solves_bits(gpu, emu):
    """3(a), 3(b) on the device, and n = 65 and n = 1 against the emulator."""
    slots, seed, ref = _problems()
    for params in (None, dict(mem_size=4)):
        pg = None if params is None else gpu.ee_params(lbfgs=params)
        pe = None if params is None else emu.ee_params(lbfgs=params)
        full = _solve_variants(gpu, pg)
        assert _same(full, emu.ee_goals(seed, ref, slots, pe))
        assert _same(gpu.ee_goals(seed[:1], ref[:1], slots[:1], pg), emu.ee_goals(seed[:1], ref[:1], slots[:1], pe))
    assert gpu.ee_ms() > 0.0


@pytest.mark.gpu
def test_gpu_deviation_and_selection_bits(gpu, emu):
    assert all(_same(a, b) for a, b in zip(_deviation(gpu)[:1], _deviation(emu)[:1]))
    assert _same(_deviation(gpu)[1:], _deviation(emu)[1:])
    assert _same(_end_to_end(gpu), _end_to_end(emu))


@pytest.mark.gpu
def test_gpu_real_field():
    """256 problems on a full-size 200 x 200 x 16 tables map from topay_generate_worlds: the lanes of a wave gather from a real
    field.  Targets are getFKPose of sampled arm states; the emulator gets the same fields through get_map / set_map."""
    g = api.MomaTrajOptBatch(device=0)
    e = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    prm = api.world_params(0, lib=g.L)
    assert g.generate_worlds(prm, [77])[0] == 1
    e2, e3, _ = g.get_map(0)
    dims = np.array([200, 200, 16], dtype=np.int32)
    assert e3.size == 200 * 200 * 16
    org = np.array([-10.0, -10.0, 0.0])
    e.set_map(org, 0.1, dims, org, org + dims * 0.1, e2, e3, 0)
    rng = np.random.default_rng(3)
    star = np.concatenate([rng.uniform(-8, 8, (256, 2)), rng.uniform(-3, 3, (256, 1)), rng.uniform(-1, 1, (256, 7)) * JMAX * 0.5], axis=1)
    seed = star + 0.05 * rng.uniform(-1, 1, (256, 10))
    ref = wl.EeGoal.pose(star)
    a, b = g.ee_goals(seed, ref), e.ee_goals(seed, ref)
    assert _same(a, b)
    assert np.isin(a[2], SUCCESS).sum() >= 128
    g.close()
    e.close()
