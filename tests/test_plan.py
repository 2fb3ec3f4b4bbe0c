"""topay_plan_calls == Planner::planMomaParallel (src/planner/src/planner.cpp:792-1061): the whole planning call in one entry.

Checker: `_compose`, the composition of the single entry points through api.py -- topo_paths with n = 1 per call and try
(instance 2 c + t), plan2d_jps, dense_path, one mcrrt_plan per call and try (first_instance 16 c + 8 t), set_init_traj,
set_groups, optimize, check_feasible, scenario_records, getTrajs.  Both sides run the same kernels in the same order on the
same inputs, so every comparison is bit for bit: the result table, the per-candidate table, the winners' cost / duration,
their durations / coefficients / knots and the whole-body init paths.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB, set_map
from harness import workload as wl
from topay_amd import api


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _build_maps(opt, tb):
    """Every scenario's map into its own slot, built by the library from the occupancy grids (front-end fields included)."""
    slot = {s: k for k, s in enumerate(tb.scenarios)}
    for s_ in tb.scenarios:
        w = tb.world(s_)
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, w.occ3d, map_id=slot[s_])
    return slot


def _calls(tb, slot):
    """One planning call per scenario: (start [S, 10], goal [S, 10], map slot [S])."""
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]
    start = np.array([tb.paths[offs[b]] for b in first])
    goal = np.array([tb.paths[offs[b + 1] - 1] for b in first])
    mid = np.array([slot[tb.scen[b]] for b in first], dtype=np.int32)
    return start, goal, mid


def _capped(lib_path=None, s1=40, s2=40, outer=2):
    """A context whose solves are shortened through topay_params_t (as tests/test_emu_parity.py does for the emulator)."""
    L = api.load(lib_path)
    p = api.default_params(L)
    p.s1_lbfgs.max_iterations = s1
    p.s2_lbfgs.max_iterations = s2
    p.alm_max_outer = outer
    return api.MomaTrajOptBatch(params=p, device=0, lib_path=lib_path)


def _compose(opt, start, end, mid, start_v=None, prm=None, first_call=0):
    """The planning call as the composition of the single entry points.  Returns the tables of plan_calls -- result [n, 8],
    candidates [n, 2, 8, 4], winner_cost_duration [n, 2] -- and per call the winner's (durations, coeffs, knots) or None and
    its whole-body init path ([0, 10] without a winner)."""
    prm = prm if prm is not None else opt.plan_params()
    n = len(start)
    sv = np.zeros((n, 10)) if start_v is None else np.asarray(start_v, dtype=np.float64).reshape(n, 10)
    res = np.zeros((n, 8), dtype=np.int32)
    res[:, 1] = -1
    res[:, 4] = -1
    res[:, 7] = -1
    cand = np.zeros((n, 2, 8, 4), dtype=np.int32)
    wcd = np.full((n, 2), np.nan)
    trajs, fronts = [None] * n, [np.zeros((0, 10))] * n
    thr = float(opt.opt_param.chassis_colli_radius) + prm.jps_margin
    for t in (0, 1):
        if t == 1 and not prm.critical_retry:
            break
        act = [p for p in range(n) if res[p, 0] == 0]
        if not act:
            break
        keep = []                                           # (call, k, whole-body path)
        for p in act:
            c = first_call + p
            paths, tst = opt.topo_paths(start[p:p + 1, :2], end[p:p + 1, :2], prm.topo, map_ids=mid[p:p + 1], critical=1 if t else None,
                                        first_instance=2 * c + t)
            cl = list(paths[0])
            if t == 0:
                jps, _, jl = opt.plan2d_jps(start[p:p + 1, :2], end[p:p + 1, :2], thr, map_ids=mid[p:p + 1], cap=512)
                if jl[0] > 512:                           # counted, not written: a candidate that fails (no raw points)
                    cl.append(np.zeros((0, 2)))
                elif len(jps[0]):
                    cl.append(jps[0])
            m = len(cl)
            res[p, 1], res[p, 2 + t], res[p, 6] = t, m, tst[0, 0]
            if m > prm.max_candidates:
                res[p, 0] = -3
                continue
            if m == 0:
                continue
            has = [k for k in range(m) if len(cl[k])]
            dense, dl = [np.zeros((0, 4))] * m, np.zeros(m, dtype=np.int32)
            d_, l_ = opt.dense_path([cl[k] for k in has], np.full(len(has), start[p, 2]), np.full(len(has), end[p, 2]), step_size=prm.dense_step,
                                    v_max=float(opt.opt_param.max_v), w_max=float(opt.opt_param.max_w)) if has else ([], [])
            for j, k in enumerate(has):
                dense[k], dl[k] = d_[j], l_[j]
            cand[p, t, :m, 0] = 1
            good = [k for k in range(m) if 2 <= dl[k] <= 255]
            cand[p, t, [k for k in range(m) if k not in good], 2] = -2
            # one search call per call and try; singly, with the candidate's own instance number, if one had to be left out
            groups = [good] if len(good) == m else [[k] for k in good]
            for g in groups:
                if not g:
                    continue
                wbs, mst, _ = opt.mcrrt_plan(dl[g], np.concatenate([dense[k] for k in g]), np.repeat(start[p:p + 1], len(g), 0),
                                             np.repeat(end[p:p + 1], len(g), 0), prm.mcrrt, map_ids=np.full(len(g), mid[p], dtype=np.int32),
                                             first_instance=16 * c + 8 * t + g[0])
                for j, k in enumerate(g):
                    cand[p, t, k, 2] = mst[j, 0]
                    if mst[j, 0] == 1 and len(wbs[j]) >= 2:
                        keep.append((p, k, wbs[j]))
        if not keep:
            continue
        calls = np.array([q[0] for q in keep], dtype=np.int32)
        ks = [q[1] for q in keep]
        bvel = np.zeros((len(keep), 20))
        bvel[:, :10] = sv[calls]
        try:
            opt.set_init_traj(np.array([len(q[2]) for q in keep], dtype=np.int32), np.concatenate([q[2] for q in keep]), boundary_vel=bvel,
                              map_ids=mid[calls])
        except api.TopayError as e:
            if "status -5" not in str(e):                   # TOPAY_ERR_TOO_MANY_PIECES: every candidate needs more than 170 pieces
                raise
            for p, k, _ in keep:
                cand[p, t, k, 0] = 2
            continue
        opt.set_groups(calls, cancel_budget=prm.cancel_budget)
        ok = opt.optimize()
        feas = opt.check_feasible()
        intr = opt.interrupted()
        N = opt.n_pieces()
        sst = opt.stats()
        for b, (p, k, _) in enumerate(keep):
            stage = 2 if N[b] == 0 else 5 if intr[b] else 3 if not ok[b] else 4 if not feas[b] else 6
            cand[p, t, k] = (stage, N[b], cand[p, t, k, 2], sst[b, 3] if N[b] > 0 else 0)
        rec, win = opt.scenario_records(calls)
        widx = [int(w) for r, w in zip(rec, win) if r["status"] == 1]
        if widx:
            tr = opt.getTrajs(widx, N)
            off = tr["piece_off"]
            for j, b in enumerate(widx):
                p = int(calls[b])
                trajs[p] = (tr["durations"][off[j]:off[j + 1]].copy(), tr["coeffs"][off[j]:off[j + 1]].copy(),
                            tr["knots_xy"][off[j] + j:off[j + 1] + j + 1].copy())
                fronts[p] = keep[b][2]
        for r, w in zip(rec, win):
            if r["status"] == 1:
                p = int(r["scenario_id"])
                res[p, 0], res[p, 4], res[p, 5], res[p, 7] = 1, ks[int(w)], r["n_pieces"], int(w)
                wcd[p] = (r["cost"], r["duration"])
    return res, cand, wcd, trajs, fronts


def _plan(opt, start, end, mid, start_v=None, prm=None, first_call=0):
    """plan_calls and its store in the shape of _compose's return value."""
    res, cand, wcd = opt.plan_calls(start, end, map_ids=mid, start_v=start_v, params=prm, first_call=first_call)
    n = len(res)
    tr = opt.plan_trajs(np.arange(n))
    off = tr["piece_off"]
    trajs = [None] * n
    for p in range(n):
        assert off[p + 1] - off[p] == (res[p, 5] if res[p, 0] == 1 else 0)
        if res[p, 0] == 1:
            trajs[p] = (tr["durations"][off[p]:off[p + 1]].copy(), tr["coeffs"][off[p]:off[p + 1]].copy(), tr["knots_xy"][off[p] + p:off[p + 1] + p + 1].copy())
    fronts = [opt.plan_front_path(p) for p in range(n)]
    return res, cand, wcd, trajs, fronts


def _same(a, b, calls=None):
    """Bit-for-bit equality of two (result, candidates, winner_cost_duration, trajs, fronts) tuples (NaN equals NaN)."""
    idx = range(len(a[0])) if calls is None else calls
    for p in idx:
        assert (a[0][p] == b[0][p]).all(), (p, a[0][p], b[0][p])
        assert (a[1][p] == b[1][p]).all(), (p, a[1][p], b[1][p])
        assert np.array_equal(a[2][p], b[2][p], equal_nan=True), (p, a[2][p], b[2][p])
        assert (a[3][p] is None) == (b[3][p] is None), p
        if a[3][p] is not None:
            assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a[3][p], b[3][p])), p
        assert a[4][p].shape == b[4][p].shape and (a[4][p] == b[4][p]).all(), p
    return True


def _counts(out):
    res, cand = out[0], out[1]
    return dict(calls=len(res), try0_winners=int(((res[:, 0] == 1) & (res[:, 1] == 0)).sum()), ran_try1=int((res[:, 1] == 1).sum()),
                try1_winners=int(((res[:, 0] == 1) & (res[:, 1] == 1)).sum()), failed_both=int(((res[:, 0] == 0) & (res[:, 1] == 1)).sum()),
                candidates0=int(res[:, 2].sum()), interrupted=int((cand[..., 0] == 5).sum()), counting=int((cand[..., 0] == 6).sum()))


@pytest.fixture(scope="module")
def emu8():
    tb = wl.TablesBatch(8, 1, base_seed=2024, nthreads=8)
    opt = _capped(EMU_LIB)
    slot = _build_maps(opt, tb)
    start, goal, mid = _calls(tb, slot)
    yield dict(opt=opt, start=start, goal=goal, mid=mid, tb=tb)
    tb.close()


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite (lane emulator)
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_calls_equals_composition(emu8):
    """Eight tables scenarios in the emulator, solves capped (40 stage-1 and 40 stage-2 iterations, 2 ALM rounds): plan_calls
    equals _compose on result, candidates, winner_cost_duration, the winners' durations / coefficients / knots and the front
    paths.  Checked on _compose alone, so that the test cannot pass vacuously: at least one call has its winner in try 0 and
    at least one runs the second try (base_seed 2024, first_call 40: seven winners in try 0, one call decided in try 1)."""
    e = emu8
    ref = _compose(e["opt"], e["start"], e["goal"], e["mid"], first_call=40)
    cnt = _counts(ref)
    print("composition:", cnt)
    assert cnt["try0_winners"] >= 1 and cnt["ran_try1"] >= 1 and cnt["candidates0"] >= 8
    out = _plan(e["opt"], e["start"], e["goal"], e["mid"], first_call=40)
    assert _same(out, ref)
    e["ref"] = ref


def test_plan_calls_independent_of_batch(emu8):
    """The result of a call depends on the call alone: all eight together, one at a time, and in reverse order -- each call
    run singly with its own first_call -- give identical rows; so do two runs in a row."""
    e = emu8
    opt, st, en, mid = e["opt"], e["start"], e["goal"], e["mid"]
    ref = e.get("ref") or _compose(opt, st, en, mid, first_call=40)
    a = _plan(opt, st, en, mid, first_call=40)
    b = _plan(opt, st, en, mid, first_call=40)
    assert _same(a, b) and _same(a, ref)
    for p in list(range(8))[::-1]:
        one = _plan(opt, st[p:p + 1], en[p:p + 1], mid[p:p + 1], first_call=40 + p)
        for i in range(5):
            x, y = one[i][0], a[i][p]
            if i == 3:
                assert (x is None) == (y is None) and (x is None or all((u == v).all() for u, v in zip(x, y))), p
            elif i == 0:                                   # (column 7 is the winner's position in the solved batch, by definition)
                assert (x[:7] == y[:7]).all() and (x[7] >= 0) == (y[7] >= 0), (p, x, y)
            else:
                assert np.array_equal(x, y, equal_nan=True), (p, i)
    # the front-end in launches of 3 calls (test hook; the library's constant is 1024): launches 2 and 3 append to the try's
    # init paths and boundary block behind the earlier ones -- the same rows
    opt.plan_test_chunk(3)
    try:
        assert _same(_plan(opt, st, en, mid, first_call=40), a)
    finally:
        opt.plan_test_chunk(0)
    # the reversed batch with first_call chosen so that call p keeps its number is not expressible (first_call + index):
    # a reversed PAIR is, through two calls that differ in their position only
    rev = _plan(opt, st[[5, 2]], en[[5, 2]], mid[[5, 2]], first_call=45)             # position 0 = call 5 -> number 45
    assert (rev[0][0, :7] == a[0][5, :7]).all() and (rev[1][0] == a[1][5]).all() and np.array_equal(rev[2][0], a[2][5], equal_nan=True)


def test_api_names_follow_the_header():
    """The three lists of names in api.py are the header's constants: each enum of include/topay.h that names the rows of a
    table has, after its prefix and in lower case, the entries of the list, in the list's order and counted from 0, and its
    last member -- the row length -- equals the list's length."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "topay.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)               # (the prose cites the names too)
    value = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        nxt = 0
        for item in filter(None, (x.strip() for x in body.split(","))):
            name, _, v = (x.strip() for x in item.partition("="))
            nxt = (int(v, 0) if v else nxt) + 1
            value[name] = nxt - 1
    for keys, prefix in ((api.PLAN_RESULT_KEYS, "TOPAY_PLAN_RES_"), (api.PLAN_STAGES, "TOPAY_PLAN_STAGE_"), (api.PLAN_STAGE_MS_KEYS, "TOPAY_PLAN_MS_")):
        mine = sorted((v, k[len(prefix):].lower()) for k, v in value.items() if k.startswith(prefix))
        assert mine == list(enumerate(keys + ["len"])), (prefix, mine)
    cols = sorted((v, k) for k, v in value.items() if k.startswith("TOPAY_PLAN_CAND_"))
    assert [k for _, k in cols] == ["TOPAY_PLAN_CAND_" + x for x in ("STAGE", "N_PIECES", "SEARCH_STATUS", "SOLVER_STATUS", "LEN")] and [v for v, _ in cols] == list(range(5))
    assert value["TOPAY_PLAN_RES_LEN"] == 8 and value["TOPAY_PLAN_MS_LEN"] == 8 and value["TOPAY_REPLAN_ST_LEN"] == 4
    assert re.search(r"#define\s+TOPAY_PLAN_MAX_CAND\s+8\b", text) and re.search(r"#define\s+TOPAY_PLAN_CAND_ROW_LEN\s+\(2 \* TOPAY_PLAN_MAX_CAND \* TOPAY_PLAN_CAND_LEN\)", text)


def test_plan_calls_refusals_and_edges(emu8):
    e = emu8
    opt, st, en, mid = e["opt"], e["start"], e["goal"], e["mid"]
    L = opt.L
    res = np.zeros((2, 8), dtype=np.int32)
    s2, e2, m2 = np.ascontiguousarray(st[:2]), np.ascontiguousarray(en[:2]), np.ascontiguousarray(mid[:2])
    # a slot filled by set_map only has no front-end fields
    set_map(opt, e["tb"].world(e["tb"].scenarios[0]), map_id=100)
    m100 = np.array([100, 100], dtype=np.int32)
    assert L.topay_plan_calls(opt.h, 2, api._ip(m100), api._dp(s2), api._dp(e2), None, None, 0, api._ip(res), None, None) == -3   # TOPAY_ERR_NO_MAP
    with pytest.raises(api.TopayError, match="front-end fields"):
        opt.plan_calls(s2, e2, map_ids=m100)
    # bad arguments
    assert L.topay_plan_calls(opt.h, 0, api._ip(m2), api._dp(s2), api._dp(e2), None, None, 0, api._ip(res), None, None) == -1
    assert L.topay_plan_calls(opt.h, 2, api._ip(m2), None, api._dp(e2), None, None, 0, api._ip(res), None, None) == -1
    assert L.topay_plan_calls(opt.h, 2, api._ip(m2), api._dp(s2), None, None, None, 0, api._ip(res), None, None) == -1
    assert L.topay_plan_calls(opt.h, 2, api._ip(m2), api._dp(s2), api._dp(e2), None, None, 0, None, None, None) == -1
    for bad in (0, 9):
        with pytest.raises(api.TopayError):
            opt.plan_calls(s2, e2, map_ids=m2, params=opt.plan_params(max_candidates=bad))
    # critical_retry = 0: the second try never runs
    ref = e.get("ref") or _compose(opt, st, en, mid, first_call=40)
    r0, c0, _ = opt.plan_calls(st, en, map_ids=mid, params=opt.plan_params(critical_retry=0), first_call=40)
    assert (r0[:, 1] == 0).all() and (r0[:, 3] == 0).all() and (c0[:, 1] == 0).all()
    assert (c0[:, 0] == ref[1][:, 0]).all()                                          # the first try is the same one
    # max_candidates below one call's count and not below its neighbour's, both in ONE batch: -3 for the first, the neighbour
    # is what the composition gives for the same batch and what it is alone under the same call number and limit.  The
    # counts depend on the call number (the roadmap's draws), so they are taken for the numbers the batch will use.
    F, chosen = 300, None
    for a_ in range(8):
        for b_ in range(8):
            if a_ == b_ or chosen:
                continue
            ca = len(opt.candidate_paths(st[[a_], :2], en[[a_], :2], mid[[a_]], first_instance=2 * F)[0])
            cb = len(opt.candidate_paths(st[[b_], :2], en[[b_], :2], mid[[b_]], first_instance=2 * (F + 1))[0])
            if ca > cb >= 1:
                chosen = (a_, b_, ca, cb)
    assert chosen, "no pair of calls with different candidate counts"
    a_, b_, ca, cb = chosen
    prm_m = opt.plan_params(max_candidates=cb)
    ab = [a_, b_]
    both = _plan(opt, st[ab], en[ab], mid[ab], prm=prm_m, first_call=F)
    assert both[0][0, 0] == -3 and both[0][0, 2] == ca and both[0][0, 4] == -1 and (both[1][0] == 0).all() and both[3][0] is None
    assert both[0][1, 0] != -3 and both[0][1, 2] == cb and (both[1][1, 0, :cb, 0] >= 1).all()
    assert _same(both, _compose(opt, st[ab], en[ab], mid[ab], prm=prm_m, first_call=F))
    alone = _plan(opt, st[[b_]], en[[b_]], mid[[b_]], prm=prm_m, first_call=F + 1)
    assert (alone[0][0, :7] == both[0][1, :7]).all()          # (column 7: the position in the solved batch)
    for i in (1, 2):
        assert np.array_equal(alone[i][0], both[i][1], equal_nan=True), i
    assert (alone[3][0] is None) == (both[3][1] is None) and (alone[3][0] is None or all((u == v).all() for u, v in zip(alone[3][0], both[3][1])))
    assert (alone[4][0] == both[4][1]).all()
    # a goal deep inside an obstacle: status 0 with both tries recorded
    w = e["tb"].world(e["tb"].scenarios[0])
    occ = np.asarray(w.occ2d).reshape(int(w.dims[0]), int(w.dims[1]))
    e2d = np.asarray(w.esdf2d).reshape(occ.shape)
    ix, iy = np.unravel_index(int(np.argmin(e2d)), e2d.shape)
    assert e2d[ix, iy] < 0
    bad_goal = en[:1].copy()
    bad_goal[0, 0] = w.origin[0] + (ix + 0.5) * w.res
    bad_goal[0, 1] = w.origin[1] + (iy + 0.5) * w.res
    rb = _plan(opt, st[:1], bad_goal, mid[:1], first_call=7)
    assert rb[0][0, 0] == 0 and rb[0][0, 1] == 1 and rb[0][0, 4] == -1 and rb[3][0] is None and len(rb[4][0]) == 0 and np.isnan(rb[2][0]).all()
    assert _same(rb, _compose(opt, st[:1], bad_goal, mid[:1], first_call=7))
    # a non-zero start_v changes the result exactly as it does for the composition
    sv = np.zeros((2, 10))
    sv[:, 0] = 0.4
    sv[:, 3] = 0.1
    a = _plan(opt, st[:2], en[:2], mid[:2], start_v=sv, first_call=40)
    assert _same(a, _compose(opt, st[:2], en[:2], mid[:2], start_v=sv, first_call=40))
    z = _plan(opt, st[:2], en[:2], mid[:2], first_call=40)
    solved = [p for p in range(2) if (a[1][p, :, :, 0] >= 3).any()]
    if solved:
        assert any((a[1][p] != z[1][p]).any() or not np.array_equal(a[2][p], z[2][p], equal_nan=True) for p in solved)


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite
# ---------------------------------------------------------------------------------------------------------------------
def _enclosed_goal(w, goal):
    """The goal moved to the centre of the map's most deeply occupied cell: no chassis path ends there."""
    e2d = np.asarray(w.esdf2d).reshape(int(w.dims[0]), int(w.dims[1]))
    ix, iy = np.unravel_index(int(np.argmin(e2d)), e2d.shape)
    g = goal.copy()
    g[0], g[1] = w.origin[0] + (ix + 0.5) * w.res, w.origin[1] + (iy + 0.5) * w.res
    return g


@pytest.mark.gpu
def test_plan_calls_on_gpu():
    """The 64 scenarios of test_planning_call_on_gpu (TablesBatch(64, 1, base_seed=2024)) plus two whose goal is enclosed,
    default parameters (cancel_budget 2400), full solves: plan_calls equals _compose on every table and on the winners'
    trajectories and front paths.  Conditions on _compose alone: more than one candidate per scenario on average, winners
    in at least half of the scenarios, at least one call decided in try 1 or failing both tries, at least one candidate
    interrupted by the cancellation window.  Then the store survives an unrelated solve on the same context."""
    tb = wl.TablesBatch(64, 1, base_seed=2024, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0)
    slot = _build_maps(opt, tb)
    start, goal, mid = _calls(tb, slot)
    for q in (0, 1):                                        # two extra calls on the maps of scenarios 0 and 1, goal enclosed
        start = np.vstack([start, start[q:q + 1]])
        goal = np.vstack([goal, _enclosed_goal(tb.world(tb.scenarios[q]), goal[q])[None]])
        mid = np.append(mid, mid[q]).astype(np.int32)
    ref = _compose(opt, start, goal, mid, first_call=1000)
    cnt = _counts(ref)
    print("composition:", cnt)
    S = 64
    assert ref[0][:S, 2].sum() > S
    assert (ref[0][:S, 0] == 1).sum() >= S // 2
    assert cnt["try1_winners"] + cnt["failed_both"] >= 1
    assert cnt["interrupted"] >= 1
    out = _plan(opt, start, goal, mid, first_call=1000)
    print("plan_calls:", _counts(out), opt.plan_stage_ms())
    assert _same(out, ref)
    # the store survives an unrelated solve on the same context
    world, _, _, lens, paths = wl.tables_scenario(0, 4)
    opt.build_esdf(world.origin, world.res, world.dims, world.min_b, world.max_b, world.occ2d, world.occ3d, map_id=200)
    opt.optimizeTraj(lens, paths, map_ids=np.full(len(lens), 200, dtype=np.int32))
    again = (out[0], out[1], out[2]) + _plan_store(opt, out[0])
    assert _same(again, ref)
    tb.close()


def _plan_store(opt, res):
    n = len(res)
    tr = opt.plan_trajs(np.arange(n))
    off = tr["piece_off"]
    trajs = [(tr["durations"][off[p]:off[p + 1]].copy(), tr["coeffs"][off[p]:off[p + 1]].copy(), tr["knots_xy"][off[p] + p:off[p + 1] + p + 1].copy())
             if res[p, 0] == 1 else None for p in range(n)]
    return trajs, [opt.plan_front_path(p) for p in range(n)]


@pytest.mark.gpu
def test_plan_calls_gpu_equals_emulator():
    """Four calls with capped solves: every output of the device is the emulator's bit for bit."""
    tb = wl.TablesBatch(4, 1, base_seed=2024, nthreads=8)
    dev, emu = _capped(None), _capped(EMU_LIB)
    slot = _build_maps(dev, tb)
    _build_maps(emu, tb)
    start, goal, mid = _calls(tb, slot)
    a = _plan(dev, start, goal, mid, first_call=40)
    b = _plan(emu, start, goal, mid, first_call=40)
    print("device:", _counts(a))
    assert a[0][:, 2].sum() >= 4 and (a[1][..., 0] >= 3).any()     # candidates were found and solved
    assert _same(a, b)
    tb.close()
