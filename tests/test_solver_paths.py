"""The L-BFGS solver's rare paths (topay_amd/csrc/topay_solve.h) against the oracle's solver in the device's order, bit for bit:
a history ring that wraps (mem_size 1, 2, 3, 8; unequal memories of the two stages), stop windows other than the default, and every
exit of a stage the default parameters never take.  The oracle's restatement of lbfgs.hpp and of the ALM loop
(oracle/topay_oracle.hpp, pinned in tests/test_oracle_kat.py) is fed the library's own evaluations through a second context, so
whatever differs is the solver logic around them.  Every case asserts on the ORACLE's counters that the path it is named after was
taken.  The CPU half runs the kernel sources in the lane emulator, the gpu half the device library (and device == emulator).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import EMU_LIB, serpentine_path, set_map
from oracle import oracle as orc
from topay_amd import api

LBFGS_FIELDS = ("mem_size", "past", "max_linesearch", "g_epsilon", "delta", "min_step", "max_step", "f_dec_coeff", "s_curv_coeff",
                "cautious_factor", "machine_prec", "max_iterations")

# lbfgs.hpp:135-184 (include/topay.h TOPAY_LBFGS*)
CONVERGENCE, STOP, CANCELED = 0, 1, 2
INVALID_FUNCVAL, MINIMUMSTEP, MAXIMUMSTEP, MAXIMUMLINESEARCH, MAXIMUMITERATION, WIDTHTOOSMALL = -1012, -1011, -1010, -1009, -1008, -1007
OK_RETS = (CONVERGENCE, STOP, CANCELED, MAXIMUMITERATION)

# One candidate per solver arithmetic (the summation order is a function of the launch class's elements per lane): name ->
# (pieces, launch class).  The two short ones are candidates 0 and 5 of the cuboids fixture, the others the shortest serpentine of
# their class.
SERPENTINE_LEN = {16: 16.0, 22: 22.0, 33: 34.0, 65: 67.0}
CANDIDATES = {"n4": (4, 0), "n11": (11, 1), "n16": (16, 2), "n22": (22, 3), "n33": (33, 4), "n65": (65, 6)}


def _path(cs, name):
    N = CANDIDATES[name][0]
    if N in SERPENTINE_LEN:
        return serpentine_path(SERPENTINE_LEN[N])
    b = {4: 0, 11: 5}[N]
    return cs["paths"][cs["offs"][b]:cs["offs"][b + 1]]


def _lib_params(lib, prm):
    p = api.default_params(api.load(lib))
    for k, v in prm.items():
        if k[:3] in ("s1_", "s2_") and k[3:] in LBFGS_FIELDS:
            setattr(p.s1_lbfgs if k[1] == "1" else p.s2_lbfgs, k[3:], v)
        else:
            assert hasattr(p, k), k
            setattr(p, k, v)
    return p


def _oracle(cs, prm, path):
    o = orc.Oracle(cs["map"])
    for k, v in prm.items():
        o.set_param(k, v)
    o.set_init_traj(path)
    return o


def _same(a, b):
    """Bit equality of two float arrays / scalars; a NaN equals a NaN (the cost of an INVALID_FUNCVAL exit)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _solve(lib, cs, paths, prm, latency_mode=0, trace=0):
    """One library solve of `paths` under the parameter set `prm`; everything a caller can read afterwards."""
    lens = np.array([len(p) for p in paths], dtype=np.int32)
    opt = api.MomaTrajOptBatch(params=_lib_params(lib, prm), device=0, lib_path=lib)
    try:
        set_map(opt, cs["world"])
        opt.set_init_traj(lens, np.concatenate(paths))
        if latency_mode:
            opt.set_latency_mode(latency_mode)
        if trace:
            opt.set_trace(trace)
        ok = opt.optimize()
        if latency_mode:
            assert opt.last_helper_launches() > 0
        B = len(paths)
        return dict(ok=ok, st=opt.stats(), alm=opt.alm_state(), cost=opt.traj_cost.copy(), x=[opt.get_x(b) for b in range(B)],
                    traj=[opt.getTraj(b) for b in range(B)], N=opt.n_pieces(), cls=[opt.class_of(int(N)) for N in opt.n_pieces()],
                    trace=[opt.get_trace(b) for b in range(B)] if trace else None)
    finally:
        opt.close()


def _replay(lib, cs, paths, prm, res, classes=None):
    """Every candidate of the library solve `res` through the oracle's solver in device order (epl, waves from class_of), evaluations
    from a second context of the same library: success, the eight counters, the iterate, traj_cost and the ALM state are EQUAL.
    Returns the oracles' stats (the conditions of a case are asserted on those) and, per candidate, the oracle's trajectory at the
    last evaluated point (what getTraj returns: moma_traj_opt.h:943-946 reads the spline of the last cost callback)."""
    lens = np.array([len(p) for p in paths], dtype=np.int32)
    ev = api.MomaTrajOptBatch(params=_lib_params(lib, prm), device=0, lib_path=lib)
    out = []
    try:
        set_map(ev, cs["world"])
        ev.set_init_traj(lens, np.concatenate(paths))
        for b, path in enumerate(paths):
            o = _oracle(cs, prm, path)
            nw, epl, k = res["cls"][b]
            assert o.N == int(res["N"][b])
            if classes is not None:
                assert (o.N, k) == classes[b], (b, o.N, k)
            last = {}

            def fn(stage, xx, lam, rho, b=b, last=last):
                last.update(stage=stage, x=xx.copy(), lam=list(lam), rho=list(rho))
                return ev.eval(stage, b, xx, lam, rho)

            okh = o.optimize_device_order(fn, epl=epl, nw=nw)
            so = o.stats()
            tag = (b, o.N, nw, epl)
            assert [so[key] for key in api.STAT_KEYS] == list(res["st"][b]), (tag, so, list(res["st"][b]))
            assert okh == bool(res["ok"][b]), tag
            assert _same(o.get_x(), res["x"][b]), tag
            assert _same(o.traj_cost(), res["cost"][b]), (tag, o.traj_cost(), res["cost"][b])
            if so["stage1_ret"] in OK_RETS:           # (a solve that ends in stage 1 never sets the multipliers: moma_traj_opt.cpp:370-374)
                assert _same(o.alm_state(), res["alm"][b]), tag
            so["s1_past"] = o.get_init_state()["s1_past"]
            so["rounds"] = o.round_stats()
            so["last"] = last
            so["success"] = okh
            out.append(so)
    finally:
        ev.close()
    return out


def _solve_vs_device_order(lib, cs, paths, prm, classes=None, latency_mode=0, trace=0):
    res = _solve(lib, cs, paths, prm, latency_mode=latency_mode, trace=trace)
    return res, _replay(lib, cs, paths, prm, res, classes)


def _short_path(cs):
    """A 0.4 m straight move from the first state of candidate 0: shorter than s1_shot_path_horizon (0.5 m), so its stage-1 stop
    window is s1_shot_path_past (moma_traj_opt.cpp:354-357); three pieces."""
    p0 = cs["paths"][cs["offs"][0]:cs["offs"][1]]
    sp = np.stack([p0[0], p0[0]])
    sp[1, 0] += 0.4
    return sp


def _traj_matches_oracle(cs, prm, path, so, traj):
    """getTraj() after a solve is the spline of the LAST evaluation (for a failed line search: the last trial, not the restored xp --
    moma_traj_opt.h:943-946, lbfgs.hpp:575-582): the oracle evaluated at that point, tolerances of test_capped_solve_matches_oracle."""
    last = so["last"]
    o = _oracle(cs, prm, path)
    o.set_alm(last["lam"], last["rho"])
    o.eval(last["stage"], last["x"])
    d, c, kn = o.get_traj()
    assert np.allclose(traj["durations"], d, rtol=1e-8) and np.allclose(traj["coeffs"], c, rtol=1e-6, atol=1e-7)
    assert np.allclose(traj["knots_xy"], kn, atol=1e-7)


# ---- wrapped ring ----------------------------------------------------------------------------------------------------------
def _ring_params(m1, m2, cap2=None):
    """Both stop tests off (delta 0: neither the rate test nor the line search's early accept can fire) and stage 1 made a problem
    that is not solved at its initial guess (s1_path_pos_weight 2 instead of 2e5; at the default every candidate's stage 1 ends within
    6..12 iterations whatever the stop test, and the 16-piece serpentine's within 2), so that every run goes to its iteration cap:
    3 m + 1 iterations per stage and per ALM round, the smallest count with which the ring has wrapped three times."""
    return dict(s1_mem_size=m1, s2_mem_size=m2, s1_max_iterations=3 * m1 + 1, s2_max_iterations=cap2 or 3 * m2 + 1, alm_max_outer=2,
                s1_delta=0.0, s2_delta=0.0, s1_path_pos_weight=2.0, alm_tolerance=0.0)   # (tolerance 0: no round ends the ALM loop with success)


def _assert_wrapped(so, prm):
    cap1, cap2 = prm["s1_max_iterations"], prm["s2_max_iterations"]
    assert cap1 >= 3 * prm["s1_mem_size"] + 1 and cap2 >= 3 * prm["s2_mem_size"] + 1
    # stage 1 and EACH of the two ALM rounds wrapped their ring three times (a run cannot exceed its cap: lbfgs.hpp:632-637)
    m1, m2 = prm["s1_mem_size"], prm["s2_mem_size"]
    assert so["stage1_iters"] >= 3 * m1 + 1, so
    assert so["alm_outer"] == 2 and len(so["rounds"]) == 2 and all(r["iters"] >= 3 * m2 + 1 for r in so["rounds"]), so
    # the ring was full from iteration m on in every round: bound = min(k, m) summed over a round's pairs (none refused)
    assert all(r["sum_bound"] == sum(min(k, m2) for k in range(1, r["iters"])) for r in so["rounds"]), so
    assert sum(r["iters"] for r in so["rounds"]) == so["stage2_iters"] and sum(r["sum_bound"] for r in so["rounds"]) == so["sum_bound"]


def _ring_case(mem, name):
    """(The 4-piece candidate -- 32 variables -- with eight pairs is at its second round's minimum after 20 iterations, where its line
    search runs out of trials: MAXIMUMLINESEARCH, 123 evaluations.  With s2_time_weight 2000 instead of 20 both rounds run 25.)"""
    return dict(_ring_params(mem, mem), **(dict(s2_time_weight=2000.0) if (mem, name) == (8, "n4") else {}))


@pytest.mark.parametrize("name", list(CANDIDATES))
@pytest.mark.parametrize("mem", [1, 2, 3, 8])
def test_wrapped_ring_equals_oracle_in_device_order_on_cpu(cuboids_small, mem, name):
    """mem_size = mem for both stages, two ALM rounds (the second round's L-BFGS starts from an empty ring: lbfgs.hpp:536-538 --
    whichever the reference does must come out), parameters of _ring_params.  Measured on the oracle in device order, all six
    candidates alike: stage 1 MAXIMUMITERATION at 3 mem + 1 = 4 / 7 / 10 / 25 iterations, stage 2 MAXIMUMITERATION in both rounds
    with 8 / 14 / 20 / 50 iterations in all, sum_bound 6 / 22 / 48 / 328; evaluations at mem 8 between 39 + 88 (11 pieces) and
    70 + 106 (16 pieces).  Lane emulator against the oracle's solver, every bit."""
    prm = _ring_case(mem, name)
    res, so = _solve_vs_device_order(EMU_LIB, cuboids_small, [_path(cuboids_small, name)], prm, classes=[CANDIDATES[name]])
    _assert_wrapped(so[0], prm)


@pytest.mark.parametrize("m1,m2", [(8, 3), (3, 8)])
def test_unequal_memories_equal_oracle_in_device_order_on_cpu(cuboids_small, m1, m2):
    """The two stages' rings differ in length (the history blocks are strided by the larger one): 4- and 11-piece candidates,
    _ring_params(m1, m2).  Oracle: stage 1 25 (10) iterations, stage 2 2 x 10 (2 x 25), every run to its cap."""
    cs = cuboids_small
    prm = _ring_params(m1, m2)
    res, so = _solve_vs_device_order(EMU_LIB, cs, [_path(cs, "n4"), _path(cs, "n11")], prm, classes=[CANDIDATES["n4"], CANDIDATES["n11"]])
    for s in so:
        _assert_wrapped(s, prm)


@pytest.mark.parametrize("name", ["n4", "n11"])
def test_wrapped_ring_matches_oracle_in_reference_order(cuboids_small, name):
    """A second witness beside the device-order replay: the mem_size = 2 case against the oracle's ordinary optimize() (serial
    sums, no fused multiply-adds), with the cap and the tolerance of test_capped_solve_matches_oracle: one ALM round of twelve
    stage-2 iterations, equal counters, the iterate to 1e-7.  Oracle: stage 1 7 iterations, stage 2 12, sum_bound 21."""
    cs = cuboids_small
    prm = dict(_ring_params(2, 2, cap2=12), alm_max_outer=1)
    path = _path(cs, name)
    res = _solve(EMU_LIB, cs, [path], prm)
    o = _oracle(cs, prm, path)
    ok = o.optimize()
    so = o.stats()
    assert so["stage1_iters"] == 7 and so["stage2_iters"] == 12 and so["sum_bound"] == 1 + 2 * 10
    assert [so[k] for k in api.STAT_KEYS] == list(res["st"][0]) and ok == bool(res["ok"][0])
    assert np.allclose(res["x"][0], o.get_x(), rtol=1e-7, atol=1e-8)


# ---- exits -------------------------------------------------------------------------------------------------------------------
# name -> (parameters, stage whose return code is aimed at, the code).  Candidates: the 4- and the 11-piece one of the fixture.  What
# the oracle (device order) returned for the two is written behind each case as (code, iterations, evaluations) of that stage.
CAUTIOUS = dict(s2_cautious_factor=1e6, s2_delta=1e-2, s2_max_iterations=25, alm_max_outer=1)
EXITS = {
    # gmax / max(1, xmax) < 1e30 at the very first evaluation of every run: k = 0, one evaluation per run (lbfgs.hpp:549-553)
    "convergence_at_start": (dict(s1_g_epsilon=1e30, s2_g_epsilon=1e30, alm_max_outer=3), 2, CONVERGENCE),          # (0, 0, 3) (0, 0, 3)
    "convergence_after_iterations": (dict(s2_g_epsilon=100.0, alm_max_outer=1), 2, CONVERGENCE),                     # see the test
    # one trial per line search: every search whose first trial is not accepted ends the run; the ALM loop goes on (429-441)
    "maxlinesearch_stage2": (dict(s2_max_linesearch=1, alm_max_outer=30), 2, MAXIMUMLINESEARCH),
    "maxlinesearch_stage1": (dict(s1_max_linesearch=2, alm_max_outer=1), 1, MAXIMUMLINESEARCH),                       # (-1009, 5, 8) (-1009, 1, 3)
    # the first bisection of the first search (from 1 / |g|, far below 0.4) leaves the admissible steps
    "minimumstep_stage2": (dict(s2_min_step=0.4, alm_max_outer=2), 2, MINIMUMSTEP),                                   # (-1011, 1, 2) both
    "minimumstep_stage1": (dict(s1_min_step=0.4, alm_max_outer=1), 1, MINIMUMSTEP),                                   # (-1011, 1, 2) both
    # a search that doubles twice from the unit step: clipped to max_step once, MAXIMUMSTEP the second time
    "maximumstep_stage2": (dict(s2_max_step=1.0, alm_max_outer=1), 2, MAXIMUMSTEP),                                   # (-1010, 22, 40) (-1010, 3, 7)
    "maximumstep_stage1": (dict(s1_max_step=1.0, alm_max_outer=1, s2_max_iterations=5), 1, MAXIMUMSTEP),                                   # n11: (-1010, 3, 8)
    # any bracket counts as closed: the first trial that fails the decrease test after a curvature failure ends the run
    "widthtoosmall_stage2": (dict(s2_machine_prec=0.9, alm_max_outer=1), 2, WIDTHTOOSMALL),                           # (-1007, 1, 7) (-1007, 34, 67)
    "widthtoosmall_stage1": (dict(s1_machine_prec=2.0, alm_max_outer=1), 1, WIDTHTOOSMALL),                           # (-1007, 1, 2) both
    # The library has no entry that starts a solve at a chosen x, so the non-finite cost is reached from the initial guess: every
    # stage-2 pair refused (y.s <= 1e6 |s|^2 |g|), the direction stays -g with unit step, and the 4-piece candidate's ninth search
    # lands where the cost is not finite
    "invalid_funcval": (dict(CAUTIOUS), 2, INVALID_FUNCVAL),                                                          # n4: (-1012, 8, 149)
    # |g|^2 overflows at the first stage-2 evaluation: the initial step 1 / sqrt(g.g) is 0 (lbfgs.hpp:288-291)
    "invalidparameters": (dict(s2_moment_weight=1e200, alm_max_outer=1), 2, -1006),                                   # (-1006, 1, 1) both
}


_EXIT_RUNS = {}   # the emulator's exit cases, computed once (the cautious-update test reads the non-finite-cost case's second candidate)


def _exit_case(lib, cs, name, latency_mode=0, trace=0):
    key = (lib, name, latency_mode, trace)
    if key not in _EXIT_RUNS:
        _EXIT_RUNS[key] = _exit_case_run(lib, cs, name, latency_mode, trace)
    return _EXIT_RUNS[key]


def _exit_case_run(lib, cs, name, latency_mode, trace):
    prm, stage, code = EXITS[name]
    paths = [_path(cs, "n4"), _path(cs, "n11")]
    res, so = _solve_vs_device_order(lib, cs, paths, prm, classes=[CANDIDATES["n4"], CANDIDATES["n11"]], latency_mode=latency_mode, trace=trace)
    key = "stage1_ret" if stage == 1 else "stage2_last_ret"
    hit = [b for b, s in enumerate(so) if s[key] == code]
    assert hit, (name, [(s["stage1_ret"], s["stage2_last_ret"]) for s in so])
    for b in hit:
        if code < 0 and np.isfinite(res["cost"][b]):   # a failing exit: what getTraj hands out afterwards
            _traj_matches_oracle(cs, prm, paths[b], so[b], res["traj"][b])
        if code < 0 and code != MAXIMUMLINESEARCH:
            assert not so[b]["success"]
    return res, so, hit


@pytest.mark.parametrize("name", list(EXITS))
def test_exit_equals_oracle_in_device_order_on_cpu(cuboids_small, name):
    """Every way out of a stage that the default parameters never take (EXITS), on the 4- and the 11-piece candidate: the lane emulator
    against the oracle's solver in device order, every bit -- the restored x == xp, the counters, success, the reported cost and the
    ALM state; for a failing exit also getTraj against the oracle's spline at the last evaluated point.  The code aimed at is asserted
    on the ORACLE's stats for at least one candidate.  Not aimed at: INCREASEGRADIENT -- d = -H g with H built from pairs that
    passed y.s > cautious_factor |s|^2 |g| >= 0 only (topay_solve.h:469, lbfgs.hpp:682), a positive definite H, so g.d > 0 needs
    a rounding accident, not a parameter."""
    res, so, hit = _exit_case(EMU_LIB, cuboids_small, name)
    prm, stage, code = EXITS[name]
    if name == "convergence_at_start":
        assert all(s["stage1_iters"] == 0 and s["stage1_evals"] == 1 and s["stage2_iters"] == 0 and s["stage2_evals"] == s["alm_outer"] == 3 for s in so)
    if name == "convergence_after_iterations":
        assert all(so[b]["rounds"][-1]["iters"] >= 1 for b in hit)
    if name == "maxlinesearch_stage2":
        # the loop went on after a round that ended so (more than one round, every one with this code or an accepted one), and such a
        # candidate still succeeds
        assert any(so[b]["success"] and len(so[b]["rounds"]) >= 2 and sum(r["ret"] == MAXIMUMLINESEARCH for r in so[b]["rounds"][:-1]) >= 1
                   for b in hit), [s["rounds"] for s in so]
    if name == "invalid_funcval":
        assert all(np.isnan(res["cost"][b]) or np.isinf(res["cost"][b]) for b in hit)


def test_cautious_update_refuses_pairs(cuboids_small):
    """s2_cautious_factor 1e6 (CAUTIOUS: one ALM round of at most 25 iterations, s2_delta 1e-2): y.s > 1e6 |s|^2 |g| holds for no
    pair, so the ring never advances -- bound stays 0, sum_bound 0, every direction is -g -- and the iteration count differs from
    the same run with the default factor.  11-piece candidate, oracle in device order: stage 2 STOP after 22 iterations and 497
    evaluations, sum_bound 0; default factor: MAXIMUMITERATION at 25 iterations, 50 evaluations, sum_bound 300."""
    cs = cuboids_small
    paths = [_path(cs, "n11")]
    so = _exit_case(EMU_LIB, cs, "invalid_funcval")[1][1:]          # (the same parameters: that case's 11-piece candidate)
    res0, so0 = _solve_vs_device_order(EMU_LIB, cs, paths, dict(CAUTIOUS, s2_cautious_factor=1e-6), classes=[CANDIDATES["n11"]])
    assert so[0]["sum_bound"] == 0 and so[0]["stage2_last_ret"] == STOP and so[0]["stage2_iters"] >= 2 and so0[0]["sum_bound"] > 0
    assert so[0]["stage2_iters"] != so0[0]["stage2_iters"]


def test_line_search_brackets_from_both_sides(cuboids_small):
    """f_dec_coeff 0.45, s_curv_coeff 0.46: the decrease and the curvature test leave a narrow window of acceptable steps, so a search
    first fails one, then the other and bisects between mu and nu (lbfgs.hpp:346-372).  Seen in the oracle as more than two evaluations
    per iteration: 4-piece candidate 12 stage-2 iterations / 52 evaluations, 11-piece 12 / 49."""
    cs = cuboids_small
    prm = dict(s1_f_dec_coeff=0.45, s1_s_curv_coeff=0.46, s2_f_dec_coeff=0.45, s2_s_curv_coeff=0.46, alm_max_outer=1, s2_max_iterations=12)
    res, so = _solve_vs_device_order(EMU_LIB, cs, [_path(cs, "n4"), _path(cs, "n11")], prm, classes=[CANDIDATES["n4"], CANDIDATES["n11"]])
    assert all(s["stage2_evals"] > 2 * s["stage2_iters"] + 1 and s["stage2_iters"] >= 6 for s in so), so


# ---- the same on the device ----------------------------------------------------------------------------------------------------
_EMU = {}     # emulator solves shared by the gpu tests: key -> _solve(EMU_LIB, ...)
TRACE = 512


def _bits_equal(a, b, idx_a=None, idx_b=None):
    """Two library solves: success, counters, cost, ALM state, iterate, every evaluated cost and the returned spline, bit for bit."""
    ia = list(range(len(a["x"]))) if idx_a is None else idx_a
    ib = list(range(len(b["x"]))) if idx_b is None else idx_b
    for p, q in zip(ia, ib):
        assert a["ok"][p] == b["ok"][q] and (a["st"][p] == b["st"][q]).all() and _same(a["cost"][p], b["cost"][q]), (p, q)
        assert _same(a["alm"][p], b["alm"][q]) and _same(a["x"][p], b["x"][q]) and _same(a["trace"][p], b["trace"][q]), (p, q)
        assert _same(a["traj"][p]["coeffs"], b["traj"][q]["coeffs"]) and _same(a["traj"][p]["durations"], b["traj"][q]["durations"]), (p, q)


def _device_case(cs, key, paths, prm, classes, check=None):
    """Device library against the oracle's solver in device order fed from the DEVICE's evaluations, against the lane emulator bit for
    bit, and once more through the helper-wave kernels (latency mode 2) for the candidates of the one-wave classes."""
    res, so = _solve_vs_device_order(None, cs, paths, prm, classes=classes, trace=TRACE)
    if check:
        check(so)
    if key not in _EMU:
        _EMU[key] = _solve(EMU_LIB, cs, paths, prm, trace=TRACE)
    _bits_equal(res, _EMU[key])
    one_wave = [b for b, (N, k) in enumerate(classes) if k <= 3]
    hres = _solve(None, cs, [paths[b] for b in one_wave], prm, latency_mode=2, trace=TRACE)
    _bits_equal(res, hres, one_wave, None)
    return res, so


@pytest.mark.gpu
def test_wrapped_ring_on_gpu(cuboids_small):
    """mem_size 2, all six candidates in one batch (_ring_params): device == oracle's solver in device order == emulator == helper-wave
    kernels.  Oracle: 7 stage-1 iterations, two rounds of 7 stage-2 iterations, sum_bound 22 for every candidate."""
    cs = cuboids_small
    prm = _ring_params(2, 2)
    _device_case(cs, "ring2", [_path(cs, n) for n in CANDIDATES], prm, list(CANDIDATES.values()),
                 check=lambda so: [_assert_wrapped(s, prm) for s in so])


@pytest.mark.gpu
@pytest.mark.parametrize("m1,m2", [(8, 3), (3, 8)])
def test_unequal_memories_on_gpu(cuboids_small, m1, m2):
    cs = cuboids_small
    prm = _ring_params(m1, m2)
    _device_case(cs, ("unequal", m1, m2), [_path(cs, "n4"), _path(cs, "n11")], prm, [CANDIDATES["n4"], CANDIDATES["n11"]],
                 check=lambda so: [_assert_wrapped(s, prm) for s in so])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXITS))
def test_exit_on_gpu(cuboids_small, name):
    """The cases of EXITS on the device: the code aimed at is reached on the oracle fed from the device's evaluations; device == emulator
    == helper-wave kernels in every bit, trace of evaluated costs included."""
    cs = cuboids_small
    res, so, hit = _exit_case(None, cs, name, trace=TRACE)
    paths = [_path(cs, "n4"), _path(cs, "n11")]
    if name not in _EMU:
        _EMU[name] = _solve(EMU_LIB, cs, paths, EXITS[name][0], trace=TRACE)
    _bits_equal(res, _EMU[name])
    _bits_equal(res, _solve(None, cs, paths, EXITS[name][0], latency_mode=2, trace=TRACE))


# ---- stop window ---------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 1, 8), (1, 8, 0), (8, 0, 1)]      # (stage-2 past, s1_normal_past, s1_shot_path_past)
_WINDOW_RUNS = {}


def _window_case(cs, w):
    """The 4-piece candidate (a normal path) and a 0.4 m one (a shot path) with the three windows w, stage 1 as in _ring_params
    (s1_path_pos_weight 2: not solved at its initial guess), a loose stage-2 delta (1e-2, the stage-1 default) and runs capped at 40."""
    if w not in _WINDOW_RUNS:
        prm = dict(s2_past=w[0], s1_normal_past=w[1], s1_shot_path_past=w[2], s1_max_iterations=40, s2_max_iterations=40, alm_max_outer=1,
                   s1_path_pos_weight=2.0, s2_delta=1e-2)
        _WINDOW_RUNS[w] = _solve_vs_device_order(EMU_LIB, cs, [_path(cs, "n4"), _short_path(cs)], prm)[1]
    return _WINDOW_RUNS[w]


@pytest.mark.parametrize("w", WINDOWS)
def test_stop_window_equals_oracle_in_device_order_on_cpu(cuboids_small, w):
    """past 0, 1 and 8 in each of the three places it can be set, never the same value in two of them.  Oracle in device order, (stage-1
    code, iterations | stage-2 code, iterations) of the normal / the shot candidate:
      (0, 1, 8): STOP 5 | MAXIMUMITERATION 40       MAXIMUMITERATION 40 | MAXIMUMITERATION 40
      (1, 8, 0): STOP 21 | STOP 3                   MAXIMUMITERATION 40 | STOP 1
      (8, 0, 1): MAXIMUMITERATION 40 | INVALID_FUNCVAL 32     STOP 5 | STOP 17
    A window of 0 never stops, a window of 8 stops no earlier than iteration 8, and the three windows give the normal candidate's
    stage 1 three different iteration counts."""
    so = _window_case(cuboids_small, w)
    normal, shot = so
    assert normal["s1_past"] == w[1] and shot["s1_past"] == w[2] and normal["s1_past"] != shot["s1_past"]     # one candidate of each kind
    for s in so:
        if s["s1_past"] == 0:
            assert s["stage1_ret"] != STOP
        if s["s1_past"] == 8 and s["stage1_ret"] == STOP:
            assert s["stage1_iters"] >= 8
        if w[0] == 0:
            assert s["stage2_last_ret"] != STOP and s["stage2_iters"] > 0
        if w[0] == 8 and s["stage2_last_ret"] == STOP:
            assert s["stage2_iters"] >= 8
    if w[1] == 8:
        assert normal["stage1_ret"] == STOP          # past 8 with a loose delta does stop, at an iteration >= 8 (above)
    if w[0] == 8:
        assert shot["stage2_last_ret"] == STOP


def test_different_windows_give_different_iteration_counts(cuboids_small):
    runs = [_window_case(cuboids_small, w) for w in WINDOWS]
    assert len({r[0]["stage1_iters"] for r in runs}) == 3 and len({r[1]["stage2_iters"] for r in runs}) == 3


# ---- parameter checks ------------------------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(s1_mem_size=0), dict(s2_mem_size=0), dict(s1_mem_size=257), dict(s2_mem_size=257), dict(s1_past=9), dict(s2_past=9),
              dict(s1_normal_past=9), dict(s1_shot_path_past=9)]


def test_out_of_range_lbfgs_parameters_are_refused(cuboids_small):
    """validate_params: mem_size outside 1..256 and a window above 8 are TOPAY_ERR_INVALID_ARG (-1) at topay_create and at
    topay_set_params; a refused topay_set_params leaves the context solving with the parameters it had (against a fresh context)."""
    cs = cuboids_small
    good = dict(s1_mem_size=3, s2_mem_size=2, s2_past=1, s1_max_iterations=6, s2_max_iterations=6, alm_max_outer=1)
    paths = [_path(cs, "n4")]
    lens = np.array([len(paths[0])], dtype=np.int32)
    fresh = _solve(EMU_LIB, cs, paths, good)
    opt = api.MomaTrajOptBatch(params=_lib_params(EMU_LIB, good), lib_path=EMU_LIB)
    try:
        set_map(opt, cs["world"])
        for bad in BAD_PARAMS:
            with pytest.raises(api.TopayError, match="status -1:"):
                api.MomaTrajOptBatch(params=_lib_params(EMU_LIB, dict(good, **bad)), lib_path=EMU_LIB)
            h = opt.L.topay_set_params(opt.h, C.byref(_lib_params(EMU_LIB, dict(good, **bad))))
            assert h == -1, bad
        ok = opt.optimizeTraj(lens, paths[0])
        assert ok[0] == fresh["ok"][0] and (opt.stats() == fresh["st"]).all() and _same(opt.get_x(0), fresh["x"][0])
        assert _same(opt.traj_cost, fresh["cost"]) and _same(opt.alm_state(), fresh["alm"])
    finally:
        opt.close()
