"""The topological roadmap of the front-end: topay_topo_paths == TopologyPRM::findTopoPaths (src/planner/src/topo_prm.cpp:60-122
and everything it calls; the ray caster src/planner/src/utils/raycast.cpp:253-346; parameters src/planner/params/topo_prm.yaml).

Checker: harness/topo_prm.hpp -- the CPU restatement in the reference's structure (ordered list of nodes with neighbour
vectors, recursive depth-first search, std::vector paths, serial loops).  The reference ships no vectors for this module,
so the restatement is pinned by closed-form cases only (an empty map, one box, a wall, rays worked out by hand); the
kernel is structured differently (one wavefront per query, node table with id lists, explicit stack, lanes over rays and
paths) and is compared with it item by item: the eight counters, the graph node by node in list order (id, type,
position bit for bit, neighbour ids in order), the kept raw paths and their shortcut versions point by point bit for bit,
the selected paths bit for bit.  Both sides draw the same counter-based random numbers (the reference seeds from
std::random_device, topo_prm.cpp:36).

A query may differ only if the restatement's min_slack < 1e-9 for it (a discrete decision within rounding of its tie).
Note that min_slack is 0 for every query that pushes a collision point: the point is the midpoint of two cell centres, so
the floor of getDisWithGradI2d (grid_map.h:408) sits exactly on an integer by construction.  What bounds the differences
is therefore the share of differing queries: none in the emulator, at most 2 % on the device (none has been observed).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import EMU_LIB, set_map
from harness import workload as wl
from topay_amd import api


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _custom_world(occ2d):
    """A 20 x 20 m world (0.1 m cells) whose fields are those of the given 2-D occupancy (every layer of the 3-D grid)."""
    w = wl.World(wl.CUBOIDS, seed=1)
    nx, ny, nz = (int(v) for v in w.dims)
    o2 = np.ascontiguousarray(occ2d, dtype=np.int8).reshape(nx * ny)
    o3 = np.ascontiguousarray(np.repeat(o2.reshape(nx * ny, 1), nz, axis=1)).reshape(-1)
    e2, e3 = np.zeros(nx * ny), np.zeros(nx * ny * nz)
    L, P8 = wl.lib(), C.POINTER(C.c_int8)
    L.wl_edt.argtypes = [P8, P8, C.c_int, C.c_int, C.c_int, C.c_double, wl.c_dp, wl.c_dp, C.c_int]
    L.wl_edt.restype = None
    L.wl_edt(o2.ctypes.data_as(P8), o3.ctypes.data_as(P8), nx, ny, nz, float(w.res), e2.ctypes.data_as(wl.c_dp), e3.ctypes.data_as(wl.c_dp), 8)
    w.esdf2d[:] = e2                                   # (a view of the harness's own buffer: the restatement reads it)
    w._front_end_fields = wl.front_end_fields(o2, o3, w.dims, w.res)
    return w


def _build_maps(opt, tb):
    """Every scenario's map into its own slot, built on the device side from the occupancy grids (so that the front-end
    fields exist); they are the CPU construction's bit for bit."""
    slot = {s: k for k, s in enumerate(tb.scenarios)}
    for s_ in tb.scenarios:
        w = tb.world(s_)
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, w.occ3d, map_id=slot[s_])
    w = tb.world(tb.scenarios[0])
    inf, cr = opt.get_map_fields(0)
    f = wl.world_front_end_fields(w)
    assert (inf == f[0]).all() and (cr == f[1]).all()
    return slot


def _queries(tb, slot):
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]       # one (start, goal) pair per scenario, as _jps_compare
    st = np.array([tb.paths[offs[b], :2] for b in first])
    en = np.array([tb.paths[offs[b + 1] - 1, :2] for b in first])
    mid = np.array([slot[tb.scen[b]] for b in first], dtype=np.int32)
    return first, st, en, mid


def _same_paths(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _same_query(opt, k, paths_k, stats_k, r):
    """Device (or emulator) result of query k against the restatement's r, item by item."""
    if list(stats_k) != list(r["stats"]):
        return False
    if r["status"] < 0:
        return len(paths_k) == 0
    g, hg = opt.topo_graph(k), r["graph"]
    ok = len(g["id"]) == len(hg["id"]) and (g["id"] == hg["id"]).all() and (g["type"] == hg["type"]).all()
    ok = ok and (g["pos"] == hg["pos"]).all() and (g["n_nb"] == hg["n_nb"]).all()
    ok = ok and all((g["nb"][i, :g["n_nb"][i]] == hg["nb"][i, :hg["n_nb"][i]]).all() for i in range(len(hg["id"])))
    ok = ok and _same_paths(opt.topo_raw_paths(k, 0), r["raw_paths"]) and _same_paths(opt.topo_raw_paths(k, 1), r["short_paths"])
    return ok and _same_paths(paths_k, r["paths"])


def _compare(opt, tb, slot, critical, seed, first_instance, max_differ):
    first, st, en, mid = _queries(tb, slot)
    prm = opt.topo_params(seed=seed)
    paths, stats = opt.topo_paths(st, en, prm, map_ids=mid, critical=1 if critical else None, first_instance=first_instance)
    hp = wl.TopoParams(seed=seed)
    assert hp.max_sample_num == prm.max_sample_num and hp.node_cap == prm.node_cap
    out = dict(same=0, ties=0, with_path=0, two=0, max_graph=0, moves=0, pushes=0, statuses=set(), paths=paths, stats=stats, ref=[])
    for k, b in enumerate(first):
        r = wl.topo_paths(tb.world(int(tb.scen[b])), st[k], en[k], hp, inst=first_instance + k, critical=critical, track_slack=True)
        out["ref"].append(r)
        if _same_query(opt, k, paths[k], stats[k], r):
            out["same"] += 1
        else:
            assert r["min_slack"] < 1e-9, (k, stats[k], r["stats"], r["min_slack"])
            out["ties"] += 1
        out["with_path"] += int(r["status"] == 1)
        out["two"] += int(len(r["paths"]) >= 2)
        out["max_graph"] = max(out["max_graph"], int(r["stats"][3]))
        out["moves"] += int(r["moves"] > 0)
        out["pushes"] += int(r["pushes"] > 0)
        out["statuses"].add(r["status"])
        for pth in r["paths"]:                          # what topay_dense_path takes: first = start, last = goal
            assert np.abs(pth[0] - st[k]).max() < 1e-9 and np.abs(pth[-1] - en[k]).max() < 1e-9
    assert out["ties"] <= max_differ * len(first), (out["same"], out["ties"], len(first))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement's known answers (no device)
# ---------------------------------------------------------------------------------------------------------------------
START, GOAL = np.array([-3.0, 0.03]), np.array([3.0, 0.02])


def test_ray_caster_known_cells():
    """Cells lineVisib tests (map origin -10, 0.1 m cells: world cell c is map cell c + 100).  The end cell is not visited; on
    a tie tMaxX == tMaxY the ray steps y first; start and end in one cell: nothing is tested."""
    w = _custom_world(np.zeros((200, 200), dtype=np.int8))
    assert wl.topo_ray_cells(w, [0.05, 0.05], [0.45, 0.05]).tolist() == [[100, 100], [101, 100], [102, 100], [103, 100]]
    assert wl.topo_ray_cells(w, [0.05, 0.05], [0.05, -0.35]).tolist() == [[100, 100], [100, 99], [100, 98], [100, 97]]
    # exact diagonal (0, 0) -> (2, 2) from the cell centre: ties at t = 0.25 and 0.75, y first each time
    assert wl.topo_ray_cells(w, [0.05, 0.05], [0.25, 0.25]).tolist() == [[100, 100], [100, 101], [101, 101], [101, 102]]
    assert wl.topo_ray_cells(w, [0.01, 0.01], [0.09, 0.09]).tolist() == []


def test_restatement_empty_map():
    """No obstacle: the first sample sees start and goal and becomes the only connector (every later one is the same
    topology); one path survives and it is the straight segment."""
    w = _custom_world(np.zeros((200, 200), dtype=np.int8))
    r = wl.topo_paths(w, START, GOAL, wl.TopoParams(seed=1), inst=0)
    assert r["status"] == 1 and list(r["stats"][3:]) == [3, 3, 1, 1, 1] and r["stats"][1] == r["stats"][2]
    assert r["graph"]["type"].tolist() == [1, 1, 2] and r["graph"]["id"].tolist() == [0, 1, 2]
    assert r["graph"]["nb"][0, 0] == 2 and r["graph"]["nb"][1, 0] == 2 and r["graph"]["nb"][2, :2].tolist() == [0, 1]
    assert len(r["paths"]) == 1 and r["paths"][0].shape == (2, 2)
    assert (r["paths"][0][0] == START).all() and np.abs(r["paths"][0][1] - GOAL).max() < 1e-12


def test_restatement_one_box():
    """A 1.0 x 2.4 m box between start and goal (blocks the straight line, narrower than the 8 m wide sampling region): two
    selected paths, one on each side.  The count depends on the draws; seed 1 gives two (so do seeds 2..7)."""
    occ = np.zeros((200, 200), dtype=np.int8)
    occ[95:105, 88:112] = 1
    w = _custom_world(occ)
    r = wl.topo_paths(w, START, GOAL, wl.TopoParams(seed=1), inst=0)
    assert r["status"] == 1 and len(r["paths"]) == 2, r["stats"]
    d = (GOAL - START) / np.linalg.norm(GOAL - START)
    sides = []
    for pth in r["paths"]:
        assert np.abs(pth[0] - START).max() < 1e-12 and np.abs(pth[-1] - GOAL).max() < 1e-12
        cr = d[0] * (pth[1:-1, 1] - START[1]) - d[1] * (pth[1:-1, 0] - START[0])     # cross product with the start-goal direction
        assert (cr > 0).all() or (cr < 0).all()
        sides.append(np.sign(cr[0]))
    assert sorted(sides) == [-1.0, 1.0]
    assert r["pushes"] > 0


def test_restatement_wall():
    """A wall across the whole sampling region: no sample sees both guards, no path."""
    occ = np.zeros((200, 200), dtype=np.int8)
    occ[98:102, :] = 1
    w = _custom_world(occ)
    r = wl.topo_paths(w, START, GOAL, wl.TopoParams(seed=1), inst=0)
    assert r["status"] == 0 and len(r["paths"]) == 0 and r["stats"][5] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. the kernel sources in the lane emulator
# ---------------------------------------------------------------------------------------------------------------------
def test_topo_kernel_sources_on_cpu():
    """16 tables scenarios, non-critical and critical, kernel in the lane emulator against the restatement; no query may
    differ.  base_seed 777: confirmed on the restatement alone that 14 of the 16 non-critical queries return a path, 12
    two or more, the largest graph has 132 nodes, every query moves a connector (topo_prm.cpp:254), 14 push a point (543-549)
    (base_seed 31337, the seed of the JPS test, gives 11 with a path)."""
    tb = wl.TablesBatch(16, 1, base_seed=777, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    slot = _build_maps(opt, tb)
    o = _compare(opt, tb, slot, False, seed=7, first_instance=100, max_differ=0.0)
    print({k: o[k] for k in ("same", "with_path", "two", "max_graph", "moves", "pushes")})
    assert o["with_path"] >= 12 and o["two"] >= 6 and o["max_graph"] > 20 and o["moves"] >= 1 and o["pushes"] >= 1, o
    c = _compare(opt, tb, slot, True, seed=7, first_instance=100, max_differ=0.0)
    print({k: c[k] for k in ("same", "with_path", "two", "max_graph", "moves", "pushes")})
    assert c["with_path"] >= 4 and c["moves"] >= 1 and c["pushes"] >= 1, c
    assert any(not _same_paths(a, b) for a, b in zip(o["paths"], c["paths"]))       # the critical field is another map
    tb.close()


def test_topo_caps_and_refusals():
    tb = wl.TablesBatch(2, 1, base_seed=777, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    slot = _build_maps(opt, tb)
    first, st, en, mid = _queries(tb, slot)
    w = tb.world(int(tb.scen[first[0]]))
    # node pool too small: status -1 and no path, on both sides
    paths, stats = opt.topo_paths(st, en, opt.topo_params(seed=7, node_cap=6), map_ids=mid)
    for k in range(2):
        r = wl.topo_paths(tb.world(int(tb.scen[first[k]])), st[k], en[k], wl.TopoParams(seed=7, node_cap=6), inst=k)
        assert stats[k, 0] == r["status"] == -1 and len(paths[k]) == 0 and list(stats[k, 1:]) == [0] * 7
    # start and goal in one cell; start inside an obstacle (every ray from or to it is blocked next to it)
    inf = wl.world_front_end_fields(w)[0].reshape(w.dims[0], w.dims[1])
    ox, oy = np.unravel_index(np.argmin(inf), inf.shape)
    blocked = np.array([(ox + 0.5) * w.res + w.origin[0], (oy + 0.5) * w.res + w.origin[1]])
    cs = np.array([st[0], blocked, st[0]])
    ce = np.array([st[0] + 1e-3, en[0], blocked])
    paths, stats = opt.topo_paths(cs, ce, opt.topo_params(seed=7), map_ids=np.zeros(3, dtype=np.int32))
    for k in range(3):
        r = wl.topo_paths(w, cs[k], ce[k], wl.TopoParams(seed=7), inst=k)
        assert _same_query(opt, k, paths[k], stats[k], r), (k, stats[k], r["stats"])
    assert stats[1, 0] == 0 and stats[2, 0] == 0
    # cap_points too small: the length is reported, nothing is written past the cap
    full, fstats = opt.topo_paths(st, en, opt.topo_params(seed=7), map_ids=mid)
    k = int(np.argmax([len(p) > 0 and max(len(q) for q in p) > 2 for p in full]))
    assert len(full[k]) > 0
    # The call owns n x cap_paths x cap_points x 2 doubles and fills what it does not use with zeros.  cap_paths = 7 leaves at
    # least one unused path slot behind the last path of every query (reserve_num = 6): a point written past the cap of a
    # path would land in the next slot -- the last path's in that unused one -- and the block behind the last query holds
    # sentinels the call must not touch.
    n, cap_paths, cap_points = 2, 7, 2
    npth, ln = np.zeros(n, dtype=np.int32), np.zeros((n, cap_paths), dtype=np.int32)
    whole = np.full((n + 1, cap_paths, cap_points, 2), -7.0)                          # [n] = the block behind the last query
    prm = opt.topo_params(seed=7)
    s = opt.L.topay_topo_paths(opt.h, n, api._ip(mid), api._dp(np.ascontiguousarray(st)), api._dp(np.ascontiguousarray(en)), None, C.byref(prm), 0,
                               cap_paths, cap_points, api._ip(npth), api._ip(ln), api._dp(whole), None)
    assert s == 0 and (whole[n] == -7.0).all()
    for q in range(n):
        assert npth[q] == len(full[q]) and [ln[q, i] for i in range(npth[q])] == [len(p) for p in full[q]] and (ln[q, npth[q]:] == 0).all()
        for i in range(npth[q]):
            assert (whole[q, i] == full[q][i][:cap_points]).all()
        assert npth[q] < cap_paths and (whole[q, npth[q]:] == 0.0).all()
    assert max(len(p) for p in full[k]) > cap_points                                  # (a path really was longer than the cap)
    # refused inputs: a slot without the front-end fields, too few path slots, nothing to do, no outputs
    buf = np.zeros((1, 6, 8, 2))
    set_map(opt, w, map_id=5)
    with pytest.raises(api.TopayError, match="topay_build_esdf_fields"):
        opt.topo_paths(st[:1], en[:1], map_ids=np.array([5], dtype=np.int32))
    assert opt.L.topay_topo_paths(opt.h, 1, api._ip(np.array([5], dtype=np.int32)), api._dp(np.ascontiguousarray(st)), api._dp(np.ascontiguousarray(en)),
                                  None, None, 0, 6, 8, api._ip(npth), api._ip(ln), api._dp(buf), None) == -3          # TOPAY_ERR_NO_MAP
    for bad in (dict(cap_paths=5), dict(n=0), dict(n=-1)):
        a = dict(n=1, cap_paths=6)
        a.update(bad)
        assert opt.L.topay_topo_paths(opt.h, a["n"], api._ip(mid), api._dp(np.ascontiguousarray(st)), api._dp(np.ascontiguousarray(en)), None, None, 0,
                                      a["cap_paths"], 8, api._ip(npth), api._ip(ln), api._dp(buf), None) == -1        # TOPAY_ERR_INVALID_ARG
    assert opt.L.topay_topo_paths(opt.h, 1, api._ip(mid), api._dp(np.ascontiguousarray(st)), api._dp(np.ascontiguousarray(en)), None, None, 0, 6, 8,
                                  None, None, None, None) == -1
    tb.close()


def test_topo_determinism():
    """The same call twice, and split into two calls with first_instance advanced: identical bits."""
    tb = wl.TablesBatch(4, 1, base_seed=777, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    slot = _build_maps(opt, tb)
    first, st, en, mid = _queries(tb, slot)
    prm = opt.topo_params(seed=3)
    a, sa = opt.topo_paths(st, en, prm, map_ids=mid, first_instance=40)
    b, sb = opt.topo_paths(st, en, prm, map_ids=mid, first_instance=40)
    c1, s1 = opt.topo_paths(st[:3], en[:3], prm, map_ids=mid[:3], first_instance=40)
    c2, s2 = opt.topo_paths(st[3:], en[3:], prm, map_ids=mid[3:], first_instance=43)
    assert (sa == sb).all() and (sa == np.concatenate([s1, s2])).all()
    for k in range(4):
        assert _same_paths(a[k], b[k]) and _same_paths(a[k], (c1 + c2)[k])
    d, sd = opt.topo_paths(st, en, prm, map_ids=mid, first_instance=41)              # other draws, another roadmap
    assert (sd != sa).any()
    tb.close()


def test_candidate_paths_limit():
    """candidate_paths refuses more than 8 candidates per query (planner.cpp:829 throws)."""
    tb = wl.TablesBatch(1, 1, base_seed=777, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    slot = _build_maps(opt, tb)
    first, st, en, mid = _queries(tb, slot)
    cand = opt.candidate_paths(st, en, mid, prm=opt.topo_params(seed=7), first_instance=100)
    topo, _ = opt.topo_paths(st, en, opt.topo_params(seed=7), map_ids=mid, first_instance=100)
    jps, _, _ = opt.plan2d_jps(st, en, float(opt.opt_param.chassis_colli_radius) + 0.1, map_ids=mid)
    assert len(cand[0]) == len(topo[0]) + int(len(jps[0]) > 0) and _same_paths(cand[0][:len(topo[0])], topo[0])
    if len(jps[0]):
        assert (cand[0][-1] == jps[0]).all()
    assert _same_paths(opt.candidate_paths(st, en, mid, critical=True, prm=opt.topo_params(seed=7), first_instance=100)[0],
                       opt.topo_paths(st, en, opt.topo_params(seed=7), map_ids=mid, critical=1, first_instance=100)[0][0])
    orig = opt.topo_paths
    opt.topo_paths = lambda *a, **k: ([[np.zeros((2, 2))] * 9], None)
    with pytest.raises(ValueError):
        opt.candidate_paths(st, en, mid, critical=True)
    opt.topo_paths = orig
    tb.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 8. on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_topo_on_gpu_matches_restatement():
    """256 tables scenarios on the device, every query compared with the restatement item by item; differences only with
    min_slack < 1e-9 and on at most 2 % of the queries.  Confirmed on the restatement alone beforehand: more than 75 % of
    the queries return a path and more than 35 % two or more (base_seed 99 delivers 75.0 % -- 192 of 256 -- and 48.4 % with
    the default 2368 samples, 79 % and 54 % with 5000)."""
    tb = wl.TablesBatch(256, 1, base_seed=99, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0)
    slot = _build_maps(opt, tb)
    o = _compare(opt, tb, slot, False, seed=11, first_instance=5000, max_differ=0.02)
    n = len(tb.scenarios)
    print(f"{n} queries: {o['same']} identical to the restatement, {o['ties']} differing with a decision within rounding of a tie; "
          f"{o['with_path']} return a path ({o['with_path'] / n:.3f}), {o['two']} two or more ({o['two'] / n:.3f}); largest graph {o['max_graph']} nodes; "
          f"statuses {sorted(o['statuses'])}; {o['moves']} move a connector, {o['pushes']} push a point")
    assert o["with_path"] >= 0.75 * n and o["two"] >= 0.35 * n and o["max_graph"] > 20 and o["moves"] >= 1 and o["pushes"] >= 1
    tb.close()


@pytest.mark.gpu
def test_gpu_equals_emulator():
    """32 queries: the device's output is the emulator's bit for bit, the graphs included."""
    tb = wl.TablesBatch(32, 1, base_seed=555, nthreads=8)
    dev, emu = api.MomaTrajOptBatch(device=0), api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    slot = _build_maps(dev, tb)
    _build_maps(emu, tb)
    first, st, en, mid = _queries(tb, slot)
    pd, sd = dev.topo_paths(st, en, dev.topo_params(seed=5), map_ids=mid, first_instance=9)
    pe, se = emu.topo_paths(st, en, emu.topo_params(seed=5), map_ids=mid, first_instance=9)
    assert (sd == se).all(), np.nonzero((sd != se).any(axis=1))
    for k in range(len(first)):
        assert _same_paths(pd[k], pe[k]), k
        if sd[k, 0] >= 0:
            gd, ge = dev.topo_graph(k), emu.topo_graph(k)
            assert all((gd[key] == ge[key]).all() for key in ("id", "type", "pos", "n_nb", "nb")), k
            assert _same_paths(dev.topo_raw_paths(k, 0), emu.topo_raw_paths(k, 0)) and _same_paths(dev.topo_raw_paths(k, 1), emu.topo_raw_paths(k, 1))
    tb.close()


def _plan(opt, cand, start, goal, mid, inst_of_last):
    """candidates -> dense_path -> mcrrt_plan -> set_init_traj (groups by scenario) -> optimize -> check_feasible -> records.
    cand: list per scenario of raw paths.  The LAST candidate of scenario s (the JPS path) searches with MCRRT instance
    inst_of_last[s] (its draws are a function of that number); the others with instances 100000 + running index.
    Returns (scenarios with a winner, converged share of the init paths MCRRT found, candidates)."""
    S = len(cand)
    scen = np.array([s for s in range(S) for _ in cand[s]], dtype=np.int32)
    flat = [pth for s in range(S) for pth in cand[s]]
    if not flat:
        return set(), 0.0, 0
    dense, _ = opt.dense_path(flat, start[scen, 2], goal[scen, 2])
    lens = np.array([len(d) for d in dense], dtype=np.int32)
    end = goal[scen].copy()
    end[:, 2] = [d[-1, 2] for d in dense]
    is_last = np.array([j == len(cand[s]) - 1 for s in range(S) for j in range(len(cand[s]))])
    wbs, mst = [None] * len(flat), np.zeros((len(flat), 8), dtype=np.int32)
    for sel, first in ((np.nonzero(~is_last)[0], None), (np.nonzero(is_last)[0], inst_of_last)):
        if first is None:
            if len(sel):
                w_, m_, _ = opt.mcrrt_plan(lens[sel], np.concatenate([dense[i] for i in sel]), start[scen[sel]], end[sel], opt.mcrrt_params(seed=5),
                                           map_ids=mid[scen[sel]], first_instance=100000)
                for j, i in enumerate(sel):
                    wbs[i], mst[i] = w_[j], m_[j]
        else:
            for i in sel:                                  # one call per scenario: the instance number is the scenario's
                w_, m_, _ = opt.mcrrt_plan(lens[[i]], dense[i], start[scen[[i]]], end[[i]], opt.mcrrt_params(seed=5), map_ids=mid[scen[[i]]],
                                           first_instance=int(first[scen[i]]))
                wbs[i], mst[i] = w_[0], m_[0]
    keep = [i for i in range(len(flat)) if mst[i, 0] == 1]
    if not keep:
        return set(), 0.0, len(flat)
    opt.set_init_traj(np.array([len(wbs[i]) for i in keep], dtype=np.int32), np.concatenate([wbs[i] for i in keep]), map_ids=mid[scen[keep]])
    opt.set_groups(scen[keep], cancel_budget=0)
    ok = opt.optimize()
    opt.check_feasible()
    rec, _ = opt.scenario_records(scen[keep])
    return {int(r["scenario_id"]) for r in rec if r["status"] == 1}, float(ok.mean()), len(flat)


@pytest.mark.gpu
def test_planning_call_on_gpu():
    """A planning call with every step on the device (planner.cpp:792-1061) for 64 scenarios: candidate_paths -> dense_path
    -> mcrrt_plan -> set_init_traj -> optimize -> check_feasible -> scenario_records, next to the same call with the JPS
    candidate alone.  Then the planner's second try (961-963): the roadmap on the critical field for the scenarios without
    a winner (and for the first 16 in any case), bit for bit the restatement's."""
    tb = wl.TablesBatch(64, 1, base_seed=2024, nthreads=8)
    opt = api.MomaTrajOptBatch(device=0)
    slot = _build_maps(opt, tb)
    first, st, en, mid = _queries(tb, slot)
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    start = np.array([tb.paths[offs[b]] for b in first])
    goal = np.array([tb.paths[offs[b + 1] - 1] for b in first])
    S = len(first)
    prm = opt.topo_params(seed=21)
    cand = opt.candidate_paths(st, en, mid, prm=prm, first_instance=700)
    jps, _, _ = opt.plan2d_jps(st, en, float(opt.opt_param.chassis_colli_radius) + 0.1, map_ids=mid)
    has_jps = [len(j) > 0 for j in jps]
    inst = 500000 + np.arange(S)
    # (where JPS found nothing the scenario's last candidate is a roadmap path; it then simply takes the scenario's number)
    win_all, conv_all, n_all = _plan(opt, cand, start, goal, mid, inst)
    win_jps, conv_jps, n_jps = _plan(opt, [[j] if h else [] for j, h in zip(jps, has_jps)], start, goal, mid, inst)
    print(f"{S} scenarios: {n_all} candidates ({n_all / S:.2f} per scenario), winners {len(win_all)}, converged {conv_all:.3f}; "
          f"JPS candidate alone: {n_jps} candidates, winners {len(win_jps)}, converged {conv_jps:.3f}")
    assert n_all > S                                        # more than one candidate per scenario on average
    assert conv_all > 0.8
    assert len(win_all) >= len(win_jps)
    # second try on the critical field
    retry = sorted(set(range(16)) | (set(range(S)) - win_all))
    cp, cs = opt.topo_paths(st[retry], en[retry], prm, map_ids=mid[retry], critical=1, first_instance=900)
    differ, ties = 0, 0
    hp = wl.TopoParams(seed=21)
    for k, s in enumerate(retry):
        r = wl.topo_paths(tb.world(int(tb.scen[first[s]])), st[s], en[s], hp, inst=900 + k, critical=True)
        if not (list(cs[k]) == list(r["stats"]) and _same_paths(cp[k], r["paths"])):
            assert r["min_slack"] < 1e-9, (s, cs[k], r["stats"])
            ties += 1
        n0 = wl.topo_paths(tb.world(int(tb.scen[first[s]])), st[s], en[s], hp, inst=900 + k, critical=False)
        differ += int(not _same_paths(r["paths"], n0["paths"]))
    print(f"critical retry on {len(retry)} scenarios ({S - len(win_all)} without a winner): {ties} ties, {differ} differ from the non-critical roadmap")
    assert ties <= 0.02 * len(retry) and differ >= 1
    tb.close()
