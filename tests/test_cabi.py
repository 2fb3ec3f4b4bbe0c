"""The drop-in boundary: the hipcc-built library exists, exports every symbol include/topay.h declares, its
parameter block has the reference defaults, and without a usable HIP device it fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from topay_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    entry.build_hip()  # hipcc cross-compiles for gfx950 without a GPU
    return api.load()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "topay.h")).read()
    # function declarations look like "topay_status topay_xxx(" / "void topay_destroy(" / "const char* topay_last_error("
    return sorted(set(re.findall(r"^(?:topay_status|void|const char\*)\s+(topay_[a-z0-9_]+)\s*\(", text, flags=re.M)))


def test_library_exports_every_declared_symbol(hip_lib):
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in include/topay.h but not exported"


def test_default_params_are_the_reference_values(hip_lib):
    p = api.default_params(hip_lib)
    assert p.int_K == 12 and p.min_piece_num == 3 and p.relu_mu == 1e-3 and p.sample_interval == 1.5
    assert list(p.energy_weights) == [0.33] + [1.0] * 8
    assert (p.s1_time_weight, p.s1_path_pos_weight, p.s1_normal_past, p.s1_shot_path_past) == (20.0, 2e5, 2, 8)
    assert (p.s1_lbfgs.mem_size, p.s1_lbfgs.delta, p.s1_lbfgs.max_iterations) == (256, 1e-2, 8000)
    assert (p.s2_lbfgs.mem_size, p.s2_lbfgs.past, p.s2_lbfgs.delta, p.s2_lbfgs.min_step) == (256, 3, 1e-4, 1e-32)
    assert (p.s2_collision_weight, p.s2_mean_time_weight, p.s2_time_weight) == (5e5, 5000.0, 50.0)
    assert list(p.alm_init_rho) == [1e4, 1e4] and p.alm_tolerance == 0.01
    assert (p.max_v, p.max_a, p.max_w, p.max_dw) == (1.0, 0.8, 1.25, 1.0)
    assert min(r for r in p.colli_point_radius if r > 0) == 0.055  # moma_param.h:110-112 floor


def test_unsupported_parameters_are_rejected(hip_lib):
    p = api.default_params(hip_lib)
    p.int_K = 32
    h = C.c_void_p()
    assert hip_lib.topay_create(C.byref(p), 0, C.byref(h)) == -6  # TOPAY_ERR_UNSUPPORTED


def test_no_device_means_loud_failure(hip_lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = api.default_params(hip_lib)
    h = C.c_void_p()
    st = hip_lib.topay_create(C.byref(p), 0, C.byref(h))
    assert st == -2  # TOPAY_ERR_NO_DEVICE
    assert b"no CPU fallback" in hip_lib.topay_last_error() or b"hip" in hip_lib.topay_last_error().lower()
    with pytest.raises(api.TopayError):
        api.MomaTrajOptBatch()


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(api.TopayError):
        api.load(str(tmp_path / "libtopay_hip.so"))


def _build_demo(out):
    """examples/cabi_demo.cpp: a plain C++ caller of include/topay.h (no Python, no torch), linked against the library."""
    import subprocess

    lib_dir = os.path.join(ROOT, "topay_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cabi_demo.cpp"), "-o", out,
                           os.path.join(lib_dir, "libtopay_hip.so"), "-Wl,-rpath," + lib_dir])


def test_cpp_caller_links_against_the_boundary(hip_lib, tmp_path):
    import subprocess

    exe = str(tmp_path / "cabi_demo")
    _build_demo(exe)
    # without a device the demo must stop at topay_create with the library's error text, not compute anything
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "topay_create" in r.stderr


@pytest.mark.gpu
def test_cpp_caller_runs_on_the_device(tmp_path):
    import subprocess

    exe = str(tmp_path / "cabi_demo")
    _build_demo(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("candidate")]
    assert len(lines) == 2 and all("success 1" in ln for ln in lines)
    # the multi-GPU exchange through the C-ABI (ncclAllGather called by the library, world size 1)
    assert "record gather over RCCL (world 1): ok" in r.stdout, r.stdout + r.stderr
    # the front-end chain through the C-ABI: 2-D path around the wall, dense path, joint-space search, trajectory
    fe = [ln for ln in r.stdout.splitlines() if ln.startswith("front-end:")]
    assert len(fe) == 2 and "joint search status 1" in fe[0] and "trajectory success 1" in fe[1], r.stdout
    # the several-processes mode of the exchange (tests/test_sharding.py runs it with two ranks where there are two GPUs) as one rank
    r = subprocess.run([exe, "--exchange", "0", "1", str(tmp_path / "comm.id")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rank 0 of 1 on device 0: record gather over RCCL, 2 records from 1 ranks: ok" in r.stdout, r.stdout + r.stderr


def test_header_is_plain_c99():
    """The boundary is a C ABI: include/topay.h must compile as C (a cgo / JNI / ctypes generator reads it as such)."""
    import subprocess

    src = '#include "topay.h"\nint main(void) { topay_params_t p; return (int)sizeof(p) == 0; }\n'
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src, text=True, check=True)


def test_reference_side_adapter_compiles_against_the_header():
    """examples/moma_traj_opt_hip.h is the class a TopAY maintainer drops into the reference: the
    reference's optimizeTraj / getTraj / traj_cost / printConstraintsSituations surface over the C-ABI, written against
    the real GridMap accessors (grid_map.h:85-86, 179, 203, 206, 213-216).  Eigen and ROS are absent here, so it is
    syntax-checked against name-and-signature stand-ins (tests/stubs/); a signature drift of include/topay.h breaks it."""
    import subprocess

    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + os.path.join(ROOT, "examples"),
                        os.path.join(ROOT, "examples", "adapter_syntax_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_parameter_file_loader_follows_the_reference_keys():
    """params_from_yaml == MomaTrajOpt::init (moma_traj_opt.h:845-941): keys of the reference's optimizer.yaml land in
    the fields the kernels read; the keys the path has no use for are reported, unknown keys too."""
    text = """
planner_node:
  moma_traj_opt:
    int_K: 12
    sample_interval: 1.25
    mean_time_lowb: 0.4
    energy_weights: [0.5, 1, 1, 1, 1, 1, 1, 1, 2]
    first_stage:
      time_weight: 21.0
      lbgfs_normal_past: 4
      lbfgs: {mem_size: 128, delta: 2.0e-2}
    second_stage:
      collision_weight: 123456.0
      mean_time_weight: 7.0
      lbfgs: {past: 5, min_step: 1.0e-30, max_iterations: 77}
      alm_param:
        init_rho: [2.0e4, 3.0e4, 1, 1, 1, 1, 1, 1, 1]
        tolerance: [0.02]
      alm_data: {max_iter: 100}
    no_such_key: 1
"""
    d = api.default_params()
    p, ignored = api.params_from_yaml(text)
    assert p.sample_interval == 1.25 and p.energy_weights[0] == 0.5 and p.energy_weights[8] == 2.0
    assert p.s1_time_weight == 21.0 and p.s1_normal_past == 4 and p.s1_lbfgs.past == 4
    assert p.s1_lbfgs.mem_size == 128 and p.s1_lbfgs.delta == 2.0e-2 and p.s1_lbfgs.max_iterations == d.s1_lbfgs.max_iterations
    assert p.s2_collision_weight == 123456.0 and p.s2_mean_time_weight == 7.0
    assert p.s2_lbfgs.past == 5 and p.s2_lbfgs.min_step == 1.0e-30 and p.s2_lbfgs.max_iterations == 77
    assert list(p.alm_init_rho) == [2.0e4, 3.0e4] and p.alm_tolerance == 0.02 and list(p.alm_gamma) == list(d.alm_gamma)
    assert p.s2_mani_pos_weight == d.s2_mani_pos_weight and p.max_v == d.max_v       # untouched keys keep the defaults
    assert sorted(ignored) == ["mean_time_lowb", "no_such_key", "second_stage/alm_data/max_iter"]
    # the library's own loader (topay_params_from_yaml, what a C++ planner calls): same fields, same report
    from conftest import EMU_LIB
    pc, ignored_c = api.params_from_yaml_c(text, lib=api.load(EMU_LIB))
    assert bytes(pc) == bytes(p) and sorted(ignored_c) == sorted(ignored)
    # the reference's own parameter file (its settings, tests/golden/optimizer.yaml) gives exactly the built-in defaults
    ref = os.path.join(ROOT, "tests", "golden", "optimizer.yaml")
    q, ign = api.params_from_yaml(ref)
    assert bytes(q) == bytes(d)
    qc, ign_c = api.params_from_yaml_c(ref, lib=api.load(EMU_LIB))
    assert bytes(qc) == bytes(d) and sorted(ign_c) == sorted(ign)
    assert sorted(ign) == ["first_stage/mean_time_weight", "mean_time_lowb", "mean_time_uppb", "second_stage/alm_data/epsilon_con",
                           "second_stage/alm_data/max_iter"]


def test_isa_lint_recognises_the_defect_pattern(tmp_path):
    """tools/isa_lint.py (run by build() on the product sources): a join block with a lane-wise copy ahead of its EXEC
    restore is reported, the regular shape is not."""
    import subprocess
    import sys

    bad = tmp_path / "bad.s"
    bad.write_text("k_x:\n\ts_and_saveexec_b64 s[4:5], vcc\n\ts_cbranch_execz .LBB0_2\n\tv_add_f64 v[0:1], v[0:1], v[2:3]\n.LBB0_2:\n"
                   "\tv_readlane_b32 s0, v255, 4\n\tv_accvgpr_write_b32 a86, v152\n\ts_or_b64 exec, exec, s[4:5]\n\ts_endpgm\n")
    good = tmp_path / "good.s"
    good.write_text("k_x:\n\ts_and_saveexec_b64 s[4:5], vcc\n\ts_cbranch_execz .LBB0_2\n\tv_add_f64 v[0:1], v[0:1], v[2:3]\n.LBB0_2:\n"
                    "\tv_readlane_b32 s0, v255, 4\n\ts_or_b64 exec, exec, s[4:5]\n\tv_accvgpr_write_b32 a86, v152\n\ts_endpgm\n")
    tool = os.path.join(ROOT, "tools", "isa_lint.py")
    assert subprocess.run([sys.executable, tool, str(bad)], capture_output=True).returncode == 1
    assert subprocess.run([sys.executable, tool, str(good)], capture_output=True).returncode == 0


def test_scenario_records_match_the_host_selection(hip_lib):
    """topay_scenario_records (planner.cpp:999-1010 inside the library, for C++ callers) against dist.scenario_records, the
    numpy restatement bench.py uses, on a solved batch of the lane emulator."""
    import numpy as np
    from conftest import EMU_LIB, set_map
    from harness import workload as wl
    from topay_amd import dist as tdist

    w, lens, paths, scen = wl.cuboids_batch(3, 2)
    p = api.default_params(api.load(EMU_LIB))
    p.s2_lbfgs.max_iterations = 10
    p.alm_max_outer = 1
    p.alm_tolerance = 10.0
    emu = api.MomaTrajOptBatch(params=p, lib_path=EMU_LIB)
    set_map(emu, w)
    ok = emu.optimizeTraj(lens, paths)
    so = np.array([7, 7, 9, 9, 4, 4], dtype=np.int32)
    recs, win = emu.scenario_records(so)
    acc = (ok & emu.check_feasible()).astype(np.int32)
    ref, rwin = tdist.scenario_records(np.array([7, 9, 4]), so, acc, emu.traj_cost, emu.n_pieces(), emu.total_durations(), return_winners=True)
    assert list(recs["scenario_id"]) == [7, 9, 4]
    for r, q in zip(recs, ref):
        assert r["scenario_id"] == q[0] and r["best_candidate"] == q[1] and r["status"] == q[2]
        if r["status"]:
            assert r["n_pieces"] == q[3] and r["cost"] == q[4] and r["duration"] == q[5]
    assert sorted(int(b) for b in win if b >= 0) == sorted(int(b) for b in rwin)
    with pytest.raises(api.TopayError):            # no communicator yet
        emu.gather_records(recs, 4, 1)
    w.close()


@pytest.mark.gpu
def test_record_gather_through_the_cabi_on_one_gpu():
    """topay_comm_unique_id / topay_comm_init / topay_gather_records: the library's own ncclAllGather (RCCL bound with dlopen),
    world size 1, beside a solve in flight on the same context."""
    import numpy as np
    from conftest import set_map
    from harness import workload as wl

    world, start, goal, lens, paths = wl.tables_scenario(2, 8)
    opt = api.MomaTrajOptBatch(device=0)
    set_map(opt, world)
    opt.optimizeTraj(lens, paths)
    recs, win = opt.scenario_records(np.full(len(lens), 5, dtype=np.int32))
    assert len(recs) == 1 and recs[0]["scenario_id"] == 5
    opt.comm_init(opt.comm_unique_id(), 1, 0)
    other = api.MomaTrajOptBatch(device=0)          # a second context keeps the device busy meanwhile
    set_map(other, world)
    other.set_init_traj(lens, paths)
    other.optimize_async()
    got = opt.gather_records(recs, 16, 1)
    other.finish()
    assert len(got) == 1 and got[0].tobytes() == recs[0].tobytes()
    empty = opt.gather_records(recs[:0], 16, 1)
    assert len(empty) == 0
    opt.comm_destroy()
    world.close()


def test_shared_map_slots_are_invalidated_when_the_owner_refills_or_goes_away(cuboids_small):
    """topay_share_maps hands out device pointers: when the owner refills a shared slot or is destroyed, the sharer must
    lose the slot (TOPAY_ERR_NO_MAP) instead of keeping a dangling descriptor."""
    from conftest import EMU_LIB, set_map
    cs = cuboids_small
    owner = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    set_map(owner, cs["world"])
    a = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    a.share_maps(owner, 0, 1)
    a.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    x = a.get_x(0)
    f0 = a.eval(1, 0, x)[0]
    set_map(owner, cs["world"])                      # the owner refills slot 0: new buffers may replace the old ones
    with pytest.raises(api.TopayError):
        a.eval(1, 0, x)                              # the resident batch used the slot: it has to be set again
    with pytest.raises(api.TopayError):
        a.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])   # ... and the slot is gone
    a.share_maps(owner, 0, 1)
    a.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    assert a.eval(1, 0, x)[0] == f0
    owner.close()                                    # the owner goes away: same rule
    with pytest.raises(api.TopayError):
        a.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    a.close()


def test_a_slot_shared_from_a_sharer_follows_the_context_that_holds_the_fields(cuboids_small):
    """A owns the fields, B shares A's slot, C shares the slot from B: C's descriptor points at A's buffers, so it is A's
    refill or destruction that must take the slot away from C -- B going away must not."""
    from conftest import EMU_LIB, set_map
    cs = cuboids_small
    a = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    set_map(a, cs["world"])
    b = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    b.share_maps(a, 0, 1)
    c = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    c.share_maps(b, 0, 1)
    c.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    x = c.get_x(0)
    f0 = c.eval(1, 0, x)[0]
    b.close()                                        # the middle context goes away: the fields are A's and stay
    assert c.eval(1, 0, x)[0] == f0
    set_map(a, cs["world"])                          # the holder refills the slot: C loses it
    with pytest.raises(api.TopayError):
        c.eval(1, 0, x)
    with pytest.raises(api.TopayError):
        c.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    c.share_maps(a, 0, 1)
    c.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    assert c.eval(1, 0, x)[0] == f0
    a.close()
    with pytest.raises(api.TopayError):
        c.set_init_traj(cs["lens"][:2], cs["paths"][:cs["offs"][2]])
    c.close()


def test_a_field_with_a_single_z_layer_is_refused(cuboids_small):
    """The ESDF lookups of the evaluation fetch the two z-neighbours of a corner pair with one 16-byte load (round 5): with a
    single layer the pair would reach past the field, so such a map is refused when it is set (the reference's maps have 16)."""
    from conftest import EMU_LIB
    w = cuboids_small["world"]
    o = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    dims = np.array([w.dims[0], w.dims[1], 1], dtype=np.int32)
    e3 = np.ascontiguousarray(w.esdf3d.reshape(w.dims[0], w.dims[1], w.dims[2])[:, :, :1])
    with pytest.raises(api.TopayError):
        o.set_map(w.origin, w.res, dims, w.min_b, w.max_b, w.esdf2d, e3)
    o.close()


def test_a_destroyed_context_has_given_back_every_allocation():
    """Device buffers own their memory (DevBuf frees in its destructor, topay_destroy frees the members by `delete`): the
    emulator's count of live hipMalloc / hipHostMalloc allocations is the same after topay_destroy as before topay_create,
    for a context that went through a map build, set_init_traj, a solve, the gate, a getter, the front-end entries with
    function-local buffers (dense path, connect collision, Reeds-Shepp, JPS), the roadmap, the joint-space search, a
    planning call, a world generation, a sensor cloud inserted and committed, a tracked trajectory swept, an end-effector goal
    and one control period of the tracking controller.  The single entries are also balanced one by one while the context
    lives: a local buffer is freed by scope.  The same holds for events and streams: every stage's stopwatch owns its pair of
    events (DevTimer), so the emulator's counts of live events and live streams are back where they were too.

    topay_dense_path has no input that fails after its allocations without faking an error: every argument check comes
    before them, and what follows can only fail through a HIP call, which the emulator never fails.  So that path is
    covered by construction (scope) and not by a case here."""
    import gc

    from conftest import EMU_LIB
    from harness import workload as wl

    L = api.load(EMU_LIB)
    L.topay_emu_live_allocations.restype = C.c_long
    live = L.topay_emu_live_allocations
    L.topay_emu_live_events.restype = C.c_long
    L.topay_emu_live_streams.restype = C.c_long
    tb = wl.TablesBatch(2, 2, base_seed=2024, nthreads=8)
    gc.collect()                                   # (contexts of earlier tests that are garbage go now, not in between)
    before = live()
    events_before, streams_before = L.topay_emu_live_events(), L.topay_emu_live_streams()
    p = api.default_params(L)
    p.s1_lbfgs.max_iterations = 20
    p.s2_lbfgs.max_iterations = 20
    p.alm_max_outer = 1
    opt = api.MomaTrajOptBatch(params=p, lib_path=EMU_LIB)
    assert live() > before
    slot = {s: k for k, s in enumerate(tb.scenarios)}
    for s_ in tb.scenarios:
        w = tb.world(s_)
        opt.build_esdf(w.origin, w.res, w.dims, w.min_b, w.max_b, w.occ2d, w.occ3d, map_id=slot[s_])
    mid = np.array([slot[s_] for s_ in tb.scen], dtype=np.int32)
    opt.set_init_traj(tb.lens, tb.paths, map_ids=mid)
    opt.optimize()
    opt.check_feasible()
    opt.getTraj(0)
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    start = np.array([tb.paths[offs[b]] for b in range(len(tb.lens))])
    end = np.array([tb.paths[offs[b + 1] - 1] for b in range(len(tb.lens))])
    held = live()                                  # what the context keeps; the entries below add nothing that outlives them
    raw = [tb.paths[offs[b]:offs[b + 1], :2] for b in range(2)]
    opt.dense_path(raw, start[:2, 2], end[:2, 2])
    assert live() == held
    n = 4
    a = np.c_[np.linspace(-2, 2, n), np.zeros(n), np.zeros(n)]
    b = a + np.array([0.5, 0.3, 0.1])
    opt.connect_collision(np.full(n, 0.7), lambda e, fr: a[e] + fr[:, None] * (b[e] - a[e]), np.zeros((n, 7)), np.full((n, 7), 0.1), 0.1)
    assert live() == held
    opt.reeds_shepp(a, b, t=0.5)
    assert live() == held
    opt.plan2d_jps(start[:2, :2], end[:2, :2], map_ids=mid[:2])
    assert live() == held
    opt.topo_paths(start[:1, :2], end[:1, :2], opt.topo_params(seed=7, max_sample_num=200), map_ids=mid[:1])
    car = np.concatenate([np.c_[tb.paths[offs[b]:offs[b + 1], :3], tb.dts[offs[b]:offs[b + 1]]] for b in range(2)])
    opt.mcrrt_plan(tb.lens[:2], car, start[:2], end[:2], opt.mcrrt_params(seed=7, max_iter=50), map_ids=mid[:2])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]
    opt.plan_calls(start[first], end[first], map_ids=mid[first], params=opt.plan_params(topo=dict(max_sample_num=200), mcrrt=dict(max_iter=50)))
    opt.plan_trajs([0, 1])
    # the subjects with stopwatches and state of their own, each on the smallest map its tests use: a 2.4 x 2.4 x 1.6 m
    # tables world (24 x 24 x 16 cells) in slot 8, a belief on 24 x 24 x 12 voxels in slot 7
    assert opt.generate_worlds(api.world_params(0, size_xy=2.4, size_z=1.6, lib=L), [5], first_map_id=8)[0] != 0
    opt.sense_reset([7], origin=(-1.2, -1.2, 0.0), res=0.1, dims=(24, 24, 12), min_b=(-1.2, -1.2, 0.0), max_b=(1.2, 1.2, 1.2))
    opt.sense_insert([7], [np.array([[0.85, 0.05, 0.55, 0.0]], dtype=np.float32)], [(0.05, 0.05, 0.55)], opt.sense_params(point_filt_num=1))
    opt.sense_commit([7])
    co = np.zeros((1, 9, 6))
    co[0, 1, 4] = 0.5                              # one piece, 0.5 m along x in 1 s
    opt.track_set(3, 1, [-0.5, 0.0, 0.0], [1.0], co)
    opt.track_safe([3], [8])
    opt.ee_goals(np.zeros((1, 10)), opt.ee_pose(np.full((1, 10), 0.1)), map_ids=[8], params=opt.ee_params(lbfgs=dict(max_iterations=2)))
    opt.mpc_reset([3])
    opt.sim_reset([3], np.zeros((1, 10)))
    opt.track_follow([3], 0.0, 1)
    assert live() > before and L.topay_emu_live_events() > events_before
    opt.close()
    assert live() == before
    assert L.topay_emu_live_events() == events_before and L.topay_emu_live_streams() == streams_before
    tb.close()


@pytest.fixture(scope="module")
def three_class_batch(cuboids_small):
    """Three candidates in three launch classes (N = 5, 12, 33: the classes N <= 10, <= 15 and <= 42) on the lane emulator,
    laid out and then solved with a cap of three iterations per stage and one ALM round.  Shared by the layout tests below."""
    from conftest import EMU_LIB, serpentine_path, set_map

    paths = [serpentine_path(L) for L in (5.0, 12.0, 34.0)]
    lens = np.array([len(q) for q in paths], dtype=np.int32)
    p = api.default_params(api.load(EMU_LIB))
    p.s1_lbfgs.max_iterations = 3
    p.s2_lbfgs.max_iterations = 3
    p.alm_max_outer = 1
    emu = api.MomaTrajOptBatch(params=p, lib_path=EMU_LIB)
    set_map(emu, cuboids_small["world"])
    emu.set_init_traj(lens, np.concatenate(paths))
    laid_out = dict(n_pieces=list(emu.n_pieces()), workspace=emu.workspace_bytes())
    emu.optimizeTraj(lens, np.concatenate(paths))
    yield emu, laid_out
    emu.close()


def test_workspace_of_three_launch_classes_is_unchanged(three_class_batch):
    """Every allocation of the resident batch is sized by the layout constants of topay_types.h (kHeadLen ... kInitXyStride):
    the sum for N = 5, 12, 33 with the default history depth is the figure the build before those constants reported for
    this same batch (taken by running this body on commit 73de4fd)."""
    emu, laid_out = three_class_batch
    assert laid_out["n_pieces"] == [5, 12, 33]
    assert laid_out["workspace"] == 2439396


def test_candidate_views_agree_across_getters_and_gates(three_class_batch):
    """The host's offsets and the kernels' views of a candidate's blocks: getTraj(i) (host copies at h_poff) against the slices of
    getTrajs([0, 1, 2]) (k_gather_results), bit for bit; and the feasibility report of the gate inside the solve, then -- after
    load_solution has invalidated it -- of the separate gate kernel, against the values commit 73de4fd gave for this batch
    (tests/golden/cabi_layout_reports.npy: [in-solve, kernel][candidate][38], recorded with this body)."""
    emu, _ = three_class_batch
    pk = emu.getTrajs([0, 1, 2])
    assert list(pk["piece_off"]) == [0, 5, 17, 50]
    for i in range(3):
        tr = emu.getTraj(i)
        a, b = pk["piece_off"][i], pk["piece_off"][i + 1]
        assert pk["durations"][a:b].tobytes() == tr["durations"].tobytes()
        assert pk["coeffs"][a:b].tobytes() == tr["coeffs"].tobytes()
        assert pk["knots_xy"][a + i:b + i + 1].tobytes() == tr["knots_xy"].tobytes()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "cabi_layout_reports.npy"))
    f, st, rep = emu.check_feasible(report=True)
    assert list(f) == [True, False, False] and list(st) == [True, False, False]
    assert rep.tobytes() == gold[0].tobytes()
    alm = emu.alm_state()[0]
    emu.load_solution(0, emu.get_x(0), alm[:2], alm[2:])
    f, st, rep = emu.check_feasible(report=True)
    assert list(f) == [True, False, False] and list(st) == [True, False, False]
    assert rep.tobytes() == gold[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Status codes of the slot checks: every entry that takes map slots or robot slots, on the lane emulator
# ---------------------------------------------------------------------------------------------------------------------
MAX_MAPS, TRACK_SLOTS = 4096, 4096      # TOPAY_MAX_MAPS, TOPAY_TRACK_SLOTS
EMPTY_MAP, ROBOT = 9, 3                 # a map slot that is never filled; the robot slot with an end_traj, a controller, a simulator


@pytest.fixture(scope="module")
def slot_ctx():
    """One emulator context: map slot 0 set by topay_set_map (8 x 8 x 2 cells, every distance 1 m), robot slot ROBOT with a
    one-piece end_traj, a controller and a simulator; a second context for topay_share_maps."""
    from conftest import EMU_LIB

    o = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    o.set_map([0, 0, 0], 0.5, [8, 8, 2], [0, 0, 0], [4, 4, 1], np.ones(64), np.ones(128), 0)
    co = np.zeros((1, 9, 6))
    co[0, 1, 4] = 0.5
    o.track_set(ROBOT, 1, [1.0, 1.0, 0.0], [1.0], co)
    o.mpc_reset([ROBOT])
    o.sim_reset([ROBOT], np.zeros((1, 10)))
    other = api.MomaTrajOptBatch(lib_path=EMU_LIB)
    yield o, other
    other.close()
    o.close()


def _tiny_world(o):
    return api.world_params(0, size_xy=10.0, lib=o.L)


def _z(*shape):
    return np.zeros(shape)


# entry -> the call with map slot m in the place of its map_id / only element of its map_ids
_MAP_ENTRIES = {
    "topay_set_init_traj": lambda o, x, m: o.set_init_traj([2], _z(2, 10), map_ids=[m]),
    "topay_get_map": lambda o, x, m: o.L.topay_get_map(o.h, m, None, None, None),
    "topay_get_map_fields": lambda o, x, m: o.L.topay_get_map_fields(o.h, m, None, None),
    "topay_get_occupancy": lambda o, x, m: o.L.topay_get_occupancy(o.h, m, None, None, None),
    "topay_share_maps": lambda o, x, m: x.share_maps(o, m, 1),
    "topay_whole_body_collision": lambda o, x, m: o.whole_body_collision(_z(1, 10), map_id=m),
    "topay_connect_collision": lambda o, x, m: o.L.topay_connect_collision(o.h, m, 1, api._ip(np.array([3], dtype=np.int32)), api._dp(_z(9)), api._dp(_z(7)),
                                                                          api._dp(_z(7)), api._ip(np.zeros(1, dtype=np.int32))),
    "topay_plan2d_jps": lambda o, x, m: o.plan2d_jps(_z(1, 2) + 1.0, _z(1, 2) + 2.0, map_ids=[m]),
    "topay_topo_paths": lambda o, x, m: o.topo_paths(_z(1, 2) + 1.0, _z(1, 2) + 2.0, map_ids=[m]),
    "topay_mcrrt_plan": lambda o, x, m: o.mcrrt_plan([2], _z(2, 4), _z(1, 10), _z(1, 10), map_ids=[m]),
    "topay_plan_calls": lambda o, x, m: o.plan_calls(_z(1, 10) + 1.0, _z(1, 10) + 2.0, map_ids=[m]),
    "topay_sample_arm": lambda o, x, m: o.sample_arm(_z(1, 10), [1], map_ids=[m]),
    "topay_sample_scenarios": lambda o, x, m: o.sample_scenarios([1], map_ids=[m]),
    "topay_track_safe": lambda o, x, m: o.track_safe([ROBOT], [m]),
    "topay_replan_calls": lambda o, x, m: o.replan_calls([ROBOT], [m], 0.0, 0.0, _z(1, 10), 1.0, 0.1, 5.0),
    "topay_ee_eval": lambda o, x, m: o.ee_eval(_z(1, 10), _z(1, 9), map_ids=[m]),
    "topay_ee_goals": lambda o, x, m: o.ee_goals(_z(1, 10), _z(1, 9), map_ids=[m]),
    "topay_ee_select": lambda o, x, m: o.ee_select([0], 1, _z(1, 10), _z(1), [0], _z(1, 9), map_ids=[m]),
    "topay_sense_insert": lambda o, x, m: o.sense_insert([m], [np.zeros((0, 4), dtype=np.float32)], [[0.0, 0.0, 0.0]]),
    "topay_sense_commit": lambda o, x, m: o.sense_commit([m]),
    "topay_sense_get": lambda o, x, m: o.L.topay_sense_get(o.h, m, None, None, None, None),
    "topay_sense_scan": lambda o, x, m: o.sense_scan([m], _z(1, 4), 2, 2, 1.0, 1.0),
    # entries that fill slots: an empty slot is what they are for, so only the two slots out of range
    "topay_set_map": lambda o, x, m: o.set_map([0, 0, 0], 0.5, [8, 8, 2], [0, 0, 0], [4, 4, 1], np.ones(64), np.ones(128), m),
    "topay_build_esdf_fields": lambda o, x, m: o.build_esdf_fields([0, 0, 0], 0.5, [8, 8, 2], [0, 0, 0], [4, 4, 1], np.zeros(64, dtype=np.int8), None,
                                                                   np.zeros(128, dtype=np.int8), map_id=m),
    "topay_generate_worlds": lambda o, x, m: o.generate_worlds(_tiny_world(o), [1], first_map_id=m),
    "topay_generate_episodes": lambda o, x, m: o.generate_episodes(_tiny_world(o), [1], first_map_id=m),
    "topay_sense_reset": lambda o, x, m: o.sense_reset([m], (0, 0, 0), 0.5, (8, 8, 2), (0, 0, 0), (4, 4, 1)),
}
_FILLERS = ("topay_set_map", "topay_build_esdf_fields", "topay_generate_worlds", "topay_generate_episodes", "topay_sense_reset")
# entry -> the call with the robot slots r (a list; the entries of one robot take r[0])
_ROBOT_ENTRIES = {
    "topay_track_set": lambda o, r: o.track_set(r[0], 1, [1.0, 1.0, 0.0], [1.0], _z(1, 9, 6)),
    "topay_track_commit_plan": lambda o, r: o.track_commit_plan(r, [0] * len(r)),
    "topay_track_get": lambda o, r: o.track_get(r[0]),
    "topay_track_clear": lambda o, r: o.track_clear(r[0]),
    "topay_track_safe": lambda o, r: o.track_safe(r, [0] * len(r)),
    "topay_replan_inputs": lambda o, r: o.replan_inputs(r, 0.0, 0.0, _z(len(r), 10), 0.1, 5.0),
    "topay_replan_calls": lambda o, r: o.replan_calls(r, [0] * len(r), 0.0, 0.0, _z(len(r), 10), 1.0, 0.1, 5.0),
    "topay_mpc_reset": lambda o, r: o.mpc_reset(r),
    "topay_mpc_set_direct": lambda o, r: o.mpc_set_direct(r),
    "topay_mpc_cmds": lambda o, r: o.mpc_cmds(r, 0.0, _z(len(r), 10)),
    "topay_mpc_probe": lambda o, r: o.mpc_probe(r[0], 0.0, _z(10), o.mpc_params()),
    "topay_mpc_get_state": lambda o, r: o.mpc_get_state(r[0]),
    "topay_sim_reset": lambda o, r: o.sim_reset(r, _z(len(r), 10)),
    "topay_sim_step": lambda o, r: o.sim_step(r, None, 0),
    "topay_track_follow": lambda o, r: o.track_follow(r, 0.0, 1),
}
_ONE_ROBOT = ("topay_track_set", "topay_track_get", "topay_track_clear", "topay_mpc_probe", "topay_mpc_get_state")


def _slot_cases():
    out = []
    for e in _MAP_ENTRIES:
        out += [(e, "map", "below"), (e, "map", "above")] + ([] if e in _FILLERS else [(e, "map", "empty")])
    for e in _ROBOT_ENTRIES:
        out += [(e, "robot", "below"), (e, "robot", "above")] + ([] if e in _ONE_ROBOT else [(e, "robot", "twice")])
    return out


def _run_slot_case(ctx, entry, kind, case):
    """(status, error text) of the call; a status of 0 comes with an empty text."""
    o, other = ctx
    try:
        if kind == "map":
            st = _MAP_ENTRIES[entry](o, other, {"below": -1, "above": MAX_MAPS, "empty": EMPTY_MAP}[case])
        else:
            st = _ROBOT_ENTRIES[entry](o, {"below": [-1], "above": [TRACK_SLOTS], "twice": [ROBOT, ROBOT]}[case])
    except api.TopayError as e:
        m = re.match(r"topay status (-?\d+): (.*)", str(e), flags=re.S)
        return int(m.group(1)), m.group(2)
    if isinstance(st, int) and st != 0:
        return st, o.L.topay_last_error().decode()
    return 0, ""


# The record: the status every case returned on commit 4d8ea03, the last one before the slot checks were gathered into
# check_map_slots and check_robot_slots, taken by running _run_slot_case there.  -1 INVALID_ARG, -3 NO_MAP, -4 NO_TRAJ.  Most
# entries answer a slot out of range with INVALID_ARG, an empty map slot with NO_MAP and a robot named twice with INVALID_ARG ...
_SLOT_STATUS = {c: {"below": -1, "above": -1, "empty": -3, "twice": -1}[c[2]] for c in _slot_cases()}
# ... and these do not: the batch upload and the map getters say NO_MAP for any slot they cannot serve; topay_track_commit_plan
# looks at the plan store first (this context has run no planning call: NO_TRAJ); the sweep and the endpoints take a robot twice.
for _e in ("topay_set_init_traj", "topay_get_map", "topay_get_map_fields", "topay_get_occupancy"):
    _SLOT_STATUS[(_e, "map", "below")] = _SLOT_STATUS[(_e, "map", "above")] = -3
for _c in ("below", "above", "twice"):
    _SLOT_STATUS[("topay_track_commit_plan", "robot", _c)] = -4
_SLOT_STATUS[("topay_track_safe", "robot", "twice")] = _SLOT_STATUS[("topay_replan_inputs", "robot", "twice")] = 0


@pytest.mark.parametrize("entry,kind,case", _slot_cases(), ids=lambda v: str(v))
def test_slot_checks_keep_their_status_codes(slot_ctx, entry, kind, case):
    status, text = _run_slot_case(slot_ctx, entry, kind, case)
    assert status == _SLOT_STATUS[(entry, kind, case)], (status, text)
    if status != 0:
        assert text and entry in text, (status, text)
