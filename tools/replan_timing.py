"""Time of the replanning cycle for S tracked trajectories on S resident tables maps.

  1. topay_track_safe: device time (HIP events around the launch: topay_track_safe_ms), 3 warm-up and 10 timed sweeps, the
     median; once against the maps the trajectories were planned on (safe: every sample is visited) and once against the
     neighbouring scenario's map (first hits: the waves leave early).  Next to it the CPU restatement (harness/replan.hpp)
     on T host threads for the same sweeps, and how many verdicts / first hits are identical.
  2. one topay_replan_calls in which every robot triggers, next to topay_plan_calls on the same endpoints with the same
     call numbers: what the cycle adds should be the sweep, the endpoint kernel and the commit.

The trajectories are the winners of one topay_plan_calls over the S scenarios (default parameters); robot i tracks winner
i mod W when only W of the S calls have one.

    python tools/replan_timing.py [S=1024] [threads=16]
"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from topay_amd import api
from harness import workload as wl

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
tb = wl.TablesBatch(S, 1, base_seed=42, nthreads=T, keep_esdf3d=0)
opt = api.MomaTrajOptBatch(device=0)
w0 = tb.world(tb.scenarios[0])
CH = 128
for c0 in range(0, S, CH):
    ws = [tb.world(s_) for s_ in tb.scenarios[c0:c0 + CH]]
    opt.build_esdf_batch(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, np.stack([w.occ2d for w in ws]), np.stack([w.occ3d for w in ws]), first_map_id=c0)
offs = np.concatenate([[0], np.cumsum(tb.lens)])
start = tb.paths[offs[:-1]].copy()
goal = tb.paths[offs[1:] - 1].copy()
all_maps = np.arange(S, dtype=np.int32)
res, _, _ = opt.plan_calls(start, goal, map_ids=all_maps, first_call=0)
win = np.nonzero(res[:, 0] == 1)[0]
W = len(win)
if W == 0:
    sys.exit("no planning call has a winner")
robots = np.arange(S, dtype=np.int32)
call = win[np.arange(S) % W]
assert opt.track_commit_plan(robots, call, which=3).all()
trajs = {int(c): opt.track_get(int(robots[k]), 1) for k, c in enumerate(win)}
pieces = np.array([len(trajs[int(c)][1]) for c in call])
dur = np.array([trajs[int(c)][1].sum() for c in call])
print(f"{S} tracked trajectories ({W} winners of {S} calls): pieces {pieces.mean():.1f} mean / {pieces.max()} max, duration {dur.mean():.2f} s mean / "
      f"{dur.max():.2f} s max = {np.ceil(dur / 0.01).sum():.0f} samples in all", flush=True)


def restate(mid):
    """The restatement's sweeps on T threads, the fields fetched 64 maps at a time (outside the timing)."""
    out, cpu = [None] * S, 0.0
    refs = {c: wl.ReplanTraj(*tr) for c, tr in trajs.items()}
    for c0 in range(0, S, 64):
        ks = range(c0, min(c0 + 64, S))
        fields = {int(m): opt.get_map(int(m))[:2] for m in set(mid[c0:c0 + 64].tolist())}
        def one(k):
            return refs[int(call[k])].safe(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, *fields[int(mid[k])])
        t0 = time.perf_counter()
        with ThreadPoolExecutor(T) as ex:
            for k, r in zip(ks, ex.map(one, ks)):
                out[k] = r
        cpu += (time.perf_counter() - t0) * 1e3
    return out, cpu


for name, mid in (("the maps planned on", call.astype(np.int32)), ("the neighbouring maps", ((call + 1) % S).astype(np.int32))):
    ms = []
    for rep in range(13):
        t0 = time.perf_counter()
        safe, fh, hit = opt.track_safe(robots, mid)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 3:
            ms.append((opt.track_safe_ms(), wall))
    ms = np.array(ms)
    visited = np.where(safe, np.ceil(dur / 0.01), (fh[:, 0] // 64 + 1) * 64).sum()
    print(f"sweep against {name}: kernel {np.median(ms[:, 0]):.3f} ms median of 10 (min {ms[:, 0].min():.3f}, max {ms[:, 0].max():.3f}), call "
          f"{np.median(ms[:, 1]):.3f} ms; {int(safe.sum())} of {S} safe, about {visited:.0f} samples visited; {S / np.median(ms[:, 0]) * 1e3:.0f} robots/s", flush=True)
    ref, cpu = restate(mid)
    same = sum(int(bool(safe[k]) == ref[k]["safe"] and fh[k, 0] == ref[k]["sample"] and fh[k, 1] == ref[k]["body"]) for k in range(S))
    near = sum(int(ref[k]["min_margin"] < 1e-6) for k in range(S))
    print(f"  restatement on {T} threads: {cpu:.1f} ms = {S / cpu * 1e3:.0f} robots/s (Python call overhead included); verdict, sample and body "
          f"identical for {same} of {S} ({near} within 1e-6 of a threshold)", flush=True)

# ---- the cycle, every robot due, next to the planning call on the same endpoints
clock = np.full(S, 0.2)
budget, horizon = 0.1, 3.0
ends = opt.replan_inputs(robots, clock, clock, goal[call], budget, horizon)
t0 = time.perf_counter()
status, en, rres, _ = opt.replan_calls(robots, call.astype(np.int32), clock, clock, goal[call], 0.0, budget, horizon, first_call=1 << 20)
cyc = (time.perf_counter() - t0) * 1e3
cyc_stage = opt.plan_stage_ms()
sweep_ms = opt.track_safe_ms()
assert (status[:, 0] >= 1).all() and np.array_equal(en[:, 0], ends[0]) and np.array_equal(en[:, 2], ends[2])
t0 = time.perf_counter()
pres, _, _ = opt.plan_calls(ends[0], ends[2], map_ids=call.astype(np.int32), start_v=ends[1], first_call=1 << 20)
pln = (time.perf_counter() - t0) * 1e3
pln_stage = opt.plan_stage_ms()
print(f"cycle: replan_calls with {S} robots due {cyc:.1f} ms (its sweep {sweep_ms:.3f} ms on the device; {int((status[:, 0] == 1).sum())} committed, "
      f"{int((status[:, 0] == 2).sum())} without a winner); plan_calls on the same endpoints {pln:.1f} ms; the cycle adds {cyc - pln:.1f} ms; "
      f"result tables identical: {bool((pres[:, :7] == rres[:, :7]).all())}")
print("  device time by stage, cycle:     ", {k: round(v, 2) for k, v in cyc_stage.items()})
print("  device time by stage, plan_calls:", {k: round(v, 2) for k, v in pln_stage.items()})
tb.close()
opt.close()
