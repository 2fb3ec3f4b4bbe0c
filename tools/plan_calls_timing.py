"""Time of topay_plan_calls next to the Python composition of the single entry points in its batched form.

S tables maps are built once (default 1024); then, in one process and alternating, `reps` times each (default 5):
  plan_calls   the whole planning call in one entry (api.plan_calls), with its per-stage device times (HIP events);
  composition  one topo_paths, one plan2d_jps, one dense_path, one mcrrt_plan and one solve per try, every intermediate
               result through the host (the instance numbers of the draws differ from plan_calls': timing only).
Prints one line per run and the medians.  Usage: plan_calls_timing.py [S] [reps]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topay_amd import api            # noqa: E402
from harness import workload as wl   # noqa: E402


def composition(opt, start, end, mid, prm, first_call):
    """The batched composition: returns the number of calls with a winner."""
    n = len(start)
    done = np.zeros(n, dtype=bool)
    thr = float(opt.opt_param.chassis_colli_radius) + prm.jps_margin
    for t in (0, 1):
        act = np.nonzero(~done)[0]
        if not len(act):
            break
        paths, _ = opt.topo_paths(start[act, :2], end[act, :2], prm.topo, map_ids=mid[act], critical=1 if t else None, first_instance=2 * first_call + t * n)
        if t == 0:
            jps, _, _ = opt.plan2d_jps(start[act, :2], end[act, :2], thr, map_ids=mid[act])
            for j in range(len(act)):
                if len(jps[j]):
                    paths[j].append(jps[j])
        call = np.array([act[j] for j in range(len(act)) for _ in paths[j][:prm.max_candidates]], dtype=np.int32)
        flat = [p for j in range(len(act)) for p in paths[j][:prm.max_candidates]]
        if not flat:
            continue
        dense, dl = opt.dense_path(flat, start[call, 2], end[call, 2], step_size=prm.dense_step)
        ok = [i for i in range(len(flat)) if 2 <= dl[i] <= 255]          # (what the search takes; plan_calls fails the others)
        if not ok:
            continue
        call, flat, dense, dl = call[ok], [flat[i] for i in ok], [dense[i] for i in ok], dl[ok]
        wbs, mst, _ = opt.mcrrt_plan(dl, np.concatenate(dense), start[call], end[call], prm.mcrrt, map_ids=mid[call], first_instance=16 * first_call + 8 * t * n)
        keep = [i for i in range(len(flat)) if mst[i, 0] == 1 and len(wbs[i]) >= 2]
        if not keep:
            continue
        opt.set_init_traj(np.array([len(wbs[i]) for i in keep], dtype=np.int32), np.concatenate([wbs[i] for i in keep]),
                          boundary_vel=np.zeros((len(keep), 20)), map_ids=mid[call[keep]])
        opt.set_groups(call[keep], cancel_budget=prm.cancel_budget)
        opt.optimize()
        opt.check_feasible()
        rec, win = opt.scenario_records(call[keep])
        w = [int(x) for r, x in zip(rec, win) if r["status"] == 1]
        if w:
            opt.getTrajs(w)
        for r in rec:
            if r["status"] == 1:
                done[int(r["scenario_id"])] = True
    return int(done.sum())


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    tb = wl.TablesBatch(S, 1, base_seed=2024, nthreads=0)
    worlds = [tb.world(s) for s in tb.scenarios]
    opt = api.MomaTrajOptBatch(device=0)
    w0 = worlds[0]
    opt.build_esdf_batch(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, np.stack([w.occ2d for w in worlds]), np.stack([w.occ3d for w in worlds]))
    offs = np.concatenate([[0], np.cumsum(tb.lens)])
    first = [int(np.nonzero(tb.scen == s_)[0][0]) for s_ in tb.scenarios]
    start = np.array([tb.paths[offs[b]] for b in first])
    end = np.array([tb.paths[offs[b + 1] - 1] for b in first])
    mid = np.arange(S, dtype=np.int32)
    prm = opt.plan_params()
    t_plan, t_comp = [], []
    for r in range(reps + 1):                              # (run 0 warms both paths up and is not counted)
        t0 = time.perf_counter()
        res, _, _ = opt.plan_calls(start, end, map_ids=mid, params=prm, first_call=0)
        opt.plan_trajs(np.arange(S))
        t1 = time.perf_counter()
        won = composition(opt, start, end, mid, prm, 0)
        t2 = time.perf_counter()
        print(f"run {r}: plan_calls {1e3 * (t1 - t0):.1f} ms ({int((res[:, 0] == 1).sum())} winners), composition {1e3 * (t2 - t1):.1f} ms ({won} winners)",
              flush=True)
        if r:
            t_plan.append(t1 - t0)
            t_comp.append(t2 - t1)
    # per-stage device times of one more plan_calls (the composition in between resets nothing they depend on)
    opt.plan_calls(start, end, map_ids=mid, params=prm, first_call=0)
    st = opt.plan_stage_ms()
    print(f"{S} calls, {reps} runs each: plan_calls median {1e3 * np.median(t_plan):.1f} ms, composition median {1e3 * np.median(t_comp):.1f} ms")
    print("plan_calls device time by stage (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in st.items()) + f"; sum {sum(st.values()):.1f}")
    tb.close()


if __name__ == "__main__":
    main()
