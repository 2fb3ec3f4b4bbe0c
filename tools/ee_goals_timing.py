#!/usr/bin/env python3
"""Time of topay_ee_goals: maps x seeds problems on resident tables maps, targets = getFKPose of sampled collision-free states.
Prints problems per second of the library (wall clock and topay_ee_ms) and of the CPU restatement on `threads` host threads,
and the spread of evals within a wave (the cost of the lock-step mapping).  usage: ee_goals_timing.py [maps] [seeds] [threads]"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from harness import workload as wl  # noqa: E402
from topay_amd import api  # noqa: E402


def main():
    n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    n_seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    opt = api.MomaTrajOptBatch(device=0)
    prm = api.world_params(0, lib=opt.L)
    built = 0
    while built < n_maps:   # resident maps in chunks of at most 256 slots
        m = min(256, n_maps - built)
        opt.generate_worlds(prm, np.arange(built, built + m) + 1000, first_map_id=built)
        built += m
    rng = np.random.default_rng(1)
    # targets: getFKPose of collision-free states, the goal of World::sampleScenario on every map (its arm is topay_sample_arm's)
    _, star, ok = opt.sample_scenarios(np.arange(n_maps) + 7, map_ids=np.arange(n_maps, dtype=np.int32))
    assert ok.all(), "a map without a scenario"
    ref = np.repeat(wl.EeGoal.pose(star), n_seeds, axis=0)
    seed = np.repeat(star, n_seeds, axis=0) + 0.05 * rng.uniform(-1, 1, (n_maps * n_seeds, 10))
    mid = np.repeat(np.arange(n_maps, dtype=np.int32), n_seeds)
    jmax = np.array([opt.opt_param.joint_pos_limit_max[q] for q in range(7)])
    seed[:, 3:] = np.clip(seed[:, 3:], -0.999 * jmax, 0.999 * jmax)   # a seed joint at its limit has no unconstrained image
    n = len(seed)
    opt.ee_goals(seed[:64], ref[:64], mid[:64])   # warm-up
    t0 = time.perf_counter()
    st, cost, code, it, ev = opt.ee_goals(seed, ref, mid)
    wall = time.perf_counter() - t0
    ms = opt.ee_ms()
    waves = [ev[k:k + 64] for k in range(0, n, 64)]
    spread = np.array([w.max() / max(1.0, w.mean()) for w in waves])
    out = dict(problems=n, wall_s=wall, device_ms=ms, problems_per_s_wall=n / wall, problems_per_s_device=n / (ms * 1e-3),
               success=float(np.isin(code, (0, 1, 2, -1008)).mean()), evals_mean=float(ev.mean()), evals_max=int(ev.max()),
               wave_max_over_mean_evals_median=float(np.median(spread)), wave_max_over_mean_evals_worst=float(spread.max()))
    m_cpu = min(n, 512)   # the restatement on a sample of the problems
    refs = {}

    def one(k):
        s = int(mid[k])
        if s not in refs:
            e2, e3, _ = opt.get_map(s)
            org = np.array([-10.0, -10.0, 0.0])
            dims = np.array([200, 200, 16], dtype=np.int32)
            refs[s] = wl.EeGoal(org, 0.1, dims, org, org + dims * 0.1, e2, e3)
        return refs[s].optimize(seed[k], ref[k])[4]

    for k in range(0, m_cpu, n_seeds):
        one(k)   # fields fetched outside the timed part
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(m_cpu)))
    out["restatement_problems_per_s"] = m_cpu / (time.perf_counter() - t0)
    out["restatement_threads"] = threads
    print(json.dumps(out))


if __name__ == "__main__":
    main()
