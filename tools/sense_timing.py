#!/usr/bin/env python3
"""Time of the sensor-cloud entries: `slots` map slots, each with one 64 x 16-ray scan of its own tables world inserted into an
empty belief and committed.  Prints the four stage times of topay_sense_ms (scan, insert, flush, commit with the fields), the wall
time of the three calls, and beside them the time of the CPU checker (harness/prob_map.hpp: update and the occupancy grids, no
fields) for the same clouds on `threads` host threads.  usage: sense_timing.py [slots] [size_xy] [threads]"""
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    size_xy = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    opt = api.MomaTrajOptBatch(device=0)
    prm = api.world_params(0, size_xy=size_xy, lib=opt.L)
    truth = np.arange(n, dtype=np.int32) + n   # the worlds in slots n .. 2n - 1, the beliefs in 0 .. n - 1
    opt.generate_worlds(prm, np.arange(n) + 1000, first_map_id=n)
    dims = opt._map_dims[n]
    org = np.array([-size_xy / 2, -size_xy / 2, 0.0])
    grid = dict(origin=org, res=prm.resolution, dims=dims, min_b=org, max_b=org + np.array(dims) * prm.resolution)
    belief = np.arange(n, dtype=np.int32)
    poses = np.tile(np.array([0.0, 0.0, 0.5, 0.0]), (n, 1))
    sp = opt.sense_params(point_filt_num=1)
    out = dict(slots=n, dims=list(dims), rays_per_slot=64 * 16)
    for rep in ("warmup", "timed"):
        opt.sense_reset(belief, **grid)
        t0 = time.perf_counter()
        off, _ = opt.sense_scan(truth, poses, 64, 16, 1.0, 5.0, copy_back=False)
        t1 = time.perf_counter()
        st = opt.sense_insert(belief, api.SENSE_LAST_SCAN, poses[:, :3], sp, cloud_off=off)
        t2 = time.perf_counter()
        opt.sense_commit(belief)
        t3 = time.perf_counter()
        assert (st == 1).all()
    out["device_ms"] = opt.sense_ms()
    out["wall_ms"] = dict(scan=1e3 * (t1 - t0), insert=1e3 * (t2 - t1), commit=1e3 * (t3 - t2))
    _, pts = opt.sense_scan(truth, poses, 64, 16, 1.0, 5.0)
    out["occupied_voxels_mean"] = float(np.mean([opt.get_occupancy(int(m))[2].sum() for m in belief[:8]]))

    def one(k):
        pm = wl.ProbMapCheck(grid["origin"], grid["res"], grid["dims"])
        pm.update(pts[k], poses[k, :3], sp)
        return int(pm.occupancy(sp)[2].sum())

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        occ = list(ex.map(one, range(n)))
    out["checker_ms"] = 1e3 * (time.perf_counter() - t0)
    out["checker_threads"] = threads
    out["checker_occupied_voxels_mean"] = float(np.mean(occ[:8]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
