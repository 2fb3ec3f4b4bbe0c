#!/usr/bin/env python3
"""Time of topay_sense_slide beside the commit that follows it: `slots` beliefs of 200 x 200 x 16 voxels (the shipped 20 x 20 x 1.6 m
map at 0.1 m), each with one random cloud inserted, slid by (3, -2, 0) voxels in one call and then committed.  Prints the median
over 20 calls after 3 warm-up calls of topay_sense_slide_ms and of entry [3] of topay_sense_ms (the commit with its fields), their
ratio, and the slide's traffic (4 bytes read and 4 written per voxel by k_sense_slide, the same again by the copy back) over its
time as a fraction of the 6.3 TB/s a streaming copy reaches on this part.  usage: sense_slide_timing.py [slots]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topay_amd import api  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s
DIMS, RES, SHIFT = (200, 200, 16), 0.1, (3, -2, 0)
WARMUP, CALLS = 3, 20


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    opt = api.MomaTrajOptBatch(device=0)
    org = np.array([-10.0, -10.0, 0.0])
    slots = np.arange(n, dtype=np.int32)
    opt.sense_reset(slots, origin=org, res=RES, dims=DIMS, min_b=org, max_b=org + np.array(DIMS) * RES)
    r = np.random.default_rng(1)
    clouds = [np.concatenate([r.uniform(-9.0, 9.0, (2000, 2)), r.uniform(0.0, 1.5, (2000, 1)), np.zeros((2000, 1))], axis=1).astype(np.float32) for _ in slots]
    assert (opt.sense_insert(slots, clouds, np.tile([0.05, 0.05, 0.5], (n, 1)), opt.sense_params(point_filt_num=1, ray_range=[0.0, 20.0])) == 1).all()
    sp = opt.sense_slide_params(threshold=0.0)
    slide_ms, commit_ms = [], []
    for it in range(WARMUP + CALLS):
        origin = opt.sense_desc(0)[0]
        sensor = origin + (np.array(DIMS) // 2 + np.array(SHIFT) + 0.5) * RES
        st, sh = opt.sense_slide(slots, np.tile(sensor, (n, 1)), sp)
        assert (st == 1).all() and (sh == np.array(SHIFT)).all(), (st, sh)
        opt.sense_commit(slots)
        if it >= WARMUP:
            slide_ms.append(opt.sense_slide_ms())
            commit_ms.append(opt.sense_ms()["commit"])
    voxels = n * DIMS[0] * DIMS[1] * DIMS[2]
    s, c = float(np.median(slide_ms)), float(np.median(commit_ms))
    out = dict(slots=n, dims=list(DIMS), shift=list(SHIFT), calls=CALLS, warmup=WARMUP, slide_ms=s, slide_ms_min_max=[min(slide_ms), max(slide_ms)],
               commit_ms=c, commit_ms_min_max=[min(commit_ms), max(commit_ms)], slide_over_commit=s / c, slide_bytes=16 * voxels,
               slide_fraction_of_hbm=16 * voxels / (s * 1e-3) / HBM_ACHIEVABLE)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
