"""Time of S tables episodes at the benchmark map, generated on the device (topay_generate_episodes: device time by stage from
HIP events -- generation, rasterisation, fields, sampling -- and wall time) next to the parent path: wl.World(..., nthreads=-1)
for every episode on T host threads, the upload through topay_build_esdf_fields, then wl_sample_arm; and the bytes each uploads.

    python tools/episode_timing.py [S=1024] [threads=16] [--device-only]

--device-only: figure (a) alone (with TOPAY_LIB: of another build of the library).
"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from topay_amd import api
from harness import workload as wl

args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 1024
T = int(args[1]) if len(args) > 1 else 16
M = 0xFFFFFFFFFFFFFFFF
seeds = [42 + k for k in range(S)]
opt = api.MomaTrajOptBatch(device=0)
prm = api.world_params(wl.TABLES, lib=opt.L)
rows = []
for rep in range(4):                      # 1 warm-up + 3 timed
    t0 = time.perf_counter()
    start, goal, status, _ = opt.generate_episodes(prm, seeds)
    wall = (time.perf_counter() - t0) * 1e3
    if rep:
        rows.append(list(opt.world_stage_ms().values()) + [wall])
r = np.median(np.array(rows), axis=0)
print(f"(a) device: {S} episodes, generation {r[0]:.2f} ms, rasterisation {r[1]:.2f} ms, fields {r[2]:.2f} ms, sampler kernel {r[3]:.2f} ms, "
      f"call {r[4]:.1f} ms wall (median of 3); rasteriser path {opt.world_last_path()}; {int((status == 1).sum())} of {S} episodes sampled", flush=True)
if "--device-only" in sys.argv:
    sys.exit(0)

# (b) the parent path
ref = api.MomaTrajOptBatch(device=0)
t0 = time.perf_counter()
s3g3 = [wl.sample_start_goal_xy((sd * 1000) & M) for sd in seeds]
def occ(k):
    return wl.World(wl.TABLES, seed=(seeds[k] * 1000) & M, keepouts=[s3g3[k][0][:2], s3g3[k][1][:2]], nthreads=-1)
with ThreadPoolExecutor(T) as ex:
    worlds = list(ex.map(occ, range(S)))
t_host = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
w0 = worlds[0]
o2, o3 = np.stack([w.occ2d for w in worlds]), np.stack([w.occ3d for w in worlds])
t_stack = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
ref.build_esdf_batch(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, o2, o3)
t_up = (time.perf_counter() - t0) * 1e3
same = sum(int((opt.get_occupancy(k)[2] == worlds[k].occ3d).all()) for k in range(0, S, max(1, S // 16)))
# wl_sample_arm needs the CPU fields of every world: the harness builds them on one thread per world
t0 = time.perf_counter()
def arms(k):
    w = wl.World(wl.TABLES, seed=(seeds[k] * 1000) & M, keepouts=[s3g3[k][0][:2], s3g3[k][1][:2]], nthreads=1)
    g, s = np.zeros(10), np.zeros(10)
    s[:3], g[:3] = s3g3[k]
    ok1, g = w.sample_arm((seeds[k] * 7919) & M, g)
    ok2, s = w.sample_arm((seeds[k] * 7919 + 1) & M, s)
    w.close()
    return ok1 and ok2
with ThreadPoolExecutor(T) as ex:
    oks = list(ex.map(arms, range(S)))
t_arm = (time.perf_counter() - t0) * 1e3
print(f"(b) parent: occupancy of {S} worlds on {T} host threads {t_host:.0f} ms, packing {t_stack:.0f} ms, upload + fields (topay_build_esdf_batch) "
      f"{t_up:.0f} ms wall ({ref.get_map(0)[2]:.1f} ms of it the fields on the device); CPU fields + wl_sample_arm on {T} threads {t_arm:.0f} ms; "
      f"{sum(oks)} episodes sampled; sampled grids identical to the device's: {same} of {len(range(0, S, max(1, S // 16)))}")
print(f"(c) upload: device path {S * (8 + 4)} B of seeds and attempts (and {S * 164} B of results back); parent path {o2.nbytes + o3.nbytes} B of occupancy")
