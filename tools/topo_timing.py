"""Time of topay_topo_paths for S queries on S resident tables maps (3 warm-up, 10 timed calls, HIP events around the
kernel: topay_last_kernel_ms) next to the CPU restatement (harness/topo_prm.hpp) on 16 host threads for the same queries.

    python tools/topo_timing.py [S=1024] [threads=16]
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
for c0 in range(0, len(tb.scenarios), CH):
    ws = [tb.world(s_) for s_ in tb.scenarios[c0:c0 + CH]]
    opt.build_esdf_batch(w0.origin, w0.res, w0.dims, w0.min_b, w0.max_b, np.stack([w.occ2d for w in ws]), np.stack([w.occ3d for w in ws]), first_map_id=c0)
offs = np.concatenate([[0], np.cumsum(tb.lens)])
n = len(tb.scenarios)
st = tb.paths[offs[:-1], :2].copy()
en = tb.paths[offs[1:] - 1, :2].copy()
mid = np.arange(n, dtype=np.int32)
prm = opt.topo_params(seed=42)
ms = []
for rep in range(13):
    t0 = time.perf_counter()
    paths, stats = opt.topo_paths(st, en, prm, map_ids=mid)
    wall = (time.perf_counter() - t0) * 1e3
    k_ms, _ = opt.last_kernel_ms()
    if rep >= 3:
        ms.append((k_ms, wall))
ms = np.array(ms)
ok = stats[:, 0] >= 0
print(f"device: {n} queries, kernel {np.median(ms[:, 0]):.2f} ms median of 10 (min {ms[:, 0].min():.2f}, max {ms[:, 0].max():.2f}), call {np.median(ms[:, 1]):.2f} ms; "
      f"{n / np.median(ms[:, 0]) * 1e3:.0f} queries/s; samples/query {stats[ok, 1].mean():.0f} ({stats[ok, 2].mean():.0f} past the clearance test), "
      f"nodes {stats[ok, 3].mean():.1f} -> {stats[ok, 4].mean():.1f}, raw paths {stats[ok, 5].mean():.1f}, selected {stats[ok, 7].mean():.2f}; "
      f"status 1 / 0 / -1 / -2: {[int((stats[:, 0] == v).sum()) for v in (1, 0, -1, -2)]}", flush=True)
fields = [opt.get_map_fields(k) for k in range(n)]
hp = wl.TopoParams(seed=42)
def one(k):
    return wl.topo_paths(tb.world(tb.scenarios[k]), st[k], en[k], hp, inst=k, track_slack=False, fields=fields[k])["stats"]
t0 = time.perf_counter()
with ThreadPoolExecutor(T) as ex:
    ref = list(ex.map(one, range(n)))
cpu = (time.perf_counter() - t0) * 1e3
same = sum(int(list(ref[k]) == list(stats[k])) for k in range(n))
print(f"restatement: {n} queries on {T} threads in {cpu:.1f} ms = {n / cpu * 1e3:.0f} queries/s (Python call overhead included); counters identical for {same} of {n}")
