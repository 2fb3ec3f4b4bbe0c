"""Time of topay_track_sample_grid for n tracked trajectories x m samples, next to what did the same work before it.

n robots on one hand-made free map (80 x 80 x 20 cells of 0.1 m, one far corner occupied), each with a 3-piece quintic of
duration about m x 0.01 s from a start of its own, so that the safety sweep visits every sample.  Sampled on the sweep's own grid
t0 = 0, step = 0.01, m samples:

  1. kinematics only (state + dstate) and kinematics with the bodies (state, dstate, ee_pose, centres, distance, clearance):
     device time of the kernel (HIP events around the launch: topay_track_sample_ms) and the host's time around the call, which
     includes the copy of the outputs back; 3 warm-up and 10 timed calls each, the median with min and max.
  2. topay_track_safe on the same robots and map: device time of the sweep (topay_track_safe_ms), same repetitions.  What is
     expected and not asserted: the variant with the bodies on the sweep's grid costs the same order as the sweep.
  3. the per-call path that existed for states at given times of tracked trajectories: topay_replan_inputs, one time per
     robot per call, so m calls of n robots; the host's time around the m calls.
  4. identical results are asserted, not timed: sample j of the grid equals call j of step 3 bit for bit.

    python tools/track_sample_timing.py [n=256] [m=512]
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from topay_amd import api

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
m = int(sys.argv[2]) if len(sys.argv) > 2 else 512
ORIGIN, RES, DIMS = np.array([-4.0, -4.0, 0.0]), 0.1, np.array([80, 80, 20], dtype=np.int32)
o2, o3 = np.zeros((80, 80), dtype=np.int8), np.zeros((80, 80, 20), dtype=np.int8)
o2[79, 79] = 1
o3[79, 79, :] = 1
opt = api.MomaTrajOptBatch(device=0)
opt.build_esdf(ORIGIN, RES, DIMS, ORIGIN, ORIGIN + DIMS * RES, o2.reshape(-1), o3.reshape(-1), map_id=0)
T = m * 0.01 - 0.005
durs = np.array([T / 3, T / 3, T / 3])
co = np.zeros((3, 9, 6))
t0 = 0.0
for i, d in enumerate(durs):   # arc-length rate 1.5 / T (1.5 m in all), yaw rate 0.4 / T, joint rates 0.3 / T
    co[i, 0, 5], co[i, 0, 4] = 0.4 / T * t0, 0.4 / T
    co[i, 1, 5], co[i, 1, 4] = 1.5 / T * t0, 1.5 / T
    for k in range(7):
        co[i, 2 + k, 5], co[i, 2 + k, 4] = 0.1 * k * (k % 2) + 0.3 / T * t0, 0.3 / T
    t0 += d
robots = np.arange(n, dtype=np.int32)
for r in robots:
    opt.track_set(int(r), 1, [-2.0 + 0.5 * (r % 5), -2.0 + 4.0 * (r // 5) / max(1, n // 5), 0.0], durs, co)
maps = np.zeros(n, dtype=np.int32)
KIN = api.SAMPLE_STATE | api.SAMPLE_DSTATE
BODY = KIN | api.SAMPLE_EE_POSE | api.SAMPLE_CENTRES | api.SAMPLE_DISTANCE | api.SAMPLE_CLEARANCE
print(f"{n} robots x {m} samples = {n * m} samples; 3 pieces, duration {durs.sum():.3f} s", flush=True)


def timed(call, dev_ms):
    rows = []
    for rep in range(13):
        t_ = time.perf_counter()
        out = call()
        wall = (time.perf_counter() - t_) * 1e3   # (the entries return after a stream synchronise)
        if rep >= 3:
            rows.append((dev_ms(), wall))
    rows = np.array(rows)
    return out, rows


for name, what in (("kinematics only", KIN), ("kinematics and bodies", BODY)):
    got, rows = timed(lambda: opt.track_sample_grid(robots, 0.0, 0.01, m, map_ids=maps, what=what), opt.track_sample_ms)
    doubles = sum(int(np.prod(tail)) for _, bit, tail in api.SAMPLE_OUTPUTS if what & bit)
    print(f"track_sample_grid, {name}: kernel {np.median(rows[:, 0]):.3f} ms median of 10 (min {rows[:, 0].min():.3f}, max {rows[:, 0].max():.3f}), "
          f"call {np.median(rows[:, 1]):.3f} ms ({8 * doubles * n * m / 1e6:.1f} MB copied back); "
          f"{n * m / np.median(rows[:, 0]) / 1e3:.2f} M samples/s on the device", flush=True)
    if what == KIN:
        kin = got
(safe, fh, hit), rows = timed(lambda: opt.track_safe(robots, maps), opt.track_safe_ms)
print(f"track_safe on the same robots: kernel {np.median(rows[:, 0]):.3f} ms median of 10 (min {rows[:, 0].min():.3f}, max {rows[:, 0].max():.3f}), "
      f"call {np.median(rows[:, 1]):.3f} ms; {int(safe.sum())} of {n} safe", flush=True)
opt.replan_inputs(robots, 0.0, 0.0, np.zeros((n, 10)), 0.0, 1e9)   # warm-up
times, t = np.zeros(m), 0.0
for j in range(m):
    times[j] = t
    t += 0.01
st, sv = np.zeros((m, n, 10)), np.zeros((m, n, 10))
t_ = time.perf_counter()
for j in range(m):
    st[j], sv[j], _, _ = opt.replan_inputs(robots, times[j], 0.0, np.zeros((n, 10)), 0.0, 1e9)
wall = (time.perf_counter() - t_) * 1e3
print(f"replan_inputs, {m} calls of {n} robots (state + dstate at one time per robot and call): {wall:.1f} ms on the host's clock", flush=True)
same = (kin["state"].reshape(n, m, 10) == st.transpose(1, 0, 2)).all() and (kin["dstate"].reshape(n, m, 10) == sv.transpose(1, 0, 2)).all()
print("grid samples equal the per-call results bit for bit:", bool(same))
assert same
opt.close()
