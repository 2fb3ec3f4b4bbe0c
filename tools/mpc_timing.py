#!/usr/bin/env python3
"""Time of the tracking controller on the device: mpc_timing.py [robots] [periods] [threads].

`robots` robot slots (default 4096) at the shipped ompc/ configuration follow one three-piece trajectory each from a start state a
few centimetres off it.  Printed: device time (topay_mpc_ms) of one topay_mpc_cmds and, per period, of one topay_track_follow of
`periods` periods (default 10); the distributions of outer iterations and QP steps per command, and max over mean within the
launch; the time of the CPU checker (harness/ompc.hpp) for the first period of 64 of the robots on `threads` host threads
(default 16), scaled to all.  The figures of docs/EXPERIMENTS.md "Tracking controller"."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from harness import workload as wl   # noqa: E402
from topay_amd import api            # noqa: E402


def traj(kind):
    durs = [[0.8, 0.7, 0.9], [0.5, 1.1, 0.6], [1.0, 0.4, 0.7]][kind]
    v, omega, th0 = [(0.5, 0.5, 3.0), (0.4, -0.3, 3.2), (0.6, 0.8, 2.9)][kind]
    co = np.zeros((3, 9, 6))
    t0 = 0.0
    for i, T in enumerate(durs):
        co[i, 0, 5], co[i, 0, 4] = th0 + omega * t0, omega
        co[i, 1, 5], co[i, 1, 4] = v * t0, v
        t0 += T
    return np.array([0.0, 0.0, th0]), np.array(durs), co


def dist(name, a):
    a = np.asarray(a, dtype=np.float64)
    print(f"  {name}: min {a.min():.0f}  median {np.median(a):.0f}  mean {a.mean():.1f}  p99 {np.percentile(a, 99):.0f}  max {a.max():.0f}  max/mean {a.max() / a.mean():.2f}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    periods = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    opt = api.MomaTrajOptBatch(device=0)
    P = opt.mpc_params()
    robots = list(range(n))
    rng = np.random.default_rng(7)
    for r in robots:
        opt.track_set(r, 1, *traj(r % 3))
    st, _, _, _ = opt.replan_inputs(robots, 0.0, 0.0, np.zeros((n, 10)), 0.0, 1e9)
    s0 = st.copy()
    s0[:, :2] += rng.uniform(-0.08, 0.08, (n, 2))
    s0[:, 2] += rng.uniform(-0.05, 0.05, n)
    opt.mpc_reset(robots, P)
    cmd, status, _ = opt.mpc_cmds(robots, 0.0, s0)
    print(f"{n} robots, shipped configuration (predict_steps {P.predict_steps}, delays {P.delay_num_v} / {P.delay_num_w}), qp_rho {P.qp_rho}")
    print(f"topay_mpc_cmds, first period (output and FIFO zero): {opt.mpc_ms():.2f} ms device time")
    dist("outer iterations", status[:, 1])
    dist("QP steps per command", status[:, 2])
    print(f"  commands with an unsolved QP: {(status[:, 0] == 3).sum()}")
    opt.mpc_reset(robots, P)
    opt.sim_reset(robots, s0, P.delay_num_v)
    _, _, ss = opt.track_follow(robots, 0.0, periods, 2)
    ms = opt.mpc_ms()
    print(f"topay_track_follow, {periods} periods: {ms:.2f} ms device time, {ms / periods:.2f} ms per period")
    dist("outer iterations", ss[:, :, 1])
    dist("QP steps per command", ss[:, :, 2])
    dist("QP steps per robot over the launch", ss[:, :, 2].sum(axis=1))
    # the checker, first period
    m = min(n, 64)
    rows = []
    for r in range(m):
        t, ts = P.dt, []
        for _ in range(P.predict_steps):
            ts.append(t)
            t += P.dt
        rs, _, _, _ = opt.replan_inputs([r] * len(ts), np.array(ts), 0.0, np.zeros((len(ts), 10)), 0.0, 1e9)
        rows.append(rs[:, :3].copy())
    chk = [wl.OmpcCheck(P) for _ in range(m)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda r: chk[r].cmd(0.0, s0[r], rows[r], None, None, 10.0), range(m)))
    dt = time.perf_counter() - t0
    print(f"checker, {m} robots on {threads} threads: {1e3 * dt:.1f} ms, i.e. {1e3 * dt * n / m:.0f} ms for {n}; {1e3 * dt * threads / m:.2f} ms per robot and thread")
    opt.close()


if __name__ == "__main__":
    main()
