"""The tracking controller and the fake robot: topay_mpc_* == OMPC (planner/src/ompc.cpp), topay_sim_* == moma_sim
(fake_moma/src/moma_sim.cpp:208-229, 251-308), topay_track_follow == both, period after period, in one launch.

Checker: harness/ompc.hpp (wl.OmpcCheck, wl.SimCheck), a serial CPU restatement.  It is handed getState's rows from the library's
own playback (topay_replan_inputs with a zero budget), so what is compared is the controller alone, and every comparison against
it is bit for bit: the library's solver and the checker's state the same expression for every number.

The QP solution is also checked without the checker, with numpy on the probed dense matrices, against OSQP's termination
criterion at eps_abs = eps_rel = 1e-6 with a factor 2 (the recomputation in another summation order moves a residual by about
1e-15, ten orders below the criterion):
    |A x - clip(A x, l, u)|_inf <= 2 (eps + eps max(|A x|, |z|)),    |P x + q + A' y|_inf <= 2 (eps + eps max(|P x|, |A' y|, |q|)).
The solver's own z is a clip result, so l <= z <= u holds exactly, and y obeys the sign rule at that z exactly (y_i > 0 only where
z_i = u_i, y_i < 0 only where z_i = l_i).  z differs from clip(A x) by no more than the primal criterion: an ADMM iterate has A x
within that distance of the box, not on its face, so the sign rule at clip(A x) itself is not a property any first-order method
has, and it is asserted at z with |z - clip(A x)| bounded by the same factor 2.
"""
import os
import re

import numpy as np
import pytest

from conftest import EMU_LIB
from harness import workload as wl
from topay_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["topay_mpc_default_params", "topay_mpc_qp_dims", "topay_mpc_reset", "topay_mpc_set_direct", "topay_mpc_cmds", "topay_mpc_probe",
               "topay_mpc_get_state", "topay_mpc_ms", "topay_sim_reset", "topay_sim_step", "topay_track_follow"]
CFGS = [(6, 2, 2), (8, 4, 2), (50, 20, 20)]
SMALL = CFGS[:2]
PERIODS = 10
PROBE_AT = 5          # the period whose first QP is probed: output and FIFO are non-zero by then
ROBOTS = [3, 700, 4095]
EPS = 1e-6


def _traj(kind):
    """Three pieces ([N, 9, 6], coefficient of t^5 first); the yaw 3.0 + omega t crosses pi within the first second."""
    durs = [[0.8, 0.7, 0.9], [0.5, 1.1, 0.6], [1.0, 0.4, 0.7]][kind]
    v, omega, th0 = [(0.5, 0.5, 3.0), (0.4, -0.3, 3.2), (0.6, 0.8, 2.9)][kind]
    co = np.zeros((3, 9, 6))
    t0 = 0.0
    for i, T in enumerate(durs):
        co[i, 0, 5], co[i, 0, 4] = th0 + omega * t0, omega
        co[i, 1, 5], co[i, 1, 4], co[i, 1, 2] = v * t0, v, 0.01 * (i + 1)
        for k in range(7):
            co[i, 2 + k, 5], co[i, 2 + k, 4] = 0.1 * k + 0.05 * t0, 0.05
        t0 += T
    return np.array([0.3 * kind, -0.2 * kind, th0]), np.array(durs), co


def _params(opt, cfg, **kw):
    # max_accel 0.3: the robot starts 8 cm behind its reference, so the first QPs run into the rate rows and the continuity bound
    kw.setdefault("max_accel", 0.3)
    return opt.mpc_params(predict_steps=cfg[0], delay_num_v=cfg[1], delay_num_w=cfg[2], **kw)


def _states(opt, robot, times):
    """getState / getDState of the slot's end_traj at `times`, from the library's playback."""
    t = np.ascontiguousarray(times, dtype=np.float64)
    st, sv, _, _ = opt.replan_inputs([robot] * len(t), t, 0.0, np.zeros((len(t), 10)), 0.0, 1e9)
    return st, sv


def _row_times(t_cur, P):
    out, t = [], t_cur + P.dt
    for _ in range(P.predict_steps):
        out.append(t)
        t += P.dt
    return out


def _now(opt, robot, t, kind):
    """The robot a few centimetres off its trajectory."""
    st, _ = _states(opt, robot, [t])
    s = st[0].copy()
    s[0] -= 0.08 * np.cos(s[2]) + 0.02 * kind
    s[1] -= 0.08 * np.sin(s[2]) - 0.03
    s[2] += 0.04 - 0.03 * kind
    return s


def _setup(opt, cfg, robots=ROBOTS, **kw):
    P = _params(opt, cfg, **kw)
    opt.mpc_reset(robots, P)
    Ts = []
    for i, r in enumerate(robots):
        s3, d, c = _traj(i % 3)
        opt.track_set(r, 1, s3, d, c)
        Ts.append(float(np.sum(d)))
    return P, Ts


def _clock(P, t0, periods):
    out, t = [], t0
    for _ in range(periods):
        out.append(t)
        t = t + 1.0 / P.ctrl_freq
    return out


def _episode(opt, cfg, periods=PERIODS):
    """PERIODS commands for the three robots in one call each, a probe at PROBE_AT, the slots' state at the end."""
    P, Ts = _setup(opt, cfg)
    E = dict(P=P, Ts=Ts, cmd=[], status=[], xopt=[], now=[], t=_clock(P, 0.1, periods), probe=None)
    for p, t in enumerate(E["t"]):
        now = np.stack([_now(opt, r, t, i) for i, r in enumerate(ROBOTS)])
        if p == PROBE_AT:
            before = opt.mpc_get_state(ROBOTS[0])
            E["probe"] = opt.mpc_probe(ROBOTS[0], t, now[0], P)
            after = opt.mpc_get_state(ROBOTS[0])
            assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2])), "the probe touched the slot"
        cmd, st, xo = opt.mpc_cmds(ROBOTS, t, now, want_xopt=True)
        E["cmd"].append(cmd); E["status"].append(st); E["xopt"].append(xo); E["now"].append(now)
    E["state"] = [opt.mpc_get_state(r) for r in ROBOTS]
    return E


def _checker_episode(opt, E):
    """The same episode through harness/ompc.hpp (opt supplies the playback only)."""
    P = E["P"]
    C = dict(cmd=[], status=[], xopt=[], probe=None)
    chk = [wl.OmpcCheck(P) for _ in ROBOTS]
    for p, t in enumerate(E["t"]):
        cmds, sts, xos = [], [], []
        for i, r in enumerate(ROBOTS):
            rows, _ = _states(opt, r, _row_times(t, P))
            a, da = _states(opt, r, [t + 1.0 / P.ctrl_freq])
            if p == PROBE_AT and i == 0:
                C["probe"] = chk[i].probe(t, E["now"][p][i], rows[:, :3], E["Ts"][i])
            cmd, st, xo = chk[i].cmd(t, E["now"][p][i], rows[:, :3], a[0, 3:], da[0, 3:], E["Ts"][i])
            cmds.append(cmd); sts.append(st); xos.append(xo)
        C["cmd"].append(np.stack(cmds)); C["status"].append(np.stack(sts)); C["xopt"].append(np.stack(xos))
    C["state"] = [c.get() for c in chk]
    return C


def _same_episode(A, B, T, maxd, b_is_checker):
    for p in range(len(A["cmd"])):
        assert np.array_equal(A["cmd"][p], B["cmd"][p]), ("cmd", p, np.abs(A["cmd"][p] - B["cmd"][p]).max())
        assert np.array_equal(A["status"][p], B["status"][p]), ("status", p, A["status"][p], B["status"][p])
        assert np.array_equal(A["xopt"][p][:, :T + 1], B["xopt"][p][:, :T + 1]), ("xopt", p)
    for sa, sb in zip(A["state"], B["state"]):
        assert np.array_equal(sa[0][:, :T], sb[0][:, :T]) and np.array_equal(sa[1][:maxd], sb[1][:maxd]), "output / FIFO"
    for k in ("P", "q", "A", "l", "u", "x", "y", "z"):
        assert np.array_equal(A["probe"][k], B["probe"][k]), ("probe", k)
    assert A["probe"]["iters"] == B["probe"]["iters"] and A["probe"]["solved"] == B["probe"]["solved"] == 1
    return True


@pytest.fixture(scope="module")
def emu():
    opt = api.MomaTrajOptBatch(device=0, lib_path=EMU_LIB)
    yield opt
    opt.close()


_EPISODES = {}


def _emu_episode(emu, cfg):
    if cfg not in _EPISODES:
        E = _episode(emu, cfg)
        _EPISODES[cfg] = (E, _checker_episode(emu, E))
    return _EPISODES[cfg]


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite (lane emulator)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_qp_construction_and_commands_match_the_checker(emu, cfg):
    """1 and 3: the probed P, q, A, l, u equal the checker's restatement of solveMPCDiff (both delay branches, the continuity
    bound on row 0), and ten periods of cmd, status, output, FIFO and xopt equal the checker's, bit for bit; the arm columns are
    getState / getDState of the tracked trajectory."""
    E, C = _emu_episode(emu, cfg)
    P = E["P"]
    assert _same_episode(E, C, cfg[0], max(cfg[1:]), True)
    out, fifo, mode = E["state"][0]
    assert np.abs(out).max() > 0 and np.abs(fifo).max() > 0 and mode == 0
    pr = E["probe"]
    dimv = cfg[0] - cfg[1]
    assert pr["l"][0] > P.min_speed and pr["u"][0] < P.max_speed and pr["u"][0] - pr["l"][0] == pytest.approx(2 * P.max_accel * P.dt)
    assert np.all(pr["l"][1:dimv] == P.min_speed)
    for p, t in enumerate(E["t"]):
        for i, r in enumerate(ROBOTS):
            a, da = _states(emu, r, [t + 1.0 / P.ctrl_freq])
            assert np.array_equal(E["cmd"][p][i, 2:9], a[0, 3:]) and np.array_equal(E["cmd"][p][i, 9:], da[0, 3:])
    assert all((st[:, 0] == 0).all() and (st[:, 1] >= 1).all() for st in E["status"])


@pytest.mark.parametrize("cfg", CFGS)
def test_qp_solution_meets_the_criterion(emu, cfg):
    """2: numpy on the probed matrices, independent of the checker (the module docstring states the bounds)."""
    pr = _emu_episode(emu, cfg)[0]["probe"]
    P, q, A, l, u, x, y, z = (pr[k] for k in ("P", "q", "A", "l", "u", "x", "y", "z"))
    assert pr["solved"] == 1 and np.array_equal(P, P.T)
    ax = A @ x
    zc = np.clip(ax, l, u)
    prim = np.abs(ax - zc).max()
    eps_p = EPS + EPS * max(np.abs(ax).max(), np.abs(zc).max())
    dual = np.abs(P @ x + q + A.T @ y).max()
    eps_d = EPS + EPS * max(np.abs(P @ x).max(), np.abs(A.T @ y).max(), np.abs(q).max())
    print(f"cfg {cfg}: iters {pr['iters']} prim {prim:.3e} / {eps_p:.3e} dual {dual:.3e} / {eps_d:.3e}")
    assert prim <= 2 * eps_p and dual <= 2 * eps_d
    assert np.all(z >= l) and np.all(z <= u) and np.abs(z - zc).max() <= 2 * eps_p
    assert np.all(z[y > 0] == u[y > 0]) and np.all(z[y < 0] == l[y < 0])
    T, dv, dw = cfg
    mx, my = (T - dv) + (T - dw), 3 * (T - dw)
    if cfg == CFGS[0]:   # the case chosen so that limits bind: an active box row and an active rate row
        assert np.any(y[:mx] != 0), "no active box row"
        assert np.any(y[mx + my:] != 0), "no active rate row"


def test_independence(emu):
    """4: a robot's result depends neither on its position in the call nor on the others."""
    cfg = CFGS[1]
    res = {}
    for order in ([0, 1, 2], [2, 0, 1], [1]):
        P, _ = _setup(emu, cfg)
        rb = [ROBOTS[i] for i in order]
        for t in _clock(P, 0.1, 3):
            now = np.stack([_now(emu, ROBOTS[i], t, i) for i in order])
            cmd, st, xo = emu.mpc_cmds(rb, t, now, want_xopt=True)
        for k, i in enumerate(order):
            res.setdefault(i, []).append((cmd[k], st[k], xo[k], emu.mpc_get_state(ROBOTS[i])[0]))
    for i, runs in res.items():
        for other in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0], other)), i


def _sim_facts(opt):
    """5: zero chassis motion for the first delay_cmds commands, command k applied at k + delay_cmds, normyaw's single wrap."""
    delay = 3
    s0 = np.array([[0.5, -0.2, 3.1, 0, 0, 0, 0, 0, 0, 0], [0.0, 0.0, -3.1, 0, 0, 0, 0, 0, 0, 0]])
    rb = [10, 11]
    opt.sim_reset(rb, s0, delay)
    chk = [wl.SimCheck(s0[i], delay) for i in range(2)]
    assert np.array_equal(opt.sim_step(rb, None, 5), s0), "moved before the first command"
    states = []
    for k in range(8):
        cmd = np.zeros((2, 16))
        cmd[:, 0], cmd[0, 1], cmd[1, 1] = 0.1 * (k + 1), 0.9 * (k + 1), -0.9 * (k + 1)
        cmd[:, 2:9] = 0.01 * k
        st = opt.sim_step(rb, cmd, 2)
        ref = np.stack([chk[i].step(cmd[i], 2) for i in range(2)])
        assert np.array_equal(st, ref), k
        states.append(st)
    states = np.stack(states)
    assert np.array_equal(states[:delay, :, :3], np.broadcast_to(s0[:, :3], (delay, 2, 3))), "chassis moved before delay_cmds commands"
    assert np.array_equal(states[:, :, 3:], np.broadcast_to((0.01 * np.arange(8))[:, None, None], (8, 2, 7))), "arm is not cmd.q"
    # command 0 (v 0.1, w 0.9) acts in step `delay`: two ticks of 0.01 s
    d = states[delay, 0] - states[delay - 1, 0]
    # (two ticks of 0.001 m with a turn of 0.009 rad between them)
    assert abs(np.hypot(d[0], d[1]) - 0.002 * np.cos(0.0045)) < 1e-12
    th = states[:, 0, 2]
    assert th[delay] == pytest.approx(3.1 + 0.9 * 0.02) and th.min() < -3.0 and np.all(np.abs(th) <= np.pi + 0.2)   # wrapped once, to the other side
    assert states[:, 1, 2].max() > 3.0
    return states


def test_simulator(emu):
    _sim_facts(emu)


def _follow_case(opt, cfg, periods, robots=ROBOTS):
    """6: topay_track_follow == the same sequence of single calls."""
    P, _ = _setup(opt, cfg, robots)
    s0 = np.stack([_now(opt, r, 0.0, i % 3) for i, r in enumerate(robots)])
    opt.sim_reset(robots, s0, cfg[1])
    st, cm, ss = opt.track_follow(robots, 0.05, periods, 2)
    follow_state = [opt.mpc_get_state(r) for r in robots]
    _setup(opt, cfg, robots)
    opt.sim_reset(robots, s0, cfg[1])
    now = s0
    for p, t in enumerate(_clock(P, 0.05, periods)):
        cmd, stat, _ = opt.mpc_cmds(robots, t, now)
        now = opt.sim_step(robots, cmd, 2)
        assert np.array_equal(cmd, cm[:, p]) and np.array_equal(stat, ss[:, p]) and np.array_equal(now, st[:, p]), p
    for a, r in zip(follow_state, robots):
        b = opt.mpc_get_state(r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return st, cm, ss


def test_follow_equals_steps(emu):
    st, cm, ss = _follow_case(emu, CFGS[0], 20)
    assert np.abs(cm[:, :, 0]).max() > 0 and np.abs(st[:, -1, :2] - st[:, 0, :2]).max() > 0


def test_closed_loop_reaches_the_goal(emu):
    """7: the small configuration, a robot following trajectory 0 from its start state through the simulator (actuator delay =
    delay_num_v commands), at the reference's max_accel: at_goal at the first period with t_cur >= T + 1.0, within 0.5 m (planner.cpp:649) of the trajectory's
    end.  The same loop through the checker gives the same commands."""
    cfg = CFGS[0]
    r = ROBOTS[0]
    P, Ts = _setup(emu, cfg, [r], max_accel=0.8)   # the reference's limits
    s3, d, c = _traj(0)
    end, _ = _states(emu, r, [Ts[0]])
    s0 = np.concatenate([s3, c[0, 2:, 5]])
    periods = int(np.ceil((Ts[0] + 1.0) * P.ctrl_freq)) + 2
    emu.sim_reset([r], s0[None], cfg[1])
    st, cm, ss = emu.track_follow([r], 0.0, periods, 2)
    ts = np.array(_clock(P, 0.0, periods))
    first = int(np.argmax(ts >= Ts[0] + 1.0))
    assert (ss[0, :first, 0] == 0).all() and (ss[0, first:, 0] == 1).all()
    dist = np.hypot(*(st[0, first, :2] - end[0, :2]))
    print(f"closed loop: {first} periods, {dist:.3f} m from the end, outer max {ss[0, :, 1].max()}, qp steps max {ss[0, :, 2].max()}")
    assert dist < 0.5
    chk, sim, now = wl.OmpcCheck(P), wl.SimCheck(s0, cfg[1]), s0
    for p in range(0, first + 1, 1):
        rows, _ = _states(emu, r, _row_times(ts[p], P))
        a, da = _states(emu, r, [ts[p] + 1.0 / P.ctrl_freq])
        cmd, stat, _ = chk.cmd(ts[p], now, rows[:, :3], a[0, 3:], da[0, 3:], Ts[0])
        assert np.array_equal(cmd, cm[0, p]) and np.array_equal(stat, ss[0, p]), p
        now = sim.step(cmd, 2)
        assert np.array_equal(now, st[0, p]), p


def _modes_and_edges(opt, cfg):
    """8: direct mode, no trajectory, t_cur past the end, an unsolvable QP.  Returns what a second library must reproduce."""
    P, Ts = _setup(opt, cfg)
    r = ROBOTS[0]
    out = []
    now = _now(opt, r, 0.2, 0)
    # no trajectory
    opt.track_clear(ROBOTS[1])
    cmd, st, _ = opt.mpc_cmds([ROBOTS[1]], 0.2, now[None])
    assert st[0, 0] == 2 and np.all(cmd[0, :2] == 0) and np.array_equal(cmd[0, 2:9], now[3:]) and np.all(cmd[0, 9:] == 0)
    out.append(cmd)
    # past the end: at goal, the state untouched
    before = opt.mpc_get_state(r)
    cmd, st, _ = opt.mpc_cmds([r], Ts[0] + 1.0, now[None])
    a, da = _states(opt, r, [Ts[0] + 1.0 + 1.0 / P.ctrl_freq])
    assert st[0, 0] == 1 and np.all(cmd[0, :2] == 0) and np.array_equal(cmd[0, 2:9], a[0, 3:]) and np.array_equal(cmd[0, 9:], da[0, 3:])
    assert np.array_equal(before[0], opt.mpc_get_state(r)[0])
    cmd2, st2, _ = opt.mpc_cmds([r], np.nextafter(Ts[0] + 1.0, 0.0), now[None])
    assert st2[0, 0] == 0
    out += [cmd, cmd2]
    # direct mode: a constant reference, the arm held; at goal after 1.0 s
    target = now[:3] + np.array([0.3, 0.1, 0.2])
    opt.mpc_set_direct([r], target[None])
    chk = wl.OmpcCheck(P)
    chk.set_direct(target)
    opt.mpc_reset([ROBOTS[2]], P)
    opt.mpc_set_direct([ROBOTS[2]], target[None])
    for t in (0.0, 0.02, 0.04):
        cmd, st, _ = opt.mpc_cmds([ROBOTS[2]], t, now[None])
        rc, rs, _ = chk.cmd(t, now)
        assert np.array_equal(cmd[0], rc) and np.array_equal(st[0], rs) and st[0, 3] == 1 and st[0, 0] == 0
        assert np.array_equal(cmd[0, 2:9], now[3:]) and np.all(cmd[0, 9:] == 0)
        out.append(cmd)
    assert cmd[0, 0] != 0 and cmd[0, 1] != 0
    cmd, st, _ = opt.mpc_cmds([ROBOTS[2]], 1.0, now[None])
    assert st[0, 0] == 1 and np.all(cmd[0, :2] == 0)
    opt.mpc_set_direct([ROBOTS[2]], None)
    assert opt.mpc_get_state(ROBOTS[2])[2] == 0
    # a QP that cannot be solved in one step: output as it was, outcome 3
    Pq = _params(opt, cfg, qp_max_iter=1, max_iter=2)
    opt.mpc_reset([r], Pq)
    cmd, st, _ = opt.mpc_cmds([r], 0.2, now[None])
    o, f, _ = opt.mpc_get_state(r)
    assert st[0, 0] == 3 and st[0, 1] == 1 and st[0, 2] == 1 and np.all(o == 0) and np.all(cmd[0, :2] == 0) and np.all(f == 0)
    out.append(cmd)
    return np.concatenate(out)


@pytest.mark.parametrize("cfg", CFGS)
def test_modes_and_edges(emu, cfg):
    _modes_and_edges(emu, cfg)


def test_refusals(emu):
    """9"""
    L = emu.L
    ok = emu.mpc_params(predict_steps=6, delay_num_v=2, delay_num_w=2)
    rb = api._ip(np.array([5], dtype=np.int32))
    for kw, code in ((dict(delay_num_v=1, delay_num_w=2), -6), (dict(delay_num_v=0, delay_num_w=0), -6), (dict(predict_steps=3), -1),
                     (dict(predict_steps=129, delay_num_v=100, delay_num_w=100), -1), (dict(predict_steps=70, delay_num_v=5, delay_num_w=5), -1),
                     (dict(max_iter=0), -1)):
        p = emu.mpc_params(**{**dict(predict_steps=6, delay_num_v=2, delay_num_w=2), **kw})
        assert L.topay_mpc_reset(emu.h, 1, rb, p) == code, kw
    now, cmd, t = np.zeros(10), np.zeros(32), np.zeros(2)
    never = api._ip(np.array([2000], dtype=np.int32))
    assert L.topay_mpc_cmds(emu.h, 1, never, api._dp(t), api._dp(now), api._dp(cmd), None, None) == -1          # never reset
    emu.mpc_reset([5, 6], ok)
    twice = api._ip(np.array([5, 5], dtype=np.int32))
    assert L.topay_mpc_cmds(emu.h, 2, twice, api._dp(t), api._dp(np.zeros(20)), api._dp(cmd), None, None) == -1   # named twice
    for bad in (np.nan, np.inf):
        assert L.topay_mpc_cmds(emu.h, 1, rb, api._dp(np.array([bad])), api._dp(now), api._dp(cmd), None, None) == -1
        s = now.copy(); s[2] = bad
        assert L.topay_mpc_cmds(emu.h, 1, rb, api._dp(t), api._dp(s), api._dp(cmd), None, None) == -1
    assert L.topay_mpc_cmds(emu.h, 1, api._ip(np.array([4096], dtype=np.int32)), api._dp(t), api._dp(now), api._dp(cmd), None, None) == -1
    assert L.topay_track_follow(emu.h, 1, rb, api._dp(t), 3, 2, None, None, None) == -1                            # no simulator
    assert L.topay_sim_reset(emu.h, 1, rb, api._dp(now), 0) == -1
    assert L.topay_mpc_cmds(emu.h, 1, rb, api._dp(t), api._dp(now), api._dp(cmd), None, None) == 0                 # (and the good call passes)


def test_entries_are_declared_and_mirrored():
    """10"""
    header = open(os.path.join(ROOT, "include", "topay.h")).read()
    L = api.load(EMU_LIB)
    for name in NEW_ENTRIES:
        assert re.search(r"topay_status\s+%s\(" % name, header), name
        assert getattr(L, name).argtypes is not None, name
    fields = re.search(r"typedef struct \{([^}]*)\} topay_mpc_params_t;", header).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in api.MpcParams._fields_]
    p = api.MpcParams()
    L.topay_mpc_default_params(p)
    assert (p.du_threshold, p.dt, p.ctrl_freq, p.max_iter, p.predict_steps, p.delay_num_v, p.delay_num_w) == (0.001, 0.02, 50.0, 150, 50, 20, 20)
    assert (p.max_omega, p.max_domega, p.max_speed, p.min_speed, p.max_accel) == (0.9, 1.0, 1.0, -1.0, 0.8)
    assert list(p.matrix_q) == [10.0, 10.0, 3.0] and list(p.matrix_r) == [0.01, 0.01] and list(p.matrix_rd) == [15.0, 1.5]
    assert (p.qp_eps_abs, p.qp_eps_rel, p.qp_rho, p.qp_sigma, p.qp_alpha, p.qp_max_iter) == (1e-6, 1e-6, 10.0, 1e-6, 1.6, 30000)


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite: the device equals the emulator bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    opt = api.MomaTrajOptBatch(device=0)
    yield opt
    opt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_gpu_commands_and_qp_equal_the_emulator(gpu, emu, cfg):
    """1 and 3 on the device."""
    E = _emu_episode(emu, cfg)[0]
    G = _episode(gpu, cfg)
    assert _same_episode(G, E, cfg[0], max(cfg[1:]), False)


@pytest.mark.gpu
def test_gpu_simulator_equals_the_emulator(gpu, emu):
    assert np.array_equal(_sim_facts(gpu), _sim_facts(emu))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_gpu_follow_equals_steps_and_the_emulator(gpu, emu, cfg):
    g = _follow_case(gpu, cfg, 20)
    e = _follow_case(emu, cfg, 20)
    assert all(np.array_equal(a, b) for a, b in zip(g, e))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_gpu_modes_and_edges_equal_the_emulator(gpu, emu, cfg):
    assert np.array_equal(_modes_and_edges(gpu, cfg), _modes_and_edges(emu, cfg))


@pytest.mark.gpu
def test_gpu_follow_256_robots_equals_single_robot_calls(gpu):
    """256 robots x 25 periods at the shipped configuration in one launch == 256 launches of one robot.  Slow: about 260 s on an
    MI355X, one second per single-robot launch (a wave takes about 40 ms per command, docs/EXPERIMENTS.md "Tracking controller")."""
    cfg, n, periods = CFGS[2], 256, 25
    robots = list(range(100, 100 + n))
    P, _ = _setup(gpu, cfg, robots)
    s0 = np.stack([_now(gpu, r, 0.0, i % 3) + 0.001 * i for i, r in enumerate(robots)])
    gpu.sim_reset(robots, s0, cfg[1])
    st, cm, ss = gpu.track_follow(robots, 0.05, periods, 2)
    assert (ss[:, :, 0] == 0).all()
    gpu.mpc_reset(robots, P)
    gpu.sim_reset(robots, s0, cfg[1])
    for i, r in enumerate(robots):
        s1, c1, t1 = gpu.track_follow([r], 0.05, periods, 2)
        assert np.array_equal(s1[0], st[i]) and np.array_equal(c1[0], cm[i]) and np.array_equal(t1[0], ss[i]), i
