// Host side of the C-ABI, part 12: the tracking controller and the fake robot (topay_mpc.h; OMPC and moma_sim).  Robot slots are
// those of topay_host_track.h, checked by its check_robot_slots.  The slots' state lies in two device arrays of TOPAY_TRACK_SLOTS
// entries, allocated zeroed by the first reset (MpcState::alloc); every argument is checked here, before any launch.

#pragma once

static topay_status mpc_check_params(const topay_mpc_params_t& p) {
  const int T = p.predict_steps, dv = p.delay_num_v, dw = p.delay_num_w;
  if (dv < 0 || dw < 0 || T < 1) { set_err("topay_mpc: predict_steps >= 1, delays >= 0"); return TOPAY_ERR_INVALID_ARG; }
  if (dv < dw) { set_err("topay_mpc: delay_num_v < delay_num_w is not supported (the reference's code for it is commented out)"); return TOPAY_ERR_UNSUPPORTED; }
  if (std::max(dv, dw) == 0) { set_err("topay_mpc: max(delay_num_v, delay_num_w) == 0 is not supported (the reference reads an empty output_buff)"); return TOPAY_ERR_UNSUPPORTED; }
  if (T > TOPAY_MPC_MAX_STEPS || T - dw > TOPAY_MPC_MAX_STAGES) { set_err("topay_mpc: at most 128 steps and 64 stages"); return TOPAY_ERR_INVALID_ARG; }
  if (T - dv < 2) { set_err("topay_mpc: predict_steps - delay_num_v must be at least 2"); return TOPAY_ERR_INVALID_ARG; }
  if (p.max_iter < 1 || p.qp_max_iter < 1) { set_err("topay_mpc: max_iter and qp_max_iter must be at least 1"); return TOPAY_ERR_INVALID_ARG; }
  const double v[] = {p.du_threshold, p.dt, p.ctrl_freq, p.max_omega, p.max_domega, p.max_speed, p.min_speed, p.max_accel, p.matrix_q[0], p.matrix_q[1],
                      p.matrix_q[2], p.matrix_r[0], p.matrix_r[1], p.matrix_rd[0], p.matrix_rd[1], p.qp_eps_abs, p.qp_eps_rel, p.qp_rho, p.qp_sigma, p.qp_alpha};
  for (double x : v)
    if (!(std::fabs(x) < 1.0e12)) { set_err("topay_mpc: a parameter is not finite"); return TOPAY_ERR_INVALID_ARG; }
  if (!(p.dt > 0.0 && p.ctrl_freq > 0.0 && p.qp_rho > 0.0 && p.qp_sigma > 0.0 && p.qp_alpha > 0.0 && p.qp_alpha < 2.0 && p.qp_eps_abs >= 0.0 && p.qp_eps_rel >= 0.0)) {
    set_err("topay_mpc: dt, ctrl_freq, qp_rho, qp_sigma > 0, 0 < qp_alpha < 2");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (!(p.matrix_q[0] > 0.0 && p.matrix_q[1] > 0.0 && p.matrix_q[2] > 0.0 && p.matrix_r[0] > 0.0 && p.matrix_r[1] > 0.0 && p.matrix_rd[0] >= 0.0 && p.matrix_rd[1] >= 0.0)) {
    set_err("topay_mpc: matrix_q, matrix_r > 0, matrix_rd >= 0 (the Hessian's diagonal must be positive)");
    return TOPAY_ERR_INVALID_ARG;
  }
  return TOPAY_OK;
}

// The launch of k_mpc_cmds: n robots, `periods` periods each.  Outputs may be null.
static topay_status mpc_launch(topay_ctx* c, int n, const int* robots, const double* t_cur, const double* now_state, int periods, int ticks, bool follow,
                               double* cmd, int* status, double* xopt, double* states_out, const topay::MpcDense* dense) {
  const size_t N = (size_t)n, R = N * (size_t)periods;
  std::vector<topay::TrackDesc> desc(N);
  size_t lds = 0;
  for (int k = 0; k < n; k++) {
    const topay::TrackDesc* d = c->track.find(robots[k], 0);
    if (d) desc[k] = *d;
    else { desc[k].off = 0; desc[k].N = 0; desc[k].num = 0; }
    const topay_mpc_params_t& p = c->mpc.prm[robots[k]];
    lds = std::max(lds, topay::mpc_lds_doubles(p.predict_steps, p.predict_steps - p.delay_num_w) * 8);
  }
  topay::TrackDesc* d_desc; int *d_rob, *d_st; double *d_t, *d_now, *d_cmd, *d_xopt, *d_so;
  const size_t XO = 3 * (size_t)(TOPAY_MPC_MAX_STEPS + 1);
  auto lay = [&](Carver& k) {
    d_t = k.take<double>(N); d_now = k.take<double>(10 * N); d_cmd = k.take<double>(16 * R); d_xopt = k.take<double>(xopt ? XO * N : 0);
    d_so = k.take<double>(states_out ? 10 * R : 0); d_desc = k.take<topay::TrackDesc>(N); d_rob = k.take<int>(N); d_st = k.take<int>(TOPAY_MPC_ST_LEN * R);
  };
  topay_status s;
  if ((s = c->mpc.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_t, t_cur, N));
  if (now_state) HIPCHK(h2d(c, d_now, now_state, 10 * N));
  HIPCHK(h2d(c, d_desc, desc.data(), N));
  HIPCHK(h2d(c, d_rob, robots, N));
  if (xopt) HIPCHK(hipMemsetAsync(d_xopt, 0, XO * N * 8, c->stream));
  topay::MpcArgs A;
  memset(&A, 0, sizeof(A));
  A.n = n; A.periods = periods; A.ticks = ticks; A.follow = follow ? 1 : 0; A.probe = dense ? 1 : 0;
  A.robots = d_rob; A.slots = c->mpc.slots.as<topay::MpcSlot>(); A.sims = c->mpc.sims.as<topay::SimSlot>(); A.desc = d_desc;
  A.arena = c->track.arena.as<double>(); A.t_cur = d_t; A.now_state = d_now; A.cmd = d_cmd; A.status = d_st; A.xopt = xopt ? d_xopt : nullptr;
  A.states_out = states_out ? d_so : nullptr;
  if (dense) A.D = *dense;
  HIPCHK(c->mpc.timer.start(c->stream));
  hipLaunchKernelGGL(topay::k_mpc_cmds, dim3((unsigned)n), dim3(64), lds, c->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(c->mpc.timer.stop(c->stream));
  if (cmd) HIPCHK(d2h(c, cmd, d_cmd, 16 * R));
  if (status) HIPCHK(d2h(c, status, d_st, TOPAY_MPC_ST_LEN * R));
  if (xopt) HIPCHK(d2h(c, xopt, d_xopt, XO * N));
  if (states_out) HIPCHK(d2h(c, states_out, d_so, 10 * R));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!dense) (void)c->mpc.timer.read(&c->mpc.ms);
  return TOPAY_OK;
}

extern "C" {

topay_status topay_mpc_default_params(topay_mpc_params_t* p) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  memset(p, 0, sizeof(*p));
  p->du_threshold = 0.001; p->dt = 0.02; p->ctrl_freq = 50.0;
  p->max_iter = 150; p->predict_steps = 50; p->delay_num_v = 20; p->delay_num_w = 20;
  p->max_omega = 0.9; p->max_domega = 1.0; p->max_speed = 1.0; p->min_speed = -1.0; p->max_accel = 0.8;
  p->matrix_q[0] = 10.0; p->matrix_q[1] = 10.0; p->matrix_q[2] = 3.0;
  p->matrix_r[0] = 0.01; p->matrix_r[1] = 0.01;
  p->matrix_rd[0] = 15.0; p->matrix_rd[1] = 1.5;
  p->qp_eps_abs = 1.0e-6; p->qp_eps_rel = 1.0e-6;
  p->qp_rho = 10.0; p->qp_sigma = 1.0e-6; p->qp_alpha = 1.6;
  p->qp_max_iter = 30000;
  return TOPAY_OK;
}

topay_status topay_mpc_qp_dims(const topay_mpc_params_t* p, int* nx, int* nc) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = mpc_check_params(*p); s != TOPAY_OK) return s;
  const int T = p->predict_steps, dimx = 3 * (T - p->delay_num_w), dimu = (T - p->delay_num_v) + (T - p->delay_num_w);
  if (nx) *nx = dimx + dimu;
  if (nc) *nc = dimu + dimx + dimu - 2;
  return TOPAY_OK;
}

topay_status topay_mpc_reset(topay_ctx* c, int n, const int* robots, const topay_mpc_params_t* params) {
  if (!c || n <= 0 || !robots || !params) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = mpc_check_params(*params); s != TOPAY_OK) return s;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct, "topay_mpc_reset")) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status s = c->mpc.alloc(c->stream)) return s;
  topay::MpcSlot* slot = new topay::MpcSlot();
  memset(slot, 0, sizeof(*slot));
  slot->P = *params; slot->have = 1;
  hipError_t e = hipSuccess;
  for (int k = 0; k < n && e == hipSuccess; k++) e = hipMemcpyAsync(c->mpc.slots.as<topay::MpcSlot>() + robots[k], slot, sizeof(*slot), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  delete slot;
  HIPCHK(e);
  for (int k = 0; k < n; k++) { c->mpc.prm[robots[k]] = *params; c->mpc.have[robots[k]] = 1; }
  return TOPAY_OK;
}

topay_status topay_mpc_set_direct(topay_ctx* c, int n, const int* robots, const double* direct_pos) {
  if (!c || n <= 0 || !robots) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct | kRobotMpc, "topay_mpc_set_direct")) return s;
  if (direct_pos && !all_finite(direct_pos, 3 * (size_t)n)) { set_err("topay_mpc_set_direct: direct_pos must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  struct Head { int mode, have; double direct[3]; } h;   // MpcSlot's members from `mode` to `direct`, as they lie there
  static_assert(offsetof(topay::MpcSlot, have) == offsetof(topay::MpcSlot, mode) + offsetof(Head, have) &&
                    offsetof(topay::MpcSlot, direct) == offsetof(topay::MpcSlot, mode) + offsetof(Head, direct) &&
                    offsetof(topay::MpcSlot, output) == offsetof(topay::MpcSlot, mode) + sizeof(Head),
                "topay_mpc_set_direct copies mode, have, direct in one piece");
  for (int k = 0; k < n; k++) {
    h.mode = direct_pos ? 1 : 0; h.have = 1;
    for (int a = 0; a < 3; a++) h.direct[a] = direct_pos ? direct_pos[3 * (size_t)k + a] : 0.0;
    char* dst = (char*)(c->mpc.slots.as<topay::MpcSlot>() + robots[k]) + offsetof(topay::MpcSlot, mode);
    HIPCHK(hipMemcpyAsync(dst, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return TOPAY_OK;
}

topay_status topay_mpc_cmds(topay_ctx* c, int n, const int* robots, const double* t_cur, const double* now_state, double* cmd, int* status, double* xopt) {
  if (!c || n <= 0 || !robots || !t_cur || !now_state || !cmd) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct | kRobotMpc, "topay_mpc_cmds")) return s;
  if (!all_finite(t_cur, (size_t)n) || !all_finite(now_state, 10 * (size_t)n)) { set_err("topay_mpc_cmds: clocks and states must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return mpc_launch(c, n, robots, t_cur, now_state, 1, 0, false, cmd, status, xopt, nullptr, nullptr);
}

topay_status topay_mpc_probe(topay_ctx* c, int robot, double t_cur, const double* now_state, double* P, double* q, double* A, double* l, double* u,
                             double* x, double* y, double* z, int* info) {
  if (!c || !now_state) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, 1, &robot, kRobotMpc, "topay_mpc_probe")) return s;
  if (!all_finite(&t_cur, 1) || !all_finite(now_state, 10)) { set_err("topay_mpc_probe: clock and state must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const topay_mpc_params_t& p = c->mpc.prm[robot];
  int nx = 0, nc = 0;
  topay_mpc_qp_dims(&p, &nx, &nc);
  const size_t NX = (size_t)nx, NC = (size_t)nc;
  topay::MpcDense D;
  auto lay = [&](Carver& k) {
    D.P = k.take<double>(NX * NX); D.q = k.take<double>(NX); D.A = k.take<double>(NC * NX); D.l = k.take<double>(NC); D.u = k.take<double>(NC);
    D.x = k.take<double>(NX); D.y = k.take<double>(NC); D.z = k.take<double>(NC); D.info = k.take<int>(2);
  };
  if (topay_status s = c->mpc.dense.carve(lay); s != TOPAY_OK) return s;
  HIPCHK(hipMemsetAsync(c->mpc.dense.p, 0, c->mpc.dense.bytes, c->stream));
  if (topay_status s = mpc_launch(c, 1, &robot, &t_cur, now_state, 1, 0, false, nullptr, nullptr, nullptr, nullptr, &D); s != TOPAY_OK) return s;
  // whether the call reaches the QP is the kernel's decision (its sum of the durations, its mode): it says so in info[1]
  int hinfo[2] = {0, 0};
  HIPCHK(d2h_sync(c, hinfo, (const int*)D.info, 2));
  if (hinfo[1] < 0) { set_err("topay_mpc_probe: the call does not reach the QP (no end_traj, or at goal)"); return TOPAY_ERR_NO_TRAJ; }
  if (P) HIPCHK(d2h(c, P, D.P, NX * NX));
  if (q) HIPCHK(d2h(c, q, D.q, NX));
  if (A) HIPCHK(d2h(c, A, D.A, NC * NX));
  if (l) HIPCHK(d2h(c, l, D.l, NC));
  if (u) HIPCHK(d2h(c, u, D.u, NC));
  if (x) HIPCHK(d2h(c, x, D.x, NX));
  if (y) HIPCHK(d2h(c, y, D.y, NC));
  if (z) HIPCHK(d2h(c, z, D.z, NC));
  if (info) HIPCHK(d2h(c, info, D.info, 2));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_mpc_get_state(topay_ctx* c, int robot, double* output, double* fifo, int* mode) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, 1, &robot, kRobotMpc, "topay_mpc_get_state")) return s;
  HIPCHK(hipSetDevice(c->device));
  topay::MpcSlot* hs = new topay::MpcSlot();
  const hipError_t e = d2h_sync(c, (char*)hs, (const char*)(c->mpc.slots.as<topay::MpcSlot>() + robot), sizeof(*hs));
  if (e == hipSuccess) {
    if (output) memcpy(output, hs->output, sizeof(hs->output));
    if (fifo) memcpy(fifo, hs->buff, sizeof(hs->buff));
    if (mode) *mode = hs->mode;
  }
  delete hs;
  HIPCHK(e);
  return TOPAY_OK;
}

topay_status topay_mpc_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  *ms = c->mpc.ms;
  return TOPAY_OK;
}

topay_status topay_sim_reset(topay_ctx* c, int n, const int* robots, const double* state0, int delay_cmds) {
  if (!c || n <= 0 || !robots || !state0) return TOPAY_ERR_INVALID_ARG;
  if (delay_cmds < 1 || delay_cmds > TOPAY_MPC_MAX_STEPS) { set_err("topay_sim_reset: delay_cmds in 1..128"); return TOPAY_ERR_INVALID_ARG; }
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct, "topay_sim_reset")) return s;
  if (!all_finite(state0, 10 * (size_t)n)) { set_err("topay_sim_reset: states must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  if (topay_status s = c->mpc.alloc(c->stream)) return s;
  topay::SimSlot* slot = new topay::SimSlot();
  hipError_t e = hipSuccess;
  for (int k = 0; k < n && e == hipSuccess; k++) {
    memset(slot, 0, sizeof(*slot));
    for (int a = 0; a < 10; a++) slot->st[a] = state0[10 * (size_t)k + a];
    slot->delay = delay_cmds; slot->have = 1;
    e = hipMemcpyAsync(c->mpc.sims.as<topay::SimSlot>() + robots[k], slot, sizeof(*slot), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  delete slot;
  HIPCHK(e);
  for (int k = 0; k < n; k++) c->mpc.sim_have[robots[k]] = 1;
  return TOPAY_OK;
}

topay_status topay_sim_step(topay_ctx* c, int n, const int* robots, const double* cmd, int ticks, double* state) {
  if (!c || n <= 0 || !robots || ticks < 0) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct | kRobotSim, "topay_sim_step")) return s;
  if (cmd && !all_finite(cmd, 16 * (size_t)n)) { set_err("topay_sim_step: commands must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n;
  double *d_cmd, *d_state; int* d_rob;
  auto lay = [&](Carver& k) { d_cmd = k.take<double>(16 * N); d_state = k.take<double>(10 * N); d_rob = k.take<int>(N); };
  if (topay_status s = c->mpc.io.carve(lay); s != TOPAY_OK) return s;
  if (cmd) HIPCHK(h2d(c, d_cmd, cmd, 16 * N));
  HIPCHK(h2d(c, d_rob, robots, N));
  topay::SimArgs A;
  A.n = n; A.ticks = ticks; A.robots = d_rob; A.sims = c->mpc.sims.as<topay::SimSlot>(); A.cmd = cmd ? d_cmd : nullptr; A.state = d_state;
  hipLaunchKernelGGL(topay::k_sim_step, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, A);
  HIPCHK(hipGetLastError());
  if (state) HIPCHK(d2h(c, state, d_state, 10 * N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_track_follow(topay_ctx* c, int n, const int* robots, const double* t0, int periods, int ticks_per_period, double* states_out,
                                double* cmds_out, int* status_out) {
  if (!c || n <= 0 || !robots || !t0 || periods < 1 || periods > 100000 || ticks_per_period < 0) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotDistinct | kRobotMpc | kRobotSim, "topay_track_follow")) return s;
  if (!all_finite(t0, (size_t)n)) { set_err("topay_track_follow: clocks must be finite"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return mpc_launch(c, n, robots, t0, nullptr, periods, ticks_per_period, true, cmds_out, status_out, nullptr, states_out, nullptr);
}

}  // extern "C"
