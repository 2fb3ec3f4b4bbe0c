// Stand-alone sanitizer pass (own main, no Python, host only) over the tracking controller: (1) the checker harness/ompc.hpp and
// the fake robot, both delay branches and the shipped size, a short closed loop each; (2) the entries topay_mpc_* / topay_sim_* /
// topay_track_follow with the argument checks of topay_host_mpc.h, through the CPU lane-emulator build of the kernel sources:
// the refusals, reset, set_direct, commands, a probe, a simulator step and a follow.
// Build and run from the repository root:
//   g++ -O1 -g -std=c++17 -march=x86-64-v3 -ffp-contract=off -DTOPAY_LDS= -DTOPAY_GLB= -DTOPAY_CST= -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -I tests/emu/include -x c++ topay_amd/csrc/topay_hip.hip tools/mpc_sanitize.cpp \
//       -o mpc_sanitize -ldl -lpthread && ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 ./mpc_sanitize
// (detect_leaks=0: the emulator keeps the stacks of its lane fibres for the life of the process; the compile takes several minutes)
#include <cstdio>

#include "../harness/ompc.hpp"
#include "../include/topay.h"

static ompc::Params params(int T, int dv, int dw) {
  ompc::Params p{};
  p.du_threshold = 0.001; p.dt = 0.02; p.ctrl_freq = 50.0; p.max_iter = 150; p.predict_steps = T; p.delay_num_v = dv; p.delay_num_w = dw;
  p.max_omega = 0.9; p.max_domega = 1.0; p.max_speed = 1.0; p.min_speed = -1.0; p.max_accel = 0.8;
  p.matrix_q[0] = 10.0; p.matrix_q[1] = 10.0; p.matrix_q[2] = 3.0; p.matrix_r[0] = p.matrix_r[1] = 0.01; p.matrix_rd[0] = 15.0; p.matrix_rd[1] = 1.5;
  p.qp_eps_abs = p.qp_eps_rel = 1.0e-6; p.qp_rho = 10.0; p.qp_sigma = 1.0e-6; p.qp_alpha = 1.6; p.qp_max_iter = 30000;
  return p;
}

#define CHECK(call)                                                                     \
  do {                                                                                  \
    const int s_ = (call);                                                              \
    if (s_ != 0) { printf("%s -> %d (%s)\n", #call, s_, topay_last_error()); return 1; } \
  } while (0)
#define EXPECT(call, code)                                                        \
  do {                                                                            \
    const int s_ = (call);                                                        \
    if (s_ != (code)) { printf("%s -> %d, expected %d\n", #call, s_, (code)); return 1; } \
  } while (0)

// the library's entries through the emulator build
static int library() {
  topay_params_t prm;
  CHECK(topay_default_params(&prm));
  topay_ctx* c = nullptr;
  CHECK(topay_create(&prm, 0, &c));
  topay_mpc_params_t ok;
  CHECK(topay_mpc_default_params(&ok));
  ok.predict_steps = 8; ok.delay_num_v = 4; ok.delay_num_w = 2;
  const int rb[2] = {5, 4095}, twice[2] = {5, 5}, out_of_range[1] = {4096}, never[1] = {2000};
  // ---- the refusals
  topay_mpc_params_t bad = ok;
  bad.delay_num_v = 1; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_UNSUPPORTED);
  bad = ok; bad.delay_num_v = 0; bad.delay_num_w = 0; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_UNSUPPORTED);
  bad = ok; bad.predict_steps = 5; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_INVALID_ARG);
  bad = ok; bad.predict_steps = 129; bad.delay_num_v = bad.delay_num_w = 100; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_INVALID_ARG);
  bad = ok; bad.predict_steps = 70; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_INVALID_ARG);
  bad = ok; bad.dt = 0.0 / 0.0; EXPECT(topay_mpc_reset(c, 2, rb, &bad), TOPAY_ERR_INVALID_ARG);
  double now[20] = {0.02, -0.03, 3.1, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, -0.05, 0.01, -3.1, 0, 0, 0, 0, 0, 0, 0};
  double t[2] = {0.1, 0.1}, cmd[32];
  int st[8];
  EXPECT(topay_mpc_cmds(c, 1, never, t, now, cmd, st, nullptr), TOPAY_ERR_INVALID_ARG);
  EXPECT(topay_mpc_reset(c, 2, twice, &ok), TOPAY_ERR_INVALID_ARG);
  EXPECT(topay_mpc_reset(c, 1, out_of_range, &ok), TOPAY_ERR_INVALID_ARG);
  CHECK(topay_mpc_reset(c, 2, rb, &ok));
  EXPECT(topay_mpc_cmds(c, 2, twice, t, now, cmd, st, nullptr), TOPAY_ERR_INVALID_ARG);
  double tbad[2] = {0.1, 1.0 / 0.0};
  EXPECT(topay_mpc_cmds(c, 2, rb, tbad, now, cmd, st, nullptr), TOPAY_ERR_INVALID_ARG);
  now[12] = 0.0 / 0.0;
  EXPECT(topay_mpc_cmds(c, 2, rb, t, now, cmd, st, nullptr), TOPAY_ERR_INVALID_ARG);
  now[12] = -3.1;
  EXPECT(topay_track_follow(c, 2, rb, t, 3, 2, nullptr, nullptr, nullptr), TOPAY_ERR_INVALID_ARG);   // no simulator
  EXPECT(topay_sim_reset(c, 2, rb, now, 0), TOPAY_ERR_INVALID_ARG);
  EXPECT(topay_sim_step(c, 2, rb, nullptr, 2, nullptr), TOPAY_ERR_INVALID_ARG);
  // ---- no trajectory yet: outcome 2; the probe says so
  CHECK(topay_mpc_cmds(c, 2, rb, t, now, cmd, st, nullptr));
  if (st[0] != 2 || st[4] != 2) { printf("no trajectory: outcome %d %d\n", st[0], st[4]); return 1; }
  int nx = 0, nc = 0, info[2];
  CHECK(topay_mpc_qp_dims(&ok, &nx, &nc));
  std::vector<double> P((size_t)nx * nx), q(nx), A((size_t)nc * nx), l(nc), u(nc), x(nx), y(nc), z(nc), xopt(2 * 3 * (TOPAY_MPC_MAX_STEPS + 1));
  EXPECT(topay_mpc_probe(c, 5, 0.1, now, P.data(), q.data(), A.data(), l.data(), u.data(), x.data(), y.data(), z.data(), info), TOPAY_ERR_NO_TRAJ);
  // ---- a two-piece trajectory per robot: theta = 3.0 + 0.5 t (crosses pi), arc length 0.5 t
  double dur[2] = {0.8, 0.7}, coef[2 * 54] = {0}, s3[3] = {0.0, 0.0, 3.0};
  for (int i = 0; i < 2; i++) { coef[54 * i + 5] = 3.0 + 0.5 * 0.8 * i; coef[54 * i + 4] = 0.5; coef[54 * i + 6 + 5] = 0.5 * 0.8 * i; coef[54 * i + 6 + 4] = 0.5; }
  for (int r : rb) CHECK(topay_track_set(c, r, 1, s3, 2, dur, coef));
  CHECK(topay_mpc_cmds(c, 2, rb, t, now, cmd, st, xopt.data()));
  if (st[0] != 0 || st[4] != 0) { printf("commands: outcome %d %d\n", st[0], st[4]); return 1; }
  CHECK(topay_mpc_probe(c, 5, 0.12, now, P.data(), q.data(), A.data(), l.data(), u.data(), x.data(), y.data(), z.data(), info));
  if (info[1] != 1) { printf("probe: QP not solved\n"); return 1; }
  EXPECT(topay_mpc_probe(c, 5, 2.5, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, info), TOPAY_ERR_NO_TRAJ);   // at goal
  // ---- direct mode and back
  const double target[6] = {0.2, 0.1, 3.0, -0.2, 0.0, -3.0};
  CHECK(topay_mpc_set_direct(c, 2, rb, target));
  std::vector<double> outp(2 * TOPAY_MPC_MAX_STEPS), fifo(2 * TOPAY_MPC_MAX_STEPS);
  int mode = -1;
  CHECK(topay_mpc_get_state(c, 4095, outp.data(), fifo.data(), &mode));
  if (mode != 1 || fifo[2 * 3] == 0.0) { printf("set_direct damaged the slot: mode %d\n", mode); return 1; }
  CHECK(topay_mpc_cmds(c, 2, rb, t, now, cmd, st, nullptr));
  if (st[3] != 1 || st[0] != 0) { printf("direct mode: %d %d\n", st[3], st[0]); return 1; }
  CHECK(topay_mpc_set_direct(c, 2, rb, nullptr));
  // ---- the simulator and a follow
  CHECK(topay_sim_reset(c, 2, rb, now, 4));
  double state[20];
  CHECK(topay_sim_step(c, 2, rb, cmd, 2, state));
  CHECK(topay_sim_step(c, 2, rb, nullptr, 1, state));
  std::vector<double> so(2 * 6 * 10), co(2 * 6 * 16);
  std::vector<int> ss(2 * 6 * TOPAY_MPC_ST_LEN);
  CHECK(topay_track_follow(c, 2, rb, t, 6, 2, so.data(), co.data(), ss.data()));
  double ms = -1.0;
  CHECK(topay_mpc_ms(c, &ms));
  topay_destroy(c);
  printf("library entries ok (follow: robot 5 at %.4f %.4f %.4f)\n", so[50], so[51], so[52]);
  return 0;
}

int main() {
  if (library() != 0) return 1;
  const int cfg[3][3] = {{6, 2, 2}, {8, 4, 2}, {50, 20, 20}};
  for (const auto& c : cfg) {
    const ompc::Params p = params(c[0], c[1], c[2]);
    ompc::OMPC m(p);
    const double s0[10] = {-0.05, 0.03, 3.1, 0, 0, 0, 0, 0, 0, 0};
    ompc::Sim sim(s0, c[1]);
    std::vector<double> rows(3 * c[0]), xopt(3 * (c[0] + 1));
    double t = 0.0, cmd[16], arm[7] = {0, 0, 0, 0, 0, 0, 0};
    int st[4], total = 0;
    for (int period = 0; period < 12; period++) {
      double tt = t + p.dt;
      for (int j = 0; j < c[0]; j++, tt += p.dt) { rows[3 * j] = -0.5 * tt; rows[3 * j + 1] = 0.02 * tt; rows[3 * j + 2] = 3.1 + 0.4 * tt; }   // the yaw crosses pi
      if (period == 3) {
        ompc::Dense D;
        m.getCmd(true, t, 10.0, sim.st, rows.data(), arm, arm, cmd, st, nullptr, &D);
        if (!D.solved) { printf("probe: QP not solved\n"); return 1; }
      }
      m.getCmd(true, t, 10.0, sim.st, rows.data(), arm, arm, cmd, st, xopt.data());
      if (st[0] != 0) { printf("outcome %d\n", st[0]); return 1; }
      total += st[2];
      sim.step(cmd, 2);
      t = t + 1.0 / p.ctrl_freq;
    }
    m.control_state = 1;
    m.getCmd(true, 0.5, 0.0, sim.st, nullptr, arm, arm, cmd, st, xopt.data());
    m.getCmd(false, 2.0, 0.0, sim.st, nullptr, arm, arm, cmd, st, nullptr);
    printf("(%d, %d, %d): %d QP steps in 12 periods, robot at (%.4f, %.4f, %.4f)\n", c[0], c[1], c[2], total, sim.st[0], sim.st[1], sim.st[2]);
  }
  printf("mpc_sanitize ok\n");
  return 0;
}
