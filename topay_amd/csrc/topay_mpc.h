// The tracking controller and the fake robot (include/topay.h, "The tracking controller"): OMPC::getCmd (planner/src/ompc.cpp:
// 538-656) with solveMPCDiff's QP (114-536), and moma_sim's rcvVelCmdCallBack / simCallBack (fake_moma/src/moma_sim.cpp:208-229,
// 251-308).
//   k_mpc_cmds   one wave per robot: `periods` times (one command [, one simulator step, t += 1 / ctrl_freq])
//   k_sim_step   one thread per robot: one command into the actuator FIFO, then ticks of 0.01 s
// The QP in stage order.  Stage j = 0 .. nS - 1 (nS = predict_steps - delay_num_w, one lane each) holds the variables
//   (v_j, w_j, x_j, y_j, theta_j)      v_j only for j >= dd = delay_num_v - delay_num_w (else a free variable of cost 1 nothing reads)
// and the rows
//   0 box v_j | 1 box w_j | 2..4 dynamics of (x_j, y_j, theta_j) | 5 rate v_{j+1} - v_j | 6 rate w_{j+1} - w_j
// A row touches stages j - 1 .. j + 1 only: with this order P + sigma I + A' R A has half-bandwidth 5.  The arrays of stages carry
// one zero stage before and one after, so that the products below have no edge cases.  Every expression here that decides a bit
// of the result is written out with its parentheses: harness/ompc.hpp states the same expressions in serial loops.
#pragma once
#include "topay_math.h"
#include "topay_track.h"
#include "topay_wave.h"

#ifndef TOPAY_CPU_EMU
extern __shared__ double topay_mpc_smem[];
#define TOPAY_MPC_LDS topay_mpc_smem
#else
#define TOPAY_MPC_LDS ((double*)hip_emu::S().dyn_smem)
#endif

namespace topay {

struct MpcSlot {   // OMPC's members that outlive a call
  topay_mpc_params_t P;
  int mode, have;                            // control_state; reset at least once
  double direct[3];
  double output[2 * TOPAY_MPC_MAX_STEPS];    // row r at r * TOPAY_MPC_MAX_STEPS
  double buff[2 * TOPAY_MPC_MAX_STEPS];      // output_buff: entry i at 2 i, oldest first
};
struct SimSlot {   // moma_sim's globals
  double st[10];                             // now_se2, now_q
  double cur[16];                            // moma_cmd after rcvVelCmdCallBack
  int received, delay, have, pad;            // commands received so far; delay_cmds
  double fifo[2 * (TOPAY_MPC_MAX_STEPS + 1)];   // vw_buff as a ring of delay + 1 entries
};

// per stage: 0 -A(0,2) | 1 -A(1,2) | 2 -B(0,0) | 3 -B(1,0) | 4 -1 (state j - 1 in the dynamics) | 5 v_j exists | 6 rate row v exists |
//            7 rate row w exists | 8, 9 the Hessian's off-diagonals v_j v_{j+1}, w_j w_{j+1} | 10 -B(2,1) | 11 -
constexpr int kMpcC = 12;

// (A X) of stage j's rows; X and C point at stage 0
__device__ __forceinline__ void mpc_Ax(const double* C, const double* X, int j, double* r) {
  const double* c = C + kMpcC * j;
  const double* x = X + 5 * j;
  r[0] = c[5] * x[0];
  r[1] = x[1];
  r[2] = ((x[2] + c[4] * x[-3]) + c[0] * x[-1]) + c[2] * x[0];
  r[3] = ((x[3] + c[4] * x[-2]) + c[1] * x[-1]) + c[3] * x[0];
  r[4] = (x[4] + c[4] * x[-1]) + c[10] * x[1];
  r[5] = c[6] * (x[5] - x[0]);
  r[6] = c[7] * (x[6] - x[1]);
}
// (A' Y) of stage j's variables
__device__ __forceinline__ void mpc_ATy(const double* C, const double* Y, int j, double* g) {
  const double* c = C + kMpcC * j;
  const double* cn = c + kMpcC;
  const double* y = Y + 7 * j;
  g[0] = ((c[5] * y[0] + c[2] * y[2]) + c[3] * y[3]) + (c[-6] * y[-2] - c[6] * y[5]);
  g[1] = (y[1] + c[10] * y[4]) + (c[-5] * y[-1] - c[7] * y[6]);
  g[2] = y[2] + cn[4] * y[9];
  g[3] = y[3] + cn[4] * y[10];
  g[4] = ((y[4] + cn[0] * y[9]) + cn[1] * y[10]) + cn[4] * y[11];
}
// (P X) of stage j's variables; PD the Hessian's diagonal
__device__ __forceinline__ void mpc_Px(const double* C, const double* PD, const double* X, int j, double* p) {
  const double* c = C + kMpcC * j;
  const double* x = X + 5 * j;
  const double* pd = PD + 5 * j;
  p[0] = pd[0] * x[0] + (c[-4] * x[-5] + c[8] * x[5]);
  p[1] = pd[1] * x[1] + (c[-3] * x[-4] + c[9] * x[6]);
  p[2] = pd[2] * x[2];
  p[3] = pd[3] * x[3];
  p[4] = pd[4] * x[4];
}
// L D L' of the banded matrix KB (row i at 6 i: K[i][i], K[i][i-1], .. K[i][i-5]; five zero rows before row 0, entries left of
// column 0 zero), in place: D in column 0, L beside it; ID = 1 / D (five zeros before ID[0]).
__device__ __forceinline__ void mpc_band_factor(double* KB, double* ID, int n) {
  for (int i = 0; i < n; i++) {
    double* r = KB + 6 * i;
    const double u5 = r[5];
    const double u4 = r[4] - u5 * r[-24 + 1];
    const double u3 = (r[3] - u5 * r[-18 + 2]) - u4 * r[-18 + 1];
    const double u2 = ((r[2] - u5 * r[-12 + 3]) - u4 * r[-12 + 2]) - u3 * r[-12 + 1];
    const double u1 = (((r[1] - u5 * r[-6 + 4]) - u4 * r[-6 + 3]) - u3 * r[-6 + 2]) - u2 * r[-6 + 1];
    const double l5 = u5 * ID[i - 5], l4 = u4 * ID[i - 4], l3 = u3 * ID[i - 3], l2 = u2 * ID[i - 2], l1 = u1 * ID[i - 1];
    const double d = ((((r[0] - u5 * l5) - u4 * l4) - u3 * l3) - u2 * l2) - u1 * l1;
    r[0] = d; r[1] = l1; r[2] = l2; r[3] = l3; r[4] = l4; r[5] = l5;
    ID[i] = 1.0 / d;
  }
}
// b <- K^-1 b (five zero rows after row n - 1 of KB)
__device__ __forceinline__ void mpc_band_solve(const double* KB, const double* ID, double* b, int n) {
  double t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0, t5 = 0.0;
  for (int i = 0; i < n; i++) {
    const double* r = KB + 6 * i;
    const double s = ((((b[i] - r[5] * t5) - r[4] * t4) - r[3] * t3) - r[2] * t2) - r[1] * t1;
    b[i] = s;
    t5 = t4; t4 = t3; t3 = t2; t2 = t1; t1 = s;
  }
  t1 = t2 = t3 = t4 = t5 = 0.0;
  for (int i = n - 1; i >= 0; i--) {
    const double* r = KB + 6 * i;
    const double s = ((((b[i] * ID[i] - r[30 + 5] * t5) - r[24 + 4] * t4) - r[18 + 3] * t3) - r[12 + 2] * t2) - r[6 + 1] * t1;
    b[i] = s;
    t5 = t4; t4 = t3; t3 = t2; t2 = t1; t1 = s;
  }
}

// rcvVelCmdCallBack, then `ticks` of simCallBack
__device__ __forceinline__ void sim_apply(SimSlot* S, const double* cmd, int ticks) {
  if (cmd) {
    const int k = S->received, m = S->delay + 1;
    for (int a = 0; a < 16; a++) S->cur[a] = cmd[a];
    S->cur[0] = 0.0; S->cur[1] = 0.0;
    S->fifo[2 * (k % m)] = cmd[0]; S->fifo[2 * (k % m) + 1] = cmd[1];
    if (k >= S->delay) {
      const int o = (k - S->delay) % m;
      S->cur[0] = S->fifo[2 * o]; S->cur[1] = S->fifo[2 * o + 1];
    }
    S->received = k + 1;
  }
  if (S->received == 0) return;
  const double time_resolution = 0.01, pi = 3.14159265358979323846;
  for (int i = 0; i < ticks; i++) {
    const double vx = S->cur[0], wz = S->cur[1];
    double sn, cs;
    det_sincos(S->st[2], &sn, &cs);
    S->st[0] += vx * time_resolution * cs;
    S->st[1] += vx * time_resolution * sn;
    S->st[2] += wz * time_resolution;
    double y = S->st[2];
    if (y > pi) y -= 2 * pi;
    else if (y < -pi) y += 2 * pi;
    S->st[2] = y;
    for (int a = 0; a < 7; a++) S->st[3 + a] = S->cur[2 + a];
  }
}

struct SimArgs {
  int n, ticks;
  const int* robots;
  SimSlot* sims;
  const double* cmd;   // [n][16] or null
  double* state;       // [n][10]
};
__global__ void __launch_bounds__(64) k_sim_step(SimArgs A) {
  const int k = blockIdx.x * 64 + (threadIdx.x & 63);
  if (k >= A.n) return;
  SimSlot* S = A.sims + A.robots[k];
  sim_apply(S, A.cmd ? A.cmd + 16 * (size_t)k : nullptr, A.ticks);
  for (int a = 0; a < 10; a++) A.state[10 * (size_t)k + a] = S->st[a];
}

struct MpcDense {   // topay_mpc_probe: the QP in the reference's order (zeroed by the host)
  double *P, *q, *A, *l, *u, *x, *y, *z;
  int* info;
};
struct MpcArgs {
  int n, periods, ticks, follow, probe;
  const int* robots;
  MpcSlot* slots;
  SimSlot* sims;             // follow
  const TrackDesc* desc;     // [n] end_traj; N = 0: none
  const double* arena;
  const double* t_cur;       // [n]
  const double* now_state;   // [n][10] (not follow)
  double* cmd;               // [n][periods][16]
  int* status;               // [n][periods][4]
  double* xopt;              // [n][129][3] or null
  double* states_out;        // [n][periods][10] or null
  MpcDense D;
};

struct MpcLds {
  double *C, *X, *XT, *Y, *TT, *PD, *Q, *KB, *ID, *RED, *OUT, *LAST, *XB, *XR;
};
__host__ __device__ inline size_t mpc_lds_doubles(int T, int nS) {
  return (size_t)kMpcC * (nS + 2) + 2 * 5 * (size_t)(nS + 2) + 2 * 7 * (size_t)(nS + 2) + 10 * (size_t)nS + 6 * (size_t)(5 * nS + 10) + (5 * (size_t)nS + 5) +
         6 * 64 + 4 * (size_t)T + 3 * (size_t)(T + 1) + 3 * (size_t)T;
}
__device__ __forceinline__ MpcLds mpc_lds(double* p, int T, int nS) {
  MpcLds L;
  L.C = p + kMpcC; p += kMpcC * (nS + 2);
  L.X = p + 5; p += 5 * (nS + 2);
  L.XT = p + 5; p += 5 * (nS + 2);
  L.Y = p + 7; p += 7 * (nS + 2);
  L.TT = p + 7; p += 7 * (nS + 2);
  L.PD = p; p += 5 * nS;
  L.Q = p; p += 5 * nS;
  L.KB = p + 30; p += 6 * (5 * nS + 10);
  L.ID = p + 5; p += 5 * nS + 5;
  L.RED = p; p += 6 * 64;
  L.OUT = p; p += 2 * T;
  L.LAST = p; p += 2 * T;
  L.XB = p; p += 3 * (T + 1);
  L.XR = p;
  return L;
}

// One OMPC::getCmd.  Wave-uniform control flow throughout.
__device__ __forceinline__ void mpc_one(const MpcArgs& A, int k, MpcSlot* S, const topay_mpc_params_t& P, const MpcLds& L, int lane, double tcur,
                                        const double* now, double* cmd, int* status) {
  const int T = P.predict_steps, dv = P.delay_num_v, dw = P.delay_num_w, dmin = dw, dd = dv - dw, nS = T - dmin, dimv = T - dv, dimw = T - dw;
  const int maxd = dv, n5 = 5 * nS;
  const double dt = P.dt;
  const int mode = S->mode;
  const TrackDesc TD = A.desc[k];
  if (status && lane == 0) { status[TOPAY_MPC_ST_OUTCOME] = 0; status[TOPAY_MPC_ST_OUTER] = 0; status[TOPAY_MPC_ST_QP_ITERS] = 0; status[TOPAY_MPC_ST_MODE] = mode; }
  if (mode == 0 && TD.N <= 0) {   // !has_traj
    if (lane == 0) {
      cmd[0] = 0.0; cmd[1] = 0.0;
      for (int a = 0; a < 7; a++) { cmd[2 + a] = now[3 + a]; cmd[9 + a] = 0.0; }
      if (status) status[TOPAY_MPC_ST_OUTCOME] = 2;
      if (A.probe && A.D.info) A.D.info[1] = -1;   // the QP is not reached
    }
    return;
  }
  // the zero stages around the stage arrays, the zero rows around the band
  for (int t = lane; t < kMpcC * (nS + 2); t += 64) L.C[t - kMpcC] = 0.0;
  for (int t = lane; t < 5 * (nS + 2); t += 64) { L.X[t - 5] = 0.0; L.XT[t - 5] = 0.0; }
  for (int t = lane; t < 7 * (nS + 2); t += 64) { L.Y[t - 7] = 0.0; L.TT[t - 7] = 0.0; }
  for (int t = lane; t < 6 * (n5 + 10); t += 64) L.KB[t - 30] = 0.0;
  for (int t = lane; t < n5 + 5; t += 64) L.ID[t - 5] = 0.0;
  bool at_goal;
  if (mode == 0) {
    const FeasIO F = track_io(A.arena, TD);
    const double Ttot = track_duration(F);
    at_goal = tcur >= Ttot + 1.0;
    if (lane == 0) {
      double st[10], ds[10];
      track_state(F, Ttot, tcur + 1.0 / P.ctrl_freq, st);
      track_dstate(F, Ttot, tcur + 1.0 / P.ctrl_freq, ds);
      for (int a = 0; a < 7; a++) { cmd[2 + a] = st[3 + a]; cmd[9 + a] = ds[3 + a]; }
      if (at_goal) { cmd[0] = 0.0; cmd[1] = 0.0; }
    }
    if (!at_goal) {
      double t = tcur + dt;
      for (int base = 0; base < T; base += 64) {
        const double tg = track_times(t, dt, lane);
        const int j = base + lane;
        if (j < T) {
          double st[10];
          track_state(F, Ttot, tg, st);
          L.XR[3 * j] = st[0]; L.XR[3 * j + 1] = st[1]; L.XR[3 * j + 2] = st[2];
        }
      }
    }
  } else {
    at_goal = tcur >= 1.0;
    if (lane == 0) {
      cmd[0] = 0.0; cmd[1] = 0.0;
      for (int a = 0; a < 7; a++) { cmd[2 + a] = now[3 + a]; cmd[9 + a] = 0.0; }
    }
    if (!at_goal)
      for (int j = lane; j < T; j += 64) { L.XR[3 * j] = S->direct[0]; L.XR[3 * j + 1] = S->direct[1]; L.XR[3 * j + 2] = S->direct[2]; }
  }
  if (at_goal) {
    if (status && lane == 0) status[TOPAY_MPC_ST_OUTCOME] = 1;
    if (A.probe && lane == 0 && A.D.info) A.D.info[1] = -1;   // the QP is not reached
    return;
  }
  for (int t = lane; t < T; t += 64) { L.OUT[t] = S->output[t]; L.OUT[T + t] = S->output[TOPAY_MPC_MAX_STEPS + t]; }
  lds_sync();
  if (lane == 0) {   // smooth_yaw (ompc.h:153-182)
    const double pi = 3.14159265358979323846;
    double dyaw = L.XR[2] - now[2];
    while (dyaw >= pi / 2) { L.XR[2] -= pi * 2; dyaw = L.XR[2] - now[2]; }
    while (dyaw <= -pi / 2) { L.XR[2] += pi * 2; dyaw = L.XR[2] - now[2]; }
    for (int i = 0; i < T - 1; i++) {
      dyaw = L.XR[3 * (i + 1) + 2] - L.XR[3 * i + 2];
      while (dyaw >= pi / 2) { L.XR[3 * (i + 1) + 2] -= pi * 2; dyaw = L.XR[3 * (i + 1) + 2] - L.XR[3 * i + 2]; }
      while (dyaw <= -pi / 2) { L.XR[3 * (i + 1) + 2] += pi * 2; dyaw = L.XR[3 * (i + 1) + 2] - L.XR[3 * i + 2]; }
    }
  }
  const int j = lane;
  const bool act = j < nS;
  const bool hasv = act && j >= dd;
  const double sigma = P.qp_sigma, alpha = P.qp_alpha, oma = 1.0 - P.qp_alpha, rho = P.qp_rho, rho_eq = 1.0e3 * P.qp_rho;
  const double max_cv = P.max_accel * dt, max_comega = P.max_domega * dt;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double rr[7], rinv[7], lo[7], hi[7], xj[5] = {0, 0, 0, 0, 0}, yj[7] = {0, 0, 0, 0, 0, 0, 0}, zj[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < 7; r++) { rr[r] = (r >= 2 && r <= 4) ? rho_eq : rho; rinv[r] = 1.0 / rr[r]; }
  int outer = 0, qp_total = 0, unsolved = 0;
  for (int iter = 0; iter < P.max_iter; iter++) {
    if (lane == 0) {   // predictMotion(), last_output = output
      L.XB[0] = now[0]; L.XB[1] = now[1]; L.XB[2] = now[2];
      for (int i = 1; i < T + 1; i++) {
        const double vx = fmax(fmin(L.OUT[i - 1], P.max_speed), P.min_speed);
        const double w = fmax(fmin(L.OUT[T + i - 1], P.max_omega), -P.max_omega);
        double sn, cs;
        det_sincos(L.XB[3 * (i - 1) + 2], &sn, &cs);
        L.XB[3 * i] = L.XB[3 * (i - 1)] + vx * cs * dt;
        L.XB[3 * i + 1] = L.XB[3 * (i - 1) + 1] + vx * sn * dt;
        L.XB[3 * i + 2] = L.XB[3 * (i - 1) + 2] + w * dt;
      }
      for (int t = 0; t < 2 * T; t++) L.LAST[t] = L.OUT[t];
    }
    lds_sync();
    // ---- solveMPCDiff: the QP of this linearisation
    if (act) {
      const int nd = j + dmin;
      const double th = L.XB[3 * nd + 2], vx = L.OUT[nd];
      double sn, cs;
      det_sincos(th, &sn, &cs);
      const double B00 = cs * dt, B10 = sn * dt;
      const double A02 = -B10 * vx, A12 = B00 * vx;
      const double C0 = -A02 * th, C1 = -A12 * th;
      double* c = L.C + kMpcC * j;
      const bool m5 = hasv && j + 1 < nS, m6 = j + 1 < nS;
      c[0] = j > 0 ? -A02 : 0.0; c[1] = j > 0 ? -A12 : 0.0;
      c[2] = hasv ? -B00 : 0.0; c[3] = hasv ? -B10 : 0.0;
      c[4] = j > 0 ? -1.0 : 0.0; c[5] = hasv ? 1.0 : 0.0; c[6] = m5 ? 1.0 : 0.0; c[7] = m6 ? 1.0 : 0.0;
      c[8] = m5 ? -P.matrix_rd[0] * 2.0 : 0.0; c[9] = m6 ? -P.matrix_rd[1] * 2.0 : 0.0;
      c[10] = -dt; c[11] = 0.0;
      double b0, b1, b2;
      if (j == 0) {
        b0 = (L.XB[3 * nd] + A02 * th) + C0;
        b1 = (L.XB[3 * nd + 1] + A12 * th) + C1;
        b2 = th;
        if (dd > 0) { b0 += vx * B00; b1 += vx * B10; }
      } else {
        b0 = C0; b1 = C1; b2 = 0.0;
        if (j < dd) { b0 += vx * B00; b1 += vx * B10; }
      }
      const double sub_v = P.matrix_rd[0] * 2.0, sub_w = P.matrix_rd[1] * 2.0;
      double pv = 1.0, pw = 2 * (P.matrix_r[1] + sub_w);
      if (hasv) {
        pv = 2 * (P.matrix_r[0] + sub_v);
        if (j == dd) pv -= sub_v;
        if (j == nS - 1) pv -= sub_v;
      }
      if (j == 0) pw -= sub_w;
      if (j == nS - 1) pw -= sub_w;
      double* pd = L.PD + 5 * j;
      double* q = L.Q + 5 * j;
      pd[0] = pv; pd[1] = pw; q[0] = 0.0; q[1] = 0.0;
      for (int a = 0; a < 3; a++) { pd[2 + a] = P.matrix_q[a] * 2.0; q[2 + a] = -2 * P.matrix_q[a] * L.XR[3 * nd + a]; }
      lo[0] = -inf; hi[0] = inf;
      if (hasv) {
        lo[0] = P.min_speed; hi[0] = P.max_speed;
        if (j == dd) {   // vel continue
          const double vel_last = S->buff[2 * (maxd - 1)];
          lo[0] = fmax(P.min_speed, vel_last - max_cv);
          hi[0] = fmin(P.max_speed, vel_last + max_cv);
        }
      }
      lo[1] = -P.max_omega; hi[1] = P.max_omega;
      lo[2] = hi[2] = b0; lo[3] = hi[3] = b1; lo[4] = hi[4] = b2;
      lo[5] = m5 ? -max_cv : -inf; hi[5] = m5 ? max_cv : inf;
      lo[6] = m6 ? -max_comega : -inf; hi[6] = m6 ? max_comega : inf;
    }
    lds_sync();
    // ---- K = P + sigma I + A' R A, eleven columns at a time (columns 11 apart share no row), then L D L'
    for (int col = 0; col < 11; col++) {
      if (act)
        for (int a = 0; a < 5; a++) L.XT[5 * j + a] = ((5 * j + a) % 11 == col) ? 1.0 : 0.0;
      lds_sync();
      double px[5];
      if (act) {
        double ax[7];
        mpc_Ax(L.C, L.XT, j, ax);
        mpc_Px(L.C, L.PD, L.XT, j, px);
        for (int r = 0; r < 7; r++) L.TT[7 * j + r] = rr[r] * ax[r];
      }
      lds_sync();
      if (act) {
        double g[5];
        mpc_ATy(L.C, L.TT, j, g);
        for (int a = 0; a < 5; a++) {
          const int i = 5 * j + a, kk = ((i - col) % 11 + 11) % 11;
          if (kk <= 5) L.KB[6 * i + kk] = (kk <= i) ? (px[a] + sigma * L.XT[i]) + g[a] : 0.0;
        }
      }
    }
    lds_sync();
    if (lane == 0) mpc_band_factor(L.KB, L.ID, n5);
    // ---- ADMM from the x, y of the QP before (zero for the first)
    if (act) {
      for (int a = 0; a < 5; a++) L.X[5 * j + a] = xj[a];
      for (int r = 0; r < 7; r++) L.Y[7 * j + r] = yj[r];
    }
    lds_sync();
    if (act) {
      mpc_Ax(L.C, L.X, j, zj);
      for (int r = 0; r < 7; r++) L.TT[7 * j + r] = rr[r] * zj[r] - yj[r];
    }
    lds_sync();
    if (act) {
      double g[5];
      mpc_ATy(L.C, L.TT, j, g);
      for (int a = 0; a < 5; a++) L.XT[5 * j + a] = (sigma * xj[a] - L.Q[5 * j + a]) + g[a];
    }
    lds_sync();
    int it = 0, solved = 0;
    for (;;) {
      it++;
      if (lane == 0) mpc_band_solve(L.KB, L.ID, L.XT, n5);
      lds_sync();
      if (act) {
        double zt[7];
        mpc_Ax(L.C, L.XT, j, zt);
        for (int a = 0; a < 5; a++) { xj[a] = alpha * L.XT[5 * j + a] + oma * xj[a]; L.X[5 * j + a] = xj[a]; }
        for (int r = 0; r < 7; r++) {
          const double zr = alpha * zt[r] + oma * zj[r];
          const double w = zr + yj[r] * rinv[r];
          zj[r] = fmin(fmax(w, lo[r]), hi[r]);
          yj[r] = rr[r] * (w - zj[r]);
          L.Y[7 * j + r] = yj[r];
          L.TT[7 * j + r] = rr[r] * zj[r] - yj[r];
        }
      }
      lds_sync();
      const bool check = (it % 10 == 0) || it >= P.qp_max_iter;
      if (check) {
        double m[6] = {0, 0, 0, 0, 0, 0};   // |Ax - z|, |Ax|, |z|, |Px + q + A'y|, |Px|, |A'y|
        if (act) {
          double ax[7], px[5], g[5];
          mpc_Ax(L.C, L.X, j, ax);
          mpc_Px(L.C, L.PD, L.X, j, px);
          mpc_ATy(L.C, L.Y, j, g);
          for (int r = 0; r < 7; r++) { m[0] = fmax(m[0], fabs(ax[r] - zj[r])); m[1] = fmax(m[1], fabs(ax[r])); m[2] = fmax(m[2], fabs(zj[r])); }
          for (int a = 0; a < 5; a++) {
            m[3] = fmax(m[3], fabs((px[a] + L.Q[5 * j + a]) + g[a])); m[4] = fmax(m[4], fabs(px[a])); m[5] = fmax(m[5], fabs(g[a]));
          }
        }
        for (int a = 0; a < 6; a++) L.RED[6 * lane + a] = m[a];
      }
      if (act) {
        double g[5];
        mpc_ATy(L.C, L.TT, j, g);
        for (int a = 0; a < 5; a++) L.XT[5 * j + a] = (sigma * xj[a] - L.Q[5 * j + a]) + g[a];
      }
      lds_sync();
      if (check) {
        double m[6] = {0, 0, 0, 0, 0, 0}, nq = 0.0;
        for (int l2 = 0; l2 < 64; l2++)
          for (int a = 0; a < 6; a++) m[a] = fmax(m[a], L.RED[6 * l2 + a]);
        for (int t = 0; t < n5; t++) nq = fmax(nq, fabs(L.Q[t]));
        const double eps_p = P.qp_eps_abs + P.qp_eps_rel * fmax(m[1], m[2]);
        const double eps_d = P.qp_eps_abs + P.qp_eps_rel * fmax(fmax(m[4], m[5]), nq);
        if (m[0] <= eps_p && m[3] <= eps_d) { solved = 1; break; }
        if (it >= P.qp_max_iter) break;
      }
    }
    qp_total += it;
    outer = iter + 1;
    if (!solved) unsolved = 1;
    if (A.probe) {
      const int dimx = 3 * nS, mx = dimv + dimw, nx = dimx + mx;
      const MpcDense& D = A.D;
      if (act) {
        const double* c = L.C + kMpcC * j;
        const int iv = dimx + (j - dd), iw = dimx + dimv + j;
        const int row[7] = {j - dd, dimv + j, mx + 3 * j, mx + 3 * j + 1, mx + 3 * j + 2, mx + dimx + (j - dd), mx + dimx + (dimv - 1) + j};
        const bool has[7] = {hasv, true, true, true, true, c[6] != 0.0, c[7] != 0.0};
        for (int a = 0; a < 3; a++) {
          if (D.P) D.P[(size_t)(3 * j + a) * nx + 3 * j + a] = L.PD[5 * j + 2 + a];
          if (D.q) D.q[3 * j + a] = L.Q[5 * j + 2 + a];
          if (D.x) D.x[3 * j + a] = xj[2 + a];
        }
        if (hasv) {
          if (D.P) { D.P[(size_t)iv * nx + iv] = L.PD[5 * j]; if (has[5]) { D.P[(size_t)iv * nx + iv + 1] = c[8]; D.P[(size_t)(iv + 1) * nx + iv] = c[8]; } }
          if (D.x) D.x[iv] = xj[0];
        }
        if (D.P) { D.P[(size_t)iw * nx + iw] = L.PD[5 * j + 1]; if (has[6]) { D.P[(size_t)iw * nx + iw + 1] = c[9]; D.P[(size_t)(iw + 1) * nx + iw] = c[9]; } }
        if (D.x) D.x[iw] = xj[1];
        if (D.A) {
          if (hasv) D.A[(size_t)row[0] * nx + iv] = 1.0;
          D.A[(size_t)row[1] * nx + iw] = 1.0;
          for (int a = 0; a < 3; a++) D.A[(size_t)row[2 + a] * nx + 3 * j + a] = 1.0;
          if (j > 0) {
            for (int a = 0; a < 3; a++) D.A[(size_t)row[2 + a] * nx + 3 * (j - 1) + a] = c[4];
            D.A[(size_t)row[2] * nx + 3 * (j - 1) + 2] = c[0];
            D.A[(size_t)row[3] * nx + 3 * (j - 1) + 2] = c[1];
          }
          if (hasv) { D.A[(size_t)row[2] * nx + iv] = c[2]; D.A[(size_t)row[3] * nx + iv] = c[3]; }
          D.A[(size_t)row[4] * nx + iw] = c[10];
          if (has[5]) { D.A[(size_t)row[5] * nx + iv] = -1.0; D.A[(size_t)row[5] * nx + iv + 1] = 1.0; }
          if (has[6]) { D.A[(size_t)row[6] * nx + iw] = -1.0; D.A[(size_t)row[6] * nx + iw + 1] = 1.0; }
        }
        for (int r = 0; r < 7; r++)
          if (has[r]) {
            if (D.l) D.l[row[r]] = lo[r];
            if (D.u) D.u[row[r]] = hi[r];
            if (D.y) D.y[row[r]] = yj[r];
            if (D.z) D.z[row[r]] = zj[r];
          }
      }
      if (lane == 0 && D.info) { D.info[0] = it; D.info[1] = solved; }
      return;
    }
    lds_sync();
    if (solved && lane == 0) {   // (else the reference's early return: output as it was)
      for (int i = 0; i < dv; i++) L.OUT[i] = S->buff[2 * i];
      for (int i = 0; i < dw; i++) L.OUT[T + i] = S->buff[2 * i + 1];
      for (int i = 0; i < dimv; i++) L.OUT[i + dv] = L.X[5 * (i + dd)];
      for (int i = 0; i < dimw; i++) L.OUT[T + i + dw] = L.X[5 * i + 1];
    }
    if (lane == 0) {
      double du = 0;
      for (int i = 0; i < T; i++) du = du + fabs(L.OUT[i] - L.LAST[i]) + fabs(L.OUT[T + i] - L.LAST[T + i]);
      L.RED[0] = du;
    }
    lds_sync();
    const double du = L.RED[0];
    lds_sync();
    if (du <= P.du_threshold) break;
  }
  if (lane == 0) {
    if (A.xopt) {   // predictMotion(xopt)
      double* b = A.xopt + 3 * (size_t)(TOPAY_MPC_MAX_STEPS + 1) * k;
      double tx = L.XB[0], ty = L.XB[1], tth = L.XB[2];
      b[0] = tx; b[1] = ty; b[2] = tth;
      for (int i = 1; i < T + 1; i++) {
        // xbar[i - 1].second.vx is what the last predictMotion() wrote: last_output, not the output of the QP after it
        const double thi = L.XB[3 * (i - 1) + 2], vxi = L.LAST[i - 1];
        double sn, cs;
        det_sincos(thi, &sn, &cs);
        const double Bx00 = cs * dt, Bx10 = sn * dt;
        const double Ax02 = -Bx10 * vxi, Ax12 = Bx00 * vxi;
        const double Cx0 = -Ax02 * thi, Cx1 = -Ax12 * thi;
        const double nx0 = ((tx + Ax02 * tth) + Bx00 * L.OUT[i - 1]) + Cx0;
        const double nx1 = ((ty + Ax12 * tth) + Bx10 * L.OUT[i - 1]) + Cx1;
        const double nx2 = tth + dt * L.OUT[T + i - 1];
        tx = nx0; ty = nx1; tth = nx2;
        b[3 * i] = tx; b[3 * i + 1] = ty; b[3 * i + 2] = tth;
      }
    }
    cmd[0] = L.OUT[dv];
    cmd[1] = L.OUT[T + dw];
    for (int i = 0; i + 1 < maxd; i++) { S->buff[2 * i] = S->buff[2 * (i + 1)]; S->buff[2 * i + 1] = S->buff[2 * (i + 1) + 1]; }
    S->buff[2 * (maxd - 1)] = L.OUT[dv]; S->buff[2 * (maxd - 1) + 1] = L.OUT[T + dw];
    for (int t = 0; t < T; t++) { S->output[t] = L.OUT[t]; S->output[TOPAY_MPC_MAX_STEPS + t] = L.OUT[T + t]; }
    if (status) { status[TOPAY_MPC_ST_OUTCOME] = unsolved ? 3 : 0; status[TOPAY_MPC_ST_OUTER] = outer; status[TOPAY_MPC_ST_QP_ITERS] = qp_total; }
  }
}

__global__ void __launch_bounds__(64) k_mpc_cmds(MpcArgs A) {
  const int k = blockIdx.x;
  if (k >= A.n) return;
  const int lane = threadIdx.x & 63;
  const int robot = A.robots[k];
  MpcSlot* S = A.slots + robot;
  const topay_mpc_params_t P = S->P;
  const MpcLds L = mpc_lds(TOPAY_MPC_LDS, P.predict_steps, P.predict_steps - P.delay_num_w);
  double tcur = A.t_cur[k];
  for (int p = 0; p < A.periods; p++) {
    const size_t row = (size_t)k * A.periods + p;
    double now[10];
    const double* src = A.follow ? A.sims[robot].st : A.now_state + 10 * (size_t)k;
    for (int a = 0; a < 10; a++) now[a] = src[a];
    double* cmd = A.cmd + 16 * row;
    mpc_one(A, k, S, P, L, lane, tcur, now, cmd, A.status ? A.status + TOPAY_MPC_ST_LEN * row : nullptr);
    if (A.probe || !A.follow) return;
    wave_global_sync();
    if (lane == 0) {
      sim_apply(A.sims + robot, cmd, A.ticks);
      if (A.states_out)
        for (int a = 0; a < 10; a++) A.states_out[10 * row + a] = A.sims[robot].st[a];
    }
    wave_global_sync();
    lds_sync();
    tcur = tcur + 1.0 / P.ctrl_freq;
  }
}

}  // namespace topay
