// CPU restatement (checker, not product) of the tracking controller and the fake robot:
//   OMPC::init / setDirect / getCmd / predictMotion / solveMPCDiff   planner/src/ompc.cpp, include/planner/ompc.h
//   rcvVelCmdCallBack / normyaw / simCallBack                        simulator/fake_moma/src/moma_sim.cpp:208-229, 241-308
// Serial, with the reference's structure.  solveMPCDiff's QP is built twice: dense_qp() as the reference builds it (triplets in
// its variable and row order), and in the stage order the library's solver works in (include/topay.h states the method); the
// solver is the library's ADMM iteration in serial loops, with the same expression for every number, so that the library must
// reproduce it bit for bit.  The trajectory is not restated here (replan.hpp does that with libm): the caller hands getState's
// rows in, taken from the library's own playback, so that what is compared is the controller alone.
// sin / cos: prob_map::det_sincos, the library's deterministic pair.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "prob_map.hpp"

namespace ompc {

struct Params {   // = topay_mpc_params_t
  double du_threshold, dt, ctrl_freq;
  int max_iter, predict_steps, delay_num_v, delay_num_w;
  double max_omega, max_domega, max_speed, min_speed, max_accel;
  double matrix_q[3], matrix_r[2], matrix_rd[2];
  double qp_eps_abs, qp_eps_rel;
  double qp_rho, qp_sigma, qp_alpha;
  int qp_max_iter, reserved;
};

constexpr int kC = 12;

// ---- the stage-local products and the banded solver: the expressions of topay_amd/csrc/topay_mpc.h ---------------------
inline void Ax(const double* C, const double* X, int j, double* r) {
  const double* c = C + kC * j;
  const double* x = X + 5 * j;
  r[0] = c[5] * x[0];
  r[1] = x[1];
  r[2] = ((x[2] + c[4] * x[-3]) + c[0] * x[-1]) + c[2] * x[0];
  r[3] = ((x[3] + c[4] * x[-2]) + c[1] * x[-1]) + c[3] * x[0];
  r[4] = (x[4] + c[4] * x[-1]) + c[10] * x[1];
  r[5] = c[6] * (x[5] - x[0]);
  r[6] = c[7] * (x[6] - x[1]);
}
inline void ATy(const double* C, const double* Y, int j, double* g) {
  const double* c = C + kC * j;
  const double* cn = c + kC;
  const double* y = Y + 7 * j;
  g[0] = ((c[5] * y[0] + c[2] * y[2]) + c[3] * y[3]) + (c[-6] * y[-2] - c[6] * y[5]);
  g[1] = (y[1] + c[10] * y[4]) + (c[-5] * y[-1] - c[7] * y[6]);
  g[2] = y[2] + cn[4] * y[9];
  g[3] = y[3] + cn[4] * y[10];
  g[4] = ((y[4] + cn[0] * y[9]) + cn[1] * y[10]) + cn[4] * y[11];
}
inline void Px(const double* C, const double* PD, const double* X, int j, double* p) {
  const double* c = C + kC * j;
  const double* x = X + 5 * j;
  const double* pd = PD + 5 * j;
  p[0] = pd[0] * x[0] + (c[-4] * x[-5] + c[8] * x[5]);
  p[1] = pd[1] * x[1] + (c[-3] * x[-4] + c[9] * x[6]);
  p[2] = pd[2] * x[2];
  p[3] = pd[3] * x[3];
  p[4] = pd[4] * x[4];
}
inline void band_factor(double* KB, double* ID, int n) {
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
inline void band_solve(const double* KB, const double* ID, double* b, int n) {
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

struct Dense {   // the QP in the reference's order
  int nx = 0, nc = 0;
  std::vector<double> P, q, A, l, u, x, y, z;
  int iters = 0, solved = 0;
};

struct OMPC {
  Params P;
  int T, dv, dw, dmin, dd, nS, dimv, dimw, maxd;
  double max_cv, max_comega;
  std::vector<double> output, last_output;          // [2][T]: row r at r * T
  std::vector<double> output_buff;                  // [maxd][2]
  std::vector<double> xbar;                         // [T + 1][3] states; the inputs of xbar[i] are output(., i)
  std::vector<double> xref;                         // [T][3]
  int control_state = 0;
  double direct_pos[3] = {0, 0, 0};
  double now[3] = {0, 0, 0};
  // the solver's arrays (stage order, one zero stage before and after)
  std::vector<double> C_, X_, XT_, Y_, TT_, PD, Q, KB_, ID_, lo, hi, zz;
  double *C, *X, *XT, *Y, *TT, *KB, *ID;
  int last_qp_iters = 0, last_qp_solved = 0;

  explicit OMPC(const Params& p) : P(p) {   // OMPC::init
    T = p.predict_steps; dv = p.delay_num_v; dw = p.delay_num_w; dmin = std::min(dv, dw); dd = dv - dw; nS = T - dmin;
    dimv = T - dv; dimw = T - dw; maxd = std::max(dv, dw);
    max_comega = p.max_domega * p.dt;
    max_cv = p.max_accel * p.dt;
    output.assign(2 * T, 0.0); last_output = output;
    output_buff.assign(2 * maxd, 0.0);
    xbar.assign(3 * (T + 1), 0.0);
    xref.assign(3 * T, 0.0);
    C_.assign(kC * (nS + 2), 0.0); X_.assign(5 * (nS + 2), 0.0); XT_ = X_; Y_.assign(7 * (nS + 2), 0.0); TT_ = Y_;
    PD.assign(5 * nS, 0.0); Q = PD; KB_.assign(6 * (5 * nS + 10), 0.0); ID_.assign(5 * nS + 5, 0.0);
    lo.assign(7 * nS, 0.0); hi = lo; zz = lo;
    C = C_.data() + kC; X = X_.data() + 5; XT = XT_.data() + 5; Y = Y_.data() + 7; TT = TT_.data() + 7; KB = KB_.data() + 30; ID = ID_.data() + 5;
  }
  double& out(int r, int i) { return output[r * T + i]; }

  void predictMotion() {   // with stateTrans
    const double dt = P.dt;
    xbar[0] = now[0]; xbar[1] = now[1]; xbar[2] = now[2];
    for (int i = 1; i < T + 1; i++) {
      const double vx = std::fmax(std::fmin(out(0, i - 1), P.max_speed), P.min_speed);
      const double w = std::fmax(std::fmin(out(1, i - 1), P.max_omega), -P.max_omega);
      double sn, cs;
      prob_map::det_sincos(xbar[3 * (i - 1) + 2], &sn, &cs);
      xbar[3 * i] = xbar[3 * (i - 1)] + vx * cs * dt;
      xbar[3 * i + 1] = xbar[3 * (i - 1) + 1] + vx * sn * dt;
      xbar[3 * i + 2] = xbar[3 * (i - 1) + 2] + w * dt;
    }
  }
  void predictMotion(double* b) const {   // predictMotion(OMPCState*)
    const double dt = P.dt;
    double tx = xbar[0], ty = xbar[1], tth = xbar[2];
    b[0] = tx; b[1] = ty; b[2] = tth;
    for (int i = 1; i < T + 1; i++) {
      const double thi = xbar[3 * (i - 1) + 2], vxi = last_output[i - 1];   // xbar[i - 1].second.vx: set by the last predictMotion()
      double sn, cs;
      prob_map::det_sincos(thi, &sn, &cs);
      const double Bx00 = cs * dt, Bx10 = sn * dt;
      const double Ax02 = -Bx10 * vxi, Ax12 = Bx00 * vxi;
      const double Cx0 = -Ax02 * thi, Cx1 = -Ax12 * thi;
      const double nx0 = ((tx + Ax02 * tth) + Bx00 * output[i - 1]) + Cx0;
      const double nx1 = ((ty + Ax12 * tth) + Bx10 * output[i - 1]) + Cx1;
      const double nx2 = tth + dt * output[T + i - 1];
      tx = nx0; ty = nx1; tth = nx2;
      b[3 * i] = tx; b[3 * i + 1] = ty; b[3 * i + 2] = tth;
    }
  }
  void smooth_yaw() {
    const double pi = 3.14159265358979323846;
    double dyaw = xref[2] - now[2];
    while (dyaw >= pi / 2) { xref[2] -= pi * 2; dyaw = xref[2] - now[2]; }
    while (dyaw <= -pi / 2) { xref[2] += pi * 2; dyaw = xref[2] - now[2]; }
    for (int i = 0; i < T - 1; i++) {
      dyaw = xref[3 * (i + 1) + 2] - xref[3 * i + 2];
      while (dyaw >= pi / 2) { xref[3 * (i + 1) + 2] -= pi * 2; dyaw = xref[3 * (i + 1) + 2] - xref[3 * i + 2]; }
      while (dyaw <= -pi / 2) { xref[3 * (i + 1) + 2] += pi * 2; dyaw = xref[3 * (i + 1) + 2] - xref[3 * i + 2]; }
    }
  }

  // getLinearModel at xbar[node]
  struct Lin { double A02, A12, B00, B10, B21, C0, C1; };
  Lin linear(int node) const {
    const double th = xbar[3 * node + 2], vx = output[node];
    double sn, cs;
    prob_map::det_sincos(th, &sn, &cs);
    Lin m;
    m.B00 = cs * P.dt; m.B10 = sn * P.dt; m.B21 = P.dt;
    m.A02 = -m.B10 * vx; m.A12 = m.B00 * vx;
    m.C0 = -m.A02 * th; m.C1 = -m.A12 * th;
    return m;
  }

  // solveMPCDiff's matrices as the reference fills them: variables (states, v, w), rows (box v, box w, dynamics, rate v, rate w)
  void dense_qp(Dense& D) const {
    const int dimx = 3 * (T - dmin), dimu = dimv + dimw, nx = dimx + dimu;
    const int mx = dimu, my = dimx, mz = dimw + dimv - 2, nc = mx + my + mz;
    D.nx = nx; D.nc = nc;
    D.P.assign((size_t)nx * nx, 0.0); D.q.assign(nx, 0.0); D.A.assign((size_t)nc * nx, 0.0); D.l.assign(nc, 0.0); D.u.assign(nc, 0.0);
    auto Pm = [&](int r, int c) -> double& { return D.P[(size_t)r * nx + c]; };
    auto Am = [&](int r, int c) -> double& { return D.A[(size_t)r * nx + c]; };
    for (int i = 0, j = dmin; i < dimx; i += 3, j++)
      for (int a = 0; a < 3; a++) D.q[i + a] = -2 * P.matrix_q[a] * xref[3 * j + a];
    for (int i = 0; i < dimx; i += 3)
      for (int a = 0; a < 3; a++) Pm(i + a, i + a) = P.matrix_q[a] * 2.0;
    const double sub_v = P.matrix_rd[0] * 2.0, sub_w = P.matrix_rd[1] * 2.0;
    for (int i = dimx; i < dimx + dimv; i++) Pm(i, i) = 2 * (P.matrix_r[0] + sub_v);
    for (int i = dimx + dimv; i < nx; i++) Pm(i, i) = 2 * (P.matrix_r[1] + sub_w);
    Pm(dimx, dimx) -= sub_v;
    Pm(dimx + dimv - 1, dimx + dimv - 1) -= sub_v;
    Pm(dimx + dimv, dimx + dimv) -= sub_w;
    Pm(nx - 1, nx - 1) -= sub_w;
    for (int i = 0; i + 1 < dimv; i++) { Pm(dimx + i + 1, dimx + i) = -P.matrix_rd[0] * 2.0; Pm(dimx + i, dimx + i + 1) = -P.matrix_rd[0] * 2.0; }
    for (int i = 0; i + 1 < dimw; i++) { Pm(dimx + dimv + i + 1, dimx + dimv + i) = -P.matrix_rd[1] * 2.0; Pm(dimx + dimv + i, dimx + dimv + i + 1) = -P.matrix_rd[1] * 2.0; }
    // equality rows
    std::vector<double> b(my, 0.0);
    for (int i = 0; i < dimx; i++) Am(mx + i, i) = 1;
    Lin m = linear(dmin);
    const double tvx = output[dmin];
    b[0] = (xbar[3 * dmin] + m.A02 * xbar[3 * dmin + 2]) + m.C0;
    b[1] = (xbar[3 * dmin + 1] + m.A12 * xbar[3 * dmin + 2]) + m.C1;
    b[2] = xbar[3 * dmin + 2];
    auto chain = [&](int j, const Lin& g) {   // rows 3 j .. 3 j + 2 against the state before
      for (int a = 0; a < 3; a++) Am(mx + 3 * j + a, 3 * j + a - 3) = -1.0;
      Am(mx + 3 * j, 3 * j - 1) = -g.A02;
      Am(mx + 3 * j + 1, 3 * j - 1) = -g.A12;
    };
    if (dv > dw) {
      b[0] += tvx * m.B00;
      b[1] += tvx * m.B10;
      Am(mx + 2, dimx + dimv) = -m.B21;
      for (int j = 1; j < dv - dw; j++) {
        const Lin g = linear(j + dmin);
        const double vx = output[j + dmin];
        b[3 * j] = g.C0; b[3 * j + 1] = g.C1; b[3 * j + 2] = 0.0;
        b[3 * j] += vx * g.B00;
        b[3 * j + 1] += vx * g.B10;
        chain(j, g);
        Am(mx + 3 * j + 2, dimx + dimv + j) = -g.B21;
      }
      for (int j = dv - dw; j < dv - dw + (T - maxd); j++) {
        const Lin g = linear(j + dmin);
        b[3 * j] = g.C0; b[3 * j + 1] = g.C1; b[3 * j + 2] = 0.0;
        chain(j, g);
        Am(mx + 3 * j, dimx + j - (dv - dw)) = -g.B00;
        Am(mx + 3 * j + 1, dimx + j - (dv - dw)) = -g.B10;
        Am(mx + 3 * j + 2, dimx + dimv + j) = -g.B21;
      }
    } else {
      Am(mx + 0, dimx) = -m.B00;
      Am(mx + 1, dimx) = -m.B10;
      Am(mx + 2, dimx + dimv) = -m.B21;
      for (int j = 1; j < T - dv; j++) {
        const Lin g = linear(j + dv);
        b[3 * j] = g.C0; b[3 * j + 1] = g.C1; b[3 * j + 2] = 0.0;
        chain(j, g);
        Am(mx + 3 * j, dimx + j) = -g.B00;
        Am(mx + 3 * j + 1, dimx + j) = -g.B10;
        Am(mx + 3 * j + 2, dimx + dimv + j) = -g.B21;
      }
    }
    // rate rows
    for (int i = 0; i < dimv - 1; i++) { Am(mx + my + i, dimx + i) = -1.0; Am(mx + my + i, dimx + i + 1) = 1.0; }
    for (int i = dimv - 1; i < mz; i++) { Am(mx + my + i, dimx + i + 1) = -1.0; Am(mx + my + i, dimx + i + 2) = 1.0; }
    // boxes
    for (int i = 0; i < dimv; i++) { D.l[i] = P.min_speed; D.u[i] = P.max_speed; Am(i, dimx + i) = 1; }
    const double vel_last = output_buff[2 * (maxd - 1)];
    D.l[0] = std::fmax(P.min_speed, vel_last - max_cv);
    D.u[0] = std::fmin(P.max_speed, vel_last + max_cv);
    for (int i = dimv; i < mx; i++) { D.l[i] = -P.max_omega; D.u[i] = P.max_omega; Am(i, i + dimx) = 1; }
    for (int i = 0; i < my; i++) D.l[mx + i] = D.u[mx + i] = b[i];
    for (int i = 0; i < dimv - 1; i++) { D.l[mx + my + i] = -max_cv; D.u[mx + my + i] = max_cv; }
    for (int i = dimv - 1; i < mz; i++) { D.l[mx + my + i] = -max_comega; D.u[mx + my + i] = max_comega; }
  }

  // The QP in stage order, then the library's ADMM iteration from (X, Y).  Returns solved; the solution stays in X, Y, zz.
  bool solve_stage_qp() {
    const double dt = P.dt, inf = std::numeric_limits<double>::infinity();
    const int n5 = 5 * nS;
    const double sigma = P.qp_sigma, alpha = P.qp_alpha, oma = 1.0 - P.qp_alpha, rho = P.qp_rho, rho_eq = 1.0e3 * P.qp_rho;
    double rr[7], rinv[7];
    for (int r = 0; r < 7; r++) { rr[r] = (r >= 2 && r <= 4) ? rho_eq : rho; rinv[r] = 1.0 / rr[r]; }
    for (int j = 0; j < nS; j++) {
      const bool hasv = j >= dd;
      const int nd = j + dmin;
      const double th = xbar[3 * nd + 2], vx = output[nd];
      double sn, cs;
      prob_map::det_sincos(th, &sn, &cs);
      const double B00 = cs * dt, B10 = sn * dt;
      const double A02 = -B10 * vx, A12 = B00 * vx;
      const double C0 = -A02 * th, C1 = -A12 * th;
      double* c = C + kC * j;
      const bool m5 = hasv && j + 1 < nS, m6 = j + 1 < nS;
      c[0] = j > 0 ? -A02 : 0.0; c[1] = j > 0 ? -A12 : 0.0;
      c[2] = hasv ? -B00 : 0.0; c[3] = hasv ? -B10 : 0.0;
      c[4] = j > 0 ? -1.0 : 0.0; c[5] = hasv ? 1.0 : 0.0; c[6] = m5 ? 1.0 : 0.0; c[7] = m6 ? 1.0 : 0.0;
      c[8] = m5 ? -P.matrix_rd[0] * 2.0 : 0.0; c[9] = m6 ? -P.matrix_rd[1] * 2.0 : 0.0;
      c[10] = -dt; c[11] = 0.0;
      double b0, b1, b2;
      if (j == 0) {
        b0 = (xbar[3 * nd] + A02 * th) + C0;
        b1 = (xbar[3 * nd + 1] + A12 * th) + C1;
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
      double* pd = PD.data() + 5 * j;
      double* q = Q.data() + 5 * j;
      pd[0] = pv; pd[1] = pw; q[0] = 0.0; q[1] = 0.0;
      for (int a = 0; a < 3; a++) { pd[2 + a] = P.matrix_q[a] * 2.0; q[2 + a] = -2 * P.matrix_q[a] * xref[3 * nd + a]; }
      double* l = lo.data() + 7 * j;
      double* u = hi.data() + 7 * j;
      l[0] = -inf; u[0] = inf;
      if (hasv) {
        l[0] = P.min_speed; u[0] = P.max_speed;
        if (j == dd) {
          const double vel_last = output_buff[2 * (maxd - 1)];
          l[0] = std::fmax(P.min_speed, vel_last - max_cv);
          u[0] = std::fmin(P.max_speed, vel_last + max_cv);
        }
      }
      l[1] = -P.max_omega; u[1] = P.max_omega;
      l[2] = u[2] = b0; l[3] = u[3] = b1; l[4] = u[4] = b2;
      l[5] = m5 ? -max_cv : -inf; u[5] = m5 ? max_cv : inf;
      l[6] = m6 ? -max_comega : -inf; u[6] = m6 ? max_comega : inf;
    }
    // K, eleven columns at a time
    std::vector<double> xw(X, X + n5), yw(Y, Y + 7 * nS);   // the warm start (XT, TT are used by the probing)
    std::vector<double> pxs(n5);
    for (int col = 0; col < 11; col++) {
      for (int i = 0; i < n5; i++) XT[i] = (i % 11 == col) ? 1.0 : 0.0;
      for (int j = 0; j < nS; j++) {
        double ax[7];
        Ax(C, XT, j, ax);
        Px(C, PD.data(), XT, j, pxs.data() + 5 * j);
        for (int r = 0; r < 7; r++) TT[7 * j + r] = rr[r] * ax[r];
      }
      for (int j = 0; j < nS; j++) {
        double g[5];
        ATy(C, TT, j, g);
        for (int a = 0; a < 5; a++) {
          const int i = 5 * j + a, kk = ((i - col) % 11 + 11) % 11;
          if (kk <= 5) KB[6 * i + kk] = (kk <= i) ? (pxs[i] + sigma * XT[i]) + g[a] : 0.0;
        }
      }
    }
    band_factor(KB, ID, n5);
    for (int j = 0; j < nS; j++) {
      Ax(C, X, j, zz.data() + 7 * j);
      for (int r = 0; r < 7; r++) TT[7 * j + r] = rr[r] * zz[7 * j + r] - yw[7 * j + r];
    }
    for (int j = 0; j < nS; j++) {
      double g[5];
      ATy(C, TT, j, g);
      for (int a = 0; a < 5; a++) XT[5 * j + a] = (sigma * xw[5 * j + a] - Q[5 * j + a]) + g[a];
    }
    int it = 0;
    bool solved = false;
    double nq = 0.0;
    for (int t = 0; t < n5; t++) nq = std::fmax(nq, std::fabs(Q[t]));
    for (;;) {
      it++;
      band_solve(KB, ID, XT, n5);
      for (int j = 0; j < nS; j++) {
        double zt[7];
        Ax(C, XT, j, zt);
        for (int r = 0; r < 7; r++) {
          const int i = 7 * j + r;
          const double zr = alpha * zt[r] + oma * zz[i];
          const double w = zr + yw[i] * rinv[r];
          zz[i] = std::fmin(std::fmax(w, lo[i]), hi[i]);
          yw[i] = rr[r] * (w - zz[i]);
        }
      }
      for (int i = 0; i < n5; i++) { xw[i] = alpha * XT[i] + oma * xw[i]; X[i] = xw[i]; }
      for (int j = 0; j < nS; j++)
        for (int r = 0; r < 7; r++) { Y[7 * j + r] = yw[7 * j + r]; TT[7 * j + r] = rr[r] * zz[7 * j + r] - yw[7 * j + r]; }
      const bool check = (it % 10 == 0) || it >= P.qp_max_iter;
      double m[6] = {0, 0, 0, 0, 0, 0};
      if (check)
        for (int j = 0; j < nS; j++) {
          double ax[7], px[5], g[5];
          Ax(C, X, j, ax);
          Px(C, PD.data(), X, j, px);
          ATy(C, Y, j, g);
          for (int r = 0; r < 7; r++) {
            m[0] = std::fmax(m[0], std::fabs(ax[r] - zz[7 * j + r])); m[1] = std::fmax(m[1], std::fabs(ax[r])); m[2] = std::fmax(m[2], std::fabs(zz[7 * j + r]));
          }
          for (int a = 0; a < 5; a++) {
            m[3] = std::fmax(m[3], std::fabs((px[a] + Q[5 * j + a]) + g[a])); m[4] = std::fmax(m[4], std::fabs(px[a])); m[5] = std::fmax(m[5], std::fabs(g[a]));
          }
        }
      for (int j = 0; j < nS; j++) {
        double g[5];
        ATy(C, TT, j, g);
        for (int a = 0; a < 5; a++) XT[5 * j + a] = (sigma * xw[5 * j + a] - Q[5 * j + a]) + g[a];
      }
      if (check) {
        const double eps_p = P.qp_eps_abs + P.qp_eps_rel * std::fmax(m[1], m[2]);
        const double eps_d = P.qp_eps_abs + P.qp_eps_rel * std::fmax(std::fmax(m[4], m[5]), nq);
        if (m[0] <= eps_p && m[3] <= eps_d) { solved = true; break; }
        if (it >= P.qp_max_iter) break;
      }
    }
    last_qp_iters = it;
    last_qp_solved = solved ? 1 : 0;
    return solved;
  }
  void solveMPCDiff() {
    if (!solve_stage_qp()) return;
    for (int i = 0; i < dv; i++) out(0, i) = output_buff[2 * i];
    for (int i = 0; i < dw; i++) out(1, i) = output_buff[2 * i + 1];
    for (int i = 0; i < dimv; i++) out(0, i + dv) = X[5 * (i + dd)];
    for (int i = 0; i < dimw; i++) out(1, i + dw) = X[5 * i + 1];
  }
  // the stage solution in the reference's order
  void stage_to_dense(Dense& D) const {
    const int dimx = 3 * nS, mx = dimv + dimw;
    D.x.assign(D.nx, 0.0); D.y.assign(D.nc, 0.0); D.z.assign(D.nc, 0.0);
    for (int j = 0; j < nS; j++) {
      const bool hasv = j >= dd, m5 = hasv && j + 1 < nS, m6 = j + 1 < nS;
      for (int a = 0; a < 3; a++) D.x[3 * j + a] = X[5 * j + 2 + a];
      if (hasv) D.x[dimx + j - dd] = X[5 * j];
      D.x[dimx + dimv + j] = X[5 * j + 1];
      const int row[7] = {j - dd, dimv + j, mx + 3 * j, mx + 3 * j + 1, mx + 3 * j + 2, mx + dimx + (j - dd), mx + dimx + (dimv - 1) + j};
      const bool has[7] = {hasv, true, true, true, true, m5, m6};
      for (int r = 0; r < 7; r++)
        if (has[r]) { D.y[row[r]] = Y[7 * j + r]; D.z[row[r]] = zz[7 * j + r]; }
    }
    D.iters = last_qp_iters; D.solved = last_qp_solved;
  }
  void clear_warm() {
    std::fill(X_.begin(), X_.end(), 0.0); std::fill(Y_.begin(), Y_.end(), 0.0);
  }

  // OMPC::getCmd.  rows: getState(t).head(3) for t = t_cur + dt, += dt (T rows; unused in direct mode); arm_q / arm_dq:
  // getState / getDState(t_cur + 1 / ctrl_freq).tail(7).  status[4] as topay_mpc_cmds.  probe: stop after the first QP (state untouched).
  void getCmd(bool has_traj, double t_cur, double T_total, const double* now_moma_state, const double* rows, const double* arm_q, const double* arm_dq,
              double* cmd, int* status, double* xopt, Dense* probe = nullptr) {
    now[0] = now_moma_state[0]; now[1] = now_moma_state[1]; now[2] = now_moma_state[2];
    status[0] = 0; status[1] = 0; status[2] = 0; status[3] = control_state;
    if (control_state == 0 && !has_traj) {
      cmd[0] = 0.0; cmd[1] = 0.0;
      for (int i = 0; i < 7; i++) { cmd[9 + i] = 0.0; cmd[2 + i] = now_moma_state[3 + i]; }
      status[0] = 2;
      return;
    }
    bool at_goal = false;
    if (control_state == 0) {
      if (t_cur >= T_total + 1.0) at_goal = true;
      for (int i = 0; i < 7; i++) { cmd[9 + i] = arm_dq[i]; cmd[2 + i] = arm_q[i]; }
      if (at_goal) { cmd[0] = 0.0; cmd[1] = 0.0; status[0] = 1; return; }
      for (int j = 0; j < T; j++)
        for (int a = 0; a < 3; a++) xref[3 * j + a] = rows[3 * j + a];
    } else {
      cmd[0] = 0.0; cmd[1] = 0.0;
      for (int i = 0; i < 7; i++) { cmd[9 + i] = 0.0; cmd[2 + i] = now_moma_state[3 + i]; }
      if (t_cur >= 1.0) at_goal = true;
      if (at_goal) { status[0] = 1; return; }
      for (int j = 0; j < T; j++)
        for (int a = 0; a < 3; a++) xref[3 * j + a] = direct_pos[a];
    }
    smooth_yaw();
    clear_warm();
    const std::vector<double> keep = output;
    int iter, unsolved = 0, total = 0;
    for (iter = 0; iter < P.max_iter; iter++) {
      predictMotion();
      last_output = output;
      if (probe) {
        dense_qp(*probe);
        solve_stage_qp();
        stage_to_dense(*probe);
        output = keep;
        return;
      }
      solveMPCDiff();
      total += last_qp_iters;
      if (!last_qp_solved) unsolved = 1;
      status[1] = iter + 1;
      double du = 0;
      for (int i = 0; i < T; i++) du = du + std::fabs(out(0, i) - last_output[i]) + std::fabs(out(1, i) - last_output[T + i]);
      if (du <= P.du_threshold) break;
    }
    if (xopt) predictMotion(xopt);
    cmd[0] = out(0, dv);
    cmd[1] = out(1, dw);
    if (maxd > 0) {
      output_buff.erase(output_buff.begin(), output_buff.begin() + 2);
      output_buff.push_back(out(0, dv));
      output_buff.push_back(out(1, dw));
    }
    status[0] = unsolved ? 3 : 0; status[2] = total;
  }
};

// moma_sim; the ROS-time test of rcvVelCmdCallBack as a count (include/topay.h)
struct Sim {
  double st[10];
  double cur[16];
  std::vector<double> vw_buff;
  int received = 0, delay;
  Sim(const double* s0, int delay_cmds) : delay(delay_cmds) {
    for (int a = 0; a < 10; a++) st[a] = s0[a];
    for (int a = 0; a < 16; a++) cur[a] = 0.0;
  }
  static double normyaw(double yaw) {
    const double pi = 3.14159265358979323846;
    double y = yaw;
    if (y > pi) y -= 2 * pi;
    else if (y < -pi) y += 2 * pi;
    return y;
  }
  void step(const double* cmd, int ticks) {
    if (cmd) {
      for (int a = 0; a < 16; a++) cur[a] = cmd[a];
      cur[0] = 0.0; cur[1] = 0.0;
      vw_buff.push_back(cmd[0]); vw_buff.push_back(cmd[1]);
      if (received >= delay) {
        cur[0] = vw_buff[0]; cur[1] = vw_buff[1];
        vw_buff.erase(vw_buff.begin(), vw_buff.begin() + 2);
      }
      received++;
    }
    if (received == 0) return;
    const double time_resolution = 0.01;
    for (int i = 0; i < ticks; i++) {
      const double vx = cur[0], wz = cur[1];
      double sn, cs;
      prob_map::det_sincos(st[2], &sn, &cs);
      st[0] += vx * time_resolution * cs;
      st[1] += vx * time_resolution * sn;
      st[2] += wz * time_resolution;
      st[2] = normyaw(st[2]);
      for (int a = 0; a < 7; a++) st[3 + a] = cur[2 + a];
    }
  }
};

}  // namespace ompc
