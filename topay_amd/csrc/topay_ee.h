// End-effector goals: MomaTrajOpt::optimizeEE (moma_traj_opt.cpp:5-46) for a batch of independent problems, its cost
// callback eeCostCallback (48-140), MomaParam::getFKPose (moma_param.h:339-373) and getEEGrads (375-468).
//   k_ee_pose     getFKPose of n states
//   k_ee_eval     one eeCostCallback per problem at an unconstrained x (the per-evaluation parity hook)
//   k_ee_goals    optimizeEE: the L-BFGS of lbfgs.hpp:439-722 with the Lewis-Overton search (276-389), one problem per lane
//   k_ee_qualify  what topay_ee_select asks of a problem: pose residual, isWholeBodyCollision
//   k_ee_select   per group the first qualified problem of smallest cost
//
// Mapping.  Ten unknowns have nothing to spread over a wave, and most of an evaluation is serial per problem (8 sincos, a
// chain of seven 3x3 products, 55 pair clearances), so a problem is a LANE: 64 problems per wave, one wave per workgroup,
// the tail wave masked by n (a lane >= n reads nothing).  A lane is a small state machine (EE_INIT: the first evaluation is
// due; EE_SEARCH: a trial point of the line search is due; EE_DONE) and every trip of k_ee_goals' main loop performs exactly
// ONE evaluation for every live lane: what a lane does between two evaluations -- bracketing, accepting the step, the
// convergence tests, the history update and the two-loop recursion -- is the cheap part and may diverge, the expensive part
// runs with the wave converged.  A finished lane idles until its wave is done.
//
// Deviations from the reference, stated in include/topay.h too:
//   * eeCostCallback accumulates into a gradient that lbfgs_optimize never clears (moma_traj_opt.cpp:135-137, lbfgs.hpp:504,
//     523, 318: uninitialised at the first call, the previous gradient afterwards).  Here the gradient is ASSIGNED.
//   * getEEGrads rebuilds R1 = R_0 .. dR_j .. R_i for every (i, j) (O(dof^3) products).  dR_j = R_j [u_j]x for both joint
//     kinds, so the orientation rows contribute ONE moment m (the axial vector of N - N^T, N = A^T W R^T, W the residual's
//     two rows) that every joint sees through its axis, and the position rows one force at the end effector: both ride on
//     the Jacobian-transpose walk of the collision spheres (topay_mani.h: arm-local frame, because relative_R is the
//     reference's 0.7071068 literal and not orthonormal).  Parity with the CPU restatement is to tolerance.
//
// Memory.  x, g, d, xp, gp (50 doubles) and the temporaries of an evaluation are registers: every loop over them is fully
// unrolled with compile-time indices (a runtime-indexed private array goes to scratch memory).  The L-BFGS history (s, y and
// y.s: 21 doubles per pair) is in device memory, lane-interleaved [wave][pair][component][lane], so that the lanes of a wave
// that touch the same pair touch one 512-byte row per component.  LDS plan of k_ee_goals, stated once:
//   alpha [64 pairs][64 lanes] doubles = 32 KB per wave (the ring of the two-loop recursion; lane l owns column l)
#pragma once

#include "topay_feas.h"
#include "topay_mani.h"

namespace topay {

constexpr int kEeMaxMem = 64;       // longest history topay_ee_goals accepts (the reference's mem_size)
constexpr int kEeMaxPast = 8;
constexpr int kEeHistRows = 21;     // per pair: s[10] | y[10] | y.s
constexpr int kEeAlphaDoubles = kEeMaxMem * 64;
#ifndef TOPAY_EE_ESDF_AHEAD
#define TOPAY_EE_ESDF_AHEAD 11
#endif

struct EeWeights {
  double cost_scale, mani_colli_weight, self_colli_weight, clearance;
};

// A map for ONE lane: the lanes of a wave may sit on different slots, so nothing of it is forced wave-uniform (load_map is).
__device__ __forceinline__ DevMap ee_lane_map(const DevMap* maps, int slot) {
  return maps[slot];
}

// Forward kinematics shared by every kernel here.  pos = (x, y, theta, q1..q7).
//   A = Rz(theta) relative_R, p0 = (x, y, h) + Rz(theta) relative_t;  R = R_0 .. R_6 and q7 = sum R_{0..i-1}[:, 2] colli_length[i]
//   in the arm-local frame;  sphere centres as sphere_centres() forms them;  end effector p0 + A q7, rotation A R.
struct EeFk {
  double sq[7], cq[7], sth, cth;
  double A[9], R[9];
  double p0x, p0y, p0z;
  double q7[3];
  double pose[9];   // getFKPose: position | row 0 | row 1 of the rotation
};
template <bool SPHERES>
__device__ __forceinline__ void ee_fk(dev_params_ref P, const double (&pos)[10], EeFk& K, double (&Px)[TOPAY_NSPH], double (&Py)[TOPAY_NSPH],
                                      double (&Pz)[TOPAY_NSPH]) {
  {
    double ang[8], sn8[8], cs8[8];
#pragma unroll
    for (int i = 0; i < 8; i++) ang[i] = pos[2 + i];
    det_sincos_n<8>(ang, sn8, cs8);
    K.sth = sn8[0]; K.cth = cs8[0];
#pragma unroll
    for (int i = 0; i < 7; i++) { K.sq[i] = sn8[1 + i]; K.cq[i] = cs8[1 + i]; }
  }
  {
    const double Rz[9] = {K.cth, -K.sth, 0.0, K.sth, K.cth, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++)
        K.A[a * 3 + b] = Rz[a * 3 + 0] * P.relR[0 * 3 + b] + Rz[a * 3 + 1] * P.relR[1 * 3 + b] + Rz[a * 3 + 2] * P.relR[2 * 3 + b];
  }
  K.p0x = pos[0] + (K.cth * P.relT[0] - K.sth * P.relT[1]);
  K.p0y = pos[1] + (K.sth * P.relT[0] + K.cth * P.relT[1]);
  K.p0z = P.p0z;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double q0 = 0.0, q1 = 0.0, q2 = 0.0;
  int sidx = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i == 7) {   // after seven joints: the end effector (getFKPose stops here; the last sphere lies beyond it on the same axis)
#pragma unroll
      for (int a = 0; a < 9; a++) K.R[a] = R[a];
      K.q7[0] = q0; K.q7[1] = q1; K.q7[2] = q2;
    }
    const int cnt = (i % 2 == 0) ? 2 : 1;
#pragma unroll
    for (int c = 0; c < cnt; c++) {
      if (SPHERES) {
        const double lx = fma(R[2], P.sph_off[sidx], q0), ly = fma(R[5], P.sph_off[sidx], q1), lz = fma(R[8], P.sph_off[sidx], q2);
        Px[sidx] = K.p0x + fma(K.A[2], lz, fma(K.A[1], ly, K.A[0] * lx));
        Py[sidx] = K.p0y + fma(K.A[5], lz, fma(K.A[4], ly, K.A[3] * lx));
        Pz[sidx] = K.p0z + fma(K.A[8], lz, fma(K.A[7], ly, K.A[6] * lx));
      }
      sidx++;
    }
    if (i == 7) break;
    q0 = fma(R[2], P.colli_length[i], q0);
    q1 = fma(R[5], P.colli_length[i], q1);
    q2 = fma(R[8], P.colli_length[i], q2);
    joint_rotate(R, i, K.cq[i], K.sq[i]);
  }
  K.pose[0] = K.p0x + fma(K.A[2], K.q7[2], fma(K.A[1], K.q7[1], K.A[0] * K.q7[0]));
  K.pose[1] = K.p0y + fma(K.A[5], K.q7[2], fma(K.A[4], K.q7[1], K.A[3] * K.q7[0]));
  K.pose[2] = K.p0z + fma(K.A[8], K.q7[2], fma(K.A[7], K.q7[1], K.A[6] * K.q7[0]));
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 3; b++)
      K.pose[3 + 3 * a + b] = fma(K.A[a * 3 + 2], K.R[6 + b], fma(K.A[a * 3 + 1], K.R[3 + b], K.A[a * 3 + 0] * K.R[b]));
}

__device__ __forceinline__ void ee_pose_of(dev_params_ref P, const double (&pos)[10], double (&pose)[9]) {
  EeFk K;
  double Px[TOPAY_NSPH], Py[TOPAY_NSPH], Pz[TOPAY_NSPH];
  ee_fk<false>(P, pos, K, Px, Py, Pz);
#pragma unroll
  for (int a = 0; a < 9; a++) pose[a] = K.pose[a];
}

// eeCostCallback (moma_traj_opt.cpp:48-140) at the unconstrained x, gradient assigned.
__device__ __forceinline__ void ee_cost(dev_params_ref P, const DevMap& M, const EeWeights& W, const double (&x)[10], const double (&ref)[9], double& f,
                                        double (&g)[10]) {
  double pos[10];
#pragma unroll
  for (int a = 0; a < 3; a++) pos[a] = x[a];
#pragma unroll
  for (int i = 0; i < 7; i++) pos[3 + i] = sigmoidC2(x[3 + i], P.joint_pos_limit_max[i]);
  EeFk K;
  double Px[TOPAY_NSPH], Py[TOPAY_NSPH], Pz[TOPAY_NSPH];
  ee_fk<true>(P, pos, K, Px, Py, Pz);
  // the lookups' gathers ahead of their arithmetic: TOPAY_EE_ESDF_AHEAD spheres in flight beside the one being finished
  constexpr int LA = TOPAY_EE_ESDF_AHEAD;
  Esdf3dReq rq[LA + 1];
#pragma unroll
  for (int k = 0; k < LA; k++) esdf3d_issue(M, Px[k], Py[k], Pz[k], rq[k]);
  const double mu = P.relu_mu;
  // objective: 0.5 |getFKPose - ee_ref|^2 (59-61)
  double res[9];
  double ee = 0.0;
#pragma unroll
  for (int a = 0; a < 9; a++) { res[a] = K.pose[a] - ref[a]; ee += res[a] * res[a]; }
  ee *= 0.5;
  double Gx[TOPAY_NSPH], Gy[TOPAY_NSPH], Gz[TOPAY_NSPH];   // pos_grads
  double sdf = 0.0;
  // environment (73-88)
#pragma unroll
  for (int k = 0; k < TOPAY_NSPH; k++) {
    if (k + LA < TOPAY_NSPH) esdf3d_issue(M, Px[k + LA], Py[k + LA], Pz[k + LA], rq[(k + LA) % (LA + 1)]);
    double d, gx, gy, gz;
    esdf3d_finish(M, rq[k % (LA + 1)], d, gx, gy, gz);
    const double viola = P.sph_r[k] * W.cost_scale * W.clearance - d * W.cost_scale;
    Gx[k] = 0.0; Gy[k] = 0.0; Gz[k] = 0.0;
    if (viola > 0) {
      double pe, pd;
      smoothL1(P, viola, mu, pe, pd);
      const double sc = -W.mani_colli_weight * pd;
      Gx[k] = sc * gx * W.cost_scale; Gy[k] = sc * gy * W.cost_scale; Gz[k] = sc * gz * W.cost_scale;
      sdf += W.mani_colli_weight * pe;
    }
  }
  // chassis top (93-107) and sphere pairs (109-130): collision_matrix == -1 <=> non-adjacent spheres (moma_param.h:128-143)
#pragma unroll
  for (int a = 0; a < TOPAY_NSPH; a++) {
    if (a > 2) {
      const double height = P.sph_top[a] - Pz[a];
      if (height > 0) {
        double pe, pd;
        smoothL1(P, height, mu, pe, pd);
        Gz[a] += -W.self_colli_weight * pd;
        sdf += W.self_colli_weight * pe;
      }
    }
#pragma unroll
    for (int b = a + 2; b < TOPAY_NSPH; b++) {
      const double dx = Px[a] - Px[b], dy = Py[a] - Py[b], dz = Pz[a] - Pz[b];
      const double dist = P.pair_rr2[a * TOPAY_NSPH + b] - (dx * dx + dy * dy + dz * dz);
      if (dist > 0) {
        double pe, pd;
        smoothL1(P, dist, mu, pe, pd);
        const double sc = -W.self_colli_weight * pd * 2.0;
        Gx[a] += sc * dx; Gy[a] += sc * dy; Gz[a] += sc * dz;
        Gx[b] -= sc * dx; Gy[b] -= sc * dy; Gz[b] -= sc * dz;
        sdf += W.self_colli_weight * pe;
      }
    }
  }
  f = ee + sdf;
  // ---- gradient: base in the world frame (Rz is exact), joints in the arm-local frame from g' = A^T g
  double bFx = res[0], bFy = res[1];
  double bMz = fma(K.pose[0] - pos[0], res[1], -((K.pose[1] - pos[1]) * res[0]));
  // d/dtheta of the two rotation rows: d row0 = -row1, d row1 = row0
#pragma unroll
  for (int b = 0; b < 3; b++) bMz += res[6 + b] * K.pose[3 + b] - res[3 + b] * K.pose[6 + b];
  double Lx[TOPAY_NSPH], Ly[TOPAY_NSPH], Lz[TOPAY_NSPH];
#pragma unroll
  for (int k = 0; k < TOPAY_NSPH; k++) {
    bFx += Gx[k];
    bFy += Gy[k];
    bMz = fma(Px[k] - pos[0], Gy[k], fma(-(Py[k] - pos[1]), Gx[k], bMz));
    Lx[k] = fma(K.A[6], Gz[k], fma(K.A[3], Gy[k], K.A[0] * Gx[k]));
    Ly[k] = fma(K.A[7], Gz[k], fma(K.A[4], Gy[k], K.A[1] * Gx[k]));
    Lz[k] = fma(K.A[8], Gz[k], fma(K.A[5], Gy[k], K.A[2] * Gx[k]));
  }
  // the end effector's force (position rows) and moment (rotation rows) in the arm-local frame
  const double Ex = fma(K.A[6], res[2], fma(K.A[3], res[1], K.A[0] * res[0]));
  const double Ey = fma(K.A[7], res[2], fma(K.A[4], res[1], K.A[1] * res[0]));
  const double Ez = fma(K.A[8], res[2], fma(K.A[5], res[1], K.A[2] * res[0]));
  double mx, my, mz;
  {
    double Wl[9], N[9];   // W' = A^T W (W: rows res[3..5], res[6..8], 0);  N = W' R^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int b = 0; b < 3; b++) Wl[i * 3 + b] = fma(K.A[3 + i], res[6 + b], K.A[i] * res[3 + b]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) N[i * 3 + k] = fma(Wl[i * 3 + 2], K.R[k * 3 + 2], fma(Wl[i * 3 + 1], K.R[k * 3 + 1], Wl[i * 3 + 0] * K.R[k * 3 + 0]));
    mx = N[7] - N[5]; my = N[2] - N[6]; mz = N[3] - N[1];
  }
  // joints: tau_i = u_i . (Mo_beyond - o_{i+1} x F_beyond), F / Mo = sums of g' and rho x g' (+ m) beyond joint i
  double Fx = Ex, Fy = Ey, Fz = Ez;
  double Mx = fma(K.q7[1], Ez, -(K.q7[2] * Ey)) + mx;
  double My = fma(K.q7[2], Ex, -(K.q7[0] * Ez)) + my;
  double Mz = fma(K.q7[0], Ey, -(K.q7[1] * Ex)) + mz;
  {
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    int sidx = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int cnt = (i % 2 == 0) ? 2 : 1;
#pragma unroll
      for (int c = 0; c < cnt; c++) {
        const double lx = fma(R[2], P.sph_off[sidx], q0), ly = fma(R[5], P.sph_off[sidx], q1), lz = fma(R[8], P.sph_off[sidx], q2);
        Fx += Lx[sidx]; Fy += Ly[sidx]; Fz += Lz[sidx];
        Mx = fma(ly, Lz[sidx], fma(-lz, Ly[sidx], Mx));
        My = fma(lz, Lx[sidx], fma(-lx, Lz[sidx], My));
        Mz = fma(lx, Ly[sidx], fma(-ly, Lx[sidx], Mz));
        sidx++;
      }
      if (i == 7) break;
      q0 = fma(R[2], P.colli_length[i], q0);
      q1 = fma(R[5], P.colli_length[i], q1);
      q2 = fma(R[8], P.colli_length[i], q2);
      joint_rotate(R, i, K.cq[i], K.sq[i]);
    }
  }
  double tau[7];
  {
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    int sidx = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const int cnt = (i % 2 == 0) ? 2 : 1;
#pragma unroll
      for (int c = 0; c < cnt; c++) {   // link i's spheres leave the "beyond" sums
        const double lx = fma(R[2], P.sph_off[sidx], o0), ly = fma(R[5], P.sph_off[sidx], o1), lz = fma(R[8], P.sph_off[sidx], o2);
        Fx -= Lx[sidx]; Fy -= Ly[sidx]; Fz -= Lz[sidx];
        Mx = fma(-ly, Lz[sidx], fma(lz, Ly[sidx], Mx));
        My = fma(-lz, Lx[sidx], fma(lx, Lz[sidx], My));
        Mz = fma(-lx, Ly[sidx], fma(ly, Lx[sidx], Mz));
        sidx++;
      }
      o0 = fma(R[2], P.colli_length[i], o0);
      o1 = fma(R[5], P.colli_length[i], o1);
      o2 = fma(R[8], P.colli_length[i], o2);
      const int ac = (i % 2 == 0) ? 2 : 1;   // joint i turns frame i about its z (even i) or y (odd i) axis through o_{i+1}
      const double ax = R[0 * 3 + ac], ay = R[1 * 3 + ac], az = R[2 * 3 + ac];
      const double tx = Mx - fma(o1, Fz, -(o2 * Fy));
      const double ty = My - fma(o2, Fx, -(o0 * Fz));
      const double tz = Mz - fma(o0, Fy, -(o1 * Fx));
      tau[i] = fma(az, tz, fma(ay, ty, ax * tx));
      joint_rotate(R, i, K.cq[i], K.sq[i]);
    }
  }
  g[0] = bFx; g[1] = bFy; g[2] = bMz;
#pragma unroll
  for (int i = 0; i < 7; i++) g[3 + i] = tau[i] * dQdVq(x[3 + i], P.joint_pos_limit_max[i]);   // getQtoVqGrad (137)
}

__global__ void __launch_bounds__(64) k_ee_pose(int n, const double* states, double* pose) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= n) return;
  dev_params_ref P = dev_params();
  double st[10], po[9];
#pragma unroll
  for (int a = 0; a < 10; a++) st[a] = states[10 * (size_t)i + a];
  ee_pose_of(P, st, po);
#pragma unroll
  for (int a = 0; a < 9; a++) pose[9 * (size_t)i + a] = po[a];
}

__global__ void __launch_bounds__(64) k_ee_eval(int n, const DevMap* maps, const int* map_ids, EeWeights W, const double* xs, const double* ee_ref, double* f,
                                                double* g) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= n) return;
  dev_params_ref P = dev_params();
  const DevMap M = ee_lane_map(maps, map_ids ? map_ids[i] : 0);
  double x[10], ref[9], gi[10], fi;
#pragma unroll
  for (int a = 0; a < 10; a++) x[a] = xs[10 * (size_t)i + a];
#pragma unroll
  for (int a = 0; a < 9; a++) ref[a] = ee_ref[9 * (size_t)i + a];
  ee_cost(P, M, W, x, ref, fi, gi);
  f[i] = fi;
#pragma unroll
  for (int a = 0; a < 10; a++) g[10 * (size_t)i + a] = gi[a];
}

struct EeGoalArgs {
  int n;
  const int* map_ids;       // [n] or null (slot 0)
  const double* seed;       // [n][10] moma_pos on entry
  const double* ee_ref;     // [n][9]
  EeWeights W;
  DevLbfgs L;
  double* hist;             // [waves][mem_size][kEeHistRows][64]
  double* states;           // [n][10]
  double* cost;             // [n]
  int* code;                // [n]
  int* iters;               // [n]
  int* evals;               // [n]
};

enum { EE_INIT = 0, EE_SEARCH = 1, EE_DONE = 2 };

__device__ __forceinline__ double ee_dot(const double (&a)[10], const double (&b)[10]) {   // vdot: serial, products and sums rounded apart
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 10; e++) s += a[e] * b[e];
  return s;
}
__device__ __forceinline__ bool ee_converged(const double (&x)[10], const double (&g)[10], double g_epsilon) {   // lbfgs.hpp: gnorm_inf / max(1, xnorm_inf)
  double gn = 0.0, xn = 0.0;
#pragma unroll
  for (int e = 0; e < 10; e++) { gn = fmax(gn, fabs(g[e])); xn = fmax(xn, fabs(x[e])); }
  return gn / fmax(1.0, xn) < g_epsilon;
}

__global__ void __launch_bounds__(64) k_ee_goals(EeGoalArgs A, const DevMap* maps) {
  __shared__ double alpha_lds[kEeAlphaDoubles];
  dev_params_ref P = dev_params();
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 64 + lane;
  const bool mine = i < A.n;
  const int m = A.L.mem_size, past = A.L.past;
  double* hist = A.hist + (size_t)blockIdx.x * m * kEeHistRows * 64 + lane;
  auto hrow = [&](int pair, int comp) -> double& { return hist[((size_t)pair * kEeHistRows + comp) * 64]; };
  double* alpha = alpha_lds + lane;
  DevMap M;
  double x[10], g[10], d[10], xp[10], gp[10], ref[9], pf[kEeMaxPast];
  int phase = EE_DONE, ret = 0, k = 0, evals = 0, end = 0, bound = 0, count = 0;
  bool brackt = false, touched = false;
  double fx = 0.0, stp = 0.0, finit = 0.0, dginit = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll
  for (int e = 0; e < 10; e++) { x[e] = 0.0; g[e] = 0.0; d[e] = 0.0; xp[e] = 0.0; gp[e] = 0.0; }
#pragma unroll
  for (int u = 0; u < kEeMaxPast; u++) pf[u] = 0.0;
  if (mine) {
    M = ee_lane_map(maps, A.map_ids ? A.map_ids[i] : 0);
#pragma unroll
    for (int a = 0; a < 9; a++) ref[a] = A.ee_ref[9 * (size_t)i + a];
#pragma unroll
    for (int a = 0; a < 3; a++) x[a] = A.seed[10 * (size_t)i + a];
#pragma unroll
    for (int q = 0; q < 7; q++) x[3 + q] = invSigmoidC2(A.seed[10 * (size_t)i + 3 + q], P.joint_pos_limit_max[q]);   // moma_traj_opt.cpp:12-14
    phase = EE_INIT;
  }
  // the start of a line search (lbfgs.hpp:276-306) from x, g, d, stp: leaves the first trial point in x
  auto begin_search = [&]() {
#pragma unroll
    for (int e = 0; e < 10; e++) { xp[e] = x[e]; gp[e] = g[e]; }
    count = 0; brackt = false; touched = false; lo = 0.0; hi = A.L.max_step;
    if (!(stp > 0.0)) { ret = TOPAY_LBFGSERR_INVALIDPARAMETERS; phase = EE_DONE; return; }
    dginit = ee_dot(gp, d);
    if (0.0 < dginit) { ret = TOPAY_LBFGSERR_INCREASEGRADIENT; phase = EE_DONE; return; }
    finit = fx;
#pragma unroll
    for (int e = 0; e < 10; e++) x[e] = xp[e] + stp * d[e];
    phase = EE_SEARCH;
  };
  while (__any(phase != EE_DONE)) {
    const bool live = phase != EE_DONE;
    if (live) {
      ee_cost(P, M, A.W, x, ref, fx, g);
      evals++;
    }
    if (phase == EE_INIT) {   // lbfgs.hpp:504-540
      pf[0] = fx;
#pragma unroll
      for (int e = 0; e < 10; e++) d[e] = -g[e];
      k = 0;
      if (ee_converged(x, g, A.L.g_epsilon)) { ret = TOPAY_LBFGS_CONVERGENCE; phase = EE_DONE; }
      else {
        stp = 1.0 / sqrt(ee_dot(d, d));
        k = 1; end = 0; bound = 0;
        begin_search();
      }
    } else if (phase == EE_SEARCH) {   // lbfgs.hpp:307-389, after the evaluation of the trial point
      ++count;
      int ls = 0;   // > 0: accepted after `ls` evaluations; < 0: failed; 0: another trial point
      if (isinf(fx) || isnan(fx)) ls = TOPAY_LBFGSERR_INVALID_FUNCVAL;
      else if (past > 0 && fabs(finit - fx) / (fabs(finit) + 1.0) < A.L.delta / past) ls = count;   // the reference's early accept (327-330)
      else {
        bool more = true;
        if (fx > finit + stp * (A.L.f_dec_coeff * dginit)) { hi = stp; brackt = true; }
        else if (ee_dot(g, d) < A.L.s_curv_coeff * dginit) lo = stp;
        else { ls = count; more = false; }
        if (more) {
          if (A.L.max_linesearch <= count) ls = TOPAY_LBFGSERR_MAXIMUMLINESEARCH;
          else if (brackt && (hi - lo) < A.L.machine_prec * hi) ls = TOPAY_LBFGSERR_WIDTHTOOSMALL;
          else {
            if (brackt) stp = 0.5 * (lo + hi);
            else stp *= 2.0;
            if (stp < A.L.min_step) ls = TOPAY_LBFGSERR_MINIMUMSTEP;
            else if (stp > A.L.max_step) {
              if (touched) ls = TOPAY_LBFGSERR_MAXIMUMSTEP;
              else { touched = true; stp = A.L.max_step; }
            }
          }
        }
      }
      if (ls < 0) {   // lbfgs.hpp:586-593
#pragma unroll
        for (int e = 0; e < 10; e++) { x[e] = xp[e]; g[e] = gp[e]; }
        ret = ls;
        phase = EE_DONE;
      } else if (ls == 0) {
#pragma unroll
        for (int e = 0; e < 10; e++) x[e] = xp[e] + stp * d[e];
      } else {   // the step is taken: lbfgs.hpp:600-700
        bool stop = false;
        if (ee_converged(x, g, A.L.g_epsilon)) { ret = TOPAY_LBFGS_CONVERGENCE; stop = true; }
        if (!stop && 0 < past) {
          const int slot = k % past;
          if (past <= k) {
            double old = 0.0;
#pragma unroll
            for (int u = 0; u < kEeMaxPast; u++) old = u == slot ? pf[u] : old;
            const double rate = fabs(old - fx) / fmax(1.0, fabs(fx));
            if (rate < A.L.delta) { ret = TOPAY_LBFGS_STOP; stop = true; }
          }
          if (!stop) {
#pragma unroll
            for (int u = 0; u < kEeMaxPast; u++) pf[u] = u == slot ? fx : pf[u];
          }
        }
        if (!stop && A.L.max_iterations != 0 && A.L.max_iterations <= k) { ret = TOPAY_LBFGSERR_MAXIMUMITERATION; stop = true; }
        if (stop) phase = EE_DONE;
        else {
          ++k;
          double sv[10], yv[10];
#pragma unroll
          for (int e = 0; e < 10; e++) { sv[e] = x[e] - xp[e]; yv[e] = g[e] - gp[e]; }
          const double ys = ee_dot(yv, sv), yy = ee_dot(yv, yv);
#pragma unroll
          for (int e = 0; e < 10; e++) { hrow(end, e) = sv[e]; hrow(end, 10 + e) = yv[e]; }
          hrow(end, 20) = ys;
#pragma unroll
          for (int e = 0; e < 10; e++) d[e] = -g[e];
          const double cau = ee_dot(sv, sv) * sqrt(ee_dot(gp, gp)) * A.L.cautious_factor;
          if (ys > cau) {
            ++bound;
            bound = m < bound ? m : bound;
            end = (end + 1) % m;
            // The two-loop recursion.  The lanes of the wave that are here run it together to the longest of their
            // histories; a lane with a shorter one is masked out of the remaining trips.
            int j = end;
            for (int t = 0; t < bound; ++t) {
              j = (j + m - 1) % m;
              double s = 0.0;
#pragma unroll
              for (int e = 0; e < 10; e++) s += hrow(j, e) * d[e];
              const double a = s / hrow(j, 20);
              alpha[j * 64] = a;
#pragma unroll
              for (int e = 0; e < 10; e++) d[e] += (-a) * hrow(j, 10 + e);
            }
            const double sc = ys / yy;
#pragma unroll
            for (int e = 0; e < 10; e++) d[e] *= sc;
            for (int t = 0; t < bound; ++t) {
              double s = 0.0;
#pragma unroll
              for (int e = 0; e < 10; e++) s += hrow(j, 10 + e) * d[e];
              const double beta = s / hrow(j, 20);
              const double a = alpha[j * 64] - beta;
#pragma unroll
              for (int e = 0; e < 10; e++) d[e] += a * hrow(j, e);
              j = (j + 1) % m;
            }
          }
          stp = 1.0;
          begin_search();
        }
      }
    }
  }
  if (mine) {
    const bool ok = ret == TOPAY_LBFGS_CONVERGENCE || ret == TOPAY_LBFGS_STOP || ret == TOPAY_LBFGS_CANCELED || ret == TOPAY_LBFGSERR_MAXIMUMITERATION;
#pragma unroll
    for (int a = 0; a < 3; a++) A.states[10 * (size_t)i + a] = ok ? x[a] : A.seed[10 * (size_t)i + a];
#pragma unroll
    for (int q = 0; q < 7; q++)
      A.states[10 * (size_t)i + 3 + q] = ok ? sigmoidC2(x[3 + q], P.joint_pos_limit_max[q]) : A.seed[10 * (size_t)i + 3 + q];   // moma_traj_opt.cpp:34-36
    A.cost[i] = fx;
    A.code[i] = ret;
    A.iters[i] = k;
    A.evals[i] = evals;
  }
}

__device__ __forceinline__ bool ee_code_ok(int c) {   // moma_traj_opt.cpp:30-31
  return c == TOPAY_LBFGS_CONVERGENCE || c == TOPAY_LBFGS_STOP || c == TOPAY_LBFGS_CANCELED || c == TOPAY_LBFGSERR_MAXIMUMITERATION;
}

// qualified[i] = success code && |getFKPose(state) - ee_ref| <= pose_tol && (!collision_free || !isWholeBodyCollision)
__global__ void __launch_bounds__(64) k_ee_qualify(int n, const DevMap* maps, const int* map_ids, const double* states, const int* code, const double* ee_ref,
                                                   double pose_tol, int collision_free, int* qualified) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= n) return;
  dev_params_ref P = dev_params();
  bool ok = ee_code_ok(code[i]);
  double st[10], po[9];
#pragma unroll
  for (int a = 0; a < 10; a++) st[a] = states[10 * (size_t)i + a];
  ee_pose_of(P, st, po);
  double r2 = 0.0;
#pragma unroll
  for (int a = 0; a < 9; a++) { const double r = po[a] - ee_ref[9 * (size_t)i + a]; r2 += r * r; }
  ok = ok && sqrt(r2) <= pose_tol;
  if (ok && collision_free) {
    const DevMap M = ee_lane_map(maps, map_ids ? map_ids[i] : 0);
    ok = !whole_body_collision(M, st);
  }
  qualified[i] = ok ? 1 : 0;
}

// One lane per group over its members in index order: the first of smallest cost among the qualified.
__global__ void __launch_bounds__(64) k_ee_select(int n, int n_groups, const int* group_of, const int* qualified, const double* cost, const double* states,
                                                  int* winner, double* goal) {
  const int gidx = blockIdx.x * 64 + (threadIdx.x & 63);
  if (gidx >= n_groups) return;
  int best = -1;
  double bc = 0.0;
  for (int i = 0; i < n; i++) {
    if (group_of[i] != gidx || !qualified[i]) continue;
    const double c = cost[i];
    if (best < 0 || c < bc) { best = i; bc = c; }
  }
  winner[gidx] = best;
  if (best >= 0)
    for (int a = 0; a < 10; a++) goal[10 * (size_t)gidx + a] = states[10 * (size_t)best + a];
}

}  // namespace topay
