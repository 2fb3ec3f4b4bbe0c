// The stage-2 manipulator block of one even sample (manipulator_block<OCC>, a call: it takes the whole register file):
// forward kinematics of the arm's 12 collision spheres, their ESDF lookups, self collision, the Jacobian-transpose walk
// back to the joints and the joint position limits.  Reference lines at the block below.
#pragma once

#include <hip/hip_runtime.h>

#include "topay_esdf.h"
#include "topay_eval_ctx.h"
#include "topay_math.h"
#include "topay_wave.h"

// Spheres whose ESDF gathers are issued ahead of the one being finished, in a kernel built for one wave per SIMD and for
// two (where the other wave covers the latency and the request registers are what is scarce), and the scheduling fence at
// the end of a sphere's iteration in the latter (docs/EXPERIMENTS.md, rounds 4 and 5).
#define TOPAY_ESDF_LOOKAHEAD 2
#define TOPAY_ESDF_LOOKAHEAD_OCC2 1
#define TOPAY_OCC2_FENCE 1
// 1: work of the block whose result is exactly zero is skipped under scalar branches when no active lane of the wave needs
// it -- a sphere's base and arm-local force transforms when no lane has a force on it, the two torque walks when no lane
// has a force on any sphere (the comments at the skips say why every value keeps its bits).  0: the code paths of before,
// for the bit comparison of the two builds (tests/test_mani_skip.py) and the A/B.  A compile-time switch only.
#ifndef TOPAY_MANI_SKIP_IDLE
#define TOPAY_MANI_SKIP_IDLE 1
#endif

namespace topay {

// ---------------------------------------------------------------------------------------------
// Stage-2 manipulator block of one even sample: FK (moma_param.h:203-247), 12 ESDF lookups
// (moma_traj_opt.cpp:1477-1520), self collision (1521-1612), Jacobian-transpose (moma_param.h:249-337),
// joint position limits (1616-1666).
//
// World sphere centre  P_k = p0 + A * rho_k,  A = Rz(theta) * relative_R,  p0 = (x, y, h) + Rz(theta) * relative_t,
// where rho_k comes from the joint chain run in the arm-local frame (pure rotations).  relative_R is the
// reference's 0.7071068 literal matrix, i.e. not exactly orthonormal, so the joint torques are formed in the local
// frame from g' = A^T g:  tau_i = u_i . sum (rho - o_{i+1}) x g'  — the exact derivative of the reference's matrix
// products for any A, unlike the world-frame axis x r form.  Yaw and x, y are taken in the world frame (Rz exact).
// pos = (x, y, theta, q1..q7).  Returns cost and the "/K" gdT part; moma_grad[10] = d/d(x, y, theta, q).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void joint_rotate(double* R, int i, double c_, double s_) {
  if (i % 2 == 0) {  // R <- R * Rz(q): mixes columns 0,1
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double r0 = R[a * 3 + 0], r1 = R[a * 3 + 1];
      R[a * 3 + 0] = fma(r0, c_, r1 * s_);
      R[a * 3 + 1] = fma(r1, c_, -(r0 * s_));
    }
  } else {  // R <- R * Ry(q): mixes columns 0,2
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double r0 = R[a * 3 + 0], r2 = R[a * 3 + 2];
      R[a * 3 + 0] = fma(r0, c_, -(r2 * s_));
      R[a * 3 + 2] = fma(r0, s_, r2 * c_);
    }
  }
}

// Interface (round 5).  Nothing of the block's inputs or outputs travels through the stack any more:
//   * in: the sample (piece i, even sample index j, local half step, step) and its XY position -- the pose (theta, q1..q7)
//     is evaluated HERE from the coefficients in LDS (round 4 passed the ten pose values by value: 16 of the 32 argument
//     dwords went through scratch memory because the hidden return-value pointer took the 33rd register);
//   * out: five doubles in registers (an aggregate of at most 16 dwords is returned in VGPRs): d/dx, d/dy, d/dtheta, cost and
//     the "/K" dJ/dT part; the seven joint entries of moma_grad go to the lane's column of seven rows of the wave's LDS pass
//     buffer (mg_lds[q * 64], q = 0..6: the buffer is idle during the sample passes), each as soon as its torque is known --
//     what the 12-double return value in scratch memory did for the register pressure of the block's last part, without the
//     scratch memory.
// e = the sample's index in the candidate's self-collision block, -1 for a padding lane (results dropped, no HBM write).
struct ManiOut {
  double gx, gy, gth;
  double cost, gdT;
};
#ifdef TOPAY_ASM_MARKS   // (probe builds: comment lines in the assembly that delimit the sections of the block)
#define MMARK(k) asm volatile("; TOPAY_MARK " #k)
#else
#define MMARK(k) do { } while (0)
#endif
#ifdef TOPAY_STAMPS
__device__ long long g_mani_stamps[8];
#define MSTAMP(k)                                                                                   \
  do {                                                                                              \
    const long long now_ = (long long)__builtin_amdgcn_s_memtime();                                 \
    if (blockIdx.x == 0 && threadIdx.x == 0) g_mani_stamps[k] += now_ - mt_;                        \
    mt_ = now_;                                                                                     \
  } while (0)
#else
#define MSTAMP(k) do { } while (0)
#endif
// Register plan (round 4).  OCC = waves per SIMD the caller's kernel is built for: 1 -> 512 registers per lane, 2 -> 256.
// The block used to hold the 12 sphere centres AND 12 force accumulators (144 VGPRs) because the rare self-collision
// pairs add to the forces of two spheres at once, ahead of the per-sphere terms.  Now a sphere's force is born in the
// iteration of the sphere loop that consumes its centre (the arm-local force takes the centre's registers), and the pair
// contributions -- needed by fewer than one sample in a thousand -- are accumulated in an HBM block by the lanes that
// have any, in the pair order of before, and read back at the top of the sphere's iteration: same operands, same order,
// same bits as the 144-register version.  LA = spheres whose ESDF gathers are issued ahead (2 with one wave per SIMD;
// 1 with two, where the other wave covers the latency and the request registers are what is scarce).
template <int OCC>
__device__ __noinline__ ManiOut manipulator_block(const TOPAY_GLB DevMap* mp, lds_cdp cL, int rows, int pi, int pj, double half, double step,
                                                  double posx, double posy, int e, glb_dp mstash, lds_dp mg_lds) {
  dev_params_ref P = dev_params();
  const DevMap M = load_map(mp);
  const bool in_act = e >= 0;
  const double invK = topay_hold_f64(TOPAY_INV_K), ten = topay_hold_f64(10.0);
  const glb_dp in_stash = mstash + 36 * (in_act ? e : 0);
  // pose of the sample: order-0 polynomials of theta and the seven joints (the arc length is not part of the pose), in the
  // arithmetic of poly4 / make_basis
  double pos[10];
  pos[0] = posx; pos[1] = posy;
  double sth, cth;
  {
    const double s1 = pj * half;
    const double s2 = s1 * s1, s3 = s2 * s1, s4 = s2 * s2, s5 = s3 * s2;
#pragma unroll
    for (int d = 0; d < 9; d++) {
      if (d == 1) continue;
      lds_cdp c = cL + d * rows + 6 * pi;
      pos[d == 0 ? 2 : d + 1] = fma(c[5], s5, fma(c[4], s4, fma(c[3], s3, fma(c[2], s2, fma(c[1], s1, c[0])))));
    }
  }
  const double omg = (pj == 0 || pj == 2 * TOPAY_K) ? 0.5 : 1.0;
#if TOPAY_MANI_SKIP_IDLE
  // Lanes whose pose is not finite (or absurd: det_sincos_n turns |angle| >= 1e15 into NaN) never allow a skip: the skipped
  // arithmetic multiplies pose-derived factors by zero forces, which is zero only for finite factors.  A sum of magnitudes
  // is at least its largest term and NaN if a term is, so it is below 1e15 only if every angle and both coordinates are.
  unsigned long long forced_all;   // (wave-uniform: a lane mask in a scalar register pair)
  {
    double mag = fabs(pos[0]) + fabs(pos[1]);
#pragma unroll
    for (int d = 2; d < 10; d++) mag += fabs(pos[d]);
    forced_all = __ballot(in_act && !(mag < 1.0e15));
  }
  unsigned long long forced_any = forced_all;
#endif
  ManiOut out;
  double cost, gdTk;
  const double mu = P.relu_mu;
  const double w = omg * step;
#ifdef TOPAY_STAMPS
  long long mt_ = (long long)__builtin_amdgcn_s_memtime();
#endif
  double sq[7], cq[7];
  {
    // yaw and the seven joints, step by step across the eight angles (det_sincos_n: the constants of a step are formed once)
    double ang[8], sn8[8], cs8[8];
#pragma unroll
    for (int i = 0; i < 8; i++) ang[i] = pos[2 + i];
    det_sincos_n<8>(ang, sn8, cs8);
    sth = sn8[0]; cth = cs8[0];
#pragma unroll
    for (int i = 0; i < 7; i++) { sq[i] = sn8[1 + i]; cq[i] = cs8[1 + i]; }
  }
  MSTAMP(0);  // 8 sincos
  MMARK(0);
  double A[9];
  {
    const double Rz[9] = {cth, -sth, 0.0, sth, cth, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++)
        A[a * 3 + b] = Rz[a * 3 + 0] * P.relR[0 * 3 + b] + Rz[a * 3 + 1] * P.relR[1 * 3 + b] + Rz[a * 3 + 2] * P.relR[2 * 3 + b];
  }
  const double p0x = pos[0] + (cth * P.relT[0] - sth * P.relT[1]);
  const double p0y = pos[1] + (sth * P.relT[0] + cth * P.relT[1]);
  const double p0z = P.p0z;
  // walk 1: world sphere centres (the arm-local rho_k are not kept; the torque walks below regenerate them)
  // spheres per link: link0:{0,1} 1:{2} 2:{3,4} 3:{5} 4:{6,7} 5:{8} 6:{9,10} 7:{11}
  double Px[TOPAY_NSPH], Py[TOPAY_NSPH], Pz[TOPAY_NSPH];
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
        Px[sidx] = p0x + fma(A[2], lz, fma(A[1], ly, A[0] * lx));
        Py[sidx] = p0y + fma(A[5], lz, fma(A[4], ly, A[3] * lx));
        Pz[sidx] = p0z + fma(A[8], lz, fma(A[7], ly, A[6] * lx));
        sidx++;
      }
      q0 = fma(R[2], P.colli_length[i], q0);
      q1 = fma(R[5], P.colli_length[i], q1);
      q2 = fma(R[8], P.colli_length[i], q2);
      if (i == 7) break;
      joint_rotate(R, i, cq[i], sq[i]);
    }
  }
  MSTAMP(1);  // walk 1
  MMARK(1);
  // The joints' cosines wait in the lane's LDS column (the seven words that take the torques at the end) while the sphere
  // loop needs the registers: walk 2a reads them from there, walk 2b reads word i before torque i is written to it.  (They
  // and the sines used to be spilled to scratch memory across the loop by the compiler: 14 of the block's 25 spilled values.)
#pragma unroll
  for (int i = 0; i < 7; i++) mg_lds[i * 64] = cq[i];
  cost = 0.0;
  gdTk = 0.0;
  const double wMC = P.s2_mani_colli_weight, wSC = P.s2_self_colli_weight;
  // sphere pairs: collision_matrix == -1 <=> non-adjacent spheres (moma_param.h:128-143: at the zero pose
  // only self and neighbouring spheres overlap) — moma_traj_opt.cpp:1566-1611
  // The clearances of all 55 pairs are independent straight-line arithmetic; only a lane that sees a positive one walks
  // the penalty path, which recomputes the same expressions and keeps the forces of the two spheres in its column of the
  // HBM block (read-modify-write, pair order).
  bool anypair;
  {
    double worst[TOPAY_NSPH - 2];
    double wall = -1.0;
#pragma unroll
    for (int a = 0; a < TOPAY_NSPH - 2; a++) {
      worst[a] = -1.0;
#pragma unroll
      for (int b = a + 2; b < TOPAY_NSPH; b++) {
        const double dx = Px[a] - Px[b], dy = Py[a] - Py[b], dz = Pz[a] - Pz[b];
        const double dist = P.pair_rr2[a * TOPAY_NSPH + b] - fma(dz, dz, fma(dy, dy, dx * dx));
        worst[a] = fmax(worst[a], dist);
      }
      wall = fmax(wall, worst[a]);
    }
    anypair = in_act && wall > 0;
    if (anypair) {
      // (the centres are made opaque here: otherwise the compiler keeps the 165 coordinate differences of the screening
      // above alive for this path -- in scratch memory -- instead of recomputing the few it needs)
#pragma unroll
      for (int k = 0; k < TOPAY_NSPH; k++) { TOPAY_OPAQUE(Px[k]); TOPAY_OPAQUE(Py[k]); TOPAY_OPAQUE(Pz[k]); }
      const glb_dp sg = in_stash;
#pragma unroll
      for (int v = 0; v < 3 * TOPAY_NSPH; v++) sg[v] = 0.0;
#pragma unroll
      for (int a = 0; a < TOPAY_NSPH - 2; a++) {
        if (worst[a] > 0) {
#pragma unroll
          for (int b = a + 2; b < TOPAY_NSPH; b++) {
            const double dx = Px[a] - Px[b], dy = Py[a] - Py[b], dz = Pz[a] - Pz[b];
            const double dist = P.pair_rr2[a * TOPAY_NSPH + b] - fma(dz, dz, fma(dy, dy, dx * dx));
            if (dist > 0) {
              double pe, pd;
              smoothL1(P, dist, mu, pe, pd);
              const double sc = -w * wSC * pd * 2.0;
              sg[3 * a + 0] = fma(sc, dx, sg[3 * a + 0]);
              sg[3 * a + 1] = fma(sc, dy, sg[3 * a + 1]);
              sg[3 * a + 2] = fma(sc, dz, sg[3 * a + 2]);
              sg[3 * b + 0] = fma(-sc, dx, sg[3 * b + 0]);
              sg[3 * b + 1] = fma(-sc, dy, sg[3 * b + 1]);
              sg[3 * b + 2] = fma(-sc, dz, sg[3 * b + 2]);
              gdTk += omg * wSC * (pe * invK);
              cost += w * wSC * pe;
            }
          }
        }
      }
    }
  }
  MSTAMP(2);  // sphere pairs
  MMARK(2);
  // chassis top (spheres with index > 2, 1525-1539) and environment collision (1477-1520)
  double bFx = 0.0, bFy = 0.0, bMz = 0.0;  // base: x, y, yaw (everything rotates about the vertical axis through (x, y))
  constexpr int LA = OCC >= 2 ? TOPAY_ESDF_LOOKAHEAD_OCC2 : TOPAY_ESDF_LOOKAHEAD;  // spheres whose gathers are issued ahead
  Esdf3dReq rq[LA + 1];
  double Lx[TOPAY_NSPH], Ly[TOPAY_NSPH], Lz[TOPAY_NSPH];   // arm-local forces g' = A^T g
#pragma unroll
  for (int k = 0; k < LA; k++) esdf3d_issue(M, Px[k], Py[k], Pz[k], rq[k]);
#pragma unroll
  for (int k = 0; k < TOPAY_NSPH; k++) {
    if (k + LA < TOPAY_NSPH) esdf3d_issue(M, Px[k + LA], Py[k + LA], Pz[k + LA], rq[(k + LA) % (LA + 1)]);
    double Gx = 0.0, Gy = 0.0, Gz = 0.0;
    if (anypair) {
      const glb_cdp sg = in_stash;
      Gx = sg[3 * k + 0]; Gy = sg[3 * k + 1]; Gz = sg[3 * k + 2];
    }
    if (k >= 3) {
      const double height = P.sph_top[k] - Pz[k];
      if (height > 0) {
        double pe, pd;
        smoothL1(P, height, mu, pe, pd);
        Gz += -w * wSC * pd;
        gdTk += omg * wSC * (pe * invK);
        cost += w * wSC * pe;
      }
    }
    double d, gx, gy, gz;
#ifdef TOPAY_STAMPS
    {
      // exposed latency of this sphere's four pair gathers: cycles until they have returned (the 4 min(LA, spheres left)
      // issued after them may stay in flight), measured where the first of them is needed
      const long long w0_ = (long long)__builtin_amdgcn_s_memtime();
      constexpr int FULL = 4 * LA;   // (four pair gathers per sphere) s_waitcnt vmcnt(n): expcnt / lgkmcnt fields left at their maxima
      const int left = TOPAY_NSPH - 1 - k;
      if (left >= LA) __builtin_amdgcn_s_waitcnt(0x0f70 | (FULL & 15) | ((FULL >> 4) << 14));
      else if (left == 1) __builtin_amdgcn_s_waitcnt(0x0f70 | 4);
      else __builtin_amdgcn_s_waitcnt(0x0f70);
      const long long w1_ = (long long)__builtin_amdgcn_s_memtime();
      if (blockIdx.x == 0 && threadIdx.x == 0) { g_mani_stamps[6] += w1_ - w0_; g_mani_stamps[7] += 1; }
    }
#endif
    esdf3d_finish(M, rq[k % (LA + 1)], d, gx, gy, gz);
    const double viola = P.sph_viol[k] - d * ten;
    if (viola > 0) {
      double pe, pd;
      smoothL1(P, viola, mu, pe, pd);
      const double sc = -w * wMC * pd;
      Gx += sc * gx * ten; Gy += sc * gy * ten; Gz += sc * gz * ten;
      gdTk += omg * wMC * (pe * invK);
      cost += w * wMC * pe;
    }
#if TOPAY_MANI_SKIP_IDLE
    // Sphere k has a force in a lane only from the pair stash, the chassis top or an ESDF violation, and almost every sample
    // of a converging candidate has none.  The vote is over ACTIVE lanes: a padding lane computes on clamped inputs and its
    // results are dropped.  G is never -0.0 (it starts at +0.0, and a sum is -0.0 in round-to-nearest only if both terms
    // are), so a lane without a vote holds G = (+0, +0, +0) and, its pose being finite, the transforms below would give
    // bFx + 0, bFy + 0, bMz + (+-0) and L = (+-0, +-0, +-0).  bFx, bFy and bMz start at +0.0 and likewise never hold -0.0:
    // adding +-0 returns them bit for bit.  L = +0.0 in place of +-0 is read by the walks alone: added to or subtracted
    // from Fx, Fy, Fz and, times a finite factor, added to Mx, My, Mz -- accumulators that start at +0.0 as well.  So when
    // no active lane votes, the branch (scalar: the ballot is wave-uniform) changes no bit of any active lane's result.
    const unsigned long long forced_k = __ballot(in_act && !(Gx == 0.0 && Gy == 0.0 && Gz == 0.0)) | forced_all;
    forced_any |= forced_k;
    if (forced_k != 0) {
#endif
    bFx += Gx;
    bFy += Gy;
    bMz = fma(Px[k] - pos[0], Gy, fma(-(Py[k] - pos[1]), Gx, bMz));
    // g' = A^T g (arm-local frame); the world position is no longer needed
    Lx[k] = fma(A[6], Gz, fma(A[3], Gy, A[0] * Gx));
    Ly[k] = fma(A[7], Gz, fma(A[4], Gy, A[1] * Gx));
    Lz[k] = fma(A[8], Gz, fma(A[5], Gy, A[2] * Gx));
#if TOPAY_MANI_SKIP_IDLE
    } else {
      Lx[k] = 0.0; Ly[k] = 0.0; Lz[k] = 0.0;
    }
#endif
    if (OCC >= 2 && TOPAY_OCC2_FENCE) __builtin_amdgcn_sched_barrier(0);
  }
  MSTAMP(3);  // ESDF loop
  MMARK(3);
  // joints: tau_i = u_i . (Mo_beyond - o_{i+1} x F_beyond) with F, Mo = sums of g' and rho x g'.
  // walk 2a accumulates the totals, walk 2b peels off the links at or below each joint.
#if TOPAY_MANI_SKIP_IDLE
  // No active lane has a force on any sphere: every L is +-0, the walks' sums F and Mo stay +0.0 (they start there, see
  // above) and each torque is a sum of three products of a finite axis component with +0.0, that is +0.0 or -0.0.  The
  // seven words take +0.0 without the two chains of rotations.  Where a walk would have left -0.0 the difference does not
  // travel: the joint limits below add a nonzero term to the word or leave it, and sample_rest() and the row accumulation
  // of the gradient phase read the word only as a term of sums that start at +0.0 (qacc, aq[][]), where +0.0 and -0.0 add
  // the same.  (The cosines parked in the words are not needed on this path.)
  if (forced_any == 0) {
#pragma unroll
    for (int i = 0; i < 7; i++) mg_lds[i * 64] = 0.0;
  } else {
#endif
  double Fx = 0, Fy = 0, Fz = 0, Mx = 0, My = 0, Mz = 0;
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
      q0 = fma(R[2], P.colli_length[i], q0);
      q1 = fma(R[5], P.colli_length[i], q1);
      q2 = fma(R[8], P.colli_length[i], q2);
      if (i == 7) break;
      joint_rotate(R, i, mg_lds[i * 64], sq[i]);
    }
  }
  {
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    int sidx = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const int cnt = (i % 2 == 0) ? 2 : 1;
#pragma unroll
      for (int c = 0; c < cnt; c++) {  // remove link i's spheres from the "beyond" sums
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
      const double cqi_ = mg_lds[i * 64];   // (read before the torque takes the word)
      // joint i turns frame i about its local z (even i) or y (odd i) axis through o_{i+1}
      const int ac = (i % 2 == 0) ? 2 : 1;
      const double ax = R[0 * 3 + ac], ay = R[1 * 3 + ac], az = R[2 * 3 + ac];
      const double tx = Mx - fma(o1, Fz, -(o2 * Fy));
      const double ty = My - fma(o2, Fx, -(o0 * Fz));
      const double tz = Mz - fma(o0, Fy, -(o1 * Fx));
      mg_lds[i * 64] = fma(az, tz, fma(ay, ty, ax * tx));
      joint_rotate(R, i, cqi_, sq[i]);
    }
  }
#if TOPAY_MANI_SKIP_IDLE
  }
#endif
  MSTAMP(4);  // walks 2a/2b
  MMARK(4);
  // joint position limits — moma_traj_opt.cpp:1616-1666 (symmetric joint_pos_limit_max, reference quirk); the rare
  // contribution to a joint's entry is a read-modify-write of the lane's own LDS word
  const double wJP = P.s2_mani_pos_weight;
#pragma unroll
  for (int ji = 0; ji < 7; ji++) {
    double v = pos[ji + 3] - P.joint_pos_limit_max[ji];
    if (v > 0) {
      double pe, pd;
      smoothL1(P, v, mu, pe, pd);
      mg_lds[ji * 64] += w * wJP * pd;
      gdTk += omg * wJP * (pe * invK);
      cost += w * wJP * pe;
    }
    v = -P.joint_pos_limit_max[ji] - pos[ji + 3];
    if (v > 0) {
      double pe, pd;
      smoothL1(P, v, mu, pe, pd);
      mg_lds[ji * 64] -= w * wJP * pd;
      gdTk += omg * wJP * (pe * invK);
      cost += w * wJP * pe;
    }
  }
  MSTAMP(5);  // joint limits
  MMARK(5);
  out.gx = bFx;
  out.gy = bFy;
  out.gth = bMz;
  out.cost = cost;
  out.gdT = gdTk;
  return out;
}

}  // namespace topay
