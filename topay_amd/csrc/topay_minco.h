// The MINCO system of one trajectory (the reference's planner/include/utils/minco.hpp:824-900 and banded_system.hpp:66-145):
// the 6N x 6N banded matrix of the minimum-jerk spline's continuity conditions, its LU factorisation without pivoting, and
// the banded triangular sweeps that the spline's coefficients (minco_generate) and the adjoint solve of the gradient
// (eval_cost_grad, topay_eval.h) are formed with.  What is serial in the algorithm stays serial -- the 6N pivots of the LU
// on wave 0, the substitutions with one lane per right-hand side; the fills are divided over the NW waves of the workgroup.
#pragma once

#include <hip/hip_runtime.h>

#include "topay_eval_ctx.h"
#include "topay_wave.h"

namespace topay {

#define BAND(i, j) band[((i) - (j) + 6) * rows + (j)]

// Banded triangular sweeps with one lane per right-hand side (banded_system.hpp:96-118 and 123-145).
// The reference's substitutions are column sweeps: step j finalises x(j) and updates the six following (or
// preceding) entries of the same right-hand side.  The nine right-hand sides are independent, so lane d < 9 owns
// column d of the 6N x 9 block and carries the six pending entries in registers: a step is six independent
// multiply-subtracts with no LDS round trip and no barrier (the cross-lane version needed both, ~300 cycles per
// step).  Arithmetic and its order per entry are unchanged (mul, then sub, j ascending / descending).
//   MODE 0  L   x = b   (generate, forward):  b(i) -= A(i,j) b(j),            i = j+1..j+6
//   MODE 1  U   x = b   (generate, backward): b(i) -= A(i,j) (b(j)/A(j,j)),   i = j-1..j-6 ; stores b(j)/A(j,j)
//   MODE 2  U^T x = b   (adjoint, forward):   b(i) -= A(j,i) (b(j)/A(j,j)),   i = j+1..j+6 ; stores b(j)/A(j,j)
//   MODE 3  L^T x = b   (adjoint, backward):  b(i) -= A(j,i) b(j),            i = j-1..j-6
// rows = 6N is a multiple of 6: blocks of six steps with compile-time register indices.
//
// The factors are NOT resident in LDS (round 4): the band (84 N doubles) beside the right-hand sides (54 N) was the
// peak of the LDS plan and decided how many trajectories share a compute unit.  They stream from the candidate's LU
// block in HBM ([14][rows]: 13 diagonals, then the reciprocal diagonal; written once per evaluation by the
// factorisation) through two windows of 7 rows x 30 columns in LDS: a chunk is 24 steps (four blocks), all 64 lanes
// of the wave request the next chunk's window, the nine owner lanes sweep the current one, the requested values are
// written to the other window.  Window row r holds diagonal D0 + r (D0 = 7: the lower factor, modes 0 and 3; D0 = 0:
// the upper factor, modes 1 and 2), row 6 the reciprocal diagonal; window column = matrix column - clo.  Which value
// feeds which multiply-subtract is unchanged.
#define TOPAY_SWEEP_CHUNK 24
#define TOPAY_SWEEP_WCOLS 30
#define TOPAY_SWEEP_WIN (7 * TOPAY_SWEEP_WCOLS)   // doubles per window; the sweeps use two
// (the windows borrow the region behind the right-hand sides, EvalCtx::X: smallest at one piece)
static_assert(2 * TOPAY_SWEEP_WIN <= eval_borrow_doubles(1, 1) && 2 * TOPAY_SWEEP_WIN <= eval_borrow_doubles(1, 2) &&
              2 * TOPAY_SWEEP_WIN <= eval_borrow_doubles(1, 4), "the sweeps' windows fit behind the coefficients");
template <int MODE>
__device__ __forceinline__ void band_sweep(lds_dp v, bool owner, glb_cdp lu, lds_dp win, int rows, int lane) {
  constexpr bool FWD = (MODE == 0 || MODE == 2);
  constexpr bool SCALE = (MODE == 1 || MODE == 2);
  constexpr int D0 = (MODE == 0 || MODE == 3) ? 7 : 0;
  constexpr int CH = TOPAY_SWEEP_CHUNK, WC = TOPAY_SWEEP_WCOLS, WIN = TOPAY_SWEEP_WIN;
  constexpr int NEL = (SCALE ? 7 : 6) * WC;      // window elements in use
  constexpr int NQ = (NEL + 63) / 64;            // per lane
  double w[6];
  double x = 0.0;
#pragma unroll
  for (int t = 0; t < 6; t++) w[t] = 0.0;
  if (owner) {
    if (FWD) {
      x = v[0];
#pragma unroll
      for (int t = 0; t < 6; t++) w[t] = v[1 + t];
    } else {
      x = v[rows - 1];
#pragma unroll
      for (int t = 0; t < 6; t++) w[t] = v[rows - 2 - t];
    }
  }
  const int nchunk = (rows + CH - 1) / CH;
  // first matrix column of chunk k's window
  auto chunk_clo = [&](int k) { return FWD ? CH * k : rows - 1 - CH * k - (WC - 1); };
  auto request = [&](int k, double (&q)[NQ]) {
    const int clo = chunk_clo(k);
#pragma unroll
    for (int u = 0; u < NQ; u++) {
      const int e = lane + 64 * u;
      const int r = e / WC, cc = e - r * WC;
      int c = clo + cc;
      c = c < 0 ? 0 : (c > rows - 1 ? rows - 1 : c);   // columns outside the matrix only ever feed rows that do not exist
      const int d = (r < 6 ? D0 + r : 13);
      q[u] = lu[(d < 14 ? d : 13) * rows + c];         // (e >= NEL: a valid address, the value is dropped)
    }
  };
  auto deposit = [&](int k, const double (&q)[NQ]) {
    lds_dp wb = win + (k & 1) * WIN;
#pragma unroll
    for (int u = 0; u < NQ; u++) {
      const int e = lane + 64 * u;
      if (e < NEL) wb[e] = q[u];
    }
  };
  double q[NQ];
  request(0, q);
  deposit(0, q);
  lds_sync();
  for (int k = 0; k < nchunk; k++) {
    const bool more = k + 1 < nchunk;
    if (more) request(k + 1, q);
    if (owner) {
      lds_cdp wb = win + (k & 1) * WIN;
      const int clo = chunk_clo(k);
#pragma unroll 1
      for (int b0 = CH * k; b0 < CH * (k + 1) && b0 < rows; b0 += 6) {
        // everything the block reads from LDS, issued up front: 36 coefficients, 6 scales, 6 incoming entries
        double cf[6][6], sc[6], nw[6];
#pragma unroll
        for (int u = 0; u < 6; u++) {
          const int j = FWD ? b0 + u : rows - 1 - (b0 + u);
#pragma unroll
          for (int t = 1; t <= 6; t++) {
            int idx;
            if (MODE == 0) idx = (t - 1) * WC + (j - clo);            // A(j+t, j)
            else if (MODE == 1) idx = (6 - t) * WC + (j - clo);       // A(j-t, j)
            else if (MODE == 2) idx = (6 - t) * WC + (j + t - clo);   // A(j, j+t)
            else idx = (t - 1) * WC + (j - t - clo);                  // A(j, j-t)
            // Unconditional reads.  Where row i = j +- t falls outside the matrix the value is a never-written zero of
            // the band (modes 0, 1) or an unrelated entry (modes 2, 3) and only ever feeds window slots of rows that
            // do not exist and are never stored.
            cf[u][t - 1] = wb[idx];
          }
          if (SCALE) sc[u] = wb[6 * WC + (j - clo)];
          int in = FWD ? j + 7 : j - 7;
          in = in < 0 ? 0 : (in > rows - 1 ? rows - 1 : in);
          nw[u] = v[in];
        }
        double xo[6];
#pragma unroll
        for (int u = 0; u < 6; u++) {
          const double xs = SCALE ? x * sc[u] : x;
          xo[u] = xs;
#pragma unroll
          for (int t = 0; t < 6; t++) w[(u + t) % 6] -= cf[u][t] * xs;
          x = w[u % 6];
          w[u % 6] = nw[u];
        }
#pragma unroll
        for (int u = 0; u < 6; u++) {
          const int j = FWD ? b0 + u : rows - 1 - (b0 + u);
          v[j] = xo[u];
        }
      }
    }
    if (more) deposit(k + 1, q);
    lds_sync();
  }
}

// MINCO generate for an NW-wave workgroup: fills divided over all threads, LU on wave 0 (the pivots are a serial chain),
// substitutions on lanes 0..8 of wave 0 (band_sweep).  The band lives in the block the coefficients take
// afterwards: factorise, stash the factors in the candidate's LU block in HBM (the adjoint needs them again anyway), fill the
// right-hand sides over the band, substitute with the factors streamed back through two small windows.
template <int NW, int OCC>
__device__ __noinline__ void minco_generate(EvalCtx& C) {
  constexpr int NT = 64 * NW;
  const lds_dp c_Tp = C.Tp;
  const lds_dp c_X = C.X;
  const lds_dp c_gdT = C.gdT;
  const glb_cdp c_hd = C.hd, c_tl = C.tl;   // head / tail PVA, 9 x 3 col-major each (HBM: read once per evaluation)
  const glb_dp c_lu = C.lu;
  const glb_cdp c_x = C.x;
  dev_params_ref P = dev_params();
  const int tid = C.tid, lane = C.lane, wave = __builtin_amdgcn_readfirstlane(C.wave);
  const int N = __builtin_amdgcn_readfirstlane(C.N), rows = __builtin_amdgcn_readfirstlane(C.rows);
  lds_dp cL = C.cL;
  lds_dp band = cL;                 // [13][rows] while the system is factorised, then the coefficients' block
  lds_dp rdiag = cL + 13 * rows;
  glb_cdp Tau = c_x;
  glb_cdp Theta = c_x + N;
  glb_cdp Arc = c_x + 2 * N - 1;
  glb_cdp Vq = c_x + 3 * N - 1;

  // Everything this function reads from HBM is requested first -- the decision vector (written by the solver a moment
  // ago) and the boundary conditions -- so that the zero fills below run under the loads' latency instead of ahead of it
  // (the wave-level fences of the LDS hand-offs keep the compiler from moving loads up by itself).
  const double tau_v = tid < N ? Tau[tid] : 0.0;
  constexpr int NI = 9;   // inner-point values per thread: 9 (N - 1) <= 9 NT
  double inner_v[NI];
#pragma unroll
  for (int u = 0; u < NI; u++) {
    const int t = tid + NT * u;
    inner_v[u] = 0.0;
    if (t < 9 * (N - 1)) {
      const int i = t / 9, d = t - 9 * i;
      const int dq = d >= 2 ? d - 2 : 0;   // (clamped: the compiler may issue the loads of all three branches)
      inner_v[u] = d == 0 ? Theta[i] : (d == 1 ? Arc[i] : Vq[i * 7 + dq]);
    }
  }
  double bc_v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (tid < 9) {
    const int d = tid;
    bc_v[0] = c_hd[0 * 9 + d]; bc_v[1] = c_hd[1 * 9 + d]; bc_v[2] = c_hd[2 * 9 + d];
    bc_v[3] = (d == 1) ? Arc[N - 1] : c_tl[0 * 9 + d];   // minco_end_state(1,0) = Arc[N-1]
    bc_v[4] = c_tl[1 * 9 + d]; bc_v[5] = c_tl[2 * 9 + d];
  }
  for (int t = tid; t < 13 * rows; t += NT) band[t] = 0.0;
  if (tid < N) {
    double T1 = expC2(tau_v);  // calTfromTau, moma_traj_opt.h:778-786
    double T2 = T1 * T1, T3 = T2 * T1, T4 = T2 * T2, T5 = T4 * T1;
    c_Tp[0 * N + tid] = T1; c_Tp[1 * N + tid] = T2; c_Tp[2 * N + tid] = T3;
    c_Tp[3 * N + tid] = T4; c_Tp[4 * N + tid] = T5;
    c_gdT[tid] = 0.0;
  }
  wg_barrier<NW>();
  if (tid == 0) {
    BAND(0, 0) = 1.0; BAND(1, 1) = 1.0; BAND(2, 2) = 2.0;
  }
  if (tid < N - 1) {
    const int i = tid;
    const double T1 = c_Tp[i], T2 = c_Tp[N + i], T3 = c_Tp[2 * N + i], T4 = c_Tp[3 * N + i], T5 = c_Tp[4 * N + i];
    const int r = 6 * i;
    BAND(r + 3, r + 3) = 6.0;  BAND(r + 3, r + 4) = 24.0 * T1; BAND(r + 3, r + 5) = 60.0 * T2; BAND(r + 3, r + 9) = -6.0;
    BAND(r + 4, r + 4) = 24.0; BAND(r + 4, r + 5) = 120.0 * T1; BAND(r + 4, r + 10) = -24.0;
    BAND(r + 5, r) = 1.0; BAND(r + 5, r + 1) = T1; BAND(r + 5, r + 2) = T2; BAND(r + 5, r + 3) = T3;
    BAND(r + 5, r + 4) = T4; BAND(r + 5, r + 5) = T5;
    BAND(r + 6, r) = 1.0; BAND(r + 6, r + 1) = T1; BAND(r + 6, r + 2) = T2; BAND(r + 6, r + 3) = T3;
    BAND(r + 6, r + 4) = T4; BAND(r + 6, r + 5) = T5; BAND(r + 6, r + 6) = -1.0;
    BAND(r + 7, r + 1) = 1.0; BAND(r + 7, r + 2) = 2 * T1; BAND(r + 7, r + 3) = 3 * T2; BAND(r + 7, r + 4) = 4 * T3;
    BAND(r + 7, r + 5) = 5 * T4; BAND(r + 7, r + 7) = -1.0;
    BAND(r + 8, r + 2) = 2.0; BAND(r + 8, r + 3) = 6 * T1; BAND(r + 8, r + 4) = 12 * T2; BAND(r + 8, r + 5) = 20 * T3;
    BAND(r + 8, r + 8) = -2.0;
  }
  if (tid == NT - 1) {
    const int i = N - 1, R0 = 6 * N;
    const double T1 = c_Tp[i], T2 = c_Tp[N + i], T3 = c_Tp[2 * N + i], T4 = c_Tp[3 * N + i], T5 = c_Tp[4 * N + i];
    BAND(R0 - 3, R0 - 6) = 1.0; BAND(R0 - 3, R0 - 5) = T1; BAND(R0 - 3, R0 - 4) = T2; BAND(R0 - 3, R0 - 3) = T3;
    BAND(R0 - 3, R0 - 2) = T4; BAND(R0 - 3, R0 - 1) = T5;
    BAND(R0 - 2, R0 - 5) = 1.0; BAND(R0 - 2, R0 - 4) = 2 * T1; BAND(R0 - 2, R0 - 3) = 3 * T2; BAND(R0 - 2, R0 - 2) = 4 * T3;
    BAND(R0 - 2, R0 - 1) = 5 * T4;
    BAND(R0 - 1, R0 - 4) = 2; BAND(R0 - 1, R0 - 3) = 6 * T1; BAND(R0 - 1, R0 - 2) = 12 * T2; BAND(R0 - 1, R0 - 1) = 20 * T3;
  }
  wg_barrier<NW>();
  STAMP(C, 0);  // fills
  // LU without pivoting on wave 0 (banded_system.hpp:66-91); the other waves wait at the barrier below
  if (wave == 0) {
    const int t = lane / 7 + 1, u = lane - (lane / 7) * 7;
    // BAND(a, b) = band[(a - b + 6) rows + b]: the four entries a lane reads at pivot k are lane constants + k.  Lanes 42..63
    // read the pivot itself; a lane whose row or column lies beyond the matrix (the last six pivots) reads some other entry
    // of the band and writes nothing.
    const bool lane_in = lane < 42;
    const int o_kk = 6 * rows;
    const int o_ik = lane_in ? (t + 6) * rows : o_kk;
    const int o_ij = lane_in ? (t - u + 6) * rows + u : o_kk;
    const int o_kj = lane_in ? (6 - u) * rows + u : o_kk;
    for (int k = 0; k <= rows - 2; k++) {
      const int i = k + t, j = k + u;
      const bool act = lane_in && (i < rows) && (j < rows);
      // all four reads are issued ahead of the division: one LDS round trip per pivot instead of two, and no branch around
      // the multiply-subtract
      double akk = band[o_kk + k], aik = band[o_ik + k], aij = band[o_ij + k], akj = band[o_kj + k];
      TOPAY_OPAQUE(aij); TOPAY_OPAQUE(akj);   // (or the compiler moves these two reads back behind the division)
      const double m = aik / akk;
      const double nv = (u == 0) ? m : (aij - m * akj);
      lds_sync();
      if (act) band[o_ij + k] = nv;
      lds_sync();
    }
  }
  wg_barrier<NW>();
  STAMP(C, 1);  // LU
  for (int t = tid; t < rows; t += NT) rdiag[t] = 1.0 / BAND(t, t);
  wg_barrier<NW>();
  // factors to the candidate's LU block; nothing of the band is read from LDS after this
  for (int t = tid; t < 14 * rows; t += NT) c_lu[t] = band[t];
  if (NW == 1) lds_sync();   // (wg_global_barrier: the sweeps below read the factors back on this wave)
  else { wave_global_sync(); wg_barrier<NW>(); }
  // right-hand sides over the band: boundary conditions and inner points, zero elsewhere
  for (int t = tid; t < 9 * rows; t += NT) cL[t] = 0.0;
  wg_barrier<NW>();
  if (tid < 9) {
    const int d = tid;
    cL[d * rows + 0] = bc_v[0];
    cL[d * rows + 1] = bc_v[1];
    cL[d * rows + 2] = bc_v[2];
    cL[d * rows + rows - 3] = bc_v[3];
    cL[d * rows + rows - 2] = bc_v[4];
    cL[d * rows + rows - 1] = bc_v[5];
  }
#pragma unroll
  for (int u = 0; u < NI; u++) {
    const int t = tid + NT * u;
    if (t < 9 * (N - 1)) {
      const int i = t / 9, d = t - 9 * i;
      const int dq = d >= 2 ? d - 2 : 0;
      cL[d * rows + 6 * i + 5] = d >= 2 ? sigmoidC2(inner_v[u], P.joint_pos_limit_max[dq]) : inner_v[u];
    }
  }
  wg_barrier<NW>();
  if (wave == 0) {
    const bool owner = lane < 9;
    const lds_dp mine = cL + (owner ? lane : 8) * rows;
    band_sweep<0>(mine, owner, (glb_cdp)c_lu, c_X, rows, lane);
    band_sweep<1>(mine, owner, (glb_cdp)c_lu, c_X, rows, lane);
  }
  C.cl_in_lds = 1;
  wg_barrier<NW>();
  STAMP(C, 2);  // substitutions, LU stash
}

}  // namespace topay
