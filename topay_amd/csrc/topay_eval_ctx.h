// What every part of an evaluation is handed: the parameter block in constant memory, the scalar maps of the NLP's
// reparametrisation and its penalty function, the context of one trajectory's workgroup (EvalCtx: LDS blocks and the
// candidate's global blocks), the plan of that LDS, and the phase stamps of the diagnostics build.
#pragma once

#include <hip/hip_runtime.h>

#include "topay_types.h"

// Optimizer/robot parameters live in constant memory: every access is a scalar load the compiler can re-issue at
// the point of use instead of keeping hundreds of SGPRs of kernel arguments alive across the whole solve.
__constant__ DevParams g_P;
// The parameter block through ONE base address per function, held in a scalar register pair: the compiler otherwise forms the
// address of every field it reads from the program counter anew (s_getpc_b64 + 64-bit add: three scalar instructions ahead of
// each of the 133 parameter loads of the manipulator block -- a wave issues one instruction per four cycles whatever its kind).
// The empty asm hides where the pointer comes from, so the fields become immediate offsets from it.
typedef const TOPAY_CST DevParams& dev_params_ref;
__device__ __forceinline__ dev_params_ref dev_params() {
#ifndef TOPAY_CPU_EMU
  const TOPAY_CST DevParams* p = (const TOPAY_CST DevParams*)&g_P;
  asm("" : "+s"(p));
  return *p;
#else
  return g_P;
#endif
}

namespace topay {

// ---------------------------------------------------------------------------------------------
// scalar pieces — moma_traj_opt.h:745-830
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double expC2(double tau) {
  return tau > 0.0 ? ((0.5 * tau + 1.0) * tau + 1.0) : 1.0 / ((0.5 * tau - 1.0) * tau + 1.0);
}
__device__ __forceinline__ double logC2(double T) {
  return T > 1.0 ? (sqrt(2.0 * T - 1.0) - 1.0) : (1.0 - sqrt(2.0 / T - 1.0));
}
__device__ __forceinline__ double dTdTau(double tau) {
  if (tau > 0) return tau + 1.0;
  double den = (0.5 * tau - 1.0) * tau + 1.0;
  return (1.0 - tau) / (den * den);
}
__device__ __forceinline__ double sigmoidC2(double vq, double max_q) {
  double e = expC2(vq);
  return 2.0 * max_q * e / (1.0 + e) - max_q;
}
__device__ __forceinline__ double invSigmoidC2(double q, double max_q) {
  double b = 0.5 * (max_q + q) / max_q;
  return logC2(b / (1 - b));
}
__device__ __forceinline__ double dQdVq(double vq, double max_q) {
  double e1 = expC2(vq) + 1.0;
  return 2.0 * max_q * dTdTau(vq) / (e1 * e1);
}
// smoothL1Penalty, only meaningful for x > 0 — moma_traj_opt.h:810-830 (constants precomputed in DevParams)
__device__ __forceinline__ void smoothL1(dev_params_ref P, double x, double mu, double& f, double& df) {
  if (x < mu) {
    f = (P.sl_f4c * x + P.sl_f3c) * x * x * x;
    df = (P.sl_d3c * x + P.sl_d2c) * x * x;
  } else {
    f = x - P.sl_half;
    df = 1.0;
  }
}
// 1/K as a constant factor: the reference divides by int_K in every penalty term (e.g. moma_traj_opt.cpp:1315); a
// multiplication by the rounded reciprocal differs by at most one ulp and saves an IEEE division per term.
#define TOPAY_INV_K (1.0 / TOPAY_K)

// ---------------------------------------------------------------------------------------------
// Evaluation context of one trajectory's workgroup: its LDS blocks (eval_lds_plan below) + the candidate's global blocks
// ---------------------------------------------------------------------------------------------
struct EvalCtx {
  int lane, N, rows, n;
  // thread index in the workgroup of NW waves, wave index, small cross-wave scratch
  int tid, wave;
  lds_dp red;    // eval_misc_doubles: [8] partial sums of a workgroup reduction (two phases; NW > 1) | [2 npass_lds] pass totals |
                 // [2][NW][64] per-round costs (NW > 1) | [NW] masks
  lds_dp adj;    // [9][rows] right-hand sides / solution of the adjoint solve (the coefficients' block: == cL)
  glb_dp coefg;  // HBM copy of the coefficients (the candidate's result block), read by the dJ/dT correction
  int cl_in_lds; // the coefficients of the last evaluation are still in C.cL (0 after a gradient phase -- they are in coefg)
  // LDS
  lds_dp cL;     // [9][rows]  MINCO coefficients, column d contiguous (the reference's col-major c)
  lds_dp Tp;     // [5][N]     T, T^2..T^5
  glb_cdp hd, tl; // HBM [27] each: head / tail PVA, 9x3 col-major (read once per evaluation by the right-hand side)
  int npass_lds;  // passes the pass-total block of the LDS plan is sized for
  lds_dp gdT;    // [N]        penalty dJ/dT accumulator
  lds_dp pcs;    // [4*(N+1)]  per-piece scratch: stage-1 tracking gradient (2N) | piece-end XY (2(N+1))
  lds_dp gC;     // [9][rows]  penalty dJ/dC accumulator, element (row, d) owned by the row lane of `row`
  glb_dp sbuf;   // HBM [14][sb_stride]: per-sample gradient rows parked between the cost and the gradient phase
  int sb_stride;
  glb_dp mstash; // HBM [sb_stride][36]: forces of self-colliding sphere pairs of a sample (manipulator_block; rarely touched)
  lds_dp pw;     // [26][6]    integer powers jj^k of the Simpson sample index (constant for the whole solve)
  lds_dp X;      // behind the coefficients, eval_borrow_doubles: [13N][2] XY prefixes / positional gradients + [NW][7 or 14][64] pass
                 // buffers; the two windows of band_sweep and the solver's alpha ring borrow it (the tail of the band during the LU)
  // global
  glb_cdp x;
  glb_dp g;
  glb_dp lu;          // [14*rows] stash
  glb_cdp init_xy;
  double sx, sy, ex, ey;           // start xy, goal xy
  double lam0, lam1, rho0, rho1;   // ALM state
  double fxe0, fxe1;               // final_xy_error of this evaluation (stage 2)
  // diagnostic build only (TOPAY_STAMPS): per-phase shader-clock accumulators, [16] per trajectory
  TOPAY_GLB long long* stamps;
  long long t_last;
};

// jj^k for jj = 0..25 (sample index within a piece; 25 is read but always multiplied by zero), k = 0..5: the local time of sample jj is jj * hs, so the
// monomial basis of coefficient row k factors as (jj^k) * hs^k and the row lanes only need the three hs-powers
// of their row (basis_k(k, hs)) once per pass instead of a power chain per sample.
__device__ __forceinline__ void fill_power_table(lds_dp pw, int lane) {
  for (int t = lane; t < 156; t += 64) {
    const int jj = t / 6, k = t - 6 * jj;
    double v = 1.0;
    for (int u = 0; u < k; u++) v *= (double)jj;
    pw[t] = v;
  }
}

// Phase stamps for the diagnostic build (-DTOPAY_STAMPS): never compiled into the product library.
#ifdef TOPAY_STAMPS
#define STAMP(C, k)                                                    \
  do {                                                                 \
    const long long now_ = (long long)__builtin_amdgcn_s_memtime();    \
    if ((C).stamps && (C).lane == 0) (C).stamps[k] += now_ - (C).t_last; \
    (C).t_last = (long long)__builtin_amdgcn_s_memtime();              \
  } while (0)
#else
#define STAMP(C, k) do { } while (0)
#endif
// sub-interval stamp that does not reset the phase clock
#ifdef TOPAY_STAMPS
#define SUBSTAMP_BEGIN(C) const long long sub_t0_ = (long long)__builtin_amdgcn_s_memtime()
#define SUBSTAMP_END(C, k)                                                                                   \
  do {                                                                                                       \
    if ((C).stamps && (C).lane == 0) (C).stamps[k] += (long long)__builtin_amdgcn_s_memtime() - sub_t0_;      \
  } while (0)
#else
#define SUBSTAMP_BEGIN(C) do { } while (0)
#define SUBSTAMP_END(C, k) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// The LDS plan of an evaluation, stated once: eval_lds_plan() walks the blocks and sets the LDS fields of what it is
// given -- an EvalCtx, from the workgroup's LDS base (eval_lds_carve), or their offsets from 0 for the size (eval_lds_total).
//   Tp [5 Nmax] | gdT [Nmax] | pcs [4 (Nmax + 1)] | pw [156] | red [eval_misc_doubles] | cL [9 rows] | X [eval_borrow_doubles]
// cL and X together are the union region (eval_union_doubles): the band and its reciprocal diagonal (14 rows) while the
// system is factorised; afterwards the coefficients (then the adjoint's right-hand sides / solution) in cL and, in X, the
// positional gradients (26 Nmax) and one pass buffer per wave.  X is also what the substitutions' two windows (band_sweep)
// and, between two evaluations, the solver's alpha ring borrow: both fit at any Nmax because a pass buffer alone is at
// least 448 doubles (static_asserts in topay_minco.h and topay_solve.h).
// LDS is what decides how many trajectories share a compute unit, so the adjoint solve runs in the coefficients' block
// (a block of its own cost the bench 5.7 %, docs/EXPERIMENTS.md) and one wave holds nothing it can do without: a pass
// buffer of 7 rows (a pass's gradient rows reach the row lanes in two halves), no reduction scratch, no cost exchange.
// With np = ceil(13 Nmax / 64) passes, for every class there is (one wave: Nmax <= 112) the total in doubles is
//   one wave 90 Nmax + 609 + 2 np,   two waves 90 Nmax + 2218 + 2 np,   four waves 90 Nmax + 4268 + 2 np:
// 11.8 / 15.4 / 19.6 / 27.4 KB at Nmax = 10 / 15 / 21 / 32 on one wave, 63.0 / 78.5 / 153.4 KB at 42 / 64 / 170 on four.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr int eval_pb_rows(int NW) { return NW == 1 ? 7 : 14; }   // rows of a wave's pass buffer
__host__ __device__ constexpr int eval_npass(int Nmax) { return (TOPAY_EP * Nmax + 63) / 64; }
__host__ __device__ constexpr int eval_red_doubles(int NW) { return NW > 1 ? 8 : 0; }
// [8] partial sums of a workgroup reduction (two phases; NW > 1) | [2 npass] pass totals | [2][NW][64] per-round costs
// (NW > 1) | [NW] masks
__host__ __device__ constexpr int eval_misc_doubles(int Nmax, int NW) {
  return eval_red_doubles(NW) + 2 * eval_npass(Nmax) + (NW > 1 ? 2 * NW * 64 : 0) + NW;
}
// the union region: the band + reciprocal diagonal | the coefficients, the positional gradients and the pass buffers
// (spelled as one maximum on purpose: with the coefficients' 9 rows factored out of it, this compiler gives the solve
// kernels other code)
__host__ __device__ constexpr int eval_union_doubles(int Nmax, int NW) {
  const int rows = 6 * Nmax;
  const int lu = 14 * rows, sw = 9 * rows + 26 * Nmax + eval_pb_rows(NW) * 64 * NW;
  return lu > sw ? lu : sw;
}
// what of it lies behind the coefficients (EvalCtx::X)
__host__ __device__ constexpr int eval_borrow_doubles(int Nmax, int NW) { return eval_union_doubles(Nmax, NW) - 9 * 6 * Nmax; }
template <typename P>
struct EvalLds {   // the LDS fields of EvalCtx, as offsets
  P Tp, gdT, pcs, pw, red, cL, adj, gC, X;
};
// L = EvalCtx (P = lds_dp) or EvalLds<int>; returns the end of the plan
template <typename L, typename P>
__host__ __device__ constexpr P eval_lds_plan(L& C, P base, int Nmax, int NW) {
  const int rows = 6 * Nmax;
  P p = base;
  C.Tp = p; p += 5 * Nmax;
  C.gdT = p; p += Nmax;
  C.pcs = p; p += 4 * (Nmax + 1);
  C.pw = p; p += 156;
  C.red = p; p += eval_misc_doubles(Nmax, NW);
  C.cL = p;                // (the band of the factorisation starts here too)
  C.adj = C.cL;
  C.gC = C.adj;
  C.X = p + 9 * rows;
  return p + eval_union_doubles(Nmax, NW);
}
__host__ __device__ constexpr int eval_lds_total(int Nmax, int NW) {
  EvalLds<int> offsets{};
  return eval_lds_plan(offsets, 0, Nmax, NW);
}
__device__ __forceinline__ void eval_lds_carve(EvalCtx& C, lds_dp base, int Nmax, int NW) {
  eval_lds_plan(C, base, Nmax, NW);
  C.npass_lds = eval_npass(Nmax);
}
// The plan pinned at the limits of the launch classes (kClassTable: one wave to 10 / 15 / 21 / 32 pieces, four waves to
// 42 / 64 / 170; the helper-wave kernels of the one-wave classes: four waves) and of the kernels of topay_eval_waves.
static_assert(eval_lds_total(10, 1) == 1515 && eval_lds_total(15, 1) == 1967 && eval_lds_total(21, 1) == 2509 &&
              eval_lds_total(32, 1) == 3503 && eval_lds_total(42, 1) == 4407 && eval_lds_total(64, 1) == 6395, "LDS plan, one wave");
static_assert(eval_lds_total(42, 2) == 6016 && eval_lds_total(64, 2) == 8004, "LDS plan, two waves");
static_assert(eval_lds_total(10, 4) == 5174 && eval_lds_total(15, 4) == 5626 && eval_lds_total(21, 4) == 6168 &&
              eval_lds_total(32, 4) == 7162 && eval_lds_total(42, 4) == 8066 && eval_lds_total(64, 4) == 10054 &&
              eval_lds_total(85, 4) == 11954 && eval_lds_total(128, 4) == 15840 && eval_lds_total(TOPAY_MAX_N, 4) == 19638,
              "LDS plan, four waves");

}  // namespace topay
