// Wave and workgroup primitives of the kernels: the fixed-order reductions and scans over the 64 lanes of a wave, the
// hand-offs between lanes through LDS and through global memory, wave-uniform values forced into scalar registers, the
// barriers and reductions of a workgroup of NW = 1, 2 or 4 waves -- and the few empty asm statements and attributes by
// which the kernels steer this compiler's register allocation.  Nothing here knows about trajectories.
#pragma once

#include <hip/hip_runtime.h>

#include "topay_types.h"

// The compiler must treat the value as changed (no instruction is emitted): stops common-subexpression reuse across a
// rarely taken path, which would otherwise be paid for with registers on the common one.
#ifndef TOPAY_CPU_EMU
#define TOPAY_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define TOPAY_OPAQUE(x) do { } while (0)
#endif

// On the functions that call the non-inlined device functions.  Those callees use the whole register file, and the
// compiler lets such a function skip the saving of callee-saved registers (the caller then saves exactly what it keeps across
// the call) only if no call of it carries LLVM's `tail` marker -- which the optimiser adds to every call that is handed no
// pointer into the caller's stack frame.  Round 5 took the stack out of the manipulator block's interface, the marker
// appeared, and the block began to save and restore all 112 callee-saved VGPRs on every call (388 scratch instructions).
// With this attribute the marker is not added.
#ifndef TOPAY_CPU_EMU
#define TOPAY_CALLS_BIG_FUNCTIONS __attribute__((disable_tail_calls))
#else
#define TOPAY_CALLS_BIG_FUNCTIONS
#endif

// A wave-uniform `true` the compiler cannot see through (one s_cmp + s_cbranch): starts a new basic block on purpose.
__device__ __forceinline__ bool topay_opaque_true() {
#ifndef TOPAY_CPU_EMU
  int one = 1;
  asm volatile("" : "+s"(one));
  return one != 0;
#else
  return true;
#endif
}

namespace topay {

// ---------------------------------------------------------------------------------------------
// wave helpers (collectives: call only from wave-uniform control flow)
// ---------------------------------------------------------------------------------------------
// One fixed summation tree for every wave reduction: xor-butterfly with offsets 1,2,4,8 inside each 16-lane row
// (DPP quad_perm / row_half_mirror / row_mirror; additions commute, so all lanes of a row end up with identical
// bits), then (r0+r1)+(r2+r3) over the four rows via readlane.  Every lane receives the same bits, which keeps
// wave-uniform control flow uniform.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
#ifndef TOPAY_CPU_EMU
  // (mov_dpp: no "old" operand -- with update_dpp(lo, lo, ...) the compiler copies the source into the destination first,
  // two more 32-bit moves per level of every reduction: 8 of the 39 vector instructions per history pair of the two-loop recursion)
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, false);
#else
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
#endif
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
// rows of 16 lanes outside ROWMASK receive 0.0 (the caller adds the result)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64_rows(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROWMASK, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROWMASK, 0xF, false);
  return __hiloint2double(hi, lo);
}
// 64-lane sum: a butterfly inside every row of 16 (every lane of row k then holds r_k), then across the rows:
// (r0 + r1) + (r2 + r3), in lane 63.  The sum is 20 instructions of VALU issue -- f64 has no DPP operand form, every
// level is two 32-bit DPP moves and an add -- and that, not the latency of the chain, is what a reduction costs
// (docs/EXPERIMENTS.md); the cross-row levels replace four lane reads and three adds of rounds 1-2, same bits (the
// operands of every addition are the same, in the other order).
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]   : lane ^ 1
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]   : lane ^ 2
  v += dpp_f64<0x141>(v);  // row_half_mirror       : quad q <-> quad q^1
  v += dpp_f64<0x140>(v);  // row_mirror            : half h <-> half h^1
#ifndef TOPAY_CPU_EMU
  // Only lane 63 is read below: the rows a broadcast does not reach may hold anything, so the moves need no zeroed
  // destination (two more 32-bit moves per level with the row masks of the emulator's form; lane 63's operands are the same).
  v += dpp_f64<0x142>(v);             // row_bcast15: row k += lane 15 of row k - 1               -> lane 63: r3 + r2, lane 31: r1 + r0
  v += dpp_f64<0x143>(v);             // row_bcast31: rows 2, 3 += lane 31                        -> lane 63: (r3 + r2) + (r1 + r0)
#else
  v += dpp_f64_rows<0x142, 0xA>(v);   // row_bcast15: rows 1 and 3 += lane 15 of the row before  -> r1 + r0, r3 + r2
  v += dpp_f64_rows<0x143, 0xC>(v);   // row_bcast31: rows 2 and 3 += lane 31                    -> (r3 + r2) + (r1 + r0)
#endif
  return readlane_f64(v, 63);
}
__device__ __forceinline__ double wave_max(double v) {
  double o;
  o = dpp_f64<0xB1>(v); v = o > v ? o : v;
  o = dpp_f64<0x4E>(v); v = o > v ? o : v;
  o = dpp_f64<0x141>(v); v = o > v ? o : v;
  o = dpp_f64<0x140>(v); v = o > v ? o : v;
  const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
  const double a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
  return a > b ? a : b;
}
// LDS hand-off between lanes of the one wave of this workgroup: LDS operations of a wave complete in issue
// order, so only compiler reordering has to be prevented (no s_barrier, no vmcnt drain).
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}
// Hand-off through GLOBAL memory between the lanes of one wave (stores by some lanes, loads by others): the stores are
// complete (vmcnt) before any lane goes on, without a workgroup barrier -- usable by one wave of a several-waves workgroup.
__device__ __forceinline__ void wave_global_sync() {
#ifndef TOPAY_CPU_EMU
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#else
  __builtin_amdgcn_wave_barrier();
#endif
}
// The lane's number formed anew (two instructions, no operand): used after a call of the manipulator block, so that the
// number -- and everything derived from it -- need not be carried across the call in a register the callee clobbers.
__device__ __forceinline__ int fresh_lane_id(int known) {
#ifndef TOPAY_CPU_EMU
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  (void)known;
  return l;
#else
  return known;
#endif
}
// inclusive prefix sum over lanes
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    double o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}
// inclusive suffix sum over lanes
__device__ __forceinline__ double wave_incl_rscan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    double o = __shfl_down(v, off);
    if (lane + off < 64) v += o;
  }
  return v;
}

// A wave-uniform double forced into scalar registers.
__device__ __forceinline__ double uniform_f64(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
// Wave-uniform pointers forced into scalar registers: a value the compiler cannot prove uniform (loaded from the context
// block in private memory) lives in a vector register, and everything in vector registers that is live across the call of
// the manipulator block is saved to and restored from scratch memory around it, once per sample pass.
#ifndef TOPAY_CPU_EMU
template <typename T>
__device__ __forceinline__ TOPAY_GLB T* uniform_ptr(TOPAY_GLB T* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffu)), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (TOPAY_GLB T*)(((unsigned long long)hi << 32) | lo);
}
template <typename T>
__device__ __forceinline__ TOPAY_LDS T* uniform_ptr(TOPAY_LDS T* p) {
  return (TOPAY_LDS T*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)p);
}
#else
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) { return p; }
#endif

// Workgroup barrier that orders LDS traffic only: outstanding global loads / stores (the prefetch ring of the two-loop
// recursion, the parked gradient rows) are not drained.  Cross-wave hand-offs through global memory use __syncthreads().
__device__ __forceinline__ void wg_lds_barrier() {
#ifndef TOPAY_CPU_EMU
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#else
  __syncthreads();
#endif
}

// (one wave: the wave-level hand-off, no s_barrier)
template <int NW>
__device__ __forceinline__ void wg_barrier() {
  if (NW == 1) lds_sync();
  else wg_lds_barrier();
}

// Hand-off through GLOBAL memory (stores by some threads, loads by others).  One wave: the memory instructions of a wave are
// performed in issue order, lanes or no lanes, so only the compiler has to be kept from reordering -- no wait for the stores to
// come back (a round trip to L2 / HBM each time: the LU stash, the coefficients' move to the result block and the gradient at
// the end of every evaluation).  Several waves: the full barrier.
template <int NW>
__device__ __forceinline__ void wg_global_barrier() {
  if (NW == 1) lds_sync();
  else __syncthreads();
}

// Sum over the workgroup in a fixed order: wave tree (wave_sum), then (w0 + w1) + (w2 + w3).  `red` holds two sets of
// four partial sums used alternately, so one barrier per reduction suffices (a wave can only write a set again after
// every wave has passed the barrier that follows the reads of its previous use); `phase` is a workgroup-uniform local
// counter, and the caller separates reductions that do not share one by a barrier.
template <int NW>
__device__ __forceinline__ double wg_combine(lds_dp red, int& phase, int wave, double wsum) {
  static_assert(NW == 1 || NW == 2 || NW == 4, "waves per trajectory");
  if (NW == 1) return wsum;
  lds_dp r = red + (phase & 1) * 4;
  phase++;
  r[wave] = wsum;
  wg_lds_barrier();
  if (NW == 2) return r[0] + r[1];
  return (r[0] + r[1]) + (r[2] + r[3]);
}
template <int NW>
__device__ __forceinline__ double wg_sum(lds_dp red, int& phase, int wave, double v) {
  return wg_combine<NW>(red, phase, wave, wave_sum(v));
}
template <int NW>
__device__ __forceinline__ double wg_max(lds_dp red, int& phase, int wave, double v) {
  const double wm = wave_max(v);
  if (NW == 1) return wm;
  lds_dp r = red + (phase & 1) * 4;
  phase++;
  r[wave] = wm;
  wg_lds_barrier();
  double m = r[0] > r[1] ? r[0] : r[1];
  if (NW == 4) {
    const double m2 = r[2] > r[3] ? r[2] : r[3];
    m = m > m2 ? m : m2;
  }
  return m;
}

}  // namespace topay
