// The hand-offs of a planning call (topay_plan_calls == Planner::planMomaParallel, planner.cpp:792-1061): the small kernels
// that carry the result of one stage into the inputs of the next without a trip through the host, the choice of a call's
// winner (planner.cpp:999-1010) and the gather of the winners into the context's store.  The stages themselves are the
// kernels of the single entry points (k_topo, k_jps, k_dense_path, k_mcrrt, k_init, the solve classes, the gate).
//   k_plan_candidates    roadmap paths + JPS path of every call -> candidate table, raw paths laid out for k_dense_path
//   k_plan_pack_search   dense paths + the calls' start / end states -> inputs of k_mcrrt (one instance per candidate)
//   k_plan_pack_solver   whole-body paths (strided by layer cap) -> the solver's ragged init paths and boundary block
//   k_plan_winner        per call: stage of each of its at most 8 candidates, the first strictly shortest one that counts
//   k_plan_gather_front  the winners' whole-body init paths -> store
//   k_plan_store_gather  store -> the packed layout of topay_get_results for a selection of calls
// Plain loads, stores and IEEE double additions in the order of the host code they stand for; nothing here is contracted.
#pragma once
#include "topay_types.h"

namespace topay {

struct PlanCandArgs {
  int n;                      // calls of this launch
  int cap_paths, cap_points;  // layout of the roadmap's result: path (p, k) starts at point (p cap_paths + k) cap_points
  int jps_cap;                // points per JPS path; path p starts at point jps_base + p jps_cap
  int max_cand;
  long long jps_base;
  const int* topo_np;         // [n]
  const int* topo_len;        // [n][cap_paths]
  const int* jps_len;         // [n], or null (the second try has no JPS candidate)
  const double* start;        // [n][10]
  const double* end;          // [n][10]
  // out
  int* ncand;                 // [n]  candidates of the call; negated when more than max_cand ("Too many paths to optimize"): none is laid out
  long long* raw_off;         // [n][8]  first point of candidate k's raw path
  int* raw_len;               // [n][8]  its points, 0: no such candidate
  double* syaw;               // [n][8]
  double* eyaw;               // [n][8]
};

// One thread per call.
__global__ void k_plan_candidates(const PlanCandArgs A) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.n) return;
  int np = A.topo_np[p];
  np = np < 0 ? 0 : (np > A.cap_paths ? A.cap_paths : np);
  int jl = A.jps_len ? A.jps_len[p] : 0;
  jl = jl < 0 ? 0 : jl;
  int nc = np + (jl > 0 ? 1 : 0);
  // A JPS path of more than jps_cap points was counted by k_jps, not written: it stays a candidate of the call and fails
  // (no raw points -> no dense path -> the search reports status -2) instead of going on as a path cut short of the goal.
  if (jl > A.jps_cap) jl = 0;
  const bool too_many = nc > A.max_cand;
  A.ncand[p] = too_many ? -nc : nc;
  if (too_many) nc = 0;
  const double sy = A.start[10 * (size_t)p + 2], ey = A.end[10 * (size_t)p + 2];
  for (int k = 0; k < TOPAY_PLAN_MAX_CAND; k++) {
    const size_t s = (size_t)p * TOPAY_PLAN_MAX_CAND + k;
    long long off = 0;
    int len = 0;
    if (k < nc) {
      if (k < np) {
        off = ((long long)p * A.cap_paths + k) * A.cap_points;
        len = A.topo_len[(size_t)p * A.cap_paths + k];
        len = len < 0 ? 0 : (len > A.cap_points ? A.cap_points : len);
      } else {
        off = A.jps_base + (long long)p * A.jps_cap;
        len = jl;
      }
    }
    A.raw_off[s] = off;
    A.raw_len[s] = len;
    A.syaw[s] = sy;
    A.eyaw[s] = ey;
  }
}

// One thread per search instance i = candidate slot sel[i] (= call * 8 + k) of the launch's calls.  The chassis paths stay
// where k_dense_path wrote them: the search reads instance i's at car + 4 car_off[i].
__global__ void k_plan_pack_search(int n_inst, const int* sel, int dense_cap, const int* dense_len, const double* start, const double* end,
                                   const int* call_map, const unsigned long long* call_no, int try_no, long long* car_off, int* car_len,
                                   double* st_out, double* en_out, int* map_id, unsigned long long* inst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inst) return;
  const int s = sel[i], p = s / TOPAY_PLAN_MAX_CAND, k = s - p * TOPAY_PLAN_MAX_CAND;
  car_off[i] = (long long)s * dense_cap;
  const int L = dense_len[s];
  car_len[i] = L > dense_cap ? dense_cap : L;   // (more than 255 layers: the search reports status -2)
  for (int a = 0; a < 10; a++) {
    st_out[10 * (size_t)i + a] = start[10 * (size_t)p + a];
    en_out[10 * (size_t)i + a] = end[10 * (size_t)p + a];
  }
  map_id[i] = call_map[p];
  inst[i] = 16ull * call_no[p] + 8ull * (unsigned long long)try_no + (unsigned long long)k;
}

// One workgroup per surviving candidate j of the launch: its whole-body path (instance src[j], wb_len[src[j]] states) to
// states [path_off[j], ...) of the ragged init paths; column 0 of its 10 x 2 boundary velocity = the call's start_v.
__global__ void k_plan_pack_solver(int n, const int* src, const int* src_call, int layer_cap, const int* wb_len, const double* wb,
                                   const long long* path_off, const double* start_v, int b0, double* paths, double* bvel) {
  const int j = blockIdx.x;
  if (j >= n) return;
  const int i = src[j], L = wb_len[i];
  const double* from = wb + (size_t)i * layer_cap * 10;
  double* to = paths + 10 * path_off[j];
  for (int t = threadIdx.x; t < 10 * L; t += blockDim.x) to[t] = from[t];
  double* bv = bvel + 20 * ((size_t)b0 + j);
  for (int t = threadIdx.x; t < 20; t += blockDim.x) bv[t] = t < 10 ? (start_v ? start_v[10 * (size_t)src_call[j] + t] : 0.0) : 0.0;
}

// Stage of a solved candidate (TOPAY_PLAN_STAGE_* of include/topay.h, where TOPAY_PLAN_MAX_CAND is stated too): 2 needs more
// pieces than the build solves, 3 solver failed, 4 gate failed, 5 interrupted, 6 counts (optimizeTraj true AND
// printConstraintsSituations passed, planner.cpp:878-880).

// One lane per call q of the solved batch: its candidates are the batch members [first[q], first[q] + count[q]), in
// candidate order.  The winner is the first whose total duration is strictly the smallest (planner.cpp:999-1010); the
// duration is the sum of the pieces' in piece order, as topay_get_total_durations forms it.
__global__ void k_plan_winner(DevBatch Bt, int n_calls, const int* first, const int* count, int* stage, int* win, double* win_cost_dur) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_calls) return;
  int best = -1;
  double best_dur = 0.0;
  for (int b = first[q]; b < first[q] + count[q]; b++) {
    const int N = Bt.N[b];
    int st;
    double dur = 0.0;
    if (N <= 0) st = TOPAY_PLAN_STAGE_TOO_MANY_PIECES;
    else {
      for (int i = 0; i < N; i++) dur += Bt.T_of(Bt.poff[b])[i];
      if (Bt.interrupted[b]) st = TOPAY_PLAN_STAGE_INTERRUPTED;
      else if (!Bt.success[b]) st = TOPAY_PLAN_STAGE_SOLVER_FAILED;
      else if (!Bt.flags_of(b)[0]) st = TOPAY_PLAN_STAGE_GATE_FAILED;
      else st = TOPAY_PLAN_STAGE_COUNTS;
    }
    stage[b] = st;
    if (st == TOPAY_PLAN_STAGE_COUNTS && (best < 0 || dur < best_dur)) { best = b; best_dur = dur; }
  }
  win[q] = best;
  win_cost_dur[2 * (size_t)q] = best < 0 ? 0.0 / 0.0 : Bt.cost[best];
  win_cost_dur[2 * (size_t)q + 1] = best < 0 ? 0.0 / 0.0 : best_dur;
}

// One workgroup per winner w: its init path (batch member idx[w]) to states [front_off[w], front_off[w + 1]) of the store.
__global__ void k_plan_gather_front(int n, const int* idx, const double* paths, const long long* path_off, const int* front_off, double* out) {
  const int w = blockIdx.x;
  if (w >= n) return;
  const int L = front_off[w + 1] - front_off[w];
  const double* from = paths + 10 * path_off[idx[w]];
  double* to = out + 10 * (size_t)front_off[w];
  for (int t = threadIdx.x; t < 10 * L; t += blockDim.x) to[t] = from[t];
}

// One workgroup per selected call k: N = piece_off[k + 1] - piece_off[k] pieces from piece src_piece[k] / knot src_knot[k] of
// the store to the packed layout of topay_get_results (knots of selection k at 2 (piece_off[k] + k)).
__global__ void k_plan_store_gather(int n, const int* src_piece, const int* src_knot, const int* piece_off, const double* s_dur, const double* s_coef,
                                    const double* s_kn, double* durations, double* coeffs, double* knots) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const int N = piece_off[k + 1] - piece_off[k];
  if (N <= 0) return;
  const int p0 = piece_off[k], sp = src_piece[k], sk = src_knot[k];
  for (int t = threadIdx.x; t < N * kCoefPerPiece; t += blockDim.x) coeffs[(size_t)p0 * kCoefPerPiece + t] = s_coef[(size_t)sp * kCoefPerPiece + t];
  for (int t = threadIdx.x; t < N; t += blockDim.x) durations[p0 + t] = s_dur[sp + t];
  for (int t = threadIdx.x; t < 2 * (N + 1); t += blockDim.x) knots[2 * (size_t)(p0 + k) + t] = s_kn[2 * (size_t)sk + t];
}

}  // namespace topay
