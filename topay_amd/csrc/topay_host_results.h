// Host side of the C-ABI, part 4: getters, playback and mesh poses, the evaluation hooks, the feasibility gate, counters.

#pragma once

// Kernel for a forced number of waves per trajectory (test hook topay_eval_waves): the smallest template that holds N.
static bool class_for_waves(int N, int nw, ClassDef& out) {
  static const ClassDef w1[] = {{10, 1, 1, nullptr, k_eval1, 2}, {21, 2, 1, nullptr, k_eval2, 2}, {32, 3, 1, nullptr, k_eval3, 2},
                                {42, 4, 1, nullptr, k_eval4, 2}, {64, 6, 1, nullptr, k_eval6, 2}};
  static const ClassDef w2[] = {{42, 2, 2, nullptr, k_eval2w2, 2}, {64, 3, 2, nullptr, k_eval3w2, 2}};
  static const ClassDef w4[] = {{85, 2, 4, nullptr, k_eval2w4, 2}, {128, 3, 4, nullptr, k_eval3w4, 2}, {TOPAY_MAX_N, 4, 4, nullptr, k_eval4w4, 2}};
  const ClassDef* t = nw == 1 ? w1 : (nw == 2 ? w2 : (nw == 4 ? w4 : nullptr));
  const int cnt = nw == 1 ? 5 : (nw == 4 ? 3 : 2);
  if (!t) return false;
  for (int k = 0; k < cnt; k++)
    if (N <= t[k].max_n) { out = t[k]; return true; }
  return false;
}

static topay_status eval_one(topay_ctx* c, int stage, int i, const double* x, const double* alm_lambda, const double* alm_rho,
                             double* f, double* g, double* final_xy_error, bool commit, int force_nw = 0) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B || (stage != 1 && stage != 2) || !x) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  const int N = c->hN[i], nn = 10 * N - 8;
  if (N == 0) return TOPAY_ERR_TOO_MANY_PIECES;
  HIPCHK(h2d_sync(c, c->db.x_of(c->h_noff[i]), x, (size_t)nn));
  double alm[kAlmLen] = {alm_lambda ? alm_lambda[0] : c->hp.alm_init_lambda[0], alm_lambda ? alm_lambda[1] : c->hp.alm_init_lambda[1],
                   alm_rho ? alm_rho[0] : c->hp.alm_init_rho[0], alm_rho ? alm_rho[1] : c->hp.alm_init_rho[1]};
  HIPCHK(h2d_sync(c, c->db.alm_of(i), alm, kAlmLen));
  // single-block launch through a one-entry order array placed at the end of the order buffer
  DevBuf tmp;
  topay_status s = tmp.ensure(4);
  if (s != TOPAY_OK) return s;
  HIPCHK(h2d_sync(c, tmp.as<int>(), &i, 1));
  DevBatch d = c->db;
  d.order = tmp.as<int>();
  ClassDef cd = kClassTable[bucket_of(N)];   // the class (kernel, waves per trajectory) that also solves this candidate
  if (force_nw > 0 && !class_for_waves(N, force_nw, cd)) { set_err("no kernel with that many waves holds this candidate"); return TOPAY_ERR_UNSUPPORTED; }
  const size_t lds = class_lds_bytes(cd, N);
  if ((s = push_params(c)) != TOPAY_OK) return s;
  HIPCHK(set_kernel_attributes(c->device));
  if (force_nw > 0) HIPCHK(hipFuncSetAttribute((const void*)cd.eval, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsDoublesPerCU * 8));
  hipLaunchKernelGGL(cd.eval, dim3(1), dim3(64 * cd.nw), lds, c->stream, d, (const DevMap*)c->dmaps.p, stage | (commit ? 16 : 0), 1, N);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  if (f) HIPCHK(d2h_sync(c, f, c->fout.as<double>() + i, 1));
  if (g) HIPCHK(d2h_sync(c, g, c->db.work_of(c->h_noff[i]), (size_t)nn));
  if (final_xy_error) HIPCHK(d2h_sync(c, final_xy_error, c->db.xyerr_of(i), 2));
  return TOPAY_OK;
}

extern "C" {

topay_status topay_get_nmax(topay_ctx* c, int* nmax, int* Nmax) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (nmax) *nmax = 10 * c->Nmax - 8;
  if (Nmax) *Nmax = c->Nmax;
  return TOPAY_OK;
}

topay_status topay_get_batch(topay_ctx* c, int* success, double* cost, int* n_pieces) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  if (success) HIPCHK(d2h_sync(c, success, c->success.as<int>(), (size_t)c->B));
  if (cost) HIPCHK(d2h_sync(c, cost, c->cost.as<double>(), (size_t)c->B));
  if (n_pieces) memcpy(n_pieces, c->hN.data(), (size_t)c->B * 4);
  return TOPAY_OK;
}

topay_status topay_get_elapsed_us(topay_ctx* c, double* us, double* start_us, int* hw_id) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  if (us) HIPCHK(d2h_sync(c, us, c->elapsed.as<double>(), (size_t)c->B));
  if (start_us) HIPCHK(d2h_sync(c, start_us, c->startus.as<double>(), (size_t)c->B));
  if (hw_id) HIPCHK(d2h_sync(c, hw_id, c->hwid.as<int>(), (size_t)c->B));
  return TOPAY_OK;
}

// MomaTraj playback of candidate i: car_seq (x, y, theta, t every 0.1 s; moma_traj_opt.h:40-69) and getState at the
// given times (113-137).  seq may be NULL; *n_seq receives the number of entries (capacity seq_cap rows of 4).
topay_status topay_playback(topay_ctx* c, int i, int n_times, const double* times, double* states, int seq_cap, double* seq,
                            int* n_seq) {
  if (!c || !c->have_traj || !c->solved) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B || n_times < 0 || (n_times > 0 && (!times || !states))) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> hT((size_t)std::max(1, c->hN[i]));
  if (c->hN[i] > 0) HIPCHK(d2h_sync(c, hT.data(), c->db.T_of(c->h_poff[i]), (size_t)c->hN[i]));
  double t = 0.0;
  for (int k = 0; k < c->hN[i]; k++) t += hT[k];
  if (!(t > 0.0 && t < 1.0e4)) t = 0.0;
  const long long cap_panels = (long long)(t / 0.025) + 4;
  const long long nseq_max = cap_panels / 4 + 2;
  topay_status s;
  if ((s = c->feas_cseq.ensure((size_t)2 * (cap_panels + 1) * 8)) != TOPAY_OK) return s;
  double *d_times, *d_states, *d_seq; int* d_nseq;
  auto lay = [&](Carver& k) {
    d_times = k.take<double>((size_t)n_times); d_states = k.take<double>((size_t)n_times * 10); d_seq = k.take<double>((size_t)nseq_max * 4);
    d_nseq = k.take<int>(1);
  };
  if ((s = c->pb_io.carve(lay)) != TOPAY_OK) return s;
  if (n_times) HIPCHK(h2d(c, d_times, times, (size_t)n_times));
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  hipLaunchKernelGGL(k_playback, dim3(1), dim3(64), 0, c->stream, c->db, i, c->feas_cseq.as<double>(), cap_panels, n_times,
                     (const double*)d_times, d_states, d_seq, d_nseq);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  int ns = 0;
  HIPCHK(d2h_sync(c, &ns, d_nseq, 1));
  if (n_seq) *n_seq = ns;
  if (seq && ns > 0) HIPCHK(d2h_sync(c, seq, d_seq, (size_t)std::min(ns, seq_cap) * 4));
  if (n_times) HIPCHK(d2h_sync(c, states, d_states, (size_t)n_times * 10));
  return TOPAY_OK;
}

topay_status topay_default_mesh_params(topay_mesh_params_t* p) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  const double ll[7] = {0.2405, 0.0, 0.256, 0.0, 0.21, 0.0, 0.144};              // moma_param.h:114
  const double lo[7] = {-3.1, -2.26, -3.1, -2.355, -3.1, -2.23, -6.28};          // moma_param.h:115
  for (int i = 0; i < 7; i++) {
    p->link_length[i] = ll[i];
    p->joint_pos_limit_min[i] = lo[i];
    for (int k = 0; k < 3; k++) { p->joint_offset[3 * i + k] = 0.0; p->joint_dof_axis[3 * i + k] = 0.0; }
    if (i < 6) {                                                                  // moma_param.h:77-90
      p->joint_offset[3 * i] = (i % 2 == 0) ? -1.5708 : 1.5708;
      p->joint_dof_axis[3 * i + 1] = (i % 2 == 0) ? -1.0 : 1.0;
    } else {
      p->joint_dof_axis[3 * i + 2] = 1.0;
    }
  }
  return TOPAY_OK;
}

topay_status topay_mesh_poses(topay_ctx* c, const topay_mesh_params_t* mesh, int n, const double* states, double* parts) {
  if (!c || !mesh || n < 0 || (n > 0 && (!states || !parts))) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  topay_status s;
  double *d_st, *d_parts;
  if ((s = c->pb_io.carve([&](Carver& k) { d_st = k.take<double>((size_t)n * 10); d_parts = k.take<double>((size_t)n * 77); })) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_st, states, (size_t)n * 10));
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  hipLaunchKernelGGL(k_mesh_pose, dim3((n + 63) / 64), dim3(64), 0, c->stream, *mesh, n, (const double*)d_st, d_parts);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, parts, d_parts, (size_t)n * 77));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

// Planner::toMeshMsg (planner.cpp:2003-2056).  The sample times and the arc length are running sums over the samples
// (host, in the reference's order); getState and getMeshPose of all samples run on the device.
topay_status topay_mesh_traj(topay_ctx* c, int i, const topay_mesh_params_t* mesh, int res, int cap_states, double* parts,
                             double* yaws, double* arc_lengths, int* n_states) {
  if (!c || !c->have_traj || !c->solved) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B || !mesh || res <= 0 || cap_states < res + 1 || !parts || !yaws || !arc_lengths || !n_states) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> hT((size_t)std::max(1, c->hN[i]));
  if (c->hN[i] > 0) HIPCHK(d2h_sync(c, hT.data(), c->db.T_of(c->h_poff[i]), (size_t)c->hN[i]));
  double T = 0.0;
  for (int k = 0; k < c->hN[i]; k++) T += hT[k];
  if (!(T > 0.0 && T < 1.0e4)) { *n_states = 0; return TOPAY_OK; }
  const double intvl = T / res;
  std::vector<double> times;
  for (double t = 0.0; t < T && (int)times.size() < cap_states; t += intvl) times.push_back(t);
  const int n = (int)times.size();
  std::vector<double> st((size_t)(n + 1) * 10);
  times.push_back(0.0);                       // prev_state of the first sample = getState(0)
  topay_status s = topay_playback(c, i, n + 1, times.data(), st.data(), 0, nullptr, nullptr);
  if (s != TOPAY_OK) return s;
  if ((s = topay_mesh_poses(c, mesh, n, st.data(), parts)) != TOPAY_OK) return s;
  double acc = 0.0;
  const double* prev = &st[(size_t)n * 10];
  for (int k = 0; k < n; k++) {
    const double* cur = &st[(size_t)k * 10];
    const double dx = cur[0] - prev[0], dy = cur[1] - prev[1];
    acc += std::sqrt(dx * dx + dy * dy);
    arc_lengths[k] = acc;
    yaws[k] = cur[2];
    prev = cur;
  }
  *n_states = n;
  return TOPAY_OK;
}

topay_status topay_get_total_durations(topay_ctx* c, double* total) {
  if (!c || !c->have_traj || !total) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> hT((size_t)c->h_poff[c->B] + 1);
  HIPCHK(d2h_sync(c, hT.data(), c->T.as<double>(), (size_t)c->h_poff[c->B]));
  for (int b = 0; b < c->B; b++) {
    double t = 0.0;
    for (int i = 0; i < c->hN[b]; i++) t += hT[(size_t)c->h_poff[b] + i];  // PolyTrajectory::getTotalDuration, minco.hpp:304-313
    total[b] = c->hN[b] > 0 ? t : 0.0 / 0.0;
  }
  return TOPAY_OK;
}

topay_status topay_get_alm(topay_ctx* c, double* alm) {
  if (!c || !c->have_traj || !alm) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(d2h_sync(c, alm, c->alm.as<double>(), (size_t)c->B * kAlmLen));
  return TOPAY_OK;
}

topay_status topay_get_stats(topay_ctx* c, int* stats) {
  if (!c || !c->have_traj || !stats) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(d2h_sync(c, stats, c->stats.as<int>(), (size_t)c->B * kStatsLen));
  return TOPAY_OK;
}

topay_status topay_get_result(topay_ctx* c, int i, int* success, double* cost, int* n_pieces, double* durations,
                              double* coeffs, double* knots_xy) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const int N = c->hN[i], rows = 6 * N;
  if (N == 0) {  // not representable (more than TOPAY_MAX_N pieces): failed candidate, nothing else to report
    if (success) *success = 0;
    if (cost) *cost = 0.0 / 0.0;
    if (n_pieces) *n_pieces = 0;
    return TOPAY_OK;
  }
  if (success) HIPCHK(d2h_sync(c, success, c->success.as<int>() + i, 1));
  if (cost) HIPCHK(d2h_sync(c, cost, c->cost.as<double>() + i, 1));
  if (n_pieces) *n_pieces = N;
  if (durations) HIPCHK(d2h_sync(c, durations, c->db.T_of(c->h_poff[i]), (size_t)N));
  if (coeffs) {
    std::vector<double> cm((size_t)9 * rows);
    HIPCHK(d2h_sync(c, cm.data(), c->db.coef_of(c->h_poff[i]), cm.size()));
    // getTraj(): per piece the 6x9 block transposed, highest order first — minco.hpp:908-921
    for (int p = 0; p < N; p++)
      for (int d = 0; d < 9; d++)
        for (int k = 0; k < 6; k++) coeffs[((size_t)p * 9 + d) * 6 + k] = cm[(size_t)d * rows + 6 * p + 5 - k];
  }
  if (knots_xy)
    HIPCHK(d2h_sync(c, knots_xy, c->db.knots_of(c->h_poff[i], i), (size_t)2 * (N + 1)));
  return TOPAY_OK;
}

topay_status topay_get_results(topay_ctx* c, int n, const int* idx, int cap_pieces, int* piece_off, double* durations,
                               double* coeffs, double* knots_xy) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (n < 0 || (n > 0 && (!idx || !piece_off))) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  if (!c->solved) { set_err("topay_get_results: the batch has not been optimised"); return TOPAY_ERR_NO_TRAJ; }
  std::vector<int> off((size_t)n + 1, 0);
  for (int k = 0; k < n; k++) {
    if (idx[k] < 0 || idx[k] >= c->B) return TOPAY_ERR_INVALID_ARG;
    off[k + 1] = off[k] + c->hN[idx[k]];
  }
  const int np = off[n];
  memcpy(piece_off, off.data(), ((size_t)n + 1) * sizeof(int));
  if (np > cap_pieces) { set_err("topay_get_results: cap_pieces too small for the selection"); return TOPAY_ERR_INVALID_ARG; }
  if (np == 0 || (!durations && !coeffs && !knots_xy)) return TOPAY_OK;
  // device staging: idx | piece_off | durations | coeffs | knots, one kernel, one copy back
  const size_t kn = (size_t)2 * (np + n), dbl = (size_t)np + (size_t)np * kCoefPerPiece + kn;
  int *d_idx, *d_off; double *d_dur, *d_coef, *d_kn;
  auto lay = [&](Carver& k) {
    d_idx = k.take<int>((size_t)n); d_off = k.take<int>((size_t)n + 1);
    d_dur = k.take<double>((size_t)np); d_coef = k.take<double>((size_t)np * kCoefPerPiece); d_kn = k.take<double>(kn);   // (contiguous: one copy back)
  };
  if (topay_status s = c->pb_io.carve(lay); s != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_idx, idx, (size_t)n));
  HIPCHK(h2d(c, d_off, off.data(), (size_t)n + 1));
  // a selected candidate that was never launched (zero pieces) still owns one knot pair of the packed output: zeros
  HIPCHK(hipMemsetAsync(d_kn, 0, kn * sizeof(double), c->stream));
  hipLaunchKernelGGL(k_gather_results, dim3(n), dim3(64), 0, c->stream, c->db, n, (const int*)d_idx, (const int*)d_off, d_dur,
                     d_coef, d_kn);
  HIPCHK(hipGetLastError());
  std::vector<double> host(dbl);
  HIPCHK(d2h_sync(c, host.data(), d_dur, dbl));
  if (durations) memcpy(durations, host.data(), (size_t)np * 8);
  if (coeffs) memcpy(coeffs, host.data() + np, (size_t)np * kCoefPerPiece * 8);
  if (knots_xy) memcpy(knots_xy, host.data() + np + (size_t)np * kCoefPerPiece, kn * 8);
  return TOPAY_OK;
}

topay_status topay_get_polytraj_msg(topay_ctx* c, int i, int cap_pieces, unsigned char* order, float* coeff, float* durations,
                                    signed char* directions, int* n_pieces) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B) return TOPAY_ERR_INVALID_ARG;
  const int N = c->hN[i];
  if (n_pieces) *n_pieces = N;
  if (order) *order = 5;
  if (N == 0) return TOPAY_OK;
  if (N > cap_pieces) return TOPAY_ERR_INVALID_ARG;
  constexpr int CP = kCoefPerPiece;
  std::vector<double> dur((size_t)N), cf((size_t)N * CP);
  topay_status s = topay_get_result(c, i, nullptr, nullptr, nullptr, dur.data(), cf.data(), nullptr);
  if (s != TOPAY_OK) return s;
  for (int p = 0; p < N; p++) {
    if (durations) durations[p] = (float)dur[p];
    if (coeff)
      for (int t = 0; t < CP; t++) coeff[(size_t)p * CP + t] = (float)cf[(size_t)p * CP + t];
    if (directions) {
      // arc-length rate (dimension 1) at the middle of the piece; coefficients are highest order first
      const double* a = &cf[(size_t)p * CP + 6], t = 0.5 * dur[p];
      const double sd = ((((5.0 * a[0]) * t + 4.0 * a[1]) * t + 3.0 * a[2]) * t + 2.0 * a[3]) * t + a[4];
      directions[p] = sd < 0.0 ? -1 : 1;
    }
  }
  return TOPAY_OK;
}

topay_status topay_get_x(topay_ctx* c, int i, int* n, double* x) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (i < 0 || i >= c->B) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (c->hN[i] == 0) { if (n) *n = 0; return TOPAY_ERR_TOO_MANY_PIECES; }
  const int nn = 10 * c->hN[i] - 8;
  if (n) *n = nn;
  if (x) {
    // after optimize: the final iterate; before: the packed initial guess
    if (c->solved) HIPCHK(d2h_sync(c, x, c->db.x_of(c->h_noff[i]), (size_t)nn));
    else HIPCHK(d2h_sync(c, x, c->db.x0_of(i), (size_t)nn));
  }
  return TOPAY_OK;
}

topay_status topay_eval(topay_ctx* c, int stage, int i, const double* x, const double* alm_lambda, const double* alm_rho,
                        double* f, double* g, double* final_xy_error) {
  return eval_one(c, stage, i, x, alm_lambda, alm_rho, f, g, final_xy_error, false);
}

// Test hook: the same evaluation by the kernel with `waves` wavefronts per trajectory (1, 2 or 4) instead of the
// candidate's class default.  An evaluation is order-identical whatever the number of waves (topay_eval.h): the
// results must agree bit for bit.
topay_status topay_eval_waves(topay_ctx* c, int stage, int i, int waves, const double* x, const double* alm_lambda, const double* alm_rho,
                              double* f, double* g, double* final_xy_error) {
  if (waves != 1 && waves != 2 && waves != 4) return TOPAY_ERR_INVALID_ARG;
  return eval_one(c, stage, i, x, alm_lambda, alm_rho, f, g, final_xy_error, false, waves);
}

// The spline of a given decision vector as candidate i's result (MomaTrajOpt keeps the MINCO state of its last cost
// evaluation, moma_traj_opt.h:943-946: getTraj() after an evaluation at x returns exactly this): one stage-2
// evaluation at x with the given ALM state, after which getTraj / playback / gate / message entry points serve x's
// trajectory.  Replay and warm-start entry; the cost stored is the stage-2 cost at x.
topay_status topay_load_solution(topay_ctx* c, int i, const double* x, const double* alm_lambda, const double* alm_rho) {
  topay_status s = eval_one(c, 2, i, x, alm_lambda, alm_rho, nullptr, nullptr, nullptr, true);
  if (s == TOPAY_OK) {
    c->solved = true;
    c->gate_done = false;   // (the gate of a loaded trajectory: the separate kernel)
    const int zero = 0;     // the candidate has a trajectory now, whatever a solve before left in its flag
    HIPCHK(h2d_sync(c, c->interrupted.as<int>() + i, &zero, 1));
  }
  return s;
}

// Batched hook: evaluate every candidate `repeats` times at its packed initial guess x0 (ALM state = initial).
topay_status topay_eval_batch(topay_ctx* c, int stage, int repeats, double* f) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if ((stage != 1 && stage != 2) || repeats == 0) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  // x <- x0 (strided copy), alm <- init
  std::vector<double> x0((size_t)c->B * kX0Stride), xs((size_t)c->h_noff[c->B] + 1, 0.0), alm((size_t)c->B * kAlmLen);
  HIPCHK(d2h_sync(c, x0.data(), c->x0.as<double>(), x0.size()));
  for (int b = 0; b < c->B; b++) {
    if (c->hN[b] == 0) continue;
    const int nn = 10 * c->hN[b] - 8;
    memcpy(&xs[(size_t)c->h_noff[b]], &x0[(size_t)b * kX0Stride], (size_t)nn * 8);
    double* ab = &alm[(size_t)kAlmLen * b];
    ab[0] = c->hp.alm_init_lambda[0]; ab[1] = c->hp.alm_init_lambda[1];
    ab[2] = c->hp.alm_init_rho[0]; ab[3] = c->hp.alm_init_rho[1];
  }
  HIPCHK(h2d_sync(c, c->x.as<double>(), xs.data(), (size_t)c->h_noff[c->B]));
  HIPCHK(h2d_sync(c, c->alm.as<double>(), alm.data(), alm.size()));
  HIPCHK(c->eval_timer.start(c->stream));
  topay_status s = launch_classes<true>(c, false, stage, repeats);
  if (s != TOPAY_OK) return s;
  HIPCHK(c->eval_timer.stop(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->eval_timer.read(&c->last_ms));
  if (f) HIPCHK(d2h_sync(c, f, c->fout.as<double>(), (size_t)c->B));
  return TOPAY_OK;
}

topay_status topay_check_feasible(topay_ctx* c, int* feasible) {
  return topay_feasibility_report(c, feasible, nullptr, nullptr);
}

topay_status topay_feasibility_report(topay_ctx* c, int* feasible, int* strict, double* report) {
  if (!c || !c->have_traj || !c->solved) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  const int B = c->B;
  if (c->gate_done) {   // the solving waves have gated their own trajectories: verdicts and extremes are resident
    std::vector<int> fl((size_t)B * 2);
    HIPCHK(d2h_sync(c, fl.data(), c->feas_flags.as<int>(), fl.size()));
    for (int b = 0; b < B; b++) {
      if (feasible) feasible[b] = fl[2 * b];
      if (strict) strict[b] = fl[2 * b + 1];
    }
    if (report) HIPCHK(d2h_sync(c, report, c->feas_report.as<double>(), (size_t)B * kReportLen));
    return TOPAY_OK;
  }
  // scratch is sized from the longest returned trajectory
  std::vector<double> hT((size_t)c->h_poff[B] + 1);
  HIPCHK(d2h_sync(c, hT.data(), c->T.as<double>(), (size_t)c->h_poff[B]));
  double tmax = 0.0;
  for (int b = 0; b < B; b++) {
    double t = 0.0;
    for (int i = 0; i < c->hN[b]; i++) t += hT[(size_t)c->h_poff[b] + i];
    if (t > 0.0 && t < 1.0e4 && t > tmax) tmax = t;
  }
  const long long cap_panels = (long long)(tmax / 0.025) + 4, cap_samples = (long long)(tmax / 0.01) + 16;
  topay_status s;
  if ((s = c->feas_cseq.ensure((size_t)B * 2 * (cap_panels + 1) * 8)) != TOPAY_OK) return s;
  if ((s = c->feas_tk.ensure((size_t)B * cap_samples * 8)) != TOPAY_OK) return s;
  if ((s = c->feas_report.ensure((size_t)B * kReportLen * 8)) != TOPAY_OK) return s;
  if ((s = c->feas_flags.ensure((size_t)B * 2 * 4)) != TOPAY_OK) return s;
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  hipLaunchKernelGGL(k_feasible, dim3(B), dim3(64), 0, c->stream, c->db, (const DevMap*)c->dmaps.p, c->feas_cseq.as<double>(),
                     c->feas_tk.as<double>(), cap_panels, cap_samples, c->feas_report.as<double>(), c->feas_flags.as<int>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<int> fl((size_t)B * 2), intr(B);
  HIPCHK(d2h_sync(c, fl.data(), c->feas_flags.as<int>(), fl.size()));
  // an interrupted candidate has no trajectory (its result block holds the spline of the evaluation it was stopped in):
  // its verdicts stay 0 / 0, as the in-solve path and the cancellation post-pass of topay_synchronize write them
  HIPCHK(d2h_sync(c, intr.data(), c->interrupted.as<int>(), (size_t)B));
  bool changed = false;
  for (int b = 0; b < B; b++)
    if (intr[b] && (fl[2 * b] || fl[2 * b + 1])) { fl[2 * b] = 0; fl[2 * b + 1] = 0; changed = true; }
  if (changed) HIPCHK(h2d_sync(c, c->feas_flags.as<int>(), fl.data(), fl.size()));
  c->gate_done = true;   // resident until the next solve, load or re-initialisation (each resets it)
  for (int b = 0; b < B; b++) {
    if (feasible) feasible[b] = fl[2 * b];
    if (strict) strict[b] = fl[2 * b + 1];
  }
  if (report) HIPCHK(d2h_sync(c, report, c->feas_report.as<double>(), (size_t)B * kReportLen));
  return TOPAY_OK;
}

// Debug / parity tooling: record f of every evaluation of the next topay_optimize (cap per candidate; 0 = off).
topay_status topay_set_trace(topay_ctx* c, int cap) {
  if (!c || !c->have_traj || cap < 0) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  c->trace_cap = cap;
  c->db.trace = nullptr;
  c->db.trace_cap = 0;
  if (cap > 0) {
    topay_status s = c->trace.ensure((size_t)c->B * cap * 8);
    if (s != TOPAY_OK) return s;
    HIPCHK(hipMemsetAsync(c->trace.p, 0, (size_t)c->B * cap * 8, c->stream));
    c->db.trace = c->trace.as<double>();
    c->db.trace_cap = cap;
  }
  return TOPAY_OK;
}
topay_status topay_get_trace(topay_ctx* c, int i, double* out) {
  if (!c || !c->have_traj || c->trace_cap <= 0 || i < 0 || i >= c->B) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(d2h_sync(c, out, c->trace.as<double>() + (size_t)i * c->trace_cap, (size_t)c->trace_cap));
  return TOPAY_OK;
}

// Test hook: evaluate the deterministic sin/cos/atan2 (and an IEEE sqrt/div probe) on the device.
topay_status topay_test_math(topay_ctx* c, int n, const double* a, const double* b, double* out4n) {
  if (!c || n <= 0 || !a || !b || !out4n) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  DevBuf da, dbb, dout;
  topay_status s;
  if ((s = da.ensure((size_t)n * 8)) != TOPAY_OK || (s = dbb.ensure((size_t)n * 8)) != TOPAY_OK ||
      (s = dout.ensure((size_t)n * 32)) != TOPAY_OK)
    return s;
  HIPCHK(h2d_sync(c, da.as<double>(), a, (size_t)n));
  HIPCHK(h2d_sync(c, dbb.as<double>(), b, (size_t)n));
  hipLaunchKernelGGL(k_math, dim3((n + 63) / 64), dim3(64), 0, c->stream, da.as<double>(), dbb.as<double>(), dout.as<double>(), n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(d2h_sync(c, out4n, dout.as<double>(), (size_t)n * 4));
  return TOPAY_OK;
}

// Launch class of a candidate with n_pieces pieces: waves per trajectory and decision-vector elements per thread of
// the kernel that solves (and, through topay_eval, evaluates) it.  The division of the L-BFGS vectors over the threads
// -- and with it the rounding of every dot product -- is a function of these two; parity tooling that restates the
// solver in the device's order needs them (oracle/: device-order mode).
topay_status topay_class_of(int n_pieces, int* waves, int* elements_per_thread, int* class_index) {
  if (n_pieces <= 0 || n_pieces > TOPAY_MAX_N) return TOPAY_ERR_TOO_MANY_PIECES;
  const int k = bucket_of(n_pieces);
  const ClassDef& cd = kClassTable[k];
  if (waves) *waves = 1;
  if (elements_per_thread) *elements_per_thread = 2 * cd.srmax();
  if (class_index) *class_index = k;
  return TOPAY_OK;
}

// Device memory held by the resident batch (everything topay_set_init_traj sized), in bytes.
topay_status topay_workspace_bytes(topay_ctx* c, unsigned long long* bytes) {
  if (!c || !bytes) return TOPAY_ERR_INVALID_ARG;
  *bytes = (unsigned long long)c->workspace_bytes;
  return TOPAY_OK;
}

topay_status topay_gate_timeouts(topay_ctx* c, int* n) {
  if (!c || !n) return TOPAY_ERR_INVALID_ARG;
  *n = c->gate_timeouts;
  return TOPAY_OK;
}

topay_status topay_last_kernel_ms(topay_ctx* c, double* ms, int* launches) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  if (ms) *ms = c->last_ms;
  if (launches) *launches = c->last_launches;
  return TOPAY_OK;
}

topay_status topay_last_helper_launches(topay_ctx* c, int* n) {
  if (!c || !n) return TOPAY_ERR_INVALID_ARG;
  *n = c->last_helper_launches;
  return TOPAY_OK;
}

#if defined(TOPAY_STAMPS) && !defined(TOPAY_CPU_EMU)
// diagnostic build only: per-phase cycle counters of the manipulator block (lane 0 of block 0)
topay_status topay_debug_mani_stamps(long long* out8) {
  HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(topay::g_mani_stamps), 64));
  return TOPAY_OK;
}
#endif

}  // extern "C"
