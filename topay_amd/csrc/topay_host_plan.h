// Host side of the C-ABI, part 7: topay_plan_calls and the store of its winners.

#pragma once

// ---------------------------------------------------------------------------------------------------------------------
// topay_plan_calls: Planner::planMomaParallel (planner.cpp:792-1061) with every hand-off on the device (topay_plan.h)
// ---------------------------------------------------------------------------------------------------------------------
// Calls per launch of the front-end stages (roadmap, JPS, dense paths, search).  The instance numbers of the draws are
// those of the call, so results do not depend on it; it bounds the roadmap's 1.1 MB per query.
#ifndef TOPAY_PLAN_CHUNK
#define TOPAY_PLAN_CHUNK 1024
#endif
static const int kPlanChunk = TOPAY_PLAN_CHUNK;
static const int kPlanDenseCap = 256;   // entries per dense path kept (the search takes at most 255 layers)
static const int kPlanJpsCap = 512;     // points per JPS path kept

// A device buffer that keeps its first `used` bytes when it has to grow.
static topay_status grow_keep(topay_ctx* c, DevBuf& b, size_t need, size_t used) {
  if (need <= b.bytes) return TOPAY_OK;
  DevBuf nb;
  topay_status s = nb.ensure(std::max(need, 2 * b.bytes));
  if (s != TOPAY_OK) return s;
  if (used > 0 && b.p) {
    hipError_t e = memcpy_sync(c, nb.p, b.p, used, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { set_err(std::string("grow_keep: ") + hipGetErrorString(e)); return TOPAY_ERR_NO_DEVICE; }
  }
  b = std::move(nb);
  return TOPAY_OK;
}

// Device time of one stage: a pair of events around its launches on the context's stream, read once the call has finished.
// Only pairs whose end has been recorded in THIS call are read (an error return between begin and end leaves none behind).
struct PlanClock {
  topay_ctx* c;
  size_t used = 0;
  explicit PlanClock(topay_ctx* c_) : c(c_) {}
  int reserve(int stage) {   // a pair for a launcher that records the events itself, around its kernels only; then done(id)
    if (used + 2 > c->pl_events.size()) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess) return -1;
      if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return -1; }
      c->pl_events.push_back(a);
      c->pl_events.push_back(b);
    }
    c->pl_event_stage.resize(c->pl_events.size() / 2);
    c->pl_event_done.resize(c->pl_events.size() / 2);
    const int id = (int)(used / 2);
    c->pl_event_stage[id] = stage;
    c->pl_event_done[id] = 0;
    used += 2;
    return id;
  }
  hipEvent_t ev(int id, int which) { return id < 0 ? nullptr : c->pl_events[2 * (size_t)id + which]; }
  void done(int id) { if (id >= 0) c->pl_event_done[id] = 1; }
  int begin(int stage) {
    const int id = reserve(stage);
    if (id >= 0) (void)hipEventRecord(ev(id, 0), c->stream);
    return id;
  }
  void end(int id) {
    if (id >= 0 && hipEventRecord(ev(id, 1), c->stream) == hipSuccess) done(id);
  }
  void collect() {
    (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i + 1 < used; i += 2) {
      float ms = 0.f;
      if (c->pl_event_done[i / 2] && hipEventElapsedTime(&ms, c->pl_events[i], c->pl_events[i + 1]) == hipSuccess)
        c->pl_stage_ms[c->pl_event_stage[i / 2]] += ms;
    }
  }
};

struct PlanTry {   // the survivors of one try, over all front-end launches: the batch that is solved
  std::vector<int> call, k, len, mid;
  std::vector<long long> off{0};
};

// One try (t = 0 plain, 1 critical) for the calls `act`: front-end in launches of kPlanChunk calls, one solve, winners
// into the store.  Fills the calls' rows of result / cand (n x 2 x 8 x 4) / wcd.  Call p has the number call_nos[p], or
// first_call + p when call_nos is null (the replanning cycle numbers its calls itself).
static topay_status plan_try(topay_ctx* c, int t, const std::vector<int>& act, const std::vector<int>& mids, const double* start, const double* end,
                             const double* start_v, const topay_plan_params_t& P, unsigned long long first_call, const unsigned long long* call_nos, int* result,
                             int* cand, double* wcd, PlanClock& clk) {
  topay_status s;
  PlanTry T;
  const int cap_paths = P.topo.reserve_num;
  const size_t chunk = (size_t)(c->pl_chunk > 0 ? c->pl_chunk : kPlanChunk);
  for (size_t a0 = 0; a0 < act.size(); a0 += chunk) {
    const int nc = (int)std::min<size_t>(chunk, act.size() - a0);
    const size_t NC = (size_t)nc, NS = NC * TOPAY_PLAN_MAX_CAND;
    // ---- the launch's calls: inputs of the caller, gathered on the host
    std::vector<double> sxy(2 * NC), exy(2 * NC), st10(10 * NC), en10(10 * NC), sv10(10 * NC, 0.0);
    std::vector<int> cmid(NC), crit(NC, t);
    std::vector<unsigned long long> inst(NC), call_no(NC);
    int cap_points = 2;
    for (int q = 0; q < nc; q++) {
      const int p = act[a0 + q];
      memcpy(&st10[10 * (size_t)q], start + 10 * (size_t)p, 80);
      memcpy(&en10[10 * (size_t)q], end + 10 * (size_t)p, 80);
      if (start_v) memcpy(&sv10[10 * (size_t)q], start_v + 10 * (size_t)p, 80);
      sxy[2 * (size_t)q] = start[10 * (size_t)p]; sxy[2 * (size_t)q + 1] = start[10 * (size_t)p + 1];
      exy[2 * (size_t)q] = end[10 * (size_t)p]; exy[2 * (size_t)q + 1] = end[10 * (size_t)p + 1];
      cmid[q] = mids[p];
      call_no[q] = call_nos ? call_nos[p] : first_call + (unsigned long long)p;
      inst[q] = 2ull * call_no[q] + (unsigned long long)t;
      const DevMap& m = c->hmaps[cmid[q]];
      cap_points = std::max(cap_points, topo_pt_cap(m.dims[0], m.dims[1]));   // no selected path has more points than its map's cap
    }
    const size_t topo_pts = NC * (size_t)cap_paths * cap_points;
    if ((s = c->pl_raw.ensure((topo_pts + NC * kPlanJpsCap) * 16)) != TOPAY_OK) return s;
    // calls: start | end | start_v (10 each), call numbers, map slots
    double *d_st, *d_en, *d_sv; unsigned long long* d_callno; int* d_cmid;
    auto lay_io = [&](Carver& k) {
      d_st = k.take<double>(10 * NC); d_en = k.take<double>(10 * NC); d_sv = k.take<double>(10 * NC);
      d_callno = k.take<unsigned long long>(NC); d_cmid = k.take<int>(NC);
    };
    if ((s = c->pl_io.carve(lay_io)) != TOPAY_OK) return s;
    HIPCHK(h2d(c, d_st, st10.data(), 10 * NC));
    HIPCHK(h2d(c, d_en, en10.data(), 10 * NC));
    HIPCHK(h2d(c, d_sv, sv10.data(), 10 * NC));
    HIPCHK(h2d(c, d_callno, call_no.data(), NC));
    HIPCHK(h2d(c, d_cmid, cmid.data(), NC));
    // ---- roadmap, JPS
    TopoDev td;
    int id = clk.reserve(0);   // (the launchers record around their kernels: uploads, allocations and waits stay outside)
    s = topo_impl(c, nc, cmid.data(), sxy.data(), exy.data(), crit.data(), &P.topo, 0, inst.data(), cap_paths, cap_points, c->pl_raw.as<double>(), false, &td,
                  clk.ev(id, 0), clk.ev(id, 1));
    if (s != TOPAY_OK) return s;
    clk.done(id);
    JpsDev jd;
    jd.len = nullptr;
    if (t == 0) {
      id = clk.reserve(1);
      s = jps_impl(c, nc, cmid.data(), sxy.data(), exy.data(), c->hp.chassis_colli_radius + P.jps_margin, kPlanJpsCap, c->pl_jps_io,
                   c->pl_raw.as<double>() + 2 * topo_pts, &jd, clk.ev(id, 0), clk.ev(id, 1));
      if (s != TOPAY_OK) return s;
      clk.done(id);
    }
    // ---- candidate table, dense paths
    double *d_syaw, *d_eyaw, *d_dense; long long* d_rawoff; int *d_ncand, *d_rawlen, *d_denselen;
    auto lay_tab = [&](Carver& k) {
      d_syaw = k.take<double>(NS); d_eyaw = k.take<double>(NS); d_rawoff = k.take<long long>(NS); d_dense = k.take<double>(NS * kPlanDenseCap * 4);
      d_ncand = k.take<int>(NC); d_rawlen = k.take<int>(NS); d_denselen = k.take<int>(NS);
    };
    if ((s = c->pl_tab.carve(lay_tab)) != TOPAY_OK) return s;
    topay::PlanCandArgs A;
    A.n = nc; A.cap_paths = cap_paths; A.cap_points = cap_points; A.jps_cap = kPlanJpsCap; A.max_cand = P.max_candidates;
    A.jps_base = (long long)topo_pts;
    A.topo_np = td.n_paths; A.topo_len = td.path_len; A.jps_len = jd.len; A.start = d_st; A.end = d_en;
    A.ncand = d_ncand; A.raw_off = d_rawoff; A.raw_len = d_rawlen; A.syaw = d_syaw; A.eyaw = d_eyaw;
    id = clk.begin(2);
    hipLaunchKernelGGL(topay::k_plan_candidates, dim3((nc + 63) / 64), dim3(64), 0, c->stream, A);
    HIPCHK(hipGetLastError());
    if ((s = dense_launch(c, (int)NS, c->pl_raw.as<double>(), d_rawoff, d_rawlen, P.dense_step, d_syaw, d_eyaw, c->hp.max_v, c->hp.max_w, kPlanDenseCap,
                          d_dense, d_denselen)) != TOPAY_OK)
      return s;
    clk.end(id);
    std::vector<int> ncand(NC), dlen(NS), tstat(NC * 8);
    HIPCHK(d2h(c, ncand.data(), d_ncand, NC));
    HIPCHK(d2h(c, dlen.data(), d_denselen, NS));
    HIPCHK(d2h(c, tstat.data(), td.stats, NC * 8));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int> sel;
    int layer_cap = 2;
    for (int q = 0; q < nc; q++) {
      const int p = act[a0 + q];
      int* r = result + 8 * (size_t)p;
      r[1] = t;
      r[2 + t] = std::abs(ncand[q]);
      r[6] = tstat[8 * (size_t)q];
      if (ncand[q] < 0) { r[0] = -3; continue; }
      for (int k = 0; k < ncand[q]; k++) {
        const int sl = q * TOPAY_PLAN_MAX_CAND + k;
        sel.push_back(sl);
        layer_cap = std::max(layer_cap, std::min(dlen[sl], 255));
        if (cand) cand[(((size_t)p * 2 + t) * 8 + k) * 4] = topay::PLAN_SEARCH_FAILED;   // until it gets further
      }
    }
    const int ni = (int)sel.size();
    if (ni == 0) continue;
    // ---- the search: hand-off kernel, k_mcrrt
    const size_t NI = (size_t)ni;
    long long* d_off; unsigned long long* d_inst; double *d_s, *d_e, *d_wb, *d_cmax; int *d_sel, *d_len, *d_mid, *d_wlen, *d_mstat;
    auto lay_mc = [&](Carver& k) {
      d_off = k.take<long long>(NI); d_inst = k.take<unsigned long long>(NI);
      d_s = k.take<double>(10 * NI); d_e = k.take<double>(10 * NI); d_wb = k.take<double>(NI * layer_cap * 10); d_cmax = k.take<double>(NI);
      d_sel = k.take<int>(NI); d_len = k.take<int>(NI); d_mid = k.take<int>(NI); d_wlen = k.take<int>(NI); d_mstat = k.take<int>(8 * NI);
    };
    if ((s = c->pl_mc.carve(lay_mc)) != TOPAY_OK) return s;
    HIPCHK(h2d(c, d_sel, sel.data(), NI));
    id = clk.begin(3);
    hipLaunchKernelGGL(topay::k_plan_pack_search, dim3((ni + 63) / 64), dim3(64), 0, c->stream, ni, (const int*)d_sel, kPlanDenseCap, (const int*)d_denselen,
                       (const double*)d_st, (const double*)d_en, (const int*)d_cmid, (const unsigned long long*)d_callno, t, d_off, d_len, d_s, d_e, d_mid,
                       d_inst);
    HIPCHK(hipGetLastError());
    McIo io;
    io.off = d_off; io.len = d_len; io.car = d_dense; io.start = d_s; io.end = d_e; io.mid = d_mid; io.inst = d_inst;
    io.wb_len = d_wlen; io.wb = d_wb; io.stats = d_mstat; io.cmax = d_cmax;
    if ((s = mcrrt_launch(c, ni, P.mcrrt, 0, layer_cap, io)) != TOPAY_OK) return s;
    clk.end(id);
    std::vector<int> wlen(NI), mstat(NI * 8);
    HIPCHK(d2h(c, wlen.data(), d_wlen, NI));
    HIPCHK(d2h(c, mstat.data(), d_mstat, 8 * NI));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int> src, src_call;
    std::vector<long long> poff;
    const int b0 = (int)T.call.size();
    for (int i = 0; i < ni; i++) {
      const int q = sel[i] / TOPAY_PLAN_MAX_CAND, k = sel[i] % TOPAY_PLAN_MAX_CAND, p = act[a0 + q];
      if (cand) cand[(((size_t)p * 2 + t) * 8 + k) * 4 + 2] = mstat[8 * (size_t)i];
      if (mstat[8 * (size_t)i] != 1 || wlen[i] < 2) continue;
      src.push_back(i);
      src_call.push_back(q);
      poff.push_back(T.off.back());
      T.call.push_back(p); T.k.push_back(k); T.len.push_back(wlen[i]); T.mid.push_back(mids[p]);
      T.off.push_back(T.off.back() + wlen[i]);
    }
    const int nsv = (int)src.size();
    if (nsv == 0) continue;
    // ---- hand-off to the solver: ragged init paths and boundary velocities of the try, appended launch by launch
    if ((s = grow_keep(c, c->pl_paths, (size_t)T.off.back() * 80, (size_t)poff[0] * 80)) != TOPAY_OK) return s;
    if ((s = grow_keep(c, c->pl_bvel, T.call.size() * 160, (size_t)b0 * 160)) != TOPAY_OK) return s;
    long long* d_poff; int *d_src, *d_srccall;
    auto lay_sel = [&](Carver& k) { d_poff = k.take<long long>((size_t)nsv); d_src = k.take<int>((size_t)nsv); d_srccall = k.take<int>((size_t)nsv); };
    if ((s = c->pl_sel.carve(lay_sel)) != TOPAY_OK) return s;
    HIPCHK(h2d(c, d_poff, poff.data(), (size_t)nsv));
    HIPCHK(h2d(c, d_src, src.data(), (size_t)nsv));
    HIPCHK(h2d(c, d_srccall, src_call.data(), (size_t)nsv));
    id = clk.begin(4);
    hipLaunchKernelGGL(topay::k_plan_pack_solver, dim3((unsigned)nsv), dim3(64), 0, c->stream, nsv, (const int*)d_src, (const int*)d_srccall, layer_cap,
                       (const int*)d_wlen, (const double*)d_wb, (const long long*)d_poff, (const double*)d_sv, b0, c->pl_paths.as<double>(),
                       c->pl_bvel.as<double>());
    HIPCHK(hipGetLastError());
    clk.end(id);
    HIPCHK(hipStreamSynchronize(c->stream));   // (the launch's buffers are reused by the next one)
  }
  const int B = (int)T.call.size();
  if (B == 0) return TOPAY_OK;   // no candidate of any call survived to the solve: the try fails for all of them
  // ---- one batch: init, groups, solve, gate
  int id = clk.begin(4);
  s = set_init_traj_impl(c, B, T.len.data(), c->pl_paths.as<double>(), c->pl_bvel.as<double>(), nullptr, T.mid.data(), hipMemcpyDeviceToDevice);
  clk.end(id);
  if (s == TOPAY_ERR_TOO_MANY_PIECES) {   // every candidate needs more pieces than the build solves
    if (cand)
      for (int b = 0; b < B; b++) cand[(((size_t)T.call[b] * 2 + t) * 8 + T.k[b]) * 4] = topay::PLAN_TOO_MANY_PIECES;
    return TOPAY_OK;
  }
  if (s != TOPAY_OK) return s;
  if ((s = topay_set_groups(c, T.call.data(), P.cancel_budget)) != TOPAY_OK) return s;
  if ((s = topay_optimize(c)) != TOPAY_OK) return s;
  c->pl_stage_ms[5] += c->last_ms;
  std::vector<int> feas(B);
  id = clk.begin(6);
  if ((s = topay_check_feasible(c, feas.data())) != TOPAY_OK) return s;
  // ---- winners: per call one lane over its candidates (adjacent in the batch, in candidate order)
  std::vector<int> qcall, first, count;
  for (int b = 0; b < B; b++) {
    if (qcall.empty() || qcall.back() != T.call[b]) { qcall.push_back(T.call[b]); first.push_back(b); count.push_back(0); }
    count.back()++;
  }
  const int Q = (int)qcall.size();
  double* d_wcd; int *d_first, *d_count, *d_win, *d_stage;
  auto lay_win = [&](Carver& k) {
    d_wcd = k.take<double>(2 * (size_t)Q);
    d_first = k.take<int>((size_t)Q); d_count = k.take<int>((size_t)Q); d_win = k.take<int>((size_t)Q); d_stage = k.take<int>((size_t)B);
  };
  if ((s = c->pl_win.carve(lay_win)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_first, first.data(), (size_t)Q));
  HIPCHK(h2d(c, d_count, count.data(), (size_t)Q));
  hipLaunchKernelGGL(topay::k_plan_winner, dim3((Q + 63) / 64), dim3(64), 0, c->stream, c->db, Q, (const int*)d_first, (const int*)d_count, d_stage, d_win, d_wcd);
  HIPCHK(hipGetLastError());
  clk.end(id);
  std::vector<int> win(Q), stage(B), sst((size_t)B * kStatsLen);
  std::vector<double> hw(2 * (size_t)Q);
  HIPCHK(d2h(c, win.data(), d_win, (size_t)Q));
  HIPCHK(d2h(c, stage.data(), d_stage, (size_t)B));
  HIPCHK(d2h(c, hw.data(), d_wcd, 2 * (size_t)Q));
  HIPCHK(d2h(c, sst.data(), c->stats.as<int>(), sst.size()));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (cand)
    for (int b = 0; b < B; b++) {
      int* e = cand + (((size_t)T.call[b] * 2 + t) * 8 + T.k[b]) * 4;
      e[0] = stage[b]; e[1] = c->hN[b]; e[3] = c->hN[b] > 0 ? sst[(size_t)b * kStatsLen + 3] : 0;
    }
  // ---- the winners into the store: trajectories in the layout of k_gather_results, init paths after them
  std::vector<int> widx, woff{0}, foff{0};
  for (int q = 0; q < Q; q++) {
    if (win[q] < 0) continue;
    const int p = qcall[q], b = win[q];
    int* r = result + 8 * (size_t)p;
    r[0] = 1; r[1] = t; r[4] = T.k[b]; r[5] = c->hN[b]; r[7] = b;
    if (wcd) { wcd[2 * (size_t)p] = hw[2 * (size_t)q]; wcd[2 * (size_t)p + 1] = hw[2 * (size_t)q + 1]; }
    topay_ctx::PlanStored& e = c->ps_calls[p];
    e.n_pieces = c->hN[b];
    e.piece0 = (int)c->ps_pieces + woff.back();
    e.knot0 = (int)c->ps_pieces + (int)c->ps_winners + woff.back() + (int)widx.size();
    e.front0 = (int)c->ps_states + foff.back();
    e.front_len = T.len[b];
    widx.push_back(b);
    woff.push_back(woff.back() + c->hN[b]);
    foff.push_back(foff.back() + T.len[b]);
  }
  const int W = (int)widx.size();
  if (W == 0) return TOPAY_OK;
  const size_t np = (size_t)woff.back(), P0 = c->ps_pieces, W0 = c->ps_winners, F0 = c->ps_states;
  if ((s = grow_keep(c, c->ps_dur, (P0 + np) * 8, P0 * 8)) != TOPAY_OK || (s = grow_keep(c, c->ps_coef, (P0 + np) * kCoefPerPiece * 8, P0 * kCoefPerPiece * 8)) != TOPAY_OK ||
      (s = grow_keep(c, c->ps_kn, 2 * (P0 + W0 + np + W) * 8, 2 * (P0 + W0) * 8)) != TOPAY_OK ||
      (s = grow_keep(c, c->ps_front, (F0 + (size_t)foff.back()) * 80, F0 * 80)) != TOPAY_OK)
    return s;
  int *d_idx, *d_woff, *d_foff;
  auto lay_sel = [&](Carver& k) { d_idx = k.take<int>((size_t)W); d_woff = k.take<int>((size_t)W + 1); d_foff = k.take<int>((size_t)W + 1); };
  if ((s = c->pl_sel.carve(lay_sel)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_idx, widx.data(), (size_t)W));
  HIPCHK(h2d(c, d_woff, woff.data(), (size_t)W + 1));
  HIPCHK(h2d(c, d_foff, foff.data(), (size_t)W + 1));
  id = clk.begin(7);
  hipLaunchKernelGGL(k_gather_results, dim3(W), dim3(64), 0, c->stream, c->db, W, (const int*)d_idx, (const int*)d_woff, c->ps_dur.as<double>() + P0,
                     c->ps_coef.as<double>() + kCoefPerPiece * P0, c->ps_kn.as<double>() + 2 * (P0 + W0));
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(topay::k_plan_gather_front, dim3(W), dim3(64), 0, c->stream, W, (const int*)d_idx, (const double*)c->paths.as<double>(),
                     (const long long*)c->path_off.as<long long>(), (const int*)d_foff, c->ps_front.as<double>() + 10 * F0);
  HIPCHK(hipGetLastError());
  clk.end(id);
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ps_pieces += np; c->ps_winners += (size_t)W; c->ps_states += (size_t)foff.back();
  return TOPAY_OK;
}

extern "C" {

void topay_plan_default_params(topay_plan_params_t* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  topay_topo_default_params(&p->topo);
  topay_mcrrt_default_params(&p->mcrrt);
  p->dense_step = 1.414;       // planner.cpp:858
  p->jps_margin = 0.1;         // planner.cpp:816
  p->cancel_budget = 2400;     // the 100 ms of planner.cpp:946 in piece-evaluations
  p->max_candidates = 8;       // traj_opters.size(), planner.cpp:59
  p->critical_retry = 1;       // planner.cpp:961-963
}

static topay_status plan_calls_impl(topay_ctx* c, int n, const int* map_ids, const double* start, const double* end, const double* start_v,
                                    const topay_plan_params_t* params, unsigned long long first_call, const unsigned long long* call_nos, int* result,
                                    int* candidates, double* winner_cost_duration) {
  if (!c || n <= 0 || !start || !end || !result) return TOPAY_ERR_INVALID_ARG;
  topay_plan_params_t P;
  if (params) P = *params;
  else topay_plan_default_params(&P);
  if (P.max_candidates < 1 || P.max_candidates > TOPAY_PLAN_MAX_CAND || !(P.dense_step > 0.0) || P.cancel_budget < 0 || !mcrrt_params_ok(P.mcrrt) ||
      P.topo.reserve_num < 1 || P.topo.reserve_num > 16) {
    set_err("topay_plan_calls: parameters out of range (max_candidates 1..8, dense_step > 0, cancel_budget >= 0)");
    return TOPAY_ERR_INVALID_ARG;
  }
  std::vector<int> mids((size_t)n, 0);
  for (int p = 0; p < n; p++) {
    mids[p] = map_ids ? map_ids[p] : 0;
    if (mids[p] < 0 || mids[p] >= TOPAY_MAX_MAPS) return TOPAY_ERR_INVALID_ARG;
    if (!c->have_map[mids[p]]) { set_err("map slot not set"); return TOPAY_ERR_NO_MAP; }
    const DevMap& m = c->hmaps[mids[p]];
    if (!m.esdf2d_inflate || !m.esdf2d_critical) {
      set_err("topay_plan_calls: map slot " + std::to_string(mids[p]) + " has no front-end fields: fill it with topay_build_esdf*, not topay_set_map");
      return TOPAY_ERR_NO_MAP;
    }
  }
  HIPCHK(hipSetDevice(c->device));
  if (c->pending) { topay_status ws = topay_synchronize(c); if (ws != TOPAY_OK) return ws; }
  c->ps_calls.assign((size_t)n, topay_ctx::PlanStored());
  c->ps_pieces = c->ps_winners = c->ps_states = 0;
  for (int k = 0; k < 8; k++) c->pl_stage_ms[k] = 0.0;
  for (int p = 0; p < n; p++) {
    int* r = result + 8 * (size_t)p;
    r[0] = 0; r[1] = -1; r[2] = 0; r[3] = 0; r[4] = -1; r[5] = 0; r[6] = 0; r[7] = -1;
    if (winner_cost_duration) winner_cost_duration[2 * (size_t)p] = winner_cost_duration[2 * (size_t)p + 1] = 0.0 / 0.0;
  }
  if (candidates) memset(candidates, 0, (size_t)n * 2 * 8 * 4 * sizeof(int));
  PlanClock clk(c);
  topay_status s = TOPAY_OK;
  for (int t = 0; t < 2 && s == TOPAY_OK; t++) {
    if (t == 1 && !P.critical_retry) break;
    std::vector<int> act;
    for (int p = 0; p < n; p++)
      if (result[8 * (size_t)p] == 0) act.push_back(p);
    if (act.empty()) break;
    s = plan_try(c, t, act, mids, start, end, start_v, P, first_call, call_nos, result, candidates, winner_cost_duration, clk);
  }
  clk.collect();
  if (s != TOPAY_OK) { c->ps_calls.clear(); return s; }
  return TOPAY_OK;
}

topay_status topay_plan_calls(topay_ctx* c, int n, const int* map_ids, const double* start, const double* end, const double* start_v,
                              const topay_plan_params_t* params, unsigned long long first_call, int* result, int* candidates,
                              double* winner_cost_duration) {
  return plan_calls_impl(c, n, map_ids, start, end, start_v, params, first_call, nullptr, result, candidates, winner_cost_duration);
}

topay_status topay_plan_get_trajs(topay_ctx* c, int n, const int* call_idx, int cap_pieces, int* piece_off, double* durations, double* coeffs,
                                  double* knots_xy) {
  if (!c || n < 0 || (n > 0 && (!call_idx || !piece_off))) return TOPAY_ERR_INVALID_ARG;
  if (c->ps_calls.empty()) { set_err("topay_plan_get_trajs: no planning call has been run"); return TOPAY_ERR_NO_TRAJ; }
  if (n == 0) return TOPAY_OK;
  std::vector<int> off((size_t)n + 1, 0), sp((size_t)n, 0), sk((size_t)n, 0);
  for (int k = 0; k < n; k++) {
    if (call_idx[k] < 0 || call_idx[k] >= (int)c->ps_calls.size()) return TOPAY_ERR_INVALID_ARG;
    const topay_ctx::PlanStored& e = c->ps_calls[call_idx[k]];
    off[k + 1] = off[k] + e.n_pieces;
    sp[k] = e.piece0; sk[k] = e.knot0;
  }
  const int np = off[n];
  memcpy(piece_off, off.data(), ((size_t)n + 1) * sizeof(int));
  if (np > cap_pieces) { set_err("topay_plan_get_trajs: cap_pieces too small for the selection"); return TOPAY_ERR_INVALID_ARG; }
  if (!durations && !coeffs && !knots_xy) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t kn = (size_t)2 * (np + n), dbl = (size_t)np + (size_t)np * kCoefPerPiece + kn;
  int *d_sp, *d_sk, *d_off; double *d_dur, *d_coef, *d_kn;
  auto lay = [&](Carver& k) {
    d_sp = k.take<int>((size_t)n); d_sk = k.take<int>((size_t)n); d_off = k.take<int>((size_t)n + 1);
    d_dur = k.take<double>((size_t)np); d_coef = k.take<double>((size_t)np * kCoefPerPiece); d_kn = k.take<double>(kn);   // (contiguous: one copy back)
  };
  if (topay_status s = c->pb_io.carve(lay); s != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_sp, sp.data(), (size_t)n));
  HIPCHK(h2d(c, d_sk, sk.data(), (size_t)n));
  HIPCHK(h2d(c, d_off, off.data(), (size_t)n + 1));
  HIPCHK(hipMemsetAsync(d_kn, 0, kn * sizeof(double), c->stream));   // a call without a winner still owns one knot pair: zeros
  if (np > 0) {
    hipLaunchKernelGGL(topay::k_plan_store_gather, dim3(n), dim3(64), 0, c->stream, n, (const int*)d_sp, (const int*)d_sk, (const int*)d_off,
                       (const double*)c->ps_dur.as<double>(), (const double*)c->ps_coef.as<double>(), (const double*)c->ps_kn.as<double>(), d_dur, d_coef, d_kn);
    HIPCHK(hipGetLastError());
  }
  std::vector<double> host(dbl);
  HIPCHK(d2h_sync(c, host.data(), d_dur, dbl));
  if (durations) memcpy(durations, host.data(), (size_t)np * 8);
  if (coeffs) memcpy(coeffs, host.data() + np, (size_t)np * kCoefPerPiece * 8);
  if (knots_xy) memcpy(knots_xy, host.data() + np + (size_t)np * kCoefPerPiece, kn * 8);
  return TOPAY_OK;
}

topay_status topay_plan_get_front_path(topay_ctx* c, int call, int cap_states, int* n_states, double* states) {
  if (!c || !n_states || cap_states < 0) return TOPAY_ERR_INVALID_ARG;
  if (c->ps_calls.empty()) { set_err("topay_plan_get_front_path: no planning call has been run"); return TOPAY_ERR_NO_TRAJ; }
  if (call < 0 || call >= (int)c->ps_calls.size()) return TOPAY_ERR_INVALID_ARG;
  const topay_ctx::PlanStored& e = c->ps_calls[call];
  *n_states = e.front_len;
  const int w = std::min(e.front_len, cap_states);
  if (w > 0 && states) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(d2h_sync(c, states, c->ps_front.as<double>() + 10 * (size_t)e.front0, (size_t)w * 10));
  }
  return TOPAY_OK;
}

topay_status topay_plan_test_chunk(topay_ctx* c, int calls) {
  if (!c || calls < 0) return TOPAY_ERR_INVALID_ARG;
  c->pl_chunk = calls;
  return TOPAY_OK;
}

topay_status topay_plan_stage_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  for (int k = 0; k < 8; k++) ms[k] = c->pl_stage_ms[k];
  return TOPAY_OK;
}

}  // extern "C"
