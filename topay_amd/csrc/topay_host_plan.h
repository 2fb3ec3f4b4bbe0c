// Host side of the C-ABI, part 7: topay_plan_calls.  A call is up to two tries; a try (plan_try) is the stages of
// include/topay.h in their order, one function each: per front-end launch the calls, roadmap + JPS, candidate table + dense
// paths, search, hand-off to the solver; then once per try solve + gate + winner, and the winners into the store.  What passes
// between the stages is a PlanTry; every packed device block is a struct that states its layout once.  The buffers and the
// clock's stopwatches are the context's PlanWork, the winners go to its PlanStore (topay_host_ctx.h), which the getters below read.

#pragma once

// ---------------------------------------------------------------------------------------------------------------------
// topay_plan_calls: Planner::planMomaParallel (planner.cpp:792-1061) with every hand-off on the device (topay_plan.h)
// ---------------------------------------------------------------------------------------------------------------------
// Calls per launch of the front-end stages (roadmap, JPS, dense paths, search).  The instance numbers of the draws are
// those of the call, so results do not depend on it; it bounds the roadmap's 1.1 MB per query.  topay_plan_test_chunk sets another.
static const int kPlanChunk = 1024;
static const int kPlanDenseCap = 256;   // entries per dense path kept (the search takes at most 255 layers)
static const int kPlanJpsCap = 512;     // points per JPS path kept

// Rows of the caller's tables (include/topay.h: TOPAY_PLAN_RES_*, TOPAY_PLAN_CAND_*).
static int* result_row(int* result, int p) { return result + TOPAY_PLAN_RES_LEN * (size_t)p; }
static int* cand_row(int* cand, int p, int t, int k) { return cand + (((size_t)p * 2 + t) * TOPAY_PLAN_MAX_CAND + k) * TOPAY_PLAN_CAND_LEN; }

// Device time of one stage (TOPAY_PLAN_MS_*): a stopwatch around its launches on the context's stream, read once the call has
// finished.  A stage is timed once per launch of a call, so the stopwatches are taken in turn from PlanWork and their times
// summed by stage; one whose stop was never recorded (an error return between begin and end) is not read.
struct PlanClock {
  topay_ctx* c;
  PlanWork& w;
  size_t used = 0;
  explicit PlanClock(topay_ctx* c_) : c(c_), w(c_->plan) {}
  DevTimer* reserve(int stage) {   // for a launcher that starts and stops it itself, around its kernels only
    if (used == w.timers.size()) { w.timers.emplace_back(); w.timer_stage.push_back(0); }
    w.timer_stage[used] = stage;
    w.timers[used].stopped = false;
    return &w.timers[used++];
  }
  DevTimer* begin(int stage) { DevTimer* t = reserve(stage); (void)t->start(c->stream); return t; }
  void end(DevTimer* t) { (void)t->stop(c->stream); }
  void collect() {
    (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i < used; i++) {
      double ms = 0.0;
      if (w.timers[i].read(&ms) == hipSuccess) w.stage_ms[w.timer_stage[i]] += ms;
    }
  }
};

// The planning call as plan_calls_impl checked it: the caller's arrays and tables.  Call p has the number call_nos[p], or
// first_call + p when call_nos is null (the replanning cycle numbers its calls itself).
struct PlanReq {
  topay_plan_params_t P;
  std::vector<int> mids;
  const double *start, *end, *start_v; unsigned long long first_call; const unsigned long long* call_nos;
  int *result, *cand;   // n x TOPAY_PLAN_RES_LEN; n x TOPAY_PLAN_CAND_ROW_LEN or null
  double* wcd;          // n x 2 or null
  unsigned long long number(int p) const { return call_nos ? call_nos[p] : first_call + (unsigned long long)p; }
};

// ---- the packed device blocks of a try
struct PlanCallBlock {   // the launch's calls as the caller gave them: PlanWork::io
  size_t n = 0;
  double *start, *end, *start_v; unsigned long long* call_no; int* mid;   // (the states: 10 per call)
  void lay(Carver& k) {
    start = k.take<double>(10 * n); end = k.take<double>(10 * n); start_v = k.take<double>(10 * n);
    call_no = k.take<unsigned long long>(n); mid = k.take<int>(n);
  }
};
struct PlanCandBlock {   // candidate table (slot = call x TOPAY_PLAN_MAX_CAND + k) and the dense paths of its slots: PlanWork::tab
  size_t n = 0;          // calls
  double *syaw, *eyaw, *dense; long long* raw_off; int *ncand, *raw_len, *dense_len;
  void lay(Carver& k) {
    const size_t ns = n * TOPAY_PLAN_MAX_CAND;
    syaw = k.take<double>(ns); eyaw = k.take<double>(ns); raw_off = k.take<long long>(ns); dense = k.take<double>(ns * kPlanDenseCap * 4);
    ncand = k.take<int>(n); raw_len = k.take<int>(ns); dense_len = k.take<int>(ns);
  }
};
struct PlanSearchBlock {   // per search instance: the inputs k_plan_pack_search writes for k_mcrrt, and its outputs: PlanWork::mc
  size_t n = 0;
  int layer_cap = 2;       // states per whole-body path kept
  long long* off; unsigned long long* inst; double *start, *end, *wb, *cmax; int *slot, *len, *mid, *wb_len, *stats;
  void lay(Carver& k) {
    off = k.take<long long>(n); inst = k.take<unsigned long long>(n);
    start = k.take<double>(10 * n); end = k.take<double>(10 * n); wb = k.take<double>(n * layer_cap * 10); cmax = k.take<double>(n);
    slot = k.take<int>(n); len = k.take<int>(n); mid = k.take<int>(n); wb_len = k.take<int>(n); stats = k.take<int>(8 * n);
  }
};
struct PlanHandoffBlock {   // per survivor of the launch: first state of its init path, its search instance, its call in the launch: PlanWork::idx
  size_t n = 0;
  long long* path_off; int *src, *src_call;
  void lay(Carver& k) { path_off = k.take<long long>(n); src = k.take<int>(n); src_call = k.take<int>(n); }
};
struct PlanWinnerBlock {   // per call of the solved batch its candidates' range, winner, cost and duration; per candidate its stage: PlanWork::win
  size_t calls = 0, batch = 0;
  double* wcd; int *first, *count, *win, *stage;
  void lay(Carver& k) {
    wcd = k.take<double>(2 * calls);
    first = k.take<int>(calls); count = k.take<int>(calls); win = k.take<int>(calls); stage = k.take<int>(batch);
  }
};
struct PlanStoreIdxBlock {   // per winner its index in the batch, and the running piece / state offsets (PlanStore::Winners): PlanWork::idx
  size_t n = 0;
  int *idx, *piece_off, *front_off;
  void lay(Carver& k) { idx = k.take<int>(n); piece_off = k.take<int>(n + 1); front_off = k.take<int>(n + 1); }
};

// One try (t = 0 plain, 1 critical) for the calls `act`: what passes between its stages.
struct PlanTry {
  topay_ctx* c; PlanReq& R; const int t; const std::vector<int>& act; PlanClock& clk;
  // the survivors over all front-end launches: the batch that is solved
  std::vector<int> call, k, len, mid;
  std::vector<long long> off{0};
  // the front-end launch under way: calls act[a0 .. a0 + nc); the host arrays live until the launch's last wait
  size_t a0 = 0, topo_pts = 0;
  int nc = 0, cap_points = 2;
  std::vector<double> sxy, exy, st10, en10, sv10;
  std::vector<int> cmid, crit;
  std::vector<unsigned long long> inst, call_no;
  TopoDev td; JpsDev jd;   // where the roadmap and JPS left their results
  std::vector<int> sel;    // the candidate slots that are searched
  PlanCallBlock in; PlanCandBlock tab; PlanSearchBlock mc;
  int p_of(int q) const { return act[a0 + (size_t)q]; }
};

// ---- the launch's calls: inputs of the caller, gathered on the host
static topay_status plan_gather_calls(PlanTry& T) {
  topay_ctx* c = T.c;
  const PlanReq& R = T.R;
  const size_t NC = (size_t)T.nc;
  T.sxy.assign(2 * NC, 0.0); T.exy.assign(2 * NC, 0.0); T.st10.assign(10 * NC, 0.0); T.en10.assign(10 * NC, 0.0); T.sv10.assign(10 * NC, 0.0);
  T.cmid.assign(NC, 0); T.crit.assign(NC, T.t); T.inst.assign(NC, 0); T.call_no.assign(NC, 0);
  T.cap_points = 2;
  for (int q = 0; q < T.nc; q++) {
    const int p = T.p_of(q);
    const size_t q10 = 10 * (size_t)q, p10 = 10 * (size_t)p;
    memcpy(&T.st10[q10], R.start + p10, 80);
    memcpy(&T.en10[q10], R.end + p10, 80);
    if (R.start_v) memcpy(&T.sv10[q10], R.start_v + p10, 80);
    T.sxy[2 * (size_t)q] = R.start[p10]; T.sxy[2 * (size_t)q + 1] = R.start[p10 + 1];
    T.exy[2 * (size_t)q] = R.end[p10]; T.exy[2 * (size_t)q + 1] = R.end[p10 + 1];
    T.cmid[q] = R.mids[p];
    T.call_no[q] = R.number(p);
    T.inst[q] = 2ull * T.call_no[q] + (unsigned long long)T.t;
    const DevMap& m = c->hmaps[T.cmid[q]];
    T.cap_points = std::max(T.cap_points, topo_pt_cap(m.dims[0], m.dims[1]));   // no selected path has more points than its map's cap
  }
  T.topo_pts = NC * (size_t)R.P.topo.reserve_num * T.cap_points;
  topay_status s;
  if ((s = c->plan.raw.ensure((T.topo_pts + NC * kPlanJpsCap) * 16)) != TOPAY_OK) return s;
  T.in.n = NC;
  if ((s = c->plan.io.place(T.in)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, T.in.start, T.st10.data(), 10 * NC));
  HIPCHK(h2d(c, T.in.end, T.en10.data(), 10 * NC));
  HIPCHK(h2d(c, T.in.start_v, T.sv10.data(), 10 * NC));
  HIPCHK(h2d(c, T.in.call_no, T.call_no.data(), NC));
  HIPCHK(h2d(c, T.in.mid, T.cmid.data(), NC));
  return TOPAY_OK;
}

// ---- roadmap, JPS (the launchers record around their kernels: uploads, allocations and waits stay outside)
static topay_status plan_roadmap_jps(PlanTry& T) {
  topay_ctx* c = T.c;
  const topay_plan_params_t& P = T.R.P;
  double* raw = c->plan.raw.as<double>();
  topay_status s = topo_impl(c, T.nc, T.cmid.data(), T.sxy.data(), T.exy.data(), T.crit.data(), &P.topo, 0, T.inst.data(), P.topo.reserve_num, T.cap_points, raw,
                             false, &T.td, T.clk.reserve(TOPAY_PLAN_MS_ROADMAP));
  if (s != TOPAY_OK) return s;
  T.jd.len = nullptr;
  if (T.t == 0)   // (the second try has no JPS candidate)
    s = jps_impl(c, T.nc, T.cmid.data(), T.sxy.data(), T.exy.data(), c->hp.chassis_colli_radius + P.jps_margin, kPlanJpsCap, c->plan.jps_io, raw + 2 * T.topo_pts,
                 &T.jd, "topay_plan_calls", T.clk.reserve(TOPAY_PLAN_MS_JPS));
  return s;
}

// ---- candidate table, dense paths; the calls' counts into `result`, the slots that go on into T.sel
static topay_status plan_candidates(PlanTry& T) {
  topay_ctx* c = T.c;
  const PlanReq& R = T.R;
  const size_t NC = (size_t)T.nc, NS = NC * TOPAY_PLAN_MAX_CAND;
  topay_status s;
  T.tab.n = NC;
  if ((s = c->plan.tab.place(T.tab)) != TOPAY_OK) return s;
  topay::PlanCandArgs A;
  A.n = T.nc; A.cap_paths = R.P.topo.reserve_num; A.cap_points = T.cap_points; A.jps_cap = kPlanJpsCap; A.max_cand = R.P.max_candidates;
  A.jps_base = (long long)T.topo_pts;
  A.topo_np = T.td.n_paths; A.topo_len = T.td.path_len; A.jps_len = T.jd.len; A.start = T.in.start; A.end = T.in.end;
  A.ncand = T.tab.ncand; A.raw_off = T.tab.raw_off; A.raw_len = T.tab.raw_len; A.syaw = T.tab.syaw; A.eyaw = T.tab.eyaw;
  DevTimer* ev = T.clk.begin(TOPAY_PLAN_MS_DENSE);
  hipLaunchKernelGGL(topay::k_plan_candidates, dim3((T.nc + 63) / 64), dim3(64), 0, c->stream, A);
  HIPCHK(hipGetLastError());
  if ((s = dense_launch(c, (int)NS, c->plan.raw.as<double>(), T.tab.raw_off, T.tab.raw_len, R.P.dense_step, T.tab.syaw, T.tab.eyaw, c->hp.max_v, c->hp.max_w,
                        kPlanDenseCap, T.tab.dense, T.tab.dense_len)) != TOPAY_OK)
    return s;
  T.clk.end(ev);
  std::vector<int> ncand(NC), dlen(NS), tstat(NC * 8);
  HIPCHK(d2h(c, ncand.data(), T.tab.ncand, NC));
  HIPCHK(d2h(c, dlen.data(), T.tab.dense_len, NS));
  HIPCHK(d2h(c, tstat.data(), T.td.stats, NC * 8));
  HIPCHK(hipStreamSynchronize(c->stream));
  T.sel.clear();
  T.mc.layer_cap = 2;
  for (int q = 0; q < T.nc; q++) {
    const int p = T.p_of(q);
    int* r = result_row(R.result, p);
    r[TOPAY_PLAN_RES_TRY] = T.t;
    r[TOPAY_PLAN_RES_CANDIDATES0 + T.t] = std::abs(ncand[q]);
    r[TOPAY_PLAN_RES_TOPO_STATUS] = tstat[8 * (size_t)q];
    if (ncand[q] < 0) { r[TOPAY_PLAN_RES_STATUS] = -3; continue; }
    for (int k = 0; k < ncand[q]; k++) {
      const int sl = q * TOPAY_PLAN_MAX_CAND + k;
      T.sel.push_back(sl);
      T.mc.layer_cap = std::max(T.mc.layer_cap, std::min(dlen[sl], 255));
      if (R.cand) cand_row(R.cand, p, T.t, k)[TOPAY_PLAN_CAND_STAGE] = TOPAY_PLAN_STAGE_SEARCH_FAILED;   // until it gets further
    }
  }
  return TOPAY_OK;
}

// ---- the search: hand-off kernel, k_mcrrt; the lengths and statuses of the whole-body paths come back
static topay_status plan_search(PlanTry& T, std::vector<int>& wlen, std::vector<int>& mstat) {
  topay_ctx* c = T.c;
  const int ni = (int)T.sel.size();
  const size_t NI = (size_t)ni;
  PlanSearchBlock& M = T.mc;
  topay_status s;
  M.n = NI;
  if ((s = c->plan.mc.place(M)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, M.slot, T.sel.data(), NI));
  DevTimer* ev = T.clk.begin(TOPAY_PLAN_MS_SEARCH);
  hipLaunchKernelGGL(topay::k_plan_pack_search, dim3((ni + 63) / 64), dim3(64), 0, c->stream, ni, (const int*)M.slot, kPlanDenseCap, (const int*)T.tab.dense_len,
                     (const double*)T.in.start, (const double*)T.in.end, (const int*)T.in.mid, (const unsigned long long*)T.in.call_no, T.t, M.off, M.len, M.start,
                     M.end, M.mid, M.inst);
  HIPCHK(hipGetLastError());
  McIo io;
  io.off = M.off; io.len = M.len; io.car = T.tab.dense; io.start = M.start; io.end = M.end; io.mid = M.mid; io.inst = M.inst;
  io.wb_len = M.wb_len; io.wb = M.wb; io.stats = M.stats; io.cmax = M.cmax;
  if ((s = mcrrt_launch(c, ni, T.R.P.mcrrt, 0, M.layer_cap, io)) != TOPAY_OK) return s;
  T.clk.end(ev);
  wlen.resize(NI); mstat.resize(NI * 8);
  HIPCHK(d2h(c, wlen.data(), M.wb_len, NI));
  HIPCHK(d2h(c, mstat.data(), M.stats, 8 * NI));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

// ---- hand-off to the solver: the launch's survivors join the try's batch; their ragged init paths and boundary velocities
// are appended to the try's, launch by launch
static topay_status plan_handoff(PlanTry& T, const std::vector<int>& wlen, const std::vector<int>& mstat) {
  topay_ctx* c = T.c;
  std::vector<int> src, src_call;
  std::vector<long long> poff;
  const int b0 = (int)T.call.size();
  for (int i = 0; i < (int)T.sel.size(); i++) {
    const int q = T.sel[i] / TOPAY_PLAN_MAX_CAND, k = T.sel[i] % TOPAY_PLAN_MAX_CAND, p = T.p_of(q);
    if (T.R.cand) cand_row(T.R.cand, p, T.t, k)[TOPAY_PLAN_CAND_SEARCH_STATUS] = mstat[8 * (size_t)i];
    if (mstat[8 * (size_t)i] != 1 || wlen[i] < 2) continue;
    src.push_back(i);
    src_call.push_back(q);
    poff.push_back(T.off.back());
    T.call.push_back(p); T.k.push_back(k); T.len.push_back(wlen[i]); T.mid.push_back(T.R.mids[p]);
    T.off.push_back(T.off.back() + wlen[i]);
  }
  const int nsv = (int)src.size();
  if (nsv == 0) return TOPAY_OK;
  topay_status s;
  if ((s = c->plan.paths.ensure_keep(c->stream, (size_t)T.off.back() * 80, (size_t)poff[0] * 80)) != TOPAY_OK) return s;
  if ((s = c->plan.bvel.ensure_keep(c->stream, T.call.size() * 160, (size_t)b0 * 160)) != TOPAY_OK) return s;
  PlanHandoffBlock H;
  H.n = (size_t)nsv;
  if ((s = c->plan.idx.place(H)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, H.path_off, poff.data(), H.n));
  HIPCHK(h2d(c, H.src, src.data(), H.n));
  HIPCHK(h2d(c, H.src_call, src_call.data(), H.n));
  DevTimer* ev = T.clk.begin(TOPAY_PLAN_MS_INIT);
  hipLaunchKernelGGL(topay::k_plan_pack_solver, dim3((unsigned)nsv), dim3(64), 0, c->stream, nsv, (const int*)H.src, (const int*)H.src_call, T.mc.layer_cap,
                     (const int*)T.mc.wb_len, (const double*)T.mc.wb, (const long long*)H.path_off, (const double*)T.in.start_v, b0, c->plan.paths.as<double>(),
                     c->plan.bvel.as<double>());
  HIPCHK(hipGetLastError());
  T.clk.end(ev);
  HIPCHK(hipStreamSynchronize(c->stream));   // (the launch's buffers are reused by the next one)
  return TOPAY_OK;
}

// ---- one batch: init, groups, solve, gate; then per call one lane over its candidates (adjacent in the batch, in candidate
// order) for the winner.  Fills the candidates' rows and the winners' rows of `result` / `wcd`; W = the winners for the store.
static topay_status plan_solve(PlanTry& T, PlanStore::Winners& W) {
  topay_ctx* c = T.c;
  const PlanReq& R = T.R;
  const int B = (int)T.call.size(), t = T.t;
  DevTimer* ev = T.clk.begin(TOPAY_PLAN_MS_INIT);
  topay_status s = set_init_traj_impl(c, B, T.len.data(), c->plan.paths.as<double>(), c->plan.bvel.as<double>(), nullptr, T.mid.data(), hipMemcpyDeviceToDevice);
  T.clk.end(ev);
  if (s == TOPAY_ERR_TOO_MANY_PIECES) {   // every candidate needs more pieces than the build solves
    if (R.cand)
      for (int b = 0; b < B; b++) cand_row(R.cand, T.call[b], t, T.k[b])[TOPAY_PLAN_CAND_STAGE] = TOPAY_PLAN_STAGE_TOO_MANY_PIECES;
    return TOPAY_OK;
  }
  if (s != TOPAY_OK) return s;
  if ((s = topay_set_groups(c, T.call.data(), R.P.cancel_budget)) != TOPAY_OK) return s;
  if ((s = topay_optimize(c)) != TOPAY_OK) return s;
  c->plan.stage_ms[TOPAY_PLAN_MS_SOLVE] += c->last_ms;
  std::vector<int> feas(B);
  ev = T.clk.begin(TOPAY_PLAN_MS_GATE_WINNER);
  if ((s = topay_check_feasible(c, feas.data())) != TOPAY_OK) return s;
  std::vector<int> qcall, first, count;
  for (int b = 0; b < B; b++) {
    if (qcall.empty() || qcall.back() != T.call[b]) { qcall.push_back(T.call[b]); first.push_back(b); count.push_back(0); }
    count.back()++;
  }
  const int Q = (int)qcall.size();
  PlanWinnerBlock D;
  D.calls = (size_t)Q; D.batch = (size_t)B;
  if ((s = c->plan.win.place(D)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, D.first, first.data(), D.calls));
  HIPCHK(h2d(c, D.count, count.data(), D.calls));
  hipLaunchKernelGGL(topay::k_plan_winner, dim3((Q + 63) / 64), dim3(64), 0, c->stream, c->db, Q, (const int*)D.first, (const int*)D.count, D.stage, D.win, D.wcd);
  HIPCHK(hipGetLastError());
  T.clk.end(ev);
  std::vector<int> win(Q), stage(B), sst((size_t)B * kStatsLen);
  std::vector<double> hw(2 * D.calls);
  HIPCHK(d2h(c, win.data(), D.win, D.calls));
  HIPCHK(d2h(c, stage.data(), D.stage, D.batch));
  HIPCHK(d2h(c, hw.data(), D.wcd, 2 * D.calls));
  HIPCHK(d2h(c, sst.data(), c->stats.as<int>(), sst.size()));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (R.cand)
    for (int b = 0; b < B; b++) {
      int* e = cand_row(R.cand, T.call[b], t, T.k[b]);
      e[TOPAY_PLAN_CAND_STAGE] = stage[b];
      e[TOPAY_PLAN_CAND_N_PIECES] = c->hN[b];
      e[TOPAY_PLAN_CAND_SOLVER_STATUS] = c->hN[b] > 0 ? sst[(size_t)b * kStatsLen + 3] : 0;
    }
  for (int q = 0; q < Q; q++) {
    if (win[q] < 0) continue;
    const int p = qcall[q], b = win[q];
    int* r = result_row(R.result, p);
    r[TOPAY_PLAN_RES_STATUS] = 1; r[TOPAY_PLAN_RES_TRY] = t; r[TOPAY_PLAN_RES_WINNER] = T.k[b]; r[TOPAY_PLAN_RES_N_PIECES] = c->hN[b];
    r[TOPAY_PLAN_RES_WINNER_BATCH_INDEX] = b;
    if (R.wcd) { R.wcd[2 * (size_t)p] = hw[2 * (size_t)q]; R.wcd[2 * (size_t)p + 1] = hw[2 * (size_t)q + 1]; }
    W.add(p, b, c->hN[b], T.len[b]);
  }
  return TOPAY_OK;
}

// ---- the winners into the store: trajectories in the layout of k_gather_results, init paths after them
static topay_status plan_store_winners(PlanTry& T, const PlanStore::Winners& W) {
  topay_ctx* c = T.c;
  const int nw = (int)W.size();
  topay_status s;
  PlanStore::Dest dst;
  if ((s = c->plan_store.reserve(c->stream, W, dst)) != TOPAY_OK) return s;
  PlanStoreIdxBlock I;
  I.n = W.size();
  if ((s = c->plan.idx.place(I)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, I.idx, W.idx.data(), I.n));
  HIPCHK(h2d(c, I.piece_off, W.piece_off.data(), I.n + 1));
  HIPCHK(h2d(c, I.front_off, W.front_off.data(), I.n + 1));
  DevTimer* ev = T.clk.begin(TOPAY_PLAN_MS_STORE);
  hipLaunchKernelGGL(k_gather_results, dim3(nw), dim3(64), 0, c->stream, c->db, nw, (const int*)I.idx, (const int*)I.piece_off, dst.dur, dst.coef, dst.knots);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(topay::k_plan_gather_front, dim3(nw), dim3(64), 0, c->stream, nw, (const int*)I.idx, (const double*)c->paths.as<double>(),
                     (const long long*)c->path_off.as<long long>(), (const int*)I.front_off, dst.front);
  HIPCHK(hipGetLastError());
  T.clk.end(ev);
  HIPCHK(hipStreamSynchronize(c->stream));
  c->plan_store.appended(W);
  return TOPAY_OK;
}

// One try for the calls `act`: the front-end in launches of kPlanChunk calls, one solve, winners into the store.  Fills the
// calls' rows of R.result / R.cand / R.wcd.
static topay_status plan_try(topay_ctx* c, int t, const std::vector<int>& act, PlanReq& R, PlanClock& clk) {
  topay_status s;
  PlanTry T{c, R, t, act, clk};
  const size_t chunk = (size_t)(c->plan.chunk > 0 ? c->plan.chunk : kPlanChunk);
  std::vector<int> wlen, mstat;
  for (T.a0 = 0; T.a0 < act.size(); T.a0 += chunk) {
    T.nc = (int)std::min<size_t>(chunk, act.size() - T.a0);
    if ((s = plan_gather_calls(T)) != TOPAY_OK || (s = plan_roadmap_jps(T)) != TOPAY_OK || (s = plan_candidates(T)) != TOPAY_OK) return s;
    if (T.sel.empty()) continue;
    if ((s = plan_search(T, wlen, mstat)) != TOPAY_OK || (s = plan_handoff(T, wlen, mstat)) != TOPAY_OK) return s;
  }
  if (T.call.empty()) return TOPAY_OK;   // no candidate of any call survived to the solve: the try fails for all of them
  PlanStore::Winners W;
  if ((s = plan_solve(T, W)) != TOPAY_OK || W.size() == 0) return s;
  return plan_store_winners(T, W);
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
  PlanReq R;
  R.start = start; R.end = end; R.start_v = start_v; R.first_call = first_call; R.call_nos = call_nos;
  R.result = result; R.cand = candidates; R.wcd = winner_cost_duration;
  topay_plan_params_t& P = R.P;
  if (params) P = *params;
  else topay_plan_default_params(&P);
  if (P.max_candidates < 1 || P.max_candidates > TOPAY_PLAN_MAX_CAND || !(P.dense_step > 0.0) || P.cancel_budget < 0 || !mcrrt_params_ok(P.mcrrt) ||
      P.topo.reserve_num < 1 || P.topo.reserve_num > 16) {
    set_err("topay_plan_calls: parameters out of range (max_candidates 1..8, dense_step > 0, cancel_budget >= 0)");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (topay_status cs = check_map_slots(c, n, map_ids, kMapResident | kMapFront, "topay_plan_calls")) return cs;
  R.mids.assign((size_t)n, 0);
  if (map_ids) R.mids.assign(map_ids, map_ids + n);
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  c->plan_store.reset(n);
  for (int k = 0; k < TOPAY_PLAN_MS_LEN; k++) c->plan.stage_ms[k] = 0.0;
  for (int p = 0; p < n; p++) {
    int* r = result_row(result, p);
    std::fill(r, r + TOPAY_PLAN_RES_LEN, 0);
    r[TOPAY_PLAN_RES_TRY] = r[TOPAY_PLAN_RES_WINNER] = r[TOPAY_PLAN_RES_WINNER_BATCH_INDEX] = -1;
    if (winner_cost_duration) winner_cost_duration[2 * (size_t)p] = winner_cost_duration[2 * (size_t)p + 1] = 0.0 / 0.0;
  }
  if (candidates) memset(candidates, 0, (size_t)n * TOPAY_PLAN_CAND_ROW_LEN * sizeof(int));
  PlanClock clk(c);
  topay_status s = TOPAY_OK;
  for (int t = 0; t < 2 && s == TOPAY_OK; t++) {
    if (t == 1 && !P.critical_retry) break;
    std::vector<int> act;
    for (int p = 0; p < n; p++)
      if (result_row(result, p)[TOPAY_PLAN_RES_STATUS] == 0) act.push_back(p);
    if (act.empty()) break;
    s = plan_try(c, t, act, R, clk);
  }
  clk.collect();
  if (s != TOPAY_OK) { c->plan_store.clear(); return s; }
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
  PlanStore& S = c->plan_store;
  if (S.empty()) { set_err("topay_plan_get_trajs: no planning call has been run"); return TOPAY_ERR_NO_TRAJ; }
  if (n == 0) return TOPAY_OK;
  std::vector<int> off((size_t)n + 1, 0), sp((size_t)n, 0), sk((size_t)n, 0);
  for (int k = 0; k < n; k++) {
    if (!S.has(call_idx[k])) return TOPAY_ERR_INVALID_ARG;
    const PlanStore::Entry& e = S.entry(call_idx[k]);
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
                       (const double*)S.durations(), (const double*)S.coeffs(), (const double*)S.knots(), d_dur, d_coef, d_kn);
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
  PlanStore& S = c->plan_store;
  if (S.empty()) { set_err("topay_plan_get_front_path: no planning call has been run"); return TOPAY_ERR_NO_TRAJ; }
  if (!S.has(call)) return TOPAY_ERR_INVALID_ARG;
  const PlanStore::Entry& e = S.entry(call);
  *n_states = e.front_len;
  const int w = std::min(e.front_len, cap_states);
  if (w > 0 && states) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(d2h_sync(c, states, S.fronts() + PlanStore::front_double0(e), (size_t)w * 10));
  }
  return TOPAY_OK;
}

topay_status topay_plan_test_chunk(topay_ctx* c, int calls) {
  if (!c || calls < 0) return TOPAY_ERR_INVALID_ARG;
  c->plan.chunk = calls;
  return TOPAY_OK;
}

topay_status topay_plan_stage_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  for (int k = 0; k < TOPAY_PLAN_MS_LEN; k++) ms[k] = c->plan.stage_ms[k];
  return TOPAY_OK;
}

}  // extern "C"
