// Host side of the C-ABI, part 3: the resident batch -- upload and initial guess, launch classes, optimise and synchronise,
// planning-call groups and cancellation.

#pragma once

static topay_status run_init(topay_ctx* c) {
  const int B = c->B;
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  const int scratch_stride = (3 * c->Pmax + 1 + TOPAY_MAX_N) * ND;
  hipLaunchKernelGGL(k_init, dim3((B + 63) / 64), dim3(64), 0, c->stream, c->db, c->paths.as<double>(),
                     c->path_off.as<long long>(), c->path_len.as<int>(), c->bvel.as<double>(), c->bacc.as<double>(),
                     c->scratch.as<double>(), scratch_stride, TOPAY_MAX_N, kX0Stride);
  HIPCHK(hipGetLastError());
  return TOPAY_OK;
}

// topay_set_init_traj with the init paths and the boundary velocities where `kind` says they are: in host memory (the
// public entry) or already on the device (topay_plan_calls: the whole-body paths the search left there).  Lengths and map
// slots are host data either way: they size the workspace.
static topay_status set_init_traj_impl(topay_ctx* c, int batch, const int* path_len, const double* init_paths, const double* boundary_vel,
                                       const double* boundary_acc, const int* map_ids, hipMemcpyKind kind) {
  if (!c || batch <= 0 || !path_len || !init_paths) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  c->have_traj = false;
  c->solved = false;
  std::vector<long long> off(batch + 1, 0);
  int Pmax = 0;
  for (int b = 0; b < batch; b++) {
    if (path_len[b] < 2) { set_err("every init path needs at least 2 states"); return TOPAY_ERR_INVALID_ARG; }
    off[b + 1] = off[b] + path_len[b];
    Pmax = std::max(Pmax, path_len[b]);
  }
  if (check_map_slots(c, batch, map_ids, kMapResident, "topay_set_init_traj") != TOPAY_OK) return TOPAY_ERR_NO_MAP;   // (out of range too)
  std::vector<int> mids(batch, 0);
  if (map_ids) mids.assign(map_ids, map_ids + batch);
  c->B = batch;
  c->Pmax = Pmax;
  c->h_map_id = mids;
  const size_t tot = (size_t)off[batch];
  topay_status s;
#define ENS(buf, bytes) if ((s = c->buf.ensure(bytes)) != TOPAY_OK) return s
  ENS(paths, tot * 10 * 8);
  ENS(path_off, (size_t)(batch + 1) * 8);
  ENS(path_len, (size_t)batch * 4);
  ENS(bvel, (size_t)batch * 20 * 8);
  ENS(bacc, (size_t)batch * 20 * 8);
  ENS(scratch, (size_t)batch * (3 * Pmax + 1 + TOPAY_MAX_N) * ND * 8);
  ENS(N, (size_t)batch * 4);
  ENS(s1_past, (size_t)batch * 4);
  ENS(map_id, (size_t)batch * 4);
  ENS(head, (size_t)batch * kHeadLen * 8);
  ENS(tail, (size_t)batch * kHeadLen * 8);
  ENS(start_xy, (size_t)batch * 2 * 8);
  ENS(goal_xy, (size_t)batch * 2 * 8);
  ENS(init_xy, (size_t)batch * kInitXyStride * 8);
  ENS(x0, (size_t)batch * kX0Stride * 8);
  ENS(order, (size_t)batch * 4);
  HIPCHK(copy_sync(c, c->paths.as<double>(), init_paths, tot * 10, kind));
  HIPCHK(h2d_sync(c, c->path_off.as<long long>(), off.data(), (size_t)(batch + 1)));
  HIPCHK(h2d_sync(c, c->path_len.as<int>(), path_len, (size_t)batch));
  HIPCHK(h2d_sync(c, c->map_id.as<int>(), mids.data(), (size_t)batch));
  if (boundary_vel) HIPCHK(copy_sync(c, c->bvel.as<double>(), boundary_vel, (size_t)batch * 20, kind));
  else HIPCHK(hipMemsetAsync(c->bvel.p, 0, (size_t)batch * 20 * 8, c->stream));
  if (boundary_acc) HIPCHK(h2d_sync(c, c->bacc.as<double>(), boundary_acc, (size_t)batch * 20));
  else HIPCHK(hipMemsetAsync(c->bacc.p, 0, (size_t)batch * 20 * 8, c->stream));
  DevBatch& d = c->db;
  memset(&d, 0, sizeof(d));
  d.B = batch;
  d.N = c->N.as<int>(); d.s1_past = c->s1_past.as<int>(); d.map_id = c->map_id.as<int>();
  d.head = c->head.as<double>(); d.tail = c->tail.as<double>();
  d.start_xy = c->start_xy.as<double>(); d.goal_xy = c->goal_xy.as<double>();
  d.init_xy = c->init_xy.as<double>(); d.x0 = c->x0.as<double>();
  d.order = c->order.as<int>();
  if ((s = run_init(c)) != TOPAY_OK) return s;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->hN.assign(batch, 0);
  HIPCHK(d2h_sync(c, c->hN.data(), c->N.as<int>(), (size_t)batch));
  int Nmax = 0;
  for (int b = 0; b < batch; b++) {
    if (c->hN[b] <= 0) c->hN[b] = 0;  // needs more than TOPAY_MAX_N pieces: reported as failed, never launched
    Nmax = std::max(Nmax, c->hN[b]);
  }
  if (Nmax == 0) { set_err("every trajectory needs more pieces than TOPAY_MAX_N"); return TOPAY_ERR_TOO_MANY_PIECES; }
  c->Nmax = Nmax;
  c->h_poff.assign((size_t)batch + 1, 0);
  c->h_noff.assign((size_t)batch + 1, 0);
  for (int b = 0; b < batch; b++) {
    c->h_poff[b + 1] = c->h_poff[b] + c->hN[b];
    c->h_noff[b + 1] = c->h_noff[b] + (c->hN[b] > 0 ? 10 * c->hN[b] - 8 : 0);
  }
  const size_t P = (size_t)c->h_poff[batch], NN = (size_t)c->h_noff[batch];
  const int m = std::max(c->hp.s1_lbfgs.mem_size, c->hp.s2_lbfgs.mem_size);
  // launch order: longest trajectories first inside each row class (tail latency)
  std::vector<int> idx(batch);
  std::iota(idx.begin(), idx.end(), 0);
  // more pieces first, then more path states (both correlate ~0.45 with the number of evaluations a candidate needs)
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b2) {
    return c->hN[a] != c->hN[b2] ? c->hN[a] > c->hN[b2] : path_len[a] > path_len[b2];
  });
  for (auto& v : c->cls) v.clear();
  for (int b : idx) {
    if (c->hN[b] == 0) continue;
    c->cls[bucket_of(c->hN[b])].push_back(b);
  }
  c->h_path_len.assign(path_len, path_len + batch);
  {
    std::vector<int> ord;
    for (int k = topay_ctx::NBUCKET - 1; k >= 0; k--) ord.insert(ord.end(), c->cls[k].begin(), c->cls[k].end());
    ord.resize(batch, 0);
    HIPCHK(h2d_sync(c, c->order.as<int>(), ord.data(), (size_t)batch));
  }
  ENS(poff, ((size_t)batch + 1) * 8);
  ENS(noff, ((size_t)batch + 1) * 8);
  HIPCHK(h2d_sync(c, c->poff.as<long long>(), c->h_poff.data(), ((size_t)batch + 1)));
  HIPCHK(h2d_sync(c, c->noff.as<long long>(), c->h_noff.data(), ((size_t)batch + 1)));
  // every block sized by the candidates' own pieces / decision vectors (the history, 2 m n doubles per candidate, is
  // by far the largest: 0.4 MB at the benchmark's mean of 11 pieces, 7 MB at 170)
  ENS(x, NN * 8);
  ENS(work, 4 * NN * 8);
  ENS(hist_s, (size_t)m * NN * 8);
  ENS(hist_y, (size_t)m * NN * 8);
  ENS(hist_ys, (size_t)batch * m * 8);
  ENS(hist_alpha, (size_t)batch * m * 8);
  ENS(lu, kLuPerPiece * P * 8);
  ENS(success, (size_t)batch * 4);
  ENS(cost, (size_t)batch * 8);
  ENS(stats, (size_t)batch * kStatsLen * 4);
  ENS(xyerr, (size_t)batch * 2 * 8);
  ENS(coef, kCoefPerPiece * P * 8);
  ENS(T, P * 8);
  ENS(knots, 2 * (P + batch) * 8);
  ENS(alm, (size_t)batch * kAlmLen * 8);
  ENS(fout, (size_t)batch * 8);
  ENS(sbuf, kSbufPerPiece * P * 8);
  ENS(mstash, kMstashPerPiece * P * 8);
  ENS(elapsed, (size_t)batch * 8);
  ENS(startus, (size_t)batch * 8);
  ENS(hwid, (size_t)batch * 4);
  ENS(feas_flags, (size_t)batch * 2 * 4);
  ENS(feas_report, (size_t)batch * kReportLen * 8);
  ENS(interrupted, (size_t)batch * 4);
#undef ENS
  {
    DevBuf* all[] = {&c->paths, &c->path_off, &c->path_len, &c->bvel, &c->bacc, &c->scratch, &c->N, &c->s1_past, &c->map_id, &c->head, &c->tail,
                     &c->start_xy, &c->goal_xy, &c->init_xy, &c->x0, &c->order, &c->poff, &c->noff, &c->x, &c->work, &c->hist_s, &c->hist_y,
                     &c->hist_ys, &c->hist_alpha, &c->lu, &c->success, &c->cost, &c->stats, &c->xyerr, &c->coef, &c->T, &c->knots, &c->alm,
                     &c->fout, &c->sbuf, &c->mstash, &c->elapsed, &c->startus, &c->hwid};
    c->workspace_bytes = 0;
    for (DevBuf* q : all) c->workspace_bytes += q->bytes;
  }
  d.hist_m = m;
  d.poff = c->poff.as<long long>(); d.noff = c->noff.as<long long>();
  d.x = c->x.as<double>(); d.work = c->work.as<double>();
  d.hist_s = c->hist_s.as<double>(); d.hist_y = c->hist_y.as<double>();
  d.hist_ys = c->hist_ys.as<double>(); d.hist_alpha = c->hist_alpha.as<double>();
  d.lu = c->lu.as<double>();
  d.success = c->success.as<int>(); d.cost = c->cost.as<double>(); d.stats = c->stats.as<int>();
  d.xyerr = c->xyerr.as<double>(); d.coef = c->coef.as<double>(); d.T = c->T.as<double>();
  d.knots = c->knots.as<double>(); d.alm = c->alm.as<double>(); d.fout = c->fout.as<double>();
  d.sbuf = c->sbuf.as<double>();
  d.mstash = c->mstash.as<double>();
  d.elapsed_us = c->elapsed.as<double>();
  d.start_us = c->startus.as<double>();
  d.hw_id = c->hwid.as<int>();
  d.gate_in_solve = 1;
  d.feas_flags = c->feas_flags.as<int>();
  d.feas_report = c->feas_report.as<double>();
  d.interrupted = c->interrupted.as<int>();
  HIPCHK(hipMemsetAsync(c->interrupted.p, 0, (size_t)batch * 4, c->stream));
  // a new batch has no planning-call groups until topay_set_groups says so
  c->h_group.clear();
  c->n_groups = 0;
  d.group_id = nullptr; d.group_tau = nullptr; d.cancel_budget = 0; d.cancel_flag = nullptr;
  c->gate_done = false;
  HIPCHK(hipMemsetAsync(c->elapsed.p, 0, (size_t)batch * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->success.p, 0, (size_t)batch * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->cost.p, 0xFF, (size_t)batch * 8, c->stream));   // never-launched candidates: cost = NaN
  HIPCHK(hipMemsetAsync(c->stats.p, 0, (size_t)batch * kStatsLen * 4, c->stream));
  c->have_traj = true;
  return TOPAY_OK;
}

// Persistent grids.  A workgroup of class k occupies the fraction r_k of a compute unit -- the larger of its share of
// the register file (NW waves of 512 / occ registers on four SIMDs of 512) and of the 160 KB of LDS -- for the time its
// share of the class's work takes: work_k = sum of N^1.5 over the class (the cost of an evaluation grows with N, the
// number of evaluations slowly), divided by the speed-up of NW waves, times the slow-down of a wave that shares its SIMD.
// The grids are proportional to that workgroup-time and scaled so that together they ask for exactly the compute units
// there are (x oversubscription): all launches of a batch end together and none of their workgroups waits in the
// dispatcher.  nm[k] = longest candidate the class's LDS is sized for.
static void compute_grids(topay_ctx* c, const int* nm, double cus, int* grid) {
  const ClassDef* ct = kClassTable;
  double wt[topay_ctx::NBUCKET] = {0}, rk[topay_ctx::NBUCKET] = {0}, need = 0.0;
  for (int k = 0; k < topay_ctx::NBUCKET; k++) {
    grid[k] = 0;
    if (c->cls[k].empty()) continue;
    double t = ct[k].nw == 1 ? 1.0 : (ct[k].nw == 2 ? 1.0 / 1.48 : 0.5);   // time of a workgroup per unit of work
    const double regs = (double)ct[k].nw / (4.0 * ct[k].occ), lds = (double)class_lds_bytes(ct[k], nm[k]) / (160.0 * 1024.0);
    rk[k] = std::max(regs, lds);
    // a wave that shares its SIMD runs slower (two of them get through kOcc2Gain times the work of one); classes whose LDS
    // keeps them from sharing are not slowed down
    if (ct[k].occ == 2 && lds <= 0.1875) t *= 2.0 / kOcc2Gain;
    // the smallest class's workgroups cannot take over anybody's queue, the others can take over its: it gets less than its share
    // (measured in round 3, factor 1.0 / 0.9 / 0.8 / 0.7: serial step 1.00 / 0.99 / 0.98 / 0.97 s)
    if (k == 0) t *= 0.8;
    for (int b : c->cls[k]) wt[k] += t * std::pow((double)c->hN[b], 1.5);
    need += wt[k] * rk[k];
  }
  if (need <= 0.0) return;
  const double G = cus / need;
  for (int k = 0; k < topay_ctx::NBUCKET; k++) {
    if (c->cls[k].empty()) continue;
    grid[k] = std::max(1, std::min((int)c->cls[k].size(), (int)std::floor(G * wt[k] + 0.5)));
  }
}

// Dynamic LDS above the 64 KB default needs the attribute; it is set once per device to the most a kernel can ask
// for (the launch itself passes the size it needs), not per launch: two host threads launching different contexts
// would otherwise interleave set(small), set(large), launch(large).
static std::once_flag g_attr_once[16];
static hipError_t g_attr_err[16];
static hipError_t set_kernel_attributes(int device) {
  std::call_once(g_attr_once[device % 16], [device] {
    (void)device;
    hipError_t e = hipSuccess;
    const ClassDef* ct = kClassTable;
    // The whole LDS of a compute unit for every kernel: an attribute below a launch's request is an error on a runtime
    // that enforces it, and nothing is gained by asking for less.
    const int lds = kLdsDoublesPerCU * 8;
    for (int k = 0; k < TOPAY_NBUCKET && e == hipSuccess; k++) {
      e = hipFuncSetAttribute((const void*)ct[k].solve, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)ct[k].eval, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e == hipSuccess && ct[k].lat) e = hipFuncSetAttribute((const void*)ct[k].lat, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
    g_attr_err[device % 16] = e;
  });
  return g_attr_err[device % 16];
}

// Lowest class whose queue a workgroup of class k may go on with once its own is empty.  A stolen candidate is solved by
// the STEALING class's kernel, which has at least as many rows per lane: the solver's elements sit in the same pairs of the
// same lanes (the extra registers hold masked zeros) and the evaluation is order-identical over rows per thread, so the
// bits are those of the candidate's own class.  Only classes whose workgroups have the same number of waves, and never
// across the long / common boundary (a resident workgroup of a long class holds LDS or whole compute units the common
// classes' workgroups want).
static int steal_floor(int k) {
  const ClassDef* ct = kClassTable;
  int lo = k;
  while (lo > 0 && ct[lo - 1].nw == ct[k].nw && ((lo - 1 >= kBigFirst) == (k >= kBigFirst))) lo--;
  return lo;
}

template <bool EVAL, typename... Args>
static topay_status launch_classes(topay_ctx* c, bool persistent, Args... args) {
  // One launch per N-bucket, each on its own stream so that the tail of one bucket overlaps the others.
  // Longest jobs first.  The context's main stream waits for all of them (events), so the caller's
  // stopwatch on the main stream brackets the whole solve.
  const ClassDef* ct = kClassTable;
  int launches = 0, helper_launches = 0, off = 0;
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  HIPCHK(set_kernel_attributes(c->device));
  int slots = 0;
  if (persistent) {
    if (c->qnext.ensure(sizeof(int) * topay_ctx::NBUCKET) != TOPAY_OK) return TOPAY_ERR_NO_DEVICE;
    HIPCHK(hipMemsetAsync(c->qnext.p, 0, sizeof(int) * topay_ctx::NBUCKET, c->stream));
    slots = c->simd_slots;
  }
  int pgrid[topay_ctx::NBUCKET] = {0}, nmk[topay_ctx::NBUCKET] = {0};
  for (int k = 0; k < topay_ctx::NBUCKET; k++) {
    for (int b : c->cls[k]) nmk[k] = std::max(nmk[k], c->hN[b]);
    // classes that may take over each other's queues run the same kernel: its LDS must hold the longest candidate of any of them
    if (persistent && c->steal)
      for (int k2 = steal_floor(k); k2 < k; k2++)
        for (int b : c->cls[k2]) nmk[k] = std::max(nmk[k], c->hN[b]);
  }
  if (persistent) {
    // 8 % more workgroups than SIMD slots: in steady state 3-5 % of the SIMDs have no workgroup because the ones still
    // pending do not find LDS on the compute units where a SIMD is free (54-107 KB workgroups beside 21-36 KB ones); a few
    // pending workgroups more, mostly of the small classes, fill those.  Measured, interleaved on one box
    // (1.0 / 1.08): 10.01 / 10.20, 10.06 / 10.19, 10.04 / 10.07k trajectories/s; 1.2 is no better.
    compute_grids(c, nmk, slots / 4.0 * 1.08, pgrid);
  }
  HIPCHK(hipEventRecord(c->bstart, c->stream));  // params + resets on the main stream come first
  for (int k = topay_ctx::NBUCKET - 1; k >= 0; k--) {
    const std::vector<int>& v = c->cls[k];
    const int nk = (int)v.size();
    if (nk == 0) continue;
    const int nm = nmk[k];
    DevBatch d = c->db;
    d.order = c->db.order + off;
    int grid = nk;
    if (persistent) {
      d.order = c->db.order;
      d.queue_next = c->qnext.as<int>();
      d.queue_class = k;
      d.queue_lowest = c->steal ? steal_floor(k) : k;
      int o2 = 0;
      for (int kk = topay_ctx::NBUCKET - 1; kk >= 0; kk--) {   // `order` holds the classes largest first
        d.queue_off[kk] = o2;
        d.queue_count[kk] = (int)c->cls[kk].size();
        o2 += d.queue_count[kk];
      }
      grid = pgrid[k];
    }
    off += nk;
    // helper-wave kernels (topay_set_latency_mode): a one-wave class of a small batch runs on four-wave workgroups whose
    // extra waves only join the evaluations -- same bits, shorter sample sweeps
    const bool lat = !EVAL && ct[k].lat && (c->latency_mode == 2 || (c->latency_mode == 1 && c->B <= c->simd_slots));
    size_t lds = class_lds_bytes(ct[k], nm);
    if (lat) {
      lds = (size_t)(eval_lds_total(nm, kLatWaves) + solve_tail_doubles(true)) * sizeof(double);
      grid = nk;   // a workgroup per candidate of the class
    }
    if (k == topay_ctx::NBUCKET - 2 && !c->cls[topay_ctx::NBUCKET - 1].empty() && c->bstream[k] == c->stream)
      HIPCHK(hipStreamCreateWithFlags(&c->bstream[k], hipStreamNonBlocking));   // both long classes in one batch: they must not serialise
    hipStream_t st = c->bstream[k];
    if (st != c->stream) HIPCHK(hipStreamWaitEvent(st, c->bstart, 0));
    if constexpr (EVAL) hipLaunchKernelGGL(ct[k].eval, dim3(grid), dim3(64 * ct[k].nw), lds, st, d, (const DevMap*)c->dmaps.p, args..., nm);
    else if (lat) { hipLaunchKernelGGL(ct[k].lat, dim3(grid), dim3(64 * kLatWaves), lds, st, d, (const DevMap*)c->dmaps.p, nm); helper_launches++; }
    else hipLaunchKernelGGL(ct[k].solve, dim3(grid), dim3(64 * ct[k].nw), lds, st, d, (const DevMap*)c->dmaps.p, nm);
    HIPCHK(hipGetLastError());
    if (st != c->stream) HIPCHK(hipEventRecord(c->bevent[k], st));
    launches++;
  }
  for (int k = 0; k < topay_ctx::NBUCKET; k++)
    if (!c->cls[k].empty() && c->bstream[k] != c->stream) HIPCHK(hipStreamWaitEvent(c->stream, c->bevent[k], 0));
  c->last_launches = launches;
  c->last_helper_launches = helper_launches;
  return TOPAY_OK;
}


static bool batch_done(topay_ctx* p) { return !p->pending || hipStreamQuery(p->stream) == hipSuccess; }

// Launch order of the resident batch: inside every class longest first (the tail of a batch), or -- with the planner's
// cancellation -- shortest first (see topay_set_groups).
static topay_status upload_order(topay_ctx* c, bool shortest_first) {
  std::vector<int> ord;
  for (int k = topay_ctx::NBUCKET - 1; k >= 0; k--) {
    std::vector<int>& v = c->cls[k];
    if (shortest_first) std::stable_sort(v.begin(), v.end(), [&](int a, int b2) { return c->hN[a] < c->hN[b2]; });
    else std::stable_sort(v.begin(), v.end(), [&](int a, int b2) {
      return c->hN[a] != c->hN[b2] ? c->hN[a] > c->hN[b2] : (c->h_path_len[a] != c->h_path_len[b2] ? c->h_path_len[a] > c->h_path_len[b2] : a < b2);
    });
    ord.insert(ord.end(), v.begin(), v.end());
  }
  ord.resize(c->B, 0);
  HIPCHK(h2d_sync(c, c->order.as<int>(), ord.data(), (size_t)c->B));
  return TOPAY_OK;
}

extern "C" {

topay_status topay_set_init_traj(topay_ctx* c, int batch, const int* path_len, const double* init_paths,
                                 const double* boundary_vel, const double* boundary_acc, const int* map_ids) {
  return set_init_traj_impl(c, batch, path_len, init_paths, boundary_vel, boundary_acc, map_ids, hipMemcpyHostToDevice);
}

topay_status topay_reset(topay_ctx* c) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  c->solved = false;
  return run_init(c);
}

topay_status topay_optimize_async(topay_ctx* c) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status s0 = wait_pending(c)) return s0;   // a second solve on a context whose first has not been waited for: finish that one first
  {
    // Dispatch gate.  Batches of different contexts run on different streams; issued at the same time their waves
    // would be dispatched alternately and both would end in the same long tail.  Holding the new batch back until
    // every candidate of the previous one is resident gives oldest-first scheduling without stream priorities: the
    // new waves take exactly the SIMDs the previous batch's tail leaves idle.  Host-side wait on a counter in pinned
    // memory (<= one bulk phase); results do not depend on it.
    std::lock_guard<std::mutex> lk(g_issue_mutex);
    topay_ctx* p = g_last_issued;
    if (p && p != c && p->pending && p->device == c->device && p->h_started) {
      volatile int* cnt = p->h_started;
      const auto t0 = std::chrono::steady_clock::now();
      while (*cnt < p->n_gate) {
        if (batch_done(p)) break;  // finished (or never launched anything)
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) {
          // scheduling only: the batch is issued anyway, but the caller can see that the hand-over did not happen
          c->gate_timeouts++;
          set_err("dispatch gate: the previous batch did not become resident within 120 s; issuing anyway");
          break;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
      }
    }
    c->h_started[0] = 0;
    int nl = 0, ng = 0;
    for (int k = 0; k < topay_ctx::NBUCKET; k++) {
      nl += (int)c->cls[k].size();
      if (k < kBigFirst) ng += (int)c->cls[k].size();
    }
    c->n_launched = nl;
    // The gate waits for the candidates of the three common classes only: the few workgroups of the two classes of
    // long candidates need 70 / 104 KB of LDS and may not find a compute unit with that much free until the previous
    // batch's tail -- holding the whole next batch back for them leaves the rest of the device idle meanwhile.
    c->n_gate = ng;
    c->db.gate_maxN = kBucketMaxN[kBigFirst - 1];   // (the common classes: up to 32 pieces)
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, c->h_started, 0));
    c->db.started = (int*)dp;
    g_last_issued = c;
  }
  HIPCHK(c->solve_timer.start(c->stream));
  // cancellation state of this solve: nobody has succeeded yet (clock "infinity"), nothing is interrupted
  c->h_cancel[0] = 0;
  {
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, c->h_cancel, 0));
    c->db.cancel_flag = (const int*)dp;
  }
  c->h_started[12] = 0;
  {
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, c->h_started + 12, 0));
    c->db.gate_truncated = (int*)dp;
  }
  c->db.cancel_budget = c->n_groups > 0 ? c->cancel_budget : 0;
  if (c->n_groups > 0) HIPCHK(hipMemsetAsync(c->group_tau.p, 0x7f, (size_t)c->n_groups * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->interrupted.p, 0, (size_t)c->B * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->feas_flags.p, 0, (size_t)c->B * 8, c->stream));
  c->gate_done = false;
  // candidates that were not launched keep success = 0 and cost = NaN
  HIPCHK(hipMemsetAsync(c->success.p, 0, (size_t)c->B * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->cost.p, 0xFF, (size_t)c->B * 8, c->stream));
  topay_status s = launch_classes<false>(c, c->persistent);
  if (s != TOPAY_OK) {
    // some class launches may already be running on the batch's buffers: nothing may touch them before they have ended
    for (int k = 0; k < topay_ctx::NBUCKET; k++)
      if (c->bstream[k]) (void)hipStreamSynchronize(c->bstream[k]);
    (void)hipStreamSynchronize(c->stream);
    return s;
  }
  HIPCHK(c->solve_timer.stop(c->stream));
  c->pending = true;
  return TOPAY_OK;
}

topay_status topay_synchronize(topay_ctx* c) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->pending) {
    HIPCHK(c->solve_timer.read(&c->last_ms));
    c->solved = true;
    c->pending = false;
    // (a candidate whose history block could not hold the gate's scratch -- a small mem_size -- was left ungated by its
    // wave: the verdicts are then taken by the separate kernel, with scratch of the right size, at the first request)
    c->gate_done = c->h_started[12] == 0;
    if (c->n_groups > 0 && c->cancel_budget > 0) {
      // The rule, applied once more to the finished batch so that the outcome does not depend on WHEN a candidate saw its
      // group's clock: a candidate counts iff its own work clock is within cancel_budget of the smallest clock of a
      // feasible success of its planning call.  (A candidate stopped on the device had already passed that limit with
      // the clock it saw, which was no smaller than the final one; one that ran to its end before the first success of
      // its call was published is stopped here.)
      const int B = c->B;
      std::vector<int> succ(B), st((size_t)B * kStatsLen), fl((size_t)B * 2), intr(B), tau(c->n_groups);
      HIPCHK(d2h_sync(c, succ.data(), c->success.as<int>(), (size_t)B));
      HIPCHK(d2h_sync(c, st.data(), c->stats.as<int>(), st.size()));
      HIPCHK(d2h_sync(c, fl.data(), c->feas_flags.as<int>(), fl.size()));
      HIPCHK(d2h_sync(c, intr.data(), c->interrupted.as<int>(), (size_t)B));
      HIPCHK(d2h_sync(c, tau.data(), c->group_tau.as<int>(), (size_t)c->n_groups));
      bool changed = false;
      for (int b = 0; b < B; b++) {
        const int g = c->h_group[b];
        if (g < 0 || intr[b] || c->hN[b] == 0) continue;
        const int* sb = &st[(size_t)b * kStatsLen];
        const long long clock = (long long)(sb[2] + sb[5]) * c->hN[b];
        if (clock > (long long)tau[g] + c->cancel_budget) {
          intr[b] = 1; succ[b] = 0; fl[2 * b] = 0; fl[2 * b + 1] = 0;
          st[(size_t)b * kStatsLen + 3] = TOPAY_INTERRUPTED;
          changed = true;
        }
      }
      if (changed) {
        HIPCHK(h2d_sync(c, c->success.as<int>(), succ.data(), (size_t)B));
        HIPCHK(h2d_sync(c, c->stats.as<int>(), st.data(), st.size()));
        HIPCHK(h2d_sync(c, c->feas_flags.as<int>(), fl.data(), fl.size()));
        HIPCHK(h2d_sync(c, c->interrupted.as<int>(), intr.data(), (size_t)B));
      }
    }
  }
  return TOPAY_OK;
}

// == the planner's thread group (planner.cpp:829-952): group_id[b] = planning call (scenario) of candidate b, -1 = none.
// With a positive cancel budget the candidates of a call that are still running `budget` piece-evaluations after the
// call's first success that passes the gate are interrupted (threads.interrupt_all() 100 ms after future_succ; the unit
// is alm_work_budget's: 24 000 = 1 s, so 100 ms = 2400).  Call after topay_set_init_traj; 0 / NULL switches it off.
topay_status topay_set_groups(topay_ctx* c, const int* group_id, int cancel_budget) {
  if (!c || !c->have_traj) return TOPAY_ERR_NO_TRAJ;
  if (cancel_budget < 0) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const bool had_groups = c->n_groups > 0;
  c->h_group.clear();
  c->n_groups = 0;
  c->cancel_budget = cancel_budget;
  c->db.group_id = nullptr; c->db.group_tau = nullptr;
  if (!group_id || cancel_budget == 0) {
    if (had_groups) return upload_order(c, false);   // back to longest first
    return TOPAY_OK;
  }
  // The in-solve gate's scratch is the candidate's dead L-BFGS history block (mem_size x n doubles twice); a candidate whose
  // block is too short is left to the separate kernel and would never publish its call's clock: the window would silently
  // stay shut.  64 rows hold the gate's panels and sample times of a trajectory three times as long as its initial guess.
  if (std::max(c->hp.s1_lbfgs.mem_size, c->hp.s2_lbfgs.mem_size) < 64) {
    set_err("cancellation window: the L-BFGS mem_size must be at least 64 (the in-solve gate works in the history block)");
    return TOPAY_ERR_INVALID_ARG;
  }
  // the caller's ids (any integers >= 0, e.g. global scenario numbers of a sharded sweep; -1 = no planning call) become
  // dense indices: the device holds one clock per planning call that is present, not one per possible id
  std::vector<int> dense(c->B, -1);
  {
    std::vector<int> ids;
    for (int b = 0; b < c->B; b++) {
      if (group_id[b] < -1) return TOPAY_ERR_INVALID_ARG;
      if (group_id[b] >= 0) ids.push_back(group_id[b]);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    for (int b = 0; b < c->B; b++)
      if (group_id[b] >= 0) dense[b] = (int)(std::lower_bound(ids.begin(), ids.end(), group_id[b]) - ids.begin());
    c->n_groups = (int)ids.size();
  }
  const int ng = c->n_groups;
  c->h_group = dense;
  if (ng == 0) { c->cancel_budget = cancel_budget; return TOPAY_OK; }
  topay_status s;
  if ((s = c->group_id.ensure((size_t)c->B * 4)) != TOPAY_OK) return s;
  if ((s = c->group_tau.ensure((size_t)std::max(1, ng) * 4)) != TOPAY_OK) return s;
  HIPCHK(h2d_sync(c, c->group_id.as<int>(), dense.data(), (size_t)c->B));
  c->db.group_id = c->group_id.as<int>();
  c->db.group_tau = c->group_tau.as<int>();
  // Launch order with cancellation: shortest candidates first inside every class.  Without it the longest go first (they
  // are the tail of the batch); with it they are the ones the rule interrupts, and they can only be stopped early if the
  // short candidates of their planning call -- the ones that succeed first on the work clock -- have already run.  The
  // outcome does not depend on the order (the rule is applied to the candidates' own clocks), only the time saved does.
  return upload_order(c, true);
}

// Helper-wave kernels for small batches (include/topay.h)
topay_status topay_set_latency_mode(topay_ctx* c, int mode) {
  if (!c || mode < 0 || mode > 2) return TOPAY_ERR_INVALID_ARG;
  c->latency_mode = mode;
  return TOPAY_OK;
}

// threads.interrupt_all() for the solve in flight (planner.cpp:952): every candidate stops at its next interruption
// point (top of the ALM loop / next stage-2 evaluation); returns at once, topay_synchronize waits for the kernels.
topay_status topay_cancel(topay_ctx* c) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  if (c->h_cancel) __atomic_store_n(c->h_cancel, 1, __ATOMIC_RELEASE);
  return TOPAY_OK;
}

// interrupted[b] = 1: candidate b was stopped by the cancellation rule or by topay_cancel (no trajectory, success 0)
topay_status topay_get_interrupted(topay_ctx* c, int* interrupted) {
  if (!c || !c->have_traj || !interrupted) return TOPAY_ERR_NO_TRAJ;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  HIPCHK(d2h_sync(c, interrupted, c->interrupted.as<int>(), (size_t)c->B));
  return TOPAY_OK;
}

topay_status topay_optimize(topay_ctx* c) {
  topay_status s = topay_optimize_async(c);
  if (s != TOPAY_OK) return s;
  return topay_synchronize(c);
}

topay_status topay_optimize_within(topay_ctx* c, double budget_ms, int* timed_out) {
  if (timed_out) *timed_out = 0;
  if (!(budget_ms > 0.0)) return TOPAY_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  topay_status s = topay_optimize_async(c);
  if (s != TOPAY_OK) return s;
  while (hipStreamQuery(c->stream) == hipErrorNotReady) {
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= budget_ms) {
      (void)topay_cancel(c);
      if (timed_out) *timed_out = 1;
      break;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  return topay_synchronize(c);
}

}  // extern "C"
