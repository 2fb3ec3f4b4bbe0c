// Host side of the C-ABI, part 9: tracked trajectories (end_traj / global_traj of every robot slot), the one check of the robot
// slots an entry names, the safety sweep, the endpoints of a replan, the sampling of tracked trajectories and the replanning
// cycle (topay_track.h; Planner::safeCallback and replanCallback).

#pragma once

// ---------------------------------------------------------------------------------------------------------------------
// The store.  One arena (TrackState::arena) holds every tracked trajectory in the layout stated in topay_track.h; it grows by
// ragged offsets and keeps its contents.  A slot whose block is large enough for its next trajectory reuses it; one that is
// not gets a new block and the old one is lost.  Blocks are sized to a power of two, so the lost blocks of a slot sum to
// less than its last one: the arena is bounded by four times the largest need of every (slot, which), whatever the order
// of the trajectories (include/topay.h states it).  track_commit_impl takes every (robot, w) at most once per call: two
// workgroups would write one block.
// ---------------------------------------------------------------------------------------------------------------------
static const double kTrackPanel = 0.1 / 4;   // seq_res / approx_res (moma_traj_opt.h:28-29), the expression of the kernels

static bool track_duration_ok(const double* dur, int N, double& T) {   // the gate's "no trajectory" rule
  T = 0.0;
  for (int i = 0; i < N; i++) T += dur[i];
  return T > 0.0 && T < 1.0e4;
}

struct TrackPut {   // one trajectory on its way into the arena
  int robot, w;     // w: 0 end_traj, 1 global_traj
  int N;
  double T;
  long long src_piece, src_start;
};

// Blocks for `puts` (reused or appended), then k_track_commit from (s_dur, s_coef, s_start) on the device.
static topay_status track_commit_impl(topay_ctx* c, const std::vector<TrackPut>& puts, const double* s_dur, const double* s_coef, const double* s_start) {
  const size_t n = puts.size();
  if (n == 0) return TOPAY_OK;
  if (c->track.slots.empty()) c->track.slots.resize(TOPAY_TRACK_SLOTS);
  std::vector<topay::TrackDesc> dst(n);
  std::vector<long long> sp(n), ss(n), cap(n);
  size_t used = c->track.used;
  for (size_t k = 0; k < n; k++) {
    const TrackPut& p = puts[k];
    const long long num = (long long)std::floor(p.T / kTrackPanel);
    const long long need = topay::track_doubles(p.N, num);
    const TrackSlot& sl = c->track.slots[p.robot];
    dst[k].N = p.N;
    dst[k].num = (int)num;
    if (sl.cap[p.w] >= need) { dst[k].off = sl.d[p.w].off; cap[k] = sl.cap[p.w]; }
    else {
      long long blk = 1024;
      while (blk < need) blk *= 2;
      dst[k].off = (long long)used; cap[k] = blk; used += (size_t)blk;
    }
    sp[k] = p.src_piece; ss[k] = p.src_start;
  }
  topay_status s;
  if ((s = c->track.arena.ensure_keep(c->stream, used * 8, c->track.used * 8)) != TOPAY_OK) return s;
  topay::TrackDesc* d_dst; long long *d_sp, *d_ss;
  auto lay = [&](Carver& k) { d_sp = k.take<long long>(n); d_ss = k.take<long long>(n); d_dst = k.take<topay::TrackDesc>(n); };
  if ((s = c->track.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_sp, sp.data(), n));
  HIPCHK(h2d(c, d_ss, ss.data(), n));
  HIPCHK(h2d(c, d_dst, dst.data(), n));
  hipLaunchKernelGGL(topay::k_track_commit, dim3((unsigned)n), dim3(64), 0, c->stream, (int)n, (const topay::TrackDesc*)d_dst, (const long long*)d_sp,
                     (const long long*)d_ss, s_dur, s_coef, s_start, c->track.arena.as<double>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  c->track.used = used;
  for (size_t k = 0; k < n; k++) {
    TrackSlot& sl = c->track.slots[puts[k].robot];
    sl.d[puts[k].w] = dst[k];
    sl.cap[puts[k].w] = cap[k];
    sl.T[puts[k].w] = puts[k].T;
  }
  return TOPAY_OK;
}

// What an entry asks of the robot slots it names (check_robot_slots).
enum : unsigned {
  kRobotDistinct = 1,   // every slot is named once
  kRobotEndTraj = 2,    // ... has an end_traj
  kRobotMpc = 4,        // ... a controller that was reset (topay_mpc_reset)
  kRobotSim = 8         // ... a simulator that was reset (topay_sim_reset)
};
// The one check of robot slots: robots[0 .. n).  A slot out of range, named twice or never reset is TOPAY_ERR_INVALID_ARG, one
// without an end_traj TOPAY_ERR_NO_TRAJ; the error text names the entry (`who`).
static topay_status check_robot_slots(topay_ctx* c, int n, const int* robots, unsigned need, const char* who) {
  std::vector<char> seen(need & kRobotDistinct ? TOPAY_TRACK_SLOTS : 0, 0);
  for (int k = 0; k < n; k++)
    if (robots[k] < 0 || robots[k] >= TOPAY_TRACK_SLOTS) { set_err(std::string(who) + ": robot slot out of range"); return TOPAY_ERR_INVALID_ARG; }
  for (int k = 0; k < n && (need & kRobotDistinct); k++) {
    if (seen[robots[k]]) { set_err(std::string(who) + ": a robot slot is named twice"); return TOPAY_ERR_INVALID_ARG; }
    seen[robots[k]] = 1;
  }
  for (int k = 0; k < n; k++) {
    const int r = robots[k];
    const std::string slot = std::string(who) + ": robot slot " + std::to_string(r);
    if ((need & kRobotEndTraj) && !c->track.find(r, 0)) { set_err(slot + " has no end_traj"); return TOPAY_ERR_NO_TRAJ; }
    if ((need & kRobotMpc) && (c->mpc.have.empty() || !c->mpc.have[r])) { set_err(slot + " was never reset (topay_mpc_reset)"); return TOPAY_ERR_INVALID_ARG; }
    if ((need & kRobotSim) && (c->mpc.sim_have.empty() || !c->mpc.sim_have[r])) { set_err(slot + " has no simulator (topay_sim_reset)"); return TOPAY_ERR_INVALID_ARG; }
  }
  return TOPAY_OK;
}

static topay_status track_safe_impl(topay_ctx* c, int n, const int* robots, const int* map_ids, int* safe, int* first_hit, double* hit) {
  const size_t N = (size_t)n;
  std::vector<topay::TrackDesc> desc(N);
  for (int k = 0; k < n; k++) desc[k] = *c->track.find(robots[k], 0);
  topay::TrackDesc* d_desc; int *d_mid, *d_safe, *d_fh; double* d_hit;
  auto lay = [&](Carver& k) {
    d_hit = k.take<double>(2 * N); d_desc = k.take<topay::TrackDesc>(N); d_mid = k.take<int>(N); d_safe = k.take<int>(N); d_fh = k.take<int>(2 * N);
  };
  topay_status s;
  if ((s = c->track.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_desc, desc.data(), N));
  HIPCHK(h2d(c, d_mid, map_ids, N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  topay::TrackSafeArgs A;
  A.n = n; A.desc = d_desc; A.arena = c->track.arena.as<double>(); A.map_id = d_mid; A.safe = d_safe; A.first_hit = d_fh; A.hit = d_hit;
  HIPCHK(c->track.safe_timer.start(c->stream));
  hipLaunchKernelGGL(topay::k_track_safe, dim3((unsigned)n), dim3(64), 0, c->stream, A, (const DevMap*)c->dmaps.p);
  HIPCHK(hipGetLastError());
  HIPCHK(c->track.safe_timer.stop(c->stream));
  if (safe) HIPCHK(d2h(c, safe, d_safe, N));
  if (first_hit) HIPCHK(d2h(c, first_hit, d_fh, 2 * N));
  if (hit) HIPCHK(d2h(c, hit, d_hit, 2 * N));
  HIPCHK(hipStreamSynchronize(c->stream));
  (void)c->track.safe_timer.read(&c->track.safe_ms);
  return TOPAY_OK;
}

static topay_status track_endpoints_impl(topay_ctx* c, int n, const int* robots, const double* t_replan, const double* t_begin, const double* global_goal,
                                         double budget, double horizon, double* start, double* start_v, double* goal, int* goal_source) {
  const size_t N = (size_t)n;
  bool clocks = all_finite(t_replan, N) && all_finite(t_begin, N);
  for (int k = 0; k < n; k++) clocks = clocks && t_begin[k] >= 0.0;   // (the walk along global_traj starts at t_begin)
  if (!clocks) { set_err("topay_replan_inputs: the clocks must be finite, t_since_begin not negative"); return TOPAY_ERR_INVALID_ARG; }
  if (!all_finite(&budget, 1) || !(horizon >= 0.0)) return TOPAY_ERR_INVALID_ARG;
  std::vector<topay::TrackDesc> de(N), dg(N);
  for (int k = 0; k < n; k++) {
    de[k] = *c->track.find(robots[k], 0);
    const topay::TrackDesc* g = c->track.find(robots[k], 1);
    if (g) dg[k] = *g;
    else { dg[k].off = 0; dg[k].N = 0; dg[k].num = 0; }
  }
  topay::TrackDesc *d_de, *d_dg; double *d_tr, *d_tb, *d_gg, *d_st, *d_sv, *d_go; int* d_src;
  auto lay = [&](Carver& k) {
    d_tr = k.take<double>(N); d_tb = k.take<double>(N); d_gg = k.take<double>(10 * N);
    d_st = k.take<double>(10 * N); d_sv = k.take<double>(10 * N); d_go = k.take<double>(10 * N);   // (contiguous: one copy back)
    d_de = k.take<topay::TrackDesc>(N); d_dg = k.take<topay::TrackDesc>(N); d_src = k.take<int>(N);
  };
  topay_status s;
  if ((s = c->track.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_tr, t_replan, N));
  HIPCHK(h2d(c, d_tb, t_begin, N));
  HIPCHK(h2d(c, d_gg, global_goal, 10 * N));
  HIPCHK(h2d(c, d_de, de.data(), N));
  HIPCHK(h2d(c, d_dg, dg.data(), N));
  topay::TrackEndArgs A;
  A.n = n; A.end_desc = d_de; A.glob_desc = d_dg; A.arena = c->track.arena.as<double>(); A.t_replan = d_tr; A.t_begin = d_tb; A.global_goal = d_gg;
  A.budget = budget; A.horizon = horizon; A.start = d_st; A.start_v = d_sv; A.goal = d_go; A.goal_source = d_src;
  hipLaunchKernelGGL(topay::k_track_endpoints, dim3((unsigned)n), dim3(64), 0, c->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, start, d_st, 10 * N));
  HIPCHK(d2h(c, start_v, d_sv, 10 * N));
  HIPCHK(d2h(c, goal, d_go, 10 * N));
  HIPCHK(d2h(c, goal_source, d_src, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampling (k_track_sample).  An output of topay_track_sample / _grid may lie on the host or on the device.  The host code had no
// convention for device outputs before these entries (every other entry copies back), so the pointer itself is asked:
// hipPointerGetAttributes.  Device memory of the context's device is written by the kernel where it lies; anything else (plain,
// pinned or managed host memory) gets a block of the io buffer and a copy back.
// ---------------------------------------------------------------------------------------------------------------------
struct SampleOut {
  double* user = nullptr;   // the caller's pointer; null: not asked for
  double* dev = nullptr;    // where the kernel writes
  size_t count = 0;         // doubles
  bool direct = false;      // dev == user
};
static topay_status sample_out(topay_ctx* c, double* user, bool asked, size_t count, SampleOut& o) {
  o = SampleOut();
  if (!user || !asked) return TOPAY_OK;
  o.user = user; o.count = count;
#ifndef TOPAY_CPU_EMU
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, user) != hipSuccess) (void)hipGetLastError();   // memory the runtime has never seen: the host's
  else if (at.type == hipMemoryTypeDevice) {
    if (at.device != c->device) { set_err("topay_track_sample: an output lies on another device than the context"); return TOPAY_ERR_INVALID_ARG; }
    o.direct = true; o.dev = user;
  }
#endif
  return TOPAY_OK;
}

struct TrackSampleOuts { double *state, *dstate, *ee_pose, *clearance, *centres, *duration, *distance; };

// Robot k's samples are rows off[k] .. off[k + 1] - 1.  times: the rows' times, or null for a grid call (t0[k], += step).
static topay_status track_sample_impl(topay_ctx* c, int n, const int* robots, int w, const int* map_ids, const std::vector<int>& off, const double* times,
                                      const double* t0, double step, int what, const TrackSampleOuts& U) {
  const size_t N = (size_t)n, M = (size_t)off[N];
  // the work table (TrackSampleItem)
  std::vector<topay::TrackDesc> desc(N);
  std::vector<topay::TrackSampleItem> items;
  for (int k = 0; k < n; k++) {
    desc[k] = *c->track.find(robots[k], w);
    const int cnt = off[k + 1] - off[k];
    double t = times ? 0.0 : t0[k];
    int b = 0;
    do {
      topay::TrackSampleItem I;
      I.robot = k; I.row0 = off[k] + 64 * b; I.count = std::min(64, cnt - 64 * b); I.head = b == 0; I.t_first = t;
      items.push_back(I);
      if (!times)
        for (int j = 0; j < 64; j++) t += step;   // (the sums of track_times, in its order)
      b++;
    } while (64 * b < cnt);
  }
  const size_t NI = items.size();
  // the outputs: what is asked for and has somewhere to go
  const int K = topay::kSampleBodies;
  SampleOut o_st, o_dv, o_ee, o_cl, o_ce, o_du, o_di;
  topay_status s;
  if ((s = sample_out(c, U.state, what & topay::kSampleState, 10 * M, o_st)) != TOPAY_OK || (s = sample_out(c, U.dstate, what & topay::kSampleDState, 10 * M, o_dv)) != TOPAY_OK ||
      (s = sample_out(c, U.ee_pose, what & topay::kSampleEePose, 9 * M, o_ee)) != TOPAY_OK || (s = sample_out(c, U.clearance, what & topay::kSampleClearance, K * M, o_cl)) != TOPAY_OK ||
      (s = sample_out(c, U.centres, what & topay::kSampleCentres, 3 * TOPAY_NSPH * M, o_ce)) != TOPAY_OK || (s = sample_out(c, U.duration, true, N, o_du)) != TOPAY_OK ||
      (s = sample_out(c, U.distance, what & topay::kSampleDistance, K * M, o_di)) != TOPAY_OK)
    return s;
  SampleOut* outs[7] = {&o_st, &o_dv, &o_ee, &o_cl, &o_ce, &o_du, &o_di};
  int eff = 0;
  const int bit[7] = {topay::kSampleState, topay::kSampleDState, topay::kSampleEePose, topay::kSampleClearance, topay::kSampleCentres, 0, topay::kSampleDistance};
  for (int a = 0; a < 7; a++)
    if (outs[a]->user) eff |= bit[a];
  if (eff == 0 && !o_du.user) return TOPAY_OK;
  const bool need_map = eff & (topay::kSampleClearance | topay::kSampleDistance);
  topay::TrackSampleItem* d_items; topay::TrackDesc* d_desc; int* d_mid; double* d_times;
  auto lay = [&](Carver& k) {
    for (SampleOut* o : outs)
      if (o->user && !o->direct) o->dev = k.take<double>(o->count);
    d_times = k.take<double>(times ? M : 0); d_items = k.take<topay::TrackSampleItem>(NI); d_desc = k.take<topay::TrackDesc>(N); d_mid = k.take<int>(N);
  };
  if ((s = c->track.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_items, items.data(), NI));
  HIPCHK(h2d(c, d_desc, desc.data(), N));
  if (need_map) HIPCHK(h2d(c, d_mid, map_ids, N));
  if (times && M > 0) HIPCHK(h2d(c, d_times, times, M));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  topay::TrackSampleArgs A;
  A.n_items = (int)NI; A.what = eff; A.items = d_items; A.desc = d_desc; A.arena = c->track.arena.as<double>(); A.map_id = d_mid;
  A.times = times ? d_times : nullptr; A.step = step;
  A.state = o_st.dev; A.dstate = o_dv.dev; A.ee_pose = o_ee.dev; A.clearance = o_cl.dev; A.centres = o_ce.dev; A.duration = o_du.dev; A.distance = o_di.dev;
  const int level = eff & (topay::kSampleClearance | topay::kSampleCentres | topay::kSampleDistance) ? 2 : eff & topay::kSampleEePose ? 1 : 0;
  void (*kern)(topay::TrackSampleArgs, const DevMap*) = level == 2 ? topay::k_track_sample<2> : level == 1 ? topay::k_track_sample<1> : topay::k_track_sample<0>;
  HIPCHK(c->track.sample_timer.start(c->stream));
  hipLaunchKernelGGL(kern, dim3((unsigned)NI), dim3(64), 0, c->stream, A, (const DevMap*)c->dmaps.p);
  HIPCHK(hipGetLastError());
  HIPCHK(c->track.sample_timer.stop(c->stream));
  for (SampleOut* o : outs)
    if (o->user && !o->direct && o->count > 0) HIPCHK(d2h(c, o->user, o->dev, o->count));
  HIPCHK(hipStreamSynchronize(c->stream));
  (void)c->track.sample_timer.read(&c->track.sample_ms);
  return TOPAY_OK;
}

// What both sampling entries check ahead of their times: the slots, `which`, `what`, the maps when distances are asked for.
static topay_status track_sample_check(topay_ctx* c, int n, const int* robots, int which, const int* map_ids, int what, const char* who) {
  if (!c || n <= 0 || !robots) return TOPAY_ERR_INVALID_ARG;
  const std::string me(who);
  if (which < 1 || which > 2) { set_err(me + ": which must be 1 (end_traj) or 2 (global_traj)"); return TOPAY_ERR_INVALID_ARG; }
  if (what <= 0 || what >= 2 * topay::kSampleDistance) { set_err(me + ": what must be a sum of TOPAY_SAMPLE_* bits, at least one"); return TOPAY_ERR_INVALID_ARG; }
  if (topay_status s = check_robot_slots(c, n, robots, 0, who)) return s;   // (in range, then the maps, then the trajectories)
  if (what & (topay::kSampleClearance | topay::kSampleDistance)) {   // (the centres need no map)
    if (!map_ids) { set_err(me + ": TOPAY_SAMPLE_CLEARANCE and TOPAY_SAMPLE_DISTANCE need map_ids"); return TOPAY_ERR_INVALID_ARG; }
    if (topay_status s = check_map_slots(c, n, map_ids, kMapResident | kMap2d | kMap3d, who)) return s;
  }
  for (int k = 0; k < n; k++)
    if (!c->track.find(robots[k], which - 1)) {
      set_err(me + ": robot slot " + std::to_string(robots[k]) + (which == 1 ? " has no end_traj" : " has no global_traj"));
      return TOPAY_ERR_NO_TRAJ;
    }
  return TOPAY_OK;
}

// Winners of the last planning call into the slots: device to device from the plan store.
static topay_status track_commit_plan_impl(topay_ctx* c, int n, const int* robots, const int* call_idx, int which, int* committed) {
  PlanStore& S = c->plan_store;
  std::vector<double> hdur(std::max<size_t>(1, S.n_pieces()));
  if (S.n_pieces() > 0) HIPCHK(d2h_sync(c, hdur.data(), S.durations(), S.n_pieces()));
  std::vector<TrackPut> puts;
  for (int k = 0; k < n; k++) {
    const PlanStore::Entry& e = S.entry(call_idx[k]);
    if (committed) committed[k] = 0;
    if (e.n_pieces <= 0) continue;
    TrackPut p;
    p.robot = robots[k]; p.N = e.n_pieces; p.src_piece = e.piece0; p.src_start = PlanStore::front_double0(e);
    if (!track_duration_ok(&hdur[(size_t)e.piece0], e.n_pieces, p.T)) continue;
    for (int w = 0; w < 2; w++)
      if (which & (1 << w)) { p.w = w; puts.push_back(p); }
    if (committed) committed[k] = 1;
  }
  return track_commit_impl(c, puts, S.durations(), S.coeffs(), S.fronts());
}

extern "C" {

topay_status topay_track_set(topay_ctx* c, int robot, int which, const double* start3, int n_pieces, const double* durations, const double* coeffs) {
  if (!c || !start3 || !durations || !coeffs) return TOPAY_ERR_INVALID_ARG;
  if (topay_status cs = check_robot_slots(c, 1, &robot, 0, "topay_track_set")) return cs;
  if (which < 1 || which > 3) { set_err("topay_track_set: which must be 1 (end_traj), 2 (global_traj) or 3 (both)"); return TOPAY_ERR_INVALID_ARG; }
  if (n_pieces < 1 || n_pieces > TOPAY_MAX_N) { set_err("topay_track_set: 1..170 pieces"); return TOPAY_ERR_INVALID_ARG; }
  TrackPut p;
  p.robot = robot; p.N = n_pieces; p.src_piece = 0; p.src_start = 0;
  if (!track_duration_ok(durations, n_pieces, p.T)) { set_err("topay_track_set: the total duration must lie in (0, 1e4)"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n_pieces;
  double *d_dur, *d_coef, *d_start;
  auto lay = [&](Carver& k) { d_dur = k.take<double>(N); d_coef = k.take<double>(N * kCoefPerPiece); d_start = k.take<double>(4); };
  if (topay_status s = c->track.stage.carve(lay); s != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_dur, durations, N));
  HIPCHK(h2d(c, d_coef, coeffs, N * kCoefPerPiece));
  HIPCHK(h2d(c, d_start, start3, 3));
  std::vector<TrackPut> puts;
  for (int w = 0; w < 2; w++)
    if (which & (1 << w)) { p.w = w; puts.push_back(p); }
  return track_commit_impl(c, puts, d_dur, d_coef, d_start);
}

topay_status topay_track_commit_plan(topay_ctx* c, int n, const int* robots, const int* call_idx, int which, int* committed) {
  if (!c || n < 0 || (n > 0 && (!robots || !call_idx))) return TOPAY_ERR_INVALID_ARG;
  if (which < 1 || which > 3) { set_err("topay_track_commit_plan: which must be 1, 2 or 3"); return TOPAY_ERR_INVALID_ARG; }
  if (c->plan_store.empty()) { set_err("topay_track_commit_plan: no planning call has been run"); return TOPAY_ERR_NO_TRAJ; }
  if (topay_status cs = check_robot_slots(c, n, robots, kRobotDistinct, "topay_track_commit_plan")) return cs;
  for (int k = 0; k < n; k++)
    if (!c->plan_store.has(call_idx[k])) { set_err("topay_track_commit_plan: call " + std::to_string(call_idx[k]) + " is not in the plan store"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  return track_commit_plan_impl(c, n, robots, call_idx, which, committed);
}

topay_status topay_track_get(topay_ctx* c, int robot, int which, int cap_pieces, int* n_pieces, double* start3, double* durations, double* coeffs) {
  if (!c || !n_pieces || cap_pieces < 0) return TOPAY_ERR_INVALID_ARG;
  if (topay_status cs = check_robot_slots(c, 1, &robot, 0, "topay_track_get")) return cs;
  if (which < 1 || which > 2) { set_err("topay_track_get: which must be 1 (end_traj) or 2 (global_traj)"); return TOPAY_ERR_INVALID_ARG; }
  const topay::TrackDesc* D = c->track.find(robot, which - 1);
  *n_pieces = D ? D->N : 0;
  if (!D) return TOPAY_OK;
  if (!start3 && !durations && !coeffs) return TOPAY_OK;
  if (D->N > cap_pieces) { set_err("topay_track_get: cap_pieces too small"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const int N = D->N, rows = 6 * N;
  std::vector<double> h(4 + (size_t)N + (size_t)N * kCoefPerPiece);
  HIPCHK(d2h_sync(c, h.data(), c->track.arena.as<double>() + D->off, h.size()));
  if (start3) memcpy(start3, h.data(), 24);
  if (durations) memcpy(durations, h.data() + 4, (size_t)N * 8);
  if (coeffs) {
    const double* cm = h.data() + 4 + N;
    for (int t = 0; t < N * kCoefPerPiece; t++) {
      const int p = t / kCoefPerPiece, r = t - kCoefPerPiece * p, d = r / 6, kk = r - 6 * d;
      coeffs[t] = cm[(size_t)d * rows + 6 * p + 5 - kk];
    }
  }
  return TOPAY_OK;
}

topay_status topay_track_clear(topay_ctx* c, int robot) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  if (topay_status cs = check_robot_slots(c, 1, &robot, 0, "topay_track_clear")) return cs;
  if (!c->track.slots.empty())
    for (int w = 0; w < 2; w++) c->track.slots[robot].d[w].N = 0;   // (the block stays the slot's: its next trajectory may reuse it)
  return TOPAY_OK;
}

topay_status topay_track_safe(topay_ctx* c, int n, const int* robots, const int* map_ids, int* safe, int* first_hit, double* hit) {
  if (!c || n <= 0 || !robots || !map_ids) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, 0, "topay_track_safe")) return s;   // (in range, then the maps, then the trajectories)
  if (topay_status s = check_map_slots(c, n, map_ids, kMapResident | kMap2d | kMap3d, "topay_track_safe")) return s;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotEndTraj, "topay_track_safe")) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  return track_safe_impl(c, n, robots, map_ids, safe, first_hit, hit);
}

topay_status topay_track_safe_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  *ms = c->track.safe_ms;
  return TOPAY_OK;
}

topay_status topay_track_sample(topay_ctx* c, int n, const int* robots, int which, const int* map_ids, const int* time_off, const double* times, int what,
                                double* state, double* dstate, double* ee_pose, double* clearance, double* centres, double* duration, double* distance) {
  if (topay_status s = track_sample_check(c, n, robots, which, map_ids, what, "topay_track_sample")) return s;
  if (!time_off || time_off[0] != 0) { set_err("topay_track_sample: time_off must be given and start at 0"); return TOPAY_ERR_INVALID_ARG; }
  for (int k = 0; k < n; k++)
    if (time_off[k + 1] < time_off[k]) { set_err("topay_track_sample: time_off decreases"); return TOPAY_ERR_INVALID_ARG; }
  const std::vector<int> off(time_off, time_off + n + 1);
  if (off[(size_t)n] > 0 && (!times || !all_finite(times, (size_t)off[(size_t)n]))) {
    set_err("topay_track_sample: the times must be finite (below 1e9 in magnitude)");
    return TOPAY_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  static const double none = 0.0;   // (a call without samples is still a ragged call)
  const TrackSampleOuts U{state, dstate, ee_pose, clearance, centres, duration, distance};
  return track_sample_impl(c, n, robots, which - 1, map_ids, off, times ? times : &none, nullptr, 0.0, what, U);
}

topay_status topay_track_sample_grid(topay_ctx* c, int n, const int* robots, int which, const int* map_ids, const double* t0, double step, int m, int what,
                                     double* state, double* dstate, double* ee_pose, double* clearance, double* centres, double* duration, double* distance) {
  if (topay_status s = track_sample_check(c, n, robots, which, map_ids, what, "topay_track_sample_grid")) return s;
  if (!t0 || !all_finite(t0, (size_t)n) || !all_finite(&step, 1)) {
    set_err("topay_track_sample_grid: t0 and step must be finite (below 1e9 in magnitude)");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (m < 0 || (long long)n * m > 0x7fffffffll) { set_err("topay_track_sample_grid: m must not be negative, n * m below 2^31"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  std::vector<int> off((size_t)n + 1);
  for (int k = 0; k <= n; k++) off[(size_t)k] = k * m;
  const TrackSampleOuts U{state, dstate, ee_pose, clearance, centres, duration, distance};
  return track_sample_impl(c, n, robots, which - 1, map_ids, off, nullptr, t0, step, what, U);
}

topay_status topay_track_sample_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  *ms = c->track.sample_ms;
  return TOPAY_OK;
}

topay_status topay_replan_inputs(topay_ctx* c, int n, const int* robots, const double* t_since_replan, const double* t_since_begin,
                                 const double* global_goal, double planning_budget, double planning_horizon, double* start, double* start_v,
                                 double* goal, int* goal_source) {
  if (!c || n <= 0 || !robots || !t_since_replan || !t_since_begin || !global_goal || !start || !start_v || !goal || !goal_source) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_robot_slots(c, n, robots, kRobotEndTraj, "topay_replan_inputs")) return s;
  HIPCHK(hipSetDevice(c->device));
  return track_endpoints_impl(c, n, robots, t_since_replan, t_since_begin, global_goal, planning_budget, planning_horizon, start, start_v, goal, goal_source);
}

topay_status topay_replan_calls(topay_ctx* c, int n, const int* robots, const int* map_ids, const double* t_since_replan, const double* t_since_begin,
                                const double* now_xy, const double* global_goal, double replan_interval, double planning_budget,
                                double planning_horizon, const topay_plan_params_t* params, unsigned long long first_call, int* status,
                                double* endpoints, int* plan_result, int* plan_candidates) {
  if (!c || n <= 0 || !robots || !map_ids || !t_since_replan || !t_since_begin || !global_goal || !status) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_robot_slots(c, n, robots, 0, "topay_replan_calls")) != TOPAY_OK) return s;   // (in range, then the maps, then the trajectories)
  if ((s = check_map_slots(c, n, map_ids, kMapResident | kMap2d | kMap3d, "topay_replan_calls")) != TOPAY_OK) return s;
  if ((s = check_robot_slots(c, n, robots, kRobotEndTraj | kRobotDistinct, "topay_replan_calls")) != TOPAY_OK) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const size_t N = (size_t)n;
  // ---- 1. safety sweep (safeCallback) of every robot against its map of now
  std::vector<int> safe(N);
  if ((s = track_safe_impl(c, n, robots, map_ids, safe.data(), nullptr, nullptr)) != TOPAY_OK) return s;
  // ---- 2. trigger (replanCallback:649, 705-706)
  std::vector<int> trig;
  for (int r = 0; r < n; r++) {
    int* st = status + TOPAY_REPLAN_ST_LEN * (size_t)r;
    st[TOPAY_REPLAN_ST_OUTCOME] = 0; st[TOPAY_REPLAN_ST_SAFE] = safe[r]; st[TOPAY_REPLAN_ST_STORE_ROW] = -1; st[TOPAY_REPLAN_ST_GOAL_SOURCE] = -1;
    if (now_xy) {
      const double dx = now_xy[2 * (size_t)r] - global_goal[10 * (size_t)r], dy = now_xy[2 * (size_t)r + 1] - global_goal[10 * (size_t)r + 1];
      if (std::sqrt(dx * dx + dy * dy) < 0.5) { st[TOPAY_REPLAN_ST_OUTCOME] = 3; continue; }
    }
    if (t_since_replan[r] > replan_interval || !safe[r]) trig.push_back(r);
  }
  if (endpoints) std::fill(endpoints, endpoints + 30 * N, 0.0 / 0.0);
  if (plan_result) std::fill(plan_result, plan_result + TOPAY_PLAN_RES_LEN * N, 0);
  if (plan_candidates) std::fill(plan_candidates, plan_candidates + TOPAY_PLAN_CAND_ROW_LEN * N, 0);
  const int m = (int)trig.size();
  if (m == 0) return TOPAY_OK;
  // ---- 3. endpoints of the triggered robots
  const size_t M = (size_t)m;
  std::vector<int> rob(M), mid(M), src(M);
  std::vector<double> tr(M), tb(M), gg(10 * M), st10(10 * M), sv10(10 * M), go10(10 * M);
  std::vector<unsigned long long> call_no(M);
  for (int j = 0; j < m; j++) {
    const int r = trig[j];
    rob[j] = robots[r]; mid[j] = map_ids[r]; tr[j] = t_since_replan[r]; tb[j] = t_since_begin[r];
    memcpy(&gg[10 * (size_t)j], global_goal + 10 * (size_t)r, 80);
    call_no[j] = first_call + (unsigned long long)r;   // the robot's position among the n given, not among the triggered
  }
  if ((s = track_endpoints_impl(c, m, rob.data(), tr.data(), tb.data(), gg.data(), planning_budget, planning_horizon, st10.data(), sv10.data(), go10.data(),
                                src.data())) != TOPAY_OK)
    return s;
  // ---- 4. the planning call (planMomaParallel(local_start, local_goal, local_v))
  std::vector<int> res(TOPAY_PLAN_RES_LEN * M), cand(TOPAY_PLAN_CAND_ROW_LEN * M);
  if ((s = plan_calls_impl(c, m, mid.data(), st10.data(), go10.data(), sv10.data(), params, 0, call_no.data(), res.data(), cand.data(), nullptr)) != TOPAY_OK) return s;
  // ---- 5. winners become end_traj (planner.cpp:1010); global_traj stays
  std::vector<int> idx(M), done(M);
  std::iota(idx.begin(), idx.end(), 0);
  if ((s = track_commit_plan_impl(c, m, rob.data(), idx.data(), 1, done.data())) != TOPAY_OK) return s;
  for (int j = 0; j < m; j++) {
    const int r = trig[j];
    int* st = status + TOPAY_REPLAN_ST_LEN * (size_t)r;
    st[TOPAY_REPLAN_ST_OUTCOME] = done[j] ? 1 : 2; st[TOPAY_REPLAN_ST_STORE_ROW] = j; st[TOPAY_REPLAN_ST_GOAL_SOURCE] = src[j];
    if (endpoints) {
      memcpy(endpoints + 30 * (size_t)r, &st10[10 * (size_t)j], 80);
      memcpy(endpoints + 30 * (size_t)r + 10, &sv10[10 * (size_t)j], 80);
      memcpy(endpoints + 30 * (size_t)r + 20, &go10[10 * (size_t)j], 80);
    }
    if (plan_result) memcpy(plan_result + TOPAY_PLAN_RES_LEN * (size_t)r, &res[TOPAY_PLAN_RES_LEN * (size_t)j], TOPAY_PLAN_RES_LEN * sizeof(int));
    if (plan_candidates)
      memcpy(plan_candidates + TOPAY_PLAN_CAND_ROW_LEN * (size_t)r, &cand[TOPAY_PLAN_CAND_ROW_LEN * (size_t)j], TOPAY_PLAN_CAND_ROW_LEN * sizeof(int));
  }
  return TOPAY_OK;
}

}  // extern "C"
