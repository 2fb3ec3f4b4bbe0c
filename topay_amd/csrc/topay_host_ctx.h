// Host side of the C-ABI, part 1: the error text, owning device buffers (grow-and-discard, grow-and-keep), the carver of packed
// blocks and the stopwatch (DevTimer), the launch-class table, the state of every subject as one struct each (PlanStore, PlanWork,
// FrontState, TrackState, EeState, WorldState, SenseState, MpcState, EdtState), the context, parameters, create and destroy.

#pragma once

static thread_local std::string g_err;
static void set_err(const std::string& s) { g_err = s; }
#define HIPCHK(call)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      set_err(std::string(#call) + ": " + hipGetErrorString(e_));                                \
      return TOPAY_ERR_NO_DEVICE;                                                                \
    }                                                                                            \
  } while (0)

// From the environment the library reads TOPAY_PERSISTENT / TOPAY_STEAL (launch scheme, used by the profiling scripts and
// the parity tests) and TOPAY_RCCL_LIB, and it sets GPU_MAX_HW_QUEUES when it is loaded; nothing else.

// The layout of a packed block, stated once: a list of take<T>(count) in the order of the sub-arrays.  Run on a null base it
// gives the byte count (`off`), run on the buffer it gives the pointers (DevBuf::carve does both).
struct Carver {
  uintptr_t base;
  size_t off = 0;
  explicit Carver(void* b = nullptr) : base((uintptr_t)b) {}
  template <typename T> T* take(size_t count) {
    off = (off + alignof(T) - 1) & ~(alignof(T) - 1);
    T* q = (T*)(base + off);
    off += count * sizeof(T);
    return q;
  }
};

// A device buffer that owns its memory: freed when it goes out of scope (the early returns of the HIPCHK macro included) or with
// the context it is a member of.  Move-only.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  topay_status ensure(size_t n) {
    if (n <= bytes) return TOPAY_OK;
    release();
    const hipError_t e_ = hipMalloc(&p, n);
    if (e_ != hipSuccess) {
      p = nullptr;
      set_err("device allocation of " + std::to_string(n >> 20) + " MiB failed: " + hipGetErrorString(e_));
      return TOPAY_ERR_NO_DEVICE;
    }
    bytes = n;
    return TOPAY_OK;
  }
  // ensure() that keeps the first `used` bytes when it has to grow (at least doubling): the append of the plan store, of a
  // try's init paths and of the tracked trajectories' arena.  The copy runs on `stream` and is waited for.
  topay_status ensure_keep(hipStream_t stream, size_t need, size_t used) {
    if (need <= bytes) return TOPAY_OK;
    DevBuf nb;
    const topay_status s = nb.ensure(std::max(need, 2 * bytes));
    if (s != TOPAY_OK) return s;
    if (used > 0 && p) {
      hipError_t e = hipMemcpyAsync(nb.p, p, used, hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) { set_err(std::string("grow_keep: ") + hipGetErrorString(e)); return TOPAY_ERR_NO_DEVICE; }
    }
    *this = std::move(nb);
    return TOPAY_OK;
  }
  void release() {   // free early on purpose (a map slot being refilled, an arena, a workspace that is no longer needed)
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T> T* as() { return (T*)p; }
  template <typename F> topay_status carve(F&& lay) {   // a packed block: sized by its layout, then the layout's pointers set
    Carver size;
    lay(size);
    const topay_status s = ensure(size.off);
    Carver at(p);
    if (s == TOPAY_OK) lay(at);
    return s;
  }
  template <typename B> topay_status place(B& block) {   // ... whose layout is the block's own lay(Carver&)
    return carve([&](Carver& k) { block.lay(k); });
  }
};

// A stopwatch on a stream: a pair of events that it owns, created on first use and destroyed with it.  Move-only, like DevBuf.
// Every timed stage has one of its own, so no stage's time is overwritten by another's records.
struct DevTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool stopped = false;   // stop() has been recorded since the last start()
  DevTimer() = default;
  DevTimer(const DevTimer&) = delete; DevTimer& operator=(const DevTimer&) = delete;
  DevTimer(DevTimer&& o) noexcept { *this = std::move(o); }
  DevTimer& operator=(DevTimer&& o) noexcept {
    if (this != &o) { release(); a = o.a; b = o.b; stopped = o.stopped; o.a = o.b = nullptr; o.stopped = false; }
    return *this;
  }
  ~DevTimer() { release(); }
  hipError_t start(hipStream_t stream) {
    stopped = false;
    hipError_t e = a ? hipSuccess : hipEventCreate(&a);
    if (e == hipSuccess && !b) e = hipEventCreate(&b);
    return e == hipSuccess ? hipEventRecord(a, stream) : e;
  }
  hipError_t stop(hipStream_t stream) {
    const hipError_t e = hipEventRecord(b, stream);
    stopped = e == hipSuccess;
    return e;
  }
  // milliseconds between start and stop, once the stream has been waited for; an error when this start was never stopped
  hipError_t read(double* ms) const {
    float f = 0.f;
    const hipError_t e = stopped ? hipEventElapsedTime(&f, a, b) : hipErrorNotReady;
    if (e == hipSuccess) *ms = f;
    return e;
  }
  void release() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
    stopped = false;
  }
};

// Launch buckets by number of pieces: upper bounds (inclusive) = one bucket per kernel template (rows per lane 1 / 2 / 3 / 4 / 6).
// Each bucket is one launch on its own stream so that they run concurrently.  All streams have the SAME priority:
// mixed priorities made the hardware preempt (context-save) the low-priority waves whenever high-priority work
// arrived, and twice in ~80 runs one low-priority launch was starved for tens of seconds.  HIP maps the streams of one
// priority onto a pool of GPU_MAX_HW_QUEUES (default 4) hardware queues shared by every stream of the process, and
// streams that share a queue serialise (tools/queue_probe.hip); the library asks for 24 queues at load time (below: three contexts in
// flight use 18, and another library's stream -- RCCL's -- that lands on the queue of a persistent solve launch waits a
// whole solve; 32 and more are time-sliced by the scheduler firmware)
// when the environment does not say otherwise.  With one wave per SIMD, four workgroups of the common classes (<= 21 /
// 27 / 36 / 54 KB per wave) share a CU's 160 KB; the two rare classes of long candidates (<= 70 / 104 KB) cost their CU a
// slot or two, which is why they are kept apart from each other.
static const int kBucketMaxN[TOPAY_NBUCKET] = {10, 15, 21, 32, 42, 64, TOPAY_MAX_N};
// Launch classes are finer than kernel templates where that saves LDS: the two-rows-per-lane kernel serves N <= 15 with
// 27 KB and N <= 21 with 36 KB per workgroup (most candidates of the benchmark have 11..15 pieces).  LDS is what
// limits how many workgroups a CU hosts beside a long candidate's: giving every class-1 workgroup the 38 KB of class 2
// cost 8 % of the throughput, taking 9 KB from most of the two-rows workgroups pays the other way.
static const int kBigFirst = 4;   // the classes of long candidates (N > 32) start here

// Kernel of a launch class: rows per thread and waves per trajectory select the template; the LDS is sized by the
// longest candidate actually in the class.
typedef void (*solve_kernel_t)(DevBatch, const DevMap*, int);
typedef void (*eval_kernel_t)(DevBatch, const DevMap*, int, int, int);
struct ClassDef {
  int max_n, rmax, nw;   // rows per thread and waves of an EVALUATION of the class (= threads of its workgroups / 64)
  solve_kernel_t solve;
  eval_kernel_t eval;
  int occ = 2;   // waves per SIMD the kernel is built for (512 / occ registers per lane; every kernel: 256, no AGPRs)
  solve_kernel_t lat = nullptr;   // helper-wave kernel of a one-wave class (topay_set_latency_mode): 4 waves per workgroup
  // The solver runs on ONE wave in every class; its rows per lane (elements per lane / 2) are what the bits of a solve depend on
  // (topay_class_of).  0 = as the evaluation.  The long classes run it on wave 0 of a four-wave workgroup whose other waves
  // join the evaluations only (helper waves, topay_solve.h).
  int solver_rmax = 0;
  int srmax() const { return solver_rmax ? solver_rmax : rmax; }
  bool helpers() const { return nw > 1; }   // `solve` is a helper-wave kernel: its LDS carries the command block
};
static const int kLatWaves = 4;
// N <= 32: one wave per trajectory.  N = 33..170: the evaluations on four waves (round 4: the long candidates set the length
// of a batch), the solver on wave 0 alone with 10 / 28 vector elements per lane (round 5: every reduction of a four-wave
// solver was a workgroup reduction through LDS and a barrier).  Figures: docs/EXPERIMENTS.md.
static const ClassDef kClassTable[TOPAY_NBUCKET] = {
    {10, 1, 1, k_solve1, k_eval1, 2, k_lat1}, {15, 2, 1, k_solve2, k_eval2, 2, k_lat2}, {21, 2, 1, k_solve2, k_eval2, 2, k_lat2},
    {32, 3, 1, k_solve3, k_eval3, 2, k_lat3},
    {42, 2, 4, k_long5, k_eval2w4, 2, nullptr, 5}, {64, 2, 4, k_long5, k_eval2w4, 2, nullptr, 5},
    {TOPAY_MAX_N, 4, 4, k_long14, k_eval4w4, 2, nullptr, 14}};
// work per SIMD-second of the two-waves-per-SIMD classes relative to one wave per SIMD (sizes the launches only; assumed
// 1.0 / 1.2 / 1.4 / 1.7 / 2.0 gave 10.0k / 10.2k / 10.5k / 10.8k / 10.6k trajectories/s, docs/EXPERIMENTS.md)
static const double kOcc2Gain = 1.7;
static const int kLdsDoublesPerCU = 160 * 1024 / 8;
static size_t class_lds_bytes(const ClassDef& cd, int nm) {
  return (size_t)(eval_lds_total(nm, cd.nw) + solve_tail_doubles(cd.helpers())) * sizeof(double);
}

// Runs when the library is loaded: effective if the HIP runtime has not been initialised yet in this process
// (the runtime reads the variable once, at its first call).  A caller that initialises HIP first should export
// GPU_MAX_HW_QUEUES=24 itself.
__attribute__((constructor)) static void topay_request_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "24", 0); }
// Dispatch gate (topay_optimize_async): the context whose solve was issued last in this process.
struct topay_ctx;
static std::mutex g_issue_mutex;
// Every live context of the process (topay_create / topay_destroy), for push_params.
static std::mutex g_registry_mutex;
static std::vector<topay_ctx*> g_contexts;

static topay_ctx* g_last_issued = nullptr;

// The winners of the last topay_plan_calls, kept on the device until the next one.  Nothing outside this struct knows how they
// lie in the four buffers: a winner's pieces are contiguous (1 duration and kCoefPerPiece coefficients per piece); its N + 1
// knots follow those of the winners before it, as k_gather_results lays them out, so the winners stored so far take
// 2 (pieces + winners) doubles; an init path holds 10 doubles per state.
struct PlanStore {
  struct Entry { int n_pieces = 0, piece0 = 0, knot0 = 0, front0 = 0, front_len = 0; };   // a call without a winner: zeros
  struct Winners {   // of one try: call, index in the solved batch, and the running piece / init-path state offsets (W + 1 each)
    std::vector<int> call, idx, piece_off{0}, front_off{0};
    void add(int p, int b, int n_pieces, int front_len) {
      call.push_back(p); idx.push_back(b);
      piece_off.push_back(piece_off.back() + n_pieces); front_off.push_back(front_off.back() + front_len);
    }
    size_t size() const { return idx.size(); }
  };
  struct Dest { double *dur, *coef, *knots, *front; };   // where k_gather_results and k_plan_gather_front write a try's winners

  void reset(int n_calls) { calls.assign((size_t)n_calls, Entry()); pieces = winners = states = 0; }
  void clear() { calls.clear(); }   // a planning call that failed leaves nothing to read
  bool empty() const { return calls.empty(); }   // no planning call has been run
  bool has(int call) const { return call >= 0 && call < (int)calls.size(); }
  const Entry& entry(int call) const { return calls[(size_t)call]; }
  size_t n_pieces() const { return pieces; }
  double* durations() { return dur.as<double>(); }
  double* coeffs() { return coef.as<double>(); }
  double* knots() { return kn.as<double>(); }
  double* fronts() { return front.as<double>(); }
  static long long front_double0(const Entry& e) { return 10ll * e.front0; }

  // Room for W behind what is stored (the buffers grow keeping their contents), the entries of its calls, and the
  // destinations of the gathers.  The counts move with appended(), once the gathers have succeeded.
  topay_status reserve(hipStream_t stream, const Winners& W, Dest& d) {
    const size_t np = (size_t)W.piece_off.back(), nw = W.size(), ns = (size_t)W.front_off.back();
    for (size_t w = 0; w < nw; w++) {
      Entry& e = calls[(size_t)W.call[w]];
      e.n_pieces = W.piece_off[w + 1] - W.piece_off[w];
      e.piece0 = (int)pieces + W.piece_off[w];
      e.knot0 = (int)pieces + (int)winners + W.piece_off[w] + (int)w;
      e.front0 = (int)states + W.front_off[w];
      e.front_len = W.front_off[w + 1] - W.front_off[w];
    }
    topay_status s;
    if ((s = dur.ensure_keep(stream, (pieces + np) * 8, pieces * 8)) != TOPAY_OK ||
        (s = coef.ensure_keep(stream, (pieces + np) * kCoefPerPiece * 8, pieces * kCoefPerPiece * 8)) != TOPAY_OK ||
        (s = kn.ensure_keep(stream, 2 * (pieces + winners + np + nw) * 8, 2 * (pieces + winners) * 8)) != TOPAY_OK ||
        (s = front.ensure_keep(stream, (states + ns) * 80, states * 80)) != TOPAY_OK)
      return s;
    d.dur = durations() + pieces; d.coef = coeffs() + kCoefPerPiece * pieces; d.knots = knots() + 2 * (pieces + winners); d.front = fronts() + 10 * states;
    return TOPAY_OK;
  }
  void appended(const Winners& W) { pieces += (size_t)W.piece_off.back(); winners += W.size(); states += (size_t)W.front_off.back(); }

 private:
  DevBuf dur, coef, kn, front;
  std::vector<Entry> calls;   // per call of the last topay_plan_calls: where its winner lies
  size_t pieces = 0, winners = 0, states = 0;
};

// What a try of topay_plan_calls works in (topay_host_plan.h states the blocks' layouts), and the stage clock (PlanClock).
struct PlanWork {
  DevBuf raw, jps_io;     // raw paths of the roadmap and of JPS in one buffer; the JPS launcher's own block
  DevBuf io, tab, mc;     // per front-end launch: the calls, candidate table + dense paths, search inputs / outputs
  DevBuf paths, bvel;     // the try's init paths and boundary velocities, appended launch by launch
  DevBuf idx, win;        // index block of the hand-off to the solver, then of the store; winner block
  std::vector<DevTimer> timers;   // PlanClock: one stopwatch per timed stretch of a call, and the stage each one counts for
  std::vector<int> timer_stage;
  double stage_ms[TOPAY_PLAN_MS_LEN] = {0};
  int chunk = 0;   // topay_plan_test_chunk: calls per front-end launch, 0 = the constant
};

// The joint-space search and the roadmap (topay_host_front.h): node tables, Reeds-Shepp words and inputs of the last
// topay_mcrrt_plan (topay_mcrrt_nodes); graphs, raw paths and point buffers of the last topay_topo_paths (topay_topo_graph /
// _raw_paths) with what sized them, and the stopwatch of k_topo when the planning call does not bring its own.
struct FrontState {
  DevBuf mc_i, mc_d, mc_k, mc_rs, mc_in;
  int mc_n = 0, mc_node_cap = 0;
  DevBuf tp_i, tp_d, tp_raw, tp_pts, tp_io;
  int tp_n = 0, tp_pt_cap = 0, tp_nbuf = 0;
  topay_topo_params_t tp_P;
  DevTimer tp_timer;
};

// Tracked trajectories (topay_host_track.h): the arena, the slots' descriptors (host: what the kernels are handed per call),
// the upload block of topay_track_set, the inputs / outputs of the sweep, endpoint and sampling kernels, the device time of the
// last k_track_safe and of the last k_track_sample launch.
struct TrackSlot { topay::TrackDesc d[2] = {{0, 0, 0}, {0, 0, 0}}; long long cap[2] = {0, 0}; double T[2] = {0, 0}; };   // [0] end_traj, [1] global_traj
struct TrackState {
  DevBuf arena, stage, io;
  size_t used = 0;   // doubles of the arena handed out
  std::vector<TrackSlot> slots;
  DevTimer safe_timer, sample_timer;
  double safe_ms = 0.0, sample_ms = 0.0;
  const topay::TrackDesc* find(int robot, int w) const { return slots.empty() || slots[robot].d[w].N <= 0 ? nullptr : &slots[robot].d[w]; }
};

// End-effector goals (topay_host_ee.h): the L-BFGS history of the last topay_ee_goals (kept until the next call), the inputs /
// outputs of the ee kernels, the device time of the last topay_ee_goals.
struct EeState {
  DevBuf hist, io;
  DevTimer timer;
  double ms = 0.0;
};

// topay_generate_worlds / topay_generate_episodes (topay_host_world.h): the occupancy grids of the last call stay for
// topay_get_occupancy (slots [first, first + n) of dimensions dims), its primitive lists and its inputs / outputs; the rasteriser
// path it took (1: masks in LDS, 2: byte stores) and its device time by stage (generation, rasterisation, fields, sampling).
struct WorldState {
  DevBuf occ, prims, io;
  int first = 0, n = 0, dims[3] = {0, 0, 0}, path = 0;
  int force_path = 0, max_tries = 0;   // test hooks: 2 = byte stores whatever the map; tries per arm of an episode (0: 2000)
  enum { kGen, kRaster, kFields, kSample };
  DevTimer timer[4];
  double ms[4] = {0, 0, 0, 0};
  // the three grids of the call lie one after the other, each on a 16-byte boundary (the first path stores 16 bytes at a time)
  static size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
  const signed char* occ3_of(int slot, int* d) const {
    if (n <= 0 || slot < first || slot >= first + n || !occ.p) return nullptr;
    for (int a = 0; a < 3; a++) d[a] = dims[a];
    return (const signed char*)occ.p + (size_t)(slot - first) * dims[0] * dims[1] * dims[2];
  }
  const signed char* occ2_of(int slot, bool critical) const {   // (of a slot that has an occ3_of: after the 3-D grids, then the 2-D ones)
    const size_t n2 = (size_t)dims[0] * dims[1], b3 = pad16((size_t)n * n2 * dims[2]), b2 = pad16((size_t)n * n2);
    return (const signed char*)occ.p + b3 + (critical ? b2 : 0) + (size_t)(slot - first) * n2;
  }
  // slots [first_, first_ + n_) are refilled by something else than the world generator: its grids no longer describe them
  void forget(int first_, int n_) {
    if (n > 0 && first_ < first + n && first < first_ + n_) { n = 0; occ.release(); }
  }
};

// Sensor clouds (topay_host_sense.h): per map slot the belief (log-odds, packed counts and cache box in one block), the batch
// counter, the rays counted since the last flush and the parameters of the last insert (topay_sense_commit reads l_occ and
// chassis_height from them); the uploads of a call; the points of the last topay_sense_scan; the occupancy grids of the last
// topay_sense_commit and where each slot's lie in them (topay_get_occupancy); the device time of the last scan, insert, flush
// and commit with the fields; the scratch image of topay_sense_slide (the log-odds of the slots that moved in the largest call so
// far, never a second copy per slot) and the device time of its last call.
struct SenseBelief {
  DevBuf buf;
  float* logodds = nullptr; int* cnt = nullptr; int* box = nullptr;
  topay_map_desc_t desc;
  topay_sense_params_t prm;
  int batch_counter = 0, pending_rays = 0;
  size_t occ3_off = 0, occ2_off = 0, occ2c_off = 0;
  bool have = false, have_occ = false;
};
struct SenseState {
  std::vector<SenseBelief> slot;   // sized by the first topay_sense_reset
  DevBuf pts, io, scan, occ, slide;
  size_t scan_points = 0;
  enum { kScan, kInsert, kFlush, kCommit };
  DevTimer timer[4], slide_timer;
  double ms[4] = {0, 0, 0, 0}, slide_ms = 0;
  bool has_belief(int m) const { return m >= 0 && m < (int)slot.size() && slot[m].have; }
  bool has_occ(int m) const { return m >= 0 && m < (int)slot.size() && slot[m].have_occ; }
  const signed char* occ3_of(int m, int* d) const {
    if (!has_occ(m)) return nullptr;
    for (int a = 0; a < 3; a++) d[a] = slot[m].desc.dims[a];
    return (const signed char*)occ.p + slot[m].occ3_off;
  }
  const signed char* occ2_of(int m, bool critical) const { return (const signed char*)occ.p + (critical ? slot[m].occ2c_off : slot[m].occ2_off); }
  // slots [first, first + n) are refilled: the grids of the last commit no longer describe them
  void forget(int first, int n) {
    for (int m = first; m < first + n && m < (int)slot.size(); m++) slot[m].have_occ = false;
  }
};

// The tracking controller and the fake robot (topay_host_mpc.h): OMPC's and moma_sim's state per robot slot (allocated by the
// first reset, zero = never reset), the host's copy of each slot's parameters, the uploads / outputs of a call, the dense QP
// of topay_mpc_probe, the device time of the last topay_mpc_cmds / topay_track_follow.
struct MpcState {
  DevBuf slots, sims, io, dense;
  std::vector<topay_mpc_params_t> prm;
  std::vector<char> have, sim_have;
  DevTimer timer;
  double ms = 0.0;
  topay_status alloc(hipStream_t stream) {   // the two slot arrays, zeroed, by the first reset
    if (slots.p) return TOPAY_OK;
    topay_status s;
    if ((s = slots.ensure(sizeof(topay::MpcSlot) * TOPAY_TRACK_SLOTS)) != TOPAY_OK) return s;
    if ((s = sims.ensure(sizeof(topay::SimSlot) * TOPAY_TRACK_SLOTS)) != TOPAY_OK) return s;
    HIPCHK(hipMemsetAsync(slots.p, 0, slots.bytes, stream));
    HIPCHK(hipMemsetAsync(sims.p, 0, sims.bytes, stream));
    HIPCHK(hipStreamSynchronize(stream));
    prm.resize(TOPAY_TRACK_SLOTS);
    have.assign(TOPAY_TRACK_SLOTS, 0);
    sim_have.assign(TOPAY_TRACK_SLOTS, 0);
    return TOPAY_OK;
  }
};

// The ESDF construction (topay_host_maps.h): the uploaded occupancy grids, its workspace (released once the fields sit in
// their slots) and the device time of the last build.
struct EdtState {
  DevBuf occ, thr, tmp1, tmp2, v, z, out2;
  DevTimer timer;
  double ms = 0.0;
};

struct topay_ctx {
  int device = 0;
  topay_params_t hp;
  DevParams dp;
  hipStream_t stream = nullptr;
  // maps
  std::vector<DevMap> hmaps = std::vector<DevMap>(TOPAY_MAX_MAPS);
  std::vector<DevBuf> map2d = std::vector<DevBuf>(TOPAY_MAX_MAPS), map3d = std::vector<DevBuf>(TOPAY_MAX_MAPS);
  std::vector<DevBuf> map2d_inf = std::vector<DevBuf>(TOPAY_MAX_MAPS), map2d_crit = std::vector<DevBuf>(TOPAY_MAX_MAPS);
  // Maps built on the device as a batch live in one arena per build call (the construction writes the fields where
  // they stay; the slots' descriptors point into it), kept until the context is destroyed.
  struct MapArena { DevBuf buf; int first = 0, n = 0; };
  std::vector<MapArena> map_arenas;
  DevBuf dmaps;
  std::vector<char> have_map = std::vector<char>(TOPAY_MAX_MAPS, 0);
  // topay_share_maps: slot m of this context refers to the fields of map_owner[m] (null: its own); map_sharers = the
  // contexts that refer to slots of this one.  When the owner refills or frees a slot, the sharers' slots are invalidated
  // (have_map 0 -> TOPAY_ERR_NO_MAP) after their pending solves have finished: no context keeps a dangling descriptor.
  std::vector<topay_ctx*> map_owner = std::vector<topay_ctx*>(TOPAY_MAX_MAPS, nullptr);
  std::vector<topay_ctx*> map_sharers;
  std::vector<int> h_map_id;   // map slot of every candidate of the resident batch
  std::vector<int> h_path_len; // init-path states of every candidate (launch order inside a class)
  // batch
  int B = 0, Nmax = 0, total_states = 0, Pmax = 0;
  // pieces / decision-vector elements of the candidates before b (packed per-candidate blocks, DevBatch::poff / noff)
  std::vector<long long> h_poff, h_noff;
  DevBuf poff, noff;
  size_t workspace_bytes = 0;   // device memory of the resident batch (topay_workspace_bytes)
  // per-trajectory N (0 = not representable, skipped); launch buckets by N (LDS is sized per bucket)
  std::vector<int> hN;
  static constexpr int NBUCKET = TOPAY_NBUCKET;
  std::vector<int> cls[NBUCKET];
  hipStream_t bstream[NBUCKET] = {nullptr};
  hipEvent_t bevent[NBUCKET] = {nullptr};
  hipEvent_t bstart = nullptr;
  bool pending = false;  // a topay_optimize_async has been issued and not yet waited for
  int* h_started = nullptr;  // pinned host counter the solve kernels bump once per candidate (dispatch gate)
  int n_launched = 0;        // candidates the pending solve launched
  int n_gate = 0;            // ... of which the dispatch gate waits for (the classes of up to 32 pieces)
  int latency_mode = 0;        // topay_set_latency_mode: 0 never, 1 batches of at most one candidate per SIMD, 2 always
  bool gate_done = false;      // the resident flags / report are those of the last solve
  // cancellation: planning call of every candidate, the window after a call's first feasible success (piece-evaluations)
  std::vector<int> h_group;
  int n_groups = 0, cancel_budget = 0;
  DevBuf group_id, group_tau, interrupted;
  int* h_cancel = nullptr;     // pinned: topay_cancel
  // the one exchange of the multi-GPU path: all-gather of per-scenario records over RCCL (topay_comm_init)
  void* comm = nullptr;        // ncclComm_t
  int comm_world = 0, comm_rank = 0;
  hipStream_t comm_stream = nullptr;
  DevBuf comm_send, comm_recv;
  int gate_timeouts = 0;     // times the dispatch gate gave up waiting (topay_gate_timeouts)
  bool persistent = true;    // solve launches: one workgroup per SIMD slot pulling candidates from a queue
  bool steal = true;         // ... and draining the smaller classes' queues once its own is empty (TOPAY_STEAL=0: profiling)
  int simd_slots = 1024;
  DevBuf qnext;
  DevBuf paths, path_off, path_len, bvel, bacc, scratch;
  DevBuf N, s1_past, map_id, head, tail, start_xy, goal_xy, init_xy, x0;
  DevBuf x, work, hist_s, hist_y, hist_ys, hist_alpha, lu;
  DevBuf success, cost, stats, xyerr, coef, T, knots, alm, fout, order, trace, elapsed, startus, hwid, sbuf, mstash, feas_cseq, feas_tk, feas_report, feas_flags, pb_io;
  DevTimer solve_timer, eval_timer;   // the solve (topay_optimize_async ... topay_synchronize) and topay_eval_batch
  // the subjects beside the resident batch and the solver, one struct each (above)
  FrontState front;
  PlanWork plan;          // topay_plan_calls: what a try works in, the stage clock
  PlanStore plan_store;   // ... and the winners of the last call
  TrackState track;
  EeState ee;
  WorldState world;
  SenseState sense;
  MpcState mpc;
  EdtState edt;
  int trace_cap = 0;
  DevBatch db;
  bool have_traj = false, solved = false;
  double last_ms = 0.0;
  int last_launches = 0, last_helper_launches = 0;
};

static DevLbfgs to_dev_lbfgs(const topay_lbfgs_params_t& a) {
  DevLbfgs b;
  b.mem_size = a.mem_size; b.past = a.past; b.max_iterations = a.max_iterations; b.max_linesearch = a.max_linesearch;
  b.g_epsilon = a.g_epsilon; b.delta = a.delta; b.min_step = a.min_step; b.max_step = a.max_step;
  b.f_dec_coeff = a.f_dec_coeff; b.s_curv_coeff = a.s_curv_coeff; b.cautious_factor = a.cautious_factor;
  b.machine_prec = a.machine_prec;
  return b;
}

// finite and below `bound` in magnitude (include/topay.h states the bound of every entry that checks its inputs with this)
static bool all_finite(const double* v, size_t n, double bound = 1.0e9) {
  for (size_t i = 0; i < n; i++)
    if (!(std::fabs(v[i]) < bound)) return false;
  return true;
}

static void make_dev_params(const topay_params_t& p, DevParams& d) {
  memset(&d, 0, sizeof(d));
  d.relu_mu = p.relu_mu;
  {
    const double pe = p.relu_mu;
    d.sl_half = 0.5 * pe;
    d.sl_f3c = 1.0 / (pe * pe);
    d.sl_f4c = -0.5 * d.sl_f3c / pe;
    d.sl_d2c = 3.0 * d.sl_f3c;
    d.sl_d3c = 4.0 * d.sl_f4c;
  }
  for (int i = 0; i < 9; i++) d.energy_weights[i] = p.energy_weights[i];
  d.s1_time_weight = p.s1_time_weight; d.s1_moment_weight = p.s1_moment_weight; d.s1_acc_weight = p.s1_acc_weight;
  d.s1_domega_weight = p.s1_domega_weight; d.s1_path_pos_weight = p.s1_path_pos_weight;
  d.s2_time_weight = p.s2_time_weight; d.s2_moment_weight = p.s2_moment_weight; d.s2_acc_weight = p.s2_acc_weight;
  d.s2_domega_weight = p.s2_domega_weight; d.s2_collision_weight = p.s2_collision_weight;
  d.s2_mani_colli_weight = p.s2_mani_colli_weight; d.s2_self_colli_weight = p.s2_self_colli_weight;
  d.s2_mani_pos_weight = p.s2_mani_pos_weight; d.s2_mani_vel_weight = p.s2_mani_vel_weight;
  d.s2_mani_acc_weight = p.s2_mani_acc_weight; d.s2_mean_time_weight = p.s2_mean_time_weight;
  for (int i = 0; i < 2; i++) {
    d.alm_init_lambda[i] = p.alm_init_lambda[i]; d.alm_init_rho[i] = p.alm_init_rho[i];
    d.alm_rho_max[i] = p.alm_rho_max[i]; d.alm_gamma[i] = p.alm_gamma[i];
  }
  d.alm_tolerance = p.alm_tolerance;
  d.alm_max_outer = p.alm_max_outer;
  d.alm_work_budget = p.alm_work_budget;
  d.min_piece_num = p.min_piece_num;
  d.sample_interval = p.sample_interval;
  d.s1_normal_past = p.s1_normal_past; d.s1_shot_path_past = p.s1_shot_path_past;
  d.s1_shot_path_horizon = p.s1_shot_path_horizon;
  d.s1_lbfgs = to_dev_lbfgs(p.s1_lbfgs);
  d.s2_lbfgs = to_dev_lbfgs(p.s2_lbfgs);
  d.chassis_height = p.chassis_height; d.chassis_colli_radius = p.chassis_colli_radius;
  d.max_v = p.max_v; d.max_a = p.max_a; d.max_w = p.max_w; d.max_dw = p.max_dw;
  for (int i = 0; i < 8; i++) d.colli_length[i] = p.colli_length[i];
  int s = 0;
  for (int i = 0; i < 16 && s < TOPAY_NSPH; i++)
    if (p.colli_points[i] != 0.0) {  // moma_param.h:217-218
      d.sph_off[s] = p.colli_points[i];
      d.sph_r[s] = p.colli_point_radius[i];
      s++;
    }
  for (int i = 0; i < 7; i++) {
    d.joint_pos_limit_max[i] = p.joint_pos_limit_max[i];
    d.joint_vel_limit[i] = p.joint_vel_limit[i];
    d.joint_acc_limit[i] = p.joint_acc_limit[i];
  }
  for (int i = 0; i < 9; i++) d.relR[i] = p.relative_R[i];
  for (int i = 0; i < 3; i++) d.relT[i] = p.relative_t[i];
  // derived constants (DevParams): the expressions of the evaluation, operation by operation (this file is compiled with
  // -ffp-contract=off like the device code, so the host's products and sums are the device's)
  for (int a = 0; a < TOPAY_NSPH; a++)
    for (int b = 0; b < TOPAY_NSPH; b++) {
      const double rr = d.sph_r[a] + d.sph_r[b];
      d.pair_rr2[a * TOPAY_NSPH + b] = rr * rr;
    }
  for (int k = 0; k < TOPAY_NSPH; k++) {
    d.sph_viol[k] = d.sph_r[k] * 10.0 * 1.1;
    d.sph_top[k] = d.chassis_height + d.relT[2] + d.sph_r[k];
  }
  d.p0z = d.chassis_height + d.relT[2];
  d.max_vw = d.max_v * d.max_w;
  d.max_a2 = d.max_a * d.max_a;
  d.max_dw2 = d.max_dw * d.max_dw;
  d.chassis_r105 = d.chassis_colli_radius * 1.05;
  for (int i = 0; i < 7; i++) {
    d.joint_vel_limit2[i] = d.joint_vel_limit[i] * d.joint_vel_limit[i];
    d.joint_acc_limit2[i] = d.joint_acc_limit[i] * d.joint_acc_limit[i];
  }
}

static int sphere_layout_ok(const topay_params_t& p) {
  // the kernels hard-wire MomaParam's sphere-per-link layout {2,1,2,1,2,1,2,1}
  const int want[8] = {2, 1, 2, 1, 2, 1, 2, 1};
  for (int i = 0; i < 8; i++) {
    int c = (p.colli_points[2 * i] != 0.0) + (p.colli_points[2 * i + 1] != 0.0);
    if (c != want[i]) return 0;
    if (want[i] == 1 && p.colli_points[2 * i] != 0.0) return 0;
  }
  return 1;
}

// Every copy goes through the context's own (non-blocking) stream: null-stream operations would wait for the solves of
// every other context of the process (and they for it), which serialises batches that are meant to overlap.
// A solve in flight is waited for first by every entry that touches its inputs, reads its results or times a launch of its own.
static topay_status wait_pending(topay_ctx* c) { return c->pending ? topay_synchronize(c) : TOPAY_OK; }

static hipError_t memcpy_sync(topay_ctx* c, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, n, kind, c->stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(c->stream);
}
// Typed copies of `count` elements on the same stream, the byte count from the pointer type: synchronous like memcpy_sync
// (which stays for what really is a byte count: a struct, a whole buffer) ...
template <typename T> static hipError_t copy_sync(topay_ctx* c, T* dst, const T* src, size_t count, hipMemcpyKind kind) {
  return memcpy_sync(c, dst, src, count * sizeof(T), kind);
}
template <typename T> static hipError_t h2d_sync(topay_ctx* c, T* dst, const T* src, size_t count) {
  return copy_sync(c, dst, src, count, hipMemcpyHostToDevice);
}
template <typename T> static hipError_t d2h_sync(topay_ctx* c, T* dst, const T* src, size_t count) {
  return copy_sync(c, dst, src, count, hipMemcpyDeviceToHost);
}
// ... and asynchronous.
template <typename T> static hipError_t h2d(topay_ctx* c, T* dst, const T* src, size_t count) {
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream);
}
template <typename T> static hipError_t d2h(topay_ctx* c, T* dst, const T* src, size_t count) {
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream);
}

static topay_status validate_params(const topay_params_t* params) {
  if (params->int_K != TOPAY_K) { set_err("int_K must be 12 in this build"); return TOPAY_ERR_UNSUPPORTED; }
  if (!sphere_layout_ok(*params)) { set_err("unsupported collision sphere layout"); return TOPAY_ERR_UNSUPPORTED; }
  if (params->s1_lbfgs.mem_size <= 0 || params->s2_lbfgs.mem_size <= 0 || params->s1_lbfgs.mem_size > kLbfgsMaxMem ||
      params->s2_lbfgs.mem_size > kLbfgsMaxMem || params->s1_lbfgs.past > 8 ||
      params->s2_lbfgs.past > 8 || params->s1_shot_path_past > 8 || params->s1_normal_past > 8) {
    set_err("lbfgs mem_size must be in 1..256 (the reference uses 256) and past <= 8");
    return TOPAY_ERR_INVALID_ARG;
  }
  return TOPAY_OK;
}

static topay_status create_device_state(topay_ctx* c, int device) {
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&c->bstart));
  // One stream per launch class (the last class runs on the main stream), all non-blocking and never the null stream:
  // two contexts then use ten of the sixteen hardware queues the library asks for, and no operation of one context
  // waits for another context's solve.
  for (int k = 0; k < topay_ctx::NBUCKET; k++) {
    // (the two longest classes start on the main stream: streams are hardware queues, and 3 contexts x 7 streams beside
    // torch's and RCCL's exceed the 24 the library asks for -- a gather that shares a queue with a persistent solve
    // launch waits a whole solve, 9.1k instead of 10.0k trajectories/s through the RCCL path.  The N <= 64 class gets a
    // stream of its own the first time a batch also holds candidates of more than 64 pieces, launch_classes.)
    if (k >= topay_ctx::NBUCKET - 2) c->bstream[k] = c->stream;
    else HIPCHK(hipStreamCreateWithFlags(&c->bstream[k], hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->bevent[k]));
  }
  {
    { const char* se = getenv("TOPAY_STEAL"); c->steal = !(se && se[0] == '0'); }
    const char* pe = getenv("TOPAY_PERSISTENT");
    c->persistent = !(pe && pe[0] == '0');
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->simd_slots = 4 * prop.multiProcessorCount;   // four SIMDs per CU; a class built for two waves per SIMD launches two workgroups per slot
    // Every slot is used.  Nothing is left to what is not a solve (the init kernel, the feasibility gate and the result
    // gather of the OTHER batches in flight, the runtime's copy kernels, a collective), although resident solver waves own
    // their SIMD's whole register file and such a kernel waits until workgroups exit: measured, no gain from a standing
    // reserve with two batches in flight.
  }
  {
    void* hp = nullptr;
    HIPCHK(hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent));
    c->h_started = (int*)hp;
    c->h_started[0] = 0;
    c->h_cancel = c->h_started + 8;   // same pinned block: topay_cancel's flag
    c->h_cancel[0] = 0;
  }
  if (c->dmaps.ensure(sizeof(DevMap) * TOPAY_MAX_MAPS) != TOPAY_OK) return TOPAY_ERR_NO_DEVICE;
  memset(c->hmaps.data(), 0, sizeof(DevMap) * TOPAY_MAX_MAPS);
  return TOPAY_OK;
}

// The owner is about to refill (or free) slots [first, first + n): every context that shares one of them finishes its
// pending solve and loses the slot.
static void invalidate_sharers(topay_ctx* owner, int first, int n) {
  std::vector<topay_ctx*> sharers;
  {
    std::lock_guard<std::mutex> lk(g_registry_mutex);
    sharers = owner->map_sharers;
  }
  for (topay_ctx* s : sharers) {
    bool hit = false;
    for (int m = first; m < first + n; m++) hit = hit || s->map_owner[m] == owner;
    if (!hit) continue;
    (void)wait_pending(s);
    for (int m = first; m < first + n; m++)
      if (s->map_owner[m] == owner) {
        s->map_owner[m] = nullptr;
        s->have_map[m] = 0;
        memset(&s->hmaps[m], 0, sizeof(DevMap));
        // a resident batch that uses the slot cannot be solved, evaluated or gated any more: it has to be set again
        if (s->have_traj && std::find(s->h_map_id.begin(), s->h_map_id.end(), m) != s->h_map_id.end()) { s->have_traj = false; s->solved = false; }
      }
    bool any = false;
    for (int m = 0; m < TOPAY_MAX_MAPS; m++) any = any || s->map_owner[m] == owner;
    if (!any) {
      std::lock_guard<std::mutex> lk(g_registry_mutex);
      owner->map_sharers.erase(std::remove(owner->map_sharers.begin(), owner->map_sharers.end(), s), owner->map_sharers.end());
    }
  }
}
// slots [first, first + n) of c stop referring to another context's fields (c fills them itself, or goes away)
static void drop_shared_slots(topay_ctx* c, int first, int n) {
  std::lock_guard<std::mutex> lk(g_registry_mutex);
  for (int m = first; m < first + n; m++) {
    topay_ctx* o = c->map_owner[m];
    if (!o) continue;
    c->map_owner[m] = nullptr;
    bool any = false;
    for (int q = 0; q < TOPAY_MAX_MAPS; q++) any = any || c->map_owner[q] == o;
    if (!any) o->map_sharers.erase(std::remove(o->map_sharers.begin(), o->map_sharers.end(), c), o->map_sharers.end());
  }
}

// slots [first, first + n) are refilled: neither the world generator's occupancy grids nor the last commit's describe them any more
static void forget_occupancy(topay_ctx* c, int first, int n) {
  c->sense.forget(first, n);
  c->world.forget(first, n);
}

static int bucket_of(int N) {
  for (int k = 0; k < topay_ctx::NBUCKET; k++)
    if (N <= kBucketMaxN[k]) return k;
  return topay_ctx::NBUCKET - 1;
}

// what the __constant__ parameter block of each device holds (last push)
static DevParams g_pushed_dp[16];
static bool g_pushed_valid[16] = {false};
static topay_status push_params(topay_ctx* c) {
  // Contexts of one process may carry different parameters, and the kernels read them from one __constant__ block for
  // as long as they run: refresh it before every launch, and if a solve of another context with *different*
  // parameters is still in flight on this device, let it finish first (contexts with equal parameters overlap freely).
  {
    std::lock_guard<std::mutex> lk(g_registry_mutex);
    for (topay_ctx* q : g_contexts)
      if (q != c && q->pending && q->device == c->device && memcmp(&q->dp, &c->dp, sizeof(DevParams)) != 0) {
        HIPCHK(hipStreamSynchronize(q->stream));
      }
  }
  HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_P), &c->dp, sizeof(DevParams), 0, hipMemcpyHostToDevice, c->stream));
  g_pushed_dp[c->device % 16] = c->dp;
  g_pushed_valid[c->device % 16] = true;
  return TOPAY_OK;
}

extern "C" {

const char* topay_last_error(void) { return g_err.c_str(); }

topay_status topay_default_params(topay_params_t* p) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  memset(p, 0, sizeof(*p));
  // src/planner/params/optimizer.yaml
  p->int_K = 12; p->min_piece_num = 3; p->relu_mu = 1.0e-3; p->sample_interval = 1.5;
  const double ew[9] = {0.33, 1, 1, 1, 1, 1, 1, 1, 1};
  for (int i = 0; i < 9; i++) p->energy_weights[i] = ew[i];
  p->s1_time_weight = 20.0; p->s1_moment_weight = 1000.0; p->s1_acc_weight = 1000.0; p->s1_domega_weight = 1000.0;
  p->s1_path_pos_weight = 200000.0; p->s1_normal_past = 2; p->s1_shot_path_past = 8; p->s1_shot_path_horizon = 0.5;
  auto lb = [](topay_lbfgs_params_t& l) {  // lbfgs.hpp:15-129 defaults
    l.mem_size = 8; l.g_epsilon = 1.0e-5; l.past = 3; l.delta = 1.0e-6; l.max_iterations = 0; l.max_linesearch = 64;
    l.min_step = 1.0e-20; l.max_step = 1.0e+20; l.f_dec_coeff = 1.0e-4; l.s_curv_coeff = 0.9; l.cautious_factor = 1.0e-6;
    l.machine_prec = 1.0e-16;
  };
  lb(p->s1_lbfgs); lb(p->s2_lbfgs);
  p->s1_lbfgs.mem_size = 256; p->s1_lbfgs.g_epsilon = 0.0; p->s1_lbfgs.min_step = 0.0; p->s1_lbfgs.delta = 1.0e-2;
  p->s1_lbfgs.max_iterations = 8000; p->s1_lbfgs.past = 2;
  p->s2_lbfgs.mem_size = 256; p->s2_lbfgs.past = 3; p->s2_lbfgs.g_epsilon = 0.0; p->s2_lbfgs.min_step = 1.0e-32;
  p->s2_lbfgs.delta = 1.0e-4; p->s2_lbfgs.max_iterations = 8000;
  p->s2_time_weight = 50.0; p->s2_moment_weight = 300.0; p->s2_acc_weight = 3000.0; p->s2_domega_weight = 3000.0;
  p->s2_collision_weight = 500000.0; p->s2_mani_colli_weight = 500000.0; p->s2_self_colli_weight = 500000.0;
  p->s2_mani_pos_weight = 500.0; p->s2_mani_vel_weight = 500.0; p->s2_mani_acc_weight = 500.0;
  p->s2_mean_time_weight = 5000.0;
  for (int i = 0; i < 2; i++) {
    p->alm_init_lambda[i] = 0.0; p->alm_init_rho[i] = 1.0e4; p->alm_rho_max[i] = 1.0e10; p->alm_gamma[i] = 9.0;
  }
  p->alm_tolerance = 0.01;
  p->alm_max_outer = 30;
  p->alm_work_budget = 24000;
  // src/simulator/fake_moma/include/fake_moma/moma_param.h:36-126
  p->chassis_height = 0.155; p->chassis_colli_radius = 0.4;
  p->max_v = 1.0; p->max_a = 0.8; p->max_w = 1.25; p->max_dw = 1.0;
  const double cl[8] = {0.139, 0.1015, 0.1525, 0.1035, 0.1285, 0.0815, 0.144, 0.05};
  const double cp[16] = {0.139 - 0.09, 0.139, 0.0, 0.1015, 0.1525 - 0.08, 0.1525, 0.0, 0.1035,
                         0.1285 - 0.07, 0.1285, 0.0, 0.0815, 0.144 - 0.07, 0.144, 0.0, 0.1};
  const double cr[16] = {0.06, 0.06, 0.0, 0.08, 0.04, 0.04, 0.0, 0.07, 0.035, 0.035, 0.0, 0.06, 0.035, 0.035, 0.0, 0.08};
  for (int i = 0; i < 8; i++) p->colli_length[i] = cl[i];
  for (int i = 0; i < 16; i++) {
    p->colli_points[i] = cp[i];
    p->colli_point_radius[i] = (cr[i] > 1e-4 && cr[i] < 0.055) ? 0.055 : cr[i];  // moma_param.h:110-112
  }
  const double qm[7] = {3.1, 2.26, 3.1, 2.355, 3.1, 2.23, 6.28};
  for (int i = 0; i < 7; i++) { p->joint_pos_limit_max[i] = qm[i]; p->joint_vel_limit[i] = 2.35; p->joint_acc_limit[i] = 6.28; }
  const double rr[9] = {0.7071068, 0.7071068, 0.0, -0.7071068, 0.7071068, 0.0, 0.0, 0.0, 1.0};
  for (int i = 0; i < 9; i++) p->relative_R[i] = rr[i];
  p->relative_t[0] = 0.0; p->relative_t[1] = 0.115; p->relative_t[2] = 0.016;
  return TOPAY_OK;
}

topay_status topay_set_params(topay_ctx* c, const topay_params_t* params) {
  if (!c || !params) return TOPAY_ERR_INVALID_ARG;
  topay_status vs = validate_params(params);
  if (vs != TOPAY_OK) return vs;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  // what the resident batch was laid out with: number of pieces (init step) and history depth (workspace)
  const bool relayout = params->sample_interval != c->hp.sample_interval || params->min_piece_num != c->hp.min_piece_num ||
                        std::max(params->s1_lbfgs.mem_size, params->s2_lbfgs.mem_size) != std::max(c->hp.s1_lbfgs.mem_size, c->hp.s2_lbfgs.mem_size) ||
                        params->max_v != c->hp.max_v || params->max_a != c->hp.max_a || params->max_w != c->hp.max_w || params->max_dw != c->hp.max_dw;
  c->hp = *params;
  make_dev_params(*params, c->dp);
  if (relayout) { c->have_traj = false; c->solved = false; }
  return TOPAY_OK;
}

topay_status topay_create(const topay_params_t* params, int device, topay_ctx** out) {
  if (!params || !out) return TOPAY_ERR_INVALID_ARG;
  { topay_status vs = validate_params(params); if (vs != TOPAY_OK) return vs; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_err("no HIP device available: the MI355X HIP path is required (there is no CPU fallback)");
    return TOPAY_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { set_err("device index out of range"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(device));
  topay_ctx* c = new topay_ctx();
  c->device = device;
  c->hp = *params;
  make_dev_params(*params, c->dp);
  // a failure below releases what has been created so far (topay_destroy copes with a partly built context)
  const topay_status st = create_device_state(c, device);
  if (st != TOPAY_OK) { topay_destroy(c); return st; }
  {
    std::lock_guard<std::mutex> lk(g_registry_mutex);
    g_contexts.push_back(c);
  }
  *out = c;
  return TOPAY_OK;
}

void topay_destroy(topay_ctx* c) {
  if (!c) return;
  (void)wait_pending(c);
  invalidate_sharers(c, 0, TOPAY_MAX_MAPS);
  drop_shared_slots(c, 0, TOPAY_MAX_MAPS);
  {
    std::lock_guard<std::mutex> lk(g_registry_mutex);
    g_contexts.erase(std::remove(g_contexts.begin(), g_contexts.end(), c), g_contexts.end());
  }
  (void)hipSetDevice(c->device);
  for (int k = 0; k < topay_ctx::NBUCKET; k++) {
    if (c->bevent[k]) (void)hipEventDestroy(c->bevent[k]);
    if (c->bstream[k] && c->bstream[k] != c->stream) (void)hipStreamDestroy(c->bstream[k]);
  }
  {
    std::lock_guard<std::mutex> lk(g_issue_mutex);
    if (g_last_issued == c) g_last_issued = nullptr;
  }
  (void)topay_comm_destroy(c);
  if (c->h_started) (void)hipHostFree(c->h_started);
  if (c->bstart) (void)hipEventDestroy(c->bstart);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;   // the device buffers and the stopwatches are members: freed here
}

topay_status topay_params_from_yaml(const char* path_or_text, topay_params_t* params, char* ignored, int ignored_cap) {
  if (!path_or_text || !params) return TOPAY_ERR_INVALID_ARG;
  std::string ign, err;
  const topay_status s = topay_yaml::apply_source(path_or_text, params, ign, err);
  if (s != TOPAY_OK) { set_err("topay_params_from_yaml: " + err); return s; }
  if (ignored && ignored_cap > 0) {
    strncpy(ignored, ign.c_str(), (size_t)ignored_cap - 1);
    ignored[ignored_cap - 1] = 0;
  }
  return TOPAY_OK;
}

}  // extern "C"
