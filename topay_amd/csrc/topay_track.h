// Tracked trajectories and the replanning cycle around the planning call: what Planner::safeCallback (planner.cpp:597-638)
// and Planner::replanCallback (704-750) do with the committed trajectory while the robot moves.
//   k_track_commit     MomaTraj::setTraj / the constructor (moma_traj_opt.h:40-110): a trajectory in the layout of
//                      topay_get_results into the arena, its car_seq prefix computed once (wave scan with carry, as the gate)
//   k_track_safe       safeCallback: samples every 0.01 s against the map slot given in the call, first violation
//   k_track_endpoints  replanCallback:708-731: start = getState(t_s), start_v = getDState(t_s) (moma_traj_opt.h:149-158),
//                      local goal = first state of global_traj beyond the horizon
//   k_track_sample     getState (moma_traj_opt.h:113-137), getDState (149-158), getFKPose (moma_param.h:339-373), the sphere
//                      centres (getColliPts, 203-247) and their distances at many times per robot: one wave per 64 samples
// One wave per trajectory / robot.  A tracked trajectory lies in the arena as
//   start[4] (x, y, theta, -) | T[N] | coef[9][6N] (element d * 6N + 6i + k = coefficient of t^k: what feas_* read) |
//   cseq[num + 1][2] (chassis xy after every 0.025 s Simpson panel)
#pragma once
#include "topay_ee.h"
#include "topay_feas.h"

namespace topay {

struct TrackDesc {
  long long off;   // first double of the trajectory in the arena
  int N;           // pieces; 0: the slot holds no such trajectory
  int num;         // Simpson panels = floor(T / 0.025)
};
__host__ __device__ inline long long track_doubles(int N, long long num) { return 4 + (long long)N + 54ll * N + 2 * (num + 1); }

__device__ __forceinline__ FeasIO track_io(const double* arena, const TrackDesc& D) {
  const double* base = arena + D.off;
  FeasIO F;
  F.x0 = base[0]; F.y0 = base[1]; F.th0 = base[2];
  F.T = base + 4;
  F.coef = base + 4 + D.N;
  F.N = D.N;
  F.cseq = const_cast<double*>(base + 4 + D.N + 54 * (long long)D.N);
  F.tk = nullptr;
  F.cap_panels = D.num; F.cap_samples = 0;
  F.report = nullptr; F.feasible = nullptr; F.truncated = nullptr;
  return F;
}
__device__ __forceinline__ double track_duration(const FeasIO& F) {   // getTotalDuration (minco.hpp:304-313)
  double Ttot = 0.0;
  for (int i = 0; i < F.N; i++) Ttot += F.T[i];
  return Ttot;
}

// MomaTraj::getState (moma_traj_opt.h:113-137) from the stored car_seq: the arithmetic of playback() in topay_feas.h
__device__ __forceinline__ void track_state(const FeasIO& F, double Ttot, double tg, double* o) {
  const double seq_res = 0.1;
  const int approx_res = 4;
  const int rows = 6 * F.N;
  tg = fmin(fmax(tg, 0.0), Ttot);
  const int index = (int)floor(tg / seq_res);
  const double floor_t = index * seq_res, diff_t = tg - floor_t;
  long long pidx = (long long)index * approx_res;
  if (pidx > F.cap_panels) pidx = F.cap_panels;
  double ix, iy;
  feas_simpson(F, floor_t, floor_t + diff_t / 2.0, tg, diff_t / 6.0, ix, iy);
  double tl = tg;
  const int i = feas_locate(F.T, F.N, tl);
  o[0] = F.cseq[2 * pidx] + ix;
  o[1] = F.cseq[2 * pidx + 1] + iy;
  o[2] = feas_pos(F.coef + 0 * rows + 6 * i, tl);
#pragma unroll
  for (int d = 0; d < 7; d++) o[3 + d] = feas_pos(F.coef + (2 + d) * rows + 6 * i, tl);
}
// MomaTraj::getDState (moma_traj_opt.h:149-158): (ds/dt, dtheta/dt, 0, dq/dt[7])
__device__ __forceinline__ void track_dstate(const FeasIO& F, double Ttot, double tg, double* o) {
  const int rows = 6 * F.N;
  tg = fmin(fmax(tg, 0.0), Ttot);
  const int i = feas_locate(F.T, F.N, tg);
  o[0] = feas_vel(F.coef + 1 * rows + 6 * i, tg);
  o[1] = feas_vel(F.coef + 0 * rows + 6 * i, tg);
  o[2] = 0.0;
#pragma unroll
  for (int d = 0; d < 7; d++) o[3 + d] = feas_vel(F.coef + (2 + d) * rows + 6 * i, tg);
}
// The running sum t, t + step, t + 2 step, ... of a reference loop `for (; t < T; t += step)`, 64 values per pass: every lane
// forms the same sums in the same order, keeps the one of its position and leaves with the value the next pass starts from.
__device__ __forceinline__ double track_times(double& t, double step, int lane) {
  double mine = t;
  for (int j = 0; j < 64; j++) {
    if (j == lane) mine = t;
    t += step;
  }
  return mine;
}

// One wave per trajectory k: piece src_piece[k] of (s_dur, s_coef) -- the layout of topay_get_results, per piece 9 x 6,
// highest order first -- and the start state at s_start + src_start[k] into the arena at dst[k]; then car_seq.
__global__ void __launch_bounds__(64) k_track_commit(int n, const TrackDesc* dst, const long long* src_piece, const long long* src_start,
                                                     const double* s_dur, const double* s_coef, const double* s_start, double* arena) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const TrackDesc D = dst[k];
  const int lane = threadIdx.x & 63, N = D.N, rows = 6 * N;
  if (N <= 0) return;
  double* base = arena + D.off;
  const long long sp = src_piece[k];
  if (lane < 4) base[lane] = lane < 3 ? s_start[src_start[k] + lane] : 0.0;
  for (int t = lane; t < N; t += 64) base[4 + t] = s_dur[sp + t];
  double* coef = base + 4 + N;
  constexpr int CP = kCoefPerPiece;
  for (int t = lane; t < N * CP; t += 64) {
    const int p = t / CP, r = t - CP * p, d = r / 6, kk = r - 6 * d;
    coef[(size_t)d * rows + 6 * p + 5 - kk] = s_coef[(size_t)sp * CP + t];
  }
  wave_global_sync();
  const FeasIO F = track_io(arena, D);
  const double Ttot = track_duration(F);
  // car_seq, as the gate computes it
  const double h = 0.1 / 4;
  long long num = (long long)floor(Ttot / h);
  if (!(Ttot > 0.0 && Ttot < 1.0e4)) num = 0;
  if (num > D.num) num = D.num;   // (the host sized the block from the same sum)
  feas_car_seq(F, num, lane);
}

struct TrackSafeArgs {
  int n;
  const TrackDesc* desc;   // [n] end_traj of every robot
  const double* arena;
  const int* map_id;       // [n]
  int* safe;               // [n]
  int* first_hit;          // [n][2] sample index, body (0 chassis, 1..12 spheres); -1, -1 when safe
  double* hit;             // [n][2] time, distance of that hit; NaN when safe
};

// safeCallback (planner.cpp:597-638): one wave per robot, lanes <-> samples t = 0, 0.01, ... (the reference's running sum).
// The wave leaves after the first pass of 64 samples that holds a violation.
__global__ void __launch_bounds__(64, 2) k_track_safe(TrackSafeArgs A, const DevMap* maps) {
  const int r = blockIdx.x;
  if (r >= A.n) return;
  dev_params_ref P = dev_params();
  const int lane = threadIdx.x & 63;
  const TrackDesc D = A.desc[r];
  const FeasIO F = track_io(A.arena, D);
  const TOPAY_GLB DevMap* mp = (const TOPAY_GLB DevMap*)(maps + __builtin_amdgcn_readfirstlane(A.map_id[r]));
  const DevMap M = load_map(mp);
  const double Ttot = track_duration(F);
  bool found = false;
  double t = 0.0;
  for (int s0 = 0; t < Ttot; s0 += 64) {
    const double tg = track_times(t, 0.01, lane);
    int body = -1;
    double dist = 0.0;
    if (tg < Ttot) {
      double st[10], Px[TOPAY_NSPH], Py[TOPAY_NSPH], Pz[TOPAY_NSPH];
      track_state(F, Ttot, tg, st);
      sphere_centres(st, Px, Py, Pz);
      // the first body in the reference's order: found by walking the order backwards
#pragma unroll
      for (int k = TOPAY_NSPH - 1; k >= 0; k--) {
        const double d = feas_dist3d(M, Px[k], Py[k], Pz[k]);
        if (d < P.sph_r[k] * 0.99) { body = k + 1; dist = d; }
      }
      const double d2 = feas_dist2d(M, st[0], st[1]);
      if (d2 < P.chassis_colli_radius * 0.99) { body = 0; dist = d2; }
    }
    const unsigned long long mask = __ballot(body >= 0);
    if (mask != 0ull) {
      const int first = __ffsll(mask) - 1;
      if (lane == first) {
        A.safe[r] = 0;
        A.first_hit[2 * r] = s0 + lane; A.first_hit[2 * r + 1] = body;
        A.hit[2 * r] = tg; A.hit[2 * r + 1] = dist;
      }
      found = true;
      break;
    }
  }
  if (!found && lane == 0) {
    A.safe[r] = 1;
    A.first_hit[2 * r] = -1; A.first_hit[2 * r + 1] = -1;
    A.hit[2 * r] = 0.0 / 0.0; A.hit[2 * r + 1] = 0.0 / 0.0;
  }
}

struct TrackEndArgs {
  int n;
  const TrackDesc* end_desc;    // [n]
  const TrackDesc* glob_desc;   // [n]; N = 0: no global_traj, the goal is global_goal
  const double* arena;
  const double* t_replan;       // [n] time since the last replan
  const double* t_begin;        // [n] time since global_traj began
  const double* global_goal;    // [n][10]
  double budget, horizon;
  double* start;                // [n][10]
  double* start_v;              // [n][10]
  double* goal;                 // [n][10]
  int* goal_source;             // [n]
};

// replanCallback:708-731, one wave per robot: lanes <-> the steps t = t_begin, += 0.1, while t < T_g of the walk along
// global_traj; a ballot finds the first state whose xy is more than the horizon from the start's.
__global__ void __launch_bounds__(64, 2) k_track_endpoints(TrackEndArgs A) {
  const int r = blockIdx.x;
  if (r >= A.n) return;
  const int lane = threadIdx.x & 63;
  const FeasIO E = track_io(A.arena, A.end_desc[r]);
  const double Te = track_duration(E);
  const double ts = A.t_replan[r] + A.budget;
  double st[10];
  track_state(E, Te, ts, st);   // (every lane: the walk compares against it)
  if (lane == 0) {
    double sv[10];
    track_dstate(E, Te, ts, sv);
    for (int a = 0; a < 10; a++) { A.start[10 * (size_t)r + a] = st[a]; A.start_v[10 * (size_t)r + a] = sv[a]; }
  }
  const TrackDesc GD = A.glob_desc[r];
  bool found = false;
  if (GD.N > 0) {
    const FeasIO G = track_io(A.arena, GD);
    const double Tg = track_duration(G);
    double t = A.t_begin[r];
    for (int s0 = 0; t < Tg; s0 += 64) {
      const double tg = track_times(t, 0.1, lane);
      double gs[10];
      bool beyond = false;
      if (tg < Tg) {
        track_state(G, Tg, tg, gs);
        const double dx = gs[0] - st[0], dy = gs[1] - st[1];
        beyond = sqrt(dx * dx + dy * dy) > A.horizon;
      }
      const unsigned long long mask = __ballot(beyond);
      if (mask != 0ull) {
        const int first = __ffsll(mask) - 1;
        if (lane == first) {
          for (int a = 0; a < 10; a++) A.goal[10 * (size_t)r + a] = gs[a];
          A.goal_source[r] = s0 + lane;
        }
        found = true;
        break;
      }
    }
  }
  if (!found && lane == 0) {
    for (int a = 0; a < 10; a++) A.goal[10 * (size_t)r + a] = A.global_goal[10 * (size_t)r + a];
    A.goal_source[r] = -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// topay_track_sample: the tracked trajectories of n robots at many times each.  The bits of `what` (TOPAY_SAMPLE_* of
// include/topay.h) select the outputs; a row of an output belongs to one sample.
// ---------------------------------------------------------------------------------------------------------------------
enum : int { kSampleState = 1, kSampleDState = 2, kSampleEePose = 4, kSampleClearance = 8, kSampleCentres = 16, kSampleDistance = 32 };
constexpr int kSampleBodies = 1 + TOPAY_NSPH;   // chassis, spheres

// One work item = one wave: `count` <= 64 consecutive samples of one robot of the call, rows row0 .. row0 + count - 1 of the
// outputs.  The host flattens the ragged ranges into these, so a robot with 1000 samples and one with 1 share no trip count.
// Every robot has an item, also one without samples (count 0): its first item writes the robot's duration.
struct TrackSampleItem {
  int robot;       // position among the n robots of the call
  int row0;
  int count;
  int head;        // the robot's first item
  double t_first;  // grid calls: the running sum t0, += step up to sample row0 of the robot, formed by the host
};
struct TrackSampleArgs {
  int n_items, what;
  const TrackSampleItem* items;
  const TrackDesc* desc;    // [n]
  const double* arena;
  const int* map_id;        // [n]; read only for kSampleClearance / kSampleDistance
  const double* times;      // [rows]; null: a grid call, sample j of an item at t_first, += step (track_times)
  double step;
  double *state, *dstate, *ee_pose, *clearance, *centres, *duration, *distance;   // null or of the call's rows (duration: [n])
};

// A row of R doubles, contiguous per lane, as 16-byte stores (R odd: and one of 8).  Rows are 8-byte aligned only (9 and 13
// doubles per row; a caller's device tensor), which global stores of this width take.
typedef double track_pair __attribute__((vector_size(16), aligned(8)));
template <int R> __device__ __forceinline__ void track_store_row(double* dst, const double (&v)[R]) {
#ifndef TOPAY_CPU_EMU
#pragma unroll
  for (int a = 0; a + 1 < R; a += 2) {
    track_pair p;
    p[0] = v[a]; p[1] = v[a + 1];
    *(TOPAY_GLB track_pair*)(dst + a) = p;
  }
  if (R & 1) dst[R - 1] = v[R - 1];
#else
  for (int a = 0; a < R; a++) dst[a] = v[a];
#endif
}

// Lanes <-> samples.  LEVEL is what the launch needs at most: 0 getState / getDState, 1 and getFKPose, 2 and the twelve
// spheres with their lookups -- three kernels, so that a call for states alone does not hold the registers of the walk along
// the arm.  Inside a kernel `what` (wave-uniform) selects; an output whose bit is clear is neither computed nor written.
// Every figure is the device function of its other user: track_state / track_dstate (k_track_endpoints), ee_pose_of (k_ee_pose),
// sphere_centres, feas_dist2d / feas_dist3d (k_track_safe).  No LDS: a lane's row is contiguous (80 bytes of a state), so the
// 16-byte stores of a wave fill whole lines of its 5 KB between them; a transposed write through LDS would add a round trip
// to save nothing but the order in which those lines fill.
template <int LEVEL>
__global__ void __launch_bounds__(64, 2) k_track_sample(TrackSampleArgs A, const DevMap* maps) {
  const int it = blockIdx.x;
  if (it >= A.n_items) return;
  const int lane = threadIdx.x & 63;
  const TrackSampleItem I = A.items[it];
  const int k = __builtin_amdgcn_readfirstlane(I.robot), count = __builtin_amdgcn_readfirstlane(I.count);
  const int what = A.what;
  const FeasIO F = track_io(A.arena, A.desc[k]);
  const double Ttot = track_duration(F);
  if (I.head && lane == 0 && A.duration) A.duration[k] = Ttot;
  double tg;
  if (A.times) tg = lane < count ? A.times[(size_t)I.row0 + lane] : 0.0;
  else {
    double t = I.t_first;
    tg = track_times(t, A.step, lane);
  }
  if (lane >= count) return;
  const size_t row = (size_t)I.row0 + lane;
  if (what & kSampleDState) {
    double sv[10];
    track_dstate(F, Ttot, tg, sv);
    track_store_row<10>(A.dstate + 10 * row, sv);
  }
  if (!(what & ~kSampleDState)) return;
  double st[10];
  track_state(F, Ttot, tg, st);
  if (what & kSampleState) track_store_row<10>(A.state + 10 * row, st);
  if (LEVEL >= 1 && (what & kSampleEePose)) {
    double po[9];
    ee_pose_of(dev_params(), st, po);
    track_store_row<9>(A.ee_pose + 9 * row, po);
  }
  if (LEVEL >= 2 && (what & (kSampleClearance | kSampleCentres | kSampleDistance))) {
    dev_params_ref P = dev_params();
    double Px[TOPAY_NSPH], Py[TOPAY_NSPH], Pz[TOPAY_NSPH];
    sphere_centres(st, Px, Py, Pz);
    if (what & kSampleCentres) {
      double cc[3 * TOPAY_NSPH];
#pragma unroll
      for (int s = 0; s < TOPAY_NSPH; s++) { cc[3 * s] = Px[s]; cc[3 * s + 1] = Py[s]; cc[3 * s + 2] = Pz[s]; }
      track_store_row<3 * TOPAY_NSPH>(A.centres + 3 * TOPAY_NSPH * row, cc);
    }
    if (what & (kSampleClearance | kSampleDistance)) {
      const TOPAY_GLB DevMap* mp = (const TOPAY_GLB DevMap*)(maps + __builtin_amdgcn_readfirstlane(A.map_id[k]));
      const DevMap M = load_map(mp);
      // the twelve lookups are independent and branch-free (esdf3d_query): unrolled, their gathers go out ahead of the arithmetic
      double d[kSampleBodies];
#pragma unroll
      for (int s = 0; s < TOPAY_NSPH; s++) d[1 + s] = feas_dist3d(M, Px[s], Py[s], Pz[s]);
      d[0] = feas_dist2d(M, st[0], st[1]);
      if (what & kSampleDistance) track_store_row<kSampleBodies>(A.distance + kSampleBodies * row, d);
      if (what & kSampleClearance) {
        double cl[kSampleBodies];
        cl[0] = d[0] - P.chassis_colli_radius;
#pragma unroll
        for (int s = 0; s < TOPAY_NSPH; s++) cl[1 + s] = d[1 + s] - P.sph_r[s];
        track_store_row<kSampleBodies>(A.clearance + kSampleBodies * row, cl);
      }
    }
  }
}

}  // namespace topay
