// Sensor clouds into the map: rog_map's ProbMap (src/rog_map/src/rog_map/prob_map.cpp) on the grid of a map slot, and a range
// sensor that makes clouds from a slot whose occupancy is known.
//   k_sense_select     raycastProcess steps 1.1 and 1.2 (prob_map.cpp:686-696) when the intensity filter is on: which points of a
//                      cloud survive, in cloud order (ballot per wave, totals per tile through LDS, a running base per cloud)
//   k_sense_rays       steps 1.3, 1.4 and the ray loop (698-779): one lane per surviving point; every touched voxel gets one
//                      vector atomic add on a packed word, operation count in the low half, hit count in the high half
//   k_sense_box_gather the cache boxes of a call's slots in one array, for the host to size the flush launch by
//   k_sense_flush      probabilisticMapFromCache / hitPointUpdate / missPointUpdate (544-664): one lane per voxel of the batch's
//                      cache box (the voxels the batch's rays touched, whatever path they took: nothing else holds a count)
//   k_sense_box_reset  the cache box of a slot that has been flushed becomes empty
//   k_sense_occupancy  the belief as occ3d / occ2d / occ2d_critical (isOccupied, prob_map.h:129; the 2-D rule of
//                      GridMap::cloudCallback, grid_map.cpp:554-568, with the voxel centre as the point)
//   k_sense_slide      SlidingMap::mapSliding (sliding_map.cpp:113-166): the belief moved by whole voxels into a scratch image, what
//                      enters the window unknown
//   k_sense_scan       the range sensor: one lane per ray through occ3d (not a restatement: pointcloud_render_node needs PCL)
// Frame.  The reference indexes its world frame, floor(p / resolution) with centres at + 0.5 (ORIGIN_AT_CORNER, CMakeLists.txt:14;
// raycaster.cpp:46-63, sliding_map.cpp:175-203).  Here every position is first moved into the map's frame, u = p - origin (the
// grid is GridMap::init's, grid_map.cpp:20-60), and the reference's code runs on u: its local map is voxels 0 .. dims - 1, its
// local_map_bound_min/max_d the centres of the first and last voxel (sliding_map.cpp:93-95).
// The counts are integers and a voxel takes one float addition per flush, so the belief does not depend on the order in which
// the rays of a batch arrive.  Tail of a wave: the lanes whose rays have ended idle until the longest ray of the wave has
// (range / resolution steps per axis at the most, about 87 at 5 m and 0.1 m for a diagonal ray); neighbouring points of a scan
// are neighbouring rays, so the spread inside a wave is the depth relief of 64 adjacent rays.  Rays are not re-dealt.
#pragma once
#include "topay_math.h"
#include "topay_types.h"

namespace topay {

#define TOPAY_SENSE_BLOCK 256
// most rays a voxel can be counted by between two flushes: a ray counts a voxel once while it passes and once as its hit, and the
// low half of the packed word holds 65535
#define TOPAY_SENSE_MAX_BATCH_RAYS 32767

struct SenseP {
  float l_hit, l_miss, l_min, l_max, l_occ, l_free;
  double range_min, range_max, sqr_range_max;
  double ceil_height, ground_height;   // world frame, as the parameter file gives them
  int half_box[3];                     // half_local_update_box_i (config.hpp:378-379)
  int filt, thresh;
};
struct SenseSlot {
  double origin[3], res, res_inv;
  int dims[3];
  int flush;          // this call ends the slot's batch
  double sensor[3];   // world frame
  float* logodds;     // [nx][ny][nz]
  int* cnt;           // packed counts, same layout
  int* box;           // cache box of the batch in voxels: min x, y, z, then -max x, y, z (both reduced with atomicMin)
  int cloud_begin, cloud_len, skip, pad;   // the slot's points; skip: the sensor is above the ceiling / below the ground
};
struct SenseOccSlot {
  const float* logodds;
  signed char *occ3, *occ2, *occ2c;
  double z0, res, chassis_height;
  float l_occ;
  int dims[3];
};
struct SenseScanSlot {
  const signed char* occ3;
  double origin[3], res;
  int dims[3], pad;
  double pose[4];   // x, y, z, yaw
};
struct SenseSlideSlot {
  const float* src;   // the belief's log-odds, [nx][ny][nz]
  float* dst;         // the shifted image, same layout, in the context's scratch
  int dims[3], shift[3];
};
struct alignas(16) SensePoint { float x, y, z, i; };

// ---- RayCaster (src/rog_map/include/utils/raycaster.cpp:65-192), corner-origin branch ------------------------------------
struct SenseRay {
  int cur[3], end[3], dir[3];
  double t_bound[3], t_step[3];
};
__host__ __device__ inline int sense_floor_div(double d, double res) { return (int)floor(d / res); }   // posToIndex, raycaster.cpp:46-49
// setInput (65-147).  false: start and end share a voxel (the reference's callers go on to step(), which then ends at once).
__host__ __device__ inline bool sense_ray_set(SenseRay& R, const double* start, const double* end, double res) {
  const double big = 1.7976931348623157e308;   // numeric_limits<double>::max()
  bool any = false;
  for (int a = 0; a < 3; a++) {
    R.cur[a] = sense_floor_div(start[a], res);
    R.end[a] = sense_floor_div(end[a], res);
    const int delta = R.end[a] - R.cur[a];
    R.dir[a] = delta > 0 ? 1 : (delta < 0 ? -1 : 0);
    R.t_bound[a] = big;
    R.t_step[a] = big;
    any = any || R.dir[a] != 0;
  }
  if (!any) return false;
  double dis[3];
  for (int a = 0; a < 3; a++) dis[a] = fabs(end[a] - start[a]);
  const double t_max = sqrt(dis[0] * dis[0] + dis[1] * dis[1] + dis[2] * dis[2]);
  for (int a = 0; a < 3; a++) {
    dis[a] /= t_max;
    if (R.dir[a] == 0) continue;
    R.t_step[a] = fabs(res / dis[a]);
    const double centre = ((double)R.cur[a] + 0.5) * res;   // indexToPos, raycaster.cpp:56-59
    const double next_bound = centre + (double)R.dir[a] * res * 0.5;
    R.t_bound[a] = fabs(next_bound - start[a]) / dis[a];
  }
  return true;
}
// step (149-192): id = the voxel the ray is in; false when that is the end voxel, else the ray moves on
__host__ __device__ inline bool sense_ray_step(SenseRay& R, int* id) {
  id[0] = R.cur[0]; id[1] = R.cur[1]; id[2] = R.cur[2];
  if (R.cur[0] == R.end[0] && R.cur[1] == R.end[1] && R.cur[2] == R.end[2]) return false;
  int a;
  if (R.t_bound[0] < R.t_bound[1]) a = R.t_bound[0] < R.t_bound[2] ? 0 : 2;
  else a = R.t_bound[1] < R.t_bound[2] ? 1 : 2;
  // (indexed by constants: the arrays stay in registers)
  if (a == 0) { R.cur[0] += R.dir[0]; R.t_bound[0] += R.t_step[0]; }
  else if (a == 1) { R.cur[1] += R.dir[1]; R.t_bound[1] += R.t_step[1]; }
  else { R.cur[2] += R.dir[2]; R.t_bound[2] += R.t_step[2]; }
  return true;
}
__host__ __device__ inline bool sense_inside(const int* id, const int* dims) {   // insideLocalMap, sliding_map.cpp:78-83
  return id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[0] < dims[0] && id[1] < dims[1] && id[2] < dims[2];
}

// Steps 1.3 and 1.4 of raycastProcess (prob_map.cpp:714-746) for one point, in the map's frame: p moves to where its ray is
// cut, update_hit tells whether it still marks an obstacle.  s: the sensor; ceil_u / ground_u: the virtual heights in the frame.
__host__ __device__ inline void sense_clamp_point(const SenseP& P, const double* s, double ceil_u, double ground_u, const double* box_min,
                                                  const double* box_max, double* p, bool& update_hit) {
  update_hit = true;
  if (p[2] > ceil_u || p[2] < ground_u) {   // 1.3: cut at the virtual ceiling / ground
    update_hit = false;
    const double dz = p[2] - s[2], pc = (p[2] > ceil_u ? ceil_u : ground_u) - s[2];
    const double d[3] = {p[0] - s[0], p[1] - s[1], p[2] - s[2]};
    const double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double nrm = sqrt(n2);
    for (int a = 0; a < 3; a++) p[a] = s[a] + (n2 > 0.0 ? d[a] / nrm : d[a]) * pc / dz;   // normalized() * pc / dz
  }
  {   // 1.4: the range
    const double d[3] = {p[0] - s[0], p[1] - s[1], p[2] - s[2]};
    const double sqr_dis = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (sqr_dis > P.sqr_range_max) {
      const double k = P.range_max / sqrt(sqr_dis);
      for (int a = 0; a < 3; a++) p[a] = k * d[a] + s[a];
      update_hit = false;
    }
  }
  const double lo = fmin(fmin(p[0] - box_min[0], p[1] - box_min[1]), p[2] - box_min[2]);
  const double hi = fmax(fmax(p[0] - box_max[0], p[1] - box_max[1]), p[2] - box_max[2]);
  if (lo < 0.0 || hi > 0.0) {   // lineBoxIntersectPoint (common_lib.hpp:148-170)
    const double diff[3] = {p[0] - s[0], p[1] - s[1], p[2] - s[2]};
    double min_t = 1000000.0;
    for (int a = 0; a < 3; a++)
      if (fabs(diff[a]) > 0.0) {
        const double t1 = (box_max[a] - s[a]) / diff[a];
        if (t1 > 0.0 && t1 < min_t) min_t = t1;
        const double t2 = (box_min[a] - s[a]) / diff[a];
        if (t2 > 0.0 && t2 < min_t) min_t = t2;
      }
    for (int a = 0; a < 3; a++) p[a] = s[a] + (min_t - 1e-3) * diff[a];
    update_hit = false;
  }
}
// updateLocalBox (prob_map.cpp:792-822) in the map's frame: the box follows the sensor's voxel and stays inside the local map
__host__ __device__ inline void sense_local_box(const SenseP& P, const double* s, double res, double res_inv, const int* dims, double* box_min,
                                                double* box_max) {
  for (int a = 0; a < 3; a++) {
    const int si = (int)floor(s[a] * res_inv);   // posToGlobalIndex, sliding_map.cpp:181-183
    box_min[a] = fmax(((double)(si - P.half_box[a]) + 0.5) * res, 0.5 * res);
    box_max[a] = fmin(((double)(si + P.half_box[a]) + 0.5) * res, ((double)(dims[a] - 1) + 0.5) * res);
  }
}
__host__ __device__ inline bool sense_finite3(const double* v) {
  return fabs(v[0]) < 1.0e300 && fabs(v[1]) < 1.0e300 && fabs(v[2]) < 1.0e300;   // false for a NaN
}

#if defined(__HIPCC__) || defined(TOPAY_CPU_EMU)

__device__ __forceinline__ int sense_wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o < v ? o : v; }
  return v;
}

// Steps 1.1 and 1.2 with the intensity filter on: temperol_cnt counts the points that passed the filter, and a point survives when
// the count before it is a multiple of point_filt_num.  One workgroup per cloud walks it in tiles of its size; surv[cloud_begin + j]
// = index (in the cloud) of survivor j, n_surv[slot] = their number.
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_select(SenseP P, const SenseSlot* slots, const SensePoint* pts, int* surv, int* n_surv) {
  __shared__ int wave_pass[TOPAY_SENSE_BLOCK / TOPAY_WAVE], wave_keep[TOPAY_SENSE_BLOCK / TOPAY_WAVE];
  const SenseSlot S = slots[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & (TOPAY_WAVE - 1), wave = tid / TOPAY_WAVE, nw = blockDim.x / TOPAY_WAVE;
  int base_pass = 0, base_keep = 0;   // points that passed / survived in the tiles before this one (uniform over the block)
  for (int t0 = 0; t0 < S.cloud_len; t0 += blockDim.x) {
    const int i = t0 + tid;
    const bool pass = i < S.cloud_len && !(pts[S.cloud_begin + i].i < (float)P.thresh);
    const unsigned long long pb = __ballot(pass);
    const int before_w = __popcll(pb & ((1ull << lane) - 1ull));
    if (lane == 0) wave_pass[wave] = __popcll(pb);
    __syncthreads();
    int before = base_pass + before_w, tile_pass = 0;
    for (int w = 0; w < nw; w++) { if (w < wave) before += wave_pass[w]; tile_pass += wave_pass[w]; }
    const bool keep = pass && before % P.filt == 0;
    const unsigned long long kb = __ballot(keep);
    if (lane == 0) wave_keep[wave] = __popcll(kb);
    __syncthreads();
    int pos = base_keep + __popcll(kb & ((1ull << lane) - 1ull)), tile_keep = 0;
    for (int w = 0; w < nw; w++) { if (w < wave) pos += wave_keep[w]; tile_keep += wave_keep[w]; }
    if (keep) surv[S.cloud_begin + pos] = i;
    base_pass += tile_pass;
    base_keep += tile_keep;
    __syncthreads();   // the totals are rewritten by the next tile
  }
  if (tid == 0) n_surv[blockIdx.x] = base_keep;
}

// One lane per surviving point.  blocks_per_slot blocks serve a slot, so a wave never spans two slots.  surv == nullptr: the
// intensity filter is off and survivor j is point j * point_filt_num.
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_rays(SenseP P, const SenseSlot* slots, int blocks_per_slot, const SensePoint* pts,
                                                                  const int* surv, const int* n_surv) {
  const int slot = blockIdx.x / blocks_per_slot, j = (blockIdx.x - slot * blocks_per_slot) * blockDim.x + threadIdx.x;
  const SenseSlot S = slots[slot];
  const bool active = !S.skip && j < n_surv[slot];
  const int big = 0x7f7f7f7f;
  int mn[3] = {big, big, big}, mx[3] = {-big, -big, -big};
  if (active) {
    const int pi = surv ? surv[S.cloud_begin + j] : j * P.filt;
    const SensePoint q = pts[S.cloud_begin + pi];
    double s[3], p[3], box_min[3], box_max[3];
    for (int a = 0; a < 3; a++) s[a] = S.sensor[a] - S.origin[a];
    p[0] = (double)q.x - S.origin[0]; p[1] = (double)q.y - S.origin[1]; p[2] = (double)q.z - S.origin[2];
    if (sense_finite3(p)) {   // (a NaN or an infinity is counted by the filters like any point and casts no ray)
      sense_local_box(P, s, S.res, S.res_inv, S.dims, box_min, box_max);
      bool update_hit;
      sense_clamp_point(P, s, P.ceil_height - S.origin[2], P.ground_height - S.origin[2], box_min, box_max, p, update_hit);
      const long long sy = S.dims[2], sx = (long long)S.dims[1] * S.dims[2];
      auto touch = [&](const int* id, int word) {
        atomicAdd(S.cnt + (id[0] * sx + id[1] * sy + id[2]), word);
        for (int a = 0; a < 3; a++) { mn[a] = id[a] < mn[a] ? id[a] : mn[a]; mx[a] = id[a] > mx[a] ? id[a] : mx[a]; }
      };
      if (update_hit) {   // insertUpdateCandidate(pt_id_g, true), prob_map.cpp:756-759
        const int id[3] = {(int)floor(p[0] * S.res_inv), (int)floor(p[1] * S.res_inv), (int)floor(p[2] * S.res_inv)};
        if (sense_inside(id, S.dims)) touch(id, 0x10001);   // (a hit lies inside the update box, hence inside the map)
      }
      // the ray (762-777): from range_min along it, a miss for every voxel before the end voxel, until it leaves the map
      const double d[3] = {p[0] - s[0], p[1] - s[1], p[2] - s[2]};
      const double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      const double nrm = sqrt(n2);
      double start[3];
      for (int a = 0; a < 3; a++) start[a] = (n2 > 0.0 ? d[a] / nrm : d[a]) * P.range_min + s[a];
      SenseRay R;
      (void)sense_ray_set(R, start, p, S.res);
      int id[3];
      // (a ray moves one voxel per step and never back: inside the map it takes fewer than nx + ny + nz steps)
      for (int step = 0, cap = S.dims[0] + S.dims[1] + S.dims[2] + 8; step < cap && sense_ray_step(R, id); step++) {
        if (!sense_inside(id, S.dims)) break;
        touch(id, 1);
      }
    }
  }
  // cache box of the slot (cache_box_min / max, prob_map.cpp:669-670, 748-750, here in voxels touched): per wave, then one atomic
  for (int a = 0; a < 3; a++) { mn[a] = sense_wave_min(mn[a]); mx[a] = -sense_wave_min(-mx[a]); }
  if ((threadIdx.x & (TOPAY_WAVE - 1)) == 0 && mn[0] != big)
    for (int a = 0; a < 3; a++) { atomicMin(S.box + a, mn[a]); atomicMin(S.box + 3 + a, -mx[a]); }
}

// out[6 slot + i] = word i of the slot's cache box
__global__ void k_sense_box_gather(const SenseSlot* slots, int n, int* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6) return;
  out[i] = slots[i / 6].box[i % 6];
}
// One lane per voxel of the batch's cache box (z fastest); the host sizes the launch by the largest box of the call.  Every touched
// voxel lies inside the map (k_sense_rays), so does the box.  "Hit wins": a voxel with hits takes the hit update alone
// (prob_map.cpp:558-564).
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_flush(SenseP P, const SenseSlot* slots, int blocks_per_slot) {
  const int slot = blockIdx.x / blocks_per_slot;
  const SenseSlot S = slots[slot];
  if (!S.flush) return;
  const int x0 = S.box[0], y0 = S.box[1], z0 = S.box[2];
  if (x0 == 0x7f7f7f7f) return;   // the batch touched no voxel
  const long long sx = -S.box[3] - x0 + 1, sy = -S.box[4] - y0 + 1, sz = -S.box[5] - z0 + 1;
  const long long v = (long long)(blockIdx.x - slot * blocks_per_slot) * blockDim.x + threadIdx.x;
  if (v >= sx * sy * sz) return;
  const int z = (int)(v % sz) + z0, y = (int)((v / sz) % sy) + y0, x = (int)(v / (sz * sy)) + x0;
  const long long idx = ((long long)x * S.dims[1] + y) * S.dims[2] + z;
  const unsigned c = (unsigned)S.cnt[idx];
  if (c == 0u) return;
  const int op = (int)(c & 0xffffu), hit = (int)(c >> 16);
  float ret = S.logodds[idx];
  if (hit > 0) {
    ret += P.l_hit * hit;
    if (ret > P.l_max) ret = P.l_max;
  } else {
    ret += P.l_miss * (op - hit);
    if (ret < P.l_min) ret = P.l_min;
  }
  S.logodds[idx] = ret;
  S.cnt[idx] = 0;
}
__global__ void k_sense_box_reset(const SenseSlot* slots, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6) return;
  const SenseSlot& S = slots[i / 6];
  if (S.flush) S.box[i % 6] = 0x7f7f7f7f;
}

// One lane per (x, y) column.  A column of 16 layers on a 16-byte boundary is written with one 16-byte store.
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_occupancy(const SenseOccSlot* slots, int blocks_per_slot) {
  const int slot = blockIdx.x / blocks_per_slot;
  const SenseOccSlot S = slots[slot];
  const int col = (blockIdx.x - slot * blocks_per_slot) * blockDim.x + threadIdx.x, nz = S.dims[2];
  if (col >= S.dims[0] * S.dims[1]) return;
  const float* lo = S.logodds + (size_t)col * nz;
  signed char* o3 = S.occ3 + (size_t)col * nz;
  bool any = false, low = false;
  struct alignas(16) U4 { unsigned x, y, z, w; };
  if (nz == 16 && ((uintptr_t)o3 & 15) == 0) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int z = 0; z < 16; z++) {
      const bool occ = lo[z] >= S.l_occ;
      w[z >> 2] |= (occ ? 1u : 0u) << (8 * (z & 3));
      any = any || occ;
      low = low || (occ && S.z0 + ((double)z + 0.5) * S.res < S.chassis_height);
    }
    *(U4*)o3 = U4{w[0], w[1], w[2], w[3]};
  } else {
    for (int z = 0; z < nz; z++) {
      const bool occ = lo[z] >= S.l_occ;
      o3[z] = occ ? 1 : 0;
      any = any || occ;
      low = low || (occ && S.z0 + ((double)z + 0.5) * S.res < S.chassis_height);
    }
  }
  S.occ2c[col] = any ? 1 : 0;
  S.occ2[col] = low ? 1 : 0;
}

// SlidingMap::mapSliding (sliding_map.cpp:113-166) as a move: dst[l] = src[l + shift] where l + shift is a voxel of the grid, else 0
// (resetCell).  One lane per (x, y) column of the destination; adjacent lanes are adjacent y, so a wave reads and writes contiguous
// runs of columns, the read run displaced by a constant.  src and dst never overlap (dst is the context's scratch).  A column whose
// nz is a multiple of 4 and that does not move in z goes in 16-byte pieces (every column then starts on a 16-byte boundary: both
// bases do); otherwise float by float, a z shift moving within the column.  The host gives |shift[a]| <= dims[a].
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_slide(const SenseSlideSlot* slots, int blocks_per_slot) {
  const int slot = blockIdx.x / blocks_per_slot;
  const SenseSlideSlot S = slots[slot];
  const int col = (blockIdx.x - slot * blocks_per_slot) * blockDim.x + threadIdx.x, ny = S.dims[1], nz = S.dims[2];
  if (col >= S.dims[0] * ny) return;
  const int x = col / ny, y = col - x * ny;
  const int sx = x + S.shift[0], sy = y + S.shift[1], s2 = S.shift[2];
  const bool inside = sx >= 0 && sx < S.dims[0] && sy >= 0 && sy < ny;
  float* d = S.dst + (size_t)col * nz;
  const float* s = S.src + ((size_t)(inside ? sx : 0) * ny + (inside ? sy : 0)) * nz;
  struct alignas(16) F4 { float x, y, z, w; };
  if ((nz & 3) == 0 && s2 == 0) {
    for (int z = 0; z < nz; z += 4) *(F4*)(d + z) = inside ? *(const F4*)(s + z) : F4{0.0f, 0.0f, 0.0f, 0.0f};
  } else {
    for (int z = 0; z < nz; z++) {
      const int sz = z + s2;
      d[z] = inside && sz >= 0 && sz < nz ? s[sz] : 0.0f;
    }
  }
}

// Ray k = i * n_el + j of a pose: azimuth 2 pi i / n_az + yaw, elevation fov ((j + 0.5) / n_el - 0.5); traversed from the pose
// over `range` with the inserter's traversal.  The point is the centre of the first occupied voxel (the pose's own and the end
// voxel included); a ray that leaves the map or ends without one gives the point at 1.5 range, which the inserter clamps.
__global__ void __launch_bounds__(TOPAY_SENSE_BLOCK) k_sense_scan(const SenseScanSlot* slots, int blocks_per_slot, int n_az, int n_el, double fov,
                                                                  double range, SensePoint* out) {
  const int slot = blockIdx.x / blocks_per_slot, k = (blockIdx.x - slot * blocks_per_slot) * blockDim.x + threadIdx.x, rays = n_az * n_el;
  if (k >= rays) return;
  const SenseScanSlot S = slots[slot];
  const int i = k / n_el, j = k - i * n_el;
  const double az = 6.283185307179586 * (double)i / (double)n_az + S.pose[3], el = fov * (((double)j + 0.5) / (double)n_el - 0.5);
  double sa, ca, se, ce;
  det_sincos(az, &sa, &ca);
  det_sincos(el, &se, &ce);
  const double dir[3] = {ce * ca, ce * sa, se};
  double s[3], e[3];
  for (int a = 0; a < 3; a++) { s[a] = S.pose[a] - S.origin[a]; e[a] = s[a] + dir[a] * range; }
  SenseRay R;
  (void)sense_ray_set(R, s, e, S.res);
  int id[3];
  bool found = false;
  for (int step = 0, cap = S.dims[0] + S.dims[1] + S.dims[2] + 8; step < cap; step++) {
    const bool more = sense_ray_step(R, id);
    if (!sense_inside(id, S.dims)) break;
    if (S.occ3[((size_t)id[0] * S.dims[1] + id[1]) * S.dims[2] + id[2]]) { found = true; break; }
    if (!more) break;
  }
  SensePoint q;
  if (found) {
    q.x = (float)(S.origin[0] + ((double)id[0] + 0.5) * S.res);
    q.y = (float)(S.origin[1] + ((double)id[1] + 0.5) * S.res);
    q.z = (float)(S.origin[2] + ((double)id[2] + 0.5) * S.res);
  } else {
    q.x = (float)(S.pose[0] + dir[0] * (1.5 * range));
    q.y = (float)(S.pose[1] + dir[1] * (1.5 * range));
    q.z = (float)(S.pose[2] + dir[2] * (1.5 * range));
  }
  q.i = 0.0f;
  out[(size_t)slot * rays + k] = q;
}

#endif

}  // namespace topay
