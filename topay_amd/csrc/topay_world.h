// The first half of a benchmark episode on the device (Planner::benchmarkCallback, planner.cpp:491-548): the random world
// (random_map_generator.cpp:207-325 tables, 342-443 cuboids), its occupancy grids (GridMap::regenerateDesk / regenerateMap,
// grid_map.cpp:716-798) and the rejection sampling of start, goal and the two arm configurations (planner.cpp:498-548).
// The checker is the CPU harness (harness/workload.hpp): same statement order, same draws, same roundings.
//
//   Mt64            mt19937_64 (Matsumoto & Nishimura) with the harness's three draws; the 312-word state lives in LDS and one
//                   lane owns a generator (seeding and twist are that lane's serial loops).
//   k_world_generate  one wave per map: lane 0 draws the candidate obstacle, the wave tests it against the accepted boxes
//                   (one box per lane and round), lane 0 appends the obstacle's primitive boxes to the map's list.
//   k_world_raster_lds / k_world_raster_bytes   the point cloud and fillOccupancy in one step.  Every box is axis aligned, so
//                   the cell index of cloud point (i, j, k) along an axis depends on that axis's counter alone: a primitive
//                   marks (x, y) pairs x its set of z cells, and no point is ever stored.
//   k_world_sample_arm / k_world_sample_scenario   World::sampleArm / World::sampleScenario, one lane per instance.
//
// The harness library is built with the host compiler's default contraction of a * b + c, so its draws a + (b - a) * u, the
// snapping floor(x / res) * res + res / 2 and the desk offsets x + r * size_x are single fused operations there: they are
// written as fma() here (this file, like the rest of the library, is compiled without contraction).
#pragma once
#include <hip/hip_runtime.h>

#include "topay_feas.h"

namespace topay {

typedef unsigned long long world_u64;
typedef TOPAY_LDS world_u64* lds_u64p;
typedef TOPAY_LDS unsigned* lds_u32p;

#define TOPAY_WORLD_MAX_BOXES 2048       // accepted obstacle boxes of one map (keep-outs included): the generator's LDS list
#define TOPAY_WORLD_GUARD 2000000L       // tries of one map's rejection loops (workload.hpp:150)
#define TOPAY_WORLD_XY_DRAWS (1 << 20)   // start / goal pairs drawn before a sampler gives up (the harness loops for ever)

// mt19937_64: the state is mt[i * stride], so that the generators of the lanes of a block interleave in LDS.
template <typename P>
struct Mt64 {
  P mt;
  int stride, idx;
  __host__ __device__ __forceinline__ decltype(auto) at(int i) { return (mt[i * stride]); }
  __host__ __device__ inline void seed(world_u64 s) {
    at(0) = s;
    for (int i = 1; i < 312; i++) {
      const world_u64 p = at(i - 1);
      at(i) = 6364136223846793005ULL * (p ^ (p >> 62)) + (world_u64)i;
    }
    idx = 312;
  }
  __host__ __device__ inline void twist() {
    for (int i = 0; i < 312; i++) {
      const world_u64 x = (at(i) & 0xFFFFFFFF80000000ULL) | (at(i + 1 < 312 ? i + 1 : 0) & 0x7FFFFFFFULL);
      at(i) = at(i + 156 < 312 ? i + 156 : i - 156) ^ (x >> 1) ^ ((x & 1ULL) ? 0xB5026F5AA96619E9ULL : 0ULL);
    }
    idx = 0;
  }
  __host__ __device__ inline world_u64 next() {
    if (idx >= 312) twist();
    world_u64 x = at(idx++);
    x ^= (x >> 29) & 0x5555555555555555ULL;
    x ^= (x << 17) & 0x71D67FFFEDA60000ULL;
    x ^= (x << 37) & 0xFFF7EEE000000000ULL;
    x ^= x >> 43;
    return x;
  }
  // the harness's draws (workload.hpp:33-39)
  __host__ __device__ inline double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  __host__ __device__ inline double uni(double a, double b) { return fma(b - a, uni(), a); }
  __host__ __device__ inline int uni_int(int a, int b) { return a + (int)(next() % (world_u64)(b - a + 1)); }
};

// World::sampleStartGoalXY (planner.cpp:498-512): goal then start, accepted when 3 <= distance <= 8.  False when no pair was
// accepted in TOPAY_WORLD_XY_DRAWS draws.
template <typename R>
__host__ __device__ inline bool world_start_goal_xy(R& rng, const double* min_b, const double* max_b, double* start, double* goal) {
  for (int t = 0; t < TOPAY_WORLD_XY_DRAWS; t++) {
    goal[0] = rng.uni(min_b[0] + 2.0, max_b[0] - 2.0);
    goal[1] = rng.uni(min_b[1] + 2.0, max_b[1] - 2.0);
    goal[2] = rng.uni(-M_PI, M_PI);
    start[0] = rng.uni(min_b[0] + 2.0, max_b[0] - 2.0);
    start[1] = rng.uni(min_b[1] + 2.0, max_b[1] - 2.0);
    start[2] = rng.uni(-M_PI, M_PI);
    const double d = hypot(start[0] - goal[0], start[1] - goal[1]);
    if (d < 3.0 || d > 8.0) continue;
    return true;
  }
  return false;
}

// ---- generator ------------------------------------------------------------------------------------------------------
struct WorldGenP {
  int kind, obs0, obs1, arr_lo, arr_hi, box_cap, prim_cap, pad;
  double size_xy, cres;   // map edge, cloud resolution
  double wall_size[2], wall_h[2], float_size[2], float_h[2], desk_len[2], desk_wid[2], desk_h[2];
};
// One axis-aligned block of cloud points: coordinate of counter i along axis d is (float)(((double)(float)(i * cres) + a[d]) + b[d])
// for i < num[d] -- Box::generatePCL with (a, b) = (pos, 0), the boundary walls with (+-size / 2, -cres).
struct WorldPrim {
  double a[3], b[3];
  int num[3];
  int filt;   // the cuboids world's free_range filter applies (random_map_generator.cpp:431-436)
};
// The map the cloud is rasterised into (GridMap::init, workload.hpp:264-275)
struct WorldGrid {
  double origin[3], res_inv, chassis_height, cres;
  int dims[3], prim_cap;
};

__device__ __forceinline__ float world_pt(int i, double cres, double a, double b) {
  const float q = (float)(i * cres);
  return (float)(((double)q + a) + b);
}
__device__ __forceinline__ int world_cell(float p, double origin, double res_inv) { return (int)floor(((double)p - origin) * res_inv); }

__device__ inline void world_emit_box(WorldPrim* pr, int& np, double cres, double px, double py, double pz, double sx, double sy, double sz, int filt) {
  WorldPrim q;
  q.a[0] = px; q.a[1] = py; q.a[2] = pz;
  q.b[0] = 0.0; q.b[1] = 0.0; q.b[2] = 0.0;
  q.num[0] = (int)ceil(sx / cres); q.num[1] = (int)ceil(sy / cres); q.num[2] = (int)ceil(sz / cres);
  q.filt = filt;
  pr[np++] = q;
}
// addBoundaryWalls (workload.hpp:104-130)
__device__ inline void world_emit_walls(WorldPrim* pr, int& np, double cres, double sx, double sy) {
  const double hx = sx / 2.0, hy = sy / 2.0;
  const int n_long_x = (int)ceil(sx / cres), n_long_y = (int)ceil(sy / cres), n_thick = (int)ceil(cres * 2.0 / cres), n_z = (int)ceil(1.0 / cres);
  const double ax[4] = {-hx, -hx, hx, -hx}, ay[4] = {hy, -hy, -hy, -hy};
  for (int w = 0; w < 4; w++) {
    WorldPrim q;
    q.a[0] = ax[w]; q.a[1] = ay[w]; q.a[2] = 0.0;
    q.b[0] = -cres; q.b[1] = -cres; q.b[2] = 0.0;
    q.num[0] = w < 2 ? n_long_x : n_thick;
    q.num[1] = w < 2 ? n_thick : n_long_y;
    q.num[2] = n_z;
    q.filt = 0;
    pr[np++] = q;
  }
}
// generateDesk (workload.hpp:133-140): four legs and the top
__device__ inline void world_emit_desk(WorldPrim* pr, int& np, double cres, double px, double py, double sx, double sy, double sz) {
  const double leg_width = 0.05, desktop_thickness = 0.05;
  const double cx[4] = {px, px + (sx - leg_width), px, px + (sx - leg_width)};
  const double cy[4] = {py, py, py + (sy - leg_width), py + (sy - leg_width)};
  for (int c = 0; c < 4; c++) world_emit_box(pr, np, cres, cx[c], cy[c], 0.0, leg_width, leg_width, sz, 0);
  world_emit_box(pr, np, cres, px, py, sz, sx, sy, desktop_thickness, 0);
}

// Box::overlap2d / overlap of the candidate c (pos 0..2, size 3..5) against box j of the list; touching counts
__device__ __forceinline__ bool world_overlap(const TOPAY_LDS double* c, const TOPAY_LDS double* bx, int cap, int j) {
  for (int a = 0; a < 2; a++) {
    const double min1 = c[a], max1 = c[a] + c[3 + a], min2 = bx[a * cap + j], max2 = bx[a * cap + j] + bx[(3 + a) * cap + j];
    if (max1 < min2 || max2 < min1) return false;
  }
  return c[2] + c[5] > bx[2 * cap + j] && c[2] < bx[2 * cap + j] + bx[5 * cap + j];
}

// generateDeskCase / generateCuboidCase (workload.hpp:143-225).  One wave per map.  Dynamic LDS: the generator's state
// [312 words], the accepted boxes as six arrays [box_cap], the candidate [16].  prims: [n][prim_cap], count / status: [n].
__global__ void k_world_generate(WorldGenP P, int n, const world_u64* seeds, const double* keepouts, WorldPrim* prims, int* count, int* status) {
  const int m = blockIdx.x, lane = threadIdx.x;
  TOPAY_LDS double* L = TOPAY_LDS_PTR;
  Mt64<lds_u64p> rng{(lds_u64p)L, 1, 312};
  TOPAY_LDS double* bx = L + 312;
  TOPAY_LDS double* cand = bx + 6 * P.box_cap;
  const int cap = P.box_cap;
  WorldPrim* pr = prims + (size_t)m * P.prim_cap;
  const double cres = P.cres, half = P.size_xy / 2.0;
  int np = 0, nb = 0;
  if (lane == 0) {
    rng.seed(seeds[m]);
    world_emit_walls(pr, np, cres, P.size_xy, P.size_xy);
    if (P.kind == 0 && keepouts)
      for (int k = 0; k < 2; k++) {   // spawn boxes at start and goal (grid_map.cpp:766-770)
        bx[0 * cap + k] = keepouts[(size_t)m * 4 + 2 * k] - 0.5; bx[1 * cap + k] = keepouts[(size_t)m * 4 + 2 * k + 1] - 0.5; bx[2 * cap + k] = 0.0;
        bx[3 * cap + k] = 1.0; bx[4 * cap + k] = 1.0; bx[5 * cap + k] = 1.0;
      }
  }
  if (P.kind == 0 && keepouts) nb = 2;
  lds_sync();
  long guard = 0;
  bool tripped = false;
  for (int stage = 0; stage < 2; stage++) {
    const int want = stage == 0 ? P.obs0 : P.obs1;
    int placed = 0;
    while (placed < want) {
      if (++guard > TOPAY_WORLD_GUARD) { tripped = true; break; }
      if (lane == 0) {
        double x = rng.uni(-half, half), y = rng.uni(-half, half);
        x = fma(floor(x / cres), cres, cres / 2.0);
        y = fma(floor(y / cres), cres, cres / 2.0);
        double z = 0.0, sx, sy, sz, ux = 0.0, uy = 0.0, row = 1.0, col = 1.0;
        if (P.kind == 0 && stage == 0) {
          ux = rng.uni(P.desk_wid[0], P.desk_wid[1]);
          uy = rng.uni(P.desk_len[0], P.desk_len[1]);
          sz = rng.uni(P.desk_h[0], P.desk_h[1]);
          row = rng.uni_int(P.arr_lo, P.arr_hi);
          col = rng.uni_int(P.arr_lo, P.arr_hi);
          sx = ux * row;
          sy = uy * col;
        } else if (P.kind == 0 || stage == 0) {
          sx = rng.uni(P.wall_size[0], P.wall_size[1]);
          sy = rng.uni(P.wall_size[0], P.wall_size[1]);
          sz = rng.uni(P.wall_h[0], P.wall_h[1]);
        } else {
          sx = rng.uni(P.float_size[0], P.float_size[1]);
          sy = rng.uni(P.float_size[0], P.float_size[1]);
          sz = rng.uni(P.float_size[0], P.float_size[1]);
          z = rng.uni(P.float_h[0], P.float_h[1]);
        }
        cand[0] = x; cand[1] = y; cand[2] = z; cand[3] = sx; cand[4] = sy; cand[5] = sz;
        cand[6] = ux; cand[7] = uy; cand[8] = row; cand[9] = col;
      }
      lds_sync();
      bool hit = false;
      for (int j = lane; j < nb; j += TOPAY_WAVE) hit = hit || world_overlap(cand, bx, cap, j);
      if (P.kind == 1 && lane == 0) {   // the spawn box of the cuboids world: (-0.5, -0.5) + (1, 1), 2-D test
        bool o = true;
        for (int a = 0; a < 2; a++) o = o && !(cand[a] + cand[3 + a] < -0.5 || -0.5 + 1.0 < cand[a]);
        hit = hit || o;
      }
      const bool collision = __any(hit ? 1 : 0) != 0;
      if (!collision) {
        const int row = (int)cand[8], col = (int)cand[9];
        if (lane == 0) {
          for (int a = 0; a < 6; a++) bx[a * cap + nb] = cand[a];
          if (P.kind == 0 && stage == 0) {
            for (int r = 0; r < row; r++)
              for (int c = 0; c < col; c++)
                world_emit_desk(pr, np, cres, fma((double)r, cand[6], cand[0]), fma((double)c, cand[7], cand[1]), cand[6], cand[7], cand[5]);
          } else {
            world_emit_box(pr, np, cres, cand[0], cand[1], cand[2], cand[3], cand[4], cand[5], P.kind == 1 ? 1 : 0);
          }
        }
        nb++;
        placed++;
      }
      lds_sync();   // the candidate is rewritten by the next try
    }
  }
  if (lane == 0) {
    count[m] = np;
    status[m] = tripped ? -1 : 1;
  }
}

// ---- rasteriser -----------------------------------------------------------------------------------------------------
struct alignas(16) WorldU4 { unsigned x, y, z, w; };

__device__ __forceinline__ void world_lds_or(lds_u32p p, unsigned v) {
#ifndef TOPAY_CPU_EMU
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  *p |= v;
#endif
}
// the z cells of a primitive as a bit mask (nz <= 32) and whether a point of it lies below the chassis height (grid_map.cpp:737)
__device__ __forceinline__ void world_z_set(const WorldPrim& q, const WorldGrid& G, unsigned& zmask, bool& zlow) {
  zmask = 0u;
  zlow = false;
  for (int k = 0; k < q.num[2]; k++) {
    const float pz = world_pt(k, G.cres, q.a[2], q.b[2]);
    const int iz = world_cell(pz, G.origin[2], G.res_inv);
    if (iz >= 0 && iz <= G.dims[2] - 1 && iz < 32) zmask |= 1u << iz;
    zlow = zlow || (double)pz < G.chassis_height;
  }
}
// (x, y) pair t of a primitive -> its cell, or -1 when the point lies outside the map or inside the free range
__device__ __forceinline__ int world_xy_cell(const WorldPrim& q, const WorldGrid& G, int t) {
  const int i = t / q.num[1], j = t - i * q.num[1];
  const float px = world_pt(i, G.cres, q.a[0], q.b[0]), py = world_pt(j, G.cres, q.a[1], q.b[1]);
  const float free_range = 0.5f;
  if (q.filt && px > -free_range && px < free_range && py > -free_range && py < free_range) return -1;
  const int ix = world_cell(px, G.origin[0], G.res_inv), iy = world_cell(py, G.origin[1], G.res_inv);
  if (ix < 0 || iy < 0 || ix > G.dims[0] - 1 || iy > G.dims[1] - 1) return -1;
  return ix * G.dims[1] + iy;
}
__device__ __forceinline__ unsigned world_spread4(unsigned bits) {   // bits 0..3 -> the low bit of bytes 0..3
  return (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
}

// First path: one workgroup per map keeps the map in LDS as one z mask per column (16 bits when nz <= 16, else 32) and two bits
// per column (below the chassis / any height); waves take primitives and OR into them; at the end the block writes every byte of
// the three grids with 16-byte stores.  Needs nz <= 32, nx * ny a multiple of 16 and the masks to fit (world_lds_bytes).
__host__ __device__ inline size_t world_lds_bytes(int nx, int ny, int nz) {
  const size_t n2 = (size_t)nx * ny;
  return n2 * (nz <= 16 ? 2 : 4) + 2 * ((n2 + 31) / 32) * 4;
}
template <int BITS>
__global__ void k_world_raster_lds(WorldGrid G, const WorldPrim* prims, const int* count, signed char* occ3, signed char* occ2, signed char* occ2c) {
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (TOPAY_WAVE - 1), wave = tid / TOPAY_WAVE, nwaves = blockDim.x / TOPAY_WAVE;
  const int n2 = G.dims[0] * G.dims[1], nz = G.dims[2];
  const int mask_words = BITS == 16 ? (n2 + 1) / 2 : n2, bit_words = (n2 + 31) / 32;
  lds_u32p masks = (lds_u32p)TOPAY_LDS_PTR;
  lds_u32p low = masks + mask_words;
  lds_u32p any = low + bit_words;
  for (int i = tid; i < mask_words + 2 * bit_words; i += blockDim.x) masks[i] = 0u;
  __syncthreads();
  const WorldPrim* pr = prims + (size_t)m * G.prim_cap;
  const int np = count[m];
  for (int p = wave; p < np; p += nwaves) {
    const WorldPrim q = pr[p];
    unsigned zmask;
    bool zlow;
    world_z_set(q, G, zmask, zlow);
    const int pairs = q.num[0] * q.num[1];
    for (int t = lane; t < pairs; t += TOPAY_WAVE) {
      const int cell = world_xy_cell(q, G, t);
      if (cell < 0 || q.num[2] <= 0) continue;
      if (zmask) {
        if (BITS == 16) world_lds_or(masks + (cell >> 1), zmask << ((cell & 1) * 16));
        else world_lds_or(masks + cell, zmask);
      }
      world_lds_or(any + (cell >> 5), 1u << (cell & 31));
      if (zlow) world_lds_or(low + (cell >> 5), 1u << (cell & 31));
    }
  }
  __syncthreads();
  auto mask_of = [&](int cell) -> unsigned { return BITS == 16 ? (masks[cell >> 1] >> ((cell & 1) * 16)) & 0xffffu : masks[cell]; };
  WorldU4* o3 = (WorldU4*)(occ3 + (size_t)m * n2 * nz);
  const int chunks3 = (int)(((long long)n2 * nz) / 16);
  for (int c = tid; c < chunks3; c += blockDim.x) {
    int cell = (int)(((long long)c * 16) / nz), z = (int)(((long long)c * 16) - (long long)cell * nz);
    unsigned mk = mask_of(cell), w[4];
    for (int k = 0; k < 4; k++) {
      unsigned v = 0u;
      for (int b = 0; b < 4; b++) {
        v |= ((mk >> z) & 1u) << (8 * b);
        if (++z == nz) { z = 0; cell++; mk = cell < n2 ? mask_of(cell) : 0u; }
      }
      w[k] = v;
    }
    o3[c] = WorldU4{w[0], w[1], w[2], w[3]};
  }
  WorldU4* o2 = (WorldU4*)(occ2 + (size_t)m * n2);
  WorldU4* oc = (WorldU4*)(occ2c + (size_t)m * n2);
  for (int c = tid; c < n2 / 16; c += blockDim.x) {
    const unsigned a = (low[c >> 1] >> ((c & 1) * 16)) & 0xffffu, b = (any[c >> 1] >> ((c & 1) * 16)) & 0xffffu;
    o2[c] = WorldU4{world_spread4(a), world_spread4(a >> 4), world_spread4(a >> 8), world_spread4(a >> 12)};
    oc[c] = WorldU4{world_spread4(b), world_spread4(b >> 4), world_spread4(b >> 8), world_spread4(b >> 12)};
  }
}

// Second path, any map: the grids are cleared beforehand; one wave per (map, primitive) stores a byte 1 per marked cell (every
// writer stores the same value, so the races between primitives are benign).
__global__ void k_world_raster_bytes(WorldGrid G, const WorldPrim* prims, const int* count, signed char* occ3, signed char* occ2, signed char* occ2c) {
  const int m = blockIdx.x / G.prim_cap, p = blockIdx.x - m * G.prim_cap, lane = threadIdx.x;
  if (p >= count[m]) return;
  const WorldPrim q = prims[(size_t)m * G.prim_cap + p];
  if (q.num[2] <= 0) return;
  const size_t n2 = (size_t)G.dims[0] * G.dims[1];
  const int nz = G.dims[2];
  bool zlow = false;
  for (int k = 0; k < q.num[2]; k++) zlow = zlow || (double)world_pt(k, G.cres, q.a[2], q.b[2]) < G.chassis_height;
  signed char* o3 = occ3 + (size_t)m * n2 * nz;
  const int pairs = q.num[0] * q.num[1];
  for (int t = lane; t < pairs; t += TOPAY_WAVE) {
    const int cell = world_xy_cell(q, G, t);
    if (cell < 0) continue;
    occ2c[(size_t)m * n2 + cell] = 1;
    if (zlow) occ2[(size_t)m * n2 + cell] = 1;
    for (int k = 0; k < q.num[2]; k++) {
      const int iz = world_cell(world_pt(k, G.cres, q.a[2], q.b[2]), G.origin[2], G.res_inv);
      if (iz >= 0 && iz <= nz - 1) o3[(size_t)cell * nz + iz] = 1;
    }
  }
}

// ---- samplers -------------------------------------------------------------------------------------------------------
// Generators of a sampler block: 16 x 312 words = 39 KB of LDS, interleaved by lane.  A block lasts as long as the lane with the
// most tries, and the 2 x 1024 arms of a benchmark batch are 128 such blocks on 256 compute units: wider blocks only add lanes
// that wait (docs/EXPERIMENTS.md "Episodes on the device").  At most 64.
#ifndef TOPAY_WORLD_SAMPLER_LANES
#define TOPAY_WORLD_SAMPLER_LANES 16
#endif

// World::sampleArm (planner.cpp:529-548): joints U[min, max] until no whole-body collision
template <typename R>
__device__ inline bool world_sample_arm(R& rng, const DevMap& M, double* st, int max_tries, int& tries) {
  dev_params_ref P = dev_params();
  for (int t = 0; t < max_tries; t++) {
    for (int i = 0; i < 7; i++) {
      const double qmax = P.joint_pos_limit_max[i], qmin = -P.joint_pos_limit_max[i];
      st[3 + i] = fma(qmax - qmin, rng.uni(), qmin);
    }
    tries = t + 1;
    if (!whole_body_collision(M, st)) return true;
  }
  return false;
}
__device__ __forceinline__ bool world_collision2d(const DevMap& M, double px, double py, double thr) {   // grid_map.h:511-536
  const double d = feas_dist2d(M, px, py);
  return !(d < 1.0e+9) || d < thr;
}

__global__ void __launch_bounds__(64) k_world_sample_arm(const DevMap* maps, int n, const int* map_ids, const world_u64* seeds, int max_tries, double* states,
                                   int* ok, int* tries) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Mt64<lds_u64p> rng{(lds_u64p)TOPAY_LDS_PTR + threadIdx.x, (int)blockDim.x, 312};
  rng.seed(seeds[i]);
  const DevMap M = maps[map_ids[i]];
  double st[10];
  for (int k = 0; k < 10; k++) st[k] = states[(size_t)i * 10 + k];
  int t = 0;
  ok[i] = world_sample_arm(rng, M, st, max_tries, t) ? 1 : 0;
  tries[i] = t;
  for (int k = 3; k < 10; k++) states[(size_t)i * 10 + k] = st[k];
}

// World::sampleScenario (workload.hpp:731-741)
__global__ void __launch_bounds__(64) k_world_sample_scenario(const DevMap* maps, int n, const int* map_ids, const world_u64* seeds, double* start, double* goal, int* ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Mt64<lds_u64p> rng{(lds_u64p)TOPAY_LDS_PTR + threadIdx.x, (int)blockDim.x, 312};
  rng.seed(seeds[i]);
  const DevMap M = maps[map_ids[i]];
  double s[10], g[10];
  for (int k = 0; k < 10; k++) { s[k] = 0.0; g[k] = 0.0; }
  int found = 0, t = 0;
  for (int attempt = 0; attempt < 10000 && !found; attempt++) {
    if (!world_start_goal_xy(rng, M.min_b, M.max_b, s, g)) break;
    if (world_collision2d(M, s[0], s[1], 0.5) || world_collision2d(M, g[0], g[1], 0.5)) continue;
    if (!world_sample_arm(rng, M, g, 2000, t)) continue;
    if (!world_sample_arm(rng, M, s, 2000, t)) continue;
    found = 1;
  }
  ok[i] = found;
  for (int k = 0; k < 10; k++) { start[(size_t)i * 10 + k] = s[k]; goal[(size_t)i * 10 + k] = g[k]; }
}

// test hook: outputs skip .. skip + n - 1 of a generator
__global__ void k_world_mt64(world_u64 seed, int skip, int n, world_u64* out) {
  if (threadIdx.x != 0) return;
  Mt64<lds_u64p> rng{(lds_u64p)TOPAY_LDS_PTR, 1, 312};
  rng.seed(seed);
  for (int i = 0; i < skip; i++) (void)rng.next();
  for (int i = 0; i < n; i++) out[i] = rng.next();
}

}  // namespace topay
