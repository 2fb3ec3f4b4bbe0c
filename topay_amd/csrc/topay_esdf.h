// ESDF lookups: distance and gradient by bi- / trilinear interpolation of a map's 2-D and 3-D distance fields, as the
// reference's map/include/map/grid_map.h:364-441 (2-D) and 443-509 (3-D) form them; out of map => d = 0, grad = 0.  The 3-D
// lookup also comes in two halves (issue the gathers, finish the arithmetic) for the manipulator block's sphere loop.
#pragma once

#include <hip/hip_runtime.h>

#include "topay_types.h"
#include "topay_wave.h"

namespace topay {

// Clamped cell index pair (i, i+1) -> (lo, hi) as grid_map.h:727-733 does, without ever forming i + 1 on an
// unclamped i: a saturated float->int conversion (points far outside the map) would overflow, and the compiler
// may assume it does not.
__device__ __forceinline__ void clamp_pair(int i, int top, int& lo, int& hi) {
  const int ic = i < -1 ? -1 : (i > top ? top : i);
  lo = ic < 0 ? 0 : ic;
  hi = ic + 1 > top ? top : ic + 1;
}

__device__ __forceinline__ DevMap load_map(const TOPAY_GLB DevMap* mp) {
  DevMap m;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    m.origin[a] = uniform_f64(mp->origin[a]);
    m.min_b[a] = uniform_f64(mp->min_b[a]);
    m.max_b[a] = uniform_f64(mp->max_b[a]);
    m.dims[a] = __builtin_amdgcn_readfirstlane(mp->dims[a]);
  }
  m.res = uniform_f64(mp->res);
  m.res_inv = uniform_f64(mp->res_inv);
  m.pad = 0;
  {
    const unsigned long long p2 = (unsigned long long)mp->esdf2d, p3 = (unsigned long long)mp->esdf3d;
    const unsigned lo2 = __builtin_amdgcn_readfirstlane((int)(p2 & 0xffffffffu)), hi2 = __builtin_amdgcn_readfirstlane((int)(p2 >> 32));
    const unsigned lo3 = __builtin_amdgcn_readfirstlane((int)(p3 & 0xffffffffu)), hi3 = __builtin_amdgcn_readfirstlane((int)(p3 >> 32));
    m.esdf2d = (glb_cdp)(((unsigned long long)hi2 << 32) | lo2);
    m.esdf3d = (glb_cdp)(((unsigned long long)hi3 << 32) | lo3);
  }
  return m;
}

__device__ __forceinline__ void esdf2d_query(const DevMap& M, double px, double py, double& dist, double& gx, double& gy) {
  bool in = !(px < M.min_b[0] + 1e-4 || py < M.min_b[1] + 1e-4 || px > M.max_b[0] - 1e-4 || py > M.max_b[1] - 1e-4);
  dist = 0.0; gx = 0.0; gy = 0.0;
  if (in) {
    const double r = M.res, ri = M.res_inv;
    int ix = (int)floor((px - 0.5 * r - M.origin[0]) * ri);
    int iy = (int)floor((py - 0.5 * r - M.origin[1]) * ri);
    double dx = (px - ((ix + 0.5) * r + M.origin[0])) * ri;
    double dy = (py - ((iy + 0.5) * r + M.origin[1])) * ri;
    const int ny = M.dims[1];
    int x0, x1, y0, y1;
    clamp_pair(ix, M.dims[0] - 1, x0, x1);
    clamp_pair(iy, ny - 1, y0, y1);
    glb_cdp e = M.esdf2d;
    double v00 = e[(size_t)x0 * ny + y0], v01 = e[(size_t)x0 * ny + y1];
    double v10 = e[(size_t)x1 * ny + y0], v11 = e[(size_t)x1 * ny + y1];
    double v0 = v00 * (1 - dx) + v10 * dx;
    double v1 = v01 * (1 - dx) + v11 * dx;
    dist = v0 * (1 - dy) + v1 * dy;
    gy = (v1 - v0) * ri;
    double g0 = (1 - dy) * (v10 - v00);
    g0 += dy * (v11 - v01);
    gx = g0 * ri;
  }
}

__device__ __forceinline__ void esdf3d_query(const DevMap& M, double px, double py, double pz, double& dist, double& gx,
                                             double& gy, double& gz) {
  bool in = !(px < M.min_b[0] + 1e-4 || py < M.min_b[1] + 1e-4 || pz < M.min_b[2] + 1e-4 ||
              px > M.max_b[0] - 1e-4 || py > M.max_b[1] - 1e-4 || pz > M.max_b[2] - 1e-4);
  // branch-free: the gathers are issued unconditionally at clamped indices (so that the scheduler can start them
  // early and overlap several spheres) and the result is discarded for points outside the map (d = 0, grad = 0)
  {
    const double r = M.res, ri = M.res_inv;
    int ix = (int)floor((px - 0.5 * r - M.origin[0]) * ri);
    int iy = (int)floor((py - 0.5 * r - M.origin[1]) * ri);
    int iz = (int)floor((pz - 0.5 * r - M.origin[2]) * ri);
    double dx = (px - ((ix + 0.5) * r + M.origin[0])) * ri;
    double dy = (py - ((iy + 0.5) * r + M.origin[1])) * ri;
    double dz = (pz - ((iz + 0.5) * r + M.origin[2])) * ri;
    const int ny = M.dims[1], nz = M.dims[2];
    int x0, x1, y0, y1, z0, z1;
    clamp_pair(ix, M.dims[0] - 1, x0, x1);
    clamp_pair(iy, ny - 1, y0, y1);
    clamp_pair(iz, nz - 1, z0, z1);
    glb_cdp e = M.esdf3d;
    size_t b00 = ((size_t)x0 * ny + y0) * nz, b01 = ((size_t)x0 * ny + y1) * nz;
    size_t b10 = ((size_t)x1 * ny + y0) * nz, b11 = ((size_t)x1 * ny + y1) * nz;
    double v000 = e[b00 + z0], v001 = e[b00 + z1], v010 = e[b01 + z0], v011 = e[b01 + z1];
    double v100 = e[b10 + z0], v101 = e[b10 + z1], v110 = e[b11 + z0], v111 = e[b11 + z1];
    const double ex = 1 - dx, ey = 1 - dy, ez = 1.0 - dz;
    double v00 = fma(v100, dx, v000 * ex);
    double v01 = fma(v101, dx, v001 * ex);
    double v10 = fma(v110, dx, v010 * ex);
    double v11 = fma(v111, dx, v011 * ex);
    double v0 = fma(v10, dy, v00 * ey);
    double v1 = fma(v11, dy, v01 * ey);
    dist = fma(v1, dz, v0 * ez);
    gz = (v1 - v0) * ri;
    gy = fma(v11 - v01, dz, (v10 - v00) * ez) * ri;
    double g0 = ez * ey * (v100 - v000);
    g0 = fma(ez * dy, v110 - v010, g0);
    g0 = fma(dz * ey, v101 - v001, g0);
    g0 = fma(dz * dy, v111 - v011, g0);
    gx = g0 * ri;
  }
  dist = in ? dist : 0.0; gx = in ? gx : 0.0; gy = in ? gy : 0.0; gz = in ? gz : 0.0;
}

// The same lookup split in two so that the gathers of the next sphere can be in flight while the penalties of the
// current one (divergent branches the scheduler will not move loads across) are evaluated.
//
// Four 16-byte gathers instead of eight 8-byte ones (round 5).  The two z-neighbours of a corner pair are adjacent doubles of
// the field (x-major, z fastest), so one load fetches both: the pair starts at zb = min(z0, nz - 2) and the clamped indices z0,
// z1 (equal at either face of the map) pick their element of it -- the same eight values into the same arithmetic, half the
// vector-memory instructions.  A gather costs the compute unit's L1 one tag lookup per lane whatever its width, and eight waves
// of a compute unit share that L1: 96 -> 48 such instructions per call of the manipulator block.  (The loads are 8-byte
// aligned; a pair that straddles a cache line costs two lookups, one case in eight or sixteen.  nz >= 2 is checked when a map
// is set: with a single layer the pair would reach past the field.)
typedef double esdf_pair __attribute__((vector_size(16), aligned(8)));
struct Esdf3dReq {
  esdf_pair p00, p01, p10, p11;   // (z pair) of the rows (x0, y0), (x0, y1), (x1, y0), (x1, y1)
  double dx, dy, dz;
  bool in, z0hi, z1hi;            // z0 / z1 is the pair's second element
};
__device__ __forceinline__ void esdf3d_issue(const DevMap& M, double px, double py, double pz, Esdf3dReq& q) {
  q.in = !(px < M.min_b[0] + 1e-4 || py < M.min_b[1] + 1e-4 || pz < M.min_b[2] + 1e-4 ||
           px > M.max_b[0] - 1e-4 || py > M.max_b[1] - 1e-4 || pz > M.max_b[2] - 1e-4);
  const double r = M.res, ri = M.res_inv;
  int ix = (int)floor((px - 0.5 * r - M.origin[0]) * ri);
  int iy = (int)floor((py - 0.5 * r - M.origin[1]) * ri);
  int iz = (int)floor((pz - 0.5 * r - M.origin[2]) * ri);
  q.dx = (px - ((ix + 0.5) * r + M.origin[0])) * ri;
  q.dy = (py - ((iy + 0.5) * r + M.origin[1])) * ri;
  q.dz = (pz - ((iz + 0.5) * r + M.origin[2])) * ri;
  const int ny = M.dims[1], nz = M.dims[2];
  int x0, x1, y0, y1, z0, z1;
  clamp_pair(ix, M.dims[0] - 1, x0, x1);
  clamp_pair(iy, ny - 1, y0, y1);
  clamp_pair(iz, nz - 1, z0, z1);
  glb_cdp e = M.esdf3d;
  // One linear index with a multiply (integer multiplies run at a quarter of the vector rate), the other rows by adding the
  // strides of the axes along which the clamped neighbour differs (x1 - x0, y1 - y0 are 0 or 1).  A field has fewer than
  // 2^32 cells (checked when the map is set), so the indices are 32-bit.
  const int zb = z0 < nz - 2 ? z0 : nz - 2;
  q.z0hi = z0 != zb;
  q.z1hi = z1 != zb;
  const unsigned i00 = ((unsigned)x0 * (unsigned)ny + (unsigned)y0) * (unsigned)nz + (unsigned)zb;
  const unsigned sx = x1 != x0 ? (unsigned)(ny * nz) : 0u, sy = y1 != y0 ? (unsigned)nz : 0u;
  const unsigned i01 = i00 + sy, i10 = i00 + sx;
  const unsigned i11 = i10 + sy;
#ifndef TOPAY_CPU_EMU
  typedef const TOPAY_GLB esdf_pair* pair_ptr;
  q.p00 = *(pair_ptr)(e + (size_t)i00);
  q.p01 = *(pair_ptr)(e + (size_t)i01);
  q.p10 = *(pair_ptr)(e + (size_t)i10);
  q.p11 = *(pair_ptr)(e + (size_t)i11);
#else
  q.p00[0] = e[(size_t)i00]; q.p00[1] = e[(size_t)i00 + 1];
  q.p01[0] = e[(size_t)i01]; q.p01[1] = e[(size_t)i01 + 1];
  q.p10[0] = e[(size_t)i10]; q.p10[1] = e[(size_t)i10 + 1];
  q.p11[0] = e[(size_t)i11]; q.p11[1] = e[(size_t)i11 + 1];
#endif
}
__device__ __forceinline__ void esdf3d_finish(const DevMap& M, const Esdf3dReq& q, double& dist, double& gx, double& gy,
                                              double& gz) {
  const double ri = M.res_inv;
  const double dx = q.dx, dy = q.dy, dz = q.dz;
  const double ex = 1 - dx, ey = 1 - dy, ez = 1.0 - dz;
  const double v000 = q.z0hi ? q.p00[1] : q.p00[0], v001 = q.z1hi ? q.p00[1] : q.p00[0];
  const double v010 = q.z0hi ? q.p01[1] : q.p01[0], v011 = q.z1hi ? q.p01[1] : q.p01[0];
  const double v100 = q.z0hi ? q.p10[1] : q.p10[0], v101 = q.z1hi ? q.p10[1] : q.p10[0];
  const double v110 = q.z0hi ? q.p11[1] : q.p11[0], v111 = q.z1hi ? q.p11[1] : q.p11[0];
  double v00 = fma(v100, dx, v000 * ex);
  double v01 = fma(v101, dx, v001 * ex);
  double v10 = fma(v110, dx, v010 * ex);
  double v11 = fma(v111, dx, v011 * ex);
  double v0 = fma(v10, dy, v00 * ey);
  double v1 = fma(v11, dy, v01 * ey);
  dist = fma(v1, dz, v0 * ez);
  gz = (v1 - v0) * ri;
  gy = fma(v11 - v01, dz, (v10 - v00) * ez) * ri;
  double g0 = ez * ey * (v100 - v000);
  g0 = fma(ez * dy, v110 - v010, g0);
  g0 = fma(dz * ey, v101 - v001, g0);
  g0 = fma(dz * dy, v111 - v011, g0);
  gx = g0 * ri;
  dist = q.in ? dist : 0.0; gx = q.in ? gx : 0.0; gy = q.in ? gy : 0.0; gz = q.in ? gz : 0.0;
}

}  // namespace topay
