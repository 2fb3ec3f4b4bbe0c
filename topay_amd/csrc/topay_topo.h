// The topological roadmap of the front-end on the device: TopologyPRM::findTopoPaths (planner/src/topo_prm.cpp:60-122)
// with everything it calls -- createGraph 124-212, findVisibGuard 214-233, needConnection 235-263, getSample 265-276,
// lineVisib 278-315, pruneGraph 317-344, searchPaths / depthFirstSearch 656-734, shortcutPaths / shortcutPath 512-582,
// discretizeLine / discretizePath 472-506, 584-616, sameTopoPath 424-448, pruneEquivalent 346-382, selectShortPaths 384-422,
// pathLength, shortestPath; the ray caster RayCaster::setInput / step (planner/src/utils/raycast.cpp:31-48, 253-346); the
// map queries getDistCoarse2d / 2i, getDisWithGradI2d, indexToPos3d, boundIndex2d, getOffset (map/include/map/grid_map.h).
// One wavefront per (start, goal) query, as k_jps and k_mcrrt.  The roadmap is sequential (every sample meets the graph
// the earlier ones left), what the wave parallelises is the work inside a step:
//   sampling      64 samples are drawn and tested against the clearance at once (the draws are counter-based, so sample k
//                 does not depend on the graph); the survivors go through the serial part in index order;
//   visibility    lane g casts the ray to guard g (list order, connectors skipped), a ballot picks the first three;
//   sameTopoPath  lane i casts the ray between the i-th points of the two discretised paths;
//   shortcutPath  sequential along a path, independent across paths: lane i shortens kept raw path i (at most 64);
//   pruneGraph, the depth-first search and the selection by node count are lane 0's.
// The graph (node table with up to TOPAY_TOPO_MAX_NB neighbour ids per node), the raw paths (node-id lists) and the point
// buffers live in a per-call allocation in device memory (TopoBatch); the node id is the node's index in the table,
// which is also the list order of the reference (push_back, ids counted up), an erased node has type 0.
// Deterministic where the reference is not (include/topay.h, topay_topo_params_t); harness/topo_prm.hpp is the CPU
// restatement with the same rules and the same arithmetic (z = 0 terms dropped: they add exact zeros).
#pragma once
#include "topay_front.h"
#include "topay_mcrrt.h"

namespace topay {

#define TOPAY_TOPO_RAWLEN 100   // path_list(100), topo_prm.cpp:666: a raw path has fewer nodes than this
#define TOPAY_TOPO_DFS_CAP 2000000   // nodes the depth-first search may enter (it enumerates simple paths; the reference has no bound)

struct TopoParams {   // == topay_topo_params_t
  double sample_inflate_x, sample_inflate_y, clearance, ratio_to_short;
  int max_sample_num, max_raw_path, max_raw_path2, reserve_num, node_cap, reserved;
  unsigned long long seed;
};

struct TopoBatch {
  int n, cap_paths, cap_points;
  int pt_cap, nbuf;             // points per point buffer (the cap of the largest map of the call), buffers per query: S[i] = i, D[i] = R2 + i, T[k][0..1] = 2 R2 + 2 k + (0, 1)
  unsigned long long inst_base;
  const unsigned long long* inst;   // instance number per query (topay_plan_calls), or null: inst_base + query
  const int* map_id;
  const double* start;          // n x 2
  const double* end;            // n x 2
  const int* critical;          // n, or null
  TopoParams P;
  // scratch, per query
  int* nd_type;                 // [node_cap]  1 guard, 2 connector, 0 erased by pruneGraph
  int* nd_nnb;                  // [node_cap]
  int* nd_nb;                   // [node_cap][TOPAY_TOPO_MAX_NB]
  double* nd_pos;               // [node_cap][2]
  int* guards;                  // [node_cap]  ids of the guards in list order
  unsigned short* raw;          // [max_raw_path][TOPAY_TOPO_RAWLEN]  raw paths as node ids
  int* raw_len;                 // [max_raw_path]
  int* keep;                    // [max_raw_path2]  the raw paths searchPaths keeps
  double* pts;                  // [nbuf][pt_cap][2]
  int* pts_len;                 // [nbuf]
  int* meta;                    // [8]: nodes created, kept raw paths, raw paths found, status of lane 0's part, nodes after pruning
  // results
  int* n_paths;                 // [n]
  int* path_len;                // [n][cap_paths]
  double* path_xy;              // [n][cap_paths][cap_points][2]
  int* stats;                   // [n][8]
};

struct TopoCtx {
  DevMap M;
  glb_cdp coarse;               // esdf_buffer_2d_inflate, or _critical
  int nx, ny, lane;
  double res, offx, offy;
};

__device__ __forceinline__ double topo_coarse(const TopoCtx& C, int ix, int iy) {   // boundIndex2d + getDistCoarse2i
  ix = max(min(ix, C.nx - 1), 0);
  iy = max(min(iy, C.ny - 1), 0);
  return C.coarse[(size_t)ix * C.ny + iy];
}
__device__ __forceinline__ double topo_intbound(double s, double ds) {   // raycast.cpp:35-48; fmod(v, 1) = v - trunc(v), exactly
  if (ds < 0) { s = -s; ds = -ds; }
  s = s - trunc(s);
  s = s + 1.0;
  s = s - trunc(s);
  return (1 - s) / ds;
}
// lineVisib (topo_prm.cpp:278-315) on RayCaster (z = 0: tMaxZ = +inf, the z branch is never taken).  The cell under test
// is int(ray cell + offset) clamped into the map; the end cell is not tested; a tie tMaxX == tMaxY steps y.  A traversal
// that has not reached the end cell after |dx| + |dy| steps (the reference would not terminate) ends as visible.
__device__ inline bool topo_line_visib(const TopoCtx& C, double p1x, double p1y, double p2x, double p2y, double thresh, double& pcx, double& pcy) {
  const double sx = p1x / C.res, sy = p1y / C.res, ex = p2x / C.res, ey = p2y / C.res;
  int x = (int)floor(sx), y = (int)floor(sy);
  const int endx = (int)floor(ex), endy = (int)floor(ey);
  const double dx = endx - x, dy = endy - y;
  const int stepx = dx == 0.0 ? 0 : (dx < 0.0 ? -1 : 1), stepy = dy == 0.0 ? 0 : (dy < 0.0 ? -1 : 1);
  if (stepx == 0 && stepy == 0) return true;
  double tmx = topo_intbound(sx, dx), tmy = topo_intbound(sy, dy);
  const double tdx = (double)stepx / dx, tdy = (double)stepy / dy;
  const int budget = abs(endx - x) + abs(endy - y);
  double prevx = (x + 0.5) * C.M.res + C.M.origin[0], prevy = (y + 0.5) * C.M.res + C.M.origin[1];   // indexToPos3d(floor(p1 / res))
  for (int it = 0; it < budget; ++it) {
    if (x == endx && y == endy) break;
    const int ix = (int)((double)x + C.offx), iy = (int)((double)y + C.offy);
    const double curx = (ix + 0.5) * C.M.res + C.M.origin[0], cury = (iy + 0.5) * C.M.res + C.M.origin[1];
    if (topo_coarse(C, ix, iy) <= thresh) {
      pcx = 0.5 * (curx + prevx);
      pcy = 0.5 * (cury + prevy);
      return false;
    }
    prevx = curx; prevy = cury;
    if (tmx < tmy) { x += stepx; tmx += tdx; }
    else { y += stepy; tmy += tdy; }
  }
  return true;
}
__device__ __forceinline__ double topo_dist(double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  return sqrt(dx * dx + dy * dy);
}
__device__ inline double topo_path_length(const double* P, int n) {   // pathLength, topo_prm.cpp:462-470
  double length = 0.0;
  for (int i = 0; i + 1 < n; ++i) length += topo_dist(P[2 * i], P[2 * i + 1], P[2 * i + 2], P[2 * i + 3]);
  return length;
}
// point i of discretizePath(path, pt_num), topo_prm.cpp:472-506.  false: undefined in the reference (no interval, or an
// interval of zero length).
__device__ inline bool topo_disc_point(const double* P, int n, int pt_num, int i, double len_total, double& ox, double& oy) {
  const double dl = len_total / double(pt_num - 1);
  const double cur_l = double(i) * dl;
  double acc = 0.0;
  for (int j = 0; j + 1 < n; ++j) {
    const double nxt = topo_dist(P[2 * j], P[2 * j + 1], P[2 * j + 2], P[2 * j + 3]) + acc;
    if (cur_l >= acc - 1e-4 && cur_l <= nxt + 1e-4) {
      const double den = nxt - acc;
      if (!(den > 0.0)) return false;
      const double lambda = (cur_l - acc) / den;
      ox = (1 - lambda) * P[2 * j] + lambda * P[2 * j + 2];
      oy = (1 - lambda) * P[2 * j + 1] + lambda * P[2 * j + 3];
      return true;
    }
    acc = nxt;
  }
  return false;
}
// sameTopoPath(path1, path2, thresh = 0), topo_prm.cpp:424-448.  Wave-collective (uniform arguments).  err = -2 when a
// discretisation is undefined in the reference; the reference discretises both paths before it casts the first ray, so
// a path of more than 64 points is checked for that in a pass of its own.
__device__ inline bool topo_same_topo(const TopoCtx& C, const double* P1, int n1, const double* P2, int n2, int& err) {
  if (n1 < 2 || n2 < 2) { err = -2; return false; }
  const double len1 = topo_path_length(P1, n1), len2 = topo_path_length(P2, n2);
  const double max_len = len1 > len2 ? len1 : (len2 > len1 ? len2 : len1);
  const int pt_num = (int)ceil(max_len / C.res);
  if (pt_num > 64) {
    for (int base = 0; base < pt_num; base += 64) {
      const int i = base + C.lane;
      double ax, ay;
      const bool bad = i < pt_num && (!topo_disc_point(P1, n1, pt_num, i, len1, ax, ay) || !topo_disc_point(P2, n2, pt_num, i, len2, ax, ay));
      if (__any(bad)) { err = -2; return false; }
    }
  }
  for (int base = 0; base < pt_num; base += 64) {
    const int i = base + C.lane;
    bool bad = false, blocked = false;
    if (i < pt_num) {
      double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0, pcx, pcy;
      bad = !topo_disc_point(P1, n1, pt_num, i, len1, ax, ay) || !topo_disc_point(P2, n2, pt_num, i, len2, bx, by);
      if (!bad) blocked = !topo_line_visib(C, ax, ay, bx, by, 0.0, pcx, pcy);
    }
    if (__any(bad)) { err = -2; return false; }
    if (__any(blocked)) return false;
  }
  return true;
}

// One iteration of shortcutPath's loop (topo_prm.cpp:516-562) by one lane: `in` (n_in points) -> discretised into D ->
// shortened into `out`.  Returns 0: out holds the shortened path; 1: the discretisation has fewer than two points (the
// reference stores it and returns: n_out = 0); 2: the result is longer than the input (the reference keeps the input
// and stops iterating; out is not valid); -1: a buffer is full.
template <typename In>
__device__ inline int topo_shortcut_iter(const TopoCtx& C, const DevMap& Mf, In in, int n_in, double* D, double* out, int pt_cap, int& n_out,
                                         int& pushes) {
  // discretizePath(path), 599-616, with discretizeLine 584-597
  int nd = 0;
  double len1 = 0.0;
  n_out = 0;
  if (n_in >= 2) {
    double ax, ay;
    in(0, ax, ay);
    for (int i = 0; i + 1 < n_in; ++i) {
      double bx, by;
      in(i + 1, bx, by);
      const double dx = bx - ax, dy = by - ay;
      const double len = sqrt(dx * dx + dy * dy);
      len1 += len;
      const int seg_num = (int)ceil(len / C.res);
      if (seg_num > 0) {
        const int cnt = (i != n_in - 2) ? seg_num : seg_num + 1;   // (the last point of an inner segment is popped again)
        if (nd + cnt > pt_cap) return -1;
        for (int k = 0; k < cnt; ++k) {
          D[2 * (nd + k)] = ax + dx * double(k) / double(seg_num);
          D[2 * (nd + k) + 1] = ay + dy * double(k) / double(seg_num);
        }
        nd += cnt;
      }
      ax = bx; ay = by;
    }
  }
  if (nd < 2) return 1;
  // visibility path shortening, 526-552
  double backx = D[0], backy = D[1], len2 = 0.0;
  out[0] = backx; out[1] = backy;
  int cnt = 1;
  for (int i = 1; i < nd; ++i) {
    const double qx = D[2 * i], qy = D[2 * i + 1];
    double cx, cy;
    if (topo_line_visib(C, backx, backy, qx, qy, C.res, cx, cy)) continue;
    double dist, gx, gy;
    esdf2d_query(Mf, cx, cy, dist, gx, gy);   // getDisWithGradI2d(colli_pt, dist, grad, false, use_critical)
    const double gn = sqrt(gx * gx + gy * gy);
    if (gn > 1e-3) {
      gx = gx / gn; gy = gy / gn;
      double dirx = qx - backx, diry = qy - backy;
      const double dz = dirx * dirx + diry * diry;
      if (dz > 0.0) { const double dn = sqrt(dz); dirx = dirx / dn; diry = diry / dn; }
      const double dt = gx * dirx + gy * diry;
      double px = gx - dt * dirx, py = gy - dt * diry;
      const double pz = px * px + py * py;
      if (pz > 0.0) { const double pn = sqrt(pz); px = px / pn; py = py / pn; }
      cx = cx + C.res * px;
      cy = cy + C.res * py;
      pushes++;
    }
    len2 += topo_dist(backx, backy, cx, cy);
    out[2 * cnt] = cx; out[2 * cnt + 1] = cy;
    backx = cx; backy = cy;
    cnt++;
    if (cnt >= pt_cap) return -1;
  }
  len2 += topo_dist(backx, backy, D[2 * (nd - 1)], D[2 * (nd - 1) + 1]);
  out[2 * cnt] = D[2 * (nd - 1)]; out[2 * cnt + 1] = D[2 * (nd - 1) + 1];
  cnt++;
  n_out = cnt;
  if (len2 > len1) return 2;
  return 0;
}

__global__ void __launch_bounds__(64) k_topo(const DevMap* maps, const TopoBatch B) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= B.n) return;
  const TopoParams& P = B.P;
  TopoCtx C;
  C.M = maps[B.map_id[p]];
  const bool critical = B.critical ? B.critical[p] != 0 : false;
  C.coarse = critical ? C.M.esdf2d_critical : C.M.esdf2d_inflate;
  DevMap Mf = C.M;   // the field of the collision-point push: the plain 2-D field, or the critical one
  if (critical) Mf.esdf2d = C.M.esdf2d_critical;
  C.nx = C.M.dims[0]; C.ny = C.M.dims[1]; C.lane = lane;
  C.res = C.M.res;
  C.offx = 0.5 - C.M.origin[0] / C.M.res;   // getOffset, grid_map.h:208
  C.offy = 0.5 - C.M.origin[1] / C.M.res;
  const size_t nb0 = (size_t)p * P.node_cap;
  int* nd_type = B.nd_type + nb0;
  int* nd_nnb = B.nd_nnb + nb0;
  int* nd_nb = B.nd_nb + nb0 * TOPAY_TOPO_MAX_NB;
  double* nd_pos = B.nd_pos + 2 * nb0;
  int* guards = B.guards + nb0;
  unsigned short* raw = B.raw + (size_t)p * P.max_raw_path * TOPAY_TOPO_RAWLEN;
  int* raw_len = B.raw_len + (size_t)p * P.max_raw_path;
  int* keep = B.keep + (size_t)p * P.max_raw_path2;
  double* pts = B.pts + (size_t)p * B.nbuf * B.pt_cap * 2;
  int* pts_len = B.pts_len + (size_t)p * B.nbuf;
  int* meta = B.meta + 8 * (size_t)p;
  int* stats = B.stats + 8 * (size_t)p;
  auto buf = [&](int b) { return pts + (size_t)b * B.pt_cap * 2; };
  const int R2 = P.max_raw_path2;
  // points a path of THIS query's map may have (the buffers are strided by the largest map of the call, B.pt_cap)
  const int pt_cap = min(B.pt_cap, 2 * (int)ceil(sqrt((double)C.nx * C.nx + (double)C.ny * C.ny)) + 512);
  const double sx = B.start[2 * (size_t)p], sy = B.start[2 * (size_t)p + 1], ex = B.end[2 * (size_t)p], ey = B.end[2 * (size_t)p + 1];
  const unsigned long long inst = B.inst ? B.inst[p] : B.inst_base + (unsigned long long)p;
  int n_drawn = 0, n_passed = 0, nodes_before = 0, nodes_after = 0, raw_found = 0, n_filtered = 0;
  auto finish = [&](int status, int n_sel) {
    if (lane == 0) {
      const bool ok = status >= 0;
      stats[0] = status; stats[1] = ok ? n_drawn : 0; stats[2] = ok ? n_passed : 0; stats[3] = ok ? nodes_before : 0;
      stats[4] = ok ? nodes_after : 0; stats[5] = ok ? raw_found : 0; stats[6] = ok ? n_filtered : 0; stats[7] = ok ? n_sel : 0;
      B.n_paths[p] = ok ? n_sel : 0;
    }
  };
  if (lane < 8) meta[lane] = 0;
  for (int k = lane; k < B.cap_paths; k += 64) B.path_len[(size_t)p * B.cap_paths + k] = 0;
  for (int k = lane; k < B.nbuf; k += 64) pts_len[k] = 0;

  // ---- createGraph, topo_prm.cpp:124-212
  if (lane == 0) {
    nd_type[0] = 1; nd_nnb[0] = 0; nd_pos[0] = sx; nd_pos[1] = sy; guards[0] = 0;
    nd_type[1] = 1; nd_nnb[1] = 0; nd_pos[2] = ex; nd_pos[3] = ey; guards[1] = 1;
  }
  wave_global_sync();
  int n_nodes = 2, n_guards = 2;
  const double r0 = 0.5 * topo_dist(sx, sy, ex, ey) + P.sample_inflate_x, r1 = P.sample_inflate_y;
  const double tx = 0.5 * (sx + ex), ty = 0.5 * (sy + ey);
  double xt0 = ex - tx, xt1 = ey - ty;
  {
    const double z = xt0 * xt0 + xt1 * xt1;
    if (z > 0.0) { const double nn = sqrt(z); xt0 = xt0 / nn; xt1 = xt1 / nn; }
  }
  double yt0 = -xt1, yt1 = xt0;   // xtf x (0, 0, -1)
  {
    const double z = yt0 * yt0 + yt1 * yt1;
    if (z > 0.0) { const double nn = sqrt(z); yt0 = yt0 / nn; yt1 = yt1 / nn; }
  }
  for (int base = 0; base < P.max_sample_num; base += 64) {
    const int k = base + lane;
    double px = 0.0, py = 0.0;
    bool pass = false;
    if (k < P.max_sample_num) {
      const double a = (2.0 * mcrrt_u01(P.seed, inst, (unsigned long long)k, 0) - 1.0) * r0;
      const double b = (2.0 * mcrrt_u01(P.seed, inst, (unsigned long long)k, 1) - 1.0) * r1;
      px = (xt0 * a + yt0 * b) + tx;
      py = (xt1 * a + yt1 * b) + ty;
      const int ix = (int)floor((px - C.M.origin[0]) * C.M.res_inv), iy = (int)floor((py - C.M.origin[1]) * C.M.res_inv);
      pass = !(topo_coarse(C, ix, iy) <= P.clearance);
    }
    n_drawn = min(base + 64, P.max_sample_num);
    unsigned long long m = __ballot(pass);
    n_passed += __popcll(m);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const double qx = __shfl(px, src), qy = __shfl(py, src);
      // findVisibGuard: the first three visible guards in list order (the reference breaks after the third)
      int nv = 0, v0 = -1, v1 = -1;
      for (int gb = 0; gb < n_guards && nv <= 2; gb += 64) {
        const int gi = gb + lane;
        bool vis = false;
        if (gi < n_guards) {
          const int g = guards[gi];
          double pcx, pcy;
          vis = topo_line_visib(C, qx, qy, nd_pos[2 * g], nd_pos[2 * g + 1], C.res, pcx, pcy);
        }
        unsigned long long mm = __ballot(vis);
        while (mm && nv <= 2) {
          const int f = __ffsll((long long)mm) - 1;
          mm &= mm - 1;
          const int g = guards[gb + f];
          if (nv == 0) v0 = g;
          else if (nv == 1) v1 = g;
          nv++;
        }
      }
      if (nv == 0) {
        if (n_nodes >= P.node_cap) { finish(-1, 0); return; }
        if (lane == 0) {
          nd_type[n_nodes] = 1; nd_nnb[n_nodes] = 0; nd_pos[2 * n_nodes] = qx; nd_pos[2 * n_nodes + 1] = qy;
          guards[n_guards] = n_nodes;
        }
        n_nodes++; n_guards++;
        wave_global_sync();
      } else if (nv == 2) {
        // needConnection, 235-263
        const int na = nd_nnb[v0], nbn = nd_nnb[v1];
        double path1[6], path2[6];
        path1[0] = nd_pos[2 * v0]; path1[1] = nd_pos[2 * v0 + 1]; path1[2] = qx; path1[3] = qy;
        path1[4] = nd_pos[2 * v1]; path1[5] = nd_pos[2 * v1 + 1];
        path2[0] = path1[0]; path2[1] = path1[1]; path2[4] = path1[4]; path2[5] = path1[5];
        bool need = true;
        for (int i = 0; i < na && need; ++i)
          for (int j = 0; j < nbn && need; ++j) {
            const int c = nd_nb[v0 * TOPAY_TOPO_MAX_NB + i];
            if (c != nd_nb[v1 * TOPAY_TOPO_MAX_NB + j]) continue;
            path2[2] = nd_pos[2 * c]; path2[3] = nd_pos[2 * c + 1];
            int err = 0;
            const bool same = topo_same_topo(C, path1, 3, path2, 3, err);
            if (err) { finish(err, 0); return; }
            if (same) {
              if (topo_path_length(path1, 3) < topo_path_length(path2, 3)) {   // line 254: the connector moves
                wave_global_sync();   // (every lane has read the old position)
                if (lane == 0) { nd_pos[2 * c] = qx; nd_pos[2 * c + 1] = qy; }
                wave_global_sync();
              }
              need = false;
            }
          }
        if (need) {
          if (n_nodes >= P.node_cap || na >= TOPAY_TOPO_MAX_NB || nbn >= TOPAY_TOPO_MAX_NB) { finish(-1, 0); return; }
          wave_global_sync();   // (every lane has read the neighbour counts)
          if (lane == 0) {
            nd_type[n_nodes] = 2; nd_nnb[n_nodes] = 2; nd_pos[2 * n_nodes] = qx; nd_pos[2 * n_nodes + 1] = qy;
            nd_nb[n_nodes * TOPAY_TOPO_MAX_NB] = v0; nd_nb[n_nodes * TOPAY_TOPO_MAX_NB + 1] = v1;
            nd_nb[v0 * TOPAY_TOPO_MAX_NB + na] = n_nodes; nd_nnb[v0] = na + 1;
            nd_nb[v1 * TOPAY_TOPO_MAX_NB + nbn] = n_nodes; nd_nnb[v1] = nbn + 1;
          }
          n_nodes++;
          wave_global_sync();
        }
      }
    }
  }
  nodes_before = n_nodes;

  // ---- lane 0: pruneGraph (317-344), searchPaths / depthFirstSearch (656-734)
  wave_global_sync();
  if (lane == 0) {
    // nodes with at most one neighbour go, one after the other, until none is left (start and goal stay); the order
    // of removal does not change the result, the neighbour lists keep their order
    int alive = n_nodes;
    for (bool changed = true; changed && alive > 2;) {
      changed = false;
      for (int id = 2; id < n_nodes && alive > 2; ++id) {
        if (nd_type[id] == 0 || nd_nnb[id] > 1) continue;
        for (int m2 = 0; m2 < n_nodes; ++m2) {
          if (nd_type[m2] == 0 || m2 == id) continue;
          const int cnt = nd_nnb[m2];
          int* nbl = nd_nb + m2 * TOPAY_TOPO_MAX_NB;
          for (int t = 0; t < cnt; ++t)
            if (nbl[t] == id) {
              for (int u = t; u + 1 < cnt; ++u) nbl[u] = nbl[u + 1];
              nd_nnb[m2] = cnt - 1;
              break;
            }
        }
        nd_type[id] = 0; nd_nnb[id] = 0;
        alive--;
        changed = true;
      }
    }
    // depth-first search with an explicit stack: vis = the chain of visited nodes, nxt = the neighbour to try next (-1: the
    // node has just been entered and its goal check is still to do)
    unsigned short vis[TOPAY_TOPO_RAWLEN];
    int nxt[TOPAY_TOPO_RAWLEN];
    int depth = 1, n_raw = 0, st = 0, entries = 0;
    vis[0] = 0; nxt[0] = -1;
    while (depth > 0 && st == 0 && n_raw < P.max_raw_path) {
      const int cur = vis[depth - 1], cnt = nd_nnb[cur];
      const int* nbl = nd_nb + cur * TOPAY_TOPO_MAX_NB;
      if (nxt[depth - 1] < 0) {
        if (depth >= TOPAY_TOPO_RAWLEN || ++entries > TOPAY_TOPO_DFS_CAP) { st = -2; break; }
        nxt[depth - 1] = 0;
        bool reaches = false;
        for (int i = 0; i < cnt; ++i) if (nbl[i] == 1) { reaches = true; break; }
        if (reaches) {
          if (depth + 1 >= TOPAY_TOPO_RAWLEN) { st = -2; break; }
          unsigned short* rp = raw + (size_t)n_raw * TOPAY_TOPO_RAWLEN;
          for (int j = 0; j < depth; ++j) rp[j] = vis[j];
          rp[depth] = 1;
          raw_len[n_raw] = depth + 1;
          n_raw++;
          continue;   // (the loop condition ends the search when max_raw_path is reached)
        }
      }
      int i = nxt[depth - 1];
      int next = -1;
      for (; i < cnt; ++i) {
        const int cand = nbl[i];
        if (cand == 1) continue;
        bool revisit = false;
        for (int j = 0; j < depth; ++j) if (vis[j] == cand) { revisit = true; break; }
        if (revisit) continue;
        next = cand;
        break;
      }
      if (next < 0) { depth--; continue; }
      nxt[depth - 1] = i + 1;
      vis[depth] = (unsigned short)next; nxt[depth] = -1;
      depth++;
    }
    // the raw paths with the fewest nodes first, up to max_raw_path2 (664-688)
    int n_keep = 0;
    if (st == 0) {
      int mn = 100000, mx = 1;
      for (int i = 0; i < n_raw; ++i) { mx = max(mx, raw_len[i]); mn = min(mn, raw_len[i]); }
      for (int s = mn; s <= mx && n_keep < R2; ++s)
        for (int i = 0; i < n_raw && n_keep < R2; ++i)
          if (raw_len[i] == s) keep[n_keep++] = i;
    }
    meta[0] = n_nodes; meta[1] = n_keep; meta[2] = n_raw; meta[3] = st; meta[4] = alive;
  }
  wave_global_sync();
  const int n_keep = meta[1];
  raw_found = meta[2];
  nodes_after = meta[4];
  if (meta[3] != 0) { finish(meta[3], 0); return; }

  // ---- shortcutPaths (568-582, parallel_shortcut: one iteration): lane i shortens kept raw path i into S[i]
  {
    int err = 0;
    if (lane < n_keep) {
      const unsigned short* rp = raw + (size_t)keep[lane] * TOPAY_TOPO_RAWLEN;
      const int n_in = raw_len[keep[lane]];
      auto in = [&](int j, double& x, double& y) { x = nd_pos[2 * rp[j]]; y = nd_pos[2 * rp[j] + 1]; };
      int n_out = 0, pushes = 0;
      const int r = topo_shortcut_iter(C, Mf, in, n_in, buf(R2 + lane), buf(lane), pt_cap, n_out, pushes);
      if (r < 0) err = r;
      else if (r == 2) {   // longer than the raw path: the raw path stays
        double* o = buf(lane);
        for (int j = 0; j < n_in; ++j) in(j, o[2 * j], o[2 * j + 1]);
        n_out = n_in;
      }
      pts_len[lane] = n_out;
    }
    if (__any(err != 0)) { finish(-1, 0); return; }
  }
  wave_global_sync();

  // ---- pruneEquivalent (346-382) over the shortened paths
  int exist[64];
  int n_exist = 0;
  if (n_keep > 0) {
    exist[n_exist++] = 0;
    for (int i = 1; i < n_keep; ++i) {
      bool new_path = true;
      for (int j = 0; j < n_exist && new_path; ++j) {
        int err = 0;
        const bool same = topo_same_topo(C, buf(i), pts_len[i], buf(exist[j]), pts_len[exist[j]], err);
        if (err) { finish(err, 0); return; }
        if (same) new_path = false;
      }
      if (new_path) exist[n_exist++] = i;
    }
  }
  n_filtered = n_exist;

  // ---- selectShortPaths (384-422): up to reserve_num paths, shortest first, while shorter than ratio_to_short x the shortest
  double mylen = 1.0e300;
  if (lane < n_exist) mylen = topo_path_length(buf(exist[lane]), pts_len[exist[lane]]);
  int sel[16];
  int n_sel = 0;
  double min_len = 0.0;
  for (int i = 0; i < P.reserve_num && i < n_exist; ++i) {
    int short_id = -1;
    double best = 100000000;
    for (int j = 0; j < n_exist; ++j) {
      const double lj = __shfl(mylen, j);
      if (lj < best) { short_id = j; best = lj; }
    }
    if (short_id < 0) break;   // (nothing below 1e8 is left: the reference would index with -1)
    if (i == 0) min_len = best;
    else if (!(best / min_len < P.ratio_to_short)) break;
    sel[n_sel++] = exist[short_id];
    if (lane == short_id) mylen = 1.0e300;   // erased from the list
  }
  // shortcutPath(path, i, 5) for the selected ones: lane k iterates S[sel[k]] -> T[k][0] -> T[k][1] -> T[k][0] ...
  int myfin = -1;
  {
    int err = 0;
    if (lane < n_sel) {
      int cur = sel[lane], n_cur = pts_len[cur];
      for (int it = 0; it < 5; ++it) {
        const int dst = 2 * R2 + 2 * lane + (it & 1);
        const double* src = buf(cur);
        auto in = [&](int j, double& x, double& y) { x = src[2 * j]; y = src[2 * j + 1]; };
        int n_out = 0, pushes = 0;
        const int r = topo_shortcut_iter(C, Mf, in, n_cur, buf(R2 + sel[lane]), buf(dst), pt_cap, n_out, pushes);
        if (r < 0) { err = r; break; }
        if (r == 2) break;                                      // no shorter: the input of this iteration is the result
        pts_len[dst] = n_out;
        cur = dst; n_cur = n_out;
        if (r == 1) break;                                      // (an empty discretisation is stored and ends the call)
      }
      myfin = cur;
    }
    if (__any(err != 0)) { finish(-1, 0); return; }
  }
  wave_global_sync();
  int fin[16];
  for (int k = 0; k < n_sel; ++k) fin[k] = __shfl(myfin, k);
  // pruneEquivalent of the selected paths
  int out_id[16];
  int n_out = 0;
  if (n_sel > 0) {
    out_id[n_out++] = fin[0];
    for (int i = 1; i < n_sel; ++i) {
      bool new_path = true;
      for (int j = 0; j < n_out && new_path; ++j) {
        int err = 0;
        const bool same = topo_same_topo(C, buf(fin[i]), pts_len[fin[i]], buf(out_id[j]), pts_len[out_id[j]], err);
        if (err) { finish(err, 0); return; }
        if (same) new_path = false;
      }
      if (new_path) out_id[n_out++] = fin[i];
    }
  }
  for (int k = 0; k < n_out && k < B.cap_paths; ++k) {
    const double* src = buf(out_id[k]);
    const int len = pts_len[out_id[k]];
    double* dst = B.path_xy + ((size_t)p * B.cap_paths + k) * B.cap_points * 2;
    for (int j = lane; j < len && j < B.cap_points; j += 64) { dst[2 * j] = src[2 * j]; dst[2 * j + 1] = src[2 * j + 1]; }
    if (lane == 0) B.path_len[(size_t)p * B.cap_paths + k] = len;
  }
  finish(n_out > 0 ? 1 : 0, n_out);
}

}  // namespace topay
