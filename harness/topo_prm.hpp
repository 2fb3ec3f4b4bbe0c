// CPU restatement of the topological roadmap of the front-end, TopologyPRM::findTopoPaths -- the checker of
// topay_topo_paths (topay_amd/csrc/topay_topo.h).  Reference: src/planner/src/topo_prm.cpp
//   findTopoPaths 60-122, createGraph 124-212, findVisibGuard 214-233, needConnection 235-263, getSample 265-276,
//   lineVisib 278-315, pruneGraph 317-344, pruneEquivalent 346-382, selectShortPaths 384-422, sameTopoPath 424-448,
//   shortestPath 450-461, pathLength 462-470, discretizePath(path, pt_num) 472-506, shortcutPath 512-566,
//   shortcutPaths 568-582, discretizeLine 584-597, discretizePath(path) 599-616, searchPaths 656-691,
//   depthFirstSearch 693-734;
// the ray caster src/planner/src/utils/raycast.cpp: signum / mod / intbound 31-48, RayCaster::setInput 253-300, step
// 302-346; the map queries src/map/include/map/grid_map.h: getDisWithGradI2d 364-441, boundIndex2d 727-733, posToIndex2d
// 744-759, indexToPos3d 785-795, getDistCoarse2d / 2i 887-940, getOffset 208; parameters src/planner/params/topo_prm.yaml.
//
// Written in the reference's own structure: an ordered std::list of nodes with neighbour vectors, a recursive depth-first
// search, std::vector paths of 3-vectors whose z is 0, serial loops.  The restatement is UNPINNED by the reference: the
// reference ships no vectors for this module and cannot be run here (ROS, Eigen).  Eigen is restated as: normalized() =
// component / sqrt(squared norm) and the vector itself when the squared norm is not positive (Eigen 3.3), norm() = sqrt of
// the sum of squares in x, y, z order, matrix * vector = row sums in column order.  What pins this file are the closed-form
// cases of tests/test_topo.py (empty map, one box, a wall, hand-worked rays).
//
// Where the reference is not reproducible this file and the device follow the same deterministic rules (include/topay.h,
// topay_topo_params_t):
//   - rand_pos_(eng_) (default_random_engine(rd_()), topo_prm.cpp:36-37, 268-269): draw `axis` of sample k of instance i
//     is 2 * mcrrt_u01(seed, i, k, axis) - 1;
//   - the 0.01 s of accumulated wall time (max_sample_time) is part of the count max_sample_num;
//   - status -1: the graph needs more than node_cap nodes, a node more than WL_TOPO_MAX_NB neighbours, or a discretised /
//     shortened path more than pt_cap points (the device's pools);
//   - status -2, undefined in the reference: a raw path of 100 nodes or more (path_list(100) is indexed by the size; the
//     search gives up as soon as its chain of visited nodes reaches 100), discretizePath finds no interval (idx = -1, lines
//     491-500; always so for pt_num == 1, where dl is a division by zero) or lands on an interval of zero length (lambda
//     is 0/0);
//     or the depth-first search has entered WL_TOPO_DFS_CAP nodes (it enumerates simple paths: no bound in the reference);
//   - a ray whose traversal has not reached the end cell after |dx| + |dy| steps (the number an exact traversal needs)
//     would run forever in the reference; it ends there and counts as visible.
// min_slack: the smallest distance of any discrete decision from its tie (arguments of floor / ceil / int() from an
// integer, len2 > len1, the two pathLength comparisons, rat < ratio_to_short, the 1e-4 windows of discretizePath, the
// 1e-3 test of the gradient's norm).  Comparisons of stored field values with clearance / thresh are exact on both sides.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <list>
#include <memory>
#include <vector>

#include "mcrrt.hpp"
#include "workload.hpp"

namespace topay_wl {

#define WL_TOPO_MAX_NB 32   // == TOPAY_TOPO_MAX_NB
#define WL_TOPO_DFS_CAP 2000000   // == TOPAY_TOPO_DFS_CAP: nodes the depth-first search may enter

struct TopoParams {   // == topay_topo_params_t
  double sample_inflate_x, sample_inflate_y, clearance, ratio_to_short;
  int max_sample_num, max_raw_path, max_raw_path2, reserve_num, node_cap, reserved;
  unsigned long long seed;
};

// points per discretised / shortened path the device keeps room for (topay_host_front.h: topo_pt_cap)
inline int topo_pt_cap(int nx, int ny) { return 2 * (int)std::ceil(std::sqrt((double)nx * nx + (double)ny * ny)) + 512; }

typedef std::array<double, 3> V3;
inline V3 operator+(const V3& a, const V3& b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline V3 operator-(const V3& a, const V3& b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline V3 operator*(double s, const V3& a) { return {s * a[0], s * a[1], s * a[2]}; }
inline V3 operator*(const V3& a, double s) { return {a[0] * s, a[1] * s, a[2] * s}; }
inline V3 operator/(const V3& a, double s) { return {a[0] / s, a[1] / s, a[2] / s}; }
inline double dot3(const V3& a, const V3& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double norm3(const V3& a) { return std::sqrt(dot3(a, a)); }
inline V3 normalized3(const V3& a) {
  const double z = dot3(a, a);
  if (z > 0.0) return a / std::sqrt(z);
  return a;
}
inline V3 cross3(const V3& a, const V3& b) { return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}; }

struct TopoAbort { int status; };

// RayCaster (raycast.cpp:253-346)
class RayCaster {
 public:
  static int signum(int x) { return x == 0 ? 0 : x < 0 ? -1 : 1; }
  static double mod(double value, double modulus) { return std::fmod(std::fmod(value, modulus) + modulus, modulus); }
  static double intbound(double s, double ds) {
    if (ds < 0) return intbound(-s, -ds);
    s = mod(s, 1);
    return (1 - s) / ds;
  }
  bool setInput(const V3& start, const V3& end) {
    start_ = start; end_ = end;
    x_ = (int)std::floor(start_[0]); y_ = (int)std::floor(start_[1]); z_ = (int)std::floor(start_[2]);
    endX_ = (int)std::floor(end_[0]); endY_ = (int)std::floor(end_[1]); endZ_ = (int)std::floor(end_[2]);
    dx_ = endX_ - x_; dy_ = endY_ - y_; dz_ = endZ_ - z_;
    stepX_ = signum((int)dx_); stepY_ = signum((int)dy_); stepZ_ = signum((int)dz_);
    tMaxX_ = intbound(start_[0], dx_); tMaxY_ = intbound(start_[1], dy_); tMaxZ_ = intbound(start_[2], dz_);
    tDeltaX_ = ((double)stepX_) / dx_; tDeltaY_ = ((double)stepY_) / dy_; tDeltaZ_ = ((double)stepZ_) / dz_;
    steps_left_ = std::abs(endX_ - x_) + std::abs(endY_ - y_) + std::abs(endZ_ - z_);
    if (stepX_ == 0 && stepY_ == 0 && stepZ_ == 0) return false;
    return true;
  }
  bool step(V3& ray_pt) {
    ray_pt = {(double)x_, (double)y_, (double)z_};
    if (x_ == endX_ && y_ == endY_ && z_ == endZ_) return false;
    if (steps_left_-- <= 0) return false;   // (the deterministic end of a traversal that missed its end cell, see the header)
    if (tMaxX_ < tMaxY_) {
      if (tMaxX_ < tMaxZ_) { x_ += stepX_; tMaxX_ += tDeltaX_; }
      else { z_ += stepZ_; tMaxZ_ += tDeltaZ_; }
    } else {
      if (tMaxY_ < tMaxZ_) { y_ += stepY_; tMaxY_ += tDeltaY_; }
      else { z_ += stepZ_; tMaxZ_ += tDeltaZ_; }
    }
    return true;
  }
  V3 start_, end_;
  int x_, y_, z_, endX_, endY_, endZ_, stepX_, stepY_, stepZ_, steps_left_;
  double dx_, dy_, dz_, tMaxX_, tMaxY_, tMaxZ_, tDeltaX_, tDeltaY_, tDeltaZ_;
};

class TopologyPRM {
 public:
  enum { Guard = 1, Connector = 2 };
  struct GraphNode {
    typedef std::shared_ptr<GraphNode> Ptr;
    V3 pos_;
    int type_, id_;
    std::vector<Ptr> neighbors_;
    GraphNode(const V3& p, int t, int id) : pos_(p), type_(t), id_(id) {}
  };
  typedef std::vector<V3> Path;

  const GridMap& gm;
  const double* inflate_;    // esdf_buffer_2d_inflate
  const double* critical_;   // esdf_buffer_2d_critical
  TopoParams prm;
  uint64_t inst;
  bool use_critical = false;
  double resolution_;
  V3 offset_;
  int pt_cap;
  // results and counters
  std::list<GraphNode::Ptr> graph_;
  std::vector<Path> raw_paths_, short_paths_, short_paths_first_;
  std::vector<Path> filtered_paths, select_paths;
  int samples_drawn = 0, samples_passed = 0, nodes_before = 0, nodes_after = 0, raw_found = 0;
  int n_moves = 0, n_pushes = 0, dfs_entries = 0;
  double min_slack = 1e300;
  bool track_slack = false;
  std::vector<std::array<int, 2>> visited_cells;   // cells a ray tested (filled when record_cells)
  bool record_cells = false;

  TopologyPRM(const GridMap& g, const double* inflate, const double* critical, const TopoParams& p, uint64_t instance)
      : gm(g), inflate_(inflate), critical_(critical), prm(p), inst(instance) {
    resolution_ = gm.resolution;
    for (int a = 0; a < 3; a++) offset_[a] = 0.5 - gm.origin[a] / gm.resolution;   // getOffset, grid_map.h:208
    pt_cap = topo_pt_cap(gm.voxel_num[0], gm.voxel_num[1]);
  }
  ~TopologyPRM() { for (auto& n : graph_) n->neighbors_.clear(); }   // (the neighbour pointers form cycles)

  void slack_int(double v) { if (track_slack) min_slack = std::min(min_slack, std::fabs(v - std::round(v))); }
  void slack_cmp(double a, double b) { if (track_slack) min_slack = std::min(min_slack, std::fabs(a - b)); }

  // ---- map queries
  double coarseAt(int ix, int iy) const {   // boundIndex2d + the field (grid_map.h:906-910, 933-937)
    ix = std::max(std::min(ix, gm.voxel_num[0] - 1), 0);
    iy = std::max(std::min(iy, gm.voxel_num[1] - 1), 0);
    return (use_critical ? critical_ : inflate_)[gm.addr2(ix, iy)];
  }
  double getDistCoarse2d(double px, double py) {
    const double fx = (px - gm.origin[0]) * gm.resolution_inv, fy = (py - gm.origin[1]) * gm.resolution_inv;
    slack_int(fx); slack_int(fy);
    return coarseAt((int)std::floor(fx), (int)std::floor(fy));
  }
  void indexToPos3d(const int id[3], V3& pos) const {
    for (int a = 0; a < 3; a++) pos[a] = (id[a] + 0.5) * gm.resolution + gm.origin[a];
  }
  // getDisWithGradI2d(pos, dist, grad, inflate = false, critical): the plain field, or the critical one
  void getDisWithGradI2d(double px, double py, double& distance, double grad[2]) {
    if (!gm.isInMap2d(px, py)) { distance = 0.0; grad[0] = grad[1] = 0.0; return; }
    const double p[2] = {px, py};
    int idx[2];
    double diff[2];
    for (int a = 0; a < 2; a++) {
      const double pm = p[a] - 0.5 * gm.resolution;
      const double f = (pm - gm.origin[a]) * gm.resolution_inv;
      slack_int(f);
      idx[a] = (int)std::floor(f);
      const double ip = (idx[a] + 0.5) * gm.resolution + gm.origin[a];
      diff[a] = (p[a] - ip) * gm.resolution_inv;
    }
    const double* field = use_critical ? critical_ : gm.esdf2d.data();
    double values[2][2];
    for (int x = 0; x < 2; x++)
      for (int y = 0; y < 2; y++) values[x][y] = field[gm.addr2(gm.bnd(idx[0] + x, 0), gm.bnd(idx[1] + y, 1))];
    const double v0 = values[0][0] * (1 - diff[0]) + values[1][0] * diff[0];
    const double v1 = values[0][1] * (1 - diff[0]) + values[1][1] * diff[0];
    distance = v0 * (1 - diff[1]) + v1 * diff[1];
    grad[1] = (v1 - v0) * gm.resolution_inv;
    grad[0] = (1 - diff[1]) * (values[1][0] - values[0][0]);
    grad[0] += diff[1] * (values[1][1] - values[0][1]);
    grad[0] *= gm.resolution_inv;
  }

  // ---- topo_prm.cpp:278-315
  bool lineVisib(const V3& p1, const V3& p2, double thresh, V3& pc) {
    V3 ray_pt;
    int pt_id[3];
    const V3 start = p1 / resolution_, end = p2 / resolution_;
    if (track_slack) for (int a = 0; a < 2; a++) { slack_int(start[a]); slack_int(end[a]); }
    RayCaster caster;
    const bool flag = caster.setInput(start, end);
    int prev[3] = {(int)std::floor(start[0]), (int)std::floor(start[1]), (int)std::floor(start[2])};
    while (flag && caster.step(ray_pt)) {
      pt_id[0] = (int)(ray_pt[0] + offset_[0]);
      pt_id[1] = (int)(ray_pt[1] + offset_[1]);
      pt_id[2] = 0;
      if (track_slack) { slack_int(ray_pt[0] + offset_[0]); slack_int(ray_pt[1] + offset_[1]); }
      if (record_cells) visited_cells.push_back({pt_id[0], pt_id[1]});
      const double dist = coarseAt(pt_id[0], pt_id[1]);
      if (dist <= thresh) {
        V3 pc1, pc2;
        indexToPos3d(pt_id, pc1);
        indexToPos3d(prev, pc2);
        pc = 0.5 * (pc1 + pc2);
        pc[2] = 0.0;
        return false;
      }
      for (int a = 0; a < 3; a++) prev[a] = pt_id[a];
    }
    return true;
  }

  // ---- topo_prm.cpp:265-276
  V3 getSample(int k) {
    V3 pt;
    pt[0] = (2.0 * mcrrt_u01(prm.seed, inst, (uint64_t)k, 0) - 1.0) * sample_r_[0];
    pt[1] = (2.0 * mcrrt_u01(prm.seed, inst, (uint64_t)k, 1) - 1.0) * sample_r_[1];
    pt[2] = 0.0;
    V3 r;
    for (int i = 0; i < 3; i++) r[i] = (rotation_[i][0] * pt[0] + rotation_[i][1] * pt[1] + rotation_[i][2] * pt[2]) + translation_[i];
    return r;
  }

  // ---- topo_prm.cpp:124-212
  void createGraph(const V3& start, const V3& end) {
    graph_.clear();
    graph_.push_back(std::make_shared<GraphNode>(start, Guard, 0));
    graph_.push_back(std::make_shared<GraphNode>(end, Guard, 1));
    sample_r_[0] = 0.5 * norm3(end - start) + prm.sample_inflate_x;
    sample_r_[1] = prm.sample_inflate_y;
    sample_r_[2] = 0.0;
    translation_ = 0.5 * (start + end);
    const V3 downward = {0, 0, -1};
    const V3 xtf = normalized3(end - translation_);
    const V3 ytf = normalized3(cross3(xtf, downward));
    const V3 ztf = cross3(xtf, ytf);
    for (int i = 0; i < 3; i++) { rotation_[i][0] = xtf[i]; rotation_[i][1] = ytf[i]; rotation_[i][2] = ztf[i]; }
    int node_id = 1;
    int sample_num = 0;
    while (sample_num < prm.max_sample_num) {
      const V3 pt = getSample(sample_num);
      ++sample_num;
      samples_drawn = sample_num;
      const double dist = getDistCoarse2d(pt[0], pt[1]);
      if (dist <= prm.clearance) continue;
      samples_passed++;
      std::vector<GraphNode::Ptr> visib_guards = findVisibGuard(pt);
      if (visib_guards.size() == 0) {
        if ((int)graph_.size() >= prm.node_cap) throw TopoAbort{-1};
        graph_.push_back(std::make_shared<GraphNode>(pt, Guard, ++node_id));
      } else if (visib_guards.size() == 2) {
        if (!needConnection(visib_guards[0], visib_guards[1], pt)) continue;
        if ((int)graph_.size() >= prm.node_cap) throw TopoAbort{-1};
        if ((int)visib_guards[0]->neighbors_.size() >= WL_TOPO_MAX_NB || (int)visib_guards[1]->neighbors_.size() >= WL_TOPO_MAX_NB) throw TopoAbort{-1};
        GraphNode::Ptr connector = std::make_shared<GraphNode>(pt, Connector, ++node_id);
        graph_.push_back(connector);
        visib_guards[0]->neighbors_.push_back(connector);
        visib_guards[1]->neighbors_.push_back(connector);
        connector->neighbors_.push_back(visib_guards[0]);
        connector->neighbors_.push_back(visib_guards[1]);
      }
    }
    nodes_before = (int)graph_.size();
    pruneGraph();
    nodes_after = (int)graph_.size();
  }

  // ---- topo_prm.cpp:214-233
  std::vector<GraphNode::Ptr> findVisibGuard(const V3& pt) {
    std::vector<GraphNode::Ptr> visib_guards;
    V3 pc;
    int visib_num = 0;
    for (auto iter = graph_.begin(); iter != graph_.end(); ++iter) {
      if ((*iter)->type_ == Connector) continue;
      if (lineVisib(pt, (*iter)->pos_, resolution_, pc)) {
        visib_guards.push_back(*iter);
        ++visib_num;
        if (visib_num > 2) break;
      }
    }
    return visib_guards;
  }

  // ---- topo_prm.cpp:235-263
  bool needConnection(GraphNode::Ptr g1, GraphNode::Ptr g2, const V3& pt) {
    Path path1(3), path2(3);
    path1[0] = g1->pos_; path1[1] = pt; path1[2] = g2->pos_;
    path2[0] = g1->pos_; path2[2] = g2->pos_;
    for (size_t i = 0; i < g1->neighbors_.size(); ++i)
      for (size_t j = 0; j < g2->neighbors_.size(); ++j)
        if (g1->neighbors_[i]->id_ == g2->neighbors_[j]->id_) {
          path2[1] = g1->neighbors_[i]->pos_;
          if (sameTopoPath(path1, path2, 0.0)) {
            const double l1 = pathLength(path1), l2 = pathLength(path2);
            slack_cmp(l1, l2);
            if (l1 < l2) { g1->neighbors_[i]->pos_ = pt; n_moves++; }   // line 254: the connector MOVES
            return false;
          }
        }
    return true;
  }

  // ---- topo_prm.cpp:317-344
  void pruneGraph() {
    if (graph_.size() > 2) {
      for (auto iter1 = graph_.begin(); iter1 != graph_.end() && graph_.size() > 2; ++iter1) {
        if ((*iter1)->id_ <= 1) continue;
        if ((*iter1)->neighbors_.size() <= 1) {
          for (auto iter2 = graph_.begin(); iter2 != graph_.end(); ++iter2)
            for (auto it_nb = (*iter2)->neighbors_.begin(); it_nb != (*iter2)->neighbors_.end(); ++it_nb)
              if ((*it_nb)->id_ == (*iter1)->id_) { (*iter2)->neighbors_.erase(it_nb); break; }
          (*iter1)->neighbors_.clear();   // (a shared_ptr cycle would keep the erased node alive; the reference leaks it)
          graph_.erase(iter1);
          iter1 = graph_.begin();
        }
      }
    }
  }

  // ---- topo_prm.cpp:656-734
  void searchPaths() {
    raw_paths_.clear();
    std::vector<GraphNode::Ptr> visited;
    visited.push_back(graph_.front());
    depthFirstSearch(visited);
    raw_found = (int)raw_paths_.size();
    int min_node_num = 100000, max_node_num = 1;
    std::vector<std::vector<int>> path_list(100);
    for (int i = 0; i < (int)raw_paths_.size(); ++i) {
      if ((int)raw_paths_[i].size() > max_node_num) max_node_num = (int)raw_paths_[i].size();
      if ((int)raw_paths_[i].size() < min_node_num) min_node_num = (int)raw_paths_[i].size();
      path_list[(int)raw_paths_[i].size()].push_back(i);
    }
    std::vector<Path> filter_raw_paths;
    for (int i = min_node_num; i <= max_node_num; ++i) {
      bool reach_max = false;
      for (size_t j = 0; j < path_list[i].size(); ++j) {
        filter_raw_paths.push_back(raw_paths_[path_list[i][j]]);
        if ((int)filter_raw_paths.size() >= prm.max_raw_path2) { reach_max = true; break; }
      }
      if (reach_max) break;
    }
    raw_paths_ = filter_raw_paths;
  }
  void depthFirstSearch(std::vector<GraphNode::Ptr>& vis) {
    if (vis.size() >= 100) throw TopoAbort{-2};   // any path from here has more than 100 nodes
    if (++dfs_entries > WL_TOPO_DFS_CAP) throw TopoAbort{-2};   // (the search is exponential in the worst case; the device gives up here too)
    GraphNode::Ptr cur = vis.back();
    for (size_t i = 0; i < cur->neighbors_.size(); ++i)
      if (cur->neighbors_[i]->id_ == 1) {
        Path path;
        for (size_t j = 0; j < vis.size(); ++j) path.push_back(vis[j]->pos_);
        path.push_back(cur->neighbors_[i]->pos_);
        if (path.size() >= 100) throw TopoAbort{-2};
        raw_paths_.push_back(path);
        if ((int)raw_paths_.size() >= prm.max_raw_path) return;
        break;
      }
    for (size_t i = 0; i < cur->neighbors_.size(); ++i) {
      if (cur->neighbors_[i]->id_ == 1) continue;
      bool revisit = false;
      for (size_t j = 0; j < vis.size(); ++j)
        if (cur->neighbors_[i]->id_ == vis[j]->id_) { revisit = true; break; }
      if (revisit) continue;
      vis.push_back(cur->neighbors_[i]);
      depthFirstSearch(vis);
      if ((int)raw_paths_.size() >= prm.max_raw_path) return;
      vis.pop_back();
    }
  }

  // ---- topo_prm.cpp:462-470, 450-461
  double pathLength(const Path& path) const {
    double length = 0.0;
    if (path.size() < 2) return length;
    for (size_t i = 0; i < path.size() - 1; ++i) length += norm3(path[i + 1] - path[i]);
    return length;
  }
  int shortestPath(std::vector<Path>& paths) {
    int short_id = -1;
    double min_len = 100000000;
    for (int i = 0; i < (int)paths.size(); ++i) {
      const double len = pathLength(paths[i]);
      slack_cmp(len, min_len);
      if (len < min_len) { short_id = i; min_len = len; }
    }
    return short_id;
  }

  // ---- topo_prm.cpp:472-506
  Path discretizePath(const Path& path, int pt_num) {
    if (path.size() < 2) throw TopoAbort{-2};   // (an empty shortened path: the reference's loops run on size() - 1 of an unsigned zero)
    std::vector<double> len_list;
    len_list.push_back(0.0);
    for (size_t i = 0; i + 1 < path.size(); ++i) len_list.push_back(norm3(path[i + 1] - path[i]) + len_list[i]);
    const double len_total = len_list.back();
    const double dl = len_total / double(pt_num - 1);
    Path dis_path;
    for (int i = 0; i < pt_num; ++i) {
      const double cur_l = double(i) * dl;
      int idx = -1;
      for (size_t j = 0; j + 1 < len_list.size(); ++j) {
        if (track_slack) { slack_cmp(cur_l, len_list[j] - 1e-4); slack_cmp(cur_l, len_list[j + 1] + 1e-4); }
        if (cur_l >= len_list[j] - 1e-4 && cur_l <= len_list[j + 1] + 1e-4) { idx = (int)j; break; }
      }
      if (idx < 0) throw TopoAbort{-2};
      const double den = len_list[idx + 1] - len_list[idx];
      if (!(den > 0.0)) throw TopoAbort{-2};
      const double lambda = (cur_l - len_list[idx]) / den;
      dis_path.push_back((1 - lambda) * path[idx] + lambda * path[idx + 1]);
    }
    return dis_path;
  }

  // ---- topo_prm.cpp:424-448
  bool sameTopoPath(const Path& path1, const Path& path2, double thresh) {
    const double len1 = pathLength(path1), len2 = pathLength(path2);
    const double max_len = std::max(len1, len2);
    slack_int(max_len / resolution_);
    const int pt_num = (int)std::ceil(max_len / resolution_);
    const Path pts1 = discretizePath(path1, pt_num), pts2 = discretizePath(path2, pt_num);
    V3 pc;
    for (int i = 0; i < pt_num; ++i)
      if (!lineVisib(pts1[i], pts2[i], thresh, pc)) return false;
    return true;
  }

  // ---- topo_prm.cpp:584-616
  Path discretizeLine(const V3& p1, const V3& p2) {
    const V3 dir = p2 - p1;
    const double len = norm3(dir);
    slack_int(len / resolution_);
    const int seg_num = (int)std::ceil(len / resolution_);
    Path line_pts;
    if (seg_num <= 0) return line_pts;
    for (int i = 0; i <= seg_num; ++i) line_pts.push_back(p1 + dir * double(i) / double(seg_num));
    return line_pts;
  }
  Path discretizePath(const Path& path) {
    Path dis_path, segment;
    if (path.size() < 2) return dis_path;
    for (size_t i = 0; i + 1 < path.size(); ++i) {
      segment = discretizeLine(path[i], path[i + 1]);
      if (segment.size() < 1) continue;
      dis_path.insert(dis_path.end(), segment.begin(), segment.end());
      if (i != path.size() - 2) dis_path.pop_back();
      if ((int)dis_path.size() > pt_cap) throw TopoAbort{-1};
    }
    return dis_path;
  }

  // ---- topo_prm.cpp:512-566
  void shortcutPath(Path path, int path_id, int iter_num) {
    Path short_path = path, last_path;
    for (int k = 0; k < iter_num; ++k) {
      last_path = short_path;
      Path dis_path = discretizePath(short_path);
      if (dis_path.size() < 2) { short_paths_[path_id] = dis_path; return; }
      V3 colli_pt, grad, dir, push_dir;
      double dist;
      short_path.clear();
      short_path.push_back(dis_path.front());
      for (size_t i = 1; i < dis_path.size(); ++i) {
        if (lineVisib(short_path.back(), dis_path[i], resolution_, colli_pt)) continue;
        double grad_2d[2];
        getDisWithGradI2d(colli_pt[0], colli_pt[1], dist, grad_2d);
        grad = {grad_2d[0], grad_2d[1], 0.0};
        slack_cmp(norm3(grad), 1e-3);
        if (norm3(grad) > 1e-3) {
          grad = normalized3(grad);
          dir = normalized3(dis_path[i] - short_path.back());
          push_dir = grad - dot3(grad, dir) * dir;
          push_dir = normalized3(push_dir);
          colli_pt = colli_pt + resolution_ * push_dir;
          n_pushes++;
        }
        short_path.push_back(colli_pt);
        if ((int)short_path.size() >= pt_cap) throw TopoAbort{-1};
      }
      short_path.push_back(dis_path.back());
      const double len1 = pathLength(last_path), len2 = pathLength(short_path);
      slack_cmp(len1, len2);
      if (len2 > len1) { short_path = last_path; break; }
    }
    short_paths_[path_id] = short_path;
  }
  void shortcutPaths() {   // parallel_shortcut: true -> iter_num = 1 for every raw path
    short_paths_.resize(raw_paths_.size());
    for (size_t i = 0; i < raw_paths_.size(); ++i) shortcutPath(raw_paths_[i], (int)i, 1);
  }

  // ---- topo_prm.cpp:346-382
  std::vector<Path> pruneEquivalent(std::vector<Path>& paths) {
    std::vector<Path> pruned_paths;
    if (paths.size() < 1) return pruned_paths;
    std::vector<int> exist_paths_id;
    exist_paths_id.push_back(0);
    for (int i = 1; i < (int)paths.size(); ++i) {
      bool new_path = true;
      for (size_t j = 0; j < exist_paths_id.size(); ++j)
        if (sameTopoPath(paths[i], paths[exist_paths_id[j]], 0.0)) { new_path = false; break; }
      if (new_path) exist_paths_id.push_back(i);
    }
    for (size_t i = 0; i < exist_paths_id.size(); ++i) pruned_paths.push_back(paths[exist_paths_id[i]]);
    return pruned_paths;
  }

  // ---- topo_prm.cpp:384-422
  std::vector<Path> selectShortPaths(std::vector<Path>& paths, int /*step*/) {
    std::vector<Path> short_paths;
    double min_len = 0.0;
    for (int i = 0; i < prm.reserve_num && paths.size() > 0; ++i) {
      const int path_id = shortestPath(paths);
      if (path_id < 0) break;   // (nothing shorter than 1e8 is left: the reference would index with -1; the device stops here too)
      if (i == 0) {
        short_paths.push_back(paths[path_id]);
        min_len = pathLength(paths[path_id]);
        paths.erase(paths.begin() + path_id);
      } else {
        const double rat = pathLength(paths[path_id]) / min_len;
        slack_cmp(rat, prm.ratio_to_short);
        if (rat < prm.ratio_to_short) {
          short_paths.push_back(paths[path_id]);
          paths.erase(paths.begin() + path_id);
        } else {
          break;
        }
      }
    }
    for (size_t i = 0; i < short_paths.size(); ++i) {
      shortcutPath(short_paths[i], (int)i, 5);
      short_paths[i] = short_paths_[i];
    }
    short_paths = pruneEquivalent(short_paths);
    return short_paths;
  }

  // ---- topo_prm.cpp:60-122.  Returns the status: 1 at least one path, 0 none, -1 / -2 see the header.
  int findTopoPaths(const V3& start, const V3& end, bool critical) {
    use_critical = critical;
    for (int a = 0; a < 3; a++) offset_[a] = 0.5 - gm.origin[a] / gm.resolution;
    try {
      createGraph(start, end);
      searchPaths();
      shortcutPaths();
      short_paths_first_ = short_paths_;
      filtered_paths = pruneEquivalent(short_paths_);
      n_filtered = (int)filtered_paths.size();
      std::vector<Path> work = filtered_paths;   // (selectShortPaths erases from its argument)
      select_paths = selectShortPaths(work, 1);
    } catch (const TopoAbort& a) {
      select_paths.clear();
      return a.status;
    }
    return select_paths.empty() ? 0 : 1;
  }
  int n_filtered = 0;

 private:
  V3 sample_r_, translation_;
  double rotation_[3][3];
};

}  // namespace topay_wl
