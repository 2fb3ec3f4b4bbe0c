// Stand-alone sanitizer pass over the sensor-cloud entries (topay_sense_*) through the CPU lane-emulator build of the kernel
// sources: reset, three inserts (a plain cloud, one through the intensity filter, one into an open batch), commit, get.
// Build and run from the repository root (host only; no device, no Python):
//   g++ -O1 -g -std=c++17 -march=x86-64-v3 -ffp-contract=off -DTOPAY_LDS= -DTOPAY_GLB= -DTOPAY_CST= -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -I tests/emu/include -x c++ topay_amd/csrc/topay_hip.hip tools/sense_sanitize.cpp \
//       -o sense_sanitize -ldl -lpthread && ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 ./sense_sanitize
// (detect_leaks=0: the emulator keeps the stacks of its lane fibres for the life of the process; the compile takes several minutes)
#include <cstdio>
#include <vector>

#include "../include/topay.h"

#define CHECK(call)                                                                     \
  do {                                                                                  \
    const int s_ = (call);                                                              \
    if (s_ != 0) { printf("%s -> %d (%s)\n", #call, s_, topay_last_error()); return 1; } \
  } while (0)

int main() {
  topay_params_t prm;
  CHECK(topay_default_params(&prm));
  topay_ctx* c = nullptr;
  CHECK(topay_create(&prm, 0, &c));
  topay_map_desc_t d = {{-1.2, -1.2, 0.0}, 0.1, {24, 24, 16}, {-1.2, -1.2, 0.0}, {1.2, 1.2, 1.6}};
  const int ids[2] = {3, 4};
  CHECK(topay_sense_reset(c, 2, ids, &d));
  topay_sense_params_t sp;
  CHECK(topay_sense_default_params(&sp));
  sp.point_filt_num = 2;
  std::vector<float> pts;
  unsigned r = 12345u;
  auto uni = [&](float lo, float hi) { r = r * 1664525u + 1013904223u; return lo + (hi - lo) * (float)(r >> 8) / 16777216.0f; };
  for (int i = 0; i < 700; i++) { pts.push_back(uni(-2.f, 2.f)); pts.push_back(uni(-2.f, 2.f)); pts.push_back(uni(-0.3f, 2.f)); pts.push_back((float)(i % 3) * 4.f); }
  const int off[3] = {0, 400, 700};
  const double sensor[6] = {0.05, 0.05, 0.55, -0.4, 0.3, 0.9};
  int st[2];
  CHECK(topay_sense_insert(c, 2, ids, off, pts.data(), sensor, &sp, st));
  sp.intensity_thresh = 3;
  CHECK(topay_sense_insert(c, 2, ids, off, pts.data(), sensor, &sp, st));
  sp.batch_update_size = 2;
  CHECK(topay_sense_insert(c, 2, ids, off, pts.data(), sensor, &sp, st));
  CHECK(topay_sense_commit(c, 2, ids));
  std::vector<float> lo(24 * 24 * 16);
  std::vector<int> op(lo.size()), hit(lo.size());
  int bc = -1, touched = 0, counted = 0;
  CHECK(topay_sense_get(c, 3, lo.data(), op.data(), hit.data(), &bc));
  for (size_t i = 0; i < lo.size(); i++) { touched += lo[i] != 0.f; counted += op[i] > 0; }
  std::vector<signed char> o3(lo.size());
  CHECK(topay_get_occupancy(c, 4, nullptr, nullptr, o3.data()));
  int occ = 0;
  for (signed char v : o3) occ += v;
  printf("sense_sanitize ok: %d voxels with a belief, %d with open counts, batch counter %d, %d occupied in slot 4\n", touched, counted, bc, occ);
  topay_destroy(c);
  return (touched > 0 && counted > 0 && bc == 1) ? 0 : 2;
}
