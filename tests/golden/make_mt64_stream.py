"""Writes mt64_stream.npz: the first 1000 outputs of the C++ library's std::mt19937_64 for three seeds (tests/test_world.py compares
the device's generator with them, all 64 bits).  Needs a C++ compiler (CXX, default g++).

    python tests/golden/make_mt64_stream.py
"""
import os, subprocess, sys, tempfile
import numpy as np

SEEDS = [1, 42, 2 ** 63 + 12345]
N = 1000
SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
int main(int argc, char** argv) {
  const int n = std::atoi(argv[1]);
  for (int a = 2; a < argc; a++) {
    std::mt19937_64 g(std::strtoull(argv[a], nullptr, 10));
    for (int i = 0; i < n; i++) std::printf("%llu\n", (unsigned long long)g());
  }
  return 0;
}
"""

here = os.path.dirname(os.path.abspath(__file__))
with tempfile.TemporaryDirectory() as d:
    src, exe = os.path.join(d, "mt64.cpp"), os.path.join(d, "mt64")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-o", exe, src])
    txt = subprocess.check_output([exe, str(N)] + [str(s) for s in SEEDS], text=True)
out = np.array([int(v) for v in txt.split()], dtype=np.uint64).reshape(len(SEEDS), N)
# a value known from elsewhere, so that a broken tool chain does not write a fixture
assert int(out[0, 0]) == 2469588189546311528, "mt19937_64(1) starts with 2469588189546311528"
np.savez(os.path.join(here, "mt64_stream.npz"), seeds=np.array(SEEDS, dtype=np.uint64), out=out)
print("wrote", os.path.join(here, "mt64_stream.npz"), out.shape, file=sys.stderr)
