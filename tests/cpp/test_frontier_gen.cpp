// C++ host-side check (GPU needed): direct::polyhedronGenerator::integrateScan(..., track_known) / getKnown / setKnown / frontiers
// (direct_amd/host/poly_utils.hpp) against what ClusterGenerator.integrate_scan / known_grid / frontiers returned for the same scan
// and the same calls, which the caller recorded in the input file.  Before a tracked scan, and after an untracked one, frontiers
// throws.  The exit status is the number of disagreements.
//   usage: test_frontier_gen <in.bin>
//   in.bin: int32 dims[3]; float64 res, lower[3], origin[3], max_range; int32 n; float32 xyz[n][3]; uint8 known[X*Y*Z];
//           int32 n_calls; per call: int32 min_size, min_d2, capacity; int64 stats[6]; int32 label[w], size[w], centroid[w][3],
//           rep[w][3] with w = stats[4]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../direct_amd/host/poly_utils.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(100); }
}

int main(int argc, char** argv) {
  if (argc < 2) return 100;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 100;
  int32_t dims[3], n, n_calls;
  double res, max_range;
  std::array<double, 3> lower, origin;
  rd(f, dims, 3); rd(f, &res, 1); rd(f, lower.data(), 3); rd(f, origin.data(), 3); rd(f, &max_range, 1); rd(f, &n, 1);
  std::vector<float> xyz((size_t)n * 3);
  rd(f, xyz.data(), xyz.size());
  std::vector<uint8_t> known((size_t)dims[0] * dims[1] * dims[2]);
  rd(f, known.data(), known.size());
  rd(f, &n_calls, 1);
  direct::polyhedronGenerator gen(res, lower, dims[0], dims[1], dims[2], 1000, 0, 2, 64, 64);
  auto refused = [&] {
    try { gen.frontiers(); } catch (const std::runtime_error&) { return true; }
    return false;
  };
  int differ = refused() ? 0 : 1;  // no map, no known grid
  gen.integrateScan(xyz.data(), n, 3, origin, max_range, {{0, 0, 0}}, DIRECT_SCAN_RESET, true);
  differ += gen.getKnown() == known ? 0 : 1;
  for (int k = 0; k < n_calls; k++) {
    int32_t par[3];
    int64_t stats[6];
    rd(f, par, 3); rd(f, stats, 6);
    const size_t w = (size_t)stats[4];
    std::vector<int32_t> label(w), size(w);
    std::vector<std::array<int32_t, 3>> centroid(w), rep(w);
    rd(f, label.data(), w); rd(f, size.data(), w); rd(f, w ? &centroid[0][0] : nullptr, 3 * w); rd(f, w ? &rep[0][0] : nullptr, 3 * w);
    const direct::polyhedronGenerator::Frontiers r = gen.frontiers(par[0], par[1], par[2]);
    const long long got[6] = {r.known, r.frontier, r.components, r.kept, r.written, r.largest};
    int bad = 0;
    for (int i = 0; i < 6; i++) bad += got[i] == stats[i] ? 0 : 1;
    bad += (r.label == label && r.size == size && r.centroid == centroid && r.rep == rep) ? 0 : 1;
    differ += bad;
    std::printf("min_size %d, min_d2 %d, capacity %d: %lld frontier voxels, %lld components, %lld kept, %lld written, %d disagreements\n",
                par[0], par[1], par[2], r.frontier, r.components, r.kept, r.written, bad);
  }
  gen.integrateScan(xyz.data(), n, 3, origin, max_range);  // untracked: the known grid is dropped
  differ += refused() ? 0 : 1;
  gen.setKnown(known.data());                              // ... and back
  differ += gen.getKnown() == known ? 0 : 1;
  differ += refused() ? 1 : 0;
  std::fclose(f);
  return differ;
}
