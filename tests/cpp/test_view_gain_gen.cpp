// C++ host-side check (GPU needed): direct::polyhedronGenerator::viewGain (direct_amd/host/poly_utils.hpp) against what
// ClusterGenerator.view_gain returned for the same map, known grid, candidates, direction sets and ranges, which the caller recorded
// in the input file.  Before the map and the known grid are set, viewGain throws.  The exit status is the number of disagreements.
//   usage: test_view_gain_gen <in.bin>
//   in.bin: int32 dims[3]; uint8 map[X*Y*Z], known[X*Y*Z]; int32 n, n_sets, n_dirs; int32 voxel[n][3], set[n];
//           float32 dirs[n_sets][n_dirs][3]; int32 n_calls; per call: float64 range_vox; int32 with_sets; int32 code[n], gain[n],
//           seen[n], ends[n][4]
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
  int32_t dims[3], n, n_sets, n_dirs, n_calls;
  rd(f, dims, 3);
  const size_t G = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<uint8_t> map(G), known(G);
  rd(f, map.data(), G); rd(f, known.data(), G);
  rd(f, &n, 1); rd(f, &n_sets, 1); rd(f, &n_dirs, 1);
  std::vector<std::array<int32_t, 3>> voxel(n);
  std::vector<int32_t> set(n);
  std::vector<std::array<float, 3>> dirs((size_t)n_sets * n_dirs);
  rd(f, n ? &voxel[0][0] : nullptr, 3 * (size_t)n); rd(f, set.data(), (size_t)n); rd(f, &dirs[0][0], 3 * dirs.size());
  rd(f, &n_calls, 1);
  direct::polyhedronGenerator gen(0.15, {{0.0, 0.0, 0.0}}, dims[0], dims[1], dims[2], 1000, 0, 2, 64, 64);
  auto refused = [&] {
    try { gen.viewGain(voxel, dirs, n_sets, 5.0); } catch (const std::runtime_error&) { return true; }
    return false;
  };
  int differ = refused() ? 0 : 1;  // no map
  gen.setMap(map.data());
  differ += refused() ? 0 : 1;     // no known grid
  gen.setKnown(known.data());
  for (int k = 0; k < n_calls; k++) {
    double range_vox;
    int32_t with_sets;
    rd(f, &range_vox, 1); rd(f, &with_sets, 1);
    std::vector<int32_t> code(n), gain(n), seen(n);
    std::vector<std::array<int32_t, 4>> ends(n);
    rd(f, code.data(), (size_t)n); rd(f, gain.data(), (size_t)n); rd(f, seen.data(), (size_t)n); rd(f, n ? &ends[0][0] : nullptr, 4 * (size_t)n);
    const direct::polyhedronGenerator::ViewGain r = gen.viewGain(voxel, dirs, n_sets, range_vox, with_sets ? &set : nullptr);
    const int bad = (r.code == code ? 0 : 1) + (r.gain == gain ? 0 : 1) + (r.seen == seen ? 0 : 1) + (r.ends == ends ? 0 : 1);
    differ += bad;
    long long total = 0;
    for (int32_t v : r.gain) total += v;
    std::printf("range_vox %g, %s: %d candidates, gain %lld in all, %d disagreements\n", range_vox, with_sets ? "sets" : "set 0", (int)n,
                total, bad);
  }
  differ += gen.getKnown() == known ? 0 : 1;  // ... and the call left the grids alone
  differ += gen.getMap() == map ? 0 : 1;
  std::fclose(f);
  return differ;
}
