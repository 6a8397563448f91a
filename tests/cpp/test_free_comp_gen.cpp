// C++ host-side check (GPU needed): direct::polyhedronGenerator::buildFreeComponents / reachable (direct_amd/host/poly_utils.hpp)
// against what ClusterGenerator.build_free_components / reachable returned for the same map, floor and pairs, which the caller
// recorded in the input file.  Before a build, and after the map has been set again, reachable throws.  The exit status is the
// number of disagreements.
//   usage: test_free_comp_gen <in.bin>
//   in.bin: int32 dims[3]; float64 res, lower[3]; uint8 map[X*Y*Z]; int32 n_floors; per floor: int32 min_d2; int64 stats[4];
//           int32 n; float64 starts[n][3], goals[n][3]; int32 rtn[n], goal_size[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../direct_amd/host/poly_utils.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(100); }
}

int main(int argc, char** argv) {
  if (argc < 2) return 100;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 100;
  int32_t dims[3], n_floors;
  double res;
  std::array<double, 3> lower;
  rd(f, dims, 3); rd(f, &res, 1); rd(f, lower.data(), 3);
  std::vector<uint8_t> map((size_t)dims[0] * dims[1] * dims[2]);
  rd(f, map.data(), map.size());
  rd(f, &n_floors, 1);
  direct::polyhedronGenerator gen(res, lower, dims[0], dims[1], dims[2], 1000, 0, 64, 4096, 64);
  gen.setMap(map.data());
  gen.buildDistanceField();
  int differ = 0;
  const std::vector<std::array<double, 3>> one = {{{lower[0], lower[1], lower[2]}}};
  auto refused = [&] {
    try { gen.reachable(one, one); } catch (const std::runtime_error&) { return true; }
    return false;
  };
  differ += refused() ? 0 : 1;  // no labels yet
  for (int k = 0; k < n_floors; k++) {
    int32_t min_d2, n;
    int64_t stats[4];
    rd(f, &min_d2, 1); rd(f, stats, 4); rd(f, &n, 1);
    std::vector<std::array<double, 3>> starts(n), goals(n);
    std::vector<int32_t> rtn(n), size(n), got_size;
    rd(f, &starts[0][0], (size_t)n * 3); rd(f, &goals[0][0], (size_t)n * 3); rd(f, rtn.data(), n); rd(f, size.data(), n);
    const direct::polyhedronGenerator::FreeComponents c = gen.buildFreeComponents(min_d2);
    const bool same_stats = c.enterable == stats[0] && c.components == stats[1] && c.largest == stats[2] && c.largest_label == stats[3];
    const std::vector<int32_t> got = gen.reachable(starts, goals, &got_size);
    int bad = 0;
    for (int i = 0; i < n; i++) bad += (got[i] == rtn[i] && got_size[i] == size[i]) ? 0 : 1;
    differ += bad + (same_stats ? 0 : 1);
    std::printf("min_d2 %d: %lld enterable voxels in %lld components, stats agree %d, %d of %d pairs differ\n", min_d2, c.enterable,
                c.components, (int)same_stats, bad, n);
  }
  gen.setMap(map.data());
  differ += refused() ? 0 : 1;  // the map was set again: stale
  std::fclose(f);
  return differ;
}
