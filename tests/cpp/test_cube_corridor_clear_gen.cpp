// C++ host-side check (GPU needed): direct::polyhedronGenerator::cubeCorridorClearBatch (direct_amd/host/poly_utils.hpp) against
// the outputs of ClusterGenerator.cube_corridors_clear for the same map, paths and floor, which the caller recorded in the input
// file.  Planes, centres and seeds must agree bit for bit for both walks; the first call builds a floor table, the second reuses
// it; and without a distance field the call throws.  The exit status is the number of disagreements.
//   usage: test_cube_corridor_clear_gen <in.bin>
//   in.bin: the input format of test_corridor_gen.cpp; then int32 min_d2, cap; then for pop_back = 1, 0:
//           int32 n_seg[np], float64 planes[np][cap][6][4], centers[np][cap][3], seeds[np][cap][3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  int32_t dims[3], np, min_d2, cap;
  double res;
  std::array<double, 3> lower;
  rd(f, dims, 3); rd(f, &res, 1); rd(f, lower.data(), 3); rd(f, &np, 1);
  std::vector<std::vector<std::array<double, 3>>> paths(np);
  for (auto& p : paths) {
    int32_t len;
    rd(f, &len, 1);
    p.resize(len);
    rd(f, &p[0][0], (size_t)len * 3);
  }
  std::vector<uint8_t> map((size_t)dims[0] * dims[1] * dims[2]);
  rd(f, map.data(), map.size());
  rd(f, &min_d2, 1); rd(f, &cap, 1);
  direct::polyhedronGenerator gen(res, lower, dims[0], dims[1], dims[2], 1000, 0, 64, 4096, 64);
  gen.setMap(map.data());
  int differ = 0;
  {  // clear mode without a field is refused, never rebuilt silently; neutral mode needs none
    std::vector<direct::PlainCorridor> got(np);
    std::vector<direct::PlainCorridor*> pg;
    for (auto& c : got) pg.push_back(&c);
    bool thrown = false;
    try { gen.cubeCorridorClearBatch(paths, pg, min_d2, true); } catch (const std::runtime_error&) { thrown = true; }
    differ += thrown ? 0 : 1;
    for (const auto& c : got) differ += c.polyhedrons.empty() ? 0 : 1;
    gen.cubeCorridorClearBatch(paths, pg, 1, true);
    differ += gen.lastTableBuilt() ? 1 : 0;
  }
  gen.buildDistanceField();
  for (int pop = 1; pop >= 0; pop--) {
    std::vector<int32_t> n_seg(np);
    std::vector<double> planes((size_t)np * cap * 24), centers((size_t)np * cap * 3), seeds((size_t)np * cap * 3);
    rd(f, n_seg.data(), n_seg.size()); rd(f, planes.data(), planes.size()); rd(f, centers.data(), centers.size()); rd(f, seeds.data(), seeds.size());
    std::vector<direct::PlainCorridor> got(np);
    std::vector<direct::PlainCorridor*> pg;
    for (auto& c : got) pg.push_back(&c);
    const std::vector<bool> ok = gen.cubeCorridorClearBatch(paths, pg, min_d2, pop != 0);
    differ += gen.lastTableBuilt() == (pop == 1) ? 0 : 1;
    int kept = 0, bad = 0;
    for (int p = 0; p < np; p++) {
      bool same = ok[p] && (int)got[p].polyhedrons.size() == n_seg[p];
      for (int k = 0; same && k < n_seg[p]; k++) {
        const auto& q = got[p].polyhedrons[k];
        const size_t at = (size_t)p * cap + k;
        same = q.planes.size() == 6 && std::memcmp(q.center.data(), &centers[at * 3], 24) == 0 && std::memcmp(q.seed_coord.data(), &seeds[at * 3], 24) == 0;
        for (int j = 0; same && j < 6; j++) same = std::memcmp(q.planes[j].data(), &planes[(at * 6 + j) * 4], 32) == 0;
      }
      bad += same ? 0 : 1;
      kept += (int)got[p].polyhedrons.size();
    }
    differ += bad;
    std::printf("pop_back %d, min_d2 %d: %d paths, %d kept polytopes, table built %d, %d paths differ\n", pop, min_d2, np, kept,
                (int)gen.lastTableBuilt(), bad);
  }
  std::fclose(f);
  return differ;
}
