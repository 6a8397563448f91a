// C++ host-side check (GPU needed): direct::polyhedronGenerator::clusterCorridorBatch (direct_amd/host/poly_utils.hpp), the walk on
// the device, against the lock-step walks of the same class on the same generator (itr_cluster_max as given): corridorGenerationBatch
// for pop_back = true, corridorInsertGenerationBatch into empty corridors for pop_back = false.  Planes, centres and seeds must
// agree bit for bit and every path must complete; the exit status is the number of paths that differ.
//   usage: test_cluster_corridor_gen <in.bin> <itr_cluster_max> <capacity>     (the input format of test_corridor_gen.cpp)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../direct_amd/host/poly_utils.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(100); }
}

static bool same(const direct::PlainCorridor& a, const direct::PlainCorridor& b) {
  if (a.polyhedrons.size() != b.polyhedrons.size()) return false;
  for (size_t k = 0; k < a.polyhedrons.size(); k++) {
    const auto &p = a.polyhedrons[k], &q = b.polyhedrons[k];
    if (p.planes.size() != q.planes.size()) return false;
    for (size_t j = 0; j < p.planes.size(); j++)
      if (std::memcmp(p.planes[j].data(), q.planes[j].data(), 32) != 0) return false;
    if (std::memcmp(p.center.data(), q.center.data(), 24) != 0 || std::memcmp(p.seed_coord.data(), q.seed_coord.data(), 24) != 0) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) return 100;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 100;
  const int itr_cluster_max = std::atoi(argv[2]), capacity = std::atoi(argv[3]);
  int32_t dims[3], np;
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
  std::fclose(f);
  direct::polyhedronGenerator gen(res, lower, dims[0], dims[1], dims[2], 1000, itr_cluster_max, 8, capacity, capacity);
  gen.setMap(map.data());
  int differ = 0;
  for (int pop = 1; pop >= 0; pop--) {
    std::vector<direct::PlainCorridor> want(np), got(np);
    std::vector<direct::PlainCorridor*> pw, pg;
    for (auto& c : want) pw.push_back(&c);
    for (auto& c : got) pg.push_back(&c);
    if (pop) {
      const std::vector<bool> ok = gen.corridorGenerationBatch(paths, pw);
      for (int p = 0; p < np; p++) differ += ok[p] ? 0 : 1;
    } else {
      const std::vector<int> ok = gen.corridorInsertGenerationBatch(paths, pw);
      for (int p = 0; p < np; p++) differ += ok[p] == 1 ? 0 : 1;
    }
    const int rounds = gen.lastRounds(), polytopes = gen.lastPolytopes();
    const std::vector<bool> ok = gen.clusterCorridorBatch(paths, pg, pop != 0);
    int kept = 0;
    for (int p = 0; p < np; p++) {
      differ += (ok[p] && same(want[p], got[p])) ? 0 : 1;
      kept += (int)got[p].polyhedrons.size();
    }
    if (gen.lastRounds() != rounds || gen.lastPolytopes() != polytopes) differ++;
    std::printf("pop_back %d: %d paths, lock step %d rounds for %d polytopes; on the device %d rounds, %d due, %d generated, %d kept, %d differ so far\n",
                pop, np, rounds, polytopes, gen.lastRounds(), gen.lastPolytopes(), gen.lastUniqueSeeds(), kept, differ);
  }
  return differ;
}
