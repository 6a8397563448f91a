// C++ host-side check (GPU needed): direct::polyhedronGenerator::integrateScan / getMap (direct_amd/host/poly_utils.hpp) against
// what ClusterGenerator.integrate_scan returned for the same sequence of scans, which the caller recorded in the input file.  The
// first scan follows a setMap of the recorded start map (so DIRECT_SCAN_ADOPT has something to adopt).  The exit status is the
// number of disagreements.
//   usage: test_map_scan_gen <in.bin>
//   in.bin: int32 dims[3]; float64 res, lower[3], origin[3], max_range; uint8 start_map[X*Y*Z]; int32 n_scans; per scan:
//           int32 mode, inflate[3], n; float32 xyz[n][3]; int64 stats[8]; uint8 map[X*Y*Z]
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
  int32_t dims[3], n_scans;
  double res, max_range;
  std::array<double, 3> lower, origin;
  rd(f, dims, 3); rd(f, &res, 1); rd(f, lower.data(), 3); rd(f, origin.data(), 3); rd(f, &max_range, 1);
  const size_t G = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<uint8_t> map(G);
  rd(f, map.data(), G);
  rd(f, &n_scans, 1);
  direct::polyhedronGenerator gen(res, lower, dims[0], dims[1], dims[2], 1000, 0, 2, 64, 64);
  gen.setMap(map.data());
  int differ = 0;
  for (int k = 0; k < n_scans; k++) {
    int32_t head[5];
    int64_t stats[8];
    rd(f, head, 5);
    std::vector<float> xyz((size_t)head[4] * 3);
    rd(f, xyz.data(), xyz.size()); rd(f, stats, 8); rd(f, map.data(), G);
    const direct::polyhedronGenerator::ScanResult r =
        gen.integrateScan(xyz.data(), head[4], 3, origin, max_range, {{head[1], head[2], head[3]}}, head[0]);
    const long long got[8] = {r.points, r.skipped_nonfinite, r.truncated, r.outside, r.raw_occupied, r.occupied, r.set, r.cleared};
    int bad = 0;
    for (int i = 0; i < 8; i++) bad += got[i] == stats[i] ? 0 : 1;
    bad += r.changed() == (stats[6] + stats[7] > 0) ? 0 : 1;
    bad += gen.getMap() == map ? 0 : 1;
    differ += bad;
    std::printf("scan %d (mode %d, %d points): %lld occupied, %lld set, %lld cleared, %d disagreements\n", k, head[0], head[4],
                r.occupied, r.set, r.cleared, bad);
  }
  try {  // an origin outside the map is refused, and says so
    gen.integrateScan(nullptr, 0, 3, {{lower[0] - 1.0, lower[1], lower[2]}}, max_range);
    differ++;
  } catch (const std::runtime_error&) {
  }
  std::fclose(f);
  return differ;
}
