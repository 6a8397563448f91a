// Rules of direct_cluster_free_components / direct_cluster_reachable_batch (include/direct_cluster.h, "free-space components"):
// which voxels are enterable, the 13 forward neighbours in their fixed order, find / unite of the union-find, the flatten, size
// and stats rules, the rule that judges one (start, goal) pair, and the key that says whether a label set still serves.  Plain
// C++ behind a qualifier macro: the kernels of free_comp.h call these functions with atomics as their load / min primitives, and
// g++ compiles the same header with plain reads and writes for the CPU tests (tests/free_comp_harness.py).  Integers only: there
// is nothing a compiler could contract.
//
// The union-find links by smaller index, so at all times
//   (I1) parent[v] <= v for every enterable v (a root has parent[v] == v);
//   (I2) a word of parent only ever decreases (the one write primitive is a minimum);
//   (I3) v and parent[v] lie in the same component of the graph: sets only merge, and never across components;
//   (I4) a stale read is an older, larger ancestor or an older root: it costs another turn of a loop, never a wrong set.
// A set's root is its smallest index: the smallest element m has parent[m] <= m inside its own set, hence parent[m] == m.  So once
// every edge has been united the root of v is the smallest index of v's component, whatever order the unions ran in.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_FREECOMP_HD __host__ __device__ __forceinline__
#else
#define DIRECT_FREECOMP_HD inline
#endif

namespace direct {
namespace freecomp {

constexpr int kTile = 8;                         // voxels per tile edge: the grid paths' tiling (gridpath::kTile)
constexpr int kTileVox = kTile * kTile * kTile;
constexpr int kForward = 13;                     // the lexicographically positive half of the 26 offsets
// the codes of a pair: DIRECT_GRID_PATH_OK / _NO_PATH / _BAD_ENDPOINT
constexpr int kOk = 0, kNoPath = 1, kBadEndpoint = 2;
// bits of the sticky error word: a loop passed its trip bound, or a parent word broke (I1)
constexpr int kErrFind = 1, kErrUnite = 2, kErrParent = 4;

// min_d2 <= 1 is the graph without a floor (D2 is 0 exactly on occupied voxels): one normal form, 0
DIRECT_FREECOMP_HD int32_t normal_floor(int32_t min_d2) { return min_d2 <= 1 ? 0 : min_d2; }

// enterable(v) = map byte of v == 0 && (min_d2 <= 1 || D2[v] >= min_d2); d2 is not read (and may be null) without a floor
DIRECT_FREECOMP_HD bool enterable(const uint8_t* map, const int32_t* d2, long long v, int32_t min_d2) {
  return map[v] == 0 && (min_d2 <= 1 || d2[v] >= min_d2);
}

// Forward neighbour k = 0 .. 12 in ascending (dx, dy, dz) lexicographic order: (0, 0, 1), (0, 1, -1), ... (1, 1, 1)
DIRECT_FREECOMP_HD void forward_offset(int k, int& dx, int& dy, int& dz) {
  const int q = k + 14;
  dx = q / 9 - 1;
  dy = (q / 3) % 3 - 1;
  dz = q % 3 - 1;
}
// all 26, in the grid paths' order (the centre left out)
DIRECT_FREECOMP_HD void neighbour_offset(int k, int& dx, int& dy, int& dz) {
  const int q = k < 13 ? k : k + 1;
  dx = q / 9 - 1;
  dy = (q / 3) % 3 - 1;
  dz = q % 3 - 1;
}

// The root of v.  load(i) reads parent[i]; amin(i, x) stores min(parent[i], x) and returns what the word held.  Indices fall
// strictly along a chain, so it ends within `bound` (the number of words) steps.  On the way v is pointed at its grandparent
// (path halving): an ancestor, so (I1) - (I3) hold.
template <class Load, class Min>
DIRECT_FREECOMP_HD int find(Load load, Min amin, int v, int bound, int* err) {
  for (int trip = 0; trip <= bound; trip++) {
    const int p = load(v);
    if (p == v) return v;
    if (p < 0 || p > v) {
      *err |= kErrParent;
      return v;
    }
    const int gp = load(p);
    if (gp >= 0 && gp < p) amin(v, gp);
    v = p;
  }
  *err |= kErrFind;
  return v;
}
// find without a write: the flatten pass
template <class Load>
DIRECT_FREECOMP_HD int root_of(Load load, int v, int bound, int* err) {
  for (int trip = 0; trip <= bound; trip++) {
    const int p = load(v);
    if (p == v) return v;
    if (p < 0 || p > v) {
      *err |= kErrParent;
      return v;
    }
    v = p;
  }
  *err |= kErrFind;
  return v;
}

// Joins the sets of a and b, lock-free: find both roots, link the larger to the smaller with ONE minimum; if the word no longer
// held the larger root (someone linked it meanwhile, to `old`), the minimum has either changed nothing (old < lo) or replaced the
// link to old by one to lo - either way old and lo are what is left to join.  max(a, b) falls strictly from turn to turn, so the
// loop ends within `bound` turns.
template <class Load, class Min>
DIRECT_FREECOMP_HD void unite(Load load, Min amin, int a, int b, int bound, int* err) {
  for (int trip = 0; trip <= bound; trip++) {
    a = find(load, amin, a, bound, err);
    b = find(load, amin, b, bound, err);
    if (a == b || *err) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = amin(hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
  *err |= kErrUnite;
}

// Stats: the largest component as ONE 64-bit key whose maximum is order-independent: the larger size wins, then the smaller label
DIRECT_FREECOMP_HD unsigned long long stat_key(int32_t size, int32_t label) {
  return ((unsigned long long)(uint32_t)size << 32) | (uint32_t)(0x7fffffff - label);
}
DIRECT_FREECOMP_HD int32_t stat_size(unsigned long long key) { return (int32_t)(key >> 32); }
DIRECT_FREECOMP_HD int32_t stat_label(unsigned long long key) { return key ? 0x7fffffff - (int32_t)(key & 0xffffffffull) : -1; }

DIRECT_FREECOMP_HD bool inside(const int32_t* p, int X, int Y, int Z) {
  return p[0] >= 0 && p[0] < X && p[1] >= 0 && p[1] < Y && p[2] >= 0 && p[2] < Z;
}

// The code the path calls would return for the pair (s, g), OVERFLOW folded into OK (ROUND_LIMIT cannot be foretold).
// label_at(i) is label[i]: -1 exactly on voxels that are not enterable.  *goal_label: the goal's label, -1 when the goal is
// outside the map or not enterable.  The start's own byte and D2 are never looked at: a start that is not enterable leaves
// through any enterable neighbour.
template <class LabelAt>
DIRECT_FREECOMP_HD int reach_pair(const int32_t* s, const int32_t* g, int X, int Y, int Z, LabelAt label_at, int32_t* goal_label) {
  *goal_label = -1;
  const bool g_in = inside(g, X, Y, Z);
  int32_t gl = -1;
  if (g_in) gl = label_at((g[0] * Y + g[1]) * Z + g[2]);
  *goal_label = gl;
  if (!g_in || !inside(s, X, Y, Z)) return kBadEndpoint;
  if (s[0] == g[0] && s[1] == g[1] && s[2] == g[2]) return kOk;
  if (gl < 0) return kNoPath;
  const int32_t sl = label_at((s[0] * Y + s[1]) * Z + s[2]);
  if (sl >= 0) return sl == gl ? kOk : kNoPath;
  for (int k = 0; k < 26; k++) {
    int dx, dy, dz;
    neighbour_offset(k, dx, dy, dz);
    const int32_t n[3] = {s[0] + dx, s[1] + dy, s[2] + dz};
    if (inside(n, X, Y, Z) && label_at((n[0] * Y + n[1]) * Z + n[2]) == gl) return kOk;
  }
  return kNoPath;
}

// What a label set was built from.  It serves while the map has not been set again and, when it was built with a floor, no
// distance field call has run since; a set built without a floor never looked at the field.
struct Key {
  unsigned long long map_gen, field_gen;
  int32_t floor;   // normal form
  int32_t valid;
};
DIRECT_FREECOMP_HD bool key_serves(const Key& k, unsigned long long map_gen, unsigned long long field_gen) {
  return k.valid && k.map_gen == map_gen && (k.floor == 0 || k.field_gen == field_gen);
}

}  // namespace freecomp
}  // namespace direct
