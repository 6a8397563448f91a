// CPU test of the known grid's rows of direct_amd/csrc/resident_state.h (built with -fsanitize=address,undefined by
// tests/test_known_state_cpp.py): the rows DESIGN.md 6.22 has for the known grid on a zero-initialised object, and random event
// sequences against a naive restatement kept here, with the columns the known grid must NOT move asserted beside it.  Prints PASS
// and returns 0, or says which check failed.
#include "../../direct_amd/csrc/resident_state.h"

#include <cstdio>
#include <cstring>
#include <random>

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

namespace {
namespace rs = direct::resident;

enum Outcome { kRefused, kDeviceError, kOk };

// ---- the entry points of direct_cluster.hip as sequences of events, with the outcome given ----------------------------------
void scan(rs::State& s, Outcome o, bool track, bool cells_changed) {
  if (o == kRefused) return;  // unknown flags among them: the handle is left as it was
  const bool had_map = s.has_map();
  s.scan_began();
  if (track) s.known_scan_began();
  else s.known_dropped();
  s.scan_ended(o == kDeviceError ? rs::ScanEnd::failed : (!had_map || cells_changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged));
  if (track) s.known_ended(o == kOk);
}
void set_known(rs::State& s, Outcome o) {
  if (o == kRefused) return;
  s.known_dropped();
  if (o == kOk) s.known_set();
}
void set_map(rs::State& s, Outcome o) {
  s.map_edit_began();
  if (o == kOk) s.map_ready();
}
void map_from_cloud(rs::State& s, Outcome o) {
  s.map_edit_began();
  if (o == kDeviceError) s.map_lost();
  if (o == kOk) s.map_ready();
}
// what direct_cluster_frontier is refused with by the handle's state, in its order: 0 none, 5 no map, 6 no known grid, 7 the field
int frontier_refusal(const rs::State& s, int32_t min_d2) {
  if (!s.has_map()) return 5;
  if (!s.has_known()) return 6;
  if (min_d2 > 1 && s.field_refusal(min_d2, 0)) return 7;
  return 0;
}

int rows() {
  rs::State s;
  std::memset(&s, 0, sizeof(s));
  CHECK(!s.has_known() && !s.has_map() && !s.has_scan_grid());           // a zeroed State has no known grid
  CHECK(frontier_refusal(s, 0) == 5);
  scan(s, kOk, true, true);                                              // a tracked scan that ends well has one
  CHECK(s.has_known() && s.has_map() && s.has_scan_grid() && frontier_refusal(s, 0) == 0 && frontier_refusal(s, 4) == 7);
  scan(s, kRefused, false, false);                                       // a refused scan, tracked or not, leaves it
  scan(s, kRefused, true, false);
  CHECK(s.has_known());
  scan(s, kDeviceError, true, true);                                     // a failed tracked scan leaves none - and no scan grid, no map
  CHECK(!s.has_known() && !s.has_scan_grid() && !s.has_map());
  scan(s, kOk, true, true);
  CHECK(s.has_known());
  scan(s, kOk, false, false);                                            // an untracked scan drops it, and nothing else
  CHECK(!s.has_known() && s.has_scan_grid() && s.has_map() && frontier_refusal(s, 0) == 6);
  set_known(s, kOk);                                                     // set_known creates it
  CHECK(s.has_known() && frontier_refusal(s, 0) == 0);
  set_map(s, kOk);                                                       // set_map and map_from_cloud keep it
  CHECK(s.has_known());
  map_from_cloud(s, kOk);
  CHECK(s.has_known());
  map_from_cloud(s, kDeviceError);                                       // ... even when the map is lost: it describes observation
  CHECK(s.has_known() && !s.has_map() && frontier_refusal(s, 0) == 5);
  set_known(s, kDeviceError);                                            // a failed set_known leaves none
  CHECK(!s.has_known());
  set_known(s, kRefused);
  CHECK(!s.has_known());
  // the known grid's events move no other column: the field, its labels and the scan grid
  rs::State t;
  std::memset(&t, 0, sizeof(t));
  set_map(t, kOk);
  t.field_call_began(); t.field_build_began(); t.field_built(100);
  t.label_build_began(); t.labels_built(4);
  set_known(t, kOk);
  CHECK(t.has_known() && t.has_map() && !t.field_refusal(4, 0) && t.labels_serve() && frontier_refusal(t, 4) == 0 && frontier_refusal(t, 101) == 7);
  scan(t, kOk, true, false);                                             // a tracked scan that changes no cell keeps the field
  CHECK(t.has_known() && !t.field_refusal(4, 0) && t.labels_serve());
  scan(t, kOk, true, true);                                              // one that does makes it stale, as the untracked one
  CHECK(t.has_known() && t.field_refusal(4, 0) && !t.labels_serve() && frontier_refusal(t, 0) == 0 && frontier_refusal(t, 4) == 7);
  return 0;
}

int random_sequences() {
  std::mt19937 gen(11);
  for (int run = 0; run < 200; run++) {
    rs::State s;
    std::memset(&s, 0, sizeof(s));
    bool known = false;  // the restatement: one bit
    for (int step = 0; step < 60; step++) {
      const int ev = (int)(gen() % 5);
      const Outcome o = (Outcome)(gen() % 3);
      const bool track = gen() % 2, changed = gen() % 2;
      const bool map_before = s.has_map(), scan_before = s.has_scan_grid();
      if (ev == 0) {
        scan(s, o, track, changed);
        if (o != kRefused) known = track && o == kOk;
      } else if (ev == 1) {
        set_known(s, o);
        if (o != kRefused) known = o == kOk;
        CHECK(s.has_map() == map_before && s.has_scan_grid() == scan_before);
      } else if (ev == 2) {
        set_map(s, o);
      } else if (ev == 3) {
        map_from_cloud(s, o);
      } else {
        const rs::State before = s;  // a question writes nothing
        (void)frontier_refusal(s, (int32_t)(gen() % 6));
        CHECK(std::memcmp(&before, &s, sizeof(s)) == 0);
      }
      CHECK(s.has_known() == known);
    }
  }
  return 0;
}
}  // namespace

int main() {
  static_assert(sizeof(rs::State) <= 256, "the handle's state stays small");
  if (rows() || random_sequences()) return 1;
  std::printf("PASS\n");
  return 0;
}
