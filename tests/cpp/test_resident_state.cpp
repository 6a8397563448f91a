// CPU test of direct_amd/csrc/resident_state.h (built with -fsanitize=address,undefined by tests/test_resident_state_cpp.py): every
// row of the event table of DESIGN.md 6.22 on a zero-initialised object with every column asserted after every row, random event
// sequences against a naive restatement kept here, the life cycle of the floor slots, the cap rule's texts, and what a zeroed
// object answers.  Prints PASS and returns 0, or says which check failed.
#include "../../direct_amd/csrc/resident_state.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <random>
#include <string>

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

namespace {
namespace rs = direct::resident;
namespace cc = direct::cubecor;

constexpr int32_t kUncapped = 0x3fffffff;  // what an uncapped field is built with: above every floor of these tests
const char* const kNoField = "no valid distance field: call direct_cluster_distance_field after the map changes";
const char* const kAboveCap = "min_d2 or n_penalty above the cap2 the distance field was built with";

// ---- the entry points of direct_cluster.hip as sequences of events, with the outcome given ----------------------------------
enum Outcome { kRefused, kDeviceError, kOk };

void set_map(rs::State& s, Outcome o) {  // (a set_map whose copy fails leaves "has a map" as it was)
  s.map_edit_began();
  if (o == kOk) s.map_ready();
}
void map_from_cloud(rs::State& s, Outcome o) {
  s.map_edit_began();
  if (o == kDeviceError) s.map_lost();
  if (o == kOk) s.map_ready();
}
void scan(rs::State& s, Outcome o, bool cells_changed) {
  if (o == kRefused) return;
  const bool had_map = s.has_map();
  s.scan_began();
  s.scan_ended(o == kDeviceError ? rs::ScanEnd::failed : (!had_map || cells_changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged));
}
void distance_field(rs::State& s, Outcome o, int32_t cap2) {
  s.field_call_began();
  if (o == kRefused || !s.has_map()) return;
  s.field_build_began();
  if (o == kOk) s.field_built(cap2);
}
bool free_components(rs::State& s, Outcome o, int32_t floor) {  // -> whether the call got past its refusals
  if (o == kRefused || !s.has_map() || (floor && s.field_refusal(floor, 0))) return false;
  s.label_build_began();
  if (o == kOk) s.labels_built(floor);
  return true;
}
void generation(rs::State& s, Outcome o, int n) {
  if (o == kRefused || !s.has_map()) return;
  s.clusters_overwritten();
  if (o == kOk) s.generation_left(n);
}
// cube_corridor_clear_batch in clear mode -> 1 built a table, 0 reused one, -1 refused or failed
int clear_corridors(rs::State& s, Outcome o, int32_t floor, long long count) {
  if (o == kRefused || !s.has_map() || s.field_refusal(floor, 0)) return -1;
  int hit = 1;
  const int slot = s.floor_chosen(floor, &hit);
  if (o == kDeviceError) {
    if (!hit) s.floor_build_failed(slot);
    return -1;
  }
  if (!hit) s.floor_built(slot, floor, count);
  s.floor_used(slot);
  return hit ? 0 : 1;
}

// ---- the columns ---------------------------------------------------------------------------------------------------------
bool floor_resident(const rs::State& s, int32_t floor) {  // asked of a copy: choosing a slot is an event
  rs::State c = s;
  int hit = 0;
  c.floor_chosen(floor, &hit);
  return hit != 0;
}
struct Cols {
  bool map, scan, field, floor2, labels;
  int clusters;
};
bool same(const Cols& a, const Cols& b) {
  return a.map == b.map && a.scan == b.scan && a.field == b.field && a.floor2 == b.floor2 && a.labels == b.labels && a.clusters == b.clusters;
}
Cols cols(const rs::State& s) {  // floor2: a clear corridor call with floor 2 would be served, and from a resident table
  return Cols{s.has_map(), s.has_scan_grid(), s.field_refusal(0, 0) == nullptr, !s.field_refusal(2, 0) && floor_resident(s, 2), s.labels_serve(),
              s.clusters_resident()};
}
#define ROW(s, ...) CHECK(same(cols(s), Cols{__VA_ARGS__}))

// ---- every row of the table, in one sequence: map, scan grid, field, floor table of 2, labels, clusters ------------------------
int table_rows() {
  rs::State s = {};
  ROW(s, false, false, false, false, false, 0);
  set_map(s, kOk);
  ROW(s, true, false, false, false, false, 0);
  distance_field(s, kOk, kUncapped);
  ROW(s, true, false, true, false, false, 0);
  CHECK(clear_corridors(s, kOk, 2, 7) == 1);  // a miss: built
  ROW(s, true, false, true, true, false, 0);
  CHECK(clear_corridors(s, kOk, 2, 9) == 0);  // a hit: the count is the build's
  CHECK(free_components(s, kOk, 2));
  ROW(s, true, false, true, true, true, 0);
  CHECK(s.labels_floor() == 2);
  generation(s, kOk, 2);
  ROW(s, true, false, true, true, true, 2);
  // set_map past its null check: field and labels stale at once; a device error leaves "has a map" as it was
  set_map(s, kDeviceError);
  ROW(s, true, false, false, false, false, 2);
  distance_field(s, kOk, kUncapped);
  CHECK(free_components(s, kOk, 0));
  ROW(s, true, false, true, false, true, 2);
  // map_from_cloud: stale also when refused; lost on a device error; ready on success
  map_from_cloud(s, kRefused);
  ROW(s, true, false, false, false, false, 2);
  map_from_cloud(s, kDeviceError);
  ROW(s, false, false, false, false, false, 2);
  map_from_cloud(s, kOk);
  ROW(s, true, false, false, false, false, 2);
  distance_field(s, kOk, kUncapped);
  CHECK(clear_corridors(s, kOk, 2, 7) == 1);
  CHECK(free_components(s, kOk, 2));
  ROW(s, true, false, true, true, true, 2);
  // map_integrate_scan: refused, unchanged, changed, failed; the grid is not present between its first touch and a good end
  scan(s, kRefused, true);
  ROW(s, true, false, true, true, true, 2);
  scan(s, kOk, false);
  ROW(s, true, true, true, true, true, 2);
  s.scan_began();
  ROW(s, true, false, true, true, true, 2);
  s.scan_ended(rs::ScanEnd::unchanged);
  ROW(s, true, true, true, true, true, 2);
  scan(s, kOk, true);
  ROW(s, true, true, false, false, false, 2);
  distance_field(s, kOk, kUncapped);
  CHECK(free_components(s, kOk, 2));
  scan(s, kDeviceError, false);
  ROW(s, false, false, false, false, false, 2);
  scan(s, kOk, false);  // no cell changed, but the handle had no map: changed
  ROW(s, true, true, false, false, false, 2);
  // distance_field: past its null check labels with a floor are stale, also when refused; floor-less labels stay
  distance_field(s, kOk, kUncapped);
  CHECK(clear_corridors(s, kOk, 2, 7) == 1);
  CHECK(free_components(s, kOk, 2));
  distance_field(s, kRefused, 0);
  ROW(s, true, true, true, true, false, 2);  // the field and its floor table are the old ones
  CHECK(free_components(s, kOk, 0));
  distance_field(s, kRefused, 0);
  ROW(s, true, true, true, true, true, 2);
  distance_field(s, kDeviceError, 0);  // past allocation: field stale
  ROW(s, true, true, false, false, true, 2);
  distance_field(s, kOk, 9);  // ready with its cap2; serial + 1: the floor table misses
  ROW(s, true, true, true, false, true, 2);
  CHECK(clear_corridors(s, kOk, 2, 7) == 1);
  CHECK(std::string(s.field_refusal(10, 0)) == kAboveCap);
  // free_components: past refusals the labels are stale; ready only on success
  CHECK(!free_components(s, kOk, 10));  // refused by the cap: the labels stay
  ROW(s, true, true, true, true, true, 2);
  CHECK(free_components(s, kDeviceError, 2));
  ROW(s, true, true, true, true, false, 2);
  CHECK(free_components(s, kOk, 2));
  ROW(s, true, true, true, true, true, 2);
  // the cluster storage
  generation(s, kRefused, 1);
  ROW(s, true, true, true, true, true, 2);
  generation(s, kDeviceError, 1);
  ROW(s, true, true, true, true, true, 0);
  generation(s, kOk, 1);
  ROW(s, true, true, true, true, true, 1);
  s.clusters_overwritten();  // convex_test, hull_planes_batch with caller voxels, corridor_batch
  ROW(s, true, true, true, true, true, 0);
  return 0;
}

// ---- the floor slots: two slots, three floors ------------------------------------------------------------------------------
int floor_slots() {
  static_assert(cc::kFloorSlots == 2, "the life cycle below is written for two slots");
  rs::State s = {};
  set_map(s, kOk);
  distance_field(s, kOk, kUncapped);
  int hit = 1;
  const int a = s.floor_chosen(2, &hit);  // a miss into an empty slot
  CHECK(!hit);
  CHECK(!floor_resident(s, 2));           // empty until its build has drained
  s.floor_built(a, 2, 11);
  s.floor_used(a);
  CHECK(floor_resident(s, 2) && s.floor_count(a) == 11);
  CHECK(s.floor_chosen(2, &hit) == a && hit);  // a hit
  s.floor_used(a);
  const int b = s.floor_chosen(4, &hit);  // a miss into the other empty slot
  CHECK(!hit && b != a);
  s.floor_built(b, 4, 22);
  s.floor_used(b);
  CHECK(s.floor_chosen(2, &hit) == a && hit);  // 2 is now the more recently used
  s.floor_used(a);
  CHECK(s.floor_chosen(5, &hit) == b && !hit);  // a miss into the least recently used slot: 4 goes
  CHECK(!floor_resident(s, 4) && !floor_resident(s, 5) && floor_resident(s, 2));
  s.floor_build_failed(b);  // a failed build leaves the slot empty
  CHECK(!floor_resident(s, 5));
  CHECK(s.floor_chosen(5, &hit) == b && !hit);  // and the next miss goes into it, not over 2
  s.floor_built(b, 5, 33);
  s.floor_used(b);
  CHECK(floor_resident(s, 5) && floor_resident(s, 2) && s.floor_count(b) == 33 && s.floor_count(a) == 11);
  distance_field(s, kRefused, 0);  // no new field: both stay
  CHECK(floor_resident(s, 5) && floor_resident(s, 2));
  distance_field(s, kOk, kUncapped);  // a new field serial misses everywhere
  CHECK(!floor_resident(s, 5) && !floor_resident(s, 2) && !floor_resident(s, 4));
  CHECK(clear_corridors(s, kOk, 2, 1) == 1 && clear_corridors(s, kOk, 2, 1) == 0);
  return 0;
}

// ---- the cap rule's texts, and a zeroed object ------------------------------------------------------------------------------
int cap_rule_and_zero() {
  unsigned char raw[sizeof(rs::State)];
  std::memset(raw, 0, sizeof raw);
  rs::State z;
  std::memcpy(&z, raw, sizeof z);
  CHECK(!z.has_map() && !z.has_scan_grid() && !z.labels_serve() && z.clusters_resident() == 0);
  CHECK(std::string(z.field_refusal(0, 0)) == kNoField && std::string(z.field_refusal(5, 7)) == kNoField);
  CHECK(std::memcmp(&z, raw, sizeof z) == 0);  // no question writes
  rs::State s = {};
  CHECK(std::memcmp(&s, raw, sizeof s) == 0);
  set_map(s, kOk);
  distance_field(s, kOk, 9);
  CHECK(!s.field_refusal(9, 9) && !s.field_refusal(0, 0));
  CHECK(std::string(s.field_refusal(10, 0)) == kAboveCap && std::string(s.field_refusal(0, 10)) == kAboveCap);
  distance_field(s, kOk, kUncapped);  // an uncapped field refuses nothing
  CHECK(!s.field_refusal(kUncapped, 65536) && !s.field_refusal(1 << 20, 0));
  set_map(s, kOk);
  CHECK(std::string(s.field_refusal(0, 0)) == kNoField);
  return 0;
}

// ---- random sequences against a naive restatement ---------------------------------------------------------------------------
// One boolean per product, and the number of the map edit / field build / field call a product was built from.
struct Model {
  bool map = false, scan = false, field = false, labels = false;
  int clusters = 0;
  long map_no = 0, build_no = 0, call_no = 0;  // map edits, successful field builds, field calls so far
  int32_t cap2 = 0;
  long labels_map = 0, labels_call = 0;
  int32_t labels_floor = 0;
  struct Table {
    bool held = false;
    int32_t floor = 0;
    long build = 0, used = 0;
  } tab[2];
  long clock = 0;

  void edit_map() { map_no++; field = false; }
  bool field_serves(int32_t floor) const { return field && floor <= cap2; }
  bool labels_serve() const { return labels && labels_map == map_no && (labels_floor == 0 || labels_call == call_no); }
  int table_of(int32_t floor) const {
    for (int k = 0; k < 2; k++)
      if (tab[k].held && tab[k].floor == floor && tab[k].build == build_no) return k;
    return -1;
  }
  int victim() const {
    for (int k = 0; k < 2; k++)
      if (!tab[k].held) return k;
    return tab[0].used <= tab[1].used ? 0 : 1;
  }
};

int random_sequences() {
  std::mt19937 rng(20261021u);
  const int32_t floors[3] = {2, 4, 5};
  for (int seq = 0; seq < 4000; seq++) {
    rs::State s = {};
    Model m;
    for (int step = 0; step < 48; step++) {
      const Outcome o = (Outcome)(rng() % 8 < 1 ? kRefused : (rng() % 8 < 1 ? kDeviceError : kOk));
      const int32_t floor = floors[rng() % 3];
      switch (rng() % 8) {
        case 0:
          set_map(s, o == kRefused ? kOk : o);
          m.edit_map();
          if (o != kDeviceError) m.map = true;
          break;
        case 1:
          map_from_cloud(s, o);
          m.edit_map();
          if (o != kRefused) m.map = o == kOk;
          break;
        case 2: {
          const bool cells = rng() % 2;
          scan(s, o, cells);
          if (o == kRefused) break;
          if (o == kDeviceError || cells || !m.map) m.edit_map();
          m.map = m.scan = o == kOk;
          break;
        }
        case 3: {
          const int32_t cap2 = rng() % 2 ? kUncapped : 4;
          distance_field(s, o, cap2);
          m.call_no++;
          if (o == kRefused || !m.map) break;
          m.field = o == kOk;
          if (o == kOk) { m.build_no++; m.cap2 = cap2; }
          break;
        }
        case 4: {
          const int32_t f = rng() % 3 ? floor : 0;
          const bool ran = free_components(s, o, f);
          CHECK(ran == (o != kRefused && m.map && (f == 0 || m.field_serves(f))));
          if (!ran) break;
          m.labels = o == kOk;
          m.labels_map = m.map_no; m.labels_call = m.call_no; m.labels_floor = f;
          break;
        }
        case 5: {
          const int n = 1 + (int)(rng() % 4);
          generation(s, o, n);
          if (o != kRefused && m.map) m.clusters = o == kOk ? n : 0;
          break;
        }
        case 6:
          s.clusters_overwritten();
          m.clusters = 0;
          break;
        default: {
          const int got = clear_corridors(s, o, floor, step);
          int want = -1;
          if (o != kRefused && m.map && m.field_serves(floor)) {
            int k = m.table_of(floor);
            const bool hit = k >= 0;
            if (!hit) {
              k = m.victim();
              m.tab[k].held = false;
            }
            if (o == kOk) {
              if (!hit) { m.tab[k].held = true; m.tab[k].floor = floor; m.tab[k].build = m.build_no; }
              m.tab[k].used = ++m.clock;
              want = hit ? 0 : 1;
            }
          }
          CHECK(got == want);
          break;
        }
      }
      CHECK(s.has_map() == m.map && s.has_scan_grid() == m.scan && s.clusters_resident() == m.clusters);
      CHECK(s.labels_serve() == m.labels_serve());
      if (m.labels_serve()) CHECK(s.labels_floor() == m.labels_floor);
      for (const int32_t f : {0, 2, 4, 5}) {
        const char* why = s.field_refusal(f, 0);
        CHECK((why == nullptr) == m.field_serves(f));
        if (why) CHECK(std::string(why) == (m.field ? kAboveCap : kNoField));
        if (f) CHECK(floor_resident(s, f) == (m.table_of(f) >= 0));
      }
    }
  }
  return 0;
}
}  // namespace

int main() {
  if (table_rows() || floor_slots() || cap_rule_and_zero() || random_sequences()) return 1;
  std::printf("PASS\n");
  return 0;
}
