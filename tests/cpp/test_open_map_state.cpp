// CPU test of the open map's rows of direct_amd/csrc/resident_state.h (built with -fsanitize=address,undefined by
// tests/test_open_map_state_cpp.py): the rows DESIGN.md 6.22 has for the open map on a zero-initialised object, and random event
// sequences against a naive restatement kept here, with the columns the open map must NOT move asserted beside it.
// Prints PASS and returns 0, or says which check failed.
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

// ---- the entry points of direct_cluster.hip as sequences of events, with the outcome given; `occupied`: the handle's policy ----
void scan_end(rs::State& s, Outcome o, bool track, bool cells_changed, bool had_map, bool occupied) {
  s.scan_ended(o == kDeviceError ? rs::ScanEnd::failed : (!had_map || cells_changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged));
  if (track) s.known_ended(o == kOk);
  if (o == kOk && occupied) s.open_map_ready();
}
void plain_scan(rs::State& s, Outcome o, bool track, bool cells_changed, bool occupied) {
  if (o == kRefused || (occupied && !track)) return;  // an untracked scan under the policy is refused
  const bool had_map = s.has_map();
  s.scan_began();
  if (track) s.known_scan_began();
  else s.known_dropped();
  s.evidence_dropped();
  scan_end(s, o, track, cells_changed, had_map, occupied);
}
void evidence_scan(rs::State& s, Outcome o, bool track, bool cells_changed, bool occupied) {
  if (o == kRefused || (occupied && !track)) return;
  const bool had_map = s.has_map();
  s.scan_began();
  s.evidence_scan_began();
  if (track) s.known_scan_began();
  else s.known_dropped();
  scan_end(s, o, track, cells_changed, had_map, occupied);
  s.evidence_ended(o == kOk);
}
void set_known(rs::State& s, Outcome o) {
  if (o == kRefused) return;
  s.known_dropped();
  if (o == kOk) s.known_set();
}
void set_evidence(rs::State& s, Outcome o) {
  if (o == kRefused) return;
  s.evidence_dropped();
  if (o == kOk) s.evidence_set();
}
void set_map(rs::State& s, Outcome o) {  // o == kRefused here: past the null check, failed before the map was ready
  s.map_edit_began();
  if (o == kOk) s.map_ready();
}
void map_from_cloud(rs::State& s, Outcome o) {
  s.map_edit_began();
  if (o == kDeviceError) s.map_lost();
  if (o == kOk) s.map_ready();
}
void distance_field(rs::State& s, Outcome o) {
  s.field_call_began();
  if (o == kRefused) return;
  s.field_build_began();
  if (o == kOk) s.field_built(100);
}
void ask_everything(const rs::State& s) {
  (void)s.has_map(); (void)s.has_scan_grid(); (void)s.has_known(); (void)s.has_evidence(); (void)s.has_open_map(); (void)s.field_refusal(4, 0);
  (void)s.labels_serve(); (void)s.labels_floor(); (void)s.clusters_resident(); (void)s.floor_count(0);
}

int rows() {
  rs::State s;
  std::memset(&s, 0, sizeof(s));
  CHECK(!s.has_open_map() && !s.has_map());                       // a zeroed State has no open map
  plain_scan(s, kOk, true, true, false);                          // a scan under FREE: stays lost
  CHECK(!s.has_open_map() && s.has_map() && s.has_scan_grid() && s.has_known());
  plain_scan(s, kOk, true, true, true);                           // a successful scan under OCCUPIED: ready
  CHECK(s.has_open_map() && s.has_map() && s.has_scan_grid() && s.has_known());
  plain_scan(s, kRefused, true, true, true);                      // a refused scan keeps it ...
  plain_scan(s, kOk, false, true, true);                          // ... and so does the untracked one, which the policy refuses
  CHECK(s.has_open_map() && s.has_known());
  {                                                               // any scan past its refusals: lost until it has ended well
    rs::State mid = s;
    mid.scan_began();
    CHECK(!mid.has_open_map() && !mid.has_scan_grid());
  }
  plain_scan(s, kOk, true, false, true);                          // a scan that changes no cell leaves a new one, and the field stands
  CHECK(s.has_open_map());
  evidence_scan(s, kOk, true, true, true);                        // the evidence scan as the plain one
  CHECK(s.has_open_map() && s.has_evidence());
  evidence_scan(s, kDeviceError, true, true, true);               // a device error: stays lost
  CHECK(!s.has_open_map() && !s.has_map());
  evidence_scan(s, kOk, true, true, true);
  CHECK(s.has_open_map());
  plain_scan(s, kOk, true, false, false);                         // a scan under FREE past its refusals loses it, changed cells or not
  CHECK(!s.has_open_map() && s.has_map());
  plain_scan(s, kOk, true, true, true);
  set_map(s, kOk);                                                // set_map past its null check: lost
  CHECK(!s.has_open_map() && s.has_map());
  plain_scan(s, kOk, true, true, true);
  set_map(s, kRefused);                                           // ... whatever becomes of the call
  CHECK(!s.has_open_map());
  plain_scan(s, kOk, true, true, true);
  map_from_cloud(s, kRefused);                                    // map_from_cloud alike: refused, failed or well ended
  CHECK(!s.has_open_map());
  plain_scan(s, kOk, true, true, true);
  map_from_cloud(s, kDeviceError);
  CHECK(!s.has_open_map() && !s.has_map());
  plain_scan(s, kOk, true, true, true);
  map_from_cloud(s, kOk);
  CHECK(!s.has_open_map() && s.has_map());
  // every other row keeps it, and its events move no other column
  plain_scan(s, kOk, true, true, true);
  distance_field(s, kOk);
  s.label_build_began(); s.labels_built(4);
  s.generation_left(3);
  CHECK(s.has_open_map() && !s.field_refusal(4, 0) && s.labels_serve() && s.clusters_resident() == 3);
  set_known(s, kOk); set_known(s, kDeviceError); set_evidence(s, kOk); set_evidence(s, kDeviceError);
  distance_field(s, kRefused); s.clusters_overwritten();
  int hit = 0;
  s.floor_used(s.floor_chosen(4, &hit));
  CHECK(s.has_open_map() && s.has_map() && s.has_scan_grid());
  distance_field(s, kOk);
  s.label_build_began(); s.labels_built(0);
  rs::State t = s;
  t.open_map_ready();                                             // ready on ready: nothing else moves
  CHECK(std::memcmp(&t, &s, sizeof(s)) == 0);
  plain_scan(s, kOk, true, false, true);                          // nothing learned under the policy: field and labels still serve
  CHECK(s.has_open_map() && !s.field_refusal(4, 0) && s.labels_serve());
  plain_scan(s, kOk, true, true, true);                           // something learned: stale, and a new open map
  CHECK(s.has_open_map() && s.field_refusal(4, 0) && !s.labels_serve());
  return 0;
}

int random_sequences() {
  std::mt19937 gen(29);
  for (int run = 0; run < 300; run++) {
    rs::State s;
    std::memset(&s, 0, sizeof(s));
    bool open = false, evid = false, known = false, map = false, scan = false;  // the restatement: five bits
    for (int step = 0; step < 80; step++) {
      const int ev = (int)(gen() % 9);
      const Outcome o = (Outcome)(gen() % 3);
      const bool track = gen() % 2, changed = gen() % 2, occupied = gen() % 2;
      if (ev == 0 || ev == 1) {
        if (ev == 0) evidence_scan(s, o, track, changed, occupied);
        else plain_scan(s, o, track, changed, occupied);
        if (o != kRefused && !(occupied && !track)) {
          open = occupied && o == kOk;
          evid = ev == 0 && o == kOk;
          known = track && o == kOk;
          map = scan = o == kOk;
        }
      } else if (ev == 2) {
        set_evidence(s, o);
        if (o != kRefused) evid = o == kOk;
      } else if (ev == 3) {
        set_known(s, o);
        if (o != kRefused) known = o == kOk;
      } else if (ev == 4) {
        set_map(s, o);
        open = false;
        if (o == kOk) map = true;
      } else if (ev == 5) {
        map_from_cloud(s, o);
        open = false;
        if (o == kDeviceError) map = false;
        if (o == kOk) map = true;
      } else if (ev == 6) {
        distance_field(s, o);
      } else if (ev == 7) {
        s.label_build_began();
        if (o == kOk) s.labels_built(0);
      } else {
        const rs::State before = s;  // a question writes nothing
        ask_everything(s);
        CHECK(std::memcmp(&before, &s, sizeof(s)) == 0);
      }
      CHECK(s.has_open_map() == open && s.has_evidence() == evid && s.has_known() == known && s.has_map() == map && s.has_scan_grid() == scan);
      CHECK(!s.has_open_map() || (s.has_map() && s.has_scan_grid()));  // an open map stands beside the map of the scan that wrote both
    }
  }
  return 0;
}
}  // namespace

int main() {
  static_assert(sizeof(rs::State) <= 256, "the handle's state stays small");
  static_assert(std::is_trivially_copyable<rs::State>::value, "plain data");
  if (rows() || random_sequences()) return 1;
  std::printf("PASS\n");
  return 0;
}
