// CPU test of the evidence grid's rows of direct_amd/csrc/resident_state.h (built with -fsanitize=address,undefined by
// tests/test_evidence_state_cpp.py): the rows DESIGN.md 6.22 has for the evidence grid on a zero-initialised object, and random
// event sequences against a naive restatement kept here, with the columns the evidence grid must NOT move asserted beside it.
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

// ---- the entry points of direct_cluster.hip as sequences of events, with the outcome given ----------------------------------
void plain_scan(rs::State& s, Outcome o, bool track, bool cells_changed) {
  if (o == kRefused) return;
  const bool had_map = s.has_map();
  s.scan_began();
  if (track) s.known_scan_began();
  else s.known_dropped();
  s.evidence_dropped();
  s.scan_ended(o == kDeviceError ? rs::ScanEnd::failed : (!had_map || cells_changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged));
  if (track) s.known_ended(o == kOk);
}
void evidence_scan(rs::State& s, Outcome o, bool track, bool cells_changed) {
  if (o == kRefused) return;
  const bool had_map = s.has_map();
  s.scan_began();
  s.evidence_scan_began();
  if (track) s.known_scan_began();
  else s.known_dropped();
  s.scan_ended(o == kDeviceError ? rs::ScanEnd::failed : (!had_map || cells_changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged));
  if (track) s.known_ended(o == kOk);
  s.evidence_ended(o == kOk);
}
void set_evidence(rs::State& s, Outcome o) {
  if (o == kRefused) return;
  s.evidence_dropped();
  if (o == kOk) s.evidence_set();
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
// every question there is: none may write
void ask_everything(const rs::State& s) {
  (void)s.has_map(); (void)s.has_scan_grid(); (void)s.has_known(); (void)s.has_evidence(); (void)s.field_refusal(4, 0);
  (void)s.labels_serve(); (void)s.labels_floor(); (void)s.clusters_resident(); (void)s.floor_count(0);
}

int rows() {
  rs::State s;
  std::memset(&s, 0, sizeof(s));
  CHECK(!s.has_evidence() && !s.has_known() && !s.has_map() && !s.has_scan_grid());   // a zeroed State has no evidence grid
  evidence_scan(s, kRefused, true, true);                                             // a refused call leaves everything
  CHECK(!s.has_evidence() && !s.has_map() && !s.has_scan_grid());
  evidence_scan(s, kOk, false, true);                                                 // success makes it ready, with map and scan grid
  CHECK(s.has_evidence() && s.has_map() && s.has_scan_grid() && !s.has_known());
  evidence_scan(s, kRefused, false, false);                                           // a refused call keeps the column
  CHECK(s.has_evidence());
  {                                                                                   // past the refusals it is lost until the call has ended well
    rs::State mid = s;
    mid.scan_began();
    mid.evidence_scan_began();
    CHECK(!mid.has_evidence() && !mid.has_scan_grid());
  }
  evidence_scan(s, kDeviceError, true, true);                                         // a device error loses it - and map, scan grid, known grid
  CHECK(!s.has_evidence() && !s.has_map() && !s.has_scan_grid() && !s.has_known());
  evidence_scan(s, kOk, true, true);                                                  // a tracked one leaves a known grid too
  CHECK(s.has_evidence() && s.has_known() && s.has_map() && s.has_scan_grid());
  evidence_scan(s, kOk, false, false);                                                // an untracked one drops the known grid, as the plain scan
  CHECK(s.has_evidence() && !s.has_known());
  plain_scan(s, kRefused, false, false);                                              // a refused plain scan keeps the evidence
  CHECK(s.has_evidence());
  plain_scan(s, kOk, true, false);                                                    // a plain scan past its refusals loses it, and nothing else
  CHECK(!s.has_evidence() && s.has_map() && s.has_scan_grid() && s.has_known());
  set_evidence(s, kOk);                                                               // set_evidence: ready once drained
  CHECK(s.has_evidence() && s.has_map() && s.has_scan_grid() && s.has_known());
  set_evidence(s, kRefused);
  CHECK(s.has_evidence());
  set_map(s, kOk);                                                                    // set_map and map_from_cloud keep it
  CHECK(s.has_evidence());
  map_from_cloud(s, kOk);
  CHECK(s.has_evidence());
  map_from_cloud(s, kDeviceError);                                                    // ... even when the map is lost: it describes observation
  CHECK(s.has_evidence() && !s.has_map());
  set_known(s, kOk);                                                                  // the known grid's events do not move it
  set_known(s, kDeviceError);
  CHECK(s.has_evidence());
  set_evidence(s, kDeviceError);                                                      // a failed set_evidence loses it
  CHECK(!s.has_evidence());
  plain_scan(s, kDeviceError, false, true);
  CHECK(!s.has_evidence());
  // the evidence grid's events move no other column: the field, its labels, the known grid, the clusters
  rs::State t;
  std::memset(&t, 0, sizeof(t));
  set_map(t, kOk);
  t.field_call_began(); t.field_build_began(); t.field_built(100);
  t.label_build_began(); t.labels_built(4);
  t.generation_left(3);
  set_known(t, kOk);
  set_evidence(t, kOk);
  CHECK(t.has_evidence() && t.has_known() && t.has_map() && !t.field_refusal(4, 0) && t.labels_serve() && t.clusters_resident() == 3);
  set_evidence(t, kDeviceError);
  CHECK(!t.has_evidence() && t.has_known() && t.has_map() && !t.field_refusal(4, 0) && t.labels_serve() && t.clusters_resident() == 3);
  evidence_scan(t, kOk, true, false);                                                 // an evidence scan that changes no cell keeps the field
  CHECK(t.has_evidence() && t.has_known() && !t.field_refusal(4, 0) && t.labels_serve());
  evidence_scan(t, kOk, true, true);                                                  // one that does makes it stale, as the plain one
  CHECK(t.has_evidence() && t.has_known() && t.field_refusal(4, 0) && !t.labels_serve() && t.clusters_resident() == 3);
  return 0;
}

int random_sequences() {
  std::mt19937 gen(23);
  for (int run = 0; run < 300; run++) {
    rs::State s;
    std::memset(&s, 0, sizeof(s));
    bool evid = false, known = false, map = false, scan = false;  // the restatement: four bits
    for (int step = 0; step < 80; step++) {
      const int ev = (int)(gen() % 7);
      const Outcome o = (Outcome)(gen() % 3);
      const bool track = gen() % 2, changed = gen() % 2;
      if (ev == 0 || ev == 1) {
        if (ev == 0) evidence_scan(s, o, track, changed);
        else plain_scan(s, o, track, changed);
        if (o != kRefused) {
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
        if (o == kOk) map = true;
      } else if (ev == 5) {
        map_from_cloud(s, o);
        if (o == kDeviceError) map = false;
        if (o == kOk) map = true;
      } else {
        const rs::State before = s;  // a question writes nothing
        ask_everything(s);
        CHECK(std::memcmp(&before, &s, sizeof(s)) == 0);
      }
      CHECK(s.has_evidence() == evid && s.has_known() == known && s.has_map() == map && s.has_scan_grid() == scan);
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
