// What is resident on a cluster handle, and whether it still describes the map.  Host code only, no HIP: the
// ONE owner of every validity fact of direct_cluster_handle_s.  The handle keeps the device pointers, blocks and workspaces; this
// struct keeps what is true of them.  direct_cluster.hip reaches the members only through the functions below: an entry point
// says what HAPPENED (an event), asks what it needs to know (a question), and assigns nothing.
// tests/cpp/test_resident_state.cpp replays every row of the design's table and random event sequences on the CPU.
//
// Two properties the C boundary depends on:
//   - All-zero bytes mean "nothing resident": every question answers from a zeroed object (no map, no valid field, no valid
//     labels, no scan grid, no known grid, no evidence grid, no open map, 0 clusters), and no question writes.  The ABI tests hand the library a zeroed buffer
//     as a handle and assert that a refused call wrote not one byte of it.
//   - No pointers, trivially copyable, a few dozen bytes.
//
// The field has TWO counters, and they are not one:
//   - the serial counts SUCCESSFUL builds.  It keys the floor tables: a table matches only the field it was built from, and a
//     refused or failed distance_field leaves the field, hence the tables, as they were (info[0] of the next clear corridor
//     call stays 0).
//   - the generation counts EVERY distance_field call past its null check, refused ones included.  It keys labels built with a
//     floor: after any such call they no longer count as describing the field (the labels' refusal says so), which a caller can
//     rely on without knowing whether the call got as far as the device.
// Merging them would change one of the two answers after a refused distance_field.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "cube_corridor_clear_math.h"
#include "free_comp_math.h"

namespace direct {
namespace resident {

enum class ScanEnd { unchanged, changed, failed };

struct State {
  // ---- the map and its summed-area table --------------------------------------------------------------------------------
  // set_map, map_from_cloud, past their null check and before their refusals: the field and the labels are stale at once,
  // whatever becomes of the call
  void map_edit_began() {
    field_valid_ = 0;
    have_open_ = 0;  // the caller's bytes, or a scan's new map: an open map no longer stands beside them (see below)
    map_gen_++;
  }
  void map_lost() { have_map_ = 0; }   // a device error behind a write to the map: nothing describes its bytes
  void map_ready() { have_map_ = 1; }  // the map and its table have drained
  bool has_map() const { return have_map_ != 0; }

  // ---- the scan grid -----------------------------------------------------------------------------------------------------
  // map_integrate_scan touches the grids: not present until the call has ended well - and neither is an open map
  void scan_began() { have_scan_ = have_open_ = 0; }
  // unchanged: set + cleared == 0 on a handle that had a map - the table, the field, the floor tables and the labels stay
  void scan_ended(ScanEnd how) {
    if (how != ScanEnd::unchanged) map_edit_began();
    have_map_ = have_scan_ = how != ScanEnd::failed;
  }
  bool has_scan_grid() const { return have_scan_ != 0; }

  // ---- the known grid (what the tracked scans have observed; it describes observation, not occupancy: no map event touches it)
  void known_scan_began() { have_known_ = 0; }      // a tracked scan writes it: not present until the call has ended well
  void known_ended(bool ok) { have_known_ = ok; }   // ... which a device error does not
  void known_set() { have_known_ = 1; }             // set_known has drained: the caller's bytes, or all zero
  void known_dropped() { have_known_ = 0; }         // an untracked scan past its refusals (its rays were not recorded), a failed set_known
  bool has_known() const { return have_known_ != 0; }

  // ---- the evidence grid (what the evidence scans have counted per voxel; like the known grid it describes observation: no
  // map event touches it, and neither frontier nor view_gain_batch does)
  void evidence_scan_began() { have_evid_ = 0; }     // an evidence scan folds into it: not present until the call has ended well
  void evidence_ended(bool ok) { have_evid_ = ok; }  // ... which a device error does not
  void evidence_set() { have_evid_ = 1; }            // set_evidence has drained: the caller's bytes, or all zero
  // a PLAIN scan past its refusals (it writes the scan grid behind the evidence's back), a failed set_evidence
  void evidence_dropped() { have_evid_ = 0; }
  bool has_evidence() const { return have_evid_ != 0; }

  // ---- the open map (the unknown policy DIRECT_UNKNOWN_OCCUPIED: the map as a scan derives it BEFORE unobserved space is closed;
  // view_gain_batch and DIRECT_SCAN_ADOPT read it where it is held).  It stands beside the map of the scan that wrote both: any
  // scan past its refusals loses it, and so do set_map and map_from_cloud past their null check (map_edit_began); a successful
  // scan under the policy makes it ready again, a scan under DIRECT_UNKNOWN_FREE or a device error leaves it lost.
  void open_map_ready() { have_open_ = 1; }  // behind scan_ended of a successful scan under the policy
  bool has_open_map() const { return have_open_ != 0; }

  // ---- the distance field ------------------------------------------------------------------------------------------------
  void field_call_began() { field_gen_++; }    // every distance_field past its null check: labels built with a floor are stale
  void field_build_began() { field_valid_ = 0; }  // past its refusals and allocation: the device is about to write the field
  void field_built(int32_t cap2) {
    field_valid_ = 1;
    field_cap2_ = cap2;
    field_serial_++;  // every floor table misses
  }
  // What a call that reads the field with floor min_d2 and an n_penalty-entry table is refused with, or null.  A stored cap2
  // means "at least cap2": neither the floor nor the table may tell values at or above it apart (an uncapped field has
  // cap2 = DIRECT_DIST_NONE, which refuses nothing).  (0, 0) asks for a valid field alone.
  const char* field_refusal(int32_t min_d2, int32_t n_penalty) const {
    if (!field_valid_) return "no valid distance field: call direct_cluster_distance_field after the map changes";
    if (min_d2 > field_cap2_ || n_penalty > field_cap2_) return "min_d2 or n_penalty above the cap2 the distance field was built with";
    return nullptr;
  }

  // ---- the floor tables of the clear corridors: cubecor::kFloorSlots slots, least recently used replaced ------------------
  // The slot a clear-mode call uses.  *hit = 0: the slot is the victim of a build and holds nothing until floor_built.
  int floor_chosen(int32_t min_d2, int* hit) {
    const int slot = cubecor::floor_slot_choose(floor_slot_, cubecor::kFloorSlots, min_d2, field_serial_, hit);
    if (!*hit) floor_slot_[slot].valid = 0;
    return slot;
  }
  void floor_build_failed(int slot) { floor_slot_[slot].valid = 0; }
  void floor_built(int slot, int32_t min_d2, long long count) {  // its build has drained without an error
    cubecor::FloorSlot& s = floor_slot_[slot];
    s.min_d2 = min_d2; s.serial = field_serial_; s.count = count; s.valid = 1;
  }
  void floor_used(int slot) { floor_slot_[slot].used = ++floor_clock_; }  // every clear-mode success, hit or built
  long long floor_count(int slot) const { return floor_slot_[slot].count; }

  // ---- the free-space labels ---------------------------------------------------------------------------------------------
  void label_build_began() { label_key_.valid = 0; }
  void labels_built(int32_t floor) { label_key_ = freecomp::Key{map_gen_, field_gen_, floor, 1}; }  // floor in normal form
  bool labels_serve() const { return freecomp::key_serves(label_key_, map_gen_, field_gen_); }
  int32_t labels_floor() const { return label_key_.floor; }

  // ---- the resident clusters ---------------------------------------------------------------------------------------------
  void clusters_overwritten() { clusters_ = 0; }
  void generation_left(int n) { clusters_ = n; }  // seeds of a polygon_generation_batch whose clusters are still in the storage
  int clusters_resident() const { return clusters_; }

 private:
  int32_t have_map_, have_scan_;
  int32_t field_valid_, field_cap2_;
  unsigned long long field_serial_;      // successful field builds
  unsigned long long map_gen_, field_gen_;  // map edits / distance_field calls, refused ones included
  unsigned long long floor_clock_;       // ticks at every use of a slot: least recently used is the smallest FloorSlot::used
  cubecor::FloorSlot floor_slot_[cubecor::kFloorSlots];
  freecomp::Key label_key_;              // what the labels were built from (valid == 0: none)
  int32_t clusters_;
  int32_t have_known_;
  int32_t have_evid_;
  int32_t have_open_;
};
static_assert(std::is_trivially_copyable<State>::value && std::is_standard_layout<State>::value, "plain data: zero bytes are a State");
static_assert(sizeof(State) <= 256, "a handle is far smaller than the 64 KiB the ABI tests hand over");

}  // namespace resident
}  // namespace direct
