"""TEST INFRASTRUCTURE of tests/test_unknown_policy_restatement.py, tests/test_gpu_unknown_policy.py and
tools/unknown_policy_bench.py: what one scan under DIRECT_UNKNOWN_OCCUPIED (include/direct_cluster.h, "unknown space as occupied")
must leave, twice over.
  restate_plain / restate_evidence
               written from the definition's TEXT on top of map_scan_harness.restate / dilate, frontier_harness.known_restate and
               evidence_harness.restate, which are imported and not edited: open = dilate(raw, inflate), map = open | (known == 0),
               the stats counted on the map, and the two policy counts.
  build / run  a g++ program with its own main around direct_amd/csrc/map_close_math.h that emulates k_scan_close as lane loops on
               one thread - groups of 16 voxels packed into four 32-bit words as the kernel packs them, the last group byte by
               byte, a group stored only where it changed - on heap buffers of exactly G bytes.
               build(..., sanitize=True) is the same program under -fsanitize=address,undefined, run stand-alone.
  refusal / policy_known
               what mapclose::scan_refusal and mapclose::policy_known (the functions the library calls) answer, through the same
               program.
There is no reference counterpart."""
import os
import subprocess

import numpy as np

from tests import evidence_harness as eh
from tests import frontier_harness as fh
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests.cpp_program import compile_program

FREE, OCCUPIED = 0, 1
COUNTS = ("raw_ones", "map_ones", "set", "cleared", "closed", "open_ones")


def close(open_map, known, raw, before):
    """The byte rule and the six counts, from the definition: -> (map, int64 [6] in the order of COUNTS)"""
    o = (np.asarray(open_map) != 0)
    new = (o | (np.asarray(known) == 0)).astype(np.uint8)
    old = np.zeros(new.shape, np.uint8) if before is None else np.asarray(before, np.uint8)
    counts = [int((np.asarray(raw) == 1).sum()), int(new.sum()), int(((old != new) & (new == 1)).sum()), int(((old != new) & (new == 0)).sum()),
              int(((new == 1) & ~o).sum()), int(o.sum())]
    return new, np.array(counts, np.int64)


def restate_plain(points, origin, max_range, inflate=(0, 0, 0), mode="continue", raw=None, before=None, known=None, open_before=None,
                  touched=None, dims=sh.DIMS, res=sh.RES, lower=sh.LOWER, upper=sh.UPPER):
    """One tracked plain scan under the policy.  raw: the scan grid the handle holds (None: none); before: its map (None: none, all
    0); known: its known grid (None: none); open_before: the open map it holds (None: none) - what ADOPT adopts in place of the map.
    touched: evidence_harness.touch_grid's result for these points, where a test shares the walks between cases (the carve clears
    what it passes, then the mark sets the returns; tests/test_unknown_policy_restatement.py holds the two ways equal).
    -> dict(raw, open, map, known, stats int64 [8], closed, open_ones)"""
    kw = dict(dims=dims, res=res, lower=lower, upper=upper)
    if mode == "reset":
        start, kn0 = None, None
    elif mode == "continue":
        start, kn0 = raw, known
    else:
        assert before is not None
        start, kn0 = (before if open_before is None else open_before), known
    if touched is None:
        grid, _, s = sh.restate(points, origin, max_range, (0, 0, 0), raw=start, before=None, **kw)
        kn = fh.known_restate(points, origin, max_range, kn0, **kw)
    else:
        touch, skipped, truncated, outside = touched
        grid = np.zeros(dims, np.uint8) if start is None else np.array(start, np.uint8)
        grid[touch == 1] = 0
        grid[touch == 2] = 1
        kn = (np.zeros(dims, np.uint8) if kn0 is None else (np.asarray(kn0) != 0).astype(np.uint8)) | (touch != 0).astype(np.uint8)
        s = [len(mh._rows(points)), skipped, truncated, outside]
    opened = sh.dilate(grid, inflate)
    new, c = close(opened, kn, grid, before)
    stats = np.array(list(s[:4]) + list(c[:4]), np.int64)
    return dict(raw=grid, open=opened, map=new, known=kn, stats=stats, closed=int(c[4]), open_ones=int(c[5]))


def restate_evidence(points, origin, max_range, par=eh.DEFAULTS, inflate=(0, 0, 0), mode="continue", ev=None, before=None, known=None,
                     open_before=None, touched=None, dims=sh.DIMS, res=sh.RES, lower=sh.LOWER, upper=sh.UPPER):
    """One tracked evidence scan under the policy; arguments as restate_plain and evidence_harness.restate.
    -> dict(ev, raw, open, map, known, stats int64 [12], closed, open_ones)"""
    src = before if open_before is None or mode != "adopt" else open_before       # the fold's map operand
    w = eh.restate(points, origin, max_range, par, inflate, mode, ev, src, known, True, dims, res, lower, upper, touched)
    new, c = close(w["map"], w["known"], w["raw"], before)
    stats = np.array(list(w["stats"][:4]) + list(c[:4]) + list(w["stats"][8:]), np.int64)
    return dict(ev=w["ev"], raw=w["raw"], open=w["map"], map=new, known=w["known"], stats=stats, closed=int(c[4]), open_ones=int(c[5]))


HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "map_close_math.h"
namespace mcl = direct::mapclose;
// --refusal policy flags: prints mcl::scan_refusal's message, or "ok";  --policy v: prints 1 or 0, mcl::policy_known
// in: int64 G, lanes; uint8 open[G], known[G], raw[G], before[G]      out: int64 counts[6]; uint8 map[G]
struct W16 { uint32_t w[4]; };
static W16 load(const uint8_t* p, int n) {  // n == 16: the 128-bit load; the tail: n bytes and not one more
  W16 r = {{0u, 0u, 0u, 0u}};
  if (n == mcl::kGroup) memcpy(r.w, p, 16);
  else
    for (int k = 0; k < n; k++) r.w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  return r;
}
static void store(uint8_t* p, int n, const W16& v) {
  if (n == mcl::kGroup) memcpy(p, v.w, 16);
  else
    for (int k = 0; k < n; k++) p[k] = (uint8_t)(v.w[k >> 2] >> (8 * (k & 3)));
}
int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--refusal")) {
    const char* why = mcl::scan_refusal(atoi(argv[2]), atoi(argv[3]));
    printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "--policy")) {
    printf("%d\n", (int)mcl::policy_known(atoi(argv[2])));
    return 0;
  }
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  long long hdr[2];
  if (!f || fread(hdr, 8, 2, f) != 2) return 1;
  const long long G = hdr[0], lanes = hdr[1];
  // exactly G bytes each, on the heap: a read or a write past the tail is the sanitizer's finding
  std::unique_ptr<uint8_t[]> open(new uint8_t[G]), known(new uint8_t[G]), raw(new uint8_t[G]), map(new uint8_t[G]);
  if (fread(open.get(), 1, G, f) != (size_t)G || fread(known.get(), 1, G, f) != (size_t)G || fread(raw.get(), 1, G, f) != (size_t)G ||
      fread(map.get(), 1, G, f) != (size_t)G)
    return 1;
  fclose(f);
  long long cnt[6] = {0, 0, 0, 0, 0, 0};
  long long stores = 0;
  const long long groups = mcl::groups(G);
  for (long long lane = 0; lane < lanes; lane++)          // k_scan_close: a lane owns the groups lane, lane + lanes, ...
    for (long long g = lane; g < groups; g += lanes) {
      const long long at = mcl::group_at(g);
      const int n = mcl::group_size(G, g);
      if (n < 1 || n > mcl::kGroup || at + n > G) return 4;
      const W16 o = load(open.get() + at, n), kn = load(known.get() + at, n), r = load(raw.get() + at, n), m0 = load(map.get() + at, n);
      W16 m1 = {{0u, 0u, 0u, 0u}};
      for (int k = 0; k < mcl::kGroup; k++) {
        const int w = k >> 2, sh = 8 * (k & 3);
        const uint8_t ob = (uint8_t)(o.w[w] >> sh), kb = (uint8_t)(kn.w[w] >> sh), rb = (uint8_t)(r.w[w] >> sh), before = (uint8_t)(m0.w[w] >> sh);
        const bool live = k < n;
        const uint8_t now = live ? mcl::close_byte(ob, kb) : (uint8_t)0;
        m1.w[w] |= (uint32_t)now << sh;
        cnt[0] += live && rb == 1;
        cnt[1] += now;
        cnt[2] += live && before != now && now == 1;
        cnt[3] += live && before != now && now == 0;
        cnt[4] += live && mcl::closed(ob, now);
        cnt[5] += live && ob == 1;
      }
      if (memcmp(m0.w, m1.w, 16)) { store(map.get() + at, n, m1); stores++; }
    }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  fwrite(cnt, 8, 6, o);
  fwrite(&stores, 8, 1, o);
  fwrite(map.get(), 1, G, o);
  fclose(o);
  return 0;
}
'''


def build(workdir, sanitize=False):
    name = "unknown_policy_harness_san" if sanitize else "unknown_policy_harness"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return str(workdir), compile_program(workdir, name, HARNESS, extra)


def refusal(harness, policy, flags):
    """-> the message a scan with these flags is refused with under this policy, or 'ok'"""
    return subprocess.check_output([harness[1], "--refusal", str(int(policy)), str(int(flags))], text=True).strip()


def policy_known(harness, value):
    return subprocess.check_output([harness[1], "--policy", str(int(value))], text=True).strip() == "1"


def run(harness, open_map, known, raw, before, lanes=64):
    """-> (map, int64 [6] in the order of COUNTS, groups stored) of the header program's close pass"""
    d, exe = harness
    shape = np.asarray(open_map).shape
    G = int(np.prod(shape))
    tag = os.path.basename(exe)
    fin, fout = os.path.join(d, tag + "_in.bin"), os.path.join(d, tag + "_out.bin")
    with open(fin, "wb") as f:
        np.array([G, int(lanes)], np.int64).tofile(f)
        for g in (open_map, known, raw, before):
            (np.zeros(G, np.uint8) if g is None else np.ascontiguousarray(g, np.uint8)).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        counts = np.fromfile(f, np.int64, 6)
        stores = int(np.fromfile(f, np.int64, 1)[0])
        new = np.fromfile(f, np.uint8, G).reshape(shape)
        assert f.read() == b""
    os.remove(fout)
    return new, counts, stores


def same_close(harness, want, before, lanes=64):
    """the header program's close pass on a restatement's open map, known grid and scan grid equals the restatement's map and counts"""
    new, counts, _ = run(harness, want["open"], want["known"], want["raw"], before, lanes)
    assert np.array_equal(new, want["map"]), int((new != want["map"]).sum())
    assert counts.tolist() == list(want["stats"][4:8]) + [want["closed"], want["open_ones"]], (counts, want["stats"])


# ---- the scene of "the reason for the feature", shared by the CPU and the GPU tests -------------------------------------------

def dijkstra(path_harness, grid, starts, goals):
    """the heap Dijkstra ("full") of tests/grid_path_harness.py's program on `grid` -> dict(rtn, path_cost, paths, ...)"""
    from tests import grid_path_harness as gh
    return gh.run(path_harness, grid, np.array(starts, np.int32), np.array(goals, np.int32), sides=("full",), fields=False)["full"]


def l_scene(dims=sh.DIMS):
    """-> dict(known, start, goal, island_goal): an L of two perpendicular arms, 3 voxels thick, along x = 4..6 (y = 4..31) and
    y = 29..31 (x = 4..35) at z = 4..6, whose far ends a straight path joins through unobserved space; and a second known island
    that only unobserved space connects to the L"""
    known = np.zeros(dims, np.uint8)
    known[4:7, 4:32, 4:7] = 1
    known[4:36, 29:32, 4:7] = 1
    known[30:36, 4:10, 4:7] = 1      # the island
    return dict(known=known, start=(5, 5, 5), goal=(34, 30, 5), island_goal=(33, 6, 5))
