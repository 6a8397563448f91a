// CPU test of direct_amd/csrc/sched_ticket.h (built by tests/test_sched_ticket_cpp.py, optionally with
// -fsanitize=address,undefined): the ticket arithmetic of the ticket-scheduled hot kernel.  For every launch shape the
// tickets are drawn in counter order, as the kernel's waves draw them, and replayed against a model of done_epoch: each
// (trajectory, iteration, half) exactly once and in order, each ticket waiting for exactly its predecessor, help-only
// tickets never running, whole-trip mode equal to the mapping (t / B, t % B) x chunk.  Prints PASS and returns 0, or says
// which check failed.
#include "../../direct_amd/csrc/sched_ticket.h"

#include <cstdio>
#include <vector>

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

namespace {
using namespace direct::sched;

int launch_case(int B, int n, int tail, int half, int chunk) {
  const TicketPlan P = ticket_plan(B, n, chunk, half, tail);
  const int eff_chunk = half ? 1 : chunk;
  const int units = half ? 2 * n : (n + eff_chunk - 1) / eff_chunk;
  CHECK((int)P.nb == B && (int)P.units == units && P.chunk == eff_chunk && P.half == half);
  CHECK(P.total == (unsigned)(B * units));
  CHECK(P.total_help == P.total + (unsigned)(B * tail));
  std::vector<int> published(B, 0);   // done_epoch without the finished bit
  std::vector<int> next_iter(B, 0);   // trips of the outer loop issued so far
  std::vector<int> next_half(B, 0);   // half tickets: which half comes next
  for (unsigned t = 0; t < P.total_help; t++) {
    const Ticket k = ticket_decode(P, t);
    CHECK(k.slot >= 0 && k.slot < B);
    CHECK((unsigned)k.unit * P.nb + (unsigned)k.slot == t);
    if (t < P.total) {
      CHECK(k.runs == 1 && k.unit < units);
      // the predecessor rule: exactly the units before this one.  Drawn in counter order and with every unit published
      // as soon as it is drawn, that is what the trajectory has published - no ticket waits for a ticket behind it
      CHECK(k.waits_for == k.unit);
      CHECK(published[k.slot] == k.waits_for);
      const Work w = unit_work(P, k.unit);
      if (half) {
        CHECK(w.n == 1);
        CHECK(w.part == (next_half[k.slot] ? kPartSearch : kPartBackward));
        CHECK(w.iter0 == next_iter[k.slot]);
        CHECK(w.iter0 == k.unit / 2 && (w.part == kPartSearch) == (k.unit % 2 == 1));
        if (next_half[k.slot]) next_iter[k.slot]++;
        next_half[k.slot] ^= 1;
      } else {
        // the mapping of the whole-trip scheduler: epoch t / B, trajectory t % B, `chunk` trips, the last epoch shorter
        CHECK(k.unit == (int)(t / (unsigned)B) && k.slot == (int)(t % (unsigned)B));
        const int left = n - k.unit * eff_chunk;
        CHECK(w.part == kPartWhole && w.iter0 == k.unit * eff_chunk && w.n == (left < eff_chunk ? left : eff_chunk));
        CHECK(w.n >= 1 && w.iter0 == next_iter[k.slot]);
        next_iter[k.slot] += w.n;
      }
      published[k.slot] = published_after(k.unit);
      CHECK(published[k.slot] == k.unit + 1);
    } else {
      // help-only: behind the last unit, waits for all of them, never runs (and unit_work is never asked)
      CHECK(k.runs == 0 && k.unit >= units && k.unit < units + tail);
      CHECK(k.waits_for == units);
      CHECK(published[k.slot] == units);
    }
  }
  for (int b = 0; b < B; b++) {
    CHECK(next_iter[b] == n && next_half[b] == 0 && published[b] == units);
  }
  // a helper-less launch has no tail whatever the knob says: the wrapper passes tail = 0
  const TicketPlan Q = ticket_plan(B, n, chunk, half, 0);
  CHECK(Q.total_help == Q.total && Q.total == P.total);
  return 0;
}
}  // namespace

int main() {
  const int Bs[] = {1, 3, 64}, ns[] = {1, 2, 20}, tails[] = {0, 8}, chunks[] = {1, 2, 3};
  for (int B : Bs)
    for (int n : ns)
      for (int tail : tails) {
        for (int chunk : chunks) {
          if (launch_case(B, n, tail, 0, chunk)) return 1;
          if (launch_case(B, n, tail, 1, chunk)) return 1;  // half tickets ignore the chunk
        }
      }
  // a non-positive chunk reads as 1
  CHECK(ticket_plan(3, 5, 0, 0, 0).chunk == 1 && ticket_plan(3, 5, -2, 0, 0).units == 5u);
  std::printf("PASS\n");
  return 0;
}
