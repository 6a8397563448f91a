// Ticket arithmetic of the dynamically scheduled hot kernel (k_iterate_dyn, direct_ddp.hip), in plain C++ so that the
// kernel, its host wrapper and a CPU test (tests/cpp/test_sched_ticket.cpp) share one definition.
//
// A launch of n iterations over nb trajectories hands out tickets 0, 1, 2, ... from one counter.  Ticket t is UNIT
// t / nb of trajectory slot t % nb.  Units of a trajectory run strictly in order: unit u waits until u units of that
// trajectory have been published (done_epoch[b] >= u).
//   whole tickets: a unit is `chunk` trips of the outer loop (the last one may be shorter); units = ceil(n / chunk)
//   half tickets:  a unit is HALF a trip; unit u is iteration u / 2, half u % 2 (0: the backward sweep with its
//                  regulariser retries, 1: the line search and the exit rules); units = 2 n; chunk is 1
// Behind the last unit come `tail` rounds of HELP-ONLY tickets (launches with helpers): their holders wait for the
// trajectory's last unit like any waiter, and so join what its owner has open, but never run a unit.
#pragma once

#if defined(__HIPCC__)
#define SCHED_FN __host__ __device__ inline
#else
#define SCHED_FN inline
#endif

namespace direct {
namespace sched {

constexpr int kPartWhole = 0;     // a whole trip of the outer loop
constexpr int kPartBackward = 1;  // the backward sweep and its retries
constexpr int kPartSearch = 2;    // the line search and the exit rules

struct TicketPlan {
  unsigned nb;          // trajectories of the launch
  unsigned units;       // units per trajectory
  unsigned total;       // tickets that run a unit: nb * units
  unsigned total_help;  // total + the help-only tickets
  int n_iters, chunk, half;
};

// tail: rounds of help-only tickets (0 for a launch without helpers)
SCHED_FN TicketPlan ticket_plan(int nb, int n_iters, int chunk, int half, int tail) {
  TicketPlan P;
  P.nb = (unsigned)nb;
  P.n_iters = n_iters;
  P.half = half ? 1 : 0;
  P.chunk = (P.half || chunk < 1) ? 1 : chunk;
  P.units = P.half ? 2u * (unsigned)n_iters : (unsigned)((n_iters + P.chunk - 1) / P.chunk);
  P.total = P.nb * P.units;
  P.total_help = P.total + P.nb * (unsigned)tail;
  return P;
}

struct Ticket {
  int unit;       // t / nb (help-only tickets: >= units)
  int slot;       // t % nb: the trajectory's position in the launch
  int waits_for;  // published units of the trajectory this ticket waits for
  int runs;       // 0: help-only, never runs a unit
};

// t < P.total_help
SCHED_FN Ticket ticket_decode(const TicketPlan& P, unsigned t) {
  Ticket k;
  k.unit = (int)(t / P.nb);
  k.slot = (int)(t - (unsigned)k.unit * P.nb);
  k.waits_for = k.unit < (int)P.units ? k.unit : (int)P.units;  // the tail follows the last unit
  k.runs = t < P.total ? 1 : 0;
  return k;
}

struct Work {
  int iter0;  // first iteration of the unit, counted from the start of the launch
  int n;      // trips of the outer loop the unit covers (half tickets: the one trip it is half of)
  int part;   // kPart...
};

// unit < P.units
SCHED_FN Work unit_work(const TicketPlan& P, int unit) {
  Work w;
  if (P.half) {
    w.iter0 = unit >> 1;
    w.n = 1;
    w.part = (unit & 1) ? kPartSearch : kPartBackward;
  } else {
    w.iter0 = unit * P.chunk;
    const int left = P.n_iters - w.iter0;
    w.n = left < P.chunk ? left : P.chunk;
    w.part = kPartWhole;
  }
  return w;
}

// what done_epoch[b] holds once `unit` has been published (without the finished bit)
SCHED_FN int published_after(int unit) { return unit + 1; }

}  // namespace sched
}  // namespace direct
