// dilqr_cost_check.h — the pieces of the whole-solve kernel's speculative cost
// route (k_mpc_solve_fixed, dilqr_fused.h) that do not need a
// GPU: the test of one cost record against the guessed diag(q), p, and the
// schedule that spreads those tests over the steps of the first iterations.
// Plain C++ on the host (tests/host/cost_check_host.cpp compiles this header
// alone), __device__ code in the library.
#pragma once
#ifdef __HIPCC__
#include "dilqr_device.h"
#define DILQR_HD __host__ __device__ __forceinline__
#else
#define DILQR_HD inline
#endif

namespace dilqr {

DILQR_HD unsigned f32_bits(float x) { return __builtin_bit_cast(unsigned, x); }

// Zero iff the caller's record (C_t, c_t) is diag(dg), cc bit for bit: every
// off-diagonal word +0.0, the diagonal and c words those of dg, cc.  For a
// record 0 that passes it against its own diagonal and c, "every record passes
// it" is exactly cost flags kCostSym | kCostDiag | kCostTinv (pack_cost /
// same_bits over all t).  One xor/or reduction, compared once by the caller.
template <int d>
DILQR_HD unsigned cost_record_diff(const float (&C)[d][d], const float (&c)[d], const float (&dg)[d],
                                   const float (&cc)[d]) {
  unsigned x = 0u;
#pragma unroll
  for (int i = 0; i < d; ++i) {
#pragma unroll
    for (int j = 0; j < d; ++j) x |= i == j ? f32_bits(C[i][i]) ^ f32_bits(dg[i]) : f32_bits(C[i][j]);
    x |= f32_bits(c[i]) ^ f32_bits(cc[i]);
  }
  return x;
}

// Which step of the solve reads which record.  Records 0 and T-1 are tested
// before the solve starts (the guard); records 1 .. T-2 are read one at a time
// into a one-record buffer, each tested ("folded") when the next one is
// issued.  That is R + 1 events for R = T - 2 records — the first only loads,
// the last only folds — spread evenly (a Bresenham accumulator: no division
// in the step) over the ticks of the first min(spread, iters) iterations, one
// tick per sweep step.  The waves of a launch run in
// step, so without more ado all of them would issue a record at the same tick
// and HBM would see the whole batch's record as one burst (each wave then
// waits for the burst, not for its own 10 KB); the first event of wave w
// therefore falls on tick stagger(w, gap) of the gap between two events, and
// at any tick only 1/gap of the waves load.  spread = 0, or a solve with fewer
// ticks than planned, leaves the rest to drain(): take_fold() / take_load()
// hand out every record exactly once, in order, however the ticks fall.
// Every field is wave-uniform.
struct SpecSchedule {
  int last;      // the last record to test, T - 2 (none when T < 3)
  int loaded;    // records issued so far: 1 .. loaded
  int folded;    // records tested so far: 1 .. folded (folded <= loaded <= folded + 1)
  int events;    // R + 1, or 0 when nothing is spread
  int fired;
  int ticks;     // the ticks the events are spread over
  int acc;
  // the tick, 0 .. gap-1, of wave w's first event (a multiplicative hash: the
  // waves of one XCD or CU, which are strided in w, get every offset)
  static DILQR_HD int stagger(unsigned wave, int gap) {
    return (int)(((wave * 2654435761u) >> 16) % (unsigned)gap);
  }
  DILQR_HD void init(int T, int iters, int spread, int ticks_per_iteration, unsigned wave) {
    last = T - 2;
    loaded = 0;
    folded = 0;
    const int its = spread < iters ? spread : iters;
    ticks = its > 0 ? its * ticks_per_iteration : 0;
    events = (T > 2 && ticks >= T - 1) ? T - 1 : 0;
    fired = 0;
    acc = ticks - events;
    if (events > 0) acc -= stagger(wave, ticks / events) * events;   // (>= 0: the offset is < ticks / events)
  }
  // one call per step; true when an event falls on it
  DILQR_HD bool tick() {
    if (fired == events) return false;
    acc += events;
    if (acc < ticks) return false;
    acc -= ticks;
    ++fired;
    return true;
  }
  // the buffered record is to be tested now (and leaves the buffer)
  DILQR_HD bool take_fold() {
    if (folded == loaded) return false;
    ++folded;
    return true;
  }
  // the record to issue now, or 0 when every record has been issued
  DILQR_HD int take_load() {
    if (loaded >= last) return 0;
    return ++loaded;
  }
  DILQR_HD bool done() const { return folded >= last; }
};

}  // namespace dilqr
