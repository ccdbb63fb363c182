// dilqr_stop_rule.h — the MPC loop's stop rule (mpc_explicit.py:264, 279,
// 297-299) and best-iterate test, plain C++ on the host
// (tests/host/stop_rule_host.cpp compiles this header alone), and the
// quirk-row norm (__device__).  The per-iteration launches split the rule so
// that no launch waits on a grid-wide fan-in:
//  * k_mpc_norm_rows (after iteration k): full_du_norm with the reference's
//    batch-mixing rows (the .transpose(1,2).contiguous().view(n_batch,-1) quirk,
//    lqr_step_explicit.py:245-247), best_du of the problems that took iteration
//    k, and per-workgroup partials (max row norm, any "improved") into plane
//    k&1 of the sync area.  Plain stores only.
//  * mpc_decide, in the prologue of iteration k+1 (every workgroup, redundantly,
//    identically): reduce the partials of iteration k, apply the stop rule to the
//    control state S_k -> S_{k+1}; workgroup 0 publishes S_{k+1} in ctrl[(k+1)&1].
//    The kernel boundary orders everything, so no fences or atomics are needed
//    (measured: the former last-workgroup fan-in cost 8 of 14 us per iteration).
// Sync area (uints): [16 + (2*par + 0)*G_MAX + blk] max bits, [16 + (2*par+1)*G_MAX
// + blk] any, G_MAX = ceil(B/64).
#pragma once
#include "dilqr_cost_check.h"
#ifdef __HIPCC__
#include "dilqr_device.h"
#endif

namespace dilqr {

// best-iterate test (mpc_explicit.py:277-283): iteration 0 always takes it
DILQR_HD bool mpc_takes_best(bool first, float cost, float best_cost, float best_cost_eps) {
  return first || cost <= best_cost + best_cost_eps;
}

struct StopState { int n_not_improved, stopped; };

// `max < eps` on the bits of a row norm (>= 0: uint order is float order; a NaN fails it).
// The max is below eps iff every term of it is: mpc_decide ballots its lanes' partial maxima.
DILQR_HD bool du_below(unsigned max_bits, float eps) { return __builtin_bit_cast(float, max_bits) < eps; }

// One application of the rule, after an iteration that is not the solve's last:
// count the iterations without an improvement, stop below eps or past lim.
// any: some problem took the best-iterate branch in an iteration after the first.
DILQR_HD StopState stop_rule_step(int n_not_improved, bool any, bool below, int lim) {
  StopState s;
  s.n_not_improved = any ? 0 : n_not_improved + 1;          // mpc_explicit.py:264, 279
  s.stopped = (below || s.n_not_improved > lim) ? 1 : 0;    // 297-299
  return s;
}

#ifdef __HIPCC__
DEV int sync_gmax(int B) { return (B + 63) / 64; }

// The 2-norm of a quirk row of TM squared entries, summed in index order (the
// order fixes the bits)
DEV float quirk_row_norm(const float* p, int TM) {
  float s = 0.f;
  for (int i = 0; i < TM; ++i) s += p[i];
  return sqrtf(s);
}
#endif

}  // namespace dilqr
