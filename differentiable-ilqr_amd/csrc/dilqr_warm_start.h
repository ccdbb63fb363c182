// dilqr_warm_start.h — which row of a solve's plan feeds row t of the next
// solve's u_init in a closed loop (dilqr_mpc_advance_f32, tu_advance.hip): the
// reference's rule with its quirk (il_env.py:139-140), the plain shift, the
// cold start.  Plain C++ on the host (tests/host/advance_host.cpp compiles this
// header alone), __device__ code in the library.
#pragma once
#include "../../include/dilqr.h"
#include "dilqr_cost_check.h"   // DILQR_HD

namespace dilqr {

constexpr int kWarmZero = -1;   // warm_source: the row is zero

// a mode the entry point takes at this horizon.  The reference writes
// u_init[-2] = u_init[-3], which indexes out of range below T = 3.
DILQR_HD bool warm_mode_ok(int mode, int T) {
  if (T < 1) return false;
  if (mode == DILQR_WARM_REFERENCE) return T >= 3;
  return mode == DILQR_WARM_SHIFT || mode == DILQR_WARM_COLD;
}

// The row of u_plan [T,B,m] that u_warm[t] copies, 0 <= t < T, or kWarmZero.
//  REFERENCE: u_init = cat(u[1:], 0); u_init[-2] = u_init[-3] (il_env.py:139-140):
//             row T-2 repeats row T-3's source, u[T-2]; u[T-1] is never read
//  SHIFT:     u_init = cat(u[1:], 0)
//  COLD:      zeros
DILQR_HD int warm_source(int mode, int T, int t) {
  if (mode == DILQR_WARM_COLD || t >= T - 1) return kWarmZero;
  if (mode == DILQR_WARM_REFERENCE && t == T - 2) return T - 2;
  return t + 1;
}

}  // namespace dilqr
