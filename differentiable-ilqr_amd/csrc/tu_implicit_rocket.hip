// tu_implicit_rocket.hip — the DiLQR implicit backward for rocket
// (16 lanes per problem, dilqr_implicit_group.h; rocket.py:263-323, 541-820).
#include "dilqr_common.h"
#include "dilqr_implicit_group.h"
#include "dilqr_launch.h"

namespace dilqr {

int implicit_rocket_ws_floats() { return ImplicitGroupWs<Rocket>::REC; }

int launch_implicit_rocket(const ImplicitArgs& a) {
#define IMPL_LAUNCH(MODE_)                                                                         \
  k_implicit_backward_group<Rocket, gen::RocketD2, MODE_><<<grid_group(a.B), 64, 0, a.stream>>>(  \
      a.T, a.B, a.theta, a.C, a.c, a.x, a.u, a.K, a.dl_dx, a.dl_du, a.bd, a.ws, a.dC, a.dc, a.dtheta)
  if (a.bd.mode == DILQR_BOUNDS_NONE) IMPL_LAUNCH(GAIN_UNC);
  else IMPL_LAUNCH(GAIN_ZERO_I);
#undef IMPL_LAUNCH
  return launched();
}

}  // namespace dilqr
