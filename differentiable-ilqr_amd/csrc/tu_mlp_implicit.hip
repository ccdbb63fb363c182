// tu_mlp_implicit.hip — the DiLQR implicit backward with the one-hidden-layer
// network as the dynamics (dilqr_mlp.h): the exact derivative of the iLQR fixed
// point, curvature of the dynamics included, by the algebra of
// oracle/adjoint.py implicit_backward_fast.
//
// At a solution tau = (x, u), with lam_t the primal costates
// (lqr_step_explicit.py:305-319), the active set I = {|u - bound| <= 1e-8}
// held fixed, F_t = d f / d tau (tau_t) and g = [dl_dx; dl_du]:
//   M_t   = sum_i lam_{t+1,i} d^2 f_i / d tau^2 (tau_t) = W1^T diag(h) W1,
//           h_j = (W2^T lam_{t+1})_j act''(z_j); M_{T-1} = 0; relu: M = 0
//   y     = the LQR solution with cost matrices C_t + M_t, linear term -g_t,
//           dynamics F_t from x_0 = 0, active controls zeroed
//   w_t   = g_t - M_t y_t
//   dlam_t = C_xx y_x + C_xu y_u - w_x + F_x,t^T dlam_{t+1}
//   dC_t = -1/2 (y tau^T + tau y^T)      dc_t = -y_t       dx_init = -dlam_0
//   dF_t = -(dlam_{t+1} tau_t^T + lam_{t+1} y_t^T)         df_t = -dlam_{t+1}
// The gradient into the weights is dilqr_mlp_linearize_vjp_f32 on (dF, df).
// No env_dx quirks (reversed gains, closed-loop gradx) belong here, and the
// gains of the no-op step are not needed.
//
// One problem per lane, three passes over T as k_implicit_backward
// (tu_implicit.hip):
//   B (t down): lam, F_t and M_t from one walk over the hidden units; Riccati
//               step with C_t + M_t, c_back = -g_t, active set masked; the
//               gains -> ws
//   C (t up)  : y (F_t from a Jacobian walk) -> ws
//   D (t down): lam again by the same costate_step, F_t and M_t y_t from one
//               walk (M is not formed: W1^T (h o (W1 y))); w, dlam; dC, dc,
//               dF, df stored as coalesced wave records; dx_init at t = 0
// so three walks per (t, b) for sigmoid; for relu they are Jacobian walks.
#include "dilqr_mlp.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_mlp_implicit.h"

using namespace dilqr;

extern "C" {

int dilqr_mlp_implicit_ws_floats(int n, int m) {
#define X(N_, M_) if (n == N_ && m == M_) return MlpImplicitWs<N_, M_>::REC;
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return -1;
}

int dilqr_mlp_implicit_backward_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* C, const float* c,
                                    const float* x, const float* u, const float* dl_dx, const float* dl_du,
                                    dilqr_bounds bounds, float* ws, float* dx_init, float* dC, float* dc, float* dF,
                                    float* df, void* stream) {
  if (T < 1 || B < 0) return DILQR_E_ARG;
  if (!C || !c || !x || !u || !dl_dx || !dl_du || !ws || !dx_init || !dC || !dc) return DILQR_E_ARG;
  if ((dF == nullptr) != (df == nullptr)) return DILQR_E_ARG;
  const void* ps[] = {C, c, x, u, dl_dx, dl_du, ws, dx_init, dC, dc, dF, df};
  for (const void* q : ps) if (!al16(q)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = OneHidden::check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const MlpArg a = OneHidden::arg(mlp);
  const Bounds bd = mkb(bounds);
  const size_t lds = OneHidden::lds_bytes(n, m, a);
  return mlp_dispatch<OneHidden>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_mlp_implicit_backward<MD><<<grid_for(B), kBlock, lds, S(stream)>>>(T, B, a, C, c, x, u, dl_dx, dl_du, bd, ws,
                                                                        dx_init, dC, dc, dF, df);
  });
}

}  // extern "C"
