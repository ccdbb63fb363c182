// tu_mpc_mlp.hip — C-ABI of the fused MPC path on the one-hidden-layer
// network: one fused iLQR iteration per launch, and a whole stop-rule solve in
// one launch for a small batch.  The kernels are instantiated per (n, m) in
// tu_mpc_mlp_<n><m>.hip (dilqr_mlp_fused.h); this unit checks and dispatches.
#include "dilqr_common.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_mlp_fused.h"

using namespace dilqr;

extern "C" {

int dilqr_mlp_ilqr_iterate_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x_init, const float* C,
                               const float* c, const float* x, const float* u, dilqr_bounds bounds,
                               float linesearch_decay, int max_linesearch_iter, float* ws, float* x_out,
                               float* u_out, float* cost, float* du_sq, float* alpha, const float* old_cost,
                               dilqr_mpc_ctrl* ctrl, void* stream) {
  if (T < 1 || B < 0 || max_linesearch_iter < 1) return DILQR_E_ARG;
  if (!x_init || !C || !c || !x || !u || !ws || !x_out || !u_out || !cost || !du_sq || !alpha) return DILQR_E_ARG;
  const void* ps[] = {x_init, C, c, x, u, ws, x_out, u_out};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = OneHidden::check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const MlpIterArgs a{T, B, OneHidden::arg(mlp), x_init, C, c, x, u, mkb(bounds), linesearch_decay, max_linesearch_iter,
                      ws, x_out, u_out, cost, du_sq, alpha, old_cost, ctrl, S(stream)};
#define X(N_, M_) if (n == N_ && m == M_) return launch_mlp_ilqr_iterate_##N_##_##M_(a, mlp.activation);
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return DILQR_E_SHAPE;
}

int dilqr_mlp_mpc_solve_small_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x_init,
                                  const float* u_init, const float* C, const float* c, dilqr_bounds bounds,
                                  float linesearch_decay, int max_linesearch_iter, int iterations,
                                  float best_cost_eps, float eps, int not_improved_lim, float* xa, float* ua,
                                  float* xb, float* ub, float* ws, float* cost, float* alpha, float* du_sq,
                                  float* full_du_norm, float* best_x, float* best_u, float* best_cost,
                                  float* best_du, dilqr_mpc_ctrl* ctrl, void* stream) {
  if (T < 1 || B < 0 || max_linesearch_iter < 1 || iterations < 1) return DILQR_E_ARG;
  if (!x_init || !C || !c || !xa || !ua || !xb || !ub || !ws || !cost || !alpha || !du_sq || !full_du_norm ||
      !best_x || !best_u || !best_cost || !best_du || !ctrl)
    return DILQR_E_ARG;
  const void* ps[] = {x_init, u_init, C, c, xa, ua, xb, ub, ws, best_x, best_u};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = OneHidden::check(n, m, mlp)) return rc;
  if (B > kSmallMax || !mlp_small_ok(n, m)) return DILQR_E_SHAPE;
  if (B == 0) return 0;
  const MlpSolveArgs a{T, B, OneHidden::arg(mlp), x_init, u_init, C, c, mkb(bounds), linesearch_decay, max_linesearch_iter,
                       iterations, best_cost_eps, eps, not_improved_lim,
                       MlpSolveBufs{xa, ua, xb, ub, ws, cost, alpha, du_sq, full_du_norm, best_x, best_u, best_cost,
                                    best_du, ctrl},
                       S(stream)};
#define X(N_, M_) if (n == N_ && m == M_) return launch_mlp_mpc_solve_small_##N_##_##M_(a, mlp.activation);
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return DILQR_E_SHAPE;
}

}  // extern "C"
