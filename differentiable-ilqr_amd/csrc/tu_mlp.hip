// tu_mlp.hip — learned dynamics on device: the model kernels (dynamics,
// Jacobian, rollout, linearisation) and the rollout + line search instantiated
// for the one-hidden-layer network of dilqr_mlp.h, and their C-ABI (the bodies
// are the templates of dilqr_mlp_entry.h).
#include "dilqr_mlp_entry.h"

using namespace dilqr;

extern "C" {

int dilqr_mlp_dynamics_f32(int n, int m, int N, dilqr_mlp mlp, const float* x, const float* u, float* out,
                           void* stream) {
  return net_dynamics<OneHidden>(n, m, N, mlp, x, u, out, stream);
}

int dilqr_mlp_linear_dyn_f32(int n, int m, int N, dilqr_mlp mlp, const float* x, const float* u, float* D,
                             void* stream) {
  return net_linear_dyn<OneHidden>(n, m, N, mlp, x, u, D, stream);
}

int dilqr_mlp_rollout_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x_init, const float* u,
                          float* x_out, void* stream) {
  return net_rollout<OneHidden>(n, m, T, B, mlp, x_init, u, x_out, stream);
}

int dilqr_mlp_linearize_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x, const float* u, float* F,
                            float* f, void* stream) {
  return net_linearize<OneHidden>(n, m, T, B, mlp, x, u, F, f, stream);
}

int dilqr_mlp_lqr_forward_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x_init, const float* C,
                              const float* c, const float* x, const float* u, const float* K, const float* k,
                              dilqr_bounds bounds, const unsigned char* u_zero_I, float linesearch_decay,
                              int max_linesearch_iter, float* x_out, float* u_out, float* cost, float* du_sq,
                              float* alpha, const float* old_cost, void* stream) {
  return net_lqr_forward<OneHidden>(n, m, T, B, mlp, x_init, C, c, x, u, K, k, bounds, u_zero_I, linesearch_decay,
                                    max_linesearch_iter, x_out, u_out, cost, du_sq, alpha, old_cost, stream);
}

}  // extern "C"
