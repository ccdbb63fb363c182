// tu_mlp2_slew.hip — learned dynamics with two hidden layers under the
// slew-rate augmentation (dynamics.py:133-156, mpc_explicit.py:383-466):
// rollout, linearisation and rollout + line search of  x~ = [u_prev; x]
// instantiated for CtrlThrough over the network (dilqr_ctrl_through.h), and
// their C-ABI.  The bodies are the templates of dilqr_mlp_entry.h on
// Slewed<TwoHidden>; (n, m) are the network's, the state buffers are n + m wide.
// Every launch carries the first layer's activations in dynamic LDS, as in
// tu_mlp2.hip.
#include "dilqr_mlp_entry.h"

using namespace dilqr;

extern "C" {

int dilqr_mlp2_slew_rollout_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x_init, const float* u,
                                float* x_out, void* stream) {
  return net_rollout<Slewed<TwoHidden>>(slew_n(n, m), m, T, B, mlp, x_init, u, x_out, stream);
}

int dilqr_mlp2_slew_linearize_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x, const float* u,
                                  float* F, float* f, void* stream) {
  return net_linearize<Slewed<TwoHidden>>(slew_n(n, m), m, T, B, mlp, x, u, F, f, stream);
}

int dilqr_mlp2_slew_lqr_forward_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x_init, const float* C,
                                    const float* c, const float* x, const float* u, const float* K, const float* k,
                                    dilqr_bounds bounds, const unsigned char* u_zero_I, float linesearch_decay,
                                    int max_linesearch_iter, float* x_out, float* u_out, float* cost, float* du_sq,
                                    float* alpha, const float* old_cost, void* stream) {
  return net_lqr_forward<Slewed<TwoHidden>>(slew_n(n, m), m, T, B, mlp, x_init, C, c, x, u, K, k, bounds, u_zero_I,
                                            linesearch_decay, max_linesearch_iter, x_out, u_out, cost, du_sq, alpha,
                                            old_cost, stream);
}

}  // extern "C"
