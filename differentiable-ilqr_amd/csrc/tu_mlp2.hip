// tu_mlp2.hip — learned dynamics with two hidden layers on device: the model
// kernels (dynamics, Jacobian, rollout, linearisation) and the rollout + line
// search instantiated for the network of dilqr_mlp2.h, and their C-ABI.  Every
// launch carries the first layer's activations in dynamic LDS (256 H1 bytes).
#include "dilqr_common.h"
#include "dilqr_forward.h"
#include "dilqr_mlp2.h"
#include "dilqr_mlp2_abi.h"
#include "dilqr_model_kernels.h"

using namespace dilqr;

extern "C" {

int dilqr_mlp2_dynamics_f32(int n, int m, int N, dilqr_mlp2 mlp, const float* x, const float* u, float* out,
                            void* stream) {
  if (N < 0 || !x || !u || !out || !al16(x) || !al16(u) || !al16(out)) return DILQR_E_ARG;
  if (int rc = mlp2_check(n, m, mlp)) return rc;
  if (N == 0) return 0;
  const Mlp2Arg a = mka2(mlp);
  const size_t lds = mlp2_lds_bytes(a.H1);
  return mlp2_dispatch(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_dynamics<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(N, a, x, u, out);
  });
}

int dilqr_mlp2_linear_dyn_f32(int n, int m, int N, dilqr_mlp2 mlp, const float* x, const float* u, float* D,
                              void* stream) {
  if (N < 0 || !x || !u || !D || !al16(x) || !al16(u) || !al16(D)) return DILQR_E_ARG;
  if (int rc = mlp2_check(n, m, mlp)) return rc;
  if (N == 0) return 0;
  const Mlp2Arg a = mka2(mlp);
  const size_t lds = mlp2_lds_bytes(a.H1);
  return mlp2_dispatch(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_linear_dyn<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(N, a, x, u, D);
  });
}

int dilqr_mlp2_rollout_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x_init, const float* u,
                           float* x_out, void* stream) {
  if (T < 1 || B < 0 || !x_init || !u || !x_out) return DILQR_E_ARG;
  if (!al16(x_init) || !al16(u) || !al16(x_out)) return DILQR_E_ARG;
  if (int rc = mlp2_check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const Mlp2Arg a = mka2(mlp);
  const size_t lds = mlp2_lds_bytes(a.H1);
  return mlp2_dispatch(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_rollout<MD><<<grid_for(B), kBlock, lds, S(stream)>>>(T, B, a, x_init, u, x_out);
  });
}

int dilqr_mlp2_linearize_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x, const float* u, float* F,
                             float* f, void* stream) {
  if (T < 1 || B < 0 || !x || !u || !F || !f) return DILQR_E_ARG;
  if (!al16(x) || !al16(u) || !al16(F) || !al16(f)) return DILQR_E_ARG;
  if (int rc = mlp2_check(n, m, mlp)) return rc;
  const long long N = (long long)(T - 1) * B;
  if (N == 0) return 0;
  const Mlp2Arg a = mka2(mlp);
  const size_t lds = mlp2_lds_bytes(a.H1);
  return mlp2_dispatch(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_linearize<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(T, B, a, x, u, F, f);
  });
}

int dilqr_mlp2_lqr_forward_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x_init, const float* C,
                               const float* c, const float* x, const float* u, const float* K, const float* k,
                               dilqr_bounds bounds, const unsigned char* u_zero_I, float linesearch_decay,
                               int max_linesearch_iter, float* x_out, float* u_out, float* cost, float* du_sq,
                               float* alpha, const float* old_cost, void* stream) {
  if (T < 1 || B < 0 || max_linesearch_iter < 1) return DILQR_E_ARG;
  if (!x_init || !C || !c || !x || !u || !K || !k || !x_out || !u_out || !cost) return DILQR_E_ARG;
  const void* ps[] = {x_init, C, c, x, u, K, k, x_out, u_out};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = mlp2_check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const Bounds bd = mkb(bounds);
  const Mlp2Arg a = mka2(mlp);
  const size_t lds = mlp2_lds_bytes(a.H1);
  return mlp2_dispatch(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_lqr_forward<MD::N, MD::M, MD><<<grid_for(B), kBlock, lds, S(stream)>>>(
        T, B, a, nullptr, nullptr, x_init, C, c, x, u, K, k, bd, u_zero_I, linesearch_decay, max_linesearch_iter,
        x_out, u_out, cost, du_sq, alpha, old_cost);
  });
}

}  // extern "C"
