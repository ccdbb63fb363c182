// dilqr_mlp_entry.h — the five entry points every kind of network has
// (dynamics, Jacobian, rollout, linearisation, rollout + line search), written
// once over the traits of dilqr_mlp_abi.h: argument checks, the zero-size early
// return, the launch of the shared model kernels.  tu_mlp.hip and tu_mlp2.hip
// define their extern "C" names as single calls of these.
#pragma once
#include "dilqr_common.h"
#include "dilqr_forward.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_model_kernels.h"

namespace dilqr {
namespace {

template <class Net>
int net_dynamics(int n, int m, int N, const typename Net::Desc& mlp, const float* x, const float* u, float* out,
                 void* stream) {
  if (N < 0 || !x || !u || !out || !al16(x) || !al16(u) || !al16(out)) return DILQR_E_ARG;
  if (int rc = Net::check(n, m, mlp)) return rc;
  if (N == 0) return 0;
  const typename Net::Arg a = Net::arg(mlp);
  const size_t lds = Net::lds_bytes(n, m, a);
  return mlp_dispatch<Net>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_dynamics<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(N, a, x, u, out);
  });
}

template <class Net>
int net_linear_dyn(int n, int m, int N, const typename Net::Desc& mlp, const float* x, const float* u, float* D,
                   void* stream) {
  if (N < 0 || !x || !u || !D || !al16(x) || !al16(u) || !al16(D)) return DILQR_E_ARG;
  if (int rc = Net::check(n, m, mlp)) return rc;
  if (N == 0) return 0;
  const typename Net::Arg a = Net::arg(mlp);
  const size_t lds = Net::lds_bytes(n, m, a);
  return mlp_dispatch<Net>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_linear_dyn<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(N, a, x, u, D);
  });
}

template <class Net>
int net_rollout(int n, int m, int T, int B, const typename Net::Desc& mlp, const float* x_init, const float* u,
                float* x_out, void* stream) {
  if (T < 1 || B < 0 || !x_init || !u || !x_out) return DILQR_E_ARG;
  if (!al16(x_init) || !al16(u) || !al16(x_out)) return DILQR_E_ARG;
  if (int rc = Net::check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const typename Net::Arg a = Net::arg(mlp);
  const size_t lds = Net::lds_bytes(n, m, a);
  return mlp_dispatch<Net>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_rollout<MD><<<grid_for(B), kBlock, lds, S(stream)>>>(T, B, a, x_init, u, x_out);
  });
}

template <class Net>
int net_linearize(int n, int m, int T, int B, const typename Net::Desc& mlp, const float* x, const float* u, float* F,
                  float* f, void* stream) {
  if (T < 1 || B < 0 || !x || !u || !F || !f) return DILQR_E_ARG;
  if (!al16(x) || !al16(u) || !al16(F) || !al16(f)) return DILQR_E_ARG;
  if (int rc = Net::check(n, m, mlp)) return rc;
  const long long N = (long long)(T - 1) * B;
  if (N == 0) return 0;
  const typename Net::Arg a = Net::arg(mlp);
  const size_t lds = Net::lds_bytes(n, m, a);
  return mlp_dispatch<Net>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_linearize<MD><<<grid_for(N), kBlock, lds, S(stream)>>>(T, B, a, x, u, F, f);
  });
}

template <class Net>
int net_lqr_forward(int n, int m, int T, int B, const typename Net::Desc& mlp, const float* x_init, const float* C,
                    const float* c, const float* x, const float* u, const float* K, const float* k,
                    dilqr_bounds bounds, const unsigned char* u_zero_I, float linesearch_decay,
                    int max_linesearch_iter, float* x_out, float* u_out, float* cost, float* du_sq, float* alpha,
                    const float* old_cost, void* stream) {
  if (T < 1 || B < 0 || max_linesearch_iter < 1) return DILQR_E_ARG;
  if (!x_init || !C || !c || !x || !u || !K || !k || !x_out || !u_out || !cost) return DILQR_E_ARG;
  const void* ps[] = {x_init, C, c, x, u, K, k, x_out, u_out};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = Net::check(n, m, mlp)) return rc;
  if (B == 0) return 0;
  const Bounds bd = mkb(bounds);
  const typename Net::Arg a = Net::arg(mlp);
  const size_t lds = Net::lds_bytes(n, m, a);
  return mlp_dispatch<Net>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_lqr_forward<MD::N, MD::M, MD><<<grid_for(B), kBlock, lds, S(stream)>>>(
        T, B, a, nullptr, nullptr, x_init, C, c, x, u, K, k, bd, u_zero_I, linesearch_decay, max_linesearch_iter,
        x_out, u_out, cost, du_sq, alpha, old_cost);
  });
}

}  // namespace
}  // namespace dilqr
