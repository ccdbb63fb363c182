// dilqr_mlp2_abi.h — host side of the dilqr_mlp2_* entry points (tu_mlp2.hip):
// the two-hidden-layer descriptor's checks, its kernel-argument form and the
// dispatch on (n, m, activation).  Beside dilqr_mlp_abi.h, whose shape list and
// Tag it uses.
#pragma once
#include "dilqr_common.h"
#include "dilqr_mlp2.h"
#include "dilqr_mlp_abi.h"

namespace dilqr {
namespace {

// the descriptor's own errors (the header's order: pointers, shape, activation)
inline int mlp2_check(int n, int m, const dilqr_mlp2& p) {
  const void* ps[] = {p.W1, p.b1, p.W2, p.b2, p.W3, p.b3};
  for (const void* q : ps) if (!q || !al16(q)) return DILQR_E_ARG;
  if (!mlp_shape_ok(n, m) || p.n_hidden1 < 1 || p.n_hidden1 > kMlpMaxHidden || p.n_hidden2 < 1 ||
      p.n_hidden2 > kMlpMaxHidden)
    return DILQR_E_SHAPE;
  if (p.activation != DILQR_MLP_SIGMOID && p.activation != DILQR_MLP_RELU) return DILQR_E_MODE;
  return 0;
}

inline Mlp2Arg mka2(const dilqr_mlp2& p) {
  return Mlp2Arg{p.n_hidden1, p.n_hidden2, p.passthrough, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3};
}

// fn(Tag<Mlp2<n, m, activation>>) for a checked descriptor
template <class Fn>
int mlp2_dispatch(int n, int m, int activation, Fn&& fn) {
#define X(N_, M_)                                              \
  if (n == N_ && m == M_) {                                    \
    if (activation == DILQR_MLP_SIGMOID) fn(Tag<Mlp2<N_, M_, DILQR_MLP_SIGMOID>>{}); \
    else fn(Tag<Mlp2<N_, M_, DILQR_MLP_RELU>>{});              \
    return launched();                                         \
  }
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return DILQR_E_SHAPE;
}

}  // namespace
}  // namespace dilqr
