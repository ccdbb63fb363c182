// dilqr_mlp_abi.h — host side of the dilqr_mlp_* entry points, shared by the
// units that define them (tu_mlp.hip, tu_mlp_vjp.hip): the descriptor's checks,
// its kernel-argument form and the dispatch on (n, m, activation).
#pragma once
#include "dilqr_common.h"
#include "dilqr_mlp.h"

namespace dilqr {
namespace {

template <class T>
struct Tag {
  using type = T;
};

inline bool mlp_shape_ok(int n, int m) {
#define X(N_, M_) if (n == N_ && m == M_) return true;
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return false;
}

// the descriptor's own errors (the header's order: pointers, shape, activation)
inline int mlp_check(int n, int m, const dilqr_mlp& p) {
  const void* ps[] = {p.W1, p.b1, p.W2, p.b2};
  for (const void* q : ps) if (!q || !al16(q)) return DILQR_E_ARG;
  if (!mlp_shape_ok(n, m) || p.n_hidden < 1 || p.n_hidden > kMlpMaxHidden) return DILQR_E_SHAPE;
  if (p.activation != DILQR_MLP_SIGMOID && p.activation != DILQR_MLP_RELU) return DILQR_E_MODE;
  return 0;
}

inline MlpArg mka(const dilqr_mlp& p) { return MlpArg{p.n_hidden, p.passthrough, p.W1, p.b1, p.W2, p.b2}; }

// fn(Tag<Mlp<n, m, activation>>) for a checked descriptor
template <class Fn>
int mlp_dispatch(int n, int m, int activation, Fn&& fn) {
#define X(N_, M_)                                              \
  if (n == N_ && m == M_) {                                    \
    if (activation == DILQR_MLP_SIGMOID) fn(Tag<Mlp<N_, M_, DILQR_MLP_SIGMOID>>{}); \
    else fn(Tag<Mlp<N_, M_, DILQR_MLP_RELU>>{});               \
    return launched();                                         \
  }
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return DILQR_E_SHAPE;
}

}  // namespace
}  // namespace dilqr
