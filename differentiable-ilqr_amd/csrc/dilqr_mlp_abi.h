// dilqr_mlp_abi.h — host side of the dilqr_mlp_* and dilqr_mlp2_* entry points,
// shared by every unit that defines one (tu_mlp.hip, tu_mlp2.hip, tu_mpc_mlp.hip,
// tu_mlp_implicit.hip, tu_mlp2_implicit.hip, tu_mlp_vjp.hip, tu_mlp2_vjp.hip, tu_mlp_slew.hip,
// tu_mlp2_slew.hip).  A kind of network is
// described once, by a traits type (OneHidden, TwoHidden): its C descriptor, its
// kernel-argument form, its device model, the descriptor's checks and the
// dynamic LDS of a launch.  The dispatch on (n, m, activation) is written once
// over the traits.  A third kind of network is one more traits type here.
#pragma once
#include <initializer_list>

#include "dilqr_common.h"
#include "dilqr_ctrl_through.h"
#include "dilqr_mlp.h"
#include "dilqr_mlp2.h"

namespace dilqr {
namespace {

template <class T>
struct Tag {
  using type = T;
};

constexpr bool mlp_shape_ok(int n, int m) {
#define X(N_, M_) if (n == N_ && m == M_) return true;
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return false;
}

// a descriptor's own errors (the header's order: pointers, shape, activation)
inline int mlp_check_desc(int n, int m, std::initializer_list<const void*> weights, std::initializer_list<int> widths,
                          int activation) {
  for (const void* q : weights) if (!q || !al16(q)) return DILQR_E_ARG;
  if (!mlp_shape_ok(n, m)) return DILQR_E_SHAPE;
  for (int H : widths) if (H < 1 || H > kMlpMaxHidden) return DILQR_E_SHAPE;
  if (activation != DILQR_MLP_SIGMOID && activation != DILQR_MLP_RELU) return DILQR_E_MODE;
  return 0;
}

// one hidden layer: dilqr_mlp, the model of dilqr_mlp.h
struct OneHidden {
  using Desc = dilqr_mlp;
  using Arg = MlpArg;
  template <int N_, int M_, int ACT>
  using Model = Mlp<N_, M_, ACT>;
  static int check(int n, int m, const Desc& p) {
    return mlp_check_desc(n, m, {p.W1, p.b1, p.W2, p.b2}, {p.n_hidden}, p.activation);
  }
  static Arg arg(const Desc& p) { return Arg{p.n_hidden, p.passthrough, p.W1, p.b1, p.W2, p.b2}; }
  static size_t lds_bytes(int, int, const Arg&) { return 0; }
};

// two hidden layers: dilqr_mlp2, the model of dilqr_mlp2.h
struct TwoHidden {
  using Desc = dilqr_mlp2;
  using Arg = Mlp2Arg;
  template <int N_, int M_, int ACT>
  using Model = Mlp2<N_, M_, ACT>;
  static int check(int n, int m, const Desc& p) {
    return mlp_check_desc(n, m, {p.W1, p.b1, p.W2, p.b2, p.W3, p.b3}, {p.n_hidden1, p.n_hidden2}, p.activation);
  }
  static Arg arg(const Desc& p) {
    return Arg{p.n_hidden1, p.n_hidden2, p.passthrough, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3};
  }
  static size_t lds_bytes(int, int, const Arg& a) { return mlp2_lds_bytes(a.H1); }
};

// a network under the slew-rate augmentation (dilqr_ctrl_through.h): the same
// descriptor, argument and LDS, the model CtrlThrough over the network's.  Here
// (n, m) are the augmented system's, n = the network's n + m; both it and the
// network's own (n - m, m) must be shapes of DILQR_FOR_EACH_SHAPE.
template <class Net>
struct Slewed {
  using Desc = typename Net::Desc;
  using Arg = typename Net::Arg;
  template <int N_, int M_, int ACT>
  using Model = CtrlThrough<typename Net::template Model<N_ - M_, M_, ACT>>;
  template <int N_, int M_>
  static constexpr bool kServes = mlp_shape_ok(N_ - M_, M_);
  static int check(int n, int m, const Desc& p) {
    if (int rc = Net::check(n - m, m, p)) return rc;
    return mlp_shape_ok(n, m) ? 0 : DILQR_E_SHAPE;
  }
  static Arg arg(const Desc& p) { return Net::arg(p); }
  static size_t lds_bytes(int n, int m, const Arg& a) { return Net::lds_bytes(n - m, m, a); }
};

// the augmented state's width for a network's (n, m) as the dilqr_*_slew_*
// entry points receive them; sizes no network has give no shape at all
inline int slew_n(int n, int m) { return n >= 1 && m >= 1 && n <= 64 && m <= 64 ? n + m : -1; }

// the shapes of DILQR_FOR_EACH_SHAPE a kind has kernels for: all of them,
// unless it says otherwise (kServes<n, m>)
template <class Net, int N_, int M_, class = void>
struct NetServes : std::true_type {};
template <class Net, int N_, int M_>
struct NetServes<Net, N_, M_, std::void_t<decltype(Net::template kServes<N_, M_>)>>
    : std::bool_constant<Net::template kServes<N_, M_>> {};

// fn(Tag<Net::Model<n, m, activation>>) for a checked descriptor
template <class Net, class Fn>
int mlp_dispatch(int n, int m, int activation, Fn&& fn) {
#define X(N_, M_)                                                                                     \
  if constexpr (NetServes<Net, N_, M_>::value) if (n == N_ && m == M_) {                              \
    if (activation == DILQR_MLP_SIGMOID) fn(Tag<typename Net::template Model<N_, M_, DILQR_MLP_SIGMOID>>{}); \
    else fn(Tag<typename Net::template Model<N_, M_, DILQR_MLP_RELU>>{});                             \
    return launched();                                                                                \
  }
  DILQR_FOR_EACH_SHAPE(X)
#undef X
  return DILQR_E_SHAPE;
}

}  // namespace
}  // namespace dilqr
