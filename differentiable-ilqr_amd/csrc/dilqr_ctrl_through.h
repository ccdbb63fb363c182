// dilqr_ctrl_through.h — the reference's CtrlPassthroughDynamics
// (dynamics.py:133-156) as a device model over any base model: the state of the
// slew-rate augmentation (mpc_explicit.py:383-466) is  x~_t = [u_{t-1}; x_t],
//   x~_{t+1} = [u_t; f(x_t, u_t)],
// and its Jacobian with respect to [x~; u] = [u_{t-1}; x_t; u_t] is the
// reference's _F,
//   [ 0 0 I ]     rows 0..M:  the control, copied
//   [ 0 R S ]     rows M.. :  the base model's [R S].
// The zeros and ones are literals, so k_linearize's  f = x' - D tau~  only adds
// exact zero products to a sum that starts at +0 before it reaches the base
// model's terms: the lower block of F~, f~ has the base kernel's bits, the
// upper block of f~ is u - 1 * u = 0.
//
// Arg and load() are the base model's (Mlp2 points at its LDS column there; the
// launch carries the base model's dynamic LDS).  The model kernels
// (dilqr_model_kernels.h) and the line search (dilqr_forward.h) take it as any
// other model.  The fused iteration does not: it would want an FSparsity for
// the [0 0 I] rows.
#pragma once
#include "dilqr_device.h"

namespace dilqr {

template <class Base>
struct CtrlThrough {
  static constexpr int BN = Base::N, M = Base::M, N = BN + M, D = N + M, BD = BN + M, kAct = Base::kAct;
  static constexpr bool kForwardJacobian = true;   // forward_jacobian(): the base model's one walk
  using Arg = typename Base::Arg;
  Base base;

  DEV void load(const Arg& a) { base.load(a); }

  static DEV void state_of(const float (&xt)[N], float (&x)[BN]) {
#pragma unroll
    for (int i = 0; i < BN; ++i) x[i] = xt[M + i];
  }
  static DEV void put_forward(const float (&u)[M], const float (&ob)[BN], float (&o)[N]) {
#pragma unroll
    for (int a = 0; a < M; ++a) o[a] = u[a];
#pragma unroll
    for (int i = 0; i < BN; ++i) o[M + i] = ob[i];
  }
  static DEV void put_jacobian(const float (&Jb)[BN][BD], float (&J)[N][D]) {
#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
      for (int k = 0; k < D; ++k) J[a][k] = k == N + a ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < BN; ++i) {
#pragma unroll
      for (int k = 0; k < M; ++k) J[M + i][k] = 0.0f;
#pragma unroll
      for (int k = 0; k < BD; ++k) J[M + i][M + k] = Jb[i][k];
    }
  }

  // dynamics.py:140-156
  DEV void forward(const float (&xt)[N], const float (&u)[M], float (&o)[N]) const {
    float x[BN], ob[BN];
    state_of(xt, x);
    base.forward(x, u, ob);
    put_forward(u, ob, o);
  }
  // mpc_explicit.py:383-466: _F
  DEV void jacobian(const float (&xt)[N], const float (&u)[M], float (&J)[N][D]) const {
    float x[BN], Jb[BN][BD];
    state_of(xt, x);
    base.jacobian(x, u, Jb);
    put_jacobian(Jb, J);
  }
  DEV void forward_jacobian(const float (&xt)[N], const float (&u)[M], float (&o)[N], float (&J)[N][D]) const {
    float x[BN], ob[BN], Jb[BN][BD];
    state_of(xt, x);
    base.forward_jacobian(x, u, ob, Jb);
    put_forward(u, ob, o);
    put_jacobian(Jb, J);
  }
};

}  // namespace dilqr
