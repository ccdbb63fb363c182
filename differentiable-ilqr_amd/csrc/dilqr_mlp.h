// dilqr_mlp.h — device model of the reference's NNDynamics with one hidden
// layer (dynamics.py:15-130):  x' = W2 act(W1 [x;u] + b1) + b2  (+ x with
// passthrough), act = sigmoid or relu, and its Jacobian as grad_input writes it
// (dynamics.py:92-130):  W2 diag(act') W1  (+ I on the state block), act' =
// a(1-a) for sigmoid, (a > 0) for relu.  No control clamp.
//
// Mapping: one row (problem) per lane.  The weights are the same for every
// lane, so each lane walks the hidden units j = 0..H-1 with wave-uniform weight
// addresses:  z_j = b1_j + W1_j . tau,  a_j = act(z_j),  o_i += W2_ij a_j,
// J_ik += (W2_ij act'_j) W1_jk.  No activation is stored; the live state is the
// n*d + n + d accumulators.  W1 [H,d], b1 [H], W2 [n,H], b2 [n] are torch's
// nn.Linear layouts, read in place.
//
// Weight reads: through the constant address space — the addresses are
// wave-uniform, so the compiler issues scalar loads and the weights never
// occupy vector registers.  (Staging them in LDS once per workgroup was
// measured and lost)
#pragma once
#include <type_traits>

#include "dilqr_device.h"

namespace dilqr {

constexpr int kMlpMaxHidden = DILQR_MLP_MAX_HIDDEN;

// the model as the kernels receive it (by value, a kernel argument)
struct MlpArg {
  int H, passthrough;
  const float *W1, *b1, *W2, *b2;
};

typedef const __attribute__((address_space(4))) float* MlpW;

template <int N_, int M_, int ACT>
struct Mlp {
  static constexpr int N = N_, M = M_, D = N_ + M_, kAct = ACT;
  static constexpr bool kForwardJacobian = true;   // forward_jacobian(): one walk over the hidden units
  using Arg = MlpArg;
  int H;
  bool pt;
  MlpW W1, b1, W2, b2;

  DEV void load(const MlpArg& a) {
    H = a.H;
    pt = a.passthrough != 0;
    W1 = (MlpW)a.W1; b1 = (MlpW)a.b1; W2 = (MlpW)a.W2; b2 = (MlpW)a.b2;
  }

  // a = act(z), g = act'(z) as grad_input forms it from a (dynamics.py:107-118)
  static DEV void activate(float z, float& a, float& g) {
    if constexpr (ACT == DILQR_MLP_RELU) {
      a = fmaxf(z, 0.f);
      g = a > 0.f ? 1.f : 0.f;
    } else {
      a = vrcp(1.0f + __expf(-z));
      g = a * (1.0f - a);
    }
  }

  // the line search's pair of candidates: each component is the float
  // activation of that component (__expf + vrcp, the relu gate), so a packed
  // evaluation rounds like two scalar ones (dilqr_device.h)
  static DEV void activate(f2 z, f2& a, f2& g) {
    float a0, g0, a1, g1;
    activate(z.x, a0, g0);
    activate(z.y, a1, g1);
    a = f2{a0, a1};
    g = f2{g0, g1};
  }

  // S: float, or f2 for the value of two trajectories at once (FWD only; the
  // weights are scalars either way, so each component is the float walk)
  template <bool FWD, bool JAC, class S>
  DEV void walk(const S (&x)[N], const S (&u)[M], S (*o)[N], float (*J)[N][D]) const {
    static_assert(!JAC || std::is_same_v<S, float>, "the Jacobian is formed for one trajectory");
    S tau[D], acc[N];
    float Jr[N][D];
#pragma unroll
    for (int i = 0; i < N; ++i) tau[i] = x[i];
#pragma unroll
    for (int a = 0; a < M; ++a) tau[N + a] = u[a];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      acc[i] = S(FWD ? b2[i] : 0.f);
#pragma unroll
      for (int k = 0; k < D; ++k) Jr[i][k] = 0.f;
    }
#pragma unroll 4
    for (int j = 0; j < H; ++j) {
      float w[D];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = W1[j * D + k];
      S z = S(b1[j]);
#pragma unroll
      for (int k = 0; k < D; ++k) z += w[k] * tau[k];
      S a, g;
      activate(z, a, g);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w2 = W2[i * H + j];
        if constexpr (FWD) acc[i] += w2 * a;
        if constexpr (JAC) {
          const float s = w2 * g;
#pragma unroll
          for (int k = 0; k < D; ++k) Jr[i][k] += s * w[k];
        }
      }
    }
    if constexpr (FWD) {
#pragma unroll
      for (int i = 0; i < N; ++i) (*o)[i] = pt ? acc[i] + x[i] : acc[i];
    }
    if constexpr (JAC) {
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int k = 0; k < D; ++k) (*J)[i][k] = (pt && i == k) ? Jr[i][k] + 1.0f : Jr[i][k];
    }
  }

  // what the fused iteration (dilqr_fused.h) asks of a model besides these:
  // every entry of the Jacobian is a function of (x, u), and none of it can be
  // read off the rollout's x_{t+1}
  using FSparsity = DenseF;
  static constexpr bool kJacFromNext = false;

  // dynamics.py:66-90 (S = f2: the line search's two candidates)
  template <class S>
  DEV void forward(const S (&x)[N], const S (&u)[M], S (&o)[N]) const {
    walk<true, false, S>(x, u, &o, nullptr);
  }
  // dynamics.py:92-130: [R S]
  DEV void jacobian(const float (&x)[N], const float (&u)[M], float (&J)[N][D]) const {
    walk<false, true, float>(x, u, nullptr, &J);
  }
  DEV void forward_jacobian(const float (&x)[N], const float (&u)[M], float (&o)[N], float (&J)[N][D]) const {
    walk<true, true, float>(x, u, &o, &J);
  }

  // The Jacobian and, from the same walk, the Lagrangian Hessian of the
  // dynamics for multipliers lam (the implicit backward, tu_mlp_implicit.hip):
  //   M = sum_i lam_i d^2 f_i / d tau^2 = W1^T diag(h) W1,
  //   h_j = (W2^T lam)_j act''(z_j),  act'' = g (1 - 2a) for sigmoid
  // (the h of tu_mlp_vjp.hip).  relu has act'' = 0: its M is zero and callers
  // take jacobian() instead; the passthrough adds nothing to M.  z_j, a_j and
  // the row W1_j are read once per unit.  M is symmetric:
  //   FULL  Mu gets its D (D + 1) / 2 entries on and above the diagonal, row by
  //         row ((0,0), (0,1), .., (0,D-1), (1,1), ..)
  //   else  My = M y as W1^T (h o (W1 y)): M is never formed
  template <bool FULL>
  DEV void jacobian_lag(const float (&x)[N], const float (&u)[M], const float (&lam)[N], const float (*y)[D],
                        float (&J)[N][D], float (*Mu)[D * (D + 1) / 2], float (*My)[D]) const {
    static_assert(ACT == DILQR_MLP_SIGMOID, "relu: M = 0, use jacobian()");
    float tau[D], Jr[N][D];
#pragma unroll
    for (int i = 0; i < N; ++i) tau[i] = x[i];
#pragma unroll
    for (int a = 0; a < M; ++a) tau[N + a] = u[a];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int k = 0; k < D; ++k) Jr[i][k] = 0.f;
    if constexpr (FULL) {
#pragma unroll
      for (int e = 0; e < D * (D + 1) / 2; ++e) (*Mu)[e] = 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) (*My)[k] = 0.f;
    }
#pragma unroll 4
    for (int j = 0; j < H; ++j) {
      float w[D];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = W1[j * D + k];
      float z = b1[j];
#pragma unroll
      for (int k = 0; k < D; ++k) z += w[k] * tau[k];
      float a, g;
      activate(z, a, g);
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w2 = W2[i * H + j];
        p += w2 * lam[i];
        const float s = w2 * g;
#pragma unroll
        for (int k = 0; k < D; ++k) Jr[i][k] += s * w[k];
      }
      const float h = p * (g * (1.0f - 2.0f * a));
      if constexpr (FULL) {
        int e = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float hk = h * w[k];
#pragma unroll
          for (int l = k; l < D; ++l) (*Mu)[e++] += hk * w[l];
        }
      } else {
        float wy = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) wy += w[k] * (*y)[k];
        const float hw = h * wy;
#pragma unroll
        for (int k = 0; k < D; ++k) (*My)[k] += hw * w[k];
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int k = 0; k < D; ++k) J[i][k] = (pt && i == k) ? Jr[i][k] + 1.0f : Jr[i][k];
  }
};

}  // namespace dilqr
