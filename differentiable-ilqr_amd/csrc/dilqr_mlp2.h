// dilqr_mlp2.h — device model of the reference's NNDynamics with two hidden
// layers (dynamics.py:15-130; il_exp.py:123 writes [H, H] for learned dynamics):
//   x' = W3 act(W2 act(W1 [x;u] + b1) + b2) + b3   (+ x with passthrough),
// act = sigmoid or relu, and its Jacobian as grad_input chains it
// (dynamics.py:92-130):  W3 D2 W2 D1 W1  (+ I on the state block), D = diag(act')
// formed from the activation as Mlp::activate does (dilqr_mlp.h).
//
// Mapping: one row (problem) per lane, as for Mlp; every weight is read through
// the constant address space at a wave-uniform address (scalar loads).
//
// Layer 1: a1_j = act(b1_j + W1_j . tau) for j < H1, written to the lane's own
// column of a dynamic-LDS array [H1][64] (256 H1 bytes per one-wave workgroup;
// consecutive lanes are consecutive banks, so neither the write nor the read
// conflicts).  A lane reads back only what it wrote: no barrier, and a tail
// workgroup whose other lanes have returned needs none either.
//
// Layer 2, kBlk units l at a time:  z2_l = b2_l + sum_j W2_lj a1_j  and, when the
// Jacobian is wanted, the unit's tangent  P_lk = sum_j (W2_lj g1_j) W1_jk, k < d
// (the first layer's tangent g1_j W1_j is a per-lane scalar times a wave-uniform
// row and is never stored).  Then a2 = act(z2_l), o_i += W3_il a2 and
// J_ik += (W3_il g2) P_lk.  One LDS read of a1_j feeds the kBlk accumulators;
// nothing is stored per layer-2 unit.  About 2 H2 H1 (d + 2) FLOP per
// linearised row.
#pragma once
#include "dilqr_device.h"
#include "dilqr_mlp.h"

namespace dilqr {

// the model as the kernels receive it (by value, a kernel argument)
struct Mlp2Arg {
  int H1, H2, passthrough;
  const float *W1, *b1, *W2, *b2, *W3, *b3;
};

typedef const __attribute__((address_space(4))) float* Mlp2W;

// the dynamic LDS of a launch: the [H1][kBlock] array of first-layer activations
inline size_t mlp2_lds_bytes(int H1) { return sizeof(float) * 64 * (size_t)H1; }

// the dynamic LDS of the implicit backward's launch (dilqr_mlp_implicit.h): a1,
// then one region that is v during jacobian_lag (sigmoid only) and the staging
// area of the wave's records (64 d^2 floats) between the walks
inline size_t mlp2_implicit_lds_bytes(int H1, int d, bool sigmoid) {
  const size_t v = sigmoid ? mlp2_lds_bytes(H1) : 0, rec = sizeof(float) * 64 * (size_t)d * d;
  return mlp2_lds_bytes(H1) + (v > rec ? v : rec);
}

template <int N_, int M_, int ACT>
struct Mlp2 {
  static constexpr int N = N_, M = M_, D = N_ + M_, kAct = ACT;
  static constexpr bool kForwardJacobian = true;   // forward_jacobian(): one walk over both layers
  // layer-2 units per pass over the first layer's activations: the forward
  // alone keeps kBlkF sums, the Jacobian kBlkJ sums and kBlkJ tangents of D
  // floats beside its N*D accumulators (sized so that no instantiation spills).
  // These and the unroll by 8 of the loops over the first layer are the
  // measured choice (profiles/nn_mlp2/ab_unroll_block.txt): eight consecutive
  // weights of a row come as one scalar load; 16 spills in the (6,2) Jacobian
  static constexpr int kBlkF = 8, kBlkJ = 4;
  // jacobian_lag's units per pass: its tangents stand beside the N*D Jacobian
  // and the D (D + 1) / 2 entries of M (profiles/nn_mlp2_implicit/resource_usage.txt)
  static constexpr int kBlkL = 4;
  using Arg = Mlp2Arg;
  using L1 = Mlp<N_, M_, ACT>;                     // activate(): the one-layer model's
  int H1, H2;
  bool pt;
  Mlp2W W1, b1, W2, b2, W3, b3;
  float* a1;                                       // this lane's column of the LDS array: a1[j * 64]

  DEV void load(const Mlp2Arg& a) {
    extern __shared__ float mlp2_lds[];
    H1 = a.H1; H2 = a.H2;
    pt = a.passthrough != 0;
    W1 = (Mlp2W)a.W1; b1 = (Mlp2W)a.b1; W2 = (Mlp2W)a.W2; b2 = (Mlp2W)a.b2; W3 = (Mlp2W)a.W3; b3 = (Mlp2W)a.b3;
    a1 = mlp2_lds + (threadIdx.x & 63);
  }

  // act' from the stored activation (dynamics.py:107-118), as Mlp::activate forms it
  static DEV float gate(float a) {
    if constexpr (ACT == DILQR_MLP_RELU) return a > 0.f ? 1.f : 0.f;
    else return a * (1.0f - a);
  }

  // BLK layer-2 units from l0 on: their pre-activations (and tangents) over the
  // first layer, then their contribution to the output (and the Jacobian)
  template <bool FWD, bool JAC, int BLK>
  DEV void units(int l0, float (&acc)[N], float (&Jr)[N][D]) const {
    float z2[BLK], P[BLK][D];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
      z2[q] = b2[l0 + q];
#pragma unroll
      for (int k = 0; k < D; ++k) P[q][k] = 0.f;
    }
#pragma unroll 8
    for (int j = 0; j < H1; ++j) {
      const float a = a1[j * 64];
      if constexpr (JAC) {
        const float g = gate(a);
        float w[D];
#pragma unroll
        for (int k = 0; k < D; ++k) w[k] = W1[j * D + k];
#pragma unroll
        for (int q = 0; q < BLK; ++q) {
          const float w2 = W2[(l0 + q) * H1 + j];
          z2[q] += w2 * a;
          const float s = w2 * g;
#pragma unroll
          for (int k = 0; k < D; ++k) P[q][k] += s * w[k];
        }
      } else {
#pragma unroll
        for (int q = 0; q < BLK; ++q) z2[q] += W2[(l0 + q) * H1 + j] * a;
      }
    }
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
      float a2, g2;
      L1::activate(z2[q], a2, g2);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w3 = W3[i * H2 + l0 + q];
        if constexpr (FWD) acc[i] += w3 * a2;
        if constexpr (JAC) {
          const float s = w3 * g2;
#pragma unroll
          for (int k = 0; k < D; ++k) Jr[i][k] += s * P[q][k];
        }
      }
    }
  }

  template <bool FWD, bool JAC>
  DEV void walk(const float (&x)[N], const float (&u)[M], float (*o)[N], float (*J)[N][D]) const {
    constexpr int BLK = JAC ? kBlkJ : kBlkF;
    float tau[D], acc[N], Jr[N][D];
#pragma unroll
    for (int i = 0; i < N; ++i) tau[i] = x[i];
#pragma unroll
    for (int a = 0; a < M; ++a) tau[N + a] = u[a];
    // layer 1 into the lane's LDS column
#pragma unroll 8
    for (int j = 0; j < H1; ++j) {
      float z = b1[j];
#pragma unroll
      for (int k = 0; k < D; ++k) z += W1[j * D + k] * tau[k];
      float a, g;
      L1::activate(z, a, g);
      a1[j * 64] = a;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      acc[i] = FWD ? b3[i] : 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) Jr[i][k] = 0.f;
    }
    int l = 0;
    for (; l + BLK <= H2; l += BLK) units<FWD, JAC, BLK>(l, acc, Jr);
    for (; l < H2; ++l) units<FWD, JAC, 1>(l, acc, Jr);
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

  // dynamics.py:66-90
  DEV void forward(const float (&x)[N], const float (&u)[M], float (&o)[N]) const {
    walk<true, false>(x, u, &o, nullptr);
  }
  // dynamics.py:92-130: [R S]
  DEV void jacobian(const float (&x)[N], const float (&u)[M], float (&J)[N][D]) const {
    walk<false, true>(x, u, nullptr, &J);
  }
  DEV void forward_jacobian(const float (&x)[N], const float (&u)[M], float (&o)[N], float (&J)[N][D]) const {
    walk<true, true>(x, u, &o, &J);
  }

  // The Jacobian and, from the same walk, the Lagrangian Hessian of the
  // dynamics for multipliers lam (the implicit backward, tu_mlp2_implicit.hip;
  // the contract of Mlp::jacobian_lag).  With P the tangent units() forms,
  // s = W3^T lam, v = W2^T (s o g2), c = act'' = g (1 - 2a) for sigmoid:
  //   M = sum_i lam_i d^2 f_i / d tau^2 = P^T diag(s o c2) P + W1^T diag(v o c1) W1
  // relu has act'' = 0: its M is zero and callers take jacobian() instead; the
  // passthrough adds nothing to M.
  //   FULL  Mu gets the D (D + 1) / 2 entries on and above the diagonal, row by
  //         row ((0,0), (0,1), .., (0,D-1), (1,1), ..)
  //   else  My = M y as P^T ((s o c2) o (P y)) + W1^T ((v o c1) o (W1 y))
  // v is a second LDS column of the lane, v[j * 64] = a1[(H1 + j) * 64]: the
  // launch carries 2 * mlp2_lds_bytes(H1).  As with a1 the lane reads only what
  // it wrote (no barrier), and every sum runs in a fixed order.  v is dead
  // between two walks (each zeroes it first), so the implicit kernel stages its
  // records there (staging(); mlp2_implicit_lds_bytes sizes the region for both).
  DEV float* staging() const {
    extern __shared__ float mlp2_lds[];
    return mlp2_lds + H1 * 64;
  }

  // the first term and J from BLK layer-2 units, and their share of v
  template <bool FULL, int BLK>
  DEV void lag_units(int l0, const float (&lam)[N], const float (*y)[D], float (&Jr)[N][D],
                     float (*Mu)[D * (D + 1) / 2], float (*My)[D]) const {
    float z2[BLK], P[BLK][D];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
      z2[q] = b2[l0 + q];
#pragma unroll
      for (int k = 0; k < D; ++k) P[q][k] = 0.f;
    }
#pragma unroll 8
    for (int j = 0; j < H1; ++j) {
      const float a = a1[j * 64];
      const float g = gate(a);
      float w[D];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = W1[j * D + k];
#pragma unroll
      for (int q = 0; q < BLK; ++q) {
        const float w2 = W2[(l0 + q) * H1 + j];
        z2[q] += w2 * a;
        const float s = w2 * g;
#pragma unroll
        for (int k = 0; k < D; ++k) P[q][k] += s * w[k];
      }
    }
    float sg[BLK];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
      float a2, g2;
      L1::activate(z2[q], a2, g2);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w3 = W3[i * H2 + l0 + q];
        s += w3 * lam[i];
        const float r = w3 * g2;
#pragma unroll
        for (int k = 0; k < D; ++k) Jr[i][k] += r * P[q][k];
      }
      sg[q] = s * g2;
      const float h = s * (g2 * (1.0f - 2.0f * a2));
      if constexpr (FULL) {
        int e = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float hk = h * P[q][k];
#pragma unroll
          for (int l = k; l < D; ++l) (*Mu)[e++] += hk * P[q][l];
        }
      } else {
        float py = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) py += P[q][k] * (*y)[k];
        const float hp = h * py;
#pragma unroll
        for (int k = 0; k < D; ++k) (*My)[k] += hp * P[q][k];
      }
    }
    float* const v = a1 + H1 * 64;
#pragma unroll 8
    for (int j = 0; j < H1; ++j) {
      float s = v[j * 64];
#pragma unroll
      for (int q = 0; q < BLK; ++q) s += W2[(l0 + q) * H1 + j] * sg[q];
      v[j * 64] = s;
    }
  }

  template <bool FULL>
  DEV void jacobian_lag(const float (&x)[N], const float (&u)[M], const float (&lam)[N], const float (*y)[D],
                        float (&J)[N][D], float (*Mu)[D * (D + 1) / 2], float (*My)[D]) const {
    static_assert(ACT == DILQR_MLP_SIGMOID, "relu: M = 0, use jacobian()");
    float tau[D], Jr[N][D];
#pragma unroll
    for (int i = 0; i < N; ++i) tau[i] = x[i];
#pragma unroll
    for (int a = 0; a < M; ++a) tau[N + a] = u[a];
    float* const v = a1 + H1 * 64;
#pragma unroll 8
    for (int j = 0; j < H1; ++j) {
      float z = b1[j];
#pragma unroll
      for (int k = 0; k < D; ++k) z += W1[j * D + k] * tau[k];
      float a, g;
      L1::activate(z, a, g);
      a1[j * 64] = a;
      v[j * 64] = 0.f;
    }
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
    int l = 0;
    for (; l + kBlkL <= H2; l += kBlkL) lag_units<FULL, kBlkL>(l, lam, y, Jr, Mu, My);
    for (; l < H2; ++l) lag_units<FULL, 1>(l, lam, y, Jr, Mu, My);
    // the second term: the one-layer walk's body with h1_j = v_j c1_j
#pragma unroll 4
    for (int j = 0; j < H1; ++j) {
      const float a = a1[j * 64];
      const float h = v[j * 64] * (gate(a) * (1.0f - 2.0f * a));
      float w[D];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = W1[j * D + k];
      if constexpr (FULL) {
        int e = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float hk = h * w[k];
#pragma unroll
          for (int q = k; q < D; ++q) (*Mu)[e++] += hk * w[q];
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
