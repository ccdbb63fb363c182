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
};

}  // namespace dilqr
