// tu_mlp2_vjp.hip — the gradient into the weights of the two-hidden-layer
// network (dilqr_mlp2.h) of its linearisation (dilqr_mlp2_linearize_f32:
// F = [R S], f = x' - F tau): the backward of mpc.py:494-519 through
// NNDynamics.grad_input (dynamics.py:92-130) and forward, for incoming
// gradients gF on F and gf on f.
//
// Per row, with tau = [x; u], o = gf, Gb = gF - gf tau^T (f = x' - F tau;
// passthrough adds weight-independent terms only), a = act(z), g = act'(z)
// formed from a as Mlp::activate / Mlp2::gate do, h = g (1 - 2a) for sigmoid
// and 0 for relu (the reference's relu mask carries no gradient):
//   z1 = b1 + W1 tau,  z2 = b2 + W2 a1
//   P_lk  = sum_j W2_lj g1_j W1_jk          (the tangent Mlp2::units forms)
//   U_lk  = sum_i W3_il Gb_ik     p2_l = sum_i W3_il o_i    s2_l = U_l . P_l
//   zh2_l = g2_l p2_l + h2_l s2_l           dP_lk = g2_l U_lk
//   da1_j = sum_l W2_lj zh2_l               dg1_j = sum_l W2_lj (dP_l . W1_j)
//   zh1_j = g1_j da1_j + h1_j dg1_j
// and summed over the rows:
//   db3_i = sum o_i       dW3_il = sum [o_i a2_l + g2_l (Gb_i . P_l)]
//   db2_l = sum zh2_l     E_lj = sum zh2_l a1_j     Gacc_lkj = sum dP_lk g1_j
//   db1_j = sum zh1_j     S1_jk = sum zh1_j tau_k
//   dW2_lj = E_lj + sum_k W1_jk Gacc_lkj    dW1_jk = S1_jk + sum_l W2_lj Gacc_lkj
// zh1 is linear in da1 and dg1, which are sums over the layer-2 units l: a wave
// that holds a block of units forms that block's share of zh1, S1 and db1, and
// the shares are added afterwards.  So one kernel does all the sums over rows.
//
// Mapping: one-wave workgroups, one row per lane, the weights read through the
// constant address space at wave-uniform addresses.  Kernel A, grid
// (G, NB = ceil(H2 / LB), ceil(H1 / 64)): wave (g, lb, t) takes the 64-row
// chunks g, g + G, ..., LB layer-2 units and, in the transposed steps 2 and 4,
// the first-layer units 64 t .. 64 t + 63 (for H1 > 64 the waves (g, lb, .)
// repeat step 1; t = 0 stores its sums).  The last block repeats unit H2 - 1
// in its spare places, with zh2 = dP = 0, and stores nothing for them.  H1 is
// bounded (DILQR_MLP2_VJP_MAX_HIDDEN1 = 128) so that a1 and X fit the 64 KiB of
// LDS a launch gets without raising the function's limit.  A lane past the last row
// stays in every loop with tau = o = Gb = 0 and adds exact zeros: no lane
// returns early (the transposed sums read what the other lanes wrote).  Per
// chunk, between one-wave barriers:
//  1. layer 1 into the lane's LDS column a1[j * 65 + row]; one walk over the
//     first layer for z2 and P of the block; zh2, dP.  dW3 and db2 (and db3 in
//     block 0) are lane-private sums over all chunks, reduced across the wave
//     once at the end (xor butterfly).  X = [zh2 | dP] (LB (d + 1) values per
//     row) goes to LDS as X[c][row].
//  2. E and Gacc, the product over the chunk's rows of X with [a1 | g1]: lane j
//     owns first-layer unit j (+ 64 t), reads row r of X at one address for all
//     lanes (a broadcast, four rows per ds_read_b128) and a1[j * 65 + r]
//     transposed; the
//     odd stride makes both the row-per-lane write (bank = row) and the
//     transposed read (bank = j + r) conflict-free.  The LB (d + 1) sums stay
//     private over all chunks.  Lanes whose unit is >= H1 read column H1 - 1
//     and store nothing.
//  3. row per lane again: the lane reads its zh2, dP back from X, walks the
//     first layer a second time (the wave's 64 units only) for the block's
//     da1_j and dg1_j and overwrites a1_j with the block's share of zh1_j; tau
//     replaces the first rows of X.
//  4. S1 and db1 shares, the product over rows of zh1 with [tau | 1], transposed
//     as in 2: d + 1 more private sums.
//
// Workspace, in floats (C = d + 1, LB = 4, or 2 where n d > 30):
//   P = n H2 + H2 + H2 C H1 + NB H1 C + n
//       one slab:  dW3 [n][H2] | db2 [H2] | EG [H2][C][H1] | NB x (S1 [H1][d] | db1 [H1]) | db3 [n]
//   G = max(1, min(ceil(rows / 64), max_waves > 0 ? max_waves : min(512, max(1, 2^24 / P))))
//   floats = (G + 1) P
// (the default cap keeps the slabs within 64 MiB; the last P hold their sum).
// The waves (g, .) between them write every element of slab g, so nothing is
// initialised.  Two more launches, fixed order, writing only: the sum of the G
// slabs as k_mlp_vjp_sum does it (wave s of a workgroup adds slabs s, s + 4,
// ..., the four sums are added in wave order), then the outputs: dW2 and dW1
// from the reduced E, Gacc and S1 shares (the sums over k, over the blocks and
// over l in ascending order), db1 from its shares, the rest copied.  No
// atomics, counters or fences: the same bits on every run.
#include "dilqr_common.h"
#include "dilqr_mlp2.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_mlp_vjp_common.h"

namespace dilqr {

constexpr int kVjp2MaxHidden1 = DILQR_MLP2_VJP_MAX_HIDDEN1;
static_assert(kVjp2MaxHidden1 <= 65535 * kBlock, "one grid z per 64 first-layer units");
// the dynamic LDS of kernel A stays under the 64 KiB a launch gets without raising the function's limit
static_assert(sizeof(float) * (kVjp2MaxHidden1 * 65 + 3 + 4 * 9 * 64) <= 65536, "a1 and X in 64 KiB of LDS");
constexpr int kVjp2Stride = 65;                    // odd: see above
constexpr int kVjp2SlabBudget = 1 << 24;           // floats of slabs under the default cap

// layer-2 units per wave: the row (n d + n + d), the walk's z2 / P / dP and the
// (n + 1 + d + 1) LB + d + 1 + n sums stay in registers
inline __host__ __device__ constexpr int vjp2_lb(int n, int m) { return n * (n + m) <= 30 ? 4 : 2; }

// the lane's row: tau, o = gf and Gb = gF - gf tau^T; zeros past the last row
template <class MD>
struct Vjp2Row {
  static constexpr int n = MD::N, m = MD::M, d = MD::D;
  float tau[d], o[n], Gb[n][d];
  DEV void load(long long r, long long rows, const float* __restrict__ x, const float* __restrict__ u,
                const float* __restrict__ gF, const float* __restrict__ gf) {
#pragma unroll
    for (int k = 0; k < d; ++k) tau[k] = 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      o[i] = 0.f;
#pragma unroll
      for (int k = 0; k < d; ++k) Gb[i][k] = 0.f;
    }
    if (r < rows) {
      float xi[n], ui[m];
      ld(xi, x + (size_t)r * n); ld(ui, u + (size_t)r * m);
#pragma unroll
      for (int i = 0; i < n; ++i) tau[i] = xi[i];
#pragma unroll
      for (int a = 0; a < m; ++a) tau[n + a] = ui[a];
      if (gf) ld(o, gf + (size_t)r * n);
      if (gF) ld2(Gb, gF + (size_t)r * n * d);
    }
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int k = 0; k < d; ++k) Gb[i][k] -= o[i] * tau[k];
  }
};

// layer 1 of the lane's row into its column a1[j * 65] (a1 already offset by the lane)
template <class MD>
DEV void vjp2_layer1(const MD& md, const float (&tau)[MD::D], float* a1) {
  constexpr int d = MD::D;
#pragma unroll 8
  for (int j = 0; j < md.H1; ++j) {
    float z = md.b1[j];
#pragma unroll
    for (int k = 0; k < d; ++k) z += md.W1[j * d + k] * tau[k];
    float a, g;
    MD::L1::activate(z, a, g);
    a1[j * kVjp2Stride] = a;
  }
}

// what one walk over the first layer gives for BLK layer-2 units
template <class MD, int BLK>
struct Vjp2Units {
  float a2[BLK], g2[BLK], zh[BLK], P[BLK][MD::D], dP[BLK][MD::D];
};

// units lq[0 .. BLK-1] (wave-uniform): z2 and P as Mlp2::units<., true, .> forms
// them, then U, p2, s2, zh2, dP
template <class MD, int BLK>
DEV void vjp2_units(const MD& md, const int (&lq)[BLK], const float* a1, const Vjp2Row<MD>& row,
                    Vjp2Units<MD, BLK>& t) {
  constexpr int n = MD::N, d = MD::D;
  const int H1 = md.H1, H2 = md.H2;
  float z2[BLK];
#pragma unroll
  for (int q = 0; q < BLK; ++q) {
    z2[q] = md.b2[lq[q]];
#pragma unroll
    for (int k = 0; k < d; ++k) t.P[q][k] = 0.f;
  }
#pragma unroll 8
  for (int j = 0; j < H1; ++j) {
    const float a = a1[j * kVjp2Stride];
    const float g = MD::gate(a);
    float w[d];
#pragma unroll
    for (int k = 0; k < d; ++k) w[k] = md.W1[j * d + k];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
      const float w2 = md.W2[lq[q] * H1 + j];
      z2[q] += w2 * a;
      const float s = w2 * g;
#pragma unroll
      for (int k = 0; k < d; ++k) t.P[q][k] += s * w[k];
    }
  }
#pragma unroll
  for (int q = 0; q < BLK; ++q) {
    MD::L1::activate(z2[q], t.a2[q], t.g2[q]);
    float p2 = 0.f, U[d];
#pragma unroll
    for (int k = 0; k < d; ++k) U[k] = 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float w3 = md.W3[i * H2 + lq[q]];
      p2 += w3 * row.o[i];
#pragma unroll
      for (int k = 0; k < d; ++k) U[k] += w3 * row.Gb[i][k];
    }
    float zh = t.g2[q] * p2;
    if constexpr (MD::kAct == DILQR_MLP_SIGMOID) {
      float s2 = 0.f;
#pragma unroll
      for (int k = 0; k < d; ++k) s2 += U[k] * t.P[q][k];
      zh += (t.g2[q] * (1.0f - 2.0f * t.a2[q])) * s2;
    }
    t.zh[q] = zh;
#pragma unroll
    for (int k = 0; k < d; ++k) t.dP[q][k] = t.g2[q] * U[k];
  }
}

// floats of the dynamic LDS before X (a1, rounded up so that X is 16-byte aligned)
inline __host__ __device__ int vjp2_a1_floats(int H1) { return (H1 * kVjp2Stride + 3) & ~3; }

template <class MD>
__global__ void __launch_bounds__(kBlock) k_mlp2_linearize_vjp(long long rows, Mlp2Arg arg,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ u,
                                                               const float* __restrict__ gF,
                                                               const float* __restrict__ gf,
                                                               float* __restrict__ ws, int P) {
  constexpr int n = MD::N, d = MD::D, C = d + 1, LB = vjp2_lb(MD::N, MD::M);
  extern __shared__ float vjp2_lds[];
  MD md; md.load(arg);
  const int H1 = md.H1, H2 = md.H2;
  const int lane = threadIdx.x;
  const int l0 = blockIdx.y * LB;
  const int j0 = blockIdx.z * kBlock, ju = j0 + lane;          // the wave's first-layer units; the lane's
  const int j1 = j0 + kBlock < H1 ? j0 + kBlock : H1;
  float* const a1s = vjp2_lds;                       // [H1][65]: a1, then the block's share of zh1
  float* const Xs = vjp2_lds + vjp2_a1_floats(H1);   // [LB * C][64]: X, then tau in its first d rows
  float* const a1 = a1s + lane;
  const float* const col = a1s + (ju < H1 ? ju : H1 - 1) * kVjp2Stride;       // unit ju, transposed
  int lq[LB];
#pragma unroll
  for (int q = 0; q < LB; ++q) lq[q] = l0 + q < H2 ? l0 + q : H2 - 1;
  float aW3[LB][n], ab2[LB], aEG[LB][C], aS1[d], ab1 = 0.f, ab3[n];
#pragma unroll
  for (int q = 0; q < LB; ++q) {
    ab2[q] = 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) aW3[q][i] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) aEG[q][c] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < d; ++k) aS1[k] = 0.f;
#pragma unroll
  for (int i = 0; i < n; ++i) ab3[i] = 0.f;

  const long long chunks = (rows + 63) / 64;
  for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    __syncthreads();                                 // the previous chunk's transposed reads are done
    float tau[d];
    {                                                // 1.
      Vjp2Row<MD> row;
      row.load(ch * 64 + lane, rows, x, u, gF, gf);
#pragma unroll
      for (int k = 0; k < d; ++k) tau[k] = row.tau[k];
#pragma unroll
      for (int i = 0; i < n; ++i) ab3[i] += row.o[i];
      vjp2_layer1(md, row.tau, a1);
      Vjp2Units<MD, LB> t;
      vjp2_units<MD, LB>(md, lq, a1, row, t);
#pragma unroll
      for (int q = 0; q < LB; ++q) {
        ab2[q] += t.zh[q];
#pragma unroll
        for (int i = 0; i < n; ++i) {
          float gp = 0.f;
#pragma unroll
          for (int k = 0; k < d; ++k) gp += row.Gb[i][k] * t.P[q][k];
          aW3[q][i] += row.o[i] * t.a2[q] + t.g2[q] * gp;
        }
        const bool real = l0 + q < H2;               // a repeated unit of the last block adds nothing
        Xs[(q * C) * 64 + lane] = real ? t.zh[q] : 0.f;
#pragma unroll
        for (int k = 0; k < d; ++k) Xs[(q * C + 1 + k) * 64 + lane] = real ? t.dP[q][k] : 0.f;
      }
    }
    __syncthreads();                                 // a1 and X of all 64 rows are written
#pragma unroll 1
    for (int r = 0; r < 64; r += 4) {                // 2.
      float av[4], gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        av[e] = col[r + e];
        gv[e] = MD::gate(av[e]);
      }
#pragma unroll
      for (int q = 0; q < LB; ++q)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float4 xv = *reinterpret_cast<const float4*>(Xs + (q * C + c) * 64 + r);
          const float* mv = c == 0 ? av : gv;
          aEG[q][c] += xv.x * mv[0];
          aEG[q][c] += xv.y * mv[1];
          aEG[q][c] += xv.z * mv[2];
          aEG[q][c] += xv.w * mv[3];
        }
    }
    __syncthreads();                                 // every lane has read the a1 columns and X
    {                                                // 3.
      float zh[LB], dP[LB][d];
#pragma unroll
      for (int q = 0; q < LB; ++q) {
        zh[q] = Xs[(q * C) * 64 + lane];
#pragma unroll
        for (int k = 0; k < d; ++k) dP[q][k] = Xs[(q * C + 1 + k) * 64 + lane];
      }
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        const float a = a1[j * kVjp2Stride];
        const float g = MD::gate(a);
        float w[d];
#pragma unroll
        for (int k = 0; k < d; ++k) w[k] = md.W1[j * d + k];
        float da = 0.f, dg = 0.f;
#pragma unroll
        for (int q = 0; q < LB; ++q) {
          const float w2 = md.W2[lq[q] * H1 + j];
          da += w2 * zh[q];
          if constexpr (MD::kAct == DILQR_MLP_SIGMOID) {          // relu: h1 = 0
            float pw = 0.f;
#pragma unroll
            for (int k = 0; k < d; ++k) pw += dP[q][k] * w[k];
            dg += w2 * pw;
          }
        }
        float z1 = g * da;
        if constexpr (MD::kAct == DILQR_MLP_SIGMOID) z1 += (g * (1.0f - 2.0f * a)) * dg;
        a1[j * kVjp2Stride] = z1;
      }
      // the lane's own places of X, which it has read above
#pragma unroll
      for (int k = 0; k < d; ++k) Xs[k * 64 + lane] = tau[k];
    }
    __syncthreads();                                 // zh1 and tau of all 64 rows are written
#pragma unroll 1
    for (int r = 0; r < 64; r += 4) {                // 4.
      float zv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) zv[e] = col[r + e];
      ab1 += zv[0];
      ab1 += zv[1];
      ab1 += zv[2];
      ab1 += zv[3];
#pragma unroll
      for (int k = 0; k < d; ++k) {
        const float4 tv = *reinterpret_cast<const float4*>(Xs + k * 64 + r);
        aS1[k] += zv[0] * tv.x;
        aS1[k] += zv[1] * tv.y;
        aS1[k] += zv[2] * tv.z;
        aS1[k] += zv[3] * tv.w;
      }
    }
  }

  float* __restrict__ slab = ws + (size_t)blockIdx.x * P;
  const int ob2 = n * H2, oEG = ob2 + H2, oS1 = oEG + H2 * C * H1 + blockIdx.y * (H1 * C);
  const int ob3 = oEG + H2 * C * H1 + gridDim.y * (H1 * C);
#pragma unroll
  for (int q = 0; q < LB; ++q) {
    const int l = l0 + q;
    if (l < H2) {                                    // wave-uniform
      if (blockIdx.z == 0) {
#pragma unroll
        for (int i = 0; i < n; ++i) {
          const float v = wave_sum(aW3[q][i]);
          if (lane == 0) slab[i * H2 + l] = v;
        }
        const float vb = wave_sum(ab2[q]);
        if (lane == 0) slab[ob2 + l] = vb;
      }
      if (ju < H1) {
#pragma unroll
        for (int c = 0; c < C; ++c) slab[oEG + (l * C + c) * H1 + ju] = aEG[q][c];
      }
    }
  }
  if (ju < H1) {
#pragma unroll
    for (int k = 0; k < d; ++k) slab[oS1 + ju * d + k] = aS1[k];
    slab[oS1 + H1 * d + ju] = ab1;
  }
  if (blockIdx.y == 0 && blockIdx.z == 0) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float v = wave_sum(ab3[i]);
      if (lane == 0) slab[ob3 + i] = v;
    }
  }
}

// out[e] = sum_g ws[g][e], e < P: wave s of a workgroup adds slabs s, s + 4, ...
// in that order, the four sums are added in wave order.  Writes, never accumulates.
__global__ void __launch_bounds__(kBlock* kVjpSumSlices) k_mlp2_vjp_sum(int G, int P, const float* __restrict__ ws,
                                                                         float* __restrict__ out) {
  __shared__ float part[kVjpSumSlices][kBlock];
  const int l = threadIdx.x & (kBlock - 1), s = threadIdx.x / kBlock;
  const int e = blockIdx.x * kBlock + l;
  float acc = 0.f;
  if (e < P) {
#pragma unroll 4
    for (int g = s; g < G; g += kVjpSumSlices) acc += ws[(size_t)g * P + e];
  }
  part[s][l] = acc;
  __syncthreads();
  if (s != 0 || e >= P) return;
  float v = part[0][l];
#pragma unroll
  for (int q = 1; q < kVjpSumSlices; ++q) v += part[q][l];
  out[e] = v;
}

// the six outputs from the reduced slab r, one element per thread:
//   dW2_lj = E_lj + sum_k W1_jk Gacc_lkj                        k = 0 .. d-1 in this order
//   dW1_jk = sum_b S1[b]_jk + sum_l W2_lj Gacc_lkj              b = 0 .. NB-1, then l = 0 .. H2-1
//   db1_j  = sum_b db1[b]_j                                     b = 0 .. NB-1
// the others are copies.
__global__ void __launch_bounds__(kBlock) k_mlp2_vjp_finish(int n, int d, int NB, Mlp2Arg a,
                                                            const float* __restrict__ r, float* __restrict__ dW1,
                                                            float* __restrict__ db1, float* __restrict__ dW2,
                                                            float* __restrict__ db2, float* __restrict__ dW3,
                                                            float* __restrict__ db3) {
  const int H1 = a.H1, H2 = a.H2, C = d + 1;
  const float* __restrict__ EG = r + n * H2 + H2;
  const float* __restrict__ S1 = EG + H2 * C * H1;
  int e = blockIdx.x * kBlock + threadIdx.x;
  if (e < H2 * H1) {
    const int l = e / H1, j = e - l * H1;
    float v = EG[(l * C) * H1 + j];
    for (int k = 0; k < d; ++k) v += a.W1[j * d + k] * EG[(l * C + 1 + k) * H1 + j];
    dW2[e] = v;
    return;
  }
  e -= H2 * H1;
  if (e < H1 * d) {
    const int j = e / d, k = e - j * d;
    float v = 0.f;
    for (int b = 0; b < NB; ++b) v += S1[b * (H1 * C) + e];
    for (int l = 0; l < H2; ++l) v += a.W2[l * H1 + j] * EG[(l * C + 1 + k) * H1 + j];
    dW1[e] = v;
    return;
  }
  e -= H1 * d;
  if (e < H1) {
    float v = 0.f;
    for (int b = 0; b < NB; ++b) v += S1[b * (H1 * C) + H1 * d + e];
    db1[e] = v;
    return;
  }
  e -= H1;
  if (e < n) { db3[e] = S1[NB * (H1 * C) + e]; return; }
  e -= n;
  if (e < n * H2) { dW3[e] = r[e]; return; }
  e -= n * H2;
  if (e < H2) db2[e] = r[n * H2 + e];
}

namespace {

inline int vjp2_blocks(int n, int m, int H2) { return (H2 + vjp2_lb(n, m) - 1) / vjp2_lb(n, m); }

inline long long vjp2_slab_floats(int n, int m, int H1, int H2) {
  const long long C = n + m + 1;
  return (long long)n * H2 + H2 + (long long)H2 * C * H1 + (long long)vjp2_blocks(n, m, H2) * H1 * C + n;
}

}  // namespace
}  // namespace dilqr

using namespace dilqr;

extern "C" {

size_t dilqr_mlp2_linearize_vjp_ws_bytes(int n, int m, int T, int B, int n_hidden1, int n_hidden2, int max_waves) {
  if (n < 1 || m < 1 || T < 1 || B < 0 || n_hidden1 < 1 || n_hidden1 > kVjp2MaxHidden1 || n_hidden2 < 1 ||
      n_hidden2 > kMlpMaxHidden || max_waves < 0)
    return 0;
  const long long rows = (long long)(T - 1) * B;
  const long long P = vjp2_slab_floats(n, m, n_hidden1, n_hidden2);
  return sizeof(float) * (size_t)((vjp_groups(rows, max_waves, kVjp2SlabBudget / P) + 1) * P);
}

int dilqr_mlp2_linearize_vjp_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* x, const float* u,
                                 const float* gF, const float* gf, float* dW1, float* db1, float* dW2, float* db2,
                                 float* dW3, float* db3, int max_waves, void* ws, size_t ws_bytes, void* stream) {
  if (T < 1 || B < 0 || max_waves < 0 || !x || !u || !dW1 || !db1 || !dW2 || !db2 || !dW3 || !db3 || !ws)
    return DILQR_E_ARG;
  const void* ps[] = {x, u, gF, gf, dW1, db1, dW2, db2, dW3, db3, ws};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (int rc = TwoHidden::check(n, m, mlp)) return rc;
  if (mlp.n_hidden1 > kVjp2MaxHidden1) return DILQR_E_SHAPE;
  if (ws_bytes < dilqr_mlp2_linearize_vjp_ws_bytes(n, m, T, B, mlp.n_hidden1, mlp.n_hidden2, max_waves))
    return DILQR_E_ARG;
  const long long rows = (long long)(T - 1) * B;
  if (rows == 0) return 0;                   // no rows: nothing launched, as every dilqr_mlp2_* call
  const Mlp2Arg a = TwoHidden::arg(mlp);
  const int H1 = a.H1, H2 = a.H2, d = n + m;
  const int P = (int)vjp2_slab_floats(n, m, H1, H2);
  const int G = (int)vjp_groups(rows, max_waves, kVjp2SlabBudget / P);
  const int NB = vjp2_blocks(n, m, H2);
  float* const w = static_cast<float*>(ws);
  float* const r = w + (size_t)G * P;
  const size_t lds = sizeof(float) * (vjp2_a1_floats(H1) + vjp2_lb(n, m) * (d + 1) * 64);
  return mlp_dispatch<TwoHidden>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_mlp2_linearize_vjp<MD><<<dim3(G, NB, (H1 + kBlock - 1) / kBlock), kBlock, lds, S(stream)>>>(rows, a, x, u, gF,
                                                                                                 gf, w, P);
    k_mlp2_vjp_sum<<<(P + kBlock - 1) / kBlock, kBlock * kVjpSumSlices, 0, S(stream)>>>(G, P, w, r);
    const int E = H2 * H1 + H1 * d + H1 + n + n * H2 + H2;
    k_mlp2_vjp_finish<<<(E + kBlock - 1) / kBlock, kBlock, 0, S(stream)>>>(n, d, NB, a, r, dW1, db1, dW2, db2, dW3,
                                                                          db3);
  });
}

}  // extern "C"
