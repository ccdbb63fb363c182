// tu_mlp_vjp.hip — the gradient into the network's weights of the MLP
// linearisation (dilqr_mlp_linearize_f32: F = [R S], f = x' - F tau): the
// backward of mpc.py:494-519 through NNDynamics.grad_input (dynamics.py:92-130)
// and forward, for incoming gradients gF on F and gf on f.
//
// Per row, with tau = [x; u], z_j = b1_j + W1_j . tau, a_j = act(z_j), g_j =
// act'(z_j) as Mlp::activate forms them, h_j = g_j (1 - 2 a_j) for sigmoid and
// 0 for relu (the reference's relu mask carries no gradient), o = gf and
// Gb = gF - gf tau^T (f = x' - F tau; passthrough adds weight-independent
// terms only):
//   r_i  = sum_k Gb_ik W1_jk         q_k = sum_i W2_ij Gb_ik
//   p    = sum_i W2_ij o_i           s   = sum_i W2_ij r_i
//   zh   = g_j p + h_j s
//   dW1_jk += g_j q_k + zh tau_k     db1_j += zh
//   dW2_ij += o_i a_j + g_j r_i      db2_i += o_i
// Nothing couples two hidden units, so the units are cut into blocks of JB.
//
// Mapping (that of Mlp::walk): one row per lane, the lane holds tau, o and Gb
// in VGPRs, the weights are read at wave-uniform addresses through Mlp::load.
// Kernel A, grid (G, ceil(H / JB)), one wave per workgroup: wave (g, hb) takes
// the 64-row chunks g, g + G, g + 2G, ... and the hidden units of block hb,
// keeps their (d + 1 + n) JB sums lane-private over all of its chunks, reduces
// them once across the wave (xor butterfly, a fixed order) and stores its part
// of slab g of the workspace [G][P], P = H (d + 1) + n H + n laid out as
// dW1 | db1 | dW2 | db2.  The waves (g, *) between them write every element of
// slab g, so nothing is zeroed beforehand.  Kernel B, a second launch, writes
// each output element as the sum of its G partials in a fixed order.  No
// atomics, counters or fences: the result is the same bits on every run.
#include "dilqr_common.h"
#include "dilqr_mlp.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_mlp_vjp_common.h"

namespace dilqr {

// hidden units per wave of kernel A: the accumulators ((d + 1 + n) JB) and the
// row (n d + n + d) stay in registers
template <class MD>
constexpr int vjp_block() { return MD::N * MD::D <= 30 ? 8 : 4; }

template <class MD>
__global__ void __launch_bounds__(kBlock) k_mlp_linearize_vjp(long long rows, MlpArg arg,
                                                              const float* __restrict__ x,
                                                              const float* __restrict__ u,
                                                              const float* __restrict__ gF,
                                                              const float* __restrict__ gf,
                                                              float* __restrict__ ws, int P) {
  constexpr int n = MD::N, m = MD::M, d = MD::D, JB = vjp_block<MD>();
  MD md; md.load(arg);
  const int H = md.H;
  const int lane = threadIdx.x;
  const int j0 = blockIdx.y * JB;
  float aW1[JB][d], ab1[JB], aW2[JB][n], ab2[n];
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) {
    ab1[jj] = 0.f;
#pragma unroll
    for (int k = 0; k < d; ++k) aW1[jj][k] = 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) aW2[jj][i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < n; ++i) ab2[i] = 0.f;

  const long long chunks = (rows + 63) / 64;
  for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    // a lane past the last row stays in the loop with o = Gb = 0 (every sum
    // below then gets an exact zero from it): the wave reduction needs all lanes
    const long long r = ch * 64 + lane;
    float tau[d], o[n], Gb[n][d];
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
    for (int i = 0; i < n; ++i) {
      ab2[i] += o[i];
#pragma unroll
      for (int k = 0; k < d; ++k) Gb[i][k] -= o[i] * tau[k];
    }
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
      const int j = j0 + jj;
      if (j < H) {                                  // wave-uniform
        float w[d], w2[n];
#pragma unroll
        for (int k = 0; k < d; ++k) w[k] = md.W1[j * d + k];
#pragma unroll
        for (int i = 0; i < n; ++i) w2[i] = md.W2[i * H + j];
        float z = md.b1[j];
#pragma unroll
        for (int k = 0; k < d; ++k) z += w[k] * tau[k];
        float a, g;
        MD::activate(z, a, g);
        float p = 0.f, s = 0.f, q[d];
#pragma unroll
        for (int k = 0; k < d; ++k) q[k] = 0.f;
#pragma unroll
        for (int i = 0; i < n; ++i) {
          float ri = 0.f;
#pragma unroll
          for (int k = 0; k < d; ++k) {
            ri += Gb[i][k] * w[k];
            q[k] += w2[i] * Gb[i][k];
          }
          p += w2[i] * o[i];
          s += w2[i] * ri;
          aW2[jj][i] += o[i] * a + g * ri;
        }
        float zh = g * p;
        if constexpr (MD::kAct == DILQR_MLP_SIGMOID) zh += (g * (1.0f - 2.0f * a)) * s;
#pragma unroll
        for (int k = 0; k < d; ++k) aW1[jj][k] += g * q[k] + zh * tau[k];
        ab1[jj] += zh;
      }
    }
  }

  float* __restrict__ slab = ws + (size_t)blockIdx.x * P;
  const int oW1 = 0, ob1 = H * d, oW2 = ob1 + H, ob2 = oW2 + n * H;
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) {
    const int j = j0 + jj;
    if (j < H) {
#pragma unroll
      for (int k = 0; k < d; ++k) {
        const float v = wave_sum(aW1[jj][k]);
        if (lane == 0) slab[oW1 + j * d + k] = v;
      }
      const float vb = wave_sum(ab1[jj]);
      if (lane == 0) slab[ob1 + j] = vb;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const float v = wave_sum(aW2[jj][i]);
        if (lane == 0) slab[oW2 + i * H + j] = v;
      }
    }
  }
  if (blockIdx.y == 0) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float v = wave_sum(ab2[i]);
      if (lane == 0) slab[ob2 + i] = v;
    }
  }
}

// out[e] = sum_g ws[g][e]: wave s of a workgroup adds slabs s, s + 4, ... in
// that order, the four sums are added in wave order.  Writes, never accumulates.
__global__ void __launch_bounds__(kBlock* kVjpSumSlices) k_mlp_vjp_sum(int G, int P, const float* __restrict__ ws,
                                                                        int nW1, int nb1, int nW2,
                                                                        float* __restrict__ dW1,
                                                                        float* __restrict__ db1,
                                                                        float* __restrict__ dW2,
                                                                        float* __restrict__ db2) {
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
  if (e < nW1) dW1[e] = v;
  else if (e < nW1 + nb1) db1[e - nW1] = v;
  else if (e < nW1 + nb1 + nW2) dW2[e - nW1 - nb1] = v;
  else db2[e - nW1 - nb1 - nW2] = v;
}

namespace {

inline long long vjp_slab_floats(int n, int m, int H) { return (long long)H * (n + m + 1) + (long long)n * H + n; }

}  // namespace
}  // namespace dilqr

using namespace dilqr;

extern "C" {

size_t dilqr_mlp_linearize_vjp_ws_bytes(int n, int m, int T, int B, int n_hidden, int max_waves) {
  if (n < 1 || m < 1 || T < 1 || B < 0 || n_hidden < 1 || max_waves < 0) return 0;
  const long long rows = (long long)(T - 1) * B;
  return sizeof(float) * (size_t)(vjp_groups(rows, max_waves) * vjp_slab_floats(n, m, n_hidden));
}

int dilqr_mlp_linearize_vjp_f32(int n, int m, int T, int B, dilqr_mlp mlp, const float* x, const float* u,
                                const float* gF, const float* gf, float* dW1, float* db1, float* dW2, float* db2,
                                int max_waves, void* ws, size_t ws_bytes, void* stream) {
  if (T < 1 || B < 0 || max_waves < 0 || !x || !u || !dW1 || !db1 || !dW2 || !db2 || !ws) return DILQR_E_ARG;
  const void* ps[] = {x, u, gF, gf, dW1, db1, dW2, db2, ws};
  for (const void* p : ps) if (!al16(p)) return DILQR_E_ARG;
  if (int rc = OneHidden::check(n, m, mlp)) return rc;
  if (ws_bytes < dilqr_mlp_linearize_vjp_ws_bytes(n, m, T, B, mlp.n_hidden, max_waves)) return DILQR_E_ARG;
  const long long rows = (long long)(T - 1) * B;
  if (rows == 0) return 0;                   // no rows: nothing launched, as every dilqr_mlp_* call
  const MlpArg a = OneHidden::arg(mlp);
  const int H = a.H, d = n + m;
  const int P = (int)vjp_slab_floats(n, m, H);
  const int G = (int)vjp_groups(rows, max_waves);
  const size_t lds = OneHidden::lds_bytes(n, m, a);
  float* w = static_cast<float*>(ws);
  return mlp_dispatch<OneHidden>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    constexpr int JB = vjp_block<MD>();
    k_mlp_linearize_vjp<MD><<<dim3(G, (H + JB - 1) / JB), kBlock, lds, S(stream)>>>(rows, a, x, u, gF, gf, w, P);
    k_mlp_vjp_sum<<<(P + kBlock - 1) / kBlock, kBlock * kVjpSumSlices, 0, S(stream)>>>(G, P, w, H * d, H, n * H,
                                                                                    dW1, db1, dW2, db2);
  });
}

}  // extern "C"
