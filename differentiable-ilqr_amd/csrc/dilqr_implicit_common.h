// dilqr_implicit_common.h — what the one-problem-per-lane implicit backward
// kernels share (tu_implicit.hip: pendulum, cartpole; tu_mlp_implicit.hip: the
// one-hidden-layer network): the primal costate step and the coalesced store of
// a wave's per-(t, b) records.
#pragma once
#include "dilqr_common.h"

namespace dilqr {

// lam_t = Cxx x + Cxu u + c_x + F_x^T lam_{t+1}   (lqr_step_explicit.py:305-319);
// D is zero at t = T-1.  Passes B and D run this same function on the same
// inputs, so they hold the same bits.
template <int n, int m, class FS = DenseF>
DEV void costate_step(const float (&Ct)[n + m][n + m], const float (&cx)[n], const float (&xt)[n],
                      const float (&ut)[m], const float (&D)[n][n + m], float (&lam)[n]) {
  float nl[n];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    float s = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < n; ++j) s += Ct[i][j] * xt[j];
#pragma unroll
    for (int a = 0; a < m; ++a) s2 += Ct[i][n + a] * ut[a];
    float s3 = 0.f;
#pragma unroll
    for (int l = 0; l < n; ++l)
      if (FS::nz(l, i)) s3 += D[l][i] * lam[l];
    nl[i] = ((s + s2) + cx[i]) + s3;
  }
#pragma unroll
  for (int i = 0; i < n; ++i) lam[i] = nl[i];
}

// One wave's records of K floats for problems b0 .. b0+63 of one step are one
// contiguous run of 64*K floats ([t, b, K] layout).  Each lane writes its record
// to LDS and the wave stores the run coalesced (a 1-KiB dwordx4 run per
// instruction) instead of each lane storing its own 144-byte record: per-lane
// record stores ran at half the HBM write rate of coalesced ones
// (tools/microbench/store_patterns.hip).  One wave per workgroup
// (kBlock = 64): its LDS accesses complete in program order, so the wave
// barriers (scheduling only) are the whole synchronisation.  Lane strides of K
// dwords (K/4 float4, K/2 float2) keep the b128 / b64 writes bank-conflict free
// for the K used here (16, 36; 4, 6).
template <int K>
DEV void wave_store_records(float* __restrict__ base, const float (&r)[K], float* __restrict__ lds, int lane,
                            int nvalid) {
  static_assert(K % 2 == 0, "records of an even number of floats");
  __builtin_amdgcn_wave_barrier();                 // the previous step's reads of lds precede these writes
  if constexpr (K % 4 == 0) {
    constexpr int Q = K / 4;
    float4* L = reinterpret_cast<float4*>(lds);
#pragma unroll
    for (int i = 0; i < Q; ++i) L[lane * Q + i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
    __builtin_amdgcn_wave_barrier();
    float4* g = reinterpret_cast<float4*>(base);
    const int nv = nvalid * Q;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int i = lane + 64 * j;
      if (i < nv) g[i] = L[i];
    }
  } else {
    constexpr int Q = K / 2;
    float2* L = reinterpret_cast<float2*>(lds);
#pragma unroll
    for (int i = 0; i < Q; ++i) L[lane * Q + i] = make_float2(r[2 * i], r[2 * i + 1]);
    __builtin_amdgcn_wave_barrier();
    float2* g = reinterpret_cast<float2*>(base);
    const int nv = nvalid * Q;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int i = lane + 64 * j;
      if (i < nv) g[i] = L[i];
    }
  }
}

// wave_store_records for a record of any length: an odd K (d = 3, 5, 7 give
// odd d, d*d and n) goes through LDS dword by dword — a lane stride of K dwords,
// K odd, is bank-conflict free too — and out as 64-dword runs.
template <int K>
DEV void wave_store_records_any(float* __restrict__ base, const float (&r)[K], float* __restrict__ lds, int lane,
                                int nvalid) {
  if constexpr (K % 2 == 0) {
    wave_store_records<K>(base, r, lds, lane, nvalid);
  } else {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < K; ++i) lds[lane * K + i] = r[i];
    __builtin_amdgcn_wave_barrier();
    const int nv = nvalid * K;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int i = lane + 64 * j;
      if (i < nv) base[i] = lds[i];
    }
  }
}

}  // namespace dilqr
