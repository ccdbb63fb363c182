// dilqr_mlp_implicit.h — the kernel of the DiLQR implicit backward with a
// network as the dynamics, written once over the kind of network: MD is the
// one-hidden-layer model (dilqr_mlp.h, instantiated by tu_mlp_implicit.hip) or
// the two-hidden-layer one (dilqr_mlp2.h, tu_mlp2_implicit.hip).  What it
// computes, and the three passes, are in the header of tu_mlp_implicit.hip; the
// kind of network enters through MD::Arg, md.jacobian (F_t) and
// md.jacobian_lag (F_t with M_t, or with M_t y_t) only.  The workspace layout
// is the same for both kinds (dilqr_mlp_implicit_ws_floats serves both).  The
// staging area of the wave's records (64 d^2 floats) is static LDS, unless the
// model has LDS of its own that is dead between its walks and offers it
// (md.staging(), Mlp2: the column v of jacobian_lag).
#pragma once
#include <type_traits>

#include "dilqr_common.h"
#include "dilqr_implicit_common.h"

namespace dilqr {

template <int n, int m> struct MlpImplicitWs {
  static constexpr int d = n + m;
  static constexpr int G = m * n + m;                  // K_t, k_t of the modified Riccati step
  // floats per (t, b): the gain planes, the y planes, slack so the y region
  // starts 16-byte aligned whatever T*B is
  static constexpr int REC = G + d + 4;
  static DEV size_t y_off(int T, int B) { return ((size_t)T * B * G + 3) / 4 * 4; }
};

// MD::staging() exists: the records are staged in the model's own LDS
template <class MD, class = void>
struct StagesInModelLds : std::false_type {};
template <class MD>
struct StagesInModelLds<MD, std::void_t<decltype(&MD::staging)>> : std::true_type {};

template <class MD>
__global__ void __launch_bounds__(kBlock) k_mlp_implicit_backward(
    int T, int B, typename MD::Arg arg, const float* __restrict__ C, const float* __restrict__ c,
    const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ dl_dx,
    const float* __restrict__ dl_du, Bounds bd, float* __restrict__ ws, float* __restrict__ dx_init,
    float* __restrict__ dC, float* __restrict__ dc, float* __restrict__ dF, float* __restrict__ df) {
  constexpr int n = MD::N, m = MD::M, d = n + m;
  constexpr bool kHess = MD::kAct == DILQR_MLP_SIGMOID;      // relu: M = 0, compiled out
  using W = MlpImplicitWs<n, m>;
  constexpr int G = W::G;
  // every lane of the wave runs (pass D stores the wave's records together);
  // lanes past the batch shadow problem B-1 and store nothing
  const int lane = threadIdx.x, b0 = blockIdx.x * kBlock;
  const int nvalid = B - b0 < kBlock ? B - b0 : kBlock;
  const bool valid = lane < nvalid;
  const int b = valid ? b0 + lane : B - 1;
  MD md; md.load(arg);
  // one staging area for the four record kinds of a step (d*d is the largest):
  // the wave's LDS accesses complete in program order
  float* s_rec;
  if constexpr (StagesInModelLds<MD>::value) {
    s_rec = md.staging();
  } else {
    __shared__ __attribute__((aligned(16))) float s_static[kBlock * d * d];
    s_rec = s_static;
  }
  float* const wsG = ws;
  float* const wsY = ws + W::y_off(T, B);
  const bool want_dF = dF != nullptr;
  auto active = [&](size_t tb, int a, float ua) -> bool {
    if (bd.mode == DILQR_BOUNDS_NONE) return false;
    return fabsf(ua - bound_lo(bd, tb * m + a)) <= 1e-8f || fabsf(ua - bound_hi(bd, tb * m + a)) <= 1e-8f;
  };
  auto zero_D = [](float (&D)[n][d]) {
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int j = 0; j < d; ++j) D[i][j] = 0.f;
  };
  // ---------------- B: costates, M_t, Riccati of the C + M problem
  {
    RiccatiState<n, m> rs;
    rs.init();
    float lam[n];
#pragma unroll
    for (int i = 0; i < n; ++i) lam[i] = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b;
      float Cp[d][d], ct[d], xt[n], ut[m], gxx[n], gu[m];
      ld2(Cp, C + tb * d * d); ld(ct, c + tb * d); ld(xt, x + tb * n); ld(ut, u + tb * m);
      ld(gxx, dl_dx + tb * n); ld(gu, dl_du + tb * m);
      float D[n][d];
      // lam_t is formed from C_t before M_t is added to it
      float cx[n];
#pragma unroll
      for (int i = 0; i < n; ++i) cx[i] = ct[i];
      if (t < T - 1) {
        if constexpr (kHess) {
          float Mu[d * (d + 1) / 2];
          md.template jacobian_lag<true>(xt, ut, lam, nullptr, D, &Mu, nullptr);   // lam = lam_{t+1}
          costate_step<n, m>(Cp, cx, xt, ut, D, lam);
          int e = 0;
#pragma unroll
          for (int i = 0; i < d; ++i)
#pragma unroll
            for (int j = i; j < d; ++j) {
              const float mij = Mu[e++];
              Cp[i][j] += mij;
              if (j != i) Cp[j][i] += mij;
            }
        } else {
          md.jacobian(xt, ut, D);
          costate_step<n, m>(Cp, cx, xt, ut, D, lam);
        }
      } else {
        zero_D(D);
        costate_step<n, m>(Cp, cx, xt, ut, D, lam);
      }
      float cb[d];
#pragma unroll
      for (int i = 0; i < n; ++i) cb[i] = -gxx[i];
#pragma unroll
      for (int a = 0; a < m; ++a) cb[n + a] = -gu[a];
      float zI[m], lb[m], ub[m];
#pragma unroll
      for (int a = 0; a < m; ++a) { zI[a] = active(tb, a, ut[a]) ? 1.f : 0.f; lb[a] = ub[a] = 0.f; }
      float Kt[m][n], kt[m];
      if (bd.mode != DILQR_BOUNDS_NONE) rs.template step<GAIN_ZERO_I>(Cp, cb, D, zI, lb, ub, Kt, kt);
      else rs.template step<GAIN_UNC>(Cp, cb, D, zI, lb, ub, Kt, kt);
      float gr[G];
#pragma unroll
      for (int a = 0; a < m; ++a) {
#pragma unroll
        for (int j = 0; j < n; ++j) gr[a * n + j] = Kt[a][j];
        gr[m * n + a] = kt[a];
      }
      if (valid) SoaRec<G>::store(wsG, gr, T, t, B, b);
    }
  }
  // ---------------- C (t up): the rollout y of the modified problem (linear,
  // alpha = 1, active controls zeroed)
  {
    float yx[n];
#pragma unroll
    for (int i = 0; i < n; ++i) yx[i] = 0.f;
    for (int t = 0; t < T; ++t) {
      const size_t tb = (size_t)t * B + b;
      float xt[n], ut[m], gr[G];
      ld(xt, x + tb * n); ld(ut, u + tb * m);
      SoaRec<G>::load(gr, wsG, T, t, B, b);
      float y[d];
#pragma unroll
      for (int i = 0; i < n; ++i) y[i] = yx[i];
#pragma unroll
      for (int a = 0; a < m; ++a) {
        float s_ = 0.f;
#pragma unroll
        for (int j = 0; j < n; ++j) s_ += gr[a * n + j] * yx[j];
        y[n + a] = active(tb, a, ut[a]) ? 0.f : s_ + gr[m * n + a];
      }
      if (valid) SoaRec<d>::store(wsY, y, T, t, B, b);
      if (t < T - 1) {
        float D[n][d];
        md.jacobian(xt, ut, D);
#pragma unroll
        for (int i = 0; i < n; ++i) {
          float s_ = 0.f;
#pragma unroll
          for (int j = 0; j < d; ++j) s_ += D[i][j] * y[j];
          yx[i] = s_;
        }
      }
    }
  }
  // ---------------- D: lam, w, dlam; dC, dc, dF, df, dx_init (t down)
  {
    float lam[n], dlam[n];
#pragma unroll
    for (int i = 0; i < n; ++i) { lam[i] = 0.f; dlam[i] = 0.f; }
    for (int t = T - 1; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b, tb0 = (size_t)t * B + b0;
      float Ct[d][d], ct[d], xt[n], ut[m], gxx[n], y[d];
      ld2(Ct, C + tb * d * d); ld(ct, c + tb * d); ld(xt, x + tb * n); ld(ut, u + tb * m);
      ld(gxx, dl_dx + tb * n);
      SoaRec<d>::load(y, wsY, T, t, B, b);
      float tau[d];
#pragma unroll
      for (int i = 0; i < n; ++i) tau[i] = xt[i];
#pragma unroll
      for (int a = 0; a < m; ++a) tau[n + a] = ut[a];
      {
        // dC_t = -0.5 (y tau^T + tau y^T), dc_t = -y
        float dCt[d * d], dct[d];
#pragma unroll
        for (int i = 0; i < d; ++i) {
#pragma unroll
          for (int j = 0; j < d; ++j) dCt[i * d + j] = -0.5f * (y[i] * tau[j] + tau[i] * y[j]);
          dct[i] = -y[i];
        }
        wave_store_records_any<d * d>(dC + tb0 * d * d, dCt, s_rec, lane, nvalid);
        wave_store_records_any<d>(dc + tb0 * d, dct, s_rec, lane, nvalid);
      }
      float D[n][d], wx[n];
      if (t < T - 1) {
        if constexpr (kHess) {
          float My[d];
          md.template jacobian_lag<false>(xt, ut, lam, &y, D, nullptr, &My);       // lam = lam_{t+1}
#pragma unroll
          for (int k = 0; k < n; ++k) wx[k] = gxx[k] - My[k];
        } else {
          md.jacobian(xt, ut, D);
#pragma unroll
          for (int k = 0; k < n; ++k) wx[k] = gxx[k];
        }
        if (want_dF) {
          // dF_t = -(dlam_{t+1} tau^T + lam_{t+1} y^T), df_t = -dlam_{t+1}
          float dFt[n * d], dft[n];
#pragma unroll
          for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int j = 0; j < d; ++j) dFt[i * d + j] = -(dlam[i] * tau[j] + lam[i] * y[j]);
            dft[i] = -dlam[i];
          }
          wave_store_records_any<n * d>(dF + tb0 * n * d, dFt, s_rec, lane, nvalid);
          wave_store_records_any<n>(df + tb0 * n, dft, s_rec, lane, nvalid);
        }
      } else {
        zero_D(D);
#pragma unroll
        for (int k = 0; k < n; ++k) wx[k] = gxx[k];
      }
      // dlam_t = Cxx y_x + Cxu y_u - w_x + F_x^T dlam_{t+1}; lam_t by the pass-B recursion
      float nd[n];
#pragma unroll
      for (int i = 0; i < n; ++i) {
        float s = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int j = 0; j < n; ++j) s += Ct[i][j] * y[j];
#pragma unroll
        for (int a = 0; a < m; ++a) s2 += Ct[i][n + a] * y[n + a];
#pragma unroll
        for (int l = 0; l < n; ++l) s3 += D[l][i] * dlam[l];
        nd[i] = ((s + s2) - wx[i]) + s3;
      }
#pragma unroll
      for (int i = 0; i < n; ++i) dlam[i] = nd[i];
      float cx[n];
#pragma unroll
      for (int i = 0; i < n; ++i) cx[i] = ct[i];
      costate_step<n, m>(Ct, cx, xt, ut, D, lam);
    }
    if (valid) {
      float o[n];
#pragma unroll
      for (int i = 0; i < n; ++i) o[i] = -dlam[i];
      st(dx_init + (size_t)b * n, o);
    }
  }
}

}  // namespace dilqr
