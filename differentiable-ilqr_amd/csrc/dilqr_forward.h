// dilqr_forward.h — the standalone rollout + line search (lqr_forward,
// lqr_step_explicit.py:166-263) for one problem per lane, templated on the true
// dynamics: LinDx (NoModel) or a Model with load() and forward().  Shared by
// tu_forward.hip (LinDx and the env_dx models) and tu_mlp.hip (the network).
#pragma once
#include "dilqr_common.h"
#include "dilqr_model_kernels.h"

namespace dilqr {

// ============================================================ forward / line search
// lqr_forward (lqr_step_explicit.py:166-263), one problem per lane, the batch's
// `while any(cost > old_cost)` loop evaluated per problem (each problem's alpha
// depends only on its own cost, so this is the reference's result).
struct NoModel {};

template <int n, int m, class Model>
struct Dyn {
  Model md;
  const float* F;
  const float* f;
  int B;
  DEV void step(int t, int b, const float (&x)[n], const float (&uu)[m], float (&o)[n]) const {
    if constexpr (std::is_same_v<Model, NoModel>) {
      size_t tb = (size_t)t * B + b;
      float Ft[n][n + m];
      ld2(Ft, F + tb * n * (n + m));
#pragma unroll
      for (int i = 0; i < n; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < n; ++j) s += Ft[i][j] * x[j];
#pragma unroll
        for (int j = 0; j < m; ++j) s += Ft[i][n + j] * uu[j];
        o[i] = s;
      }
      if (f) {
        float ft[n]; ld(ft, f + tb * n);
#pragma unroll
        for (int i = 0; i < n; ++i) o[i] += ft[i];
      }
    } else {
      md.forward(x, uu, o);
    }
  }
};

// One rollout pass with step size alpha.  Gains come from (K,k) [T,B,m,n]/[T,B,m]
// (GREC == 0) or from the fused kernel's per-lane gain records (GREC floats per
// (t,b): K, k, obj_t of the current trajectory).  Returns the new cost; if
// old_cost_out != nullptr it also returns the current trajectory's cost summed
// in time order from the records.
template <int n, int m, int GREC, class DynT>
DEV float forward_pass(const DynT& dyn, int T, int B, int b, float alpha, const float* __restrict__ x_init,
                       const float* __restrict__ C, const float* __restrict__ c, const float* __restrict__ x,
                       const float* __restrict__ u, const float* __restrict__ K, const float* __restrict__ k,
                       const float* __restrict__ grec, const Bounds& bd, const unsigned char* __restrict__ zI,
                       float* __restrict__ x_out, float* __restrict__ u_out, float* __restrict__ du_sq,
                       float* old_cost_out) {
  constexpr int d = n + m;
  float xn[n], dx[n];
  ld(xn, x_init + (size_t)b * n);
#pragma unroll
  for (int i = 0; i < n; ++i) dx[i] = 0.f;
  st(x_out + (size_t)b * n, xn);
  float cost = 0.f, oldc = 0.f;
  for (int t = 0; t < T; ++t) {
    size_t tb = (size_t)t * B + b;
    float Kt[m][n], kt[m], ut[m];
    if constexpr (GREC > 0) {
      float g[GREC];
      ld(g, grec + tb * GREC);
#pragma unroll
      for (int a = 0; a < m; ++a) {
#pragma unroll
        for (int j = 0; j < n; ++j) Kt[a][j] = g[a * n + j];
        kt[a] = g[m * n + a];
      }
      oldc += g[m * n + m];
    } else {
      ld2(Kt, K + tb * m * n);
      ld(kt, k + tb * m);
    }
    ld(ut, u + tb * m);
    float nu[m];
#pragma unroll
    for (int a = 0; a < m; ++a) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < n; ++j) s += Kt[a][j] * dx[j];
      nu[a] = (s + ut[a]) + alpha * kt[a];
      if (zI && zI[tb * m + a]) nu[a] = 0.f;
      if (bd.mode != DILQR_BOUNDS_NONE) nu[a] = eclamp(nu[a], bound_lo(bd, tb * m + a), bound_hi(bd, tb * m + a));
    }
    st(u_out + tb * m, nu);
    if (du_sq) {
#pragma unroll
      for (int a = 0; a < m; ++a) {
        float e = ut[a] - nu[a];
        du_sq[((size_t)t * m + a) * B + b] = e * e;
      }
    }
    float Ct[d][d], ct[d], tau[d];
    ld2(Ct, C + tb * d * d);
    ld(ct, c + tb * d);
#pragma unroll
    for (int i = 0; i < n; ++i) tau[i] = xn[i];
#pragma unroll
    for (int a = 0; a < m; ++a) tau[n + a] = nu[a];
    cost += quad_cost(Ct, ct, tau);
    if (t < T - 1) {
      float xnext[n], xcur[n];
      dyn.step(t, b, xn, nu, xnext);
      ld(xcur, x + (tb + B) * n);
#pragma unroll
      for (int i = 0; i < n; ++i) {
        dx[i] = xnext[i] - xcur[i];
        xn[i] = xnext[i];
      }
      st(x_out + (tb + B) * n, xn);
    }
  }
  if (old_cost_out) *old_cost_out = oldc;
  return cost;
}

// The current trajectory's cost (lqr_step_explicit.py:171), formed and summed
// exactly as the fused iteration forms it inside its backward sweep (stage
// costs as tau . (C tau) + c . tau, summed over t = T-1..0), so the fused and
// unfused pipelines take the same line-search decisions bit for bit.
template <int n, int m>
DEV float traj_cost(int T, int B, int b, const float* __restrict__ C, const float* __restrict__ c,
                    const float* __restrict__ x, const float* __restrict__ u) {
  constexpr int d = n + m;
  float cost = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    size_t tb = (size_t)t * B + b;
    float Ct[d][d], ct[d], tau[d], xt[n], ut[m], Ctau[d];
    ld2(Ct, C + tb * d * d); ld(ct, c + tb * d); ld(xt, x + tb * n); ld(ut, u + tb * m);
#pragma unroll
    for (int i = 0; i < n; ++i) tau[i] = xt[i];
#pragma unroll
    for (int a = 0; a < m; ++a) tau[n + a] = ut[a];
    cost += quad_cost(Ct, ct, tau, Ctau);
  }
  return cost;
}

template <int n, int m, class Model>
__global__ void __launch_bounds__(kBlock) k_lqr_forward(int T, int B, ModelArg<Model> theta,
                                                      const float* __restrict__ F, const float* __restrict__ f,
                                                        const float* __restrict__ x_init, const float* __restrict__ C,
                                                        const float* __restrict__ c, const float* __restrict__ x,
                                                        const float* __restrict__ u, const float* __restrict__ K,
                                                        const float* __restrict__ k, Bounds bd,
                                                        const unsigned char* __restrict__ zI, float decay, int max_ls,
                                                        float* __restrict__ x_out, float* __restrict__ u_out,
                                                        float* cost_out, float* __restrict__ du_sq,
                                                        float* __restrict__ alpha_out,
                                                        const float* old_cost_in) {
  // cost_out and old_cost_in may alias (an MPC loop passes its cost buffer as
  // both): each lane reads old_cost_in[b] before it writes cost_out[b]
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Dyn<n, m, Model> dyn;
  if constexpr (!std::is_same_v<Model, NoModel>) dyn.md.load(theta);
  dyn.F = F; dyn.f = f; dyn.B = B;
  // lqr_step_explicit.py:171, or the caller's value of the same cost (an MPC
  // loop passes what its previous line search computed for this trajectory)
  const float old_cost = old_cost_in ? old_cost_in[b] : traj_cost<n, m>(T, B, b, C, c, x, u);
  float alpha = 1.f, cost = 0.f;
  for (int ls = 0; ls < max_ls; ++ls) {
    cost = forward_pass<n, m, 0>(dyn, T, B, b, alpha, x_init, C, c, x, u, K, k, nullptr, bd, zI, x_out, u_out,
                                 ls == 0 ? du_sq : nullptr, nullptr);
    if (!(cost > old_cost) || ls == max_ls - 1) break;
    alpha *= decay;                                             // lqr_step_explicit.py:249
  }
  cost_out[b] = cost;
  if (alpha_out) alpha_out[b] = alpha;                          // 254: the last pass's alpha
}

}  // namespace dilqr
