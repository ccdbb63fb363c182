// dilqr_model_kernels.h — the per-row model kernels (dynamics, Jacobian,
// rollout, linearisation), templated on a Model that provides load(),
// forward() and jacobian().  Shared by the units that instantiate them:
// tu_models.hip (the env_dx models, theta a parameter vector), tu_mlp.hip and
// tu_mlp2.hip (the networks, a by-value descriptor, dilqr_mlp.h, dilqr_mlp2.h)
// and tu_mlp_slew.hip / tu_mlp2_slew.hip (the networks under the slew-rate
// augmentation, dilqr_ctrl_through.h).
#pragma once
#include "dilqr_common.h"

namespace dilqr {

// What a model's load() takes, as the kernels receive it: the parameter vector
// theta by default; a model with another description of itself declares
// `using Arg = ...` (passed by value as a kernel argument).
template <class Model, class = void>
struct ModelArgOf {
  using type = const float* __restrict__;
};
template <class Model>
struct ModelArgOf<Model, std::void_t<typename Model::Arg>> {
  using type = typename Model::Arg;
};
template <class Model>
using ModelArg = typename ModelArgOf<Model>::type;

// A model whose forward and Jacobian share most of their work provides
// forward_jacobian(x, u, o, D) (one pass); the others are asked for both.
template <class Model, class = void>
struct HasForwardJacobian : std::false_type {};
template <class Model>
struct HasForwardJacobian<Model, std::void_t<decltype(Model::kForwardJacobian)>> : std::true_type {};

// ============================================================ model kernels
template <class Model>
__global__ void __launch_bounds__(kBlock) k_dynamics(int N, ModelArg<Model> theta,
                                                     const float* __restrict__ x, const float* __restrict__ u,
                                                     float* __restrict__ out) {
  constexpr int n = Model::N, m = Model::M;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Model md; md.load(theta);
  float xi[n], ui[m], o[n];
  ld(xi, x + (size_t)i * n); ld(ui, u + (size_t)i * m);
  md.forward(xi, ui, o);
  st(out + (size_t)i * n, o);
}

template <class Model>
__global__ void __launch_bounds__(kBlock) k_linear_dyn(int N, ModelArg<Model> theta,
                                                       const float* __restrict__ x, const float* __restrict__ u,
                                                       float* __restrict__ Dout) {
  constexpr int n = Model::N, m = Model::M, d = n + m;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Model md; md.load(theta);
  float xi[n], ui[m], D[n][d];
  ld(xi, x + (size_t)i * n); ld(ui, u + (size_t)i * m);
  md.jacobian(xi, ui, D);
  st2(Dout + (size_t)i * n * d, D);
}

// util.get_traj (util.py:104-127)
template <class Model>
__global__ void __launch_bounds__(kBlock) k_rollout(int T, int B, ModelArg<Model> theta,
                                                    const float* __restrict__ x_init, const float* __restrict__ u,
                                                    float* __restrict__ x_out) {
  constexpr int n = Model::N, m = Model::M;
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Model md; md.load(theta);
  float xt[n];
  ld(xt, x_init + (size_t)b * n);
  st(x_out + (size_t)b * n, xt);
  for (int t = 0; t < T - 1; ++t) {
    float ut[m], xn[n];
    ld(ut, u + ((size_t)t * B + b) * m);
    md.forward(xt, ut, xn);
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = xn[i];
    st(x_out + ((size_t)(t + 1) * B + b) * n, xt);
  }
}

// MPC.linearize_dynamics ANALYTIC (mpc_explicit.py:516-546)
template <class Model>
__global__ void __launch_bounds__(kBlock) k_linearize(int T, int B, ModelArg<Model> theta,
                                                      const float* __restrict__ x, const float* __restrict__ u,
                                                      float* __restrict__ F, float* __restrict__ f) {
  constexpr int n = Model::N, m = Model::M, d = n + m;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)(T - 1) * B) return;
  Model md; md.load(theta);
  float xi[n], ui[m], D[n][d], xn[n], fo[n];
  ld(xi, x + (size_t)i * n); ld(ui, u + (size_t)i * m);
  if constexpr (HasForwardJacobian<Model>::value) {
    md.forward_jacobian(xi, ui, xn, D);
  } else {
    md.forward(xi, ui, xn);
    md.jacobian(xi, ui, D);
  }
#pragma unroll
  for (int r = 0; r < n; ++r) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < n; ++j) s += D[r][j] * xi[j];
#pragma unroll
    for (int j = 0; j < m; ++j) s += D[r][n + j] * ui[j];
    fo[r] = xn[r] - s;
  }
  st2(F + (size_t)i * n * d, D);
  st(f + (size_t)i * n, fo);
}

}  // namespace dilqr
