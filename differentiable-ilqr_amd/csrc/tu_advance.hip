// tu_advance.hip — the step between two solves of a closed-loop (receding-
// horizon) MPC episode, il_env.py:134-140: apply the plan's first control to
// the plant, log the step, shift the plan into the next solve's warm start.
#include "dilqr_common.h"
#include "dilqr_warm_start.h"

namespace dilqr {

// One lane per problem.  The plant step is k_rollout's (dilqr_model_kernels.h):
// the same load(), the same forward() on the same operands in the same order,
// so x_{s+1} carries the bits of dilqr_rollout_f32's second row.  The model
// clamps the control inside forward() as the reference's dx(x, u) does; u_log
// keeps the control as the solver gave it (nominal_actions[0]).
template <class Model>
__global__ void __launch_bounds__(kBlock) k_mpc_advance(int T, int B, const float* __restrict__ theta,
                                                        const float* __restrict__ u_plan, float* x_cur,
                                                        float* __restrict__ u_warm, int warm_mode,
                                                        const float* __restrict__ C, const float* __restrict__ c,
                                                        float* x_next_log, float* __restrict__ u_log,
                                                        float* __restrict__ cost_log) {
  constexpr int n = Model::N, m = Model::M, d = n + m;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  Model md; md.load(theta);
  float xt[n], ut[m], xn[n];
  ld(xt, x_cur + (size_t)b * n);
  ld(ut, u_plan + (size_t)b * m);
  if (cost_log) {
    // 0.5 tau^T C_0 tau + c_0^T tau at (x_s, u_s), row by row from the t = 0 record
    const float* Cb = C + (size_t)b * d * d;
    const float* cb = c + (size_t)b * d;
    float tau[d];
#pragma unroll
    for (int i = 0; i < n; ++i) tau[i] = xt[i];
#pragma unroll
    for (int i = 0; i < m; ++i) tau[n + i] = ut[i];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < d; ++i) {
      float r = 0.f;
#pragma unroll
      for (int j = 0; j < d; ++j) r += Cb[i * d + j] * tau[j];
      s += tau[i] * (0.5f * r + cb[i]);
    }
    cost_log[b] = s;
  }
  md.forward(xt, ut, xn);
  st(x_cur + (size_t)b * n, xn);
  // the log rows are rows of the caller's [steps+1,B,n] and [steps,B,m] arrays:
  // 4-byte aligned only, scalar stores
#pragma unroll
  for (int i = 0; i < n; ++i) x_next_log[(size_t)b * n + i] = xn[i];
#pragma unroll
  for (int i = 0; i < m; ++i) u_log[(size_t)b * m + i] = ut[i];
  for (int t = 0; t < T; ++t) {
    const int src = warm_source(warm_mode, T, t);
    float w[m];
    if (src == kWarmZero) {
#pragma unroll
      for (int i = 0; i < m; ++i) w[i] = 0.f;
    } else {
      ld(w, u_plan + ((size_t)src * B + b) * m);
    }
    st(u_warm + ((size_t)t * B + b) * m, w);
  }
}

namespace {
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool overlap(const float* a, const float* b, size_t floats) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  const uintptr_t bytes = floats * sizeof(float);
  return pa < pb + bytes && pb < pa + bytes;
}
}  // namespace

}  // namespace dilqr

using namespace dilqr;

extern "C" {

int dilqr_mpc_advance_f32(int model, int T, int B, const float* theta_plant, const float* u_plan, float* x_cur,
                          float* u_warm, int warm_mode, const float* C, const float* c, float* x_next_log,
                          float* u_log, float* cost_log, void* stream) {
  if (T < 1 || B < 0 || !theta_plant || !u_plan || !x_cur || !u_warm || !x_next_log || !u_log) return DILQR_E_ARG;
  if (cost_log && (!C || !c)) return DILQR_E_ARG;
  if (!warm_mode_ok(warm_mode, T)) return DILQR_E_ARG;
  if (!al16(u_plan) || !al16(x_cur) || !al16(u_warm) || !al16(C) || !al16(c)) return DILQR_E_ARG;
  if (!al4(x_next_log) || !al4(u_log) || !al4(cost_log)) return DILQR_E_ARG;
  const int m = dilqr_model_num_ctrl(model);
  if (m < 0) return DILQR_E_SHAPE;          // no forward: the MLP ids, LinDx, an unknown id
  if (overlap(u_warm, u_plan, (size_t)T * B * m)) return DILQR_E_ARG;
  if (B == 0) return 0;
  MODEL_SWITCH(model, (k_mpc_advance<MD><<<grid_for(B), kBlock, 0, S(stream)>>>(
                          T, B, theta_plant, u_plan, x_cur, u_warm, warm_mode, C, c, x_next_log, u_log, cost_log)));
  return launched();
}

}  // extern "C"
