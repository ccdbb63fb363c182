// dilqr_mlp_fused.h — the fused iLQR iteration (dilqr_fused.h ilqr_problem) on
// the one-hidden-layer network of dilqr_mlp.h, on the unfused MPC loop's plain
// buffers: one iteration per launch for any batch (k_mlp_ilqr_iterate), and a
// whole stop-rule solve in one launch for a batch one workgroup holds
// (k_mlp_mpc_solve_small).  Instantiated per (n, m) in tu_mpc_mlp_<n><m>.hip;
// the entry points that call the launchers are in tu_mpc_mlp.hip.
//
// Both kernels run ilqr_problem<Mlp, BM, TRAJ_AOS, false, CostFull, PREV>: the
// Jacobian walk, RiccatiState::step, quad_cost and the pair line search the
// unfused kernels (k_linearize, the Riccati sweep, k_lqr_forward) are built
// from, so an iteration gives the bits of those three launches.
#pragma once
#include "dilqr_fused.h"
#include "dilqr_mlp.h"

namespace dilqr {

// floats per (t, b) ahead of candidate B's trajectory in the workspace: the
// gain record rounded up to whole float4s (ops.grec_floats), so candidate B's
// x records stay 16-byte aligned for every T * B
constexpr int mlp_grec_floats(int n, int m) { return (m * n + m + 1 + 3) / 4 * 4; }

// the shapes the one-launch solve is built for: (6, 2)'s fused iteration alone
// takes 256 + 236 of the 512 registers a lane can have, and the solve's loop
// state around it spilled (132-276 B of scratch per lane); it keeps the
// per-iteration launch
constexpr bool mlp_small_ok(int n, int m) { return !(n == 6 && m == 2); }

struct MlpIterArgs {
  int T, B;
  MlpArg mlp;
  const float *x_init, *C, *c, *x, *u;
  Bounds bd;
  float decay;
  int max_ls;
  float *ws, *x_out, *u_out, *cost, *du_sq, *alpha;
  const float* old_cost;
  const dilqr_mpc_ctrl* ctrl;
  hipStream_t stream;
};

// the plain buffers of the unfused loop (ops.MPCWorkspace)
struct MlpSolveBufs {
  float *xa, *ua, *xb, *ub, *ws, *cost, *alpha, *du_sq, *fdn, *best_x, *best_u, *best_cost, *best_du;
  dilqr_mpc_ctrl* ctrl;
};

struct MlpSolveArgs {
  int T, B;
  MlpArg mlp;
  const float *x_init, *u_init, *C, *c;
  Bounds bd;
  float decay;
  int max_ls, iters;
  float best_cost_eps, eps;
  int lim;
  MlpSolveBufs S;
  hipStream_t stream;
};

// One fused iteration of problem b from (x, u) into (x_out, u_out): candidate
// B of the line search rolls out into the workspace tail and is copied over
// the outputs when it wins (as k_ilqr_iterate).
template <class Model, int BM, bool PREV>
DEV void mlp_iterate_lane(int T, int B, int b, const Model& md, const float* __restrict__ x_init,
                          const float* __restrict__ C, const float* __restrict__ c, const float* __restrict__ x,
                          const float* __restrict__ u, const Bounds& bd, float decay, int max_ls,
                          float* __restrict__ ws, float* __restrict__ x_out, float* __restrict__ u_out,
                          float* __restrict__ du_sq, float prev_cost, float& cost, float& alpha) {
  constexpr int n = Model::N, m = Model::M;
  static_assert(m % 2 != 0 || n % 2 == 0, "candidate B's u records follow its x records: float2 alignment");
  float* xb = ws + (size_t)T * B * mlp_grec_floats(n, m);
  float* ub = xb + (size_t)T * B * n;
  const int win = ilqr_problem<Model, BM, TRAJ_AOS, false, CostFull<n + m>, PREV>(
      T, B, b, md, x_init, CostFull<n + m>{C, c}, nullptr, nullptr, x, u, bd, decay, max_ls, GainRecs{ws, B, b},
      x_out, u_out, xb, ub, du_sq, cost, alpha, false, prev_cost);
  if (win) copy_traj_aos<n, m>(x_out, u_out, xb, ub, T, B, b);
}

// cost_out and old_cost may alias (an MPC loop passes its cost buffer as both):
// each lane reads old_cost[b] before it writes cost_out[b]
template <class Model, int BM, bool PREV>
__global__ void __launch_bounds__(kBlock) k_mlp_ilqr_iterate(int T, int B, MlpArg a, const float* __restrict__ x_init,
                                                             const float* __restrict__ C, const float* __restrict__ c,
                                                             const float* __restrict__ x, const float* __restrict__ u,
                                                             Bounds bd, float decay, int max_ls, float* __restrict__ ws,
                                                             float* __restrict__ x_out, float* __restrict__ u_out,
                                                             float* cost_out, float* __restrict__ du_sq,
                                                             float* __restrict__ alpha_out, const float* old_cost,
                                                             const dilqr_mpc_ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stopped) return;
  Model md; md.load(a);
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float prev = 0.f;
  if constexpr (PREV) prev = old_cost[b];
  float cost, alpha;
  mlp_iterate_lane<Model, BM, PREV>(T, B, b, md, x_init, C, c, x, u, bd, decay, max_ls, ws, x_out, u_out, du_sq, prev,
                                    cost, alpha);
  cost_out[b] = cost;
  alpha_out[b] = alpha;
}

// ---------------- a whole stop-rule solve in ONE launch, B <= kSmallMax
// The unfused loop of ops.mpc_solve_unfused in one workgroup: each lane rolls
// u_init out (k_rollout's arithmetic), then per iteration runs the fused
// iteration (0 sums the old cost, later ones take the previous line search's),
// and the workgroup does what k_mpc_best + k_mpc_control do — the quirk row b
// summed in the same order after a barrier (a row mixes other waves'
// problems), the best test and copy, the max of the row norms and "any
// improved" reduced across the workgroup, then the counters and the stop rule,
// after every iteration, the last one included.  A second barrier keeps the
// next iteration's du_sq stores behind every lane's read of its row.  The two
// trajectory buffers swap every iteration.
// (The row sum and the best copy are written out here: calling quirk_row_norm
// or copy_traj_aos moved this kernel's listing.)
template <class Model, int BM>
__global__ void __launch_bounds__(kSmallMax) k_mlp_mpc_solve_small(int T, int B, MlpArg a,
                                                                   const float* __restrict__ x_init,
                                                                   const float* __restrict__ u_init,
                                                                   const float* __restrict__ C,
                                                                   const float* __restrict__ c, Bounds bd, float decay,
                                                                   int max_ls, int iters, float best_cost_eps,
                                                                   float eps, int not_improved_lim, MlpSolveBufs S) {
  constexpr int n = Model::N, m = Model::M;
  __shared__ unsigned red_max[kSmallMax / 64];
  __shared__ int red_any[kSmallMax / 64];
  const int b = threadIdx.x;
  const bool act = b < B;
  const int nw = (int)(blockDim.x + 63) / 64, w = b >> 6;
  const int TM = T * m;
  Model md; md.load(a);
  float *xc = S.xa, *uc = S.ua, *xo = S.xb, *uo = S.ub;
  if (act) {                                               // util.get_traj (k_rollout), u_init or zeros
    float xt[n];
    ld(xt, x_init + (size_t)b * n);
    st(xc + (size_t)b * n, xt);
    for (int t = 0; t < T; ++t) {
      const size_t tb = (size_t)t * B + b;
      float ut[m], xn[n];
      if (u_init) {
        ld(ut, u_init + tb * m);
      } else {
#pragma unroll
        for (int k = 0; k < m; ++k) ut[k] = 0.f;
      }
      st(uc + tb * m, ut);
      if (t < T - 1) {
        md.forward(xt, ut, xn);
#pragma unroll
        for (int i = 0; i < n; ++i) xt[i] = xn[i];
        st(xc + (tb + B) * n, xt);
      }
    }
  }
  float cost = 0.f, alpha = 0.f, best_cost = 0.f;
  int it = 0, n_not_improved = 0, stopped = 0;
  // (iteration 0 ahead of the loop, so the loop body holds one instantiation of
  // the iteration: with both inside it, what the compiler hoisted out of the
  // loop for either stayed live through the other and (6, 2) spilled)
  if (act) {
    mlp_iterate_lane<Model, BM, false>(T, B, b, md, x_init, C, c, xc, uc, bd, decay, max_ls, S.ws, xo, uo, S.du_sq,
                                       0.f, cost, alpha);
    S.cost[b] = cost;
    S.alpha[b] = alpha;
  }
  for (;;) {
    const bool first = it == 0;
    __syncthreads();                                       // every lane's du rows of this iteration are stored
    unsigned mx = 0u;
    int any = 0;
    if (act) {                                             // k_mpc_best, problem b
      float s = 0.f;                                       // quirk_row_norm
      const float* p = S.du_sq + (size_t)b * TM;
      for (int i = 0; i < TM; ++i) s += p[i];
      const float fdn = sqrtf(s);
      S.fdn[b] = fdn;
      mx = __float_as_uint(fdn);
      bool take = first;
      if (!take && cost <= best_cost + best_cost_eps) {
        take = true;
        any = 1;
      }
      if (take) {
        best_cost = cost;
        S.best_cost[b] = cost;
        S.best_du[b] = fdn;
        for (int t = 0; t < T; ++t) {                       // copy_traj_aos
          const size_t tb = (size_t)t * B + b;
          float xt[n], ut[m];
          ld(xt, xo + tb * n); ld(ut, uo + tb * m);
          st(S.best_x + tb * n, xt); st(S.best_u + tb * m, ut);
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = __shfl_xor(mx, off, 64);
      mx = o > mx ? o : mx;
      any |= __shfl_xor(any, off, 64);
    }
    if ((b & 63) == 0) { red_max[w] = mx; red_any[w] = any; }
    __syncthreads();                                       // (also: every lane has read its row)
    mx = 0u;
    any = 0;
    for (int i = 0; i < nw; ++i) { mx = red_max[i] > mx ? red_max[i] : mx; any |= red_any[i]; }
    it += 1;                                               // k_mpc_control
    n_not_improved += 1;
    if (!first && any) n_not_improved = 0;
    if (__uint_as_float(mx) < eps || n_not_improved > not_improved_lim) stopped = 1;
    if (stopped || it == iters) break;
    float* tx = xc; xc = xo; xo = tx;
    float* tu = uc; uc = uo; uo = tu;
    if (act) {
      mlp_iterate_lane<Model, BM, true>(T, B, b, md, x_init, C, c, xc, uc, bd, decay, max_ls, S.ws, xo, uo, S.du_sq,
                                        cost, cost, alpha);
      S.cost[b] = cost;
      S.alpha[b] = alpha;
    }
  }
  if (b == 0) {                                            // the control word k_mpc_control leaves
    dilqr_mpc_ctrl o = {};
    o.iter = it;
    o.stopped = stopped;
    o.n_not_improved = n_not_improved;
    *S.ctrl = o;
  }
}

// ---------------------------------------------------------------- launchers
template <int N_, int M_>
int launch_mlp_ilqr_iterate(const MlpIterArgs& a, int activation) {
  with_flag(activation == DILQR_MLP_SIGMOID, [&](auto sig) {
    using MD = Mlp<N_, M_, decltype(sig)::value ? DILQR_MLP_SIGMOID : DILQR_MLP_RELU>;
    with_bounds_mode(a.bd.mode, [&](auto bm) {
      with_flag(a.old_cost != nullptr, [&](auto prev) {
        k_mlp_ilqr_iterate<MD, decltype(bm)::value, decltype(prev)::value><<<grid_for(a.B), kBlock, 0, a.stream>>>(
            a.T, a.B, a.mlp, a.x_init, a.C, a.c, a.x, a.u, a.bd, a.decay, a.max_ls, a.ws, a.x_out, a.u_out, a.cost,
            a.du_sq, a.alpha, a.old_cost, a.ctrl);
      });
    });
  });
  return launched();
}

template <int N_, int M_>
int launch_mlp_mpc_solve_small(const MlpSolveArgs& a, int activation) {
  if (a.B > kSmallMax) return DILQR_E_SHAPE;
  if constexpr (!mlp_small_ok(N_, M_)) {
    return DILQR_E_SHAPE;
  } else {
    const int threads = (a.B + 63) / 64 * 64;
    with_flag(activation == DILQR_MLP_SIGMOID, [&](auto sig) {
      using MD = Mlp<N_, M_, decltype(sig)::value ? DILQR_MLP_SIGMOID : DILQR_MLP_RELU>;
      with_bounds_mode(a.bd.mode, [&](auto bm) {
        k_mlp_mpc_solve_small<MD, decltype(bm)::value><<<1, threads, 0, a.stream>>>(
            a.T, a.B, a.mlp, a.x_init, a.u_init, a.C, a.c, a.bd, a.decay, a.max_ls, a.iters, a.best_cost_eps, a.eps,
            a.lim, a.S);
      });
    });
    return launched();
  }
}

// one unit per (n, m) defines its pair (DILQR_MLP_FUSED_UNIT in the unit)
#define X(N_, M_)                                                                \
  int launch_mlp_ilqr_iterate_##N_##_##M_(const MlpIterArgs& a, int activation); \
  int launch_mlp_mpc_solve_small_##N_##_##M_(const MlpSolveArgs& a, int activation);
DILQR_FOR_EACH_SHAPE(X)
#undef X

#define DILQR_MLP_FUSED_UNIT(N_, M_)                                                                     \
  namespace dilqr {                                                                                      \
  int launch_mlp_ilqr_iterate_##N_##_##M_(const MlpIterArgs& a, int activation) {                        \
    return launch_mlp_ilqr_iterate<N_, M_>(a, activation);                                               \
  }                                                                                                      \
  int launch_mlp_mpc_solve_small_##N_##_##M_(const MlpSolveArgs& a, int activation) {                    \
    return launch_mlp_mpc_solve_small<N_, M_>(a, activation);                                            \
  }                                                                                                      \
  }

}  // namespace dilqr
