// tu_mlp2_implicit.hip — the DiLQR implicit backward with the two-hidden-layer
// network as the dynamics (dilqr_mlp2.h): the kernel of dilqr_mlp_implicit.h on
// the Mlp2 model.  Everything is as in tu_mlp_implicit.hip (y, w, dlam, dC, dc,
// dF, df, dx_init, the three passes, the workspace) but F_t and M_t: with
//   z1 = W1 tau + b1, z2 = W2 act(z1) + b2, g = act'(z), c = act''(z),
//   P = W2 diag(g1) W1, s = W3^T lam_{t+1}, v = W2^T (s o g2),
//   F_t = W3 diag(g2) P (+ I on the state block),
//   M_t = P^T diag(s o c2) P + W1^T diag(v o c1) W1;  relu: M = 0
// (Mlp2::jacobian_lag).  The gradient into the weights is
// dilqr_mlp2_linearize_vjp_f32 on (dF, df).
//
// LDS per one-wave workgroup, all dynamic: the first layer's activations
// (256 H1 bytes), then one region that holds the column v during a walk with M
// (256 H1 bytes, sigmoid only) and the staging area of the wave's records
// between the walks (64 d^2 floats, 16 KiB at d = 8): v is dead there, and each
// walk zeroes it first.  At [64, 64] that is 32 KiB, so four workgroups share a
// CU's 160 KiB, one per SIMD (the two side by side, 41 KiB at d = 6, left room
// for three).  The first width is bounded (DILQR_MLP2_IMPLICIT_MAX_HIDDEN1 =
// 96): 48 KiB of the 64 KiB a launch gets without raising the function's limit.
#include "dilqr_mlp2.h"
#include "dilqr_mlp_abi.h"
#include "dilqr_mlp_implicit.h"

namespace dilqr {

constexpr int kImplicit2MaxHidden1 = DILQR_MLP2_IMPLICIT_MAX_HIDDEN1;
// a1 with v, or with the largest staging area (d = 8)
static_assert(2 * sizeof(float) * 64 * kImplicit2MaxHidden1 <= 65536 &&
              sizeof(float) * 64 * kImplicit2MaxHidden1 + sizeof(float) * kBlock * 8 * 8 <= 65536,
              "a1 and v or the staging area in 64 KiB of LDS");
#define X(N_, M_) static_assert(N_ + M_ <= 8, "the staging area is bounded for d <= 8");
DILQR_FOR_EACH_SHAPE(X)
#undef X

}  // namespace dilqr

using namespace dilqr;

extern "C" {

int dilqr_mlp2_implicit_backward_f32(int n, int m, int T, int B, dilqr_mlp2 mlp, const float* C, const float* c,
                                     const float* x, const float* u, const float* dl_dx, const float* dl_du,
                                     dilqr_bounds bounds, float* ws, float* dx_init, float* dC, float* dc, float* dF,
                                     float* df, void* stream) {
  if (T < 1 || B < 0) return DILQR_E_ARG;
  if (!C || !c || !x || !u || !dl_dx || !dl_du || !ws || !dx_init || !dC || !dc) return DILQR_E_ARG;
  if ((dF == nullptr) != (df == nullptr)) return DILQR_E_ARG;
  const void* ps[] = {C, c, x, u, dl_dx, dl_du, ws, dx_init, dC, dc, dF, df};
  for (const void* q : ps) if (!al16(q)) return DILQR_E_ARG;
  if (bad_bounds(bounds)) return DILQR_E_ARG;
  if (int rc = TwoHidden::check(n, m, mlp)) return rc;
  if (mlp.n_hidden1 > kImplicit2MaxHidden1) return DILQR_E_SHAPE;
  if (B == 0) return 0;
  const Mlp2Arg a = TwoHidden::arg(mlp);
  const Bounds bd = mkb(bounds);
  const size_t lds = mlp2_implicit_lds_bytes(a.H1, n + m, mlp.activation == DILQR_MLP_SIGMOID);
  return mlp_dispatch<TwoHidden>(n, m, mlp.activation, [&](auto tag) {
    using MD = typename decltype(tag)::type;
    k_mlp_implicit_backward<MD><<<grid_for(B), kBlock, lds, S(stream)>>>(T, B, a, C, c, x, u, dl_dx, dl_du, bd, ws,
                                                                        dx_init, dC, dc, dF, df);
  });
}

}  // extern "C"
