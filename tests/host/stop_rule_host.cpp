// Host check of the MPC stop rule's GPU-free pieces
// (differentiable-ilqr_amd/csrc/dilqr_stop_rule.h): every sequence of up to 6
// iterations over any in {0,1} x max in {0, below eps, at eps, above eps, NaN},
// for lim in 0..3 and eps in {0, 1e-3}, drives stop_rule_step the way
// mpc_decide's prologues do (the rule of iteration k-1 applied ahead of
// iteration k, the last iteration's never) and must stop at the iteration, and
// with the counter, of the reference's loop written out below.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I differentiable-ilqr_amd/csrc tests/host/stop_rule_host.cpp -o stop_rule_host
// Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "dilqr_stop_rule.h"

using namespace dilqr;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

constexpr int kMaxIters = 6;

struct Seq {
  int iters;                  // the solve's iteration budget (lqr_iter)
  int any[kMaxIters];         // some problem took the best-iterate branch in iteration k
  float mx[kMaxIters];        // iteration k's largest row norm
  float eps;
  int lim;
};

struct Outcome {
  int ran, stopped, n_not_improved;
};

// mpc_explicit.py:264, 279, 297-299: count up, reset on any improvement after
// the first iteration, stop when max < eps or the count exceeds lim; the rule
// of the last iteration is never applied
static Outcome reference(const Seq& q) {
  Outcome r{0, 0, 0};
  for (int k = 0; k < q.iters; ++k) {
    r.ran = k + 1;
    if (k == q.iters - 1) break;
    r.n_not_improved += 1;
    if (k > 0 && q.any[k]) r.n_not_improved = 0;
    if (q.mx[k] < q.eps || r.n_not_improved > q.lim) {
      r.stopped = 1;
      break;
    }
  }
  return r;
}

// the prologue of iteration k >= 1 applies the rule of iteration k-1; "any" is
// fed only by iterations after the first (S.improved is 1, not 2, in iteration 0)
static Outcome stepped(const Seq& q) {
  Outcome r{0, 0, 0};
  for (int k = 0; k < q.iters; ++k) {
    if (k > 0) {
      const bool any = k - 1 > 0 && q.any[k - 1] != 0;
      const StopState st = stop_rule_step(r.n_not_improved, any, du_below(f32_bits(q.mx[k - 1]), q.eps), q.lim);
      r.n_not_improved = st.n_not_improved;
      r.stopped = st.stopped;
      if (r.stopped) break;
    }
    r.ran = k + 1;
  }
  return r;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  long cases = 0, stops = 0;
  for (float eps : {0.f, 1e-3f}) {
    const float vals[5] = {0.f, 0.5e-3f, eps, 2e-3f, nan};
    // mpc_decide's ballot: the max (as uints) is below eps iff every term is
    for (float x : vals)
      for (float y : vals) {
        const unsigned bx = f32_bits(x), by = f32_bits(y);
        CHECK(du_below(bx > by ? bx : by, eps) == (du_below(bx, eps) && du_below(by, eps)));
        CHECK(du_below(bx, eps) == (x < eps));
      }
    for (int lim = 0; lim <= 3; ++lim)
      for (int iters = 1; iters <= kMaxIters; ++iters) {
        long total = 1;
        for (int k = 0; k < iters; ++k) total *= 10;
        for (long code = 0; code < total; ++code) {
          Seq q{};
          q.iters = iters; q.eps = eps; q.lim = lim;
          long c = code;
          for (int k = 0; k < iters; ++k, c /= 10) {
            q.any[k] = (int)(c % 10) / 5;
            q.mx[k] = vals[(c % 10) % 5];
          }
          const Outcome want = reference(q), got = stepped(q);
          CHECK(got.ran == want.ran && got.stopped == want.stopped && got.n_not_improved == want.n_not_improved);
          stops += want.stopped;
          ++cases;
        }
      }
  }
  // the best-iterate test: iteration 0 always, else cost <= best + eps (a NaN never)
  CHECK(mpc_takes_best(true, nan, 0.f, 0.f) && mpc_takes_best(true, 5.f, 1.f, 0.f));
  CHECK(mpc_takes_best(false, 1.f, 1.f, 0.f) && mpc_takes_best(false, 1.05f, 1.f, 0.1f));
  CHECK(!mpc_takes_best(false, 1.5f, 1.f, 0.1f) && !mpc_takes_best(false, nan, 1.f, 0.1f) &&
        !mpc_takes_best(false, 1.f, nan, 0.1f));
  std::printf("ok: %ld sequences, %ld stopped early\n", cases, stops);
  return 0;
}
