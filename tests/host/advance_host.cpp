// Host check of the closed-loop advance step's GPU-free piece
// (differentiable-ilqr_amd/csrc/dilqr_warm_start.h): which row of a solve's
// plan feeds row t of the next solve's u_init, for the three warm-start modes
// at T = 3, 4, 9 against the tables written out below (the reference's rule is
// il_env.py:139-140: u_init = cat(u[1:], 0), then u_init[-2] = u_init[-3]), and
// the modes and horizons the entry point refuses.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I differentiable-ilqr_amd/csrc tests/host/advance_host.cpp -o advance_host
// Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dilqr_warm_start.h"

using namespace dilqr;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

struct Row {
  int mode, T;
  std::vector<int> src;   // per t: the row of the plan, -1 = zero
};

// the reference's two statements on a plan whose row t holds the number t
static std::vector<int> reference_rule(int T) {
  std::vector<int> w;
  for (int t = 1; t < T; ++t) w.push_back(t);   // u[1:]
  w.push_back(-1);                              // cat(., zeros(1))
  w[T - 2] = w[T - 3];                          // u_init[-2] = u_init[-3]
  return w;
}

int main() {
  const Row table[] = {
      {DILQR_WARM_REFERENCE, 3, {1, 1, -1}},
      {DILQR_WARM_REFERENCE, 4, {1, 2, 2, -1}},
      {DILQR_WARM_REFERENCE, 9, {1, 2, 3, 4, 5, 6, 7, 7, -1}},
      {DILQR_WARM_SHIFT, 3, {1, 2, -1}},
      {DILQR_WARM_SHIFT, 4, {1, 2, 3, -1}},
      {DILQR_WARM_SHIFT, 9, {1, 2, 3, 4, 5, 6, 7, 8, -1}},
      {DILQR_WARM_COLD, 3, {-1, -1, -1}},
      {DILQR_WARM_COLD, 4, {-1, -1, -1, -1}},
      {DILQR_WARM_COLD, 9, {-1, -1, -1, -1, -1, -1, -1, -1, -1}},
  };
  long rows = 0;
  for (const Row& r : table) {
    CHECK((int)r.src.size() == r.T);
    CHECK(warm_mode_ok(r.mode, r.T));
    for (int t = 0; t < r.T; ++t) {
      const int s = warm_source(r.mode, r.T, t);
      CHECK(s == r.src[t]);
      CHECK(s == kWarmZero || (s >= 0 && s < r.T));     // never outside the plan
      ++rows;
    }
    if (r.mode == DILQR_WARM_REFERENCE) CHECK(r.src == reference_rule(r.T));
  }
  // every horizon the modes take stays inside the plan
  for (int mode : {DILQR_WARM_REFERENCE, DILQR_WARM_SHIFT, DILQR_WARM_COLD})
    for (int T = 1; T <= 40; ++T) {
      if (!warm_mode_ok(mode, T)) continue;
      for (int t = 0; t < T; ++t) {
        const int s = warm_source(mode, T, t);
        CHECK(s == kWarmZero || (s >= 0 && s < T));
      }
      CHECK(warm_source(mode, T, T - 1) == kWarmZero);
    }
  // refused: the reference's rule below T = 3, an unknown mode, an empty horizon
  CHECK(!warm_mode_ok(DILQR_WARM_REFERENCE, 2) && !warm_mode_ok(DILQR_WARM_REFERENCE, 1));
  CHECK(warm_mode_ok(DILQR_WARM_REFERENCE, 3));
  CHECK(warm_mode_ok(DILQR_WARM_SHIFT, 2) && warm_mode_ok(DILQR_WARM_SHIFT, 1) && warm_mode_ok(DILQR_WARM_COLD, 1));
  CHECK(!warm_mode_ok(3, 5) && !warm_mode_ok(-1, 5));
  CHECK(!warm_mode_ok(DILQR_WARM_SHIFT, 0) && !warm_mode_ok(DILQR_WARM_COLD, 0));
  std::printf("ok: %ld rows\n", rows);
  return 0;
}
