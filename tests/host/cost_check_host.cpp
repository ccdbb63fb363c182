// Host check of the speculative cost route's GPU-free pieces
// (differentiable-ilqr_amd/csrc/dilqr_cost_check.h): the schedule hands out
// every record 1 .. T-2 exactly once, in order, loads before folds, for every
// T in 1..40 x iters in 1..12 x spread in 0..12, both tick densities and several
// waves (each starts at its own offset into the gap between two events), with
// all events inside the first min(spread, iters) iterations and the drain
// taking exactly the rest; the record test sees any single changed word.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I differentiable-ilqr_amd/csrc tests/host/cost_check_host.cpp -o cost_check_host
// Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "dilqr_cost_check.h"

using dilqr::SpecSchedule;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

// what CostCheck::event / drain do with the schedule, on counters
struct Sim {
  SpecSchedule s;
  std::vector<int> loads, folds;   // per record
  int buffered = 0;                // the record in the buffer, 0: none
  int order = 0;                   // the last record folded
  explicit Sim(int T) : loads(T + 2, 0), folds(T + 2, 0) {}
  void fold() {
    CHECK(buffered == order + 1);
    ++folds[buffered];
    order = buffered;
    buffered = 0;
  }
  void load(int t) {
    CHECK(buffered == 0 && t >= 1 && t <= s.last);
    ++loads[t];
    buffered = t;
  }
  void event() {
    if (s.take_fold()) fold();
    if (const int t = s.take_load()) load(t);
  }
  void drain() {
    if (s.take_fold()) fold();
    for (int t = s.take_load(); t; t = s.take_load()) {
      load(t);
      CHECK(s.take_fold());
      fold();
    }
  }
};

static long check_schedule(int T, int iters, int spread, int tpi_mult, int extra_ticks, unsigned wave) {
  const int tpi = tpi_mult * T;                    // ticks the schedule plans per iteration
  Sim m(T);
  m.s.init(T, iters, spread, tpi, wave);
  const int R = T > 2 ? T - 2 : 0;
  const int its = spread < iters ? spread : iters;
  long events = 0, tick = 0, last_event = -1;
  int done_after = -1;                             // the iteration after which every record was folded
  for (int it = 0; it < iters; ++it) {
    for (int k = 0; k < tpi + extra_ticks; ++k, ++tick)   // (a longer line search: more ticks than planned)
      if (m.s.tick()) {
        m.event();
        ++events;
        if (last_event < 0) {
          const int gap = its * tpi / (R + 1);     // the first event: at the wave's offset into the gap
          CHECK(tick == SpecSchedule::stagger(wave, gap) && tick < gap);
        } else {                                   // ... and the rest follow evenly
          const long gap = tick - last_event, even = (long)its * tpi / (R + 1);
          CHECK(gap == even || gap == even + 1);
        }
        last_event = tick;
      }
    if (done_after < 0 && m.s.done()) done_after = it;
  }
  if (its > 0 && R > 0) {
    CHECK(m.s.done());                             // spread over the iterations: nothing left to drain
    CHECK(done_after >= 0 && done_after < its);
    CHECK(events == R + 1);
  }
  const int before = m.order;
  m.drain();
  CHECK(m.s.done() && m.buffered == 0 && m.order == R);
  if (its == 0) CHECK(before == 0);                // spread 0: the drain takes every record
  for (int t = 0; t < (int)m.loads.size(); ++t) {
    const int want = t >= 1 && t <= T - 2 ? 1 : 0;
    CHECK(m.loads[t] == want && m.folds[t] == want);
  }
  CHECK(!m.s.tick() && !m.s.take_fold() && m.s.take_load() == 0);   // and stays done
  return events;
}

template <int d>
static void check_record_diff() {
  float C[d][d], c[d], dg[d], cc[d];
  for (int i = 0; i < d; ++i) {
    for (int j = 0; j < d; ++j) C[i][j] = 0.f;
    dg[i] = C[i][i] = 0.25f * (float)(i + 1);
    cc[i] = c[i] = i == 2 ? 0.f : -0.5f * (float)i;
  }
  CHECK(dilqr::cost_record_diff(C, c, dg, cc) == 0u);
  const float poison[] = {1e-6f, -0.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::denorm_min(),
                          -std::numeric_limits<float>::infinity()};
  float* words[2] = {&C[0][0], &c[0]};
  const int counts[2] = {d * d, d};
  for (int a = 0; a < 2; ++a)
    for (int k = 0; k < counts[a]; ++k) {
      const float keep = words[a][k];
      for (float p : poison) {
        if (std::memcmp(&p, &keep, sizeof p) == 0) continue;
        words[a][k] = p;
        CHECK(dilqr::cost_record_diff(C, c, dg, cc) != 0u);
      }
      words[a][k] = std::nextafter(keep, 1e30f);   // one ulp
      CHECK(dilqr::cost_record_diff(C, c, dg, cc) != 0u);
      words[a][k] = keep;
      CHECK(dilqr::cost_record_diff(C, c, dg, cc) == 0u);
    }
  // a NaN guess equals itself bit for bit (the test is on bits, not values)
  dg[1] = C[1][1] = std::numeric_limits<float>::quiet_NaN();
  CHECK(dilqr::cost_record_diff(C, c, dg, cc) == 0u);
}

int main() {
  long cases = 0, events = 0;
  for (int T = 1; T <= 40; ++T)
    for (int iters = 1; iters <= 12; ++iters)
      for (int spread = 0; spread <= 12; ++spread)
        for (int mult = 1; mult <= 2; ++mult)
          for (int extra = 0; extra <= 3; extra += 3)
            for (unsigned wave : {0u, 1u, 2u, 7u, 255u, 1023u, 65535u}) {
              events += check_schedule(T, iters, spread, mult, extra, wave);
              ++cases;
            }
  check_record_diff<4>();
  check_record_diff<6>();
  std::printf("ok: %ld schedules, %ld events\n", cases, events);
  return 0;
}
