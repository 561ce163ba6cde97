// Host self-test of the fast round's status ladder and reliability arithmetic (svoc/verdict.hpp: round_verdict,
// RelF32, RelF32Rcp, RelF64, rel_divisor -- the code the five fast kernels and the CPU twin call) against tables
// written out here.  Stand-alone (its own main), built by tests/test_verdict_host.py with the address and
// undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <limits>

#include "svoc/verdict.hpp"

using namespace svoc;

static int g_fail = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      if (++g_fail <= 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                             \
  } while (0)

static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

// ---- the ladder alone: reliabilities placed by a stub arithmetic that counts its calls
struct Placed {
  float r1, r2;
  mutable int calls1 = 0, calls2 = 0;
  float rel1(double) const { ++calls1; return r1; }
  float rel2(double) const { ++calls2; return r2; }
};

// status by [legacy][R][rel1 inside][rel2 inside], R = 0 .. 5
//   6 RELIABILITY_INTERVAL, 8 USIZE_UNDERFLOW, 5 INDEX_OOB, 33 TOO_FEW_RELIABLE, 0 OK
static const int kLadder[2][6][2][2] = {
    {   // the contract
        {{6, 6}, {8, 8}},
        {{6, 6}, {5, 5}},
        {{6, 6}, {6, 33}},
        {{6, 6}, {6, 33}},
        {{6, 6}, {6, 0}},
        {{6, 6}, {6, 0}},
    },
    {   // legacy: no moments, so no fewest-reliable rung
        {{6, 6}, {8, 8}},
        {{6, 6}, {5, 5}},
        {{6, 6}, {6, 0}},
        {{6, 6}, {6, 0}},
        {{6, 6}, {6, 0}},
        {{6, 6}, {6, 0}},
    },
};

static void ladder_paths() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // just inside, on and just outside 0 and 1; NaN and the infinities
  const struct { float v; int inside; } edge[] = {
      {std::nextafterf(0.f, -1.f), 0}, {-0.f, 1}, {0.f, 1}, {std::nextafterf(0.f, 1.f), 1}, {0.5f, 1},
      {std::nextafterf(1.f, 0.f), 1},  {1.f, 1},  {std::nextafterf(1.f, 2.f), 0}, {nan, 0}, {inf, 0}, {-inf, 0}, {-1.f, 0},
      {2.f, 0}};
  for (int legacy = 0; legacy < 2; ++legacy)
    for (int R = 0; R <= 5; ++R)
      for (const auto& e1 : edge)
        for (const auto& e2 : edge) {
          const Placed rel{e1.v, e2.v};
          const Verdict v = round_verdict(rel, 1.0, 2.0, R, legacy != 0);
          CHECK(v.status == kLadder[legacy][R][e1.inside][e2.inside]);
          CHECK(same(v.rel1, e1.v) && rel.calls1 == 1);
          // rel2 is evaluated only where rel1 passed and R >= 2; elsewhere it reads 0
          const bool reached = e1.inside && R >= 2;
          CHECK(rel.calls2 == (reached ? 1 : 0));
          CHECK(same(v.rel2, reached ? e2.v : 0.f));
        }
  // R below 0 (f > N, the kernels that do not answer it earlier): the underflow rung
  CHECK(round_verdict(Placed{0.5f, 0.5f}, 1.0, 2.0, -1, false).status == ST_USIZE_UNDERFLOW);
  CHECK(round_verdict(Placed{0.5f, 0.5f}, 1.0, 2.0, -3, true).status == ST_USIZE_UNDERFLOW);
}

// ---- the three arithmetic forms through the ladder, at sums whose reliabilities are exact: N = 8, R = 4
struct Case {
  int cons, legacy, rel_dim, D;
  float ms;
  double s_all, s_rel;
  int status;
  float rel1, rel2;
};
static const Case kCases[] = {
    // constrained, rd = 4: rel = 1 - 2 sqrt(s / n / 4)
    {1, 0, 0, 4, 1.f, 0.0, 0.0, 0, 1.f, 1.f},
    {1, 0, 0, 4, 1.f, 2.0, 1.0, 0, 0.5f, 0.5f},       // s / n / rd = 1/16 both
    {1, 0, 0, 4, 1.f, 8.0, 4.0, 0, 0.f, 0.f},         // 1/4: on 0
    {1, 0, 0, 4, 1.f, 18.0, 1.0, 6, -0.5f, 0.f},      // 9/16: rel1 = -1/2, rel2 not reached
    {1, 0, 0, 4, 1.f, 2.0, 9.0, 6, 0.5f, -0.5f},
    {1, 0, 0, 4, 1.f, -1.0, 1.0, 6, NAN, 0.f},        // sqrt of a negative mean
    {1, 0, 0, 4, 1.f, 2.0, -1.0, 6, 0.5f, NAN},
    // the divisor: rel_dim over D, legacy over both
    {1, 0, 16, 4, 1.f, 8.0, 4.0, 0, 0.5f, 0.5f},
    {1, 1, 16, 4, 1.f, 2.0, 1.0, 0, 0.f, 0.f},        // rd = 1
    {1, 1, 0, 4, 1.f, 4.5, 1.0, 6, -0.5f, 0.f},
    // unconstrained, max_spread 1/2: rel = 1 - min(1/2, sqrt(s / n)) / (1/2); legacy and the dimension play no part
    {0, 0, 0, 4, 0.5f, 0.0, 0.0, 0, 1.f, 1.f},
    {0, 0, 0, 4, 0.5f, 0.5, 0.25, 0, 0.5f, 0.5f},     // mean 1/16
    {0, 1, 16, 4, 0.5f, 0.5, 0.25, 0, 0.5f, 0.5f},
    {0, 0, 0, 4, 0.5f, 2.0, 1.0, 0, 0.f, 0.f},        // sqrt(mean) = max_spread: on 0
    {0, 0, 0, 4, 0.5f, 32.0, 64.0, 0, 0.f, 0.f},      // clamped: never below 0
    {0, 0, 0, 4, 0.5f, -1.0, 1.0, 0, 0.f, 0.f},       // min(max_spread, NaN) = max_spread
    // max_spread = 0: 0 / 0
    {0, 0, 0, 4, 0.f, 0.5, 0.25, 6, NAN, 0.f},
    {0, 0, 0, 4, 0.f, 0.0, 0.0, 6, NAN, 0.f},
};

template <class Rel, class S>
static void form_paths() {
  for (const Case& c : kCases) {
    const Rel rel{c.cons != 0, rel_divisor<S>(c.legacy != 0, c.rel_dim, c.D), c.ms, 8, 4};
    const Verdict v = round_verdict(rel, (S)c.s_all, (S)c.s_rel, 4, c.legacy != 0);
    CHECK(v.status == c.status);
    CHECK(same(v.rel1, c.rel1));
    CHECK(same(v.rel2, c.rel2));
    // the same sums with three reliable oracles: the fewest-reliable rung (rel2 from s_rel / 3 is inexact: status only)
    if (c.status == ST_OK && c.s_rel == 0.0) {
      const Rel rel3{c.cons != 0, rel_divisor<S>(c.legacy != 0, c.rel_dim, c.D), c.ms, 8, 3};
      CHECK(round_verdict(rel3, (S)c.s_all, (S)c.s_rel, 3, c.legacy != 0).status == (c.legacy ? ST_OK : ST_TOO_FEW_RELIABLE));
    }
  }
}

int main() {
  CHECK(rel_divisor<int>(false, 0, 7) == 7 && rel_divisor<int>(false, 12, 7) == 12 && rel_divisor<int>(false, -1, 7) == 7);
  CHECK(rel_divisor<int>(true, 0, 7) == 1 && rel_divisor<int>(true, 12, 7) == 1);
  ladder_paths();
  form_paths<RelF32, float>();
  form_paths<RelF32Rcp, float>();
  form_paths<RelF64, double>();
  if (g_fail) {
    std::fprintf(stderr, "verdict_selftest: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("verdict_selftest: ok\n");
  return 0;
}
