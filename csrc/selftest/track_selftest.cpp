// Host self-test of the per-oracle track record (svoc/track.hpp): track_score_exact against wsad.hpp's own i128
// wsad_div (wdiv) at the edges -- qmax 0, 1, 2^62 - 1, 2^63 - 1, q == qmax, q == qmax - 1, the 64-bit / 128-bit
// switch at 2^43, negative q and qmax -- and over random pairs of every bit length; track_score_fast against
// double arithmetic rounded once per operation; and track_update_one over rows that hold those values, against
// a loop written from the definitions.  Stand-alone (its own main), built by tests/test_track_host.py with the
// address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "svoc/status.hpp"
#include "svoc/track.hpp"
#include "svoc/wsad.hpp"

using namespace svoc;

static int g_fail = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      if (++g_fail <= 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                             \
  } while (0)

static std::mt19937_64 rng(4500);
static int64_t of_bits(int bits) {   // a value of exactly `bits` bits (0: zero)
  if (bits == 0) return 0;
  const uint64_t lo = 1ull << (bits - 1);
  return (int64_t)(lo + rng() % lo);
}

// the definition, in the contract's own i128 routines
static int64_t ref_exact(int64_t q, int64_t qmax) {
  if (qmax <= 0) return WSAD;
  if (q < 0) return 0;
  int st = ST_OK;
  const i128 d = wdiv((i128)q, (i128)qmax, st);
  CHECK(st == ST_OK);
  return (int64_t)((i128)WSAD - d);
}

static void exact_edges() {
  const int64_t M62 = (1ll << 62) - 1, M63 = std::numeric_limits<int64_t>::max();
  const int64_t qmaxes[] = {0, 1, 2, 3, WSAD, (1ll << 43) - 1, 1ll << 43, (1ll << 43) + 1, M62, M62 + 1, M63,
                            -1, std::numeric_limits<int64_t>::min()};
  for (int64_t qm : qmaxes) {
    const int64_t qs[] = {qm, qm - (qm > std::numeric_limits<int64_t>::min()), qm / 2, qm / 2 + 1, qm / 3, 0, 1,
                          (1ll << 43) - 1, 1ll << 43, -1, -5, std::numeric_limits<int64_t>::min()};
    for (int64_t q : qs) {
      if (q > qm) continue;   // (qmax is the row's maximum)
      CHECK(track_score_exact(q, qm) == ref_exact(q, qm));
    }
  }
  // the values the issue names, as literals
  CHECK(track_score_exact(M62, M62) == 0);
  CHECK(track_score_exact(M62 - 1, M62) == 0);        // wsad_div rounds to nearest: 1e6 - 2.2e-13
  CHECK(track_score_exact(M62 / 2, M62) == 500000);
  CHECK(track_score_exact(0, M62) == WSAD);
  CHECK(track_score_exact(0, 0) == WSAD && track_score_exact(-7, -3) == WSAD);
  CHECK(track_score_exact(-1, 5) == 0);
  CHECK(track_score_exact(1, 1) == 0 && track_score_exact(0, 1) == WSAD);
  CHECK(track_score_exact(1, 3) == WSAD - 333333 && track_score_exact(2, 3) == WSAD - 666667);
  // an int64 product is wrong at 2^62: what the 128-bit path is for
  const int64_t wrapped = (int64_t)((uint64_t)(M62 - 1) * (uint64_t)WSAD + (uint64_t)(M62 / 2));
  CHECK(WSAD - wrapped / M62 != track_score_exact(M62 - 1, M62));
}

static void exact_random() {
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const int64_t qm = of_bits(1 + it % 63);
    int64_t q = of_bits((int)(rng() % 64));
    if (q > qm) q = qm - (int64_t)(rng() % 3);   // (qmax is the row's maximum: at it, or just below)
    if (q < 0) q = 0;
    if (track_score_exact(q, qm) != ref_exact(q, qm)) ++bad;
    const int64_t s = track_score_exact(q, qm);
    if (s < 0 || s > WSAD) ++bad;
  }
  CHECK(bad == 0);
}

// the float quotient and difference through double: with 53 >= 2 * 24 + 2 bits, rounding the double result to
// float gives the correctly rounded float result (double rounding is innocuous for + - * / at that width)
static int64_t ref_fast(float q, float qmax) {
  if (!(qmax > 0.f) || std::isinf(qmax) || std::isnan(qmax)) return (int64_t)1 << 32;
  if (std::isinf(q) || std::isnan(q)) return 0;
  const float r = (float)((double)q / (double)qmax);
  float s = (float)(1.0 - (double)r);
  if (s < 0.f) s = 0.f;
  if (s > 1.f) s = 1.f;
  return (int64_t)std::floor((double)s * 4294967296.0);
}

static void fast_values() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float den = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
  CHECK(track_score_fast(0.f, 0.f) == kTrackFastOne && track_score_fast(1.f, -1.f) == kTrackFastOne);
  CHECK(track_score_fast(1.f, inf) == kTrackFastOne && track_score_fast(1.f, nan) == kTrackFastOne);
  CHECK(track_score_fast(nan, nan) == kTrackFastOne && track_score_fast(nan, 1.f) == 0);
  CHECK(track_score_fast(-inf, 1.f) == 0);
  CHECK(track_score_fast(1.f, 1.f) == 0 && track_score_fast(0.f, 1.f) == kTrackFastOne);
  CHECK(track_score_fast(-1.f, 1.f) == kTrackFastOne);            // 2, clamped to 1
  CHECK(track_score_fast(-big, den) == kTrackFastOne);            // 1 + inf, clamped to 1
  CHECK(track_score_fast(big, big) == 0 && track_score_fast(0.25f, 0.5f) == kTrackFastOne / 2);
  CHECK(track_score_fast(den * 3, den * 7) == ref_fast(den * 3, den * 7));
  CHECK(track_score_fast(den, den * 7) == ref_fast(den, den * 7));
  std::uniform_real_distribution<float> u(0.f, 1.f);
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const float qm = std::ldexp(0.5f + u(rng), (int)(rng() % 40) - 30);
    const float q = qm * u(rng);
    if (track_score_fast(q, qm) != ref_fast(q, qm)) ++bad;
  }
  CHECK(bad == 0);
  CHECK(track_fmax(nan, 1.f) == 1.f && track_fmax(1.f, nan) == 1.f && track_fmax(-inf, nan) == -inf);
  CHECK(track_fmax(2.f, 1.f) == 2.f && track_fmax(1.f, 2.f) == 2.f);
}

// track_update_one over B instances against a loop from the definitions (vectors sized exactly: the address
// sanitizer sees any cell outside them)
template <typename Q, typename Ref>
static void rows(const std::vector<std::vector<Q>>& qrows, int exact, Ref ref) {
  const int64_t B = (int64_t)qrows.size() * 3;
  const int N = (int)qrows[0].size();
  std::vector<uint8_t> active(B), reliable(B * N);
  std::vector<int32_t> status(B), rounds(B), flagged(B * N), streak(B * N);
  std::vector<int64_t> score(B * N);
  std::vector<Q> qr(B * N);
  for (int64_t b = 0; b < B; ++b) {
    active[b] = b % 3 == 1 ? 0 : (b % 2 ? 255 : 1);
    status[b] = b % 3 == 2 ? ST_ZERO_VARIANCE : ST_OK;
    rounds[b] = (int32_t)(rng() % 100);
    for (int i = 0; i < N; ++i) {
      const int64_t c = b * N + i;
      qr[c] = qrows[b / 3][i];
      reliable[c] = (uint8_t)(rng() % 2);
      flagged[c] = (int32_t)(rng() % 50);
      streak[c] = (int32_t)(rng() % 5);
      score[c] = (int64_t)(rng() % (1ull << 50));
    }
  }
  auto r0 = rounds; auto f0 = flagged; auto s0 = streak; auto c0 = score;
  TrackUpdate p{};
  p.active = active.data(); p.status = status.data(); p.reliable = reliable.data(); p.qr = qr.data();
  p.rounds = rounds.data(); p.flagged = flagged.data(); p.streak = streak.data(); p.score = score.data();
  p.B = B; p.N = N; p.exact = exact;
  for (int64_t b = 0; b < B; ++b) track_update_one(p, b);
  for (int64_t b = 0; b < B; ++b) {
    const bool go = b % 3 == 0;
    CHECK(rounds[b] == r0[b] + (go ? 1 : 0));
    Q qmax = qr[b * N];
    for (int i = 1; i < N; ++i)
      if (qr[b * N + i] > qmax || qmax != qmax) qmax = qr[b * N + i];
    for (int i = 0; i < N; ++i) {
      const int64_t c = b * N + i;
      if (!go) {
        CHECK(flagged[c] == f0[c] && streak[c] == s0[c] && score[c] == c0[c]);
        continue;
      }
      const int u = reliable[c] == 0;
      CHECK(flagged[c] == f0[c] + u);
      CHECK(streak[c] == (u ? s0[c] + 1 : 0));
      CHECK(score[c] == c0[c] + ref(qr[c], qmax));
    }
  }
}

static void update_rows() {
  const int64_t M62 = (1ll << 62) - 1;
  for (int N : {1, 2, 7, 65}) {
    std::vector<std::vector<int64_t>> ex;
    for (int64_t qm : {(int64_t)0, (int64_t)1, (int64_t)WSAD, M62, (int64_t)-4}) {
      std::vector<int64_t> row(N);
      for (int i = 0; i < N; ++i) row[i] = qm > 0 ? (int64_t)(rng() % (uint64_t)(qm + 1)) : qm;
      row[N - 1] = qm;
      if (N > 1) row[0] = qm > 0 ? qm - 1 : qm;
      if (N > 2) row[1] = qm > 0 ? -3 : qm;
      ex.push_back(row);
    }
    rows<int64_t>(ex, 1, ref_exact);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<std::vector<float>> fa;
    for (float qm : {0.f, 0.75f, std::numeric_limits<float>::denorm_min() * 7, inf, nan}) {
      std::vector<float> row(N);
      for (int i = 0; i < N; ++i) row[i] = qm > 0 && qm < inf ? qm * (float)(rng() % 8) / 8.f : 0.f;
      row[N - 1] = qm;
      if (N > 1) row[0] = nan;
      fa.push_back(row);
    }
    rows<float>(fa, 0, ref_fast);
  }
}

int main() {
  exact_edges();
  exact_random();
  fast_values();
  update_rows();
  if (g_fail) {
    std::fprintf(stderr, "track_selftest: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("track_selftest: ok\n");
  return 0;
}
