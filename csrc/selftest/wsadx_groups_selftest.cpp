// Host self-test of the R <= 256 arithmetic of the wide-column exact kernel's lane-group form
// (svoc/wsad_wide.hpp: var_floor_g, zpow_g, skew_kurt_g, and the row-count-independent routines at the values
// 256 rows reach; consensus_wsadx.hip calls exactly these for NSEG > 1) against the i128 routines of svoc/wsad.hpp:
// exact integer comparisons, inside each stated precondition and at its edges.  Stand-alone (its own main), built
// by tests/test_wsadx_groups_host.py with the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "svoc/status.hpp"
#include "svoc/wsad.hpp"
#include "svoc/wsad_fast.hpp"
#include "svoc/wsad_wide.hpp"

using namespace svoc;

static int g_fail = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      if (++g_fail <= 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                             \
  } while (0)

static std::mt19937_64 rng(25600);
static int64_t uni(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }
static int64_t of_bits(int bits) { return bits == 0 ? 0 : uni(1ll << (bits - 1), (1ll << bits) - 1); }

constexpr int64_t ZMAX = 20000000;   // zpow_g's |z| <= 2e7

// ---- zpow_g against wsad_mul
static bool zpow_ok(int64_t z) {
  int st = ST_OK;
  const i128 z2 = wmul(z, z, st), z3 = wmul(z2, z, st), z4 = wmul(z2, z2, st);
  double a, b, c;
  zpow_g((double)z, a, b, c);
  return st == ST_OK && (i128)(int64_t)a == z2 && (i128)(int64_t)b == z3 && (i128)(int64_t)c == z4;
}
static void zpow_paths() {
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const int64_t z = std::min(of_bits(it % 26), ZMAX);
    if (!zpow_ok(z) || !zpow_ok(-z)) ++bad;
  }
  for (int it = 0; it < 1000000 && bad < 10; ++it)
    if (!zpow_ok(uni(-ZMAX, ZMAX))) ++bad;
  CHECK(bad == 0);
  for (int64_t z : {(int64_t)0, (int64_t)1, (int64_t)707, (int64_t)708, ZMAX, ZMAX - 1}) CHECK(zpow_ok(z) && zpow_ok(-z));
  // z at sqrt(256 * 1.5) 1e6 (256 reliable rows, variance 2) and its neighbours
  const int64_t zr = (int64_t)std::llround(std::sqrt(256.0 * 1.5) * 1e6);
  CHECK(zr == 19595918);
  for (int64_t e = -3; e <= 3; ++e) CHECK(zpow_ok(zr + e) && zpow_ok(-(zr + e)));
  // the switch to int64 at z2 = 2^25, and z2 z across 2^51 (wmul_t's limit) and across 2^51 - 2^19
  int64_t zsw = 0, z51 = 0;
  for (int64_t z = 5000000; z <= 14000000; ++z) {
    const int64_t z2 = (z * z + 500000) / 1000000;
    if (!zsw && z2 >= (1ll << 25)) zsw = z;
    if (!z51 && (i128)z2 * z >= ((i128)1 << 51)) { z51 = z; break; }
  }
  CHECK(zsw > 5700000 && zsw < 5900000 && z51 > 13000000 && z51 < 13200000);
  for (int64_t e = -2000; e <= 2000; ++e) {
    CHECK(zpow_ok(zsw + e) && zpow_ok(-(zsw + e)));
    CHECK(zpow_ok(z51 + e) && zpow_ok(-(z51 + e)));
  }
  {
    const int64_t zb = z51 - 1, za = z51;   // just below and just above 2^51
    CHECK((i128)((zb * zb + 500000) / 1000000) * zb < ((i128)1 << 51));
    CHECK((i128)((za * za + 500000) / 1000000) * za >= ((i128)1 << 51));
    CHECK(zpow_ok(zb) && zpow_ok(za) && zpow_ok(-zb) && zpow_ok(-za));
  }
  // products z2 z + 500000 within 1 of a multiple of 1e6, beyond 2^51
  int hit = 0;
  for (int64_t z = z51; z < z51 + 3000000 && hit < 2000; ++z) {
    const int64_t z2 = (z * z + 500000) / 1000000;
    const int64_t rem = (int64_t)(((i128)z2 * z + 500000) % 1000000);
    if (rem <= 1 || rem >= 999999) {
      CHECK(zpow_ok(z) && zpow_ok(-z));
      ++hit;
    }
  }
  CHECK(hit > 0);
}

// ---- skew_kurt_g against skew_from_sum / kurt_from_sum
static bool sk_ok(int64_t s3, int64_t s4, int64_t n) {
  int st = ST_OK;
  const i128 sk = skew_from_sum(s3, n, st), ku = kurt_from_sum(s4, n, st);
  int64_t a, b;
  skew_kurt_g(s3, s4, n, a, b);
  return st == ST_OK && (i128)a == sk && (i128)b == ku;
}
static void skew_kurt_paths() {
  const int64_t S3 = 256 * 8000000000ll, S4 = 256 * 160000000000ll;   // the stated bounds of the sums
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const int64_t n = it % 3 == 0 ? 256 : uni(4, 256);
    const int64_t s3 = std::min(of_bits(it % 42), S3) * (it & 1 ? 1 : -1);
    const int64_t s4 = std::min(of_bits((it / 2) % 47), S4);
    if (!sk_ok(s3, s4, n)) ++bad;
  }
  CHECK(bad == 0);
  for (int64_t n : {(int64_t)4, (int64_t)5, (int64_t)64, (int64_t)65, (int64_t)128, (int64_t)129, (int64_t)255, (int64_t)256}) {
    CHECK(sk_ok(S3, S4, n) && sk_ok(-S3, S4, n) && sk_ok(0, 0, n) && sk_ok(1, 1, n) && sk_ok(-1, 0, n));
  }
  {
    // the kurtosis dividend past 2^53: one reliable row with z = sqrt(256 * 1.5) 1e6 among 256
    const int64_t z = 19595918, z2 = (z * z + 500000) / 1000000, z4 = (z2 * z2 + 500000) / 1000000;
    CHECK((i128)z4 * 256 * 257 > ((i128)1 << 53));
    for (int64_t e = -2000; e <= 2000; ++e) CHECK(sk_ok((z2 * z + 500000) / 1000000 + e, z4 + e, 256));
    // the smallest s4 whose dividend passes 2^53, and its neighbours
    const int64_t s53 = (int64_t)((((i128)1 << 53) + 256 * 257 - 1) / (256 * 257));
    for (int64_t e = -300; e <= 300; ++e) CHECK(sk_ok(e, s53 + e, 256));
  }
}

// ---- var_floor_g; the sum of qdev at the Popoviciu extreme
static void variance_paths() {
  int bad = 0;
  for (int it = 0; it < 1000000 && bad < 10; ++it) {
    const int64_t R = it % 3 == 0 ? 256 : uni(4, 256);
    const int64_t sv = it % 11 == 0 ? INT64_MAX - uni(0, 1000) : of_bits(it % 63);
    int st = ST_OK;
    if ((i128)var_floor_g((uint64_t)sv, R) != idiv_pos64((i128)sv, R, st) || st != ST_OK) ++bad;
  }
  CHECK(bad == 0);
  // half the rows at B - (2^37 - 1), half at B + (2^37 - 1): the mean is B, every deviation 2^37 - 1
  for (int R : {256, 254, 130, 66}) {
    const int64_t d = (1ll << 37) - 1;
    uint64_t sv = 0;
    i128 ref = 0;
    bool carry = false;
    for (int i = 0; i < R; ++i) {
      int st = ST_OK;
      const uint64_t q = qdev_dd((double)(i % 2 ? d : -d));
      ref += qdev(i % 2 ? d : -d, 0, st);
      carry = carry || sv + q < sv;
      sv += q;
      CHECK(st == ST_OK);
    }
    CHECK(!carry && (i128)sv == ref && ref < ((i128)1 << 63));
    if (R == 256) CHECK(ref >= ((i128)1 << 62));   // (2^62.07: past int64's half, inside it)
    int st = ST_OK;
    const int64_t var = var_floor_g(sv, R);
    CHECK((i128)var == idiv_pos64(ref, R, st) && var < (1ll << 62));
    int64_t sd = 0;
    CHECK(wsqrt_x(var, sd) && (i128)sd == wsqrt(var, st) && st == ST_OK);
  }
  // the range's other extreme: one row at -(2^38 - 2) from the rest (deviations from the mean below 2^38)
  {
    const int R = 256;
    const int64_t far = -((1ll << 38) - 2);
    const int64_t mean = far / R;   // (255 rows at 0, one at `far`: truncated toward zero)
    uint64_t sv = 0;
    i128 ref = 0;
    int st = ST_OK;
    for (int i = 0; i < R; ++i) {
      const int64_t x = i == 17 ? far : 0;
      sv += qdev_dd((double)(x - mean));
      ref += qdev(x, mean, st);
    }
    CHECK(st == ST_OK && (i128)sv == ref && (i128)var_floor_g(sv, R) == idiv_pos64(ref, R, st));
  }
  // the contract's sqrt of a variance >= 2 ends at sd >= 0.999 sqrt(1e6 var) (the bound behind |z| < 1.97e7)
  auto sd_ok = [&](int64_t var) {
    int64_t sd = 0;
    return wsqrt_x(var, sd) && (i128)sd * sd * 1000000 >= (i128)998001 * var * 1000000;
  };
  for (int64_t var = 2; var < 2000000 && bad < 10; ++var)
    if (!sd_ok(var)) ++bad;
  for (int it = 0; it < 300000 && bad < 10; ++it)
    if (!sd_ok(std::max((int64_t)2, of_bits(2 + it % 54)))) ++bad;
  CHECK(bad == 0);
}

// ---- the reliable mean over up to 256 rows: trunc_div_d + tdiv_rel_fix with |S| < 2^45
static void mean_paths() {
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const int64_t R = it % 3 == 0 ? 256 : uni(4, 256);
    const int64_t smax = R * ((1ll << 37) - 1);
    int64_t S = it % 7 == 0 ? smax - uni(0, 300) : std::min(of_bits(it % 46), smax);
    if (it & 1) S = -S;
    int64_t B = it % 5 == 0 ? uni(-300, 300) : of_bits(it % 62);
    if (it & 2) B = -B;
    if (it % 13 == 0) B = (it & 2) ? -((1ll << 61) - 1) : (1ll << 61) - 1;
    const double Sd = (double)S, Rd = (double)R, invR = recip_lo(Rd);
    const double qd = trunc_div_d(Sd, Rd, invR);
    const int64_t mur = tdiv_rel_fix((int64_t)qd, fma(-qd, Rd, Sd) == 0.0, Sd < 0.0, B);
    int st = ST_OK;
    const i128 want = idiv((i128)R * B + S, R, st) - B;
    if (st != ST_OK || (i128)mur != want) ++bad;
  }
  CHECK(bad == 0);
}

// ---- wdiv_z at the z a reliable row of 256 reaches (|z| <= 2e7), sd >= 1414
static void z_paths() {
  int bad = 0;
  for (int it = 0; it < 2000000 && bad < 10; ++it) {
    const int64_t sd = it % 50 == 0 ? 1414 : std::max((int64_t)1414, of_bits(11 + it % 27));
    const int64_t dmax = std::min((int64_t)((1ll << 38) - 1), sd * 20);
    const int64_t d = it % 5 == 0 ? (it % 2 ? dmax : -dmax) : uni(-dmax, dmax);
    int st = ST_OK;
    const int64_t want = (int64_t)wdiv(d, sd, st);
    const double h = (double)(sd / 2), inv = 1.0 / (double)sd;
    if (st != ST_OK || wdiv_z_masked(d, 0xffffffffu, sd, h, inv) != want || wdiv_z_masked(d, 0u, sd, h, inv) != 0) ++bad;
    if (want > ZMAX + 1 || want < -ZMAX - 1) ++bad;
  }
  CHECK(bad == 0);
}

// ---- whole columns of R reliable rows: mean, variance, sqrt, z powers, skewness, kurtosis both ways
static void column_paths() {
  int done = 0, big_z3 = 0, big_ku = 0;
  for (int it = 0; it < 6000; ++it) {
    const int kind = it % 5;
    const int R = (it % 4 == 0 || kind == 3 || (kind == 1 && it % 2)) ? 256 : (int)uni(65, 256);
    const int64_t B = (it % 3 == 0) ? uni(-1000000, 1000000) : of_bits(20 + it % 41) * (it & 1 ? 1 : -1);
    std::vector<int64_t> r(R);
    const int64_t amp = kind == 0 ? (1ll << 37) - 1 : of_bits(8 + it % 29);
    for (int i = 0; i < R; ++i) r[i] = uni(-amp, amp);
    if (kind == 1) {   // every row equal but one far out: one large z
      for (int i = 0; i < R; ++i) r[i] = 0;
      r[it % R] = (it & 1 ? 1 : -1) * uni(1500 * (int64_t)R, (1ll << 37) - 1);
    }
    if (kind == 3) {   // 256 rows, every row equal but one ~27,500 out: variance 2 or 3, z near sqrt(256 * 1.5) 1e6
      for (int i = 0; i < R; ++i) r[i] = 0;
      r[it % R] = (it & 1 ? 1 : -1) * uni(27350, 27800);
    }
    if (kind == 2) {   // two values only
      for (int i = 0; i < R; ++i) r[i] = i % 2 ? amp : -amp;
    }
    // i128 reference
    int st = ST_OK;
    i128 S = 0;
    for (int i = 0; i < R; ++i) S += B + r[i];
    const i128 mean = idiv(S, R, st);
    i128 sq = 0;
    for (int i = 0; i < R; ++i) sq += qdev(B + r[i], mean, st);
    const i128 var = idiv_pos64(sq, R, st);
    const i128 sdr = wsqrt(var, st);
    if (st != ST_OK || sdr == 0) continue;   // (a revert: the kernel hands it off)
    i128 s3r = 0, s4r = 0;
    for (int i = 0; i < R; ++i) {
      const i128 z = wdiv(B + r[i] - mean, sdr, st), z2 = wmul(z, z, st);
      s3r += wmul(z2, z, st);
      s4r += wmul(z2, z2, st);
      if ((z < 0 ? -z : z) * z2 >= ((i128)1 << 51)) ++big_z3;
    }
    const i128 skr = skew_from_sum(s3r, R, st), kur = kurt_from_sum(s4r, R, st);
    CHECK(st == ST_OK);
    if (s4r * R * (R + 1) > ((i128)1 << 53)) ++big_ku;
    // the kernel's forms
    double Sd = 0.0;
    for (int i = 0; i < R; ++i) Sd += (double)r[i];
    const double Rd = (double)R, invR = recip_lo(Rd), qd = trunc_div_d(Sd, Rd, invR);
    const int64_t mur = tdiv_rel_fix((int64_t)qd, fma(-qd, Rd, Sd) == 0.0, Sd < 0.0, B);
    CHECK((i128)(B + mur) == mean);
    uint64_t sv = 0;
    for (int i = 0; i < R; ++i) sv += qdev_dd((double)r[i] - (double)mur);
    CHECK((i128)sv == sq);
    const int64_t v = var_floor_g(sv, R);
    int64_t sd = 0;
    CHECK((i128)v == var && wsqrt_x(v, sd) && (i128)sd == sdr);
    const double h = (double)(sd / 2), inv = 1.0 / (double)sd;
    double s3 = 0.0, s4 = 0.0;
    for (int i = 0; i < R; ++i) {
      const int64_t z = wdiv_z_masked(r[i] - mur, 0xffffffffu, sd, h, inv);
      CHECK(z <= ZMAX && z >= -ZMAX);
      double z2, z3, z4;
      zpow_g((double)z, z2, z3, z4);
      s3 += z3;
      s4 += z4;
    }
    int64_t sk, ku;
    skew_kurt_g((int64_t)s3, (int64_t)s4, R, sk, ku);
    CHECK((i128)(int64_t)s3 == s3r && (i128)(int64_t)s4 == s4r && (i128)sk == skr && (i128)ku == kur);
    ++done;
  }
  CHECK(done > 4000 && big_z3 > 100 && big_ku > 100);
}

int main() {
  zpow_paths();
  skew_kurt_paths();
  variance_paths();
  mean_paths();
  z_paths();
  column_paths();
  if (g_fail) {
    std::fprintf(stderr, "wsadx_groups_selftest: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("wsadx_groups_selftest: ok\n");
  return 0;
}
