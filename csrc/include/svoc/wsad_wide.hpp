// The int64 / fp64 arithmetic of the wide-column exact kernel (consensus_wsadx.hip): values up to 2^37 wsad from
// their column's base, where the fp64 forms of wsad_fast.hpp no longer hold the dividends.  Host and device: the
// kernel includes and calls exactly these routines, and the host self-test (csrc/selftest/engine_selftest.cpp
// wsadx_paths) compares each with the i128 routines of wsad.hpp inside the precondition stated on it.  A
// precondition is the CALLER's to guarantee: outside it a routine may return a wrong value, and wdiv_z's
// correction loops may run for as many steps as its estimate is off.
#pragma once

#include <math.h>
#include <stdint.h>

#include "wsad_fast.hpp"

namespace svoc {

// floor((d^2 + 500000) / 1e6) = quadratic_deviation (math.cairo:170-173) for integral |d| < 2^38 (a quotient
// below 2^56.1), in fp64: d^2 as the exact double-double p + e (fma), the quotient estimated from p (within ~20
// of the truth), then the remainder p - q0 1e6 -- an integer below 2^25, so the fma returns it exactly -- plus
// e + 500000, floored by the half-offset form (wsad_fast.hpp), added back.
SVOC_HD uint64_t qdev_dd(double d) {
  const double p = d * d;
  const double e = fma(d, d, -p);
  const double q0 = floor(p * kInv6);
  const double r = fma(-q0, kW, p) + (e + 500000.0);
  const double adj = floor((r + 0.5) * kInv6);
  return (uint64_t)(int64_t)q0 + (uint64_t)(int64_t)adj;
}

// z = wsad_div(d, sd) = I128Div(d 1e6 + sd / 2, sd) (signed_decimal.cairo:114-116) for integral |d| < 2^38,
// sd >= 2 and |z| < 2^31, given dd = (double)d, h = (double)(sd / 2), inv = 1.0 / (double)sd: the quotient
// estimated from the rounded dividend and the column's reciprocal (relative error ~2^-51, so within 1 of the
// truncated quotient), then fixed with the exact int64 remainder.
// |z| < 2^31 is the caller's to guarantee -- the kernel does it through wdiv_z_masked below.  Past it the int32
// conversion of the estimate saturates (undefined in C++) and the correction loops run |z| - 2^31 times.
SVOC_HD int64_t wdiv_z(int64_t di, double dd, int64_t sd, double h, double inv) {
  const int64_t A = di * 1000000 + (int64_t)h;
  int64_t q = (int64_t)(int32_t)trunc(fma(dd, kW, h) * inv);
  int64_t r = A - q * sd;
  if (A >= 0) {
    while (r < 0) { --q; r += sd; }
    while (r >= sd) { ++q; r -= sd; }
  } else {
    while (r > 0) { ++q; r -= sd; }
    while (r <= -sd) { --q; r += sd; }
  }
  return q;
}

// The z step of the kernel's pass 2b: wdiv_z of a row's deviation where the row is reliable (m all ones), 0
// where it is not (m zero: a failing oracle's row, or a padding row past N).  Only the reliable rows obey
// |d| <= sqrt(R) sd (they make up the variance), hence |z| <= sqrt(R) 1e6 (1 + 2^-20) < 2^31; a masked row may
// lie 2^38 wsad from the mean over a deviation of a few thousand.  Its deviation is cleared arithmetically (no
// branch) before the division: the dividend is then sd / 2, the quotient 0, and no correction step runs.
SVOC_HD int64_t wdiv_z_masked(int64_t di, uint32_t m, int64_t sd, double h, double inv) {
  const int64_t dm = (int64_t)((uint64_t)di & (((uint64_t)m << 32) | m));
  return wdiv_z(dm, (double)dm, sd, h, inv);
}

// floor((v 1e6 + g / 2) / g) = wsad_div(v, g) for 0 <= v < 2^62, 1 <= g (a quotient below 2^62): the 128-bit
// dividend estimated in fp64 (within 1 of the quotient when g >= sqrt(v 1e6) or the quotient is small), the
// remainder exact modulo 2^64; the loops absorb any larger estimate error (at most the quotient's 2^-52: 2^10).
SVOC_HD int64_t wdiv_pos_x(int64_t v, int64_t g) {
  const int64_t h = g / 2;
  int64_t q = (int64_t)(fma((double)v, 1e6, (double)h) / (double)g);
  int64_t r = (int64_t)((uint64_t)v * 1000000ull + (uint64_t)h - (uint64_t)q * (uint64_t)g);
  while (r < 0) { --q; r += g; }
  while (r >= g) { ++q; r -= g; }
  return q;
}

// sqrt (math.cairo:271-292) for 0 <= v < 2^62: the contract's Newton steps and stop rule; false where the
// contract divides by zero (sqrt(1): g = 0 after the first halving).  (Newton from above: after the first step
// g >= sqrt(v 1e6) - 1, so wdiv_pos_x's estimate error (v 1e6 2^-53 / g) stays below one.)
SVOC_HD bool wsqrt_x(int64_t v, int64_t& out) {
  if (v == 0) {
    out = 0;
    return true;
  }
  int64_t g = v / 2, g2 = g + 1000000;
  for (int i = 0; i < MAX_SQRT_ITERATIONS; ++i) {
    if (g == g2) break;
    if (g == 0) return false;
    const int64_t n = wdiv_pos_x(v, g);
    g2 = g;
    g = (g + n) / 2;
  }
  out = g;
  return true;
}

// The z-score powers of pass 2b for integral |z| <= 1e7 (the kernel's reliable rows: |z| <= sqrt(R (1 + 1 / var))
// 1e6 (1 + 2^-20) with R <= 64 and var >= 2): z2 = wsad_mul(z, z) <= 1e8, z3 = wsad_mul(z2, z) (|z2 z| <= 1e15 <
// 2^51 - 2^19) and z4 = wsad_mul(z2, z2).  The half-offset fp64 forms (wsad_fast.hpp) are exact for z2 and z3,
// and for z4 while z2 < 2^25 (|z| < 5.8); the rare larger z2 squares in int64 (<= 1e16).
SVOC_HD void zpow_x(double zd, double& z2, double& z3, double& z4) {
  z2 = wmul_pos_h(zd, zd);                                        // wsad_mul(z, z)
  if (z2 < 33554432.0) {
    z4 = wmul_pos_h(z2, z2);                                      // wsad_mul(z^2, z^2)
  } else {
    const int64_t z2i = (int64_t)z2;
    z4 = (double)((z2i * z2i + 500000) / 1000000);
  }
  z3 = wmul_t(z2, zd);                                            // wsad_mul(z^2, z)
}

// skewness = I128Div(s3 n, (n-1)(n-2)); kurtosis = I128Div(I128Div(s4 n (n+1), n-1) - 3 W (n-1)^2, (n-2)(n-3))
// (math.cairo:336-337, 359-362; the wsad.hpp skew_from_sum / kurt_from_sum) for 4 <= n <= 64 reliable rows and
// the sums of their z powers: every dividend below 2^51 (|s3| < 2^37, s4 < 2^39), so the exact fp64 truncated
// divisions of wsad_fast.hpp apply.
SVOC_HD void skew_kurt_x(double s3, double s4, double Rd, double& sk, double& ku) {
  const double k3d = (Rd - 1.0) * (Rd - 2.0), ik3 = recip_lo(k3d), ik1 = recip_lo(Rd - 1.0);
  const double t2 = 3.0e6 * (Rd - 1.0) * (Rd - 1.0), k4d = (Rd - 2.0) * (Rd - 3.0), ik4 = recip_lo(k4d);
  sk = trunc_div_d(s3 * Rd, k3d, ik3);
  const double t1 = trunc_div_d(s4 * Rd * (Rd + 1.0), Rd - 1.0, ik1);
  ku = trunc_div_d(t1 - t2, k4d, ik4);
}

// ---- Up to 256 reliable rows (consensus_wsadx.hip, NSEG > 1: lane groups of 2 / 4, 64 < N <= 256) -----------------
// The routines above that work on one row (qdev_dd, wdiv_z, wdiv_z_masked) or on one value (wdiv_pos_x, wsqrt_x) do
// not depend on the row count and are used as they are.  What changes with R <= 256 reliable rows, all within
// |x - B| < 2^37 of their column's base (a range below 2^38):
//   - the column sum of x - B stays below 256 * 2^37 = 2^45: exact in fp64, and inside trunc_div_d's |a| < 2^51 with
//     a divisor R < 2^31 and a quotient below 2^38 < 2^47 (wsad_fast.hpp; recip_lo and tdiv_rel_fix carry no bound
//     on the row count);
//   - the sum of the rows' qdev around their truncated mean m: with the exact mean mu, sum (x - m)^2 = sum (x - mu)^2
//     + R (mu - m)^2 <= R range^2 / 4 + R (Popoviciu) < R 2^74 + R, so sum qdev <= (R 2^74 + R) / 1e6 + R / 2 + R
//     < 2^62.1 at R = 256: it fits uint64 (and int64) with no carry, and var R <= the sum does too (var_floor_g);
//   - a reliable row's z: its d^2 <= 1e6 qdev + 5e5 <= 1e6 R (var + 1), and the contract's sqrt of var >= 2 ends at
//     sd >= 0.999 sqrt(1e6 var) (1414 for var = 2; pinned by the self-test), so |z| <= 1e6 sqrt(R (1 + 1 / var)) /
//     0.999 + 1 < 1.97e7 at R = 256, var = 2 (var 0 and 1 revert).  z z < 3.9e14 stays in wmul_pos_h's range, z2 z
//     reaches 7.6e15 (past wmul_t's 2^51 - 2^19) and z2 z2 1.5e17 (int64), s4 n (n + 1) 9.7e15 (past 2^53).

// floor(sv / R) = the population variance (math.cairo:208-222) from the reliable rows' sum of qdev, for
// 0 <= sv < 2^63 and 1 <= R: a plain unsigned 64-bit division, once per column (no estimate, no correction loop).
SVOC_HD int64_t var_floor_g(uint64_t sv, int64_t R) { return (int64_t)(sv / (uint64_t)R); }

// The z-score powers for integral |z| <= 2e7 (R <= 256 reliable rows, var >= 2: above): z2 = wsad_mul(z, z) <= 4e8
// by the half-offset fp64 form (z z <= 4e14 < 2.25e15).  While z2 < 2^25 (|z| < 5.8e6) the fp64 forms of zpow_x hold
// (|z2 z| < 2^25 5.8e6 < 2^48); past it z3 = I128Div(z2 z + 500000, 1e6) and z4 = I128Div(z2 z2 + 500000, 1e6) in
// int64 (|z2 z| <= 8e15, z2 z2 <= 1.6e17, both below 2^63; C's division truncates toward zero, as I128Div).
// |z3| <= 8e9 and z4 <= 1.6e11 are exact doubles.
SVOC_HD void zpow_g(double zd, double& z2, double& z3, double& z4) {
  z2 = wmul_pos_h(zd, zd);                                        // wsad_mul(z, z)
  if (z2 < 33554432.0) {
    z4 = wmul_pos_h(z2, z2);                                      // wsad_mul(z^2, z^2)
    z3 = wmul_t(z2, zd);                                          // wsad_mul(z^2, z)
  } else {
    const int64_t z2i = (int64_t)z2, zi = (int64_t)zd;
    z4 = (double)((z2i * z2i + 500000) / 1000000);
    z3 = (double)((z2i * zi + 500000) / 1000000);
  }
}

// skewness = I128Div(s3 n, (n-1)(n-2)); kurtosis = I128Div(I128Div(s4 n (n+1), n-1) - 3 W (n-1)^2, (n-2)(n-3))
// (math.cairo:336-337, 359-362; the wsad.hpp skew_from_sum / kurt_from_sum) in int64, for 4 <= n <= 256 reliable
// rows and the sums of zpow_g's powers over them: |s3| <= 256 * 8e9 < 2^41 and 0 <= s4 <= 256 * 1.6e11 < 2^46, so
// |s3 n| < 2^49 and s4 n (n + 1) < 2^46 * 65792 < 2^63.  Once per column: plain 64-bit divisions.
SVOC_HD void skew_kurt_g(int64_t s3, int64_t s4, int64_t n, int64_t& sk, int64_t& ku) {
  sk = (s3 * n) / ((n - 1) * (n - 2));
  const int64_t t1 = (s4 * n * (n + 1)) / (n - 1);
  ku = (t1 - 3 * 1000000 * (n - 1) * (n - 1)) / ((n - 2) * (n - 3));
}

}  // namespace svoc
