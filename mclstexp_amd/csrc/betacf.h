// The continued fraction of the regularised incomplete beta function I_x(a, b) by the modified Lentz recurrence, in log
// space: the p-values of csrc/gene_significance.hip (Pearson r: b = a) and csrc/markers.hip (Welch t: b = 1/2, a = nu / 2
// with a non-integer nu).  Both return log cf, NaN if the recurrence has not converged in CF_MAX_ITER trips; the caller
// adds the prefactor a log x + b log(1 - x) - log a - log B(a, b) and keeps x on the side the fraction converges from,
// x < (a + 1) / (a + b + 2).
#pragma once
#include <hip/hip_runtime.h>

constexpr int CF_MAX_ITER = 1000;   // 7 - 80 trips at n <= 4900; the trip count grows like sqrt(a)

// log of the continued fraction of I_x(a, a), x <= 1/2 (modified Lentz); NaN if it has not converged in CF_MAX_ITER trips
static __device__ double log_betacf_sym(double a, double x) {
  const double tiny = 1e-300;
  const double tol = 4.440892098500626e-16;  // 2 ulp of 1
  const double qab = 2.0 * a, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0;
  double d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= CF_MAX_ITER; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (a - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= tol) return log(h);
  }
  return NAN;
}

// the general case: log of the continued fraction of I_x(a, b), x < (a + 1) / (a + b + 2), a and b any positive reals
static __device__ double log_betacf(double a, double b, double x) {
  const double tiny = 1e-300;
  const double tol = 4.440892098500626e-16;  // 2 ulp of 1
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0;
  double d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= CF_MAX_ITER; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= tol) return log(h);
  }
  return NAN;
}
