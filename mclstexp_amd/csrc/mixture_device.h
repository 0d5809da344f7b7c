// Device functions of the Gaussian mixture, shared by csrc/mixture.hip and csrc/hmrf.hip: the
// E-step in its two passes, the M-step, the fixed-order block sum and the workspace layout.  Everything is fp64 with
// contraction off; a file that includes this header repeats the pragma after its includes.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GM_THREADS = 256;
constexpr int GM_MAX = 64;            // D <= 64, K <= 64
constexpr int GM_LDA = GM_MAX + 1;    // row stride of the Cholesky buffer in LDS
constexpr int GM_MAX_ROWS = 50000;
constexpr int GM_AHEAD = 8;           // MFMA steps of the row sums whose operands are loaded before the first of them
constexpr double GM_LOG_2PI = 1.8378770664093453;
constexpr double GM_EPS10 = 10.0 * 2.220446049250313e-16;
enum { GM_FULL = 0, GM_TIED = 1, GM_DIAG = 2, GM_SPHERICAL = 3 };

struct GmShared {
  double chol[GM_MAX * GM_LDA];
  double red[GM_THREADS];
  double nk[GM_MAX], logw[GM_MAX], logdet[GM_MAX];
  double nk_sum;
  int fail;
};

// one (model, segment) problem; every pointer already points at this problem's part
struct GmModel {
  int n, D, K, KS, type;   // KS: row stride of lr (k_max)
  const double* x;         // (n, D), row stride ld
  long long ld;
  double* w;               // (K)
  double* mu;              // (K, D)
  double* cov;             // full (K, D, D), tied (D, D), diag (K, D), spherical (K)
  double* pc;              // the precision Cholesky factors, same shapes (full / tied: upper triangular)
  double* lr;              // (n, KS): weighted log prob -> log_resp -> resp
  double* lse;             // (n): log sum_k exp(weighted log prob)
  double* mom;             // (K, ncols) moment sums of the M-step
};

__host__ __device__ inline long long gm_cov_size(int type, int k_max, int D) {
  return type == GM_FULL ? (long long)k_max * D * D : type == GM_TIED ? (long long)D * D
       : type == GM_DIAG ? (long long)k_max * D : (long long)k_max;
}

// sum of one value per thread in a fixed tree; every thread gets the result
__device__ __forceinline__ double gm_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = GM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------------------------ E-step
// log w_k and log det P_k into LDS
__device__ __forceinline__ void gm_prepare(GmShared& sh, const GmModel& m) {
  const int k = threadIdx.x, D = m.D;
  if (k < m.K) {
    double ld = 0.0;
    if (m.type == GM_FULL || m.type == GM_TIED) {
      const double* P = m.pc + (m.type == GM_FULL ? (long long)k * D * D : 0);
      for (int j = 0; j < D; ++j) ld += log(P[j * D + j]);
    } else if (m.type == GM_DIAG) {
      for (int d = 0; d < D; ++d) ld += log(m.pc[k * D + d]);
    } else {
      ld = (double)D * log(m.pc[k]);
    }
    sh.logdet[k] = ld;
    sh.logw[k] = log(m.w[k]);
  }
  __syncthreads();
}

// The E-step's first pass: lr <- the weighted log prob ((-(D log 2 pi + ss) / 2) + log det P_k) + log w_k of every row
// and component; log w_k and log det P_k stay in LDS for the second pass.
__device__ __forceinline__ void gm_density(GmShared& sh, const GmModel& m) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = m.n, D = m.D, K = m.K, KS = m.KS;
  gm_prepare(sh, m);
  const double c0 = (double)D * GM_LOG_2PI;
  if (m.type == GM_FULL || m.type == GM_TIED) {
    // one wave = 16 rows x one component: y^T = P_k^T (x - mu_k)^T, 16 columns of y at a time, d ascending.
    // lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register q of lane l is D[(l >> 4) + 4 q][l & 15].
    const int lm = lane & 15, lk = lane >> 4;
    const int nrt = (n + 15) / 16, njt = (D + 15) / 16;
    // the four waves share one component at a time (its P_k stays in L1) and take every fourth row tile
    for (int job = w; job < 4 * ((nrt + 3) / 4) * K; job += 4) {
      const int k = job / (4 * ((nrt + 3) / 4)), rt = job - k * 4 * ((nrt + 3) / 4);
      if (rt >= nrt) continue;
      const double* P = m.pc + (m.type == GM_FULL ? (long long)k * D * D : 0);
      const double* mu = m.mu + k * D;
      const int row = rt * 16 + lm;
      const bool row_ok = row < n;
      const double* xr = m.x + (long long)(row_ok ? row : n - 1) * m.ld;
      double ss = 0.0;
      for (int jt = 0; jt < njt; ++jt) {
        const int j = jt * 16 + lm, jc = j < D ? j : D - 1;
        const int dmax = min(D, jt * 16 + 16);   // P is upper triangular: P[d][j] = 0 for d > j
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < dmax; d0 += 16) {   // four steps of four d: loads first, then the products in order
          double av[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int d = d0 + 4 * u + lk, dc = d < D ? d : D - 1;
            const double pv = P[dc * D + jc];
            const double xv = xr[dc] - mu[dc];
            av[u] = (d < D && j < D && d <= j) ? pv : 0.0;   // d past D or past j enters as 0: the sum is unchanged
            bv[u] = (d < D && row_ok) ? xv : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ss += acc[q] * acc[q];
      }
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      if (lk == 0 && row_ok) m.lr[(long long)row * KS + k] = ((-0.5 * (c0 + ss)) + sh.logdet[k]) + sh.logw[k];
    }
  } else {
    for (int i = tid; i < n; i += GM_THREADS) {
      const double* xr = m.x + (long long)i * m.ld;
      for (int k = 0; k < K; ++k) {
        double ss = 0.0;
        for (int d = 0; d < D; ++d) {
          const double t = (xr[d] - m.mu[k * D + d]) * (m.type == GM_DIAG ? m.pc[k * D + d] : m.pc[k]);
          ss += t * t;
        }
        m.lr[(long long)i * KS + k] = ((-0.5 * (c0 + ss)) + sh.logdet[k]) + sh.logw[k];
      }
    }
  }
  __syncthreads();
}

// The E-step's second pass: lr <- log_resp, lse <- log sum_k exp(lr) per row; labels (argmax of log_resp, ties to the lowest
// k) and resp = exp(log_resp) where asked for.  Returns the mean over the rows (every thread) of lse.
// With a field (n, KS) (the Potts-HMRF of DESIGN 6.18) lr is first coupled, lr + (beta field), and the mean is that of
// lse - za, za the log-sum-exp of the normalised prior log w_k + (beta field_k), written to za where asked for.
__device__ __forceinline__ double gm_finalise(GmShared& sh, const GmModel& m, int* lab, double* resp, const double* field,
                                              double beta, double* za) {
  const int tid = threadIdx.x;
  const int n = m.n, K = m.K, KS = m.KS;
  double part = 0.0;
  for (int i = tid; i < n; i += GM_THREADS) {
    double* v = m.lr + (long long)i * KS;
    double zl = 0.0;
    if (field) {
      const double* f = field + (long long)i * KS;
      for (int k = 0; k < K; ++k) v[k] = v[k] + (beta * f[k]);
      double amx = sh.logw[0] + (beta * f[0]);
      for (int k = 1; k < K; ++k) amx = fmax(amx, sh.logw[k] + (beta * f[k]));
      double as = 0.0;
      for (int k = 0; k < K; ++k) as += exp((sh.logw[k] + (beta * f[k])) - amx);
      zl = amx + log(as);
      if (za) za[i] = zl;
    }
    double mx = v[0];
    for (int k = 1; k < K; ++k) mx = fmax(mx, v[k]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(v[k] - mx);
    const double l = mx + log(s);
    double best = -INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
      const double lrk = v[k] - l;
      v[k] = lrk;
      if (resp) resp[(long long)i * KS + k] = exp(lrk);
      if (lrk > best) { best = lrk; bk = k; }
    }
    if (lab) lab[i] = bk;
    m.lse[i] = l;
    part += field ? l - zl : l;
  }
  return gm_block_sum(part, sh.red) / (double)n;
}

// the E-step of the mixture: both passes
__device__ __forceinline__ double gm_estep(GmShared& sh, const GmModel& m, int* lab, double* resp) {
  gm_density(sh, m);
  return gm_finalise(sh, m, lab, resp, nullptr, 0.0, nullptr);
}

// ------------------------------------------------------------------------------------------------------------ M-step
// mom[k][c] = sum_i resp[i][k] col_c(x_i), c: 0 .. D - 1 the columns of x, D the constant 1 (n_k), then x^2 (diag / spherical)
__device__ __forceinline__ void gm_moments(const GmModel& m, int ncols) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int n = m.n, D = m.D, K = m.K, KS = m.KS;
  const int nkt = (K + 15) / 16, nct = (ncols + 15) / 16;
  for (int job = w; job < nkt * nct; job += 4) {
    const int kt = job / nct, ct = job - kt * nct;
    const int k = kt * 16 + lm, kc = k < K ? k : K - 1;
    const int c = ct * 16 + lm;
    const int xc = c < D ? c : (c > D && c < ncols ? c - D - 1 : 0);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < n; i0 += 4 * GM_AHEAD) {   // GM_AHEAD steps of four rows: loads first, then the products in order
      double av[GM_AHEAD], bv[GM_AHEAD];
#pragma unroll
      for (int u = 0; u < GM_AHEAD; ++u) {
        const int i = i0 + 4 * u + lk;
        const bool ok = i < n;               // rows past n enter as 0 x 0: the sum is unchanged
        const int ic = ok ? i : n - 1;
        const double rv = m.lr[(long long)ic * KS + kc];
        const double xv = m.x[(long long)ic * m.ld + xc];
        const double cv = c < D ? xv : (c == D ? 1.0 : (c < ncols ? xv * xv : 0.0));
        av[u] = (ok && k < K) ? rv : 0.0;
        bv[u] = ok ? cv : 0.0;
      }
#pragma unroll
      for (int u = 0; u < GM_AHEAD; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kk = kt * 16 + lk + 4 * q, cc = ct * 16 + lm;
      if (kk < K && cc < ncols) m.mom[kk * ncols + cc] = acc[q];
    }
  }
}

// full: cov_k = sum_i resp_ik (x_i - mu_k)(x_i - mu_k)^T / n_k + reg I; tied: cov <- X^T X (finished by the caller).
// One wave = one 16 x 16 tile of the lower triangle of one matrix, rows ascending; the result is mirrored.
__device__ __forceinline__ void gm_scatter(const GmShared& sh, const GmModel& m, double reg) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int n = m.n, D = m.D, KS = m.KS;
  const bool full = m.type == GM_FULL;
  const int nt = (D + 15) / 16, ntri = nt * (nt + 1) / 2;
  const int njobs = (full ? m.K : 1) * ntri;
  for (int job = w; job < njobs; job += 4) {
    const int k = job / ntri;
    int t = job - k * ntri, ti = 0;
    while (t >= ti + 1) { t -= ti + 1; ++ti; }
    const int tj = t;
    const int d1 = ti * 16 + lm, d2 = tj * 16 + lm;
    const int d1c = d1 < D ? d1 : D - 1, d2c = d2 < D ? d2 : D - 1;
    const double mu1 = full ? m.mu[k * D + d1c] : 0.0, mu2 = full ? m.mu[k * D + d2c] : 0.0;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < n; i0 += 4 * GM_AHEAD) {
      double av[GM_AHEAD], bv[GM_AHEAD];
#pragma unroll
      for (int u = 0; u < GM_AHEAD; ++u) {
        const int i = i0 + 4 * u + lk;
        const bool ok = i < n;
        const int ic = ok ? i : n - 1;
        const double* xr = m.x + (long long)ic * m.ld;
        double a = xr[d1c] - mu1, b = xr[d2c] - mu2;
        if (full) a = m.lr[(long long)ic * KS + k] * a;
        av[u] = (ok && d1 < D) ? a : 0.0;
        bv[u] = (ok && d2 < D) ? b : 0.0;
      }
#pragma unroll
      for (int u = 0; u < GM_AHEAD; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
    double* C = m.cov + (full ? (long long)k * D * D : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i1 = ti * 16 + lk + 4 * q, i2 = tj * 16 + lm;
      if (i1 < D && i2 <= i1) {
        double v = acc[q];
        if (full) {
          v = v / sh.nk[k];
          if (i1 == i2) v += reg;
        }
        C[i1 * D + i2] = v;
        C[i2 * D + i1] = v;
      }
    }
  }
}

// P (D, D) upper triangular with P^T P = C^-1: the lower Cholesky factor L of C (right-looking, in LDS), then
// P = (L^-1)^T by one forward substitution per column.  Returns 1 (every thread) at a pivot that is not positive.
__device__ __forceinline__ int gm_precision_cholesky(GmShared& sh, const double* C, double* P, int D) {
  const int tid = threadIdx.x;
  double* a = sh.chol;
  __syncthreads();
  for (int e = tid; e < D * D; e += GM_THREADS) {
    const int i = e / D, c = e - i * D;
    a[i * GM_LDA + c] = C[e];
  }
  __syncthreads();
  for (int j = 0; j < D; ++j) {
    const double piv = a[j * GM_LDA + j];
    if (!(piv > 0.0)) return 1;   // an LDS value: the same for every thread
    const double ljj = sqrt(piv);
    __syncthreads();
    for (int i = j + tid; i < D; i += GM_THREADS) a[i * GM_LDA + j] = i == j ? ljj : a[i * GM_LDA + j] / ljj;
    __syncthreads();
    const int mm = D - j - 1;
    for (int e = tid; e < mm * mm; e += GM_THREADS) {
      const int ia = e / mm, i = j + 1 + ia, c = j + 1 + (e - ia * mm);
      if (c <= i) a[i * GM_LDA + c] = a[i * GM_LDA + c] - a[i * GM_LDA + j] * a[c * GM_LDA + j];
    }
    __syncthreads();
  }
  if (tid < D) {
    const int c = tid;
    double* Pc = P + c * D;
    for (int i = 0; i < c; ++i) Pc[i] = 0.0;
    Pc[c] = 1.0 / a[c * GM_LDA + c];
    for (int i = c + 1; i < D; ++i) {
      double s = 0.0;
      for (int t = c; t < i; ++t) s += a[i * GM_LDA + t] * Pc[t];
      Pc[i] = (0.0 - s) / a[i * GM_LDA + i];
    }
  }
  __syncthreads();
  return 0;
}

// sklearn's _estimate_gaussian_parameters + _compute_precision_cholesky from lr (log_resp if from_log, else resp, which it
// becomes).  init: weights = n_k / n (_initialize), else n_k / sum n_k (_m_step).  Returns 1 (every thread) when a
// covariance is not positive definite.
__device__ __forceinline__ int gm_mstep(GmShared& sh, const GmModel& m, double reg, bool from_log, bool init) {
  const int tid = threadIdx.x;
  const int n = m.n, D = m.D, K = m.K, KS = m.KS;
  const bool wide = m.type == GM_DIAG || m.type == GM_SPHERICAL;
  const int ncols = wide ? 2 * D + 1 : D + 1;
  if (from_log) {
    for (long long e = tid; e < (long long)n * K; e += GM_THREADS) {
      const long long i = e / K;
      double* p = m.lr + i * KS + (e - i * K);
      *p = exp(*p);
    }
  }
  if (tid == 0) sh.fail = 0;
  __syncthreads();
  gm_moments(m, ncols);
  __syncthreads();
  if (tid < K) sh.nk[tid] = m.mom[tid * ncols + D] + GM_EPS10;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += sh.nk[k];
    sh.nk_sum = s;
  }
  for (int e = tid; e < K * D; e += GM_THREADS) {
    const int k = e / D, d = e - k * D;
    m.mu[e] = m.mom[k * ncols + d] / sh.nk[k];
  }
  __syncthreads();
  if (tid < K) m.w[tid] = sh.nk[tid] / (init ? (double)n : sh.nk_sum);
  if (!wide) {
    gm_scatter(sh, m, reg);
    __syncthreads();
    if (m.type == GM_TIED) {
      for (int e = tid; e < D * D; e += GM_THREADS) {
        const int d1 = e / D, d2 = e - d1 * D;
        if (d2 > d1) continue;
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += (sh.nk[k] * m.mu[k * D + d1]) * m.mu[k * D + d2];
        double v = (m.cov[d1 * D + d2] - s) / sh.nk_sum;
        if (d1 == d2) v += reg;
        m.cov[d1 * D + d2] = v;
        m.cov[d2 * D + d1] = v;
      }
      __syncthreads();
      return gm_precision_cholesky(sh, m.cov, m.pc, D);
    }
    for (int k = 0; k < K; ++k)
      if (gm_precision_cholesky(sh, m.cov + (long long)k * D * D, m.pc + (long long)k * D * D, D)) return 1;
    return 0;
  }
  if (m.type == GM_DIAG) {
    for (int e = tid; e < K * D; e += GM_THREADS) {
      const int k = e / D, d = e - k * D;
      const double mu = m.mu[e];
      const double v = ((m.mom[k * ncols + D + 1 + d] / sh.nk[k]) - mu * mu) + reg;
      m.cov[e] = v;
      if (!(v > 0.0)) sh.fail = 1;
      m.pc[e] = 1.0 / sqrt(v);
    }
  } else if (tid < K) {
    const int k = tid;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
      const double mu = m.mu[k * D + d];
      s += ((m.mom[k * ncols + D + 1 + d] / sh.nk[k]) - mu * mu) + reg;
    }
    const double v = s / (double)D;
    m.cov[k] = v;
    if (!(v > 0.0)) sh.fail = 1;
    m.pc[k] = 1.0 / sqrt(v);
  }
  __syncthreads();
  return sh.fail;
}

// ------------------------------------------------------------------------------------------------------------ kernels
struct GmWork {   // the caller's workspace, in doubles
  double* lr;     // (R, rows, k_max)
  double* lse;    // (R, rows)
  double* mom;    // (S, R, k_max, 2 D + 1)
};
__host__ __device__ inline long long gm_work_doubles(long long rows, int S, int R, int D, int k_max) {
  return (long long)R * rows * (k_max + 1) + (long long)S * R * k_max * (2 * D + 1);
}
__host__ __device__ inline GmWork gm_work(void* work, long long rows, int R, int k_max) {
  GmWork wk;
  wk.lr = static_cast<double*>(work);
  wk.lse = wk.lr + (long long)R * rows * k_max;
  wk.mom = wk.lse + (long long)R * rows;
  return wk;
}

}  // namespace
