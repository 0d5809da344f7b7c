// Exact t-SNE in two dimensions (sklearn.manifold.TSNE(method="exact"), degrees of freedom 1) for every segment (slide) of
// a row-stacked matrix; the arithmetic is the one DESIGN 6.10 states.  Everything is fp64, there are no floating-point
// atomics, no workgroup waits on another, and every summation order is a function of (n_s, tile shape) alone: a slide
// inside a batch is bit-identical to the same slide alone, and a run to its repeat.
//
//   mcl_tsne_affinities   ts_affinity_kernel: one workgroup per row; the row's squared distances are computed once into
//                         LDS, the <= 100 steps of the precision search reduce over them in a fixed order, the conditional
//                         row C_i goes to HBM.  ts_symmetrize_kernel: C + C^T in place, 32 x 32 tile pairs through LDS.
//                         ts_rowsum_kernel / ts_segsum_kernel: sum P.  ts_normalize_kernel: max(P / sum P, eps), diagonal 0.
//   mcl_tsne_gradient     ts_pair_kernel (the hot path): P is the only HBM stream, y_j is staged in LDS in chunks, a wave owns
//                         four rows, lanes stride over j, lane partials meet in a fixed butterfly.  ts_finish_kernel: sum Q,
//                         the gradient rows and, on request, the KL divergence.
//   mcl_tsne_update       ts_update_kernel: gains, update, Y and the squared norm of the gain-scaled gradient.
//
// Segments ride on grid.y; per-segment parameters (exaggeration, momentum, learning rate, active, reset) come from a small
// device table, so a stopped segment costs nothing and the host reads results only when it checks convergence.
#include "common.h"

namespace {

constexpr int TS_MAX_D = 64;
constexpr int TS_MAX_N = 16384;                 // one row of distances in LDS: 128 KiB of the 160 KiB
constexpr long long TS_MAX_PAIRS = 1ll << 31;   // sum of n_s^2
constexpr int TS_MAX_S = 65535;                 // grid.y
constexpr int TS_THREADS = 256;
constexpr int TS_SEARCH_STEPS = 100;            // sklearn's n_steps
constexpr double TS_SEARCH_TOL = 1e-5;          // PERPLEXITY_TOLERANCE
constexpr double TS_ZERO_SUM = 1e-8;            // EPSILON_DBL: what a zero sum of the search becomes
constexpr double TS_EPS = 2.220446049250313e-16;   // MACHINE_EPSILON
constexpr double TS_LN2_HI = 6.93147180369123816490e-01;   // ln 2 = hi + lo, hi with 32 significant bits
constexpr double TS_LN2_LO = 1.90821492927058770002e-10;
constexpr int TS_TILE = 32;                    // symmetrisation tile
constexpr int TS_ROWS_PER_WAVE = 4;
constexpr int TS_ROWS_PER_BLOCK = 16;           // 4 waves x 4 rows
constexpr int TS_CHUNK = 2048;                  // y_j staged per pass: 32 KiB
constexpr int TS_ACC = 7;                       // per-row sums: A0 A1 R0 R1 S K sum p'
constexpr int TS_PARAMS = 5;                    // per segment: exaggeration, momentum, learning rate, active, reset

// the segment of this workgroup: first row, rows, first pair.  False (for the whole workgroup) where the offsets the
// caller vouched for do not fit the limits the launch was sized by: nothing is read or written then.
__device__ __forceinline__ bool ts_segment(const long long* off, const long long* poff, int s, int max_n, long long pairs,
                                           long long* o, int* n, long long* po) {
  const long long lo = off[s], len = off[s + 1] - lo, p = poff[s];
  if (len < 2 || len > max_n || p < 0 || p + len * len > pairs) return false;
  *o = lo;
  *n = (int)len;
  *po = p;
  return true;
}

// ------------------------------------------------------------------------------------------------------- affinities
// d_ij: ts_sqdist (common.h), shared with neighbors.hip
template <typename T>
__global__ __launch_bounds__(TS_THREADS) void ts_affinity_kernel(const T* __restrict__ x, long long ld, int D,
                                                                 const long long* __restrict__ off,
                                                                 const long long* __restrict__ poff, int max_n,
                                                                 long long pairs, double log_perplexity, int f32_dist,
                                                                 double* __restrict__ P, double* __restrict__ beta_out) {
  extern __shared__ double ts_dist[];            // n_s distances of row i
  __shared__ double xi[TS_MAX_D];
  __shared__ double red[2][4];
  long long o, po;
  int n;
  if (!ts_segment(off, poff, blockIdx.y, max_n, pairs, &o, &n, &po)) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= n) return;
  if (tid < D) xi[tid] = (double)x[(o + i) * ld + tid];
  __syncthreads();
  for (int j = tid; j < n; j += TS_THREADS) {
    double d = ts_sqdist(xi, x + (o + j) * ld, D);
    if (f32_dist) d = (double)(float)d;
    ts_dist[j] = d;
  }
  __syncthreads();
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, sum = 1.0;
  for (int step = 0; step < TS_SEARCH_STEPS; ++step) {
    double s = 0.0, t = 0.0;
    for (int j = tid; j < n; j += TS_THREADS) {
      const double d = ts_dist[j];
      const double e = j == i ? 0.0 : exp(-d * beta);
      s += e;
      t = fma(d, e, t);
    }
    s = block_sum4<true>(s, red[0]);
    t = block_sum4<true>(t, red[1]);
    if (s == 0.0) s = TS_ZERO_SUM;
    sum = s;
    const double diff = log(s) + beta * t / s - log_perplexity;    // the same in every thread
    if (fabs(diff) <= TS_SEARCH_TOL || step == TS_SEARCH_STEPS - 1) break;   // the row keeps the beta it was made with
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  double* row = P + po + (long long)i * n;
  for (int j = tid; j < n; j += TS_THREADS) row[j] = j == i ? 0.0 : exp(-ts_dist[j] * beta) / sum;
  if (tid == 0) beta_out[o + i] = beta;
}

// P = C + C^T in place: the workgroup of tile (bi, bj), bi <= bj, owns that tile and its mirror; nobody else touches them
__global__ __launch_bounds__(TS_THREADS) void ts_symmetrize_kernel(const long long* __restrict__ off,
                                                                   const long long* __restrict__ poff, int max_n,
                                                                   long long pairs, double* __restrict__ P) {
  __shared__ double ta[TS_TILE][TS_TILE + 1], tb[TS_TILE][TS_TILE + 1];
  long long o, po;
  int n;
  if (!ts_segment(off, poff, blockIdx.z, max_n, pairs, &o, &n, &po)) return;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj || bj * TS_TILE >= n) return;
  double* Ps = P + po;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  for (int r = r0; r < TS_TILE; r += 8) {
    const int ia = bi * TS_TILE + r, ja = bj * TS_TILE + c;     // tile (bi, bj)
    ta[r][c] = (ia < n && ja < n) ? Ps[(long long)ia * n + ja] : 0.0;
    const int ib = bj * TS_TILE + r, jb = bi * TS_TILE + c;     // tile (bj, bi)
    tb[r][c] = (ib < n && jb < n) ? Ps[(long long)ib * n + jb] : 0.0;
  }
  __syncthreads();
  for (int r = r0; r < TS_TILE; r += 8) {
    const int ia = bi * TS_TILE + r, ja = bj * TS_TILE + c;
    if (ia < n && ja < n) Ps[(long long)ia * n + ja] = ta[r][c] + tb[c][r];
    const int ib = bj * TS_TILE + r, jb = bi * TS_TILE + c;
    if (bi != bj && ib < n && jb < n) Ps[(long long)ib * n + jb] = ta[c][r] + tb[r][c];
  }
}

// one wave per row: lanes stride the columns, fixed butterfly
__global__ __launch_bounds__(TS_THREADS) void ts_rowsum_kernel(const long long* __restrict__ off,
                                                               const long long* __restrict__ poff, int max_n,
                                                               long long pairs, const double* __restrict__ P,
                                                               double* __restrict__ rowsum) {
  long long o, po;
  int n;
  if (!ts_segment(off, poff, blockIdx.y, max_n, pairs, &o, &n, &po)) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const double* row = P + po + (long long)i * n;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += row[j];
  s = wave_sum(s);
  if (lane == 0) rowsum[o + i] = s;
}

// one workgroup per segment: the sum of its row sums (threads stride the rows, then block_sum4), floored at eps
__global__ __launch_bounds__(TS_THREADS) void ts_segsum_kernel(const long long* __restrict__ off, int max_n,
                                                               const double* __restrict__ rowsum,
                                                               double* __restrict__ segsum) {
  __shared__ double red[4];
  const long long o = off[blockIdx.x], len = off[blockIdx.x + 1] - o;
  if (len < 2 || len > max_n) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < (int)len; i += TS_THREADS) s += rowsum[o + i];
  s = block_sum4<true>(s, red);
  if (threadIdx.x == 0) segsum[blockIdx.x] = fmax(s, TS_EPS);
}

__global__ __launch_bounds__(TS_THREADS) void ts_normalize_kernel(const long long* __restrict__ off,
                                                                  const long long* __restrict__ poff, int max_n,
                                                                  long long pairs, const double* __restrict__ segsum,
                                                                  double* __restrict__ P) {
  long long o, po;
  int n;
  if (!ts_segment(off, poff, blockIdx.y, max_n, pairs, &o, &n, &po)) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const double total = segsum[blockIdx.y];
  double* row = P + po + (long long)i * n;
  for (int j = lane; j < n; j += 64) row[j] = j == i ? 0.0 : fmax(row[j] / total, TS_EPS);
}

// -------------------------------------------------------------------------------------------------------- pair pass
// Per row i of a segment, over all j of it (p' = exaggeration * p, w = 1 / (1 + |y_i - y_j|^2)):
//   A_i = sum p' w (y_i - y_j), R_i = sum w^2 (y_i - y_j), S_i = sum_{j != i} w, and with KL also
//   K_i = sum p' log(max(p', eps) / w) and sum p'.
// Lane l of the wave that owns the row adds j = l, l + 64, ... in rising order; the 64 partials meet in wave_sum's butterfly.
template <bool KL>
__global__ __launch_bounds__(TS_THREADS) void ts_pair_kernel(const double* __restrict__ P,
                                                             const long long* __restrict__ poff,
                                                             const double* __restrict__ Y,
                                                             const long long* __restrict__ off, int max_n,
                                                             long long pairs, long long rows,
                                                             const double* __restrict__ params,
                                                             double* __restrict__ rowacc) {
  __shared__ double2 ys[TS_CHUNK];
  long long o, po;
  int n;
  const int s = blockIdx.y;
  if (!ts_segment(off, poff, s, max_n, pairs, &o, &n, &po)) return;
  if (blockIdx.x * TS_ROWS_PER_BLOCK >= n || params[s * TS_PARAMS + 3] == 0.0) return;
  const double exaggeration = params[s * TS_PARAMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * TS_ROWS_PER_BLOCK + wave * TS_ROWS_PER_WAVE;
  const double2* Y2 = reinterpret_cast<const double2*>(Y) + o;
  int irow[TS_ROWS_PER_WAVE];
  const double* prow[TS_ROWS_PER_WAVE];
  double2 yi[TS_ROWS_PER_WAVE];
  double acc[TS_ROWS_PER_WAVE][TS_ACC];
#pragma unroll
  for (int r = 0; r < TS_ROWS_PER_WAVE; ++r) {
    irow[r] = i0 + r < n ? i0 + r : n - 1;       // a row past the end repeats the last one and is not written
    prow[r] = P + po + (long long)irow[r] * n;
    yi[r] = Y2[irow[r]];
#pragma unroll
    for (int a = 0; a < TS_ACC; ++a) acc[r][a] = 0.0;
  }
  for (int c0 = 0; c0 < n; c0 += TS_CHUNK) {
    const int cn = n - c0 < TS_CHUNK ? n - c0 : TS_CHUNK;
    __syncthreads();
    for (int t = threadIdx.x; t < cn; t += TS_THREADS) ys[t] = Y2[c0 + t];
    __syncthreads();
#pragma unroll 2
    for (int jj = lane; jj < cn; jj += 64) {
      const int j = c0 + jj;
      const double2 yj = ys[jj];
#pragma unroll
      for (int r = 0; r < TS_ROWS_PER_WAVE; ++r) {
        const double p = prow[r][j] * exaggeration;
        const double d0 = yi[r].x - yj.x, d1 = yi[r].y - yj.y;
        const double w = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
        const double pw = p * w, ww = w * w;
        acc[r][0] = fma(pw, d0, acc[r][0]);
        acc[r][1] = fma(pw, d1, acc[r][1]);
        acc[r][2] = fma(ww, d0, acc[r][2]);
        acc[r][3] = fma(ww, d1, acc[r][3]);
        acc[r][4] += j == irow[r] ? 0.0 : w;
        if (KL) {
          acc[r][5] = fma(p, log(fmax(p, TS_EPS) / w), acc[r][5]);
          acc[r][6] += p;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TS_ROWS_PER_WAVE; ++r) {
#pragma unroll
    for (int a = 0; a < (KL ? TS_ACC : 5); ++a) {
      const double v = wave_sum(acc[r][a]);
      if (lane == 0 && i0 + r < n) rowacc[a * rows + o + i0 + r] = v;
    }
  }
}

// one workgroup per segment: sum Q = sum_i S_i, grad_i = 4 (A_i - R_i / sum Q), KL = sum_i (K_i + log(sum Q) sum_j p'_ij)
__global__ __launch_bounds__(TS_THREADS) void ts_finish_kernel(const long long* __restrict__ off, int max_n, long long rows,
                                                               const double* __restrict__ params,
                                                               const double* __restrict__ rowacc, int want_kl,
                                                               double* __restrict__ grad, double* __restrict__ kl) {
  __shared__ double red[2][4];
  const int s = blockIdx.x;
  const long long o = off[s], len = off[s + 1] - o;
  if (len < 2 || len > max_n || params[s * TS_PARAMS + 3] == 0.0) return;
  const int n = (int)len;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += TS_THREADS) q += rowacc[4 * rows + o + i];
  q = block_sum4<true>(q, red[0]);
  if (want_kl) {
    // sum K_i and log(sum Q) sum p' are each several times the KL they leave, so one rounding of either is ulps of the
    // result.  The rows' own shares K_i + log(sum Q) sum_j p'_ij are summed instead, with log(sum Q) = e ln2 + log(m),
    // m in [sqrt(1/2), sqrt(2)): e ln2_hi is exact (ln2_hi has 21 trailing zero bits) and the rest is below 0.35 in size.
    int e;
    double m = frexp(q, &e);
    if (m < 0.70710678118654752) {
      m *= 2.0;
      --e;
    }
    const double l_hi = (double)e * TS_LN2_HI, l_lo = fma((double)e, TS_LN2_LO, log(m));
    double k = 0.0;
    for (int i = threadIdx.x; i < n; i += TS_THREADS) {
      const double ps = rowacc[6 * rows + o + i];
      k += fma(ps, l_hi, rowacc[5 * rows + o + i]) + ps * l_lo;
    }
    k = block_sum4<true>(k, red[1]);
    if (threadIdx.x == 0) kl[s] = k;
  }
  for (int i = threadIdx.x; i < n; i += TS_THREADS) {
    grad[2 * (o + i)] = 4.0 * (rowacc[o + i] - rowacc[2 * rows + o + i] / q);
    grad[2 * (o + i) + 1] = 4.0 * (rowacc[rows + o + i] - rowacc[3 * rows + o + i] / q);
  }
}

// ----------------------------------------------------------------------------------------------------------- update
// sklearn's _gradient_descent step on every coordinate of a segment; one workgroup per segment
__global__ __launch_bounds__(TS_THREADS) void ts_update_kernel(const double* __restrict__ grad,
                                                               const long long* __restrict__ off, int max_n,
                                                               const double* __restrict__ params, double* __restrict__ Y,
                                                               double* __restrict__ update, double* __restrict__ gains,
                                                               double* __restrict__ grad_norm2) {
  __shared__ double red[4];
  const int s = blockIdx.x;
  const long long o = off[s], len = off[s + 1] - o;
  if (len < 2 || len > max_n || params[s * TS_PARAMS + 3] == 0.0) return;
  const double momentum = params[s * TS_PARAMS + 1], lr = params[s * TS_PARAMS + 2];
  const bool reset = params[s * TS_PARAMS + 4] != 0.0;
  double nrm = 0.0;
  for (long long e = 2 * o + threadIdx.x; e < 2 * (o + len); e += TS_THREADS) {
    const double g = grad[e];
    const double u = reset ? 0.0 : update[e];
    double gain = reset ? 1.0 : gains[e];
    gain = u * g < 0.0 ? gain + 0.2 : gain * 0.8;
    gain = fmax(gain, 0.01);
    const double gg = g * gain;
    const double un = momentum * u - lr * gg;
    gains[e] = gain;
    update[e] = un;
    Y[e] += un;
    nrm = fma(gg, gg, nrm);
  }
  nrm = block_sum4<true>(nrm, red);
  if (threadIdx.x == 0) grad_norm2[s] = nrm;
}

int ts_limits(int S, long long rows, int min_n, int max_n, long long pairs) {
  if (S > TS_MAX_S || max_n > TS_MAX_N || pairs > TS_MAX_PAIRS) return MCL_EUNSUPPORTED;
  if (min_n < 2 || min_n > max_n || rows < (long long)S * min_n || rows > (long long)S * max_n || pairs < rows * min_n ||
      pairs > rows * max_n)
    return MCL_EINVAL;
  return MCL_OK;
}

}  // namespace

extern "C" {

int64_t mcl_tsne_workspace_doubles(int32_t rows, int32_t S) {
  if (rows <= 0 || S <= 0) return 0;
  return (int64_t)TS_ACC * rows + S;
}

int mcl_tsne_affinities(const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets,
                        const int64_t* pair_offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n, int64_t pairs,
                        double perplexity, int32_t float32_distances, double* work, double* P, double* beta,
                        mcl_stream_t stream) {
  if (!x || !offsets || !pair_offsets || !work || !P || !beta || S <= 0 || rows <= 0 || D <= 0 || ld < D ||
      (dtype != 0 && dtype != 1) || !(perplexity > 0.0))
    return MCL_EINVAL;
  if (D > TS_MAX_D) return MCL_EUNSUPPORTED;
  const int rc = ts_limits(S, rows, min_n, max_n, pairs);
  if (rc != MCL_OK) return rc;
  if (!(perplexity < (double)min_n)) return MCL_EINVAL;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* poff = reinterpret_cast<const long long*>(pair_offsets);
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ts_affinity_kernel<float>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, TS_MAX_N * 8);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ts_affinity_kernel<double>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, TS_MAX_N * 8);
  }
  MCL_CLEAR_ERROR();
  const size_t lds = (size_t)max_n * 8;
  const double lp = log(perplexity);
  if (dtype == 0)
    hipLaunchKernelGGL(ts_affinity_kernel<float>, dim3(max_n, S), dim3(TS_THREADS), lds, st, (const float*)x, (long long)ld,
                       D, off, poff, max_n, (long long)pairs, lp, float32_distances, P, beta);
  else
    hipLaunchKernelGGL(ts_affinity_kernel<double>, dim3(max_n, S), dim3(TS_THREADS), lds, st, (const double*)x,
                       (long long)ld, D, off, poff, max_n, (long long)pairs, lp, float32_distances, P, beta);
  MCL_CHECK_LAUNCH();
  const int tiles = ceil_div(max_n, TS_TILE);
  double* rowsum = work;
  double* segsum = work + rows;
  hipLaunchKernelGGL(ts_symmetrize_kernel, dim3(tiles, tiles, S), dim3(TS_THREADS), 0, st, off, poff, max_n,
                     (long long)pairs, P);
  hipLaunchKernelGGL(ts_rowsum_kernel, dim3(ceil_div(max_n, 4), S), dim3(TS_THREADS), 0, st, off, poff, max_n,
                     (long long)pairs, P, rowsum);
  hipLaunchKernelGGL(ts_segsum_kernel, dim3(S), dim3(TS_THREADS), 0, st, off, max_n, rowsum, segsum);
  hipLaunchKernelGGL(ts_normalize_kernel, dim3(ceil_div(max_n, 4), S), dim3(TS_THREADS), 0, st, off, poff, max_n,
                     (long long)pairs, segsum, P);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_tsne_gradient(const double* P, const int64_t* pair_offsets, const double* Y, const int64_t* offsets, int32_t S,
                      int32_t rows, int32_t min_n, int32_t max_n, int64_t pairs, const double* seg_params, int32_t want_kl,
                      double* work, double* grad, double* kl, mcl_stream_t stream) {
  if (!P || !pair_offsets || !Y || !offsets || !seg_params || !work || !grad || (want_kl && !kl) || S <= 0 || rows <= 0)
    return MCL_EINVAL;
  const int rc = ts_limits(S, rows, min_n, max_n, pairs);
  if (rc != MCL_OK) return rc;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* poff = reinterpret_cast<const long long*>(pair_offsets);
  const dim3 grid(ceil_div(max_n, TS_ROWS_PER_BLOCK), S);
  MCL_CLEAR_ERROR();
  if (want_kl)
    hipLaunchKernelGGL(ts_pair_kernel<true>, grid, dim3(TS_THREADS), 0, st, P, poff, Y, off, max_n, (long long)pairs,
                       (long long)rows, seg_params, work);
  else
    hipLaunchKernelGGL(ts_pair_kernel<false>, grid, dim3(TS_THREADS), 0, st, P, poff, Y, off, max_n, (long long)pairs,
                       (long long)rows, seg_params, work);
  hipLaunchKernelGGL(ts_finish_kernel, dim3(S), dim3(TS_THREADS), 0, st, off, max_n, (long long)rows, seg_params, work,
                     want_kl, grad, kl);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_tsne_update(const double* grad, const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n,
                    const double* seg_params, double* Y, double* update, double* gains, double* grad_norm2,
                    mcl_stream_t stream) {
  if (!grad || !offsets || !seg_params || !Y || !update || !gains || !grad_norm2 || S <= 0 || rows <= 0) return MCL_EINVAL;
  const int rc = ts_limits(S, rows, min_n, max_n, (long long)rows * min_n);
  if (rc != MCL_OK) return rc;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(ts_update_kernel, dim3(S), dim3(TS_THREADS), 0, mcl_stream(stream), grad,
                     reinterpret_cast<const long long*>(offsets), max_n, seg_params, Y, update, gains, grad_norm2);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // extern "C"
