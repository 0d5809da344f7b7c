// Spatial autocorrelation of genes on the spot lattice: Moran's I and Geary's C per (slide, gene) with the analytic moments
// under normality and a permutation test, for every slide of an evaluation per call (DESIGN 6.16 states the arithmetic,
// tests/spatial_reference.py restates it in numpy).  Slide s owns rows offsets[s] .. offsets[s + 1] of every row-stacked
// array.  The graph is a fixed-width list: nbr (rows, k) int32 segment-local, w (rows, k) fp64 (0: a pruned slot), deg (rows,).
//
//   sp_edges_kernel    one thread per row: the k neighbours after the row itself of the exact kNN list become the slots;
//                      prune 0 keeps all, 1 keeps d <= mean + population std of the row's k distances (slot order), 2 keeps
//                      d <= 2; kept edges weigh 1, or 1 / deg with row standardisation.  For a GIVEN list it validates instead
//                      (index range, finite weights >= 0, no neighbour twice) and classifies every row as binary and / or
//                      row-standardised.
//   sp_indeg_kernel    one thread per slot: counts the in-neighbours of a row BY THEIR OUT-DEGREE with integer atomics
//                      (hist[row][d]): the in-weight of a row is then sum_d hist[d] w(d) in ascending d, whatever order
//                      the atomics arrived in.
//   sp_consts_kernel   one workgroup per slide: S0 = sum w_ij, S1 = 1/2 sum (w_ij + w_ji)^2 with w_ji looked up in j's own
//                      k slots, S2 = sum_i (out_i + in_i)^2, all in the fixed row order below.
//   sp_perm_kernel     one workgroup per (slide, permutation): n unique 64-bit keys (a splitmix64 stream of (seed, p) with
//                      the low 14 bits replaced by the row index), an LDS bitonic sort, the low 14 bits of the sorted keys
//                      are the permutation, stored as uint16.
//   sp_stat_kernel     THE HOT PATH.  A workgroup takes C adjacent gene columns of one slide -- as many as its LDS holds,
//                      at most 6 --, centres them into LDS once (column-interleaved fp64: one row's C values are adjacent)
//                      and walks all permutations out of LDS: 4 groups of 256 threads take 4 permutations at a time, a
//                      thread owns the rows r, r + 256, ..., reads pi(i) and pi(nbr(i, t)) through the uint16 table and
//                      gathers z from LDS.  The observed statistic is the same kernel without a table (pi = identity).
//   sp_moments_kernel / sp_prank_kernel / sp_bh_kernel / sp_summary_kernel
//                      z and p under normality (-log10 p in log space), Benjamini-Hochberg over the genes of a slide by
//                      exact counting ranks (stats.h, as csrc/markers.hip), and per gene the folded
//                      permutation p, the mean and population variance of the sims summed over p in ascending order.
//
// THE FIXED ROW ORDER of every fp64 sum over the rows of a slide: lane r of 256 adds its rows r, r + 256, ... in ascending
// order; the 64 lanes of a wave are combined by the xor butterfly 32, 16, ... 1 (both partners add the same two numbers, so
// every lane holds one value: the halving tree p[l] += p[l + o]); the four wave totals as (t0 + t1) + (t2 + t3).  It is a
// function of n alone.  Every product and sum is rounded separately (no contraction).  No floating-point atomics, no
// workgroup waits for another: a slide inside a batch is bit-identical to the same slide alone.
#include "common.h"
#include "stats.h"

namespace {

constexpr int SP_MAX_N = 16384;          // spots per slide: 14 index bits in a permutation key, uint16 tables
constexpr int SP_MAX_K = 64;
constexpr int SP_MAX_G = 16384;
constexpr int SP_MAX_S = 65535;          // grid.y
constexpr int SP_MAX_PERMS = 65535;      // grid.x of the permutation kernel
constexpr int SP_ROW_THREADS = 256;
constexpr int SP_LANES = 256;            // row lanes of the fixed order
constexpr int SP_GROUPS = 4;             // permutations in flight per workgroup
constexpr int SP_STAT_THREADS = SP_LANES * SP_GROUPS;
constexpr int SP_CMAX = 6;               // columns per workgroup: 114 VGPRs; 7 and 8 spill at 1024 threads
constexpr int SP_Z_BYTES = 155648;       // LDS for the centred columns (152 KiB of the 160)
constexpr int SP_SORT_THREADS = 1024;
constexpr int SP_O_THREADS = 256;
constexpr int SP_BH_THREADS = 1024;
constexpr int SP_STATUS = 6;             // config, bad index, bad weight, duplicate neighbour, non-binary rows, non-standardised rows

__host__ __device__ inline long long sp_align8(long long v) { return (v + 7) & ~7ll; }
// workspace: permutation table uint16[n_perms * rows] | in-degree histogram int32[rows * hist_slots]
__host__ __device__ inline long long sp_table_bytes(long long rows, long long n_perms) { return sp_align8(rows * n_perms * 2); }

__host__ __device__ inline int sp_columns(int n) {
  int c = SP_Z_BYTES / (8 * n);
  if (c > SP_CMAX) c = SP_CMAX;
  return c < 1 ? 1 : c;
}
__host__ __device__ inline int sp_pow2ceil(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// rows of slide s, 0 when its offsets break the caller's statements: segment_rows (device.h) with r1 < r0 tested ahead of
// the subtraction and the terms in another order; the shared form changes the code of this file's kernels
__device__ __forceinline__ int sp_slide_rows(const long long* __restrict__ offsets, int s, long long rows, int min_n, int max_n,
                                             long long* r0_out) {
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  *r0_out = r0;
  if (r0 < 0 || r1 < r0 || r1 > rows || r1 - r0 < min_n || r1 - r0 > max_n) return 0;
  return (int)(r1 - r0);
}

// ------------------------------------------------------------------------------------------------------------ graph
__global__ __launch_bounds__(SP_ROW_THREADS) void sp_edges_kernel(
    const int* __restrict__ knn_idx, const double* __restrict__ knn_dist, const long long* __restrict__ offsets,
    long long rows, int min_n, int max_n, int k, int prune, int rowstd, int given, int* __restrict__ nbr,
    double* __restrict__ w, int* __restrict__ deg, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, min_n, max_n, &r0);
  if (n == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[SP_STATUS * s] = 1;
    return;
  }
  const int i = blockIdx.x * SP_ROW_THREADS + threadIdx.x;
  if (i >= n) return;
  const long long row = r0 + i;
  int* nb = nbr + row * k;
  double* ww = w + row * k;
  if (!given) {
    const double* d = knn_dist + row * (k + 1) + 1;     // position 0 of the kNN list is the row itself
    const int* id = knn_idx + row * (k + 1) + 1;
    double bound = INFINITY;
    if (prune == 1) {
      double sum = 0.0;
      for (int t = 0; t < k; ++t) sum = sum + d[t];
      const double mean = sum / (double)k;
      double q = 0.0;
      for (int t = 0; t < k; ++t) {
        const double dv = d[t] - mean;
        const double sq = dv * dv;
        q = q + sq;
      }
      bound = mean + sqrt(q / (double)k);
    } else if (prune == 2) {
      bound = 2.0;
    }
    int dg = 0, bad = 0;
    for (int t = 0; t < k; ++t) dg += d[t] <= bound;
    const double wv = rowstd ? 1.0 / (double)dg : 1.0;
    for (int t = 0; t < k; ++t) {
      int j = id[t];
      if (j < 0 || j >= n) { ++bad; j = 0; }
      nb[t] = j;
      ww[t] = d[t] <= bound ? wv : 0.0;
    }
    deg[row] = dg;
    if (bad) atomicAdd(&status[SP_STATUS * s + 1], bad);
  } else {
    int dg = 0, badi = 0, badw = 0, dup = 0;
    for (int t = 0; t < k; ++t) {
      const int j = nb[t];
      const double wt = ww[t];
      badi += j < 0 || j >= n;
      badw += !(wt >= 0.0) || isinf(wt);
      dg += wt > 0.0;
    }
    const double ws = 1.0 / (double)dg;
    int notbin = 0, notstd = 0;
    for (int t = 0; t < k; ++t) {
      const double wt = ww[t];
      if (!(wt > 0.0)) continue;
      notbin |= wt != 1.0;
      notstd |= wt != ws;
      for (int u = 0; u < t; ++u) dup += nb[u] == nb[t] && ww[u] > 0.0;
    }
    deg[row] = dg;
    if (badi) atomicAdd(&status[SP_STATUS * s + 1], badi);
    if (badw) atomicAdd(&status[SP_STATUS * s + 2], badw);
    if (dup) atomicAdd(&status[SP_STATUS * s + 3], dup);
    if (notbin) atomicAdd(&status[SP_STATUS * s + 4], 1);
    if (notstd) atomicAdd(&status[SP_STATUS * s + 5], 1);
  }
}

__global__ __launch_bounds__(SP_ROW_THREADS) void sp_indeg_kernel(
    const long long* __restrict__ offsets, long long rows, int min_n, int max_n, int k, const int* __restrict__ nbr,
    const double* __restrict__ w, const int* __restrict__ deg, int* __restrict__ hist) {
  const int s = blockIdx.y;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, min_n, max_n, &r0);
  const long long e = (long long)blockIdx.x * SP_ROW_THREADS + threadIdx.x;
  if (e >= (long long)n * k) return;
  const int i = (int)(e / k);
  const int j = nbr[r0 * k + e], d = deg[r0 + i];
  if (w[r0 * k + e] > 0.0 && j >= 0 && j < n && d >= 1 && d <= k) atomicAdd(&hist[(r0 + j) * (k + 1) + d], 1);
}

__global__ __launch_bounds__(SP_LANES) void sp_consts_kernel(
    const long long* __restrict__ offsets, long long rows, int min_n, int max_n, int k, int rowstd, int given,
    const int* __restrict__ nbr, const double* __restrict__ w, const int* __restrict__ hist,
    const int* __restrict__ status, double* __restrict__ consts) {
#pragma clang fp contract(off)
  __shared__ double red[3][SP_LANES / 64];
  const int s = blockIdx.x, r = threadIdx.x;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, min_n, max_n, &r0);
  const int* st = status + SP_STATUS * s;
  bool ok = n > 0 && st[1] == 0 && st[2] == 0 && st[3] == 0;
  // a given list is binary when every kept weight is 1, else row-standardised when every kept weight is 1 / deg
  int standardised = rowstd;
  if (given) {
    standardised = st[4] != 0;
    if (st[4] != 0 && st[5] != 0) ok = false;
  }
  if (!ok) {
    if (r < 3) consts[3 * s + r] = NAN;
    return;
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = r; i < n; i += SP_LANES) {
    const int* nb = nbr + (r0 + i) * k;
    const double* ww = w + (r0 + i) * k;
    double out = 0.0, s1 = 0.0;
    for (int t = 0; t < k; ++t) {
      const double a = ww[t];
      out = out + a;
      if (a > 0.0) {
        const int j = nb[t];
        const int* nbj = nbr + (r0 + j) * k;
        const double* wj = w + (r0 + j) * k;
        double b = 0.0;
        for (int u = 0; u < k; ++u) {
          const double wu = wj[u];
          if (nbj[u] == i && wu > 0.0) b = wu;         // at most one slot: a neighbour appears once
        }
        double term;
        if (b > 0.0 && j != i) {                        // the ordered pairs (i, j) and (j, i): one from each row
          const double ab = a + b;
          term = ab * ab;
        } else if (j == i) {                            // a self loop is one pair
          const double aa = a + a;
          term = aa * aa;
        } else {                                        // (i, j) and (j, i) both hold a alone
          const double sq = a * a;
          term = 2.0 * sq;
        }
        s1 = s1 + term;
      }
    }
    const int* h = hist + (r0 + i) * (k + 1);
    double in = 0.0;
    if (standardised) {
      for (int d = 1; d <= k; ++d) {
        const double share = (double)h[d] * (1.0 / (double)d);
        in = in + share;
      }
    } else {
      int cnt = 0;
      for (int d = 1; d <= k; ++d) cnt += h[d];
      in = (double)cnt;
    }
    const double tot = out + in;
    const double sq = tot * tot;
    a0 = a0 + out;
    a1 = a1 + s1;
    a2 = a2 + sq;
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  if ((r & 63) == 0) { red[0][r >> 6] = a0; red[1][r >> 6] = a1; red[2][r >> 6] = a2; }
  __syncthreads();
  if (r < 3) {
    const double tot = (red[r][0] + red[r][1]) + (red[r][2] + red[r][3]);
    consts[3 * s + r] = r == 1 ? 0.5 * tot : tot;
  }
}

// ----------------------------------------------------------------------------------------------------- permutations
__global__ __launch_bounds__(SP_SORT_THREADS) void sp_perm_kernel(const long long* __restrict__ offsets, long long rows,
                                                                  int max_n, int P, u64 seed,
                                                                  unsigned short* __restrict__ table) {
  extern __shared__ __align__(16) unsigned char sp_sort_lds[];
  u64* keys = reinterpret_cast<u64*>(sp_sort_lds);
  const int p = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, 2, max_n, &r0);
  if (n == 0) return;
  const int P2 = sp_pow2ceil(n);
  const u64 h = mix64(mix64(seed) ^ (u64)p);
  for (int e = tid; e < P2; e += SP_SORT_THREADS)
    keys[e] = e < n ? ((mix64(h + (u64)e) & ~0x3FFFull) | (u64)e) : ~0ull;
  __syncthreads();
  for (int k2 = 2; k2 <= P2; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < (P2 >> 1); q += SP_SORT_THREADS) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
        const int a = i, b = i + j;
        const u64 ka = keys[a], kb = keys[b];
        const bool up = (i & k2) == 0;
        if ((ka > kb) == up && ka != kb) { keys[a] = kb; keys[b] = ka; }
      }
      __syncthreads();
    }
  }
  unsigned short* out = table + r0 * P + (long long)p * n;
  for (int e = tid; e < n; e += SP_SORT_THREADS) out[e] = (unsigned short)(keys[e] & 0x3FFFull);
}

// ------------------------------------------------------------------------------------------------------- statistics
template <typename T, int C>
__global__ __launch_bounds__(SP_STAT_THREADS) void sp_stat_kernel(
    const T* __restrict__ x, long long ld, const long long* __restrict__ offsets, int S, long long rows, int G, int max_n,
    int k, const int* __restrict__ nbr, const double* __restrict__ w, const double* __restrict__ consts,
    const unsigned short* __restrict__ table, int P, double* __restrict__ mean_out, double* __restrict__ den_out,
    double* __restrict__ stat, int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char sp_lds[];
  __shared__ double part[2][SP_GROUPS][4][2 * C];
  __shared__ double mean_s[C], den_s[C];
  __shared__ int varies_s, nonfinite_s;
  double* zs = reinterpret_cast<double*>(sp_lds);           // [n][C]
  const int s = blockIdx.y;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, 2, max_n, &r0);
  if (n == 0 || sp_columns(n) != C) return;
  const int j0 = blockIdx.x * C;
  if (j0 >= G) return;
  const int cc = min(C, G - j0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = wave >> 2, wg = wave & 3, r = tid & (SP_LANES - 1);
  if (tid == 0) { varies_s = 0; nonfinite_s = 0; }

  // whole row segments: consecutive threads read the C adjacent columns of one row (a column past G reads the last one)
  const T* xs = x + r0 * ld + j0;
  const int total = n * C;
  int nf = 0;
  for (int e = tid; e < total; e += SP_STAT_THREADS) {
    const int i = e / C, q = e - i * C;
    const double v = ldd(xs + (long long)i * ld + (q < cc ? q : cc - 1));
    nf += !isfinite(v);
    zs[e] = v;
  }
  __syncthreads();
  int differs = 0;
  for (int e = tid; e < total; e += SP_STAT_THREADS) {
    const int q = e % C;
    if (zs[e] != zs[q]) differs |= 1 << q;
  }
  if (differs) atomicOr(&varies_s, differs);
  if (nf) atomicAdd(&nonfinite_s, nf);
  // the column means, in the fixed row order
  for (int q0 = 0; q0 < C; q0 += SP_GROUPS) {
    const int q = q0 + grp;
    double a = 0.0;
    if (q < C)
      for (int i = r; i < n; i += SP_LANES) a = a + zs[i * C + q];
    a = wave_sum(a);
    if (lane == 0) part[0][grp][wg][0] = a;
    __syncthreads();
    if (tid < SP_GROUPS && q0 + tid < C)
      mean_s[q0 + tid] = ((part[0][tid][0][0] + part[0][tid][1][0]) + (part[0][tid][2][0] + part[0][tid][3][0])) / (double)n;
    __syncthreads();
  }
  const int varies = varies_s;
  for (int e = tid; e < total; e += SP_STAT_THREADS) {
    const int q = e % C;
    zs[e] = ((varies >> q) & 1) ? zs[e] - mean_s[q] : 0.0;   // a constant column is exactly zero: den = 0, NaN statistics
  }
  __syncthreads();
  for (int q0 = 0; q0 < C; q0 += SP_GROUPS) {
    const int q = q0 + grp;
    double a = 0.0;
    if (q < C)
      for (int i = r; i < n; i += SP_LANES) {
        const double z = zs[i * C + q];
        const double sq = z * z;
        a = a + sq;
      }
    a = wave_sum(a);
    if (lane == 0) part[0][grp][wg][0] = a;
    __syncthreads();
    if (tid < SP_GROUPS && q0 + tid < C)
      den_s[q0 + tid] = (part[0][tid][0][0] + part[0][tid][1][0]) + (part[0][tid][2][0] + part[0][tid][3][0]);
    __syncthreads();
  }
  if (tid < cc && mean_out) {
    mean_out[(long long)s * G + j0 + tid] = mean_s[tid];
    den_out[(long long)s * G + j0 + tid] = den_s[tid];
  }
  if (tid == 0 && nonfinite_s) atomicAdd(&status[s], nonfinite_s);

  const double S0 = consts[3 * s];
  const double fI = (double)n / S0, fC = (double)(n - 1) / (2.0 * S0);
  const int* nb = nbr + r0 * k;
  const double* ww = w + r0 * k;
  const unsigned short* tb = table ? table + r0 * P : nullptr;
  const long long plane = (long long)S * P * G;              // stat: (2, S, P, G)
  const int iters = (P + SP_GROUPS - 1) / SP_GROUPS;
  const int nm1 = n - 1;
  for (int it = 0; it < iters; ++it) {
    const int p = it * SP_GROUPS + grp;
    const bool live = p < P;
    const unsigned short* pi = tb ? tb + (long long)(live ? p : 0) * n : nullptr;
    double aI[C], aC[C];
#pragma unroll
    for (int q = 0; q < C; ++q) { aI[q] = 0.0; aC[q] = 0.0; }
    if (live) {
      for (int i = r; i < n; i += SP_LANES) {
        const int pi_i = pi ? min((int)pi[i], nm1) : i;
        double zi[C], lag[C], gc[C];
#pragma unroll
        for (int q = 0; q < C; ++q) { zi[q] = zs[pi_i * C + q]; lag[q] = 0.0; gc[q] = 0.0; }
        const int* nbi = nb + (long long)i * k;
        const double* wi = ww + (long long)i * k;
        for (int t = 0; t < k; ++t) {
          const int j = min(max(nbi[t], 0), nm1);
          const double wt = wi[t];
          const int pj = pi ? min((int)pi[j], nm1) : j;
#pragma unroll
          for (int q = 0; q < C; ++q) {
            const double zj = zs[pj * C + q];
            const double prod = wt * zj;
            lag[q] = lag[q] + prod;
            const double d = zi[q] - zj;
            const double sq = d * d;
            const double wsq = wt * sq;
            gc[q] = gc[q] + wsq;
          }
        }
#pragma unroll
        for (int q = 0; q < C; ++q) {
          const double prod = zi[q] * lag[q];
          aI[q] = aI[q] + prod;
          aC[q] = aC[q] + gc[q];
        }
      }
    }
    double (*buf)[4][2 * C] = part[it & 1];
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const double tI = wave_sum(aI[q]), tC = wave_sum(aC[q]);
      if (lane == 0) { buf[grp][wg][q] = tI; buf[grp][wg][C + q] = tC; }
    }
    __syncthreads();                                         // (the other buffer is written next: one barrier per round)
    if (live && r < cc) {
      const double numI = (buf[grp][0][r] + buf[grp][1][r]) + (buf[grp][2][r] + buf[grp][3][r]);
      const double numC = (buf[grp][0][C + r] + buf[grp][1][C + r]) + (buf[grp][2][C + r] + buf[grp][3][C + r]);
      const double den = den_s[r];
      const long long o = ((long long)s * P + p) * G + j0 + r;
      stat[o] = fI * (numI / den);
      stat[plane + o] = fC * (numC / den);
    }
  }
}

// --------------------------------------------------------------------------------------------- moments, BH, summary
__global__ __launch_bounds__(SP_O_THREADS) void sp_moments_kernel(
    const long long* __restrict__ offsets, int S, long long rows, int G, int max_n, const double* __restrict__ consts,
    const double* __restrict__ stat, int two_tailed, double* __restrict__ zn, double* __restrict__ pv,
    double* __restrict__ nl) {
#pragma clang fp contract(off)
  const int s = blockIdx.y, which = blockIdx.z;
  const int g = blockIdx.x * SP_O_THREADS + threadIdx.x;
  if (g >= G) return;
  long long r0;
  const int n = sp_slide_rows(offsets, s, rows, 2, max_n, &r0);
  const long long o = ((long long)which * S + s) * G + g;
  const double nd = (double)n, S0 = consts[3 * s], S1 = consts[3 * s + 1], S2 = consts[3 * s + 2];
  const double v = stat[o], s02 = S0 * S0;
  double z;
  if (which == 0) {
    const double EI = -1.0 / (nd - 1.0);
    const double num = ((nd * nd) * S1 - nd * S2) + 3.0 * s02;
    const double VI = num / ((nd * nd - 1.0) * s02) - EI * EI;
    z = (v - EI) / sqrt(VI);
  } else {
    const double num = (2.0 * S1 + S2) * (nd - 1.0) - 4.0 * s02;
    const double VC = num / ((2.0 * (nd + 1.0)) * s02);
    z = (v - 1.0) / sqrt(VC);
  }
  double p, l;
  stats::normal_tail(z, two_tailed, &p, &l);
  if (n == 0 || isnan(z)) { z = NAN; p = NAN; l = NAN; }
  zn[o] = z;
  pv[o] = p;
  nl[o] = l;
}

// rank of every gene's p ascending (NaN as 1, equal p by gene index); scratch[rank] = p G / (rank + 1)
// (the counting loop is written out in every kernel that has it: stats.h says why it holds no shared form)
__global__ __launch_bounds__(SP_O_THREADS) void sp_prank_kernel(int G, const double* __restrict__ pvals,
                                                                int* __restrict__ prank, double* __restrict__ scratch) {
#pragma clang fp contract(off)
  __shared__ double tile[SP_O_THREADS];
  const long long base = (long long)blockIdx.y * G;
  const int g = blockIdx.x * SP_O_THREADS + threadIdx.x;
  double p = pvals[base + (g < G ? g : G - 1)];
  if (isnan(p)) p = 1.0;
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += SP_O_THREADS) {
    const int j = j0 + threadIdx.x;
    const double pj = pvals[base + (j < G ? j : G - 1)];
    tile[threadIdx.x] = isnan(pj) ? 1.0 : pj;
    __syncthreads();
    const int cnt = min(SP_O_THREADS, G - j0);
    for (int q = 0; q < cnt; ++q) rank += (tile[q] < p) || (tile[q] == p && j0 + q < g);
    __syncthreads();
  }
  if (g < G) {
    prank[base + g] = rank;
    stats::bh_stage(scratch, base, rank, p, G);
  }
}

// one workgroup per (statistic, slide): Benjamini-Hochberg in gene order; a NaN p (a constant gene) counts as p = 1 among
// the others and stays NaN itself
__global__ __launch_bounds__(SP_BH_THREADS) void sp_bh_kernel(int G, const double* __restrict__ pvals,
                                                              const int* __restrict__ prank, double* __restrict__ scratch,
                                                              double* __restrict__ adj) {
  __shared__ double cmin[SP_BH_THREADS];
  const long long base = (long long)blockIdx.x * G;
  stats::bh_adjust<SP_BH_THREADS, true>(pvals, prank, scratch, adj, base, G, cmin);
}

__global__ __launch_bounds__(SP_O_THREADS) void sp_summary_kernel(int S, int G, int P, const double* __restrict__ stat,
                                                                  const double* __restrict__ sims, int two_tailed,
                                                                  int* __restrict__ count, double* __restrict__ pval_sim,
                                                                  double* __restrict__ pval_z_sim,
                                                                  double* __restrict__ mean_sim,
                                                                  double* __restrict__ var_sim) {
#pragma clang fp contract(off)
  const int s = blockIdx.y, which = blockIdx.z;
  const int g = blockIdx.x * SP_O_THREADS + threadIdx.x;
  if (g >= G) return;
  const long long o = ((long long)which * S + s) * G + g;
  const double* col = sims + ((long long)which * S + s) * P * G + g;
  const double v = stat[o];
  int larger = 0;
  double sum = 0.0;
  for (int p = 0; p < P; ++p) {
    const double sv = col[(long long)p * G];
    larger += sv >= v;
    sum = sum + sv;
  }
  const double mean = sum / (double)P;
  double q = 0.0;
  for (int p = 0; p < P; ++p) {
    const double d = col[(long long)p * G] - mean;
    const double sq = d * d;
    q = q + sq;
  }
  const double var = q / (double)P;
  if (P - larger < larger) larger = P - larger;
  const double z = (v - mean) / sqrt(var);
  double pz, l;
  stats::normal_tail(z, two_tailed, &pz, &l);
  const bool bad = isnan(v);
  count[o] = bad ? -1 : larger;
  pval_sim[o] = bad ? NAN : ((double)larger + 1.0) / ((double)P + 1.0);
  pval_z_sim[o] = bad || isnan(z) ? NAN : pz;
  mean_sim[o] = mean;
  var_sim[o] = var;
}

inline bool sp_shape_ok(int32_t S, int64_t rows, int32_t max_n) {
  return S >= 1 && S <= SP_MAX_S && max_n >= 2 && max_n <= SP_MAX_N && rows >= 2 && rows <= (int64_t)S * max_n;
}

template <typename T, int C>
int sp_launch_stat(const void* x, int64_t ld, const int64_t* offsets, int S, int64_t rows, int G, int max_n, int k,
                   const int32_t* nbr, const double* w, const double* consts, const unsigned short* table, int P,
                   double* mean, double* den, double* stat, int32_t* status, hipStream_t st) {
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sp_stat_kernel<T, C>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, SP_Z_BYTES);
  }
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL((sp_stat_kernel<T, C>), dim3((G + C - 1) / C, S), dim3(SP_STAT_THREADS), SP_Z_BYTES, st,
                     static_cast<const T*>(x), (long long)ld, reinterpret_cast<const long long*>(offsets), S,
                     (long long)rows, G, max_n, k, nbr, w, consts, table, P, mean, den, stat, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

template <typename T>
int sp_launch_stat_all(int cmask, const void* x, int64_t ld, const int64_t* offsets, int S, int64_t rows, int G, int max_n,
                       int k, const int32_t* nbr, const double* w, const double* consts, const unsigned short* table, int P,
                       double* mean, double* den, double* stat, int32_t* status, hipStream_t st) {
  int rc = MCL_OK;
#define SP_ONE(C)                                                                                                   \
  if (rc == MCL_OK && (cmask >> C) & 1)                                                                             \
    rc = sp_launch_stat<T, C>(x, ld, offsets, S, rows, G, max_n, k, nbr, w, consts, table, P, mean, den, stat, status, st)
  SP_ONE(1); SP_ONE(2); SP_ONE(3); SP_ONE(4); SP_ONE(5); SP_ONE(6);
  static_assert(SP_CMAX == 6, "one launch per column count");
#undef SP_ONE
  return rc;
}

}  // namespace

extern "C" int64_t mcl_spatial_workspace_bytes(int64_t rows, int32_t hist_slots, int32_t n_perms) {
  if (rows < 2 || rows > (int64_t)SP_MAX_S * SP_MAX_N || hist_slots < 0 || hist_slots > SP_MAX_K + 1 || n_perms < 0 ||
      n_perms > SP_MAX_PERMS)
    return -1;
  return sp_table_bytes(rows, n_perms) + sp_align8(rows * hist_slots * 4) + 8;
}

extern "C" int32_t mcl_spatial_columns(int32_t n) { return (n < 2 || n > SP_MAX_N) ? -1 : sp_columns(n); }

extern "C" int mcl_spatial_lattice(const int32_t* knn_indices, const double* knn_distances, const int64_t* offsets,
                                   int32_t S, int64_t rows, int32_t max_n, int32_t k, int32_t prune,
                                   int32_t row_standardise, int32_t given, void* work, int32_t* nbr, double* w,
                                   int32_t* deg, double* consts, int32_t* status, mcl_stream_t stream) {
  if (!offsets || !work || !nbr || !w || !deg || !consts || !status) return MCL_EINVAL;
  if (!given && (!knn_indices || !knn_distances)) return MCL_EINVAL;
  if (!sp_shape_ok(S, rows, max_n) || k < 1 || k > SP_MAX_K || prune < 0 || prune > 2) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int min_n = given ? 2 : k + 1;
  int* hist = static_cast<int*>(work);                      // (the lattice call sizes the workspace with n_perms = 0)
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(hist, 0, (size_t)rows * (k + 1) * 4, st) != hipSuccess) return (int)hipGetLastError();
  if (hipMemsetAsync(status, 0, (size_t)S * SP_STATUS * 4, st) != hipSuccess) return (int)hipGetLastError();
  hipLaunchKernelGGL(sp_edges_kernel, dim3((max_n + SP_ROW_THREADS - 1) / SP_ROW_THREADS, S), dim3(SP_ROW_THREADS), 0, st,
                     knn_indices, knn_distances, off, (long long)rows, min_n, max_n, k, prune, row_standardise != 0,
                     given != 0, nbr, w, deg, status);
  MCL_CHECK_LAUNCH();
  const long long slots = (long long)max_n * k;
  hipLaunchKernelGGL(sp_indeg_kernel, dim3((unsigned)((slots + SP_ROW_THREADS - 1) / SP_ROW_THREADS), S),
                     dim3(SP_ROW_THREADS), 0, st, off, (long long)rows, min_n, max_n, k, nbr, w, deg, hist);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_consts_kernel, dim3(S), dim3(SP_LANES), 0, st, off, (long long)rows, min_n, max_n, k,
                     row_standardise != 0, given != 0, nbr, w, hist, status, consts);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_spatial_permutations(const int64_t* offsets, int32_t S, int64_t rows, int32_t max_n, int32_t n_perms,
                                        uint64_t seed, void* work, mcl_stream_t stream) {
  if (!offsets || !work || !sp_shape_ok(S, rows, max_n) || n_perms < 1 || n_perms > SP_MAX_PERMS) return MCL_EINVAL;
  const size_t lds = (size_t)sp_pow2ceil(max_n) * 8;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sp_perm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              SP_MAX_N * 8);
  }
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(sp_perm_kernel, dim3(n_perms, S), dim3(SP_SORT_THREADS), lds, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(offsets), (long long)rows, max_n, n_perms, (u64)seed,
                     static_cast<unsigned short*>(work));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_spatial_stats(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows,
                                 int32_t G, int32_t max_n, int32_t k, int32_t column_mask, const int32_t* nbr,
                                 const double* w, const double* consts, const void* table, int32_t n_perms, double* mean,
                                 double* den, double* stat, int32_t* status, mcl_stream_t stream) {
  if (!x || !offsets || !nbr || !w || !consts || !stat || !status) return MCL_EINVAL;
  if (!sp_shape_ok(S, rows, max_n) || G < 1 || G > SP_MAX_G || ld < G || (dtype != 0 && dtype != 1) || k < 1 ||
      k > SP_MAX_K || n_perms < 1 || n_perms > SP_MAX_PERMS || (column_mask & ~0x7E) || !column_mask)
    return MCL_EINVAL;
  if (!table && (n_perms != 1 || !mean || !den)) return MCL_EINVAL;     // the observed pass: the identity, once
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned short* tb = static_cast<const unsigned short*>(table);
  return dtype == 0 ? sp_launch_stat_all<float>(column_mask, x, ld, offsets, S, rows, G, max_n, k, nbr, w, consts, tb,
                                                n_perms, mean, den, stat, status, st)
                    : sp_launch_stat_all<double>(column_mask, x, ld, offsets, S, rows, G, max_n, k, nbr, w, consts, tb,
                                                 n_perms, mean, den, stat, status, st);
}

extern "C" int mcl_spatial_moments(const int64_t* offsets, int32_t S, int64_t rows, int32_t G, int32_t max_n,
                                   const double* consts, const double* stat, int32_t two_tailed, int32_t* prank,
                                   double* scratch, double* z_norm, double* pval_norm, double* neglog10_pval_norm,
                                   double* pval_norm_adj, mcl_stream_t stream) {
  if (!offsets || !consts || !stat || !prank || !scratch || !z_norm || !pval_norm || !neglog10_pval_norm || !pval_norm_adj)
    return MCL_EINVAL;
  if (!sp_shape_ok(S, rows, max_n) || G < 1 || G > SP_MAX_G || 2 * S > SP_MAX_S) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned gx = (G + SP_O_THREADS - 1) / SP_O_THREADS;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(sp_moments_kernel, dim3(gx, S, 2), dim3(SP_O_THREADS), 0, st,
                     reinterpret_cast<const long long*>(offsets), S, (long long)rows, G, max_n, consts, stat,
                     two_tailed != 0, z_norm, pval_norm, neglog10_pval_norm);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_prank_kernel, dim3(gx, 2 * S), dim3(SP_O_THREADS), 0, st, G, pval_norm, prank, scratch);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_bh_kernel, dim3(2 * S), dim3(SP_BH_THREADS), 0, st, G, pval_norm, prank, scratch, pval_norm_adj);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_spatial_perm_summary(int32_t S, int32_t G, int32_t n_perms, const double* stat, const double* sims,
                                        int32_t two_tailed, int32_t* count, double* pval_sim, double* pval_z_sim,
                                        double* mean_sim, double* var_sim, mcl_stream_t stream) {
  if (!stat || !sims || !count || !pval_sim || !pval_z_sim || !mean_sim || !var_sim) return MCL_EINVAL;
  if (S < 1 || S > SP_MAX_S || G < 1 || G > SP_MAX_G || n_perms < 1 || n_perms > SP_MAX_PERMS) return MCL_EINVAL;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(sp_summary_kernel, dim3((G + SP_O_THREADS - 1) / SP_O_THREADS, S, 2), dim3(SP_O_THREADS), 0,
                     static_cast<hipStream_t>(stream), S, G, n_perms, stat, sims, two_tailed != 0, count, pval_sim,
                     pval_z_sim, mean_sim, var_sim);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
