// The statistics at the end of the evaluation stages, once: the normal tail in log space, Benjamini-Hochberg over
// exact ranks, the top-n of G values.  Device code only, for the files that use it; a test
// pins every rule.  A form whose call changes its kernel stays local under a comment that names this header.
#pragma once
#include "device.h"

namespace stats {
constexpr double LN10 = 2.302585092994046;
constexpr double LN2 = 0.6931471805599453;
constexpr double SQRT2 = 1.4142135623730951;

// p = sf(|z|) (two_tailed: twice that) of the standard normal and -log10 p in log space: below |z| = sqrt 2 from p itself,
// above it from erfcx, which stays finite where p underflows
__device__ __forceinline__ void normal_tail(double z, int two_tailed, double* p_out, double* nl_out) {
#pragma clang fp contract(off)
  const double az = fabs(z) / SQRT2;
  const double e = erfc(az);
  if (two_tailed) {
    *p_out = e;
    *nl_out = az < 1.0 ? 0.0 - log10(e) : (az * az - log(erfcx(az))) / LN10;
  } else {
    const double p = 0.5 * e;
    *p_out = p;
    *nl_out = az < 1.0 ? 0.0 - log10(p) : ((az * az - log(erfcx(az))) + LN2) / LN10;
  }
}

// ---- orders: does (kj, j) come before (k, g)?  Descending; the index tells equal keys apart, so the ranks are a permutation:
// DESCENDING by ascending index (a stable sort), DESCENDING_HIGH by descending index (a stable ascending argsort backwards)
enum { DESCENDING, DESCENDING_HIGH };
template <int ORDER>
__device__ __forceinline__ int before(double kj, int j, double k, int g) {
  return (kj > k) || (kj == k && (ORDER == DESCENDING ? j < g : j > g));
}
// No shared form of the exact rank by counting against LDS tiles (marker_prank_kernel, marker_order_kernel, sp_prank_kernel,
// gene_order_kernel, listed in tests/test_device_header.py): as a function the loop loses a scalar compare and branch ahead of
// its inner loop (8 bytes, registers equal) and every entry point measures slower, loop / call in us, two processes each:
// mcl_marker_rank_adjust 136.4, 136.5 / 139.5, 139.9 at 785 genes, 502.1, 505.5 / 520.5, 521.1 at 3467; mcl_gene_rank 132.0,
// 132.3 / 136.2, 136.7; mcl_spatial_moments 65.1, 65.1 / 65.7, 65.9
// ---- Benjamini-Hochberg over G p-values ranked ascending (NaN as p = 1, equal p by index): the sorted p G / j
__device__ __forceinline__ void bh_stage(double* __restrict__ scratch, long long base, int rank, double p, int G) {
#pragma clang fp contract(off)
  scratch[base + rank] = p * ((double)G / (double)(rank + 1));
}
// one workgroup of THREADS, all threads: adj[base + g] = the suffix minimum over the sorted scratch[base .. base + G) at g's
// rank, capped at 1 (chunk minima, their suffix min-scan in ``cmin``, THREADS doubles of LDS, then each chunk backwards, in
// place: a minimum is order-free).  KEEP_NAN: a NaN p, ranked as 1 among the others, stays NaN (pvals is read only then)
template <int THREADS, bool KEEP_NAN>
__device__ __forceinline__ void bh_adjust(const double* __restrict__ pvals, const int* __restrict__ prank,
                                          double* __restrict__ scratch, double* __restrict__ adj, long long base, int G,
                                          double* cmin) {
  const int t = threadIdx.x;
  const int ch = (G + THREADS - 1) / THREADS;
  const int i0 = min(G, t * ch), i1 = min(G, i0 + ch);
  double m = INFINITY;
  for (int i = i0; i < i1; ++i) m = fmin(m, scratch[base + i]);
  cmin[t] = m;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const double other = t + o < THREADS ? cmin[t + o] : INFINITY;
    __syncthreads();
    cmin[t] = fmin(cmin[t], other);
    __syncthreads();
  }
  double run = t + 1 < THREADS ? cmin[t + 1] : INFINITY;
  for (int i = i1 - 1; i >= i0; --i) {
    run = fmin(run, scratch[base + i]);
    scratch[base + i] = run;
  }
  __threadfence_block();
  __syncthreads();
  for (int g = t; g < G; g += THREADS)
    adj[base + g] = KEEP_NAN && isnan(pvals[base + g]) ? NAN : fmin(1.0, scratch[base + prank[base + g]]);
}

constexpr int TOP_SAMPLE = 256;    // values in the sample that sets the candidate threshold
constexpr int TOP_CAP = 2048;      // candidates ranked in LDS; more -> ranked against all G values in global memory
template <int THREADS, int SAMPLE = TOP_SAMPLE, int CAP = TOP_CAP>
struct top_lds {
  double smp_v[SAMPLE];
  double cand_v[CAP];
  int smp_g[SAMPLE];
  int cand_g[CAP];
  int wave_cnt[THREADS / 64];
  double thr;
};
// top[rank] = the element of that rank in ORDER for rank < n; an entry no rank reaches -- non-finite values only --
// is left as the caller set it.  One workgroup of THREADS, every thread calls this; L is free again on return.
template <int ORDER, int THREADS, int SAMPLE, int CAP>
__device__ void top_select(const double* __restrict__ val, int G, int n, long long* __restrict__ top,
                           top_lds<THREADS, SAMPLE, CAP>& L) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // 1. threshold T = the n-th largest of an evenly strided sample: the full set's n-th largest is >= T, so every element
  //    of the top n is >= T (T = -inf when the sample holds fewer than n)
  const int ns = min(G, SAMPLE);
  if (tid == 0) L.thr = -INFINITY;
  if (tid < ns) {
    const int gs = (int)(((long long)tid * G) / ns);
    L.smp_v[tid] = val[gs];
    L.smp_g[tid] = gs;
  }
  __syncthreads();
  if (n <= ns && tid < ns) {
    const double vt = L.smp_v[tid];
    const int gt = L.smp_g[tid];
    int rank = 0;
    for (int j = 0; j < ns; ++j) rank += before<ORDER>(L.smp_v[j], L.smp_g[j], vt, gt);
    if (rank == n - 1) L.thr = vt;
  }
  __syncthreads();
  const double T = L.thr;
  // 2. candidates (value >= T) compacted in index order: ballot + a prefix over the waves, no atomics
  int count = 0;
  for (int g0 = 0; g0 < G; g0 += THREADS) {
    const int g = g0 + tid;
    const double vg = val[g < G ? g : G - 1];
    const bool f = g < G && vg >= T;
    const unsigned long long b = __ballot(f);
    if (lane == 0) L.wave_cnt[w] = __builtin_popcountll(b);
    __syncthreads();
    int ahead = count;
    for (int v = 0; v < w; ++v) ahead += L.wave_cnt[v];
    if (f) {
      const int pos = ahead + (int)lanes_below(b);
      if (pos < CAP) {
        L.cand_v[pos] = vg;
        L.cand_g[pos] = g;
      }
    }
    for (int v = 0; v < THREADS / 64; ++v) count += L.wave_cnt[v];
    __syncthreads();
  }
  // 3. exact rank of every candidate among the candidates (a non-candidate is strictly below every candidate)
  if (count <= CAP) {
    for (int c = tid; c < count; c += THREADS) {
      const double vc = L.cand_v[c];
      const int gc = L.cand_g[c];
      int rank = 0;
      for (int j = 0; j < count; ++j) rank += before<ORDER>(L.cand_v[j], L.cand_g[j], vc, gc);
      if (rank < n) top[rank] = gc;
    }
  } else {
    for (int g = tid; g < G; g += THREADS) {
      const double vg = val[g];
      if (!(vg >= T)) continue;
      int rank = 0;
      for (int j = 0; j < G; ++j) rank += before<ORDER>(val[j], j, vg, g);
      if (rank < n) top[rank] = g;
    }
  }
  __syncthreads();  // top[] is read back by the caller
}
}  // namespace stats
