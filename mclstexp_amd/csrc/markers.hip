// Marker genes of spot groups: scanpy's sc.tl.rank_genes_groups(adata, groupby, reference="rest") for every slide of an
// evaluation per call, methods "wilcoxon", "t-test" and "t-test_overestim_var" (DESIGN 6.15 states the arithmetic,
// tests/markers_reference.py restates it in numpy).  x is row-stacked (rows, G) fp32 / fp64 with row stride ld; slide s
// owns rows offsets[s] .. offsets[s + 1]; labels[row] in [0, k[s]) names the row's group, -1 drops the row from everything.
// The groups of all slides are numbered in slide order: group g of slide s is "group row" g0[s] + g, g0 = the exclusive
// prefix sum of k; every per-group output is a (sum k, G) matrix.
//
//   marker_setup_kernel   one workgroup per slide: validates offsets / k / labels (a slide that breaks a limit gets n = 0
//                         and a status count: later kernels write nothing for it and no index leaves its array), g0, the
//                         group sizes, and pos[row] = the row's index among the kept rows of its slide (-1: dropped).
//   marker_moments_kernel grid (genes / 64, group, slide), 64 gene lanes x 4 quarters of the KEPT rows: a quarter is summed
//                         in row order, the four partial sums are combined as (q0 + q1) + (q2 + q3).  Walk 1: sums and non-zero
//                         counts of the group and of the rest (its own sum, not total - group); walk 2: centred squares.
//   marker_rank_kernel    THE HOT PATH.  grid (column tiles, slide), 1024 threads.  A workgroup takes C adjacent gene
//                         columns of one slide -- as many as its LDS holds, at most 32 -- and loads them row segment by
//                         row segment.  The kept values of a column land in LDS as order-preserving integer keys (32-bit
//                         for fp32, 64-bit for fp64; -0.0 maps to +0.0's key) next to a byte with the group id, padded to
//                         a power of two P with the largest key.  A bitonic network sorts all C columns at once: one
//                         thread per compare-exchange, a barrier per stage.  At stride j >= 32 keys the two operands of a
//                         wave are two runs of consecutive words (conflict-free); below, a wave reads every other run of j
//                         words (2-way conflicts at j = 1 .. 16 for 32-bit keys: 15 of the 78 stages at P = 4096).  Then
//                         every sorted position finds its tie run [first, last] by two binary searches (skipped when both
//                         neighbours differ), adds first + last + 2 -- twice its 1-based average rank -- to its group's
//                         int64 slot in LDS, and the first of a run adds t^3 - t.  Integer sums: any order, same bits.
//   marker_test_kernel    one lane per (slide, group, gene): score, p, -log10 p (log space), log fold change.
//   marker_prank_kernel / marker_bh_kernel / marker_order_kernel
//                         Benjamini-Hochberg and the score order per (slide, group) by exact counting ranks against all G
//                         keys (value, gene index), BH by stats.h's bh_adjust: ties go to the lower gene index
//                         without a stable sort.  The suffix minimum of BH is a min-scan (order-free).
// No floating-point atomics, no workgroup waits for another, every fp64 sum's order depends on the slide alone: a slide
// inside a batch is bit-identical to the same slide alone.
#include "common.h"
#include "stats.h"
#include "betacf.h"

namespace {

constexpr int MK_MAX_N = 16384;        // spots per slide: a column's keys and group bytes sit in LDS
constexpr int MK_MAX_K = 255;          // groups per slide: the group byte 255 marks padding
constexpr int MK_MAX_G = 16384;
constexpr int MK_MAX_S = 65535;        // grid.y / grid.z
constexpr int MK_SETUP_THREADS = 256;
constexpr int MK_MOM_THREADS = 256;    // 64 gene lanes x 4 row quarters
constexpr int MK_RANK_THREADS = 1024;
constexpr int MK_CMAX = 32;            // columns per workgroup
constexpr int MK_KEY_BUDGET = 65536;   // LDS for keys + group bytes while one column fits it (two workgroups per CU)
constexpr int MK_ACC_SLOTS = 1024;     // int64 rank-sum slots: C * k <= 1024
constexpr int MK_T_THREADS = 256;
constexpr int MK_O_THREADS = 256;
constexpr int MK_BH_THREADS = 1024;

struct mk_slide {          // 32 bytes, written by marker_setup_kernel, read by everything after it
  long long row0;          // first row
  long long g0;            // first group row
  int n;                   // rows (0: the slide is skipped)
  int k;                   // groups (0: skipped)
  int nvalid;              // rows with a label >= 0
  int pad;
};

__host__ __device__ inline long long mk_align8(long long v) { return (v + 7) & ~7ll; }
// workspace layout: slide records | pos int32[rows] | rowof int32[rows] | prank int32[KT * G] | scratch double[KT * G]
struct mk_work {
  mk_slide* info;
  int* pos;      // row -> index among the kept rows of its slide, -1: dropped
  int* rowof;    // slide's first row + kept index -> row within the slide
  int* prank;
  double* scratch;
};
__host__ __device__ inline mk_work mk_carve(void* work, long long S, long long rows, long long KT, long long G) {
  char* p = static_cast<char*>(work);
  mk_work w;
  w.info = reinterpret_cast<mk_slide*>(p);
  p += mk_align8(S * (long long)sizeof(mk_slide));
  w.pos = reinterpret_cast<int*>(p);
  p += mk_align8(rows * 4);
  w.rowof = reinterpret_cast<int*>(p);
  p += mk_align8(rows * 4);
  w.prank = reinterpret_cast<int*>(p);
  p += mk_align8(KT * G * 4);
  w.scratch = reinterpret_cast<double*>(p);
  return w;
}
inline long long mk_work_bytes(long long S, long long rows, long long KT, long long G) {
  return mk_align8(S * (long long)sizeof(mk_slide)) + 2 * mk_align8(rows * 4) + mk_align8(KT * G * 4) + KT * G * 8;
}

__host__ __device__ inline int mk_pow2ceil(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
// columns a workgroup takes: what the key region holds, at most MK_CMAX, and C * k rank-sum slots
__host__ __device__ inline int mk_columns(int lds_keys, int n, int k, int keysize) {
  const int percol = mk_pow2ceil(n) * (keysize + 1);
  int c = lds_keys / percol;
  if (c > MK_CMAX) c = MK_CMAX;
  if (c > MK_ACC_SLOTS / k) c = MK_ACC_SLOTS / k;
  return c < 1 ? 1 : c;
}

// ------------------------------------------------------------------------------------------------------------ setup
__global__ __launch_bounds__(MK_SETUP_THREADS) void marker_setup_kernel(
    const long long* __restrict__ offsets, const int* __restrict__ labels, const int* __restrict__ kk, int S, long long rows,
    int max_n, int kmax, long long KT, mk_slide* __restrict__ info, int* __restrict__ pos, int* __restrict__ rowof,
    int* __restrict__ gsize,
    int* __restrict__ nvalid_out, int* __restrict__ status) {
  __shared__ long long red[MK_SETUP_THREADS];
  __shared__ int cnt[256];
  __shared__ int scan[MK_SETUP_THREADS];
  __shared__ int bad_s;
  const int s = blockIdx.x, t = threadIdx.x;
  // g0 = sum of the (clamped) k of the slides before this one: integers, any order
  long long part = 0;
  for (int q = t; q < s; q += MK_SETUP_THREADS) {
    const int kq = kk[q];
    part += (kq >= 1 && kq <= kmax) ? kq : 0;
  }
  red[t] = part;
  cnt[t] = 0;
  if (t == 0) bad_s = 0;
  __syncthreads();
  for (int o = MK_SETUP_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const long long g0 = red[0];
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  int k = kk[s];
  int config_bad = 0;
  if (k < 1 || k > kmax || g0 + k > KT) { k = 0; config_bad = 1; }
  int n = 0;
  if (r0 >= 0 && r1 >= r0 && r1 <= rows && r1 - r0 >= 2 && r1 - r0 <= max_n) n = (int)(r1 - r0);
  else config_bad = 1;
  // pos: this thread owns the rows [t ch, (t + 1) ch)
  const int ch = (n + MK_SETUP_THREADS - 1) / MK_SETUP_THREADS;
  const int i0 = min(n, t * ch), i1 = min(n, i0 + ch);
  int valid = 0, bad = 0;
  for (int i = i0; i < i1; ++i) {
    const int lab = labels[r0 + i];
    if (lab >= 0 && lab < k) {
      ++valid;
      atomicAdd(&cnt[lab], 1);
    } else if (lab != -1) {
      ++bad;
    }
  }
  scan[t] = valid;
  if (bad) atomicAdd(&bad_s, bad);
  __syncthreads();
  if (t == 0) {                                  // 256 integers: an exclusive scan in place
    int run = 0;
    for (int q = 0; q < MK_SETUP_THREADS; ++q) {
      const int v = scan[q];
      scan[q] = run;
      run += v;
    }
    mk_slide rec;
    rec.row0 = r0;
    rec.g0 = g0;
    rec.n = n;
    rec.k = n ? k : 0;
    rec.nvalid = run;
    rec.pad = 0;
    info[s] = rec;
    nvalid_out[s] = run;
    status[2 * s] = 0;
    status[2 * s + 1] = bad_s + config_bad;
  }
  __syncthreads();
  int p = scan[t];
  for (int i = i0; i < i1; ++i) {
    const int lab = labels[r0 + i];
    const bool kept = lab >= 0 && lab < k;
    if (kept) rowof[r0 + p] = i;
    pos[r0 + i] = kept ? p++ : -1;
  }
  if (n && t < k) gsize[g0 + t] = cnt[t];
}

// ---------------------------------------------------------------------------------------------------------- moments
template <typename T>
__global__ __launch_bounds__(MK_MOM_THREADS) void marker_moments_kernel(
    const T* __restrict__ x, long long ld, const int* __restrict__ labels, const mk_slide* __restrict__ info,
    const int* __restrict__ rowof, const int* __restrict__ gsize, int G, double* __restrict__ mean_g,
    double* __restrict__ var_g, double* __restrict__ mean_r, double* __restrict__ var_r, double* __restrict__ pts_g,
    double* __restrict__ pts_r, int* __restrict__ nnz_g, int* __restrict__ nnz_r, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double pa[4][64], pb[4][64];
  __shared__ int za[4][64], zb[4][64];
  __shared__ double mg_s[64], mr_s[64];
  __shared__ int nonfinite_s;
  const mk_slide inf = info[blockIdx.z];
  const int g = blockIdx.y;
  if (g >= inf.k) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int jc = j < G ? j : G - 1;
  const int n = inf.nvalid, ch = (n + 3) / 4;          // quarters of the kept rows: dropped rows change no sum's order
  const int i0 = min(n, w * ch), i1 = min(n, i0 + ch);
  const T* xs = x + inf.row0 * ld + jc;
  const int* labs = labels + inf.row0;
  const int* rows_ = rowof + inf.row0;
  if (threadIdx.x == 0) nonfinite_s = 0;
  double sg = 0.0, sr = 0.0;
  int zg = 0, zr = 0, nf = 0;
  for (int q = i0; q < i1; ++q) {
    const int i = rows_[q], lab = labs[i];
    const double v = ldd(xs + (long long)i * ld);
    nf += !isfinite(v);
    if (lab == g) { sg = sg + v; zg += v != 0.0; }
    else { sr = sr + v; zr += v != 0.0; }
  }
  pa[w][lane] = sg; pb[w][lane] = sr; za[w][lane] = zg; zb[w][lane] = zr;
  __syncthreads();
  if (g == 0 && j < G && nf) atomicAdd(&nonfinite_s, nf);
  const int ng = gsize[inf.g0 + g], nr = inf.nvalid - ng;
  if (w == 0) {
    mg_s[lane] = ((pa[0][lane] + pa[1][lane]) + (pa[2][lane] + pa[3][lane])) / (double)ng;
    mr_s[lane] = ((pb[0][lane] + pb[1][lane]) + (pb[2][lane] + pb[3][lane])) / (double)nr;
  }
  __syncthreads();
  const double mg = mg_s[lane], mr = mr_s[lane];
  const int tzg = za[0][lane] + za[1][lane] + za[2][lane] + za[3][lane];
  const int tzr = zb[0][lane] + zb[1][lane] + zb[2][lane] + zb[3][lane];
  double qg = 0.0, qr = 0.0;
  for (int q = i0; q < i1; ++q) {
    const int i = rows_[q], lab = labs[i];
    const double v = ldd(xs + (long long)i * ld);
    if (lab == g) { const double d = v - mg; const double sq = d * d; qg = qg + sq; }
    else { const double d = v - mr; const double sq = d * d; qr = qr + sq; }
  }
  __syncthreads();                       // (pa / pb are read above by wave 0 only before the second barrier)
  pa[w][lane] = qg; pb[w][lane] = qr;
  __syncthreads();
  if (w == 0 && j < G) {
    const long long o = (inf.g0 + g) * (long long)G + j;
    const double tg = (pa[0][lane] + pa[1][lane]) + (pa[2][lane] + pa[3][lane]);
    const double tr = (pb[0][lane] + pb[1][lane]) + (pb[2][lane] + pb[3][lane]);
    mean_g[o] = mg;
    mean_r[o] = mr;
    var_g[o] = ng >= 2 ? tg / (double)(ng - 1) : NAN;
    var_r[o] = nr >= 2 ? tr / (double)(nr - 1) : NAN;
    pts_g[o] = (double)tzg / (double)ng;
    pts_r[o] = (double)tzr / (double)nr;
    nnz_g[o] = tzg;
    nnz_r[o] = tzr;
  }
  if (threadIdx.x == 0 && nonfinite_s) atomicAdd(&status[2 * blockIdx.z], nonfinite_s);
}

// ------------------------------------------------------------------------------------------------------------- ranks
// the order-preserving integer image of a value; -0.0 and +0.0 share one key, unlike device.h's order_key (written through
// it, order_key(v == 0 ? 0 : v), the code of this file's kernels changes)
__device__ __forceinline__ unsigned mk_key(float v) {
  const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long mk_key(double v) {
  const unsigned long long u = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
template <typename T> struct mk_keytype;
template <> struct mk_keytype<float> { typedef unsigned type; };
template <> struct mk_keytype<double> { typedef unsigned long long type; };

template <typename T>
__global__ __launch_bounds__(MK_RANK_THREADS) void marker_rank_kernel(
    const T* __restrict__ x, long long ld, const int* __restrict__ labels, const mk_slide* __restrict__ info,
    const int* __restrict__ pos, int G, int lds_keys, long long* __restrict__ R2, long long* __restrict__ Tt) {
  typedef typename mk_keytype<T>::type K;
  extern __shared__ __align__(16) unsigned char mk_lds[];
  const mk_slide inf = info[blockIdx.y];
  const int n = inf.n, k = inf.k, N = inf.nvalid;
  if (n == 0 || k == 0) return;
  const int P = mk_pow2ceil(n);
  const int C = mk_columns(lds_keys, n, k, (int)sizeof(K));
  const int j0 = blockIdx.x * C;
  if (j0 >= G) return;
  const int Cc = min(C, G - j0);
  const int lp = 31 - __clz(P);                              // log2 P
  K* keys = reinterpret_cast<K*>(mk_lds);                    // [Cc][P]
  unsigned char* grp = mk_lds + (size_t)C * P * sizeof(K);   // [Cc][P]
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(mk_lds + lds_keys);   // [Cc][k] then ties [MK_CMAX]
  unsigned long long* tie = acc + MK_ACC_SLOTS;
  const int tid = threadIdx.x;

  for (int e = tid; e < Cc * P; e += MK_RANK_THREADS) {      // padding: the largest key, group byte 255
    if ((e & (P - 1)) >= N) { keys[e] = ~(K)0; grp[e] = 255; }
  }
  for (int e = tid; e < Cc * k; e += MK_RANK_THREADS) acc[e] = 0;
  if (tid < MK_CMAX) tie[tid] = 0;
  // whole row segments: consecutive threads read the Cc adjacent columns of one row
  const T* xs = x + inf.row0 * ld + j0;
  const int total = n * Cc;
  for (int e = tid; e < total; e += MK_RANK_THREADS) {
    const int i = e / Cc, c = e - i * Cc;
    const int ps = pos[inf.row0 + i], lab = labels[inf.row0 + i];
    const T v = xs[(long long)i * ld + c];
    if (ps >= 0) {
      keys[(c << lp) + ps] = mk_key(v);
      grp[(c << lp) + ps] = (unsigned char)lab;
    }
  }
  __syncthreads();

  const int pairs = Cc << (lp - 1);
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < pairs; q += MK_RANK_THREADS) {
        const int c = q >> (lp - 1), r = q & ((P >> 1) - 1);
        const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1));
        const int a = (c << lp) + i, b = a + j;
        const K ka = keys[a], kb = keys[b];
        const bool up = (i & k2) == 0;
        if ((ka > kb) == up && ka != kb) {
          keys[a] = kb; keys[b] = ka;
          const unsigned char ga = grp[a], gb = grp[b];
          grp[a] = gb; grp[b] = ga;
        }
      }
      __syncthreads();
    }
  }

  for (int e = tid; e < Cc * P; e += MK_RANK_THREADS) {
    const int c = e >> lp, p = e & (P - 1);
    if (p >= N) continue;
    const K* col = keys + (c << lp);
    const K kv = col[p];
    int first = p, last = p;
    if (p > 0 && col[p - 1] == kv) {                         // lower bound in [0, p)
      int lo = 0, hi = p - 1;                                // col[hi] == kv
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < kv) lo = mid + 1; else hi = mid;
      }
      first = lo;
    }
    if (p + 1 < N && col[p + 1] == kv) {                     // last equal in (p, N)
      int lo = p + 1, hi = N - 1;                            // col[lo] == kv
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (col[mid] > kv) hi = mid - 1; else lo = mid;
      }
      last = lo;
    }
    const int gi = grp[e];
    if (gi < k) atomicAdd(&acc[c * k + gi], (unsigned long long)(first + last + 2));
    if (p == first && last > first) {
      const unsigned long long t = (unsigned long long)(last - first + 1);
      atomicAdd(&tie[c], t * t * t - t);
    }
  }
  __syncthreads();
  for (int e = tid; e < Cc * k; e += MK_RANK_THREADS) {
    const int g = e / Cc, c = e - g * Cc;
    R2[(inf.g0 + g) * (long long)G + j0 + c] = (long long)acc[c * k + g];
  }
  if (tid < Cc) Tt[(long long)blockIdx.y * G + j0 + tid] = (long long)tie[tid];
}

// -------------------------------------------------------------------------------------------------------------- test
constexpr double MK_LGAMMA_HALF = 0.5723649429247001;     // log sqrt(pi)

// two-sided p of Student's t with nu degrees of freedom, I_{nu / (nu + t^2)}(nu / 2, 1 / 2), and -log10 p in log space
__device__ void mk_student_p(double t, double nu, double* p_out, double* nl_out) {
  const double t2 = t * t, a = 0.5 * nu, b = 0.5;
  if (t2 == 0.0) { *p_out = 1.0; *nl_out = 0.0; return; }
  if (isinf(t2)) { *p_out = 0.0; *nl_out = INFINITY; return; }
  const double x = nu / (nu + t2);
  const double logx = -log1p(t2 / nu), logy = -log1p(nu / t2);           // log x, log(1 - x)
  const double logB = (lgamma(a) + MK_LGAMMA_HALF) - lgamma(a + b);
  if (x < (a + 1.0) / (a + b + 2.0)) {
    double lp = ((a * logx + b * logy) - log(a) - logB) + log_betacf(a, b, x);
    lp = lp > 0.0 ? 0.0 : lp;
    *p_out = exp(lp);
    *nl_out = 0.0 - lp / stats::LN10;
  } else {                                                               // p = 1 - I_{1 - x}(1 / 2, nu / 2)
    const double y = t2 / (nu + t2);
    double lq = ((b * logy + a * logx) - log(b) - logB) + log_betacf(b, a, y);
    lq = lq > 0.0 ? 0.0 : lq;
    *p_out = 0.0 - expm1(lq);
    *nl_out = 0.0 - log1p(0.0 - exp(lq)) / stats::LN10;
  }
}

__global__ __launch_bounds__(MK_T_THREADS) void marker_test_kernel(
    int method, int tie_correct, const mk_slide* __restrict__ info, const int* __restrict__ gsize, int G,
    const double* __restrict__ mean_g, const double* __restrict__ var_g, const double* __restrict__ mean_r,
    const double* __restrict__ var_r, const long long* __restrict__ R2, const long long* __restrict__ Tt,
    double* __restrict__ scores, double* __restrict__ pvals, double* __restrict__ nlp, double* __restrict__ lfc) {
#pragma clang fp contract(off)
  const mk_slide inf = info[blockIdx.z];
  const int g = blockIdx.y;
  if (g >= inf.k) return;
  const int j = blockIdx.x * MK_T_THREADS + threadIdx.x;
  if (j >= G) return;
  const long long o = (inf.g0 + g) * (long long)G + j;
  const long long N = inf.nvalid, ng = gsize[inf.g0 + g], nr = N - ng;
  const double mg = mean_g[o], mr = mean_r[o];
  double score, p, nl;
  if (method == 0) {
    const long long num2 = R2[o] - ng * (N + 1);                       // exact: twice the centred rank sum
    const double prod = (double)(ng * nr * (N + 1));                   // < 2^53: exact
    double c = 1.0;
    if (tie_correct) {
      const long long n3 = N * N * N - N;
      c = (double)(n3 - Tt[(long long)blockIdx.z * G + j]) / (double)n3;   // 1 - T / (N^3 - N), one rounding
    }
    const double den = sqrt(c * prod / 12.0);
    double z = (0.5 * (double)num2) / den;
    if (!(den > 0.0) || isnan(z)) z = 0.0;
    score = z;
    stats::normal_tail(z, 1, &p, &nl);
  } else {
    const double nrr = method == 2 ? (double)ng : (double)nr;
    const double vg = var_g[o] / (double)ng, vr = var_r[o] / nrr;
    const double sum = vg + vr;
    const double t = (mg - mr) / sqrt(sum);
    const double nu = (sum * sum) / ((vg * vg) / ((double)ng - 1.0) + (vr * vr) / (nrr - 1.0));
    if (isnan(t) || isnan(nu)) {
      score = 0.0; p = 1.0; nl = 0.0;
    } else {
      score = t;
      mk_student_p(t, nu, &p, &nl);
      if (isnan(p)) { p = 1.0; nl = 0.0; }
    }
  }
  scores[o] = score;
  pvals[o] = p;
  nlp[o] = nl;
  lfc[o] = log2((expm1(mg) + 1e-9) / (expm1(mr) + 1e-9));
}

// --------------------------------------------------------------------------------------------- BH and the score order
// rank of every gene's p ascending (NaN as 1, equal p by gene index); scratch[rank] = p G / (rank + 1)
// (the counting loop is written out in every kernel that has it: stats.h says why it holds no shared form)
__global__ __launch_bounds__(MK_O_THREADS) void marker_prank_kernel(const mk_slide* __restrict__ info, int G,
                                                                    const double* __restrict__ pvals,
                                                                    int* __restrict__ prank, double* __restrict__ scratch) {
  __shared__ double tile[MK_O_THREADS];
  const mk_slide inf = info[blockIdx.z];
  if ((int)blockIdx.y >= inf.k) return;
  const long long base = (inf.g0 + blockIdx.y) * (long long)G;
  const int g = blockIdx.x * MK_O_THREADS + threadIdx.x;
  double p = pvals[base + (g < G ? g : G - 1)];
  if (isnan(p)) p = 1.0;
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += MK_O_THREADS) {
    const int j = j0 + threadIdx.x;
    const double pj = pvals[base + (j < G ? j : G - 1)];
    tile[threadIdx.x] = isnan(pj) ? 1.0 : pj;
    __syncthreads();
    const int cnt = min(MK_O_THREADS, G - j0);
    for (int q = 0; q < cnt; ++q) rank += (tile[q] < p) || (tile[q] == p && j0 + q < g);
    __syncthreads();
  }
  if (g < G) {
    prank[base + g] = rank;
    stats::bh_stage(scratch, base, rank, p, G);
  }
}

// one workgroup per (slide, group): suffix minimum over the sorted p G / j, capped at 1, scattered back to gene order
__global__ __launch_bounds__(MK_BH_THREADS) void marker_bh_kernel(const mk_slide* __restrict__ info, int G,
                                                                  const int* __restrict__ prank,
                                                                  double* __restrict__ scratch, double* __restrict__ adj) {
  __shared__ double cmin[MK_BH_THREADS];
  const mk_slide inf = info[blockIdx.y];
  if ((int)blockIdx.x >= inf.k) return;
  const long long base = (inf.g0 + blockIdx.x) * (long long)G;
  stats::bh_adjust<MK_BH_THREADS, false>(nullptr, prank, scratch, adj, base, G, cmin);
}

// rank of every gene by descending score (or |score|), equal scores by gene index; the first n_genes are gathered
// (the counting loop is written out in every kernel that has it: stats.h says why it holds no shared form)
__global__ __launch_bounds__(MK_O_THREADS) void marker_order_kernel(
    const mk_slide* __restrict__ info, int G, int n_genes, int rankby_abs, const double* __restrict__ scores,
    const double* __restrict__ pvals, const double* __restrict__ adj, const double* __restrict__ nlp,
    const double* __restrict__ lfc, long long* __restrict__ names, double* __restrict__ o_scores,
    double* __restrict__ o_pvals, double* __restrict__ o_adj, double* __restrict__ o_nlp, double* __restrict__ o_lfc) {
  __shared__ double tile[MK_O_THREADS];
  const mk_slide inf = info[blockIdx.z];
  if ((int)blockIdx.y >= inf.k) return;
  const long long row = inf.g0 + blockIdx.y, base = row * (long long)G;
  const int g = blockIdx.x * MK_O_THREADS + threadIdx.x;
  double v = scores[base + (g < G ? g : G - 1)];
  if (rankby_abs) v = fabs(v);
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += MK_O_THREADS) {
    const int j = j0 + threadIdx.x;
    const double vj = scores[base + (j < G ? j : G - 1)];
    tile[threadIdx.x] = rankby_abs ? fabs(vj) : vj;
    __syncthreads();
    const int cnt = min(MK_O_THREADS, G - j0);
    for (int q = 0; q < cnt; ++q) rank += (tile[q] > v) || (tile[q] == v && j0 + q < g);
    __syncthreads();
  }
  if (g < G && rank < n_genes) {
    const long long o = row * (long long)n_genes + rank;
    names[o] = g;
    o_scores[o] = scores[base + g];
    o_pvals[o] = pvals[base + g];
    o_adj[o] = adj[base + g];
    o_nlp[o] = nlp[base + g];
    o_lfc[o] = lfc[base + g];
  }
}

inline bool mk_shape_ok(int32_t S, int64_t rows, int32_t G, int32_t max_n, int32_t kmax, int64_t KT) {
  return S >= 1 && S <= MK_MAX_S && rows >= 2 && rows <= (int64_t)S * max_n && G >= 1 && G <= MK_MAX_G && max_n >= 2 &&
         max_n <= MK_MAX_N && kmax >= 1 && kmax <= MK_MAX_K && KT >= S && KT <= (int64_t)S * kmax;
}

// the LDS of a rank launch: the key region (one column of the largest slide, or the 64 KiB budget), then the slots
inline int mk_lds_keys(int max_n, int keysize) {
  const int percol = mk_pow2ceil(max_n) * (keysize + 1);
  return percol > MK_KEY_BUDGET ? percol : MK_KEY_BUDGET;
}

template <typename T>
int mk_launch_rank(const void* x, int64_t ld, const int32_t* labels, const mk_work& w, int S, int G, int max_n, int kmax,
                   int64_t* R2, int64_t* Tt, hipStream_t st) {
  const int keysize = (int)sizeof(typename mk_keytype<T>::type);
  const int lds_keys = mk_lds_keys(max_n, keysize);
  const size_t lds = (size_t)lds_keys + (MK_ACC_SLOTS + MK_CMAX) * 8;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(marker_rank_kernel<T>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, MK_MAX_N * 9 + (MK_ACC_SLOTS + MK_CMAX) * 8);
  }
  const int cmin = mk_columns(lds_keys, max_n, kmax, keysize);     // no slide takes fewer columns than this
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(marker_rank_kernel<T>, dim3((G + cmin - 1) / cmin, S), dim3(MK_RANK_THREADS), lds, st,
                     static_cast<const T*>(x), (long long)ld, labels, w.info, w.pos, G, lds_keys,
                     reinterpret_cast<long long*>(R2), reinterpret_cast<long long*>(Tt));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // namespace

extern "C" int64_t mcl_marker_workspace_bytes(int64_t rows, int64_t groups_total, int32_t S, int32_t G) {
  if (rows < 2 || groups_total < 1 || S < 1 || S > MK_MAX_S || G < 1 || G > MK_MAX_G) return -1;
  if (rows > (int64_t)S * MK_MAX_N || groups_total > (int64_t)S * MK_MAX_K) return -1;
  return mk_work_bytes(S, rows, groups_total, G);
}

extern "C" int mcl_marker_stats(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, const int32_t* labels,
                                const int32_t* k, int32_t S, int64_t rows, int32_t G, int32_t max_n, int32_t kmax,
                                int64_t groups_total, void* work, int32_t* group_sizes, int32_t* n_valid, double* mean_g,
                                double* var_g, double* mean_r, double* var_r, double* pts_g, double* pts_r,
                                int32_t* nnz_g, int32_t* nnz_r, int32_t* status, mcl_stream_t stream) {
  if (!x || !offsets || !labels || !k || !work || !group_sizes || !n_valid || !mean_g || !var_g || !mean_r || !var_r ||
      !pts_g || !pts_r || !nnz_g || !nnz_r || !status)
    return MCL_EINVAL;
  if (!mk_shape_ok(S, rows, G, max_n, kmax, groups_total) || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const mk_work w = mk_carve(work, S, rows, groups_total, G);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(marker_setup_kernel, dim3(S), dim3(MK_SETUP_THREADS), 0, st,
                     reinterpret_cast<const long long*>(offsets), labels, k, S, (long long)rows, max_n, kmax,
                     (long long)groups_total, w.info, w.pos, w.rowof, group_sizes, n_valid, status);
  MCL_CHECK_LAUNCH();
  const dim3 grid((G + 63) / 64, kmax, S);
  if (dtype == 0)
    hipLaunchKernelGGL(marker_moments_kernel<float>, grid, dim3(MK_MOM_THREADS), 0, st, static_cast<const float*>(x),
                       (long long)ld, labels, w.info, w.rowof, group_sizes, G, mean_g, var_g, mean_r, var_r, pts_g, pts_r,
                       nnz_g, nnz_r, status);
  else
    hipLaunchKernelGGL(marker_moments_kernel<double>, grid, dim3(MK_MOM_THREADS), 0, st, static_cast<const double*>(x),
                       (long long)ld, labels, w.info, w.rowof, group_sizes, G, mean_g, var_g, mean_r, var_r, pts_g, pts_r,
                       nnz_g, nnz_r, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_marker_rank_sums(const void* x, int64_t ld, int32_t dtype, const int32_t* labels, int32_t S,
                                    int64_t rows, int32_t G, int32_t max_n, int32_t kmax, int64_t groups_total, void* work,
                                    int64_t* rank_sums2, int64_t* tie_terms, mcl_stream_t stream) {
  if (!x || !labels || !work || !rank_sums2 || !tie_terms) return MCL_EINVAL;
  if (!mk_shape_ok(S, rows, G, max_n, kmax, groups_total) || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const mk_work w = mk_carve(work, S, rows, groups_total, G);
  return dtype == 0 ? mk_launch_rank<float>(x, ld, labels, w, S, G, max_n, kmax, rank_sums2, tie_terms, st)
                    : mk_launch_rank<double>(x, ld, labels, w, S, G, max_n, kmax, rank_sums2, tie_terms, st);
}

extern "C" int mcl_marker_test(int32_t method, int32_t tie_correct, int32_t S, int64_t rows, int32_t G, int32_t kmax,
                               int64_t groups_total, const void* work, const int32_t* group_sizes, const double* mean_g,
                               const double* var_g, const double* mean_r, const double* var_r, const int64_t* rank_sums2,
                               const int64_t* tie_terms, double* scores, double* pvals, double* neglog10_pvals,
                               double* logfoldchanges, mcl_stream_t stream) {
  if (!work || !group_sizes || !mean_g || !var_g || !mean_r || !var_r || !scores || !pvals || !neglog10_pvals ||
      !logfoldchanges)
    return MCL_EINVAL;
  if (method < 0 || method > 2 || (method == 0 && (!rank_sums2 || !tie_terms))) return MCL_EINVAL;
  if (!mk_shape_ok(S, rows, G, MK_MAX_N, kmax, groups_total)) return MCL_EINVAL;
  const mk_work w = mk_carve(const_cast<void*>(work), S, rows, groups_total, G);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(marker_test_kernel, dim3((G + MK_T_THREADS - 1) / MK_T_THREADS, kmax, S), dim3(MK_T_THREADS), 0,
                     static_cast<hipStream_t>(stream), method, tie_correct != 0, w.info, group_sizes, G, mean_g, var_g,
                     mean_r, var_r, reinterpret_cast<const long long*>(rank_sums2),
                     reinterpret_cast<const long long*>(tie_terms), scores, pvals, neglog10_pvals, logfoldchanges);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_marker_rank_adjust(int32_t S, int64_t rows, int32_t G, int32_t kmax, int64_t groups_total,
                                      int32_t n_genes, int32_t rankby_abs, void* work, const double* scores,
                                      const double* pvals, const double* neglog10_pvals, const double* logfoldchanges,
                                      double* pvals_adj, int64_t* names, double* top_scores, double* top_pvals,
                                      double* top_pvals_adj, double* top_neglog10_pvals, double* top_logfoldchanges,
                                      mcl_stream_t stream) {
  if (!work || !scores || !pvals || !neglog10_pvals || !logfoldchanges || !pvals_adj || !names || !top_scores ||
      !top_pvals || !top_pvals_adj || !top_neglog10_pvals || !top_logfoldchanges)
    return MCL_EINVAL;
  if (!mk_shape_ok(S, rows, G, MK_MAX_N, kmax, groups_total) || n_genes < 1 || n_genes > G) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const mk_work w = mk_carve(work, S, rows, groups_total, G);
  const dim3 grid((G + MK_O_THREADS - 1) / MK_O_THREADS, kmax, S);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(marker_prank_kernel, grid, dim3(MK_O_THREADS), 0, st, w.info, G, pvals, w.prank, w.scratch);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(marker_bh_kernel, dim3(kmax, S), dim3(MK_BH_THREADS), 0, st, w.info, G, w.prank, w.scratch,
                     pvals_adj);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(marker_order_kernel, grid, dim3(MK_O_THREADS), 0, st, w.info, G, n_genes, rankby_abs != 0, scores,
                     pvals, pvals_adj, neglog10_pvals, logfoldchanges, reinterpret_cast<long long*>(names), top_scores,
                     top_pvals, top_pvals_adj, top_neglog10_pvals, top_logfoldchanges);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
