// Rank agreement of a predicted against a measured expression matrix: Spearman's rho and Kendall's tau-b, the two values
// of ``func`` the reference's get_R(data1, data2, dim, func) (utils.py:52-65) is called with besides pearsonr, on both of
// its ``dim``s (DESIGN 6.23 states the arithmetic, tests/rank_reference.py restates it with Python integers).
//
// A PROBLEM is one pair of vectors.  axis 0 (genes, the reference's dim=1): problem (s, g) = column g of pred against column
// g of truth over the n spots of slide s; axis 1 (spots, dim=0): problem i = row i of pred against row i of truth over the G
// genes.  Both run the same kernels through (element stride, problem stride): (ld, 1) for genes, (1, ld) for spots.
//
//   rank_pair_kernel    THE HOT PATH.  grid (problem tiles, slide), 1024 threads.  A workgroup takes C adjacent problems --
//                       as many as its LDS holds, at most 32.  For pred and then for truth it lays order-preserving integer
//                       keys (32-bit for fp32, 64-bit for fp64; -0.0 shares +0.0's key) beside a uint16 payload, padded to
//                       a power of two P with the largest key, and sorts all C problems at once with a bitonic network (one
//                       thread per compare-exchange, a barrier per stage).  Every sorted position finds its tie run
//                       [first, last] by two binary searches and a = first + last + 2, twice its 1-based average rank.
//                       Sort 1 carries the original index and scatters a_x back by it; sort 2 carries a_x itself, so that
//                       after it position p holds the pair (a_x, a_y) of one element -- in truth's order, which no sum
//                       below depends on.  Per problem, in LDS, exact integers only (integer atomics: any order, same bits):
//                       Sxy = sum a_x a_y, and per side sum (t^3 - t), sum t(t-1)/2, sum t(t-1)(t-2), sum t(t-1)(2t+5) over
//                       the tie runs t.  With tau: the pairs packed as one uint32 (a_x | a_y << 16) over the spent keys, a
//                       thread owns element i of a 64-element block and walks j > i -- all lanes read the same j, a
//                       broadcast read made scalar by readfirstlane -- summing sign(a_x[i] - a_x[j]) sign(a_y[i] - a_y[j])
//                       (a 24-bit product clamped to -1 .. 1) into s and counting equal pairs (the joint ties).  O(n^2) on
//                       purpose: no merge sort, no cross-lane traffic in the loop; the ranks never leave LDS.
//   rank_finish_kernel  one lane per problem, fp64 without contraction: rho, tau-b, Kendall's asymptotic p and -log10 p (log
//                       space).  Spearman's p is Student's t with n - 2 degrees of freedom on rho, the arithmetic of
//                       mcl_pearson_pvalue (gene_significance.hip), which the caller runs on rho.
//   rank_summary_kernel one workgroup per slide: the mean rho / tau over the HEG genes (NaN propagates, np.mean) and over the
//                       defined genes, each summed in gene-index order by one lane over LDS tiles.
// LDS plan per problem: P keys (4 or 8 bytes: 8 when either side is fp64) + two uint16 arrays of P.  One problem of 16384
// fp32 elements takes 128 KiB, one of 8192 elements with an fp64 side 96 KiB: those are the limits (an fp64 side at 16384
// would need 192 KiB).  No floating-point atomics, no workgroup waits for another; every output of a problem is a function of
// its own two vectors: a slide inside a batch is bit-identical to it alone, a row-permuted slide gives the same bits.
#include "common.h"
#include "stats.h"

namespace {

constexpr int RK_MAX_N32 = 16384;      // elements per vector, both sides fp32
constexpr int RK_MAX_N64 = 8192;       // with an fp64 side
constexpr int RK_MAX_G = 16384;
constexpr int RK_MAX_S = 65535;        // grid.y
constexpr int RK_THREADS = 1024;
constexpr int RK_CMAX = 32;            // problems per workgroup
constexpr int RK_KEY_BUDGET = 65536;   // LDS for keys + payloads while one problem fits it (two workgroups per CU)
constexpr int RK_INTS = 12;            // int64 per problem: n, Sxy, Tx, Ty, xtie, ytie, x0, y0, x1, y1, joint, s
constexpr int RK_STATUS = 3;           // int32 per slide: non-finite values, 0x7fffffff - the first problem holding one, refused
constexpr int RK_F_THREADS = 256;
constexpr int RK_S_THREADS = 256;
constexpr int RK_S_TILE = 1024;

enum { I_N, I_SXY, I_TX, I_TY, I_XTIE, I_YTIE, I_X0, I_Y0, I_X1, I_Y1, I_JOINT, I_S };

__host__ __device__ inline int rk_pow2ceil(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
// problems a workgroup takes: what the key region holds, at most RK_CMAX
__host__ __device__ inline int rk_columns(int lds_keys, int n, int keysize) {
  const int c = lds_keys / (rk_pow2ceil(n) * (keysize + 4));
  return c > RK_CMAX ? RK_CMAX : (c < 1 ? 1 : c);
}
inline int rk_lds_keys(int max_n, int keysize) {
  const int one = rk_pow2ceil(max_n) * (keysize + 4);
  return one > RK_KEY_BUDGET ? one : RK_KEY_BUDGET;
}

template <typename T> struct rk_keytype;
template <> struct rk_keytype<float> { typedef unsigned type; };
template <> struct rk_keytype<double> { typedef u64 type; };

// keys of the Cc problems' elements and the padding (largest key); ``pay`` is left alone.  Consecutive lanes read
// consecutive addresses: along the problems where they are adjacent in memory (estride > 1), else along the elements.
template <typename T>
__device__ __forceinline__ void rk_load(const T* __restrict__ v, long long estride, long long pstride, int n, int Cc, int lp,
                                        typename rk_keytype<T>::type* keys, int* status, int q0) {
  typedef typename rk_keytype<T>::type K;
  const int P = 1 << lp, tid = threadIdx.x;
  for (int e = tid; e < Cc << lp; e += RK_THREADS) {
    if ((e & (P - 1)) >= n) keys[e] = ~(K)0;
  }
  const int total = n * Cc;
  const bool along_problems = pstride == 1;
  for (int e = tid; e < total; e += RK_THREADS) {
    int i, c;
    if (along_problems) { i = e / Cc; c = e - i * Cc; } else { c = e / n; i = e - c * n; }
    const T x = v[(long long)i * estride + (long long)c * pstride];
    if (!(fabs((double)x) <= DBL_MAX)) {                     // NaN or infinite: a status word, never a fault
      atomicAdd(&status[0], 1);
      atomicMax(&status[1], 0x7fffffff - (q0 + c));
    }
    keys[(c << lp) + i] = order_key(x == (T)0 ? (T)0 : x);
  }
}

// the bitonic network over Cc problems of P keys, the uint16 payload moved with its key
template <typename K>
__device__ __forceinline__ void rk_sort(K* keys, unsigned short* pay, int Cc, int lp) {
  const int P = 1 << lp, tid = threadIdx.x;
  const int pairs = Cc << (lp - 1);
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < pairs; q += RK_THREADS) {
        const int c = q >> (lp - 1), r = q & ((P >> 1) - 1);
        const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1));
        const int a = (c << lp) + i, b = a + j;
        const K ka = keys[a], kb = keys[b];
        const bool up = (i & k2) == 0;
        if ((ka > kb) == up && ka != kb) {
          keys[a] = kb; keys[b] = ka;
          const unsigned short pa = pay[a], pb = pay[b];
          pay[a] = pb; pay[b] = pa;
        }
      }
      __syncthreads();
    }
  }
}

// [first, last] of the run of keys equal to col[p], p < n, in the sorted col[0 .. n)
template <typename K>
__device__ __forceinline__ void rk_tie_run(const K* col, int p, int n, int* first_out, int* last_out) {
  const K kv = col[p];
  int first = p, last = p;
  if (p > 0 && col[p - 1] == kv) {                           // lower bound in [0, p)
    int lo = 0, hi = p - 1;                                  // col[hi] == kv
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (col[mid] < kv) lo = mid + 1; else hi = mid;
    }
    first = lo;
  }
  if (p + 1 < n && col[p + 1] == kv) {                       // last equal in (p, n)
    int lo = p + 1, hi = n - 1;                              // col[lo] == kv
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (col[mid] > kv) hi = mid - 1; else lo = mid;
    }
    last = lo;
  }
  *first_out = first;
  *last_out = last;
}

// the four tie sums of a run of t > 1 equal values, added by the first position of the run; side 0 = pred, 1 = truth
__device__ __forceinline__ void rk_tie_sums(u64* a, int side, u64 t) {
  atomicAdd(&a[I_TX + side], t * t * t - t);
  atomicAdd(&a[I_XTIE + side], t * (t - 1) / 2);
  atomicAdd(&a[I_X0 + side], t * (t - 1) * (t - 2));
  atomicAdd(&a[I_X1 + side], t * (t - 1) * (2 * t + 5));
}

// -1, 0 or 1 (v_med3_i32)
__device__ __forceinline__ int rk_sign(int v) { return min(max(v, -1), 1); }

template <typename TX, typename TY>
__global__ __launch_bounds__(RK_THREADS) void rank_pair_kernel(
    const TX* __restrict__ x, long long ldx, const TY* __restrict__ y, long long ldy,
    const long long* __restrict__ offsets, long long rows, int G, int max_n, int axis, int tau, int lds_keys,
    long long* __restrict__ ints, int* __restrict__ status) {
  typedef typename rk_keytype<TX>::type KX;
  typedef typename rk_keytype<TY>::type KY;
  constexpr int KS = sizeof(KX) > sizeof(KY) ? (int)sizeof(KX) : (int)sizeof(KY);
  extern __shared__ __align__(16) unsigned char rk_lds[];
  const int tid = threadIdx.x, seg = blockIdx.y;
  // n elements per problem, nprob problems in this segment, q_base = the segment's first problem in ``ints``
  int n;
  long long nprob, r0 = 0, q_base;
  if (axis == 0) {
    n = segment_rows(offsets, seg, rows, 2, max_n, &r0);
    nprob = G;
    q_base = (long long)seg * G;
    if (n == 0) {                                            // the offsets break what the launch was sized by
      if (tid == 0 && blockIdx.x == 0) status[RK_STATUS * seg + 2] = 1;
      return;
    }
  } else {
    n = G;
    nprob = rows;
    q_base = 0;
  }
  const int lp = 31 - __clz(rk_pow2ceil(n));                 // log2 P
  const int P = 1 << lp;
  const int C = rk_columns(lds_keys, n, KS);
  const long long j0 = (long long)blockIdx.x * C;
  if (j0 >= nprob) return;
  const int Cc = (int)min((long long)C, nprob - j0);
  unsigned char* keyb = rk_lds;                                                        // [Cc][P] keys, then the packed pairs
  unsigned short* bufA = reinterpret_cast<unsigned short*>(rk_lds + (size_t)C * P * KS);   // [Cc][P] index, then a_y
  unsigned short* bufB = bufA + (size_t)C * P;                                             // [Cc][P] a_x
  u64* acc = reinterpret_cast<u64*>(rk_lds + lds_keys);                                // [RK_CMAX][RK_INTS]
  const long long ex = axis == 0 ? ldx : 1, px = axis == 0 ? 1 : ldx;
  const long long ey = axis == 0 ? ldy : 1, py = axis == 0 ? 1 : ldy;
  const TX* xs = axis == 0 ? x + r0 * ldx + j0 : x + j0 * ldx;
  const TY* ys = axis == 0 ? y + r0 * ldy + j0 : y + j0 * ldy;
  int* st = status + RK_STATUS * seg;
  const int q0 = (int)j0;                                    // (problem index within the segment: a gene, or a row < 2^31)

  for (int e = tid; e < Cc * RK_INTS; e += RK_THREADS) acc[e] = (e % RK_INTS) == I_N ? (u64)n : 0;
  for (int e = tid; e < Cc << lp; e += RK_THREADS) {
    bufA[e] = (unsigned short)(e & (P - 1));                 // (a padding position carries an index >= n: never scattered)
    bufB[e] = 0;
  }
  // ---- pred: sort with the original index, scatter a_x back by it
  KX* kx = reinterpret_cast<KX*>(keyb);
  rk_load<TX>(xs, ex, px, n, Cc, lp, kx, st, q0);
  __syncthreads();
  rk_sort<KX>(kx, bufA, Cc, lp);
  for (int e = tid; e < Cc << lp; e += RK_THREADS) {
    const int c = e >> lp, p = e & (P - 1);
    if (p >= n) continue;
    int first, last;
    rk_tie_run<KX>(kx + (c << lp), p, n, &first, &last);
    const int i = bufA[e];
    if (i < n) bufB[(c << lp) + i] = (unsigned short)(first + last + 2);
    if (p == first && last > first) rk_tie_sums(acc + c * RK_INTS, 0, (u64)(last - first + 1));
  }
  __syncthreads();
  // ---- truth: sort with a_x as the payload; a_y lands beside it, Sxy is summed in place
  KY* ky = reinterpret_cast<KY*>(keyb);
  rk_load<TY>(ys, ey, py, n, Cc, lp, ky, st, q0);
  __syncthreads();
  rk_sort<KY>(ky, bufB, Cc, lp);
  for (int e = tid; e < Cc << lp; e += RK_THREADS) {         // (P >= 64: a wave's 64 positions belong to one problem)
    const int c = e >> lp, p = e & (P - 1);
    long long prod = 0;
    if (p < n) {
      int first, last;
      rk_tie_run<KY>(ky + (c << lp), p, n, &first, &last);
      const int ay = first + last + 2;
      bufA[e] = (unsigned short)ay;
      prod = (long long)bufB[e] * ay;
      if (p == first && last > first) rk_tie_sums(acc + c * RK_INTS, 1, (u64)(last - first + 1));
    }
    if (lp >= 6) {
      prod = wave_sum(prod);
      if ((tid & 63) == 0) atomicAdd(&acc[c * RK_INTS + I_SXY], (u64)prod);
    } else if (p < n) {
      atomicAdd(&acc[c * RK_INTS + I_SXY], (u64)prod);
    }
  }
  __syncthreads();

  if (tau) {
    unsigned* pk = reinterpret_cast<unsigned*>(keyb);        // [Cc][P]: the keys are spent
    for (int e = tid; e < Cc << lp; e += RK_THREADS) pk[e] = (unsigned)bufB[e] | ((unsigned)bufA[e] << 16);
    __syncthreads();
    // items = (problem, block of 64 elements i), dealt to the 16 waves in turn; a wave walks j > i to the problem's end
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = (n + 63) >> 6;
    for (int item = wave; item < Cc * nb; item += RK_THREADS / 64) {
      const int c = item / nb, b = item - c * nb;
      const unsigned* col = pk + (c << lp);
      const int i = (b << 6) + lane;
      const bool live = i < n;
      const unsigned mine = col[live ? i : n - 1];
      const int ax = (int)(mine & 0xFFFFu), ay = (int)(mine >> 16);
      int s = 0, joint = 0;
      const int jmid = min((b << 6) + 64, n);
      for (int j = (b << 6) + 1; j < jmid; ++j) {            // inside the block: only j > i counts
        const unsigned other = (unsigned)__builtin_amdgcn_readfirstlane((int)col[j]);
        const int sg = rk_sign(__mul24(ax - (int)(other & 0xFFFFu), ay - (int)(other >> 16)));
        const bool after = j > i;
        s += after ? sg : 0;
        joint += (after && other == mine) ? 1 : 0;
      }
      for (int j = jmid; j < n; ++j) {
        const unsigned other = (unsigned)__builtin_amdgcn_readfirstlane((int)col[j]);
        s += rk_sign(__mul24(ax - (int)(other & 0xFFFFu), ay - (int)(other >> 16)));
        joint += other == mine ? 1 : 0;
      }
      const long long ws = wave_sum((long long)(live ? s : 0));
      const long long wj = wave_sum((long long)(live ? joint : 0));
      if (lane == 0) {
        atomicAdd(&acc[c * RK_INTS + I_S], (u64)ws);
        atomicAdd(&acc[c * RK_INTS + I_JOINT], (u64)wj);
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < Cc * RK_INTS; e += RK_THREADS) ints[(q_base + j0) * RK_INTS + e] = (long long)acc[e];
}

__device__ __forceinline__ double rk_clip(double v) { return v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v); }
// num / (sqrt(a) sqrt(b)) clipped to [-1, 1], a, b > 0, |num| <= sqrt(a b) < 2^63.  Where num^2 = a b -- perfect agreement,
// an exact statement about integers -- the value is +-1 and is returned as such: sqrt(a) sqrt(a) may round to a (1 + eps)
__device__ __forceinline__ double rk_ratio(long long num, long long a, long long b) {
#pragma clang fp contract(off)
  if ((__int128)num * num == (__int128)a * b) return num < 0 ? -1.0 : 1.0;
  return rk_clip((double)num / (sqrt((double)a) * sqrt((double)b)));
}

__global__ __launch_bounds__(RK_F_THREADS) void rank_finish_kernel(const long long* __restrict__ ints, long long problems,
                                                                   int tau, double* __restrict__ rho,
                                                                   double* __restrict__ tau_b, double* __restrict__ tau_p,
                                                                   double* __restrict__ tau_nl) {
#pragma clang fp contract(off)
  const long long q = (long long)blockIdx.x * RK_F_THREADS + threadIdx.x;
  if (q >= problems) return;
  const long long* I = ints + q * RK_INTS;
  const long long n = I[I_N];
  double r = NAN, t = NAN, tp = NAN, tnl = NAN;
  if (n >= 2) {
    const long long num = n * I[I_SXY] - n * n * (n + 1) * (n + 1);
    const long long dx = n * (n * n * n - n - I[I_TX]) / 3, dy = n * (n * n * n - n - I[I_TY]) / 3;
    if (dx > 0 && dy > 0) r = rk_ratio(num, dx, dy);
    if (tau) {
      const long long n0 = n * (n - 1) / 2, s = I[I_S];
      const long long ex = n0 - I[I_XTIE], ey = n0 - I[I_YTIE];
      if (ex > 0 && ey > 0) {
        t = rk_ratio(s, ex, ey);
        if (n >= 3) {
          const long long m = n * (n - 1);
          const double var = ((double)(m * (2 * n + 5) - I[I_X1] - I[I_Y1]) / 18.0 +
                              (double)(2 * I[I_XTIE] * I[I_YTIE]) / (double)m) +
                             ((double)I[I_X0] * (double)I[I_Y0]) / (double)(9 * m * (n - 2));
          stats::normal_tail((double)s / sqrt(var), 1, &tp, &tnl);
        }
      }
    }
  }
  rho[q] = r;
  if (tau) {
    tau_b[q] = t;
    tau_p[q] = tp;
    tau_nl[q] = tnl;
  }
}

// summary[s] = { heg_rho, hvg_rho, heg_tau, hvg_tau, n_valid }; lane 0 sums rho, lane 1 tau (when given), gene by gene
__global__ __launch_bounds__(RK_S_THREADS) void rank_summary_kernel(const double* __restrict__ rho,
                                                                    const double* __restrict__ tau_b,
                                                                    const long long* __restrict__ heg, int G, int n_heg,
                                                                    double* __restrict__ summary) {
#pragma clang fp contract(off)
  __shared__ double tile[2][RK_S_TILE];
  __shared__ unsigned char member[RK_MAX_G];
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int g = tid; g < G; g += RK_S_THREADS) member[g] = 0;
  __syncthreads();
  for (int k = tid; k < n_heg; k += RK_S_THREADS) member[clamp_index((int)heg[(long long)s * n_heg + k], G)] = 1;
  const double* src = tid == 1 ? tau_b : rho;
  double heg_sum = 0.0, all_sum = 0.0;
  int valid = 0;
  for (int g0 = 0; g0 < G; g0 += RK_S_TILE) {
    __syncthreads();
    for (int e = tid; e < RK_S_TILE; e += RK_S_THREADS) {
      const long long o = (long long)s * G + min(g0 + e, G - 1);
      tile[0][e] = rho[o];
      tile[1][e] = tau_b ? tau_b[o] : NAN;
    }
    __syncthreads();
    if (tid < 2 && src) {
      const int cnt = min(RK_S_TILE, G - g0);
      for (int e = 0; e < cnt; ++e) {
        const double v = tile[tid][e];
        if (member[g0 + e]) heg_sum += v;
        if (!isnan(v)) { all_sum += v; ++valid; }
      }
    }
  }
  if (tid < 2) {
    summary[s * 5 + 2 * tid] = src ? heg_sum / (double)n_heg : NAN;
    summary[s * 5 + 2 * tid + 1] = src && valid ? all_sum / (double)valid : NAN;
    if (tid == 0) summary[s * 5 + 4] = (double)valid;
  }
}

template <typename TX, typename TY>
int rk_launch(const void* pred, int64_t ldp, const void* truth, int64_t ldt, const int64_t* offsets, int S, int64_t rows,
              int G, int max_n, int axis, int tau, int64_t* ints, int32_t* status, hipStream_t st) {
  constexpr int KS = sizeof(TX) > sizeof(TY) ? (int)sizeof(TX) : (int)sizeof(TY);
  const int lds_keys = rk_lds_keys(max_n, KS);
  const size_t lds = (size_t)lds_keys + RK_CMAX * RK_INTS * 8;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(rank_pair_kernel<TX, TY>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, RK_MAX_N32 * 8 + RK_CMAX * RK_INTS * 8);
  }
  const int cmin = rk_columns(lds_keys, max_n, KS);          // no segment takes fewer problems per workgroup than this
  const long long nprob = axis == 0 ? G : rows;
  hipLaunchKernelGGL((rank_pair_kernel<TX, TY>), dim3((unsigned)((nprob + cmin - 1) / cmin), axis == 0 ? S : 1),
                     dim3(RK_THREADS), lds, st, static_cast<const TX*>(pred), (long long)ldp, static_cast<const TY*>(truth),
                     (long long)ldt, reinterpret_cast<const long long*>(offsets), (long long)rows, G, max_n, axis, tau,
                     lds_keys, reinterpret_cast<long long*>(ints), status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

inline int rk_max_elements(int pred_dtype, int true_dtype) {
  if ((pred_dtype != 0 && pred_dtype != 1) || (true_dtype != 0 && true_dtype != 1)) return -1;
  return pred_dtype || true_dtype ? RK_MAX_N64 : RK_MAX_N32;
}

}  // namespace

extern "C" int32_t mcl_rank_max_elements(int32_t pred_dtype, int32_t true_dtype) {
  return rk_max_elements(pred_dtype, true_dtype);
}

extern "C" int32_t mcl_rank_columns(int32_t n, int32_t pred_dtype, int32_t true_dtype) {
  const int lim = rk_max_elements(pred_dtype, true_dtype);
  if (lim < 0 || n < 2 || n > lim) return -1;
  const int ks = pred_dtype || true_dtype ? 8 : 4;
  return rk_columns(rk_lds_keys(n, ks), n, ks);
}

extern "C" int mcl_rank_stats(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                              int32_t true_dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                              int32_t max_n, int32_t axis, int32_t tau, int64_t* ints, int32_t* status,
                              mcl_stream_t stream) {
  if (!pred || !truth || !ints || !status || (axis == 0 && !offsets)) return MCL_EINVAL;
  const int lim = rk_max_elements(pred_dtype, true_dtype);
  if (lim < 0 || (axis != 0 && axis != 1) || G < 1 || G > RK_MAX_G || ld_pred < G || ld_true < G || rows < 1) return MCL_EINVAL;
  if (axis == 0) {
    if (S < 1 || S > RK_MAX_S || max_n < 2 || max_n > lim || rows < 2 || rows > (int64_t)S * max_n) return MCL_EINVAL;
  } else {
    if (S != 1 || G < 2 || G > lim || max_n != G || rows > 0x7fffffffll) return MCL_EINVAL;
  }
  const hipStream_t st = mcl_stream(stream);
  const long long problems = axis == 0 ? (long long)S * G : (long long)rows;
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(ints, 0, (size_t)problems * RK_INTS * 8, st) != hipSuccess) return (int)hipGetLastError();
  if (hipMemsetAsync(status, 0, (size_t)S * RK_STATUS * 4, st) != hipSuccess) return (int)hipGetLastError();
  const int code = pred_dtype * 2 + true_dtype;
  switch (code) {
    case 0: return rk_launch<float, float>(pred, ld_pred, truth, ld_true, offsets, S, rows, G, max_n, axis, tau != 0, ints, status, st);
    case 1: return rk_launch<float, double>(pred, ld_pred, truth, ld_true, offsets, S, rows, G, max_n, axis, tau != 0, ints, status, st);
    case 2: return rk_launch<double, float>(pred, ld_pred, truth, ld_true, offsets, S, rows, G, max_n, axis, tau != 0, ints, status, st);
    default: return rk_launch<double, double>(pred, ld_pred, truth, ld_true, offsets, S, rows, G, max_n, axis, tau != 0, ints, status, st);
  }
}

extern "C" int mcl_rank_finish(const int64_t* ints, int64_t problems, int32_t tau, double* rho, double* tau_b,
                               double* tau_p, double* tau_neglog10p, mcl_stream_t stream) {
  if (!ints || !rho || (tau && (!tau_b || !tau_p || !tau_neglog10p))) return MCL_EINVAL;
  if (problems < 1 || problems > (int64_t)RK_F_THREADS * 0x7fffffffll) return MCL_EINVAL;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((problems + RK_F_THREADS - 1) / RK_F_THREADS)),
                     dim3(RK_F_THREADS), 0, mcl_stream(stream), reinterpret_cast<const long long*>(ints),
                     (long long)problems, tau != 0, rho, tau_b, tau_p, tau_neglog10p);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_rank_summary(const double* rho, const double* tau_b, const int64_t* heg, int32_t S, int32_t G,
                                int32_t n_heg, double* summary, mcl_stream_t stream) {
  if (!rho || !heg || !summary) return MCL_EINVAL;
  if (S < 1 || S > RK_MAX_S || G < 1 || G > RK_MAX_G || n_heg < 1 || n_heg > G) return MCL_EINVAL;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(rank_summary_kernel, dim3(S), dim3(RK_S_THREADS), 0, mcl_stream(stream), rho, tau_b,
                     reinterpret_cast<const long long*>(heg), G, n_heg, summary);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
