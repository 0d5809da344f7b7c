// Local spatial statistics on the spot lattice: local Moran's I_i (univariate and bivariate), Getis-Ord Gi*, the quadrant
// and hot / cold spot label of every (spot, column pair) with a CONDITIONAL permutation test -- spot i keeps its value, its
// d_i neighbours are redrawn from the slide's other n - 1 spots --, for every slide of an evaluation per call (DESIGN 6.22
// states the arithmetic, tests/hotspot_reference.py restates it in numpy).  Slide s owns rows offsets[s] .. offsets[s + 1]
// of every row-stacked array; the graph is mcl_spatial_lattice's fixed-width list (nbr, w; a slot with w = 0 is pruned).
// A pair (a, b) holds column a at the spot and lags column b over the neighbours; (j, j) is the univariate case.
//
//   hs_moments_kernel  one workgroup per (side, slide, pair): mean and den = sum z^2 of the column in THE FIXED ROW ORDER of
//                      csrc/spatial.hip (lane r of 256 adds its rows r, r + 256, ... ascending; xor butterfly 32 ... 1 in a
//                      wave; the four wave totals as (t0 + t1) + (t2 + t3)): bit-equal to mcl_spatial_stats' mean / den.
//                      A constant column has den = 0 exactly.  Counts non-finite values and bad pair columns.
//   hs_draws_kernel    one thread per (draw p, spot i): the d_i distinct spots of the draw as uint16 (slots past d_i: 0xFFFF).
//   hs_perm_kernel     THE HOT PATH.  A workgroup takes C adjacent pairs of one slide -- as many lagged columns as its LDS
//                      holds, at most 6 --, centres them into LDS once (column-interleaved fp64) and every thread owns spots
//                      tid, tid + threads, ...: the observed neighbour sum L_i in slot order, then all P draws, each computed
//                      (or read from the table) once and gathered for all C columns; per column count_ge, count_le, sum L^p
//                      and sum (L^p)^2 over p ascending.  No cross-lane operation in the loop.
//   hs_final_kernel    one thread per (spot, pair): I_i, quadrant, Gi* z and its normal tail in log space, pval_sim, the
//                      moments of the sims of I_i, z_sim and the label.
//
// The draw (p, i) of a slide is a pure function of (seed, p, i, n, d_i): Floyd's subset algorithm over a splitmix64 stream,
// h = mix(mix(mix(seed) ^ p) + i), u_t = the high 32 bits of mix(h + t), J = n - 1 - d_i + t, r = (u_t (J + 1)) >> 32,
// c_t = r unless r was drawn before (then J), spot = c_t + (c_t >= i).  Every product and sum is rounded separately (no
// contraction), no floating-point atomics, no workgroup waits for another: a slide inside a batch is bit-identical to the
// same slide alone, whatever the launch shape.
#include "common.h"
#include "stats.h"

namespace {

constexpr int HS_MAX_N = 16384;
constexpr int HS_MAX_K = 64;
constexpr int HS_MAX_G = 16384;
constexpr int HS_MAX_M = 16384;          // pairs per call
constexpr int HS_MAX_S = 65535;          // grid.y
constexpr int HS_MAX_PERMS = 65535;      // grid.y of the draw kernel
constexpr int HS_LANES = 256;            // row lanes of the fixed order
constexpr int HS_CMAX = 6;               // lagged columns per workgroup, as csrc/spatial.hip's SP_CMAX
constexpr int HS_Z_BYTES = 155648;       // LDS for the centred columns (152 KiB of the 160), as SP_Z_BYTES
constexpr int HS_O_THREADS = 256;
constexpr int HS_STATUS = 4;             // offsets broken, non-finite x, pair column out of range, draws that do not fit

__host__ __device__ inline long long hs_align8(long long v) { return (v + 7) & ~7ll; }
__host__ __device__ inline int hs_columns(int n) {
  int c = HS_Z_BYTES / (8 * n);
  if (c > HS_CMAX) c = HS_CMAX;
  return c < 1 ? 1 : c;
}
template <int KD>
constexpr int hs_threads() { return KD <= 8 ? 1024 : 256; }

// x (rows, G) in either width, as fp64
__device__ __forceinline__ double hs_ld(const void* x, int dtype, long long idx) {
  return dtype ? static_cast<const double*>(x)[idx] : (double)static_cast<const float*>(x)[idx];
}

// the d <= KD distinct spots of draw h = mix(mix(mix(seed) ^ p) + i) for spot i of n, none of them i: Floyd's algorithm.
// Fully unrolled: sp[] is indexed by constants only and stays in registers.
template <int KD>
__device__ __forceinline__ void hs_draw(u64 h, int i, int n, int d, int (&sp)[KD]) {
#pragma unroll
  for (int t = 0; t < KD; ++t) {
    if (t < d) {
      const unsigned u = (unsigned)(mix64(h + (u64)t) >> 32);
      const int J = n - 1 - d + t;
      const int r = (int)(((u64)u * (u64)(unsigned)(J + 1)) >> 32);
      const int cand = r + (r >= i);
      bool dup = false;
#pragma unroll
      for (int v = 0; v < t; ++v) dup |= sp[v] == cand;
      sp[t] = dup ? J + (J >= i) : cand;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- moments
__global__ __launch_bounds__(HS_LANES) void hs_moments_kernel(
    const void* __restrict__ x, long long ld, int dtype, const long long* __restrict__ offsets, int S, long long rows, int G,
    int max_n, const int* __restrict__ pairs, int M, double* __restrict__ mean_out, double* __restrict__ den_out,
    int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  __shared__ int varies_s;
  const int m = blockIdx.x, s = blockIdx.y, side = blockIdx.z, r = threadIdx.x;
  const long long o = ((long long)side * S + s) * M + m;
  long long r0;
  const int n = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int col = pairs[2 * m + side];
  if (n == 0 || col < 0 || col >= G) {
    if (r == 0) {
      if (n == 0) status[HS_STATUS * s] = 1;
      else atomicAdd(&status[HS_STATUS * s + 2], 1);
      mean_out[o] = NAN;
      den_out[o] = NAN;
    }
    return;
  }
  if (r == 0) varies_s = 0;
  __syncthreads();
  const long long base = r0 * ld + col;
  const double first = hs_ld(x, dtype, base);
  double a = 0.0;
  int nf = 0, differs = 0;
  for (int i = r; i < n; i += HS_LANES) {
    const double v = hs_ld(x, dtype, base + (long long)i * ld);
    nf += !isfinite(v);
    differs |= v != first;
    a = a + v;
  }
  if (differs) atomicOr(&varies_s, 1);
  if (nf) atomicAdd(&status[HS_STATUS * s + 1], nf);
  a = wave_sum(a);
  if ((r & 63) == 0) red[r >> 6] = a;
  __syncthreads();
  const double mean = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n;
  const int varies = varies_s;
  __syncthreads();
  double q = 0.0;
  if (varies)
    for (int i = r; i < n; i += HS_LANES) {
      const double z = hs_ld(x, dtype, base + (long long)i * ld) - mean;
      const double sq = z * z;
      q = q + sq;
    }
  q = wave_sum(q);
  if ((r & 63) == 0) red[r >> 6] = q;
  __syncthreads();
  if (r == 0) {
    mean_out[o] = mean;
    den_out[o] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------ draws
// kept slots of row i (w > 0), at most n - 1 of them drawn
__device__ __forceinline__ int hs_degree(const double* __restrict__ wi, int k, int n) {
  int d = 0;
  for (int t = 0; t < k; ++t) d += wi[t] > 0.0;
  return min(d, n - 1);
}

template <int KD>
__global__ __launch_bounds__(HS_O_THREADS) void hs_draws_kernel(const long long* __restrict__ offsets, long long rows, int max_n,
                                                                int k, const double* __restrict__ w, int P, u64 seed,
                                                                unsigned short* __restrict__ table) {
  const int p = blockIdx.y, s = blockIdx.z;
  const int i = blockIdx.x * HS_O_THREADS + threadIdx.x;
  long long r0;
  const int n = segment_rows(offsets, s, rows, 2, max_n, &r0);
  if (i >= n) return;
  const int d = hs_degree(w + (r0 + i) * k, k, n);
  int sp[KD];
  hs_draw<KD>(mix64(mix64(mix64(seed) ^ (u64)p) + (u64)i), i, n, d, sp);
  unsigned short* out = table + (r0 * P + (long long)p * n + i) * k;
#pragma unroll
  for (int t = 0; t < KD; ++t)
    if (t < k) out[t] = t < d ? (unsigned short)sp[t] : (unsigned short)0xFFFF;
}

// ------------------------------------------------------------------------------------------------- the permutation pass
template <int C, int KD>
__global__ __launch_bounds__(hs_threads<KD>()) void hs_perm_kernel(
    const void* __restrict__ x, long long ld, int dtype, const long long* __restrict__ offsets, int S, long long rows, int G,
    int max_n, int k, const int* __restrict__ nbr, const double* __restrict__ w, const int* __restrict__ pairs, int M,
    const double* __restrict__ mean, const double* __restrict__ den, const unsigned short* __restrict__ table, int P, u64 seed,
    double* __restrict__ lag_out, int* __restrict__ ge_out, int* __restrict__ le_out, double* __restrict__ sum1_out,
    double* __restrict__ sum2_out, int* __restrict__ deg_out, double* __restrict__ wbar_out, int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char hs_lds[];
  __shared__ int col_s[C], live_s[C];
  __shared__ double mean_s[C];
  double* zs = reinterpret_cast<double*>(hs_lds);           // [n][C]
  const int s = blockIdx.y, tid = threadIdx.x, threads = blockDim.x;
  long long r0;
  const int n = segment_rows(offsets, s, rows, 2, max_n, &r0);
  if (n == 0 || hs_columns(n) != C) return;
  const int m0 = blockIdx.x * C;
  if (m0 >= M) return;
  const int cc = min(C, M - m0);
  if (tid < C) {
    const int m = m0 + min(tid, cc - 1);                    // (a pair past M reads the last one)
    const int b = pairs[2 * m + 1];
    const bool ok = b >= 0 && b < G;
    const long long o = ((long long)S + s) * M + m;         // side 1: the lagged column
    col_s[tid] = ok ? b : 0;
    mean_s[tid] = mean[o];
    live_s[tid] = ok && den[o] > 0.0;                       // a constant column is exactly zero
  }
  __syncthreads();
  const int total = n * C;
  for (int e = tid; e < total; e += threads) {
    const int i = e / C, q = e - i * C;
    const double v = hs_ld(x, dtype, (r0 + i) * ld + col_s[q]);
    zs[e] = live_s[q] ? v - mean_s[q] : 0.0;
  }
  __syncthreads();

  const int nm1 = n - 1;
  const u64 hseed = mix64(seed);
  int bad = 0;
  for (int i = tid; i < n; i += threads) {
    const int* nbi = nbr + (r0 + i) * k;
    const double* wi = w + (r0 + i) * k;
    double L[C];
#pragma unroll
    for (int q = 0; q < C; ++q) L[q] = 0.0;
    int kept = 0;
    double wbar = 0.0;
    for (int t = 0; t < k; ++t) {
      const double wt = wi[t];
      if (wt > 0.0) {
        const int j = clamp_index(nbi[t], n);
        if (kept == 0) wbar = wt;
        ++kept;
#pragma unroll
        for (int q = 0; q < C; ++q) L[q] = L[q] + zs[j * C + q];
      }
    }
    const int d = min(kept, nm1);
    if (blockIdx.x == 0) {
      deg_out[r0 + i] = kept;
      wbar_out[r0 + i] = wbar;
    }
    int cge[C], cle[C];
    double a1[C], a2[C];
#pragma unroll
    for (int q = 0; q < C; ++q) { cge[q] = 0; cle[q] = 0; a1[q] = 0.0; a2[q] = 0.0; }
    for (int p = 0; p < P; ++p) {
      int sp[KD];
      if (table) {
        const unsigned short* tb = table + (r0 * P + (long long)p * n + i) * k;
#pragma unroll
        for (int t = 0; t < KD; ++t) {
          if (t < k) {
            const int v = tb[t];
            bad |= t < d ? (v >= n || v == i) : (v != 0xFFFF);
            sp[t] = min(v, nm1);
          }
        }
      } else {
        hs_draw<KD>(mix64(mix64(hseed ^ (u64)p) + (u64)i), i, n, d, sp);
      }
      double l[C];
#pragma unroll
      for (int q = 0; q < C; ++q) l[q] = 0.0;
#pragma unroll
      for (int t = 0; t < KD; ++t) {
        if (t < d) {
          const int j = sp[t];
#pragma unroll
          for (int q = 0; q < C; ++q) l[q] = l[q] + zs[j * C + q];
        }
      }
#pragma unroll
      for (int q = 0; q < C; ++q) {
        cge[q] += l[q] >= L[q];
        cle[q] += l[q] <= L[q];
        a1[q] = a1[q] + l[q];
        const double sq = l[q] * l[q];
        a2[q] = a2[q] + sq;
      }
    }
    const long long o = (r0 + i) * M + m0;
#pragma unroll
    for (int q = 0; q < C; ++q) {
      if (q < cc) {
        lag_out[o + q] = L[q];
        if (P > 0) {
          ge_out[o + q] = cge[q];
          le_out[o + q] = cle[q];
          sum1_out[o + q] = a1[q];
          sum2_out[o + q] = a2[q];
        }
      }
    }
  }
  if (bad) atomicAdd(&status[HS_STATUS * s + 3], 1);
}

// ----------------------------------------------------------------------------------------------------- finalisation
__global__ __launch_bounds__(HS_O_THREADS) void hs_final_kernel(
    const void* __restrict__ x, long long ld, int dtype, const long long* __restrict__ offsets, int S, long long rows, int G,
    int max_n, const int* __restrict__ pairs, int M, const double* __restrict__ mean, const double* __restrict__ den,
    const int* __restrict__ deg, const double* __restrict__ wbar, const double* __restrict__ lag, const int* __restrict__ ge,
    const int* __restrict__ le, const double* __restrict__ sum1, const double* __restrict__ sum2, int P, double alpha,
    double* __restrict__ local_i, signed char* __restrict__ quadrant, double* __restrict__ gi_z, double* __restrict__ gi_p,
    double* __restrict__ gi_nl, double* __restrict__ pval_sim, double* __restrict__ mean_sim, double* __restrict__ var_sim,
    double* __restrict__ z_sim, signed char* __restrict__ cluster) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  long long r0;
  const int n = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const long long e = (long long)blockIdx.x * HS_O_THREADS + threadIdx.x;
  if (e >= (long long)n * M) return;
  const int i = (int)(e / M), m = (int)(e - (long long)i * M);
  const int a = pairs[2 * m], b = pairs[2 * m + 1];
  const long long o = (r0 + i) * M + m;
  const bool cols_ok = a >= 0 && a < G && b >= 0 && b < G;
  const double ma = mean[(long long)s * M + m], da = den[(long long)s * M + m], db = den[((long long)S + s) * M + m];
  const bool bad = !cols_ok || !(da > 0.0) || !(db > 0.0);
  const double za = bad ? 0.0 : hs_ld(x, dtype, (r0 + i) * ld + a) - ma;
  const int d = deg[r0 + i];
  const double wb = wbar[r0 + i], L = lag[o];
  const double D = a == b ? da : sqrt(da * db);
  const double num = (double)(n - 1) * za;
  const double wl = wb * L;
  const double I = (num * wl) / D;
  const int quad = bad ? 0 : (za > 0.0 && L > 0.0) ? 1 : (za < 0.0 && L > 0.0) ? 2 : (za < 0.0 && L < 0.0) ? 3
                                                                                 : (za > 0.0 && L < 0.0) ? 4 : 0;
  local_i[o] = bad ? NAN : I;
  quadrant[o] = (signed char)quad;
  double gz = NAN, gp = NAN, gl = NAN;
  if (!bad && a == b && n - d - 1 > 0) {
    const double sd = sqrt(da / (double)n);
    const double sc = sqrt(((double)(d + 1) * (double)(n - d - 1)) / (double)(n - 1));
    gz = (za + L) / (sd * sc);
    stats::normal_tail(gz, 0, &gp, &gl);
  }
  gi_z[o] = gz;
  gi_p[o] = gp;
  gi_nl[o] = gl;
  if (P > 0) {
    const int cnt = min(ge[o], le[o]);
    const double p = ((double)cnt + 1.0) / ((double)P + 1.0);
    const double mL = sum1[o] / (double)P;
    double vL = sum2[o] / (double)P - mL * mL;
    if (vL < 0.0) vL = 0.0;
    const double f = (num * wb) / D;
    const double ms = f * mL, vs = (f * f) * vL;
    pval_sim[o] = bad ? NAN : p;
    mean_sim[o] = bad ? NAN : ms;
    var_sim[o] = bad ? NAN : vs;
    z_sim[o] = bad ? NAN : (I - ms) / sqrt(vs);
    cluster[o] = (signed char)((!bad && p <= alpha) ? quad : 0);
  }
}

inline bool hs_shape_ok(int32_t S, int64_t rows, int32_t max_n) {
  return S >= 1 && S <= HS_MAX_S && max_n >= 2 && max_n <= HS_MAX_N && rows >= 2 && rows <= (int64_t)S * max_n;
}

template <int C, int KD>
int hs_launch_perm(const void* x, int64_t ld, int dtype, const int64_t* offsets, int S, int64_t rows, int G, int max_n, int k,
                   const int32_t* nbr, const double* w, const int32_t* pairs, int M, const double* mean, const double* den,
                   const unsigned short* table, int P, uint64_t seed, double* lag, int32_t* ge, int32_t* le, double* sum1,
                   double* sum2, int32_t* deg, double* wbar, int32_t* status, hipStream_t st) {
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hs_perm_kernel<C, KD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              HS_Z_BYTES);
  }
  // every slide this launch serves has hs_columns(n) == C, so n C 8 <= HS_Z_BYTES, and n <= max_n
  const long long want = (long long)max_n * C * 8;
  const size_t lds = (size_t)(want < HS_Z_BYTES ? want : HS_Z_BYTES);
  int threads = (max_n + 63) / 64 * 64;
  if (threads > hs_threads<KD>()) threads = hs_threads<KD>();
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL((hs_perm_kernel<C, KD>), dim3((M + C - 1) / C, S), dim3(threads), lds, st, x, (long long)ld, dtype,
                     reinterpret_cast<const long long*>(offsets), S, (long long)rows, G, max_n, k, nbr, w, pairs, M, mean, den,
                     table, P, (u64)seed, lag, ge, le, sum1, sum2, deg, wbar, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

template <int KD>
int hs_launch_perm_all(int cmask, const void* x, int64_t ld, int dtype, const int64_t* offsets, int S, int64_t rows, int G,
                       int max_n, int k, const int32_t* nbr, const double* w, const int32_t* pairs, int M, const double* mean,
                       const double* den, const unsigned short* table, int P, uint64_t seed, double* lag, int32_t* ge,
                       int32_t* le, double* sum1, double* sum2, int32_t* deg, double* wbar, int32_t* status, hipStream_t st) {
  int rc = MCL_OK;
#define HS_ONE(C)                                                                                                     \
  if (rc == MCL_OK && (cmask >> C) & 1)                                                                               \
    rc = hs_launch_perm<C, KD>(x, ld, dtype, offsets, S, rows, G, max_n, k, nbr, w, pairs, M, mean, den, table, P, seed, lag, \
                               ge, le, sum1, sum2, deg, wbar, status, st)
  HS_ONE(1); HS_ONE(2); HS_ONE(3); HS_ONE(4); HS_ONE(5); HS_ONE(6);
  static_assert(HS_CMAX == 6, "one launch per column count");
#undef HS_ONE
  return rc;
}

}  // namespace

extern "C" int32_t mcl_hotspot_columns(int32_t n) { return (n < 2 || n > HS_MAX_N) ? -1 : hs_columns(n); }

extern "C" int64_t mcl_hotspot_table_bytes(int64_t rows, int32_t k, int32_t n_perms) {
  if (rows < 2 || rows > (int64_t)HS_MAX_S * HS_MAX_N || k < 1 || k > HS_MAX_K || n_perms < 1 || n_perms > HS_MAX_PERMS)
    return -1;
  return hs_align8(rows * k * n_perms * 2) + 8;
}

extern "C" int mcl_hotspot_moments(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows,
                                   int32_t G, int32_t max_n, const int32_t* pairs, int32_t M, double* mean, double* den,
                                   int32_t* status, mcl_stream_t stream) {
  if (!x || !offsets || !pairs || !mean || !den || !status) return MCL_EINVAL;
  if (!hs_shape_ok(S, rows, max_n) || G < 1 || G > HS_MAX_G || ld < G || (dtype != 0 && dtype != 1) || M < 1 || M > HS_MAX_M)
    return MCL_EINVAL;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hs_moments_kernel, dim3(M, S, 2), dim3(HS_LANES), 0, static_cast<hipStream_t>(stream), x, (long long)ld,
                     dtype, reinterpret_cast<const long long*>(offsets), S, (long long)rows, G, max_n, pairs, M, mean, den,
                     status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_hotspot_draws(const int64_t* offsets, int32_t S, int64_t rows, int32_t max_n, int32_t k, const double* w,
                                 int32_t n_perms, uint64_t seed, void* table, mcl_stream_t stream) {
  if (!offsets || !w || !table) return MCL_EINVAL;
  if (!hs_shape_ok(S, rows, max_n) || k < 1 || k > HS_MAX_K || n_perms < 1 || n_perms > HS_MAX_PERMS) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((max_n + HS_O_THREADS - 1) / HS_O_THREADS, n_perms, S);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  unsigned short* tb = static_cast<unsigned short*>(table);
  MCL_CLEAR_ERROR();
  if (k <= 8)
    hipLaunchKernelGGL(hs_draws_kernel<8>, grid, dim3(HS_O_THREADS), 0, st, off, (long long)rows, max_n, k, w, n_perms,
                       (u64)seed, tb);
  else
    hipLaunchKernelGGL(hs_draws_kernel<HS_MAX_K>, grid, dim3(HS_O_THREADS), 0, st, off, (long long)rows, max_n, k, w, n_perms,
                       (u64)seed, tb);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_hotspot_permute(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows,
                                   int32_t G, int32_t max_n, int32_t k, int32_t column_mask, const int32_t* nbr,
                                   const double* w, const int32_t* pairs, int32_t M, const double* mean, const double* den,
                                   const void* table, int32_t n_perms, uint64_t seed, double* lag, int32_t* count_ge,
                                   int32_t* count_le, double* sum1, double* sum2, int32_t* deg, double* wbar, int32_t* status,
                                   mcl_stream_t stream) {
  if (!x || !offsets || !nbr || !w || !pairs || !mean || !den || !lag || !deg || !wbar || !status) return MCL_EINVAL;
  if (!hs_shape_ok(S, rows, max_n) || G < 1 || G > HS_MAX_G || ld < G || (dtype != 0 && dtype != 1) || k < 1 ||
      k > HS_MAX_K || M < 1 || M > HS_MAX_M || n_perms < 0 || n_perms > HS_MAX_PERMS || (column_mask & ~0x7E) || !column_mask)
    return MCL_EINVAL;
  if (n_perms > 0 && (!count_ge || !count_le || !sum1 || !sum2)) return MCL_EINVAL;
  if (n_perms == 0 && table) return MCL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned short* tb = static_cast<const unsigned short*>(table);
  return k <= 8 ? hs_launch_perm_all<8>(column_mask, x, ld, dtype, offsets, S, rows, G, max_n, k, nbr, w, pairs, M, mean, den,
                                        tb, n_perms, seed, lag, count_ge, count_le, sum1, sum2, deg, wbar, status, st)
                : hs_launch_perm_all<HS_MAX_K>(column_mask, x, ld, dtype, offsets, S, rows, G, max_n, k, nbr, w, pairs, M,
                                               mean, den, tb, n_perms, seed, lag, count_ge, count_le, sum1, sum2, deg, wbar,
                                               status, st);
}

extern "C" int mcl_hotspot_finalise(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows,
                                    int32_t G, int32_t max_n, const int32_t* pairs, int32_t M, const double* mean,
                                    const double* den, const int32_t* deg, const double* wbar, const double* lag,
                                    const int32_t* count_ge, const int32_t* count_le, const double* sum1, const double* sum2,
                                    int32_t n_perms, double alpha, double* local_i, void* quadrant, double* gi_z,
                                    double* gi_pval_norm, double* gi_neglog10_pval_norm, double* pval_sim, double* mean_sim,
                                    double* var_sim, double* z_sim, void* cluster, mcl_stream_t stream) {
  if (!x || !offsets || !pairs || !mean || !den || !deg || !wbar || !lag || !local_i || !quadrant || !gi_z || !gi_pval_norm ||
      !gi_neglog10_pval_norm)
    return MCL_EINVAL;
  if (!hs_shape_ok(S, rows, max_n) || G < 1 || G > HS_MAX_G || ld < G || (dtype != 0 && dtype != 1) || M < 1 ||
      M > HS_MAX_M || n_perms < 0 || n_perms > HS_MAX_PERMS || !(alpha >= 0.0 && alpha <= 1.0))
    return MCL_EINVAL;
  if (n_perms > 0 && (!count_ge || !count_le || !sum1 || !sum2 || !pval_sim || !mean_sim || !var_sim || !z_sim || !cluster))
    return MCL_EINVAL;
  const long long cells = (long long)max_n * M;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hs_final_kernel, dim3((unsigned)((cells + HS_O_THREADS - 1) / HS_O_THREADS), S), dim3(HS_O_THREADS), 0,
                     static_cast<hipStream_t>(stream), x, (long long)ld, dtype, reinterpret_cast<const long long*>(offsets), S,
                     (long long)rows, G, max_n, pairs, M, mean, den, deg, wbar, lag, count_ge, count_le, sum1, sum2, n_perms,
                     alpha, local_i, static_cast<signed char*>(quadrant), gi_z, gi_pval_norm, gi_neglog10_pval_norm, pval_sim,
                     mean_sim, var_sim, z_sim, static_cast<signed char*>(cluster));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
