// Count tables -> highly variable genes -> the preprocessed expression matrices (the reference's hvg_her2st.py,
// hvg_cscc.py, hvg_visium.py): per slide scanpy's normalize_total(target_sum=None), log1p and
// highly_variable_genes(flavor="seurat", n_bins=20, n_top_genes), then the union / intersection of the per-slide flags and
// scprep's log(library_size_normalize(.)) of the chosen columns, written transposed.  S slides per call, each a row-major
// (n_s, G_s) fp32 or int32 matrix of its own, described by device-resident pointer / leading-dimension / row-count arrays;
// an optional int32 column map per slide gives the slide's columns of the G shared genes (no subset copy on the host).
//
// mcl_hvg_stats, four launches, everything fp64, no floating-point atomics (the LDS histograms are integer):
//   hvg_libsize_kernel  grid (ceil(max_rows/4), S): one wave per spot sums its counts over the G shared genes (four strided
//                       partials per lane, a fixed tree, then the wave butterfly).
//   hvg_target_kernel   one workgroup per slide: the median of the positive library sizes by an exact 8-bit radix select on
//                       the ordered bit patterns (both middle elements when their number is even), then the size factors
//                       f_i = s_i / median (1 where that is 0) over the library sizes, in place.
//   hvg_moments_kernel  grid (ceil(G/64), S), 4 waves: lane = gene, the waves stride over the spots (4 in flight per wave),
//                       sums of x = c / f_i and of x * x (product rounded, as numpy's multiply-then-mean), the four waves
//                       combined in wave order; then mean, var = (E[x^2] - mean^2) n / (n - 1), the 1e-12 floor,
//                       dispersion = var / mean (0 -> NaN), dispersions = log(.), means = log1p(.).
//   hvg_select_kernel   one workgroup per slide: pandas.cut's 20 bins (numpy.linspace edges, the lowest moved down by 0.1 % of
//                       the range, right-closed), per bin the mean and ddof=1 standard deviation of the non-NaN dispersions
//                       (two passes, per-thread partials per bin in LDS and a fixed tree), the single-gene rule,
//                       dispersions_norm, the cut-off by the same radix select, and the flags.
// The second kernel is the only one that writes what the first one wrote; every count is read twice (library sizes,
// moments).  Every summation order depends only on (n_s, G): a slide inside a batch is bit-identical to the slide alone.
// mcl_hvg_pool: union / intersection of the flags over the slides, then union[extra] = true.
// mcl_expression_matrices: grid (ceil(max_rows/64), S); a workgroup sums 64 spots over the K chosen columns, then walks the
//   columns 64 at a time through an LDS tile so that reads run along a spot's row and writes along the (K, n_s) output's.
#include <float.h>

#include "common.h"

namespace {

constexpr int N_BINS = 20;
constexpr int LIB_WAVES = 4;
constexpr int MOM_WAVES = 4;
constexpr int MOM_UNROLL = 4;     // spots per wave per trip
constexpr int FIN_THREADS = 256;  // == the radix of the select (one histogram bin per thread)
constexpr int MAX_G = 1 << 20;
constexpr int MAX_ROWS = 50000;

enum { ST_FLAT = 1, ST_NO_COUNTS = 2, ST_NO_DISPERSION = 4, ST_BAD_MAP = 8 };

struct SlideSet {  // device-resident arrays, one entry per slide (row_off: S + 1 entries, the spots before the slide)
  const void* const* ptr;
  const long long* ld;
  const int* rows;
  const int* ncols;
  const long long* row_off;
};

// The value of descending rank k (0 = the largest) among the valid entries of v[0..n): the positive ones (POSITIVE) or the
// non-NaN ones.  Exact: eight passes fix one byte of the key each.  Called by all FIN_THREADS threads with 0 <= k < the
// number of valid entries; hist: FIN_THREADS ints, pick: 2 ints of LDS.
template <bool POSITIVE>
__device__ double block_select_desc(const double* v, int n, int k, int* hist, int* pick) {
  const int tid = threadIdx.x;
  u64 prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FIN_THREADS) {
      const double x = v[i];
      if (POSITIVE ? x > 0.0 : !isnan(x)) {
        const u64 key = order_key(x);
        if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int d = 255, kk = k;
      for (; d > 0; --d) {
        if (kk < hist[d]) break;
        kk -= hist[d];
      }
      pick[0] = d;
      pick[1] = kk;
    }
    __syncthreads();
    prefix |= (u64)pick[0] << shift;
    mask |= 0xFFull << shift;
    k = pick[1];
    __syncthreads();
  }
  return key_value(prefix);
}

// ------------------------------------------------------------------------------------------------ 1. library sizes
template <typename T>
__global__ __launch_bounds__(LIB_WAVES * 64) void hvg_libsize_kernel(SlideSet sl, const int* __restrict__ colmaps, int G,
                                                                     double* __restrict__ lib) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.y;
  const int row = blockIdx.x * LIB_WAVES + (threadIdx.x >> 6);
  if (row >= sl.rows[s]) return;
  const int nc = sl.ncols[s];
  const T* x = static_cast<const T*>(sl.ptr[s]) + (long long)row * sl.ld[s];
  const int* map = colmaps ? colmaps + (long long)s * G : nullptr;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int g0 = lane; g0 < G; g0 += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = g0 + 64 * u;
      if (g < G) acc[u] += (double)x[clamp_index(map ? map[g] : g, nc)];
    }
  }
  const double a = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (lane == 0) lib[sl.row_off[s] + row] = a;
}

// ------------------------------------------------------------------------------ 2. median target and the size factors
__global__ __launch_bounds__(FIN_THREADS) void hvg_target_kernel(SlideSet sl, const int* __restrict__ colmaps, int G,
                                                                 double* __restrict__ lib, double* __restrict__ target_sum,
                                                                 int* __restrict__ status) {
  __shared__ int hist[FIN_THREADS];
  __shared__ int pick[2];
  __shared__ int n_pos;
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int n = sl.rows[s];
  double* v = lib + sl.row_off[s];
  if (tid == 0) n_pos = 0;
  __syncthreads();
  int bad = 0, pos = 0;
  if (colmaps) {
    const int nc = sl.ncols[s];
    for (int g = tid; g < G; g += FIN_THREADS) {
      const int c = colmaps[(long long)s * G + g];
      bad |= (c < 0 || c >= nc);
    }
  } else {
    bad = sl.ncols[s] < G;
  }
  for (int i = tid; i < n; i += FIN_THREADS) pos += v[i] > 0.0;
  if (pos) atomicAdd(&n_pos, pos);
  bad = __syncthreads_or(bad);
  const int m = n_pos;
  double med = NAN;  // numpy's median of an empty array
  if (m > 0) {
    // ascending positions (m - 1) / 2 and m / 2 = descending ranks m - 1 - (m - 1) / 2 and m - 1 - m / 2
    const double hi = block_select_desc<true>(v, n, m - 1 - m / 2, hist, pick);
    const double lo = (m & 1) ? hi : block_select_desc<true>(v, n, m - 1 - (m - 1) / 2, hist, pick);
    med = (m & 1) ? hi : (lo + hi) / 2.0;
  }
  for (int i = tid; i < n; i += FIN_THREADS) {
    double f = v[i] / med;
    if (f == 0.0) f = 1.0;  // counts += counts == 0
    v[i] = f;
  }
  if (tid == 0) {
    target_sum[s] = med;
    status[s] = (bad ? ST_BAD_MAP : 0) | (m > 0 ? 0 : ST_NO_COUNTS);
  }
}

// ------------------------------------------------------------------------------------------------ 3. gene moments
template <typename T>
__global__ __launch_bounds__(MOM_WAVES * 64) void hvg_moments_kernel(SlideSet sl, const int* __restrict__ colmaps, int G,
                                                                     const double* __restrict__ fac,
                                                                     double* __restrict__ means,
                                                                     double* __restrict__ dispersions) {
#pragma clang fp contract(off)  // numpy rounds every product and every sum: no fused multiply-add in here
  __shared__ double part[2][MOM_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int g = blockIdx.x * 64 + lane;
  const int gc = g < G ? g : G - 1;  // lanes past G load gene G-1 and store nothing
  const int n = sl.rows[s];
  const long long ld = sl.ld[s];
  const int c = clamp_index(colmaps ? colmaps[(long long)s * G + gc] : gc, sl.ncols[s]);
  const T* col = static_cast<const T*>(sl.ptr[s]) + c;
  const double* f = fac + sl.row_off[s];
  constexpr int STEP = MOM_WAVES * MOM_UNROLL;
  double sx = 0.0, sxx = 0.0;
  for (int base = w; base < n; base += STEP) {
    double xv[MOM_UNROLL];
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const int row = min(base + u * MOM_WAVES, n - 1);
      xv[u] = (double)col[(long long)row * ld] / f[row];
    }
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const double x = base + u * MOM_WAVES < n ? xv[u] : 0.0;
      sx += x;
      sxx += x * x;
    }
  }
  part[0][w][lane] = sx;
  part[1][w][lane] = sxx;
  __syncthreads();
  if (w == 0 && g < G) {
    for (int v = 1; v < MOM_WAVES; ++v) {  // fixed order: wave 0 + wave 1 + wave 2 + wave 3
      sx += part[0][v][lane];
      sxx += part[1][v][lane];
    }
    const double nn = (double)n;
    double mean = sx / nn;
    const double mean_sq = sxx / nn;
    double var = mean_sq - mean * mean;
    var *= nn / (nn - 1.0);
    if (mean == 0.0) mean = 1e-12;
    double d = var / mean;
    if (d == 0.0) d = NAN;
    const long long o = (long long)s * G + g;
    dispersions[o] = log(d);
    means[o] = log1p(mean);
  }
}

// ---------------------------------------------------------- 4. bins, normalised dispersions, cut-off and the flags
__device__ __forceinline__ double nan_to_num(double v) {
  return isnan(v) ? 0.0 : (isinf(v) ? (v > 0.0 ? DBL_MAX : -DBL_MAX) : v);
}

// sum of part[b][0 .. FIN_THREADS) into part[b][0] for every bin, a fixed tree
__device__ __forceinline__ void bin_tree(double (*part)[FIN_THREADS]) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int h = FIN_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      for (int b = 0; b < N_BINS; ++b) part[b][tid] += part[b][tid + h];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(FIN_THREADS) void hvg_select_kernel(int G, int n_top, const double* __restrict__ means_all,
                                                                 const double* __restrict__ disp_all,
                                                                 double* __restrict__ norm_all, int* __restrict__ bin_all,
                                                                 unsigned char* __restrict__ hv_all,
                                                                 double* __restrict__ cutoff, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double part[N_BINS][FIN_THREADS];
  __shared__ double edge[N_BINS + 1];
  __shared__ double bmean[N_BINS], bstd[N_BINS];
  __shared__ int bcnt[N_BINS];
  __shared__ int hist[FIN_THREADS];
  __shared__ int pick[2];
  __shared__ int n_valid;
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const double* m = means_all + (long long)s * G;
  const double* d = disp_all + (long long)s * G;
  double* z = norm_all + (long long)s * G;
  int* bin = bin_all + (long long)s * G;
  unsigned char* hv = hv_all + (long long)s * G;

  // min / max of the means (order-free), a non-finite mean disqualifies the slide
  double mn = INFINITY, mx = -INFINITY;
  int odd = 0;
  for (int g = tid; g < G; g += FIN_THREADS) {
    const double x = m[g];
    odd |= !isfinite(x);
    mn = fmin(mn, x);
    mx = fmax(mx, x);
  }
  part[0][tid] = mn;
  part[1][tid] = mx;
  if (tid < N_BINS) bcnt[tid] = 0;
  if (tid == 0) n_valid = 0;
  odd = __syncthreads_or(odd);
  for (int h = FIN_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      part[0][tid] = fmin(part[0][tid], part[0][tid + h]);
      part[1][tid] = fmax(part[1][tid], part[1][tid + h]);
    }
    __syncthreads();
  }
  mn = part[0][0];
  mx = part[1][0];
  __syncthreads();
  if (odd || !(mx > mn)) {  // pandas.cut widens a flat range by 0.1 % of the value: not reproduced, reported
    for (int g = tid; g < G; g += FIN_THREADS) {
      z[g] = NAN;
      bin[g] = 0;
      hv[g] = 0;
    }
    if (tid == 0) {
      cutoff[s] = NAN;
      status[s] |= ST_FLAT;
    }
    return;
  }
  // numpy.linspace(mn, mx, 21): arange * step + start with the last one set to mx; then bins[0] -= 0.1 % of the range
  if (tid <= N_BINS) {
    const double step = (mx - mn) / (double)N_BINS;
    double e = (double)tid * step + mn;
    if (tid == N_BINS) e = mx;
    if (tid == 0) e = e - (mx - mn) * 0.001;
    edge[tid] = e;
  }
  for (int b = 0; b < N_BINS; ++b) part[b][tid] = 0.0;
  __syncthreads();

  // bin = (edges strictly below the mean) - 1 (searchsorted side="left"); sums of the non-NaN dispersions per bin
  for (int g = tid; g < G; g += FIN_THREADS) {
    const double x = m[g];
    int below = 0;
    for (int j = 0; j <= N_BINS; ++j) below += edge[j] < x;
    const int b = min(max(below - 1, 0), N_BINS - 1);
    bin[g] = b;
    const double dv = d[g];
    if (!isnan(dv)) {
      part[b][tid] += dv;
      atomicAdd(&bcnt[b], 1);
    }
  }
  bin_tree(part);
  if (tid < N_BINS) bmean[tid] = part[tid][0] / (double)bcnt[tid];  // 0 / 0 = NaN: the mean of an empty group
  __syncthreads();
  for (int b = 0; b < N_BINS; ++b) part[b][tid] = 0.0;
  __syncthreads();
  for (int g = tid; g < G; g += FIN_THREADS) {
    const double dv = d[g];
    if (!isnan(dv)) {
      const int b = bin[g];  // written by this thread
      const double r = dv - bmean[b];
      part[b][tid] += r * r;
    }
  }
  bin_tree(part);
  if (tid < N_BINS) {
    const int c = bcnt[tid];
    double sd = c >= 2 ? sqrt(part[tid][0] / (double)(c - 1)) : NAN;
    if (c < 2) {  // std is NaN: the bin's only gene gets a normalised dispersion of 1
      sd = bmean[tid];
      bmean[tid] = 0.0;
    }
    bstd[tid] = sd;
  }
  __syncthreads();

  int valid = 0;
  for (int g = tid; g < G; g += FIN_THREADS) {
    const int b = bin[g];
    const double v = (d[g] - bmean[b]) / bstd[b];
    z[g] = v;
    valid += !isnan(v);
  }
  if (valid) atomicAdd(&n_valid, valid);
  __syncthreads();  // z[] is read back by the whole workgroup below
  const int k = min(n_top, n_valid);
  double cut = NAN;
  if (k > 0) cut = block_select_desc<false>(z, G, k - 1, hist, pick);
  for (int g = tid; g < G; g += FIN_THREADS) hv[g] = nan_to_num(z[g]) >= cut;
  if (tid == 0) {
    cutoff[s] = cut;
    if (k == 0) status[s] |= ST_NO_DISPERSION;
  }
}

// ------------------------------------------------------------------------------------------------------- pooling
__global__ __launch_bounds__(256) void hvg_pool_kernel(const unsigned char* __restrict__ hv, int S, int G,
                                                       unsigned char* __restrict__ uni, unsigned char* __restrict__ inter) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  int any = 0, all = 1;
  for (int s = 0; s < S; ++s) {
    const int f = hv[(long long)s * G + g] != 0;
    any |= f;
    all &= f;
  }
  uni[g] = (unsigned char)any;
  inter[g] = (unsigned char)all;
}

__global__ __launch_bounds__(256) void hvg_force_kernel(const int* __restrict__ extra, int n_extra, int G,
                                                        unsigned char* __restrict__ uni) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_extra) return;
  const int g = extra[i];
  if (g >= 0 && g < G) uni[g] = 1;
}

// ------------------------------------------------------------------------------------- the preprocessed matrices
template <typename T>
__global__ __launch_bounds__(256) void expr_matrices_kernel(SlideSet sl, const int* __restrict__ sel_all, int K,
                                                            float rescale, float* __restrict__ out) {
  __shared__ float tile[64][65];
  __shared__ float fac[64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int n = sl.rows[s];
  const int row0 = blockIdx.x * 64;
  if (row0 >= n) return;
  const int nc = sl.ncols[s];
  const long long ld = sl.ld[s];
  const T* x = static_cast<const T*>(sl.ptr[s]);
  const int* sel = sel_all + (long long)s * K;
  float* y = out + (long long)K * sl.row_off[s];  // (K, n) row-major

  for (int rr = 0; rr < 16; ++rr) {  // library size over the chosen genes: exact in fp64 for counts
    const int r = w * 16 + rr;
    const int row = row0 + r;
    double a = 0.0;
    if (row < n) {
      const T* xr = x + (long long)row * ld;
      for (int k = lane; k < K; k += 64) a += (double)xr[clamp_index(sel[k], nc)];
    }
    a = wave_sum(a);
    if (lane == 0) fac[r] = a != 0.0 ? (float)((double)rescale / a) : 0.f;  // an empty spot stays all-zero
  }
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const int c = clamp_index(k < K ? sel[k] : 0, nc);
    for (int rr = 0; rr < 16; ++rr) {
      const int r = w * 16 + rr;
      const int row = row0 + r;
      const float v = (row < n && k < K) ? (float)x[(long long)row * ld + c] : 0.f;
      tile[r][lane] = log10f(fmaf(v, fac[r], 1.0f));
    }
    __syncthreads();
    for (int kk = 0; kk < 16; ++kk) {
      const int ko = k0 + w * 16 + kk;
      if (ko < K && row0 + lane < n) y[(long long)ko * n + row0 + lane] = tile[lane][w * 16 + kk];
    }
    __syncthreads();
  }
}

SlideSet slide_set(const void* const* slides, const int64_t* ld, const int32_t* rows, const int32_t* ncols,
                   const int64_t* row_offsets) {
  return SlideSet{slides, reinterpret_cast<const long long*>(ld), rows, ncols,
                  reinterpret_cast<const long long*>(row_offsets)};
}

}  // namespace

extern "C" int mcl_hvg_stats(const void* const* slides, const int64_t* ld, const int32_t* rows, const int32_t* ncols,
                             const int64_t* row_offsets, int32_t dtype, const int32_t* colmaps, int32_t S, int32_t G,
                             int32_t max_rows, int32_t n_top_genes, double* work, double* means, double* dispersions,
                             double* dispersions_norm, int32_t* mean_bin, uint8_t* highly_variable, double* cutoff,
                             double* target_sum, int32_t* status, mcl_stream_t stream) {
  if (!slides || !ld || !rows || !ncols || !row_offsets || !work || !means || !dispersions || !dispersions_norm ||
      !mean_bin || !highly_variable || !cutoff || !target_sum || !status)
    return MCL_EINVAL;
  if (S < 1 || G < 2 || max_rows < 2 || n_top_genes < 1 || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (S > 65535 || G > MAX_G || max_rows > MAX_ROWS) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const SlideSet sl = slide_set(slides, ld, rows, ncols, row_offsets);
  MCL_CLEAR_ERROR();
  const dim3 lib_grid((max_rows + LIB_WAVES - 1) / LIB_WAVES, S), mom_grid((G + 63) / 64, S);
  if (dtype == 0)
    hipLaunchKernelGGL(hvg_libsize_kernel<float>, lib_grid, dim3(LIB_WAVES * 64), 0, st, sl, colmaps, G, work);
  else
    hipLaunchKernelGGL(hvg_libsize_kernel<int>, lib_grid, dim3(LIB_WAVES * 64), 0, st, sl, colmaps, G, work);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(hvg_target_kernel, dim3(S), dim3(FIN_THREADS), 0, st, sl, colmaps, G, work, target_sum, status);
  MCL_CHECK_LAUNCH();
  if (dtype == 0)
    hipLaunchKernelGGL(hvg_moments_kernel<float>, mom_grid, dim3(MOM_WAVES * 64), 0, st, sl, colmaps, G, work, means,
                       dispersions);
  else
    hipLaunchKernelGGL(hvg_moments_kernel<int>, mom_grid, dim3(MOM_WAVES * 64), 0, st, sl, colmaps, G, work, means,
                       dispersions);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(hvg_select_kernel, dim3(S), dim3(FIN_THREADS), 0, st, G, n_top_genes, means, dispersions,
                     dispersions_norm, mean_bin, highly_variable, cutoff, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_hvg_pool(const uint8_t* highly_variable, int32_t S, int32_t G, const int32_t* extra, int32_t n_extra,
                            uint8_t* union_out, uint8_t* intersection_out, mcl_stream_t stream) {
  if (!highly_variable || !union_out || !intersection_out || S < 1 || G < 1 || n_extra < 0 || (n_extra > 0 && !extra))
    return MCL_EINVAL;
  const hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hvg_pool_kernel, dim3((G + 255) / 256), dim3(256), 0, st, highly_variable, S, G, union_out,
                     intersection_out);
  MCL_CHECK_LAUNCH();
  if (n_extra > 0) {
    hipLaunchKernelGGL(hvg_force_kernel, dim3((n_extra + 255) / 256), dim3(256), 0, st, extra, n_extra, G, union_out);
    MCL_CHECK_LAUNCH();
  }
  return MCL_OK;
}

extern "C" int mcl_expression_matrices(const void* const* slides, const int64_t* ld, const int32_t* rows,
                                       const int32_t* ncols, const int64_t* row_offsets, int32_t dtype, const int32_t* sel,
                                       int32_t S, int32_t K, int32_t max_rows, float rescale, float* out,
                                       mcl_stream_t stream) {
  if (!slides || !ld || !rows || !ncols || !row_offsets || !sel || !out) return MCL_EINVAL;
  if (S < 1 || K < 1 || max_rows < 1 || (dtype != 0 && dtype != 1) || !(rescale > 0.f)) return MCL_EINVAL;
  if (S > 65535 || K > MAX_G || max_rows > MAX_ROWS) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const SlideSet sl = slide_set(slides, ld, rows, ncols, row_offsets);
  const dim3 grid((max_rows + 63) / 64, S);
  MCL_CLEAR_ERROR();
  if (dtype == 0)
    hipLaunchKernelGGL(expr_matrices_kernel<float>, grid, dim3(256), 0, st, sl, sel, K, rescale, out);
  else
    hipLaunchKernelGGL(expr_matrices_kernel<int>, grid, dim3(256), 0, st, sl, sel, K, rescale, out);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
