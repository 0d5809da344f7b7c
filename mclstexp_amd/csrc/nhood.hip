// How spot groups are arranged in the tissue (squidpy.gr.nhood_enrichment / interaction_matrix / co_occurrence), for every
// slide of an evaluation per call (DESIGN 6.20 states the arithmetic, tests/nhood_reference.py restates it in numpy).  Slide s
// owns rows offsets[s] .. offsets[s + 1]; its KEPT spots (label >= 0) in the stable order by (label, spot) are
// order[offsets[s] + j], j < n, and group c owns the positions start[c] .. start[c + 1] of that order: what
// mcl_ligrec_prepare writes.  Every quantity is an integer count: any schedule gives the same bits.
//
//   nh_compact_kernel   one thread per neighbour slot: (nbr int32, w fp64) -> one uint16, the neighbour's index or 0xFFFF
//                       for a pruned slot (w == 0); a kept slot whose index lies outside the slide counts as pruned and is
//                       counted in the status.
//   nh_counts_kernel    THE HOT PATH.  A workgroup owns (slide, every Z-th permutation, tile of source groups).  Per
//                       permutation it scatters the permuted group byte of every kept spot into LDS (spot order[pi[j]]
//                       receives the group that owns position j), walks the slide's slots -- out of LDS where the uint16
//                       list fits beside labels and cells, else through L2 -- and adds into a tile_rows x K uint32
//                       histogram with LDS integer atomics; a thread then folds the cells it owns into the running sum,
//                       sum of squares, #(>= observed) and #(<= observed), which live in LDS too, and zeroes them.  One
//                       flush by 64-bit integer atomics at the end.  Without a table (pi = identity, once) the same code
//                       writes the observed count.
//   cc_gather_kernel    the coordinates of the kept spots in sorted order; counts the non-finite ones.
//   cc_counts_kernel    a workgroup owns a 256 x 256 tile of ordered pairs (i, j) of sorted positions; a thread owns i and
//                       walks the j of the tile group by group (a group's positions are contiguous), d2 = dx dx + dy dy with
//                       every product and the sum rounded separately, the first radius with d2 <= r2 by a branch-free
//                       search over the 64 padded squared radii in LDS, an LDS atomic on (group of i within the tile, t);
//                       after every group of j the non-zero cells go to pairs[s][t][c1][c2] by integer atomics.
//   cc_prefix_kernel / cc_scores_kernel
//                       the running sum over t, then per (slide, t) the row, column and total sums and
//                       occ = (pairs / row) / (col / tot), NaN where a denominator is 0.
//
// No workgroup reads what another wrote within a launch, no floating-point atomics: a slide inside a batch is bit-identical
// to the same slide alone, run to run.
#include "common.h"

namespace {

constexpr int NH_MAX_N = 16384;          // spots per slide: the uint16 permutation tables of csrc/spatial.hip
constexpr int NH_MAX_K = 255;            // groups per slide: a byte per spot, 255 = dropped
constexpr int NH_MAX_KW = 64;            // neighbour slots per spot
constexpr int NH_MAX_S = 32767;
constexpr int NH_MAX_PERMS = 65535;
constexpr int NH_MAX_T = 64;             // radii
constexpr long long NH_MAX_TOTAL = (1ll << 31) - 1;  // S kmax^2, S T kmax^2
constexpr int NH_THREADS = 1024;
constexpr int NH_LDS_BYTES = 155648;     // dynamic LDS of nh_counts_kernel (152 KiB of the 160)
constexpr int NH_CELL_BYTES = 32;        // per (source group of the tile, target group): sum, sum of squares (8 each),
                                         // histogram, observed, n_ge, n_le (4 each)
constexpr int NH_STATUS = 4;             // the layout of mcl_ligrec_prepare: config, bad labels, [2] bad index, [3] bad coordinate
constexpr unsigned short NH_NONE = 0xFFFF;
constexpr int NH_TARGET_BLOCKS = 1024;   // workgroups a launch of the hot kernel aims at (4 per CU)
constexpr int NH_MIN_PERMS = 4;          // permutations a workgroup takes at least: what the staging is paid back over
constexpr int NH_C_THREADS = 256;
constexpr int CC_TILE = 256;

__host__ __device__ inline int nh_align16(int v) { return (v + 15) & ~15; }
// LDS left beside the two byte arrays of a slide of n rows (group of a spot, group of a sorted position)
__host__ __device__ inline int nh_budget(int n) { return NH_LDS_BYTES - 2 * nh_align16(n); }
__host__ __device__ inline int nh_tile_rows(int n, int K) {
  const int r = nh_budget(n) / (NH_CELL_BYTES * K);
  return r > K ? K : r < 1 ? 1 : r;
}
__host__ __device__ inline bool nh_staged(int n, int K, int kw) {
  return (long long)n * kw * 2 <= (long long)nh_budget(n) - (long long)nh_tile_rows(n, K) * K * NH_CELL_BYTES;
}

// the group that owns sorted position j: the last c < K with start_s[c] <= j (start_s ascending, start_s[0] = 0)
__device__ __forceinline__ int nh_group_of(const int* start_s, int K, int j) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start_s[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------- compact
__global__ __launch_bounds__(NH_C_THREADS) void nh_compact_kernel(
    const long long* __restrict__ offsets, long long rows, int max_n, const int* __restrict__ nbr,
    const double* __restrict__ w, int kw, unsigned short* __restrict__ nbr16, int* __restrict__ status) {
  const int s = blockIdx.y;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int e = blockIdx.x * NH_C_THREADS + threadIdx.x;
  if (e >= ns * kw) return;
  const long long o = r0 * kw + e;
  const int j = nbr[o];
  const bool kept = w[o] != 0.0, inside = j >= 0 && j < ns;
  if (kept && !inside) atomicAdd(&status[NH_STATUS * s + 2], 1);
  nbr16[o] = (kept && inside) ? (unsigned short)j : NH_NONE;
}

// ----------------------------------------------------------------------------------------------------------- counts
__global__ __launch_bounds__(NH_THREADS) void nh_counts_kernel(
    const long long* __restrict__ offsets, const long long* __restrict__ koff, const int* __restrict__ order,
    const int* __restrict__ start, const int* __restrict__ kk, long long rows, int max_n, int kmax,
    const unsigned short* __restrict__ nbr16, int kw, const unsigned short* __restrict__ table, int P,
    int* __restrict__ count, unsigned long long* __restrict__ stats) {
  extern __shared__ __align__(16) unsigned char nh_lds[];
  __shared__ int start_s[NH_MAX_K + 2];
  const int tile = blockIdx.x, z = blockIdx.y, Z = gridDim.y, s = blockIdx.z, tid = threadIdx.x;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int K = kk[s];
  if (ns == 0 || K < 1 || K > kmax) return;
  const int* st = start + (long long)s * (kmax + 1);
  const int n = st[K];
  if (n < 0 || n > ns) return;
  const int tr = nh_tile_rows(ns, K);
  const int g0 = tile * tr;
  if (g0 >= K) return;
  const int g1 = min(K, g0 + tr);
  const int cells = (g1 - g0) * K;

  const int na = nh_align16(ns);
  unsigned char* lab = nh_lds;                                 // [ns]: the group of a spot under the permutation, 255 = dropped
  unsigned char* gpos = nh_lds + na;                           // [n]: the group that owns a sorted position
  unsigned long long* s1 = reinterpret_cast<unsigned long long*>(nh_lds + 2 * na);
  unsigned long long* s2 = s1 + tr * K;
  unsigned* hist = reinterpret_cast<unsigned*>(s2 + tr * K);
  unsigned* obs = hist + tr * K;
  unsigned* ge = obs + tr * K;
  unsigned* le = ge + tr * K;
  unsigned short* nbr_s = reinterpret_cast<unsigned short*>(le + tr * K);
  const bool staged = nh_staged(ns, K, kw);

  for (int c = tid; c <= K; c += NH_THREADS) start_s[c] = min(max(st[c], 0), n);
  for (int i = tid; i < ns; i += NH_THREADS) lab[i] = 255;
  const long long cbase = (long long)s * kmax * kmax;
  for (int e = tid; e < cells; e += NH_THREADS) {
    s1[e] = 0; s2[e] = 0; hist[e] = 0; ge[e] = 0; le[e] = 0;
    obs[e] = table ? (unsigned)count[cbase + (long long)(g0 + e / K) * kmax + e % K] : 0u;
  }
  const int slots = ns * kw;
  const unsigned short* nb = nbr16 + r0 * kw;
  if (staged) {
    for (int e = tid; e < slots; e += NH_THREADS) nbr_s[e] = nb[e];
    nb = nbr_s;
  }
  __syncthreads();
  for (int j = tid; j < n; j += NH_THREADS) gpos[j] = (unsigned char)nh_group_of(start_s, K, j);
  __syncthreads();

  // a slide of fewer than two kept spots has no table (mcl_spatial_permutations skips it): its only permutation is the identity
  const unsigned short* tb = (table && n >= 2) ? table + koff[s] * P : nullptr;
  const int* ord = order + r0;
  const int mine = P > z ? (P - z + Z - 1) / Z : 0;            // the permutations z, z + Z, ...
  for (int m = 0; m < mine; ++m) {
    const unsigned short* pi = tb ? tb + (long long)(z + Z * m) * n : nullptr;
    for (int j = tid; j < n; j += NH_THREADS) {
      const int q = pi ? min((int)pi[j], n - 1) : j;
      lab[min(max(ord[q], 0), ns - 1)] = gpos[j];
    }
    __syncthreads();
    for (int e = tid; e < slots; e += NH_THREADS) {
      const int j = nb[e];
      if (j == NH_NONE) continue;
      const int li = lab[e / kw];
      if (li < g0 || li >= g1) continue;                       // (a dropped spot: 255 >= g1)
      const int lj = lab[j];
      if (lj >= K) continue;
      atomicAdd(&hist[(li - g0) * K + lj], 1u);
    }
    __syncthreads();
    // a thread owns its cells; the next scatter touches lab alone, and the barrier behind it orders this zeroing before
    // the next walk
    for (int e = tid; e < cells; e += NH_THREADS) {
      const unsigned v = hist[e];
      hist[e] = 0;
      if (table) {
        s1[e] += v;
        s2[e] += (unsigned long long)v * v;
        ge[e] += v >= obs[e];
        le[e] += v <= obs[e];
      } else {
        count[cbase + (long long)(g0 + e / K) * kmax + e % K] = (int)v;
      }
    }
  }
  if (!table) return;
  const long long plane = (long long)kmax * kmax;
  unsigned long long* out = stats + (long long)s * 4 * plane;
  for (int e = tid; e < cells; e += NH_THREADS) {
    const long long o = (long long)(g0 + e / K) * kmax + e % K;
    if (s1[e]) atomicAdd(&out[o], s1[e]);
    if (s2[e]) atomicAdd(&out[plane + o], s2[e]);
    if (ge[e]) atomicAdd(&out[2 * plane + o], (unsigned long long)ge[e]);
    if (le[e]) atomicAdd(&out[3 * plane + o], (unsigned long long)le[e]);
  }
}

// ---------------------------------------------------------------------------------------------------- co-occurrence
__global__ __launch_bounds__(NH_C_THREADS) void cc_gather_kernel(
    const double* __restrict__ coords, const long long* __restrict__ offsets, const int* __restrict__ order,
    const int* __restrict__ start, const int* __restrict__ kk, long long rows, int max_n, int kmax,
    double* __restrict__ sorted, int* __restrict__ status) {
  const int s = blockIdx.y;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int K = kk[s];
  if (ns == 0 || K < 1 || K > kmax) return;
  const int n = min(max(start[(long long)s * (kmax + 1) + K], 0), ns);
  const int j = blockIdx.x * NH_C_THREADS + threadIdx.x;
  if (j >= n) return;
  const int spot = min(max(order[r0 + j], 0), ns - 1);
  const double x = coords[(r0 + spot) * 2], y = coords[(r0 + spot) * 2 + 1];
  if (!isfinite(x) || !isfinite(y)) atomicAdd(&status[NH_STATUS * s + 3], 1);
  sorted[(r0 + j) * 2] = x;
  sorted[(r0 + j) * 2 + 1] = y;
}

__global__ __launch_bounds__(CC_TILE) void cc_counts_kernel(
    const double* __restrict__ sorted, const long long* __restrict__ offsets, const int* __restrict__ start,
    const int* __restrict__ kk, long long rows, int max_n, int kmax, const double* __restrict__ r2, int T,
    int* __restrict__ pairs) {
#pragma clang fp contract(off)
  __shared__ double xj_s[CC_TILE], yj_s[CC_TILE], r2_s[NH_MAX_T];
  __shared__ int start_s[NH_MAX_K + 2];
  extern __shared__ __align__(16) unsigned char cc_lds[];
  unsigned* hist_s = reinterpret_cast<unsigned*>(cc_lds);      // [group of i within the tile][t]: at most K groups
  const int s = blockIdx.z, tid = threadIdx.x;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int K = kk[s];
  if (ns == 0 || K < 1 || K > kmax) return;
  const int* st = start + (long long)s * (kmax + 1);
  const int n = min(max(st[K], 0), ns);
  const int i0 = blockIdx.y * CC_TILE, j0 = blockIdx.x * CC_TILE;
  if (i0 >= n || j0 >= n) return;
  const int i1 = min(i0 + CC_TILE, n), j1 = min(j0 + CC_TILE, n);
  for (int c = tid; c <= K; c += CC_TILE) start_s[c] = min(max(st[c], 0), n);
  if (tid < NH_MAX_T) r2_s[tid] = tid < T ? r2[(long long)s * T + tid] : __builtin_huge_val();
  if (j0 + tid < j1) {
    xj_s[tid] = sorted[(r0 + j0 + tid) * 2];
    yj_s[tid] = sorted[(r0 + j0 + tid) * 2 + 1];
  }
  __syncthreads();
  const int i = i0 + tid;
  const bool valid = i < i1;
  const double xi = valid ? sorted[(r0 + i) * 2] : 0.0, yi = valid ? sorted[(r0 + i) * 2 + 1] : 0.0;
  const int glo = nh_group_of(start_s, K, i0), ghi = nh_group_of(start_s, K, i1 - 1);
  const int gi = valid ? nh_group_of(start_s, K, i) - glo : 0;
  const int hcells = (ghi - glo + 1) * T;
  for (int e = tid; e < hcells; e += CC_TILE) hist_s[e] = 0;
  __syncthreads();
  const int cjlo = nh_group_of(start_s, K, j0), cjhi = nh_group_of(start_s, K, j1 - 1);
  for (int c2 = cjlo; c2 <= cjhi; ++c2) {
    const int a = max(start_s[c2], j0), b = min(start_s[c2 + 1], j1);
    if (a >= b) continue;                                      // (uniform: an empty group)
    if (valid) {
      for (int j = a; j < b; ++j) {
        if (j == i) continue;
        const double dx = xi - xj_s[j - j0], dy = yi - yj_s[j - j0];
        const double xx = dx * dx, yy = dy * dy;
        const double d2 = xx + yy;
        int t = 0;                                             // the first t with d2 <= r2[t]: 64 padded entries
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) t += r2_s[t + step - 1] < d2 ? step : 0;
        t += r2_s[t] < d2;
        if (t < T) atomicAdd(&hist_s[gi * T + t], 1u);
      }
    }
    __syncthreads();
    for (int e = tid; e < hcells; e += CC_TILE) {
      const unsigned v = hist_s[e];
      if (v) {
        hist_s[e] = 0;
        const int c1 = glo + e / T, t = e % T;
        atomicAdd(&pairs[(((long long)s * T + t) * kmax + c1) * kmax + c2], (int)v);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NH_C_THREADS) void cc_prefix_kernel(int kmax, int T, int* __restrict__ pairs) {
  const int s = blockIdx.y;
  const int e = blockIdx.x * NH_C_THREADS + threadIdx.x;
  const long long plane = (long long)kmax * kmax;
  if (e >= plane) return;
  int run = 0;
  for (int t = 0; t < T; ++t) {
    const long long o = ((long long)s * T + t) * plane + e;
    run += pairs[o];
    pairs[o] = run;
  }
}

__global__ __launch_bounds__(NH_C_THREADS) void cc_scores_kernel(int kmax, int T, const int* __restrict__ kk,
                                                                 const int* __restrict__ pairs, double* __restrict__ occ) {
  __shared__ int row_s[NH_MAX_K + 1], col_s[NH_MAX_K + 1];
  __shared__ int tot_s;
  const int t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int K = min(max(kk[s], 0), kmax);
  const long long base = ((long long)s * T + t) * kmax * kmax;
  if (tid < K) {
    int r = 0, c = 0;
    for (int q = 0; q < K; ++q) {
      r += pairs[base + (long long)tid * kmax + q];
      c += pairs[base + (long long)q * kmax + tid];
    }
    row_s[tid] = r;
    col_s[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int q = 0; q < K; ++q) tot += row_s[q];
    tot_s = tot;
  }
  __syncthreads();
  const int tot = tot_s;
  for (int e = tid; e < kmax * kmax; e += NH_C_THREADS) {
    const int c1 = e / kmax, c2 = e - c1 * kmax;
    double v = NAN;
    if (c1 < K && c2 < K && row_s[c1] != 0 && col_s[c2] != 0 && tot != 0) {
      const double near = (double)pairs[base + e] / (double)row_s[c1];
      const double prior = (double)col_s[c2] / (double)tot;
      v = near / prior;
    }
    occ[base + e] = v;
  }
}

inline bool nh_shape_ok(int32_t S, int64_t rows, int32_t max_n, int32_t kmax) {
  return S >= 1 && max_n >= 2 && rows >= 2 && rows <= (int64_t)S * max_n && kmax >= 1;
}
inline bool nh_limits_ok(int32_t S, int32_t max_n, int32_t kmax, int64_t planes) {
  return S <= NH_MAX_S && max_n <= NH_MAX_N && kmax <= NH_MAX_K && (long long)S * planes * kmax * kmax <= NH_MAX_TOTAL;
}

}  // namespace

extern "C" int32_t mcl_nhood_tile_rows(int32_t n, int32_t kmax) {
  return (n < 2 || n > NH_MAX_N || kmax < 1 || kmax > NH_MAX_K) ? -1 : nh_tile_rows(n, kmax);
}

extern "C" int32_t mcl_nhood_staged(int32_t n, int32_t kmax, int32_t kw) {
  if (n < 2 || n > NH_MAX_N || kmax < 1 || kmax > NH_MAX_K || kw < 1 || kw > NH_MAX_KW) return -1;
  return nh_staged(n, kmax, kw) ? 1 : 0;
}

extern "C" int64_t mcl_nhood_workspace_bytes(int64_t rows, int32_t kw) {
  if (rows < 2 || rows > (int64_t)NH_MAX_S * NH_MAX_N || kw < 1 || kw > NH_MAX_KW) return -1;
  return rows * kw * 2 + 8;
}

extern "C" int mcl_nhood_counts(const int64_t* offsets, const int64_t* kept_offsets, const int32_t* order,
                                const int32_t* start, const int32_t* k, int32_t S, int64_t rows, int32_t max_n,
                                int32_t kmax, const int32_t* nbr, const double* w, int32_t kw, const void* table,
                                int32_t n_perms, void* work, int32_t* count, int64_t* stats, int32_t* status,
                                mcl_stream_t stream) {
  if (!offsets || !kept_offsets || !order || !start || !k || !nbr || !w || !work || !count || !status) return MCL_EINVAL;
  if (!nh_shape_ok(S, rows, max_n, kmax) || kw < 1 || n_perms < 0 || (table && (!stats || n_perms < 1)) ||
      (!table && n_perms != 0))
    return MCL_EINVAL;
  if (!nh_limits_ok(S, max_n, kmax, 1) || kw > NH_MAX_KW || n_perms > NH_MAX_PERMS) return MCL_EUNSUPPORTED;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nh_counts_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              NH_LDS_BYTES);
  }
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* koff = reinterpret_cast<const long long*>(kept_offsets);
  unsigned short* nbr16 = static_cast<unsigned short*>(work);
  const size_t plane = (size_t)S * kmax * kmax;
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(count, 0, plane * 4, st) != hipSuccess) return (int)hipGetLastError();
  const long long max_slots = (long long)max_n * kw;
  hipLaunchKernelGGL(nh_compact_kernel, dim3((unsigned)((max_slots + NH_C_THREADS - 1) / NH_C_THREADS), S),
                     dim3(NH_C_THREADS), 0, st, off, (long long)rows, max_n, nbr, w, kw, nbr16, status);
  MCL_CHECK_LAUNCH();
  // the largest LDS any slide of the call can ask for: every term bounds its own (n <= max_n, K <= kmax)
  long long lds = 2ll * nh_align16(max_n);
  const long long cell_bytes = (long long)kmax * kmax * NH_CELL_BYTES;
  lds += cell_bytes < nh_budget(max_n) ? cell_bytes : nh_budget(max_n);
  lds += max_slots * 2;
  if (lds > NH_LDS_BYTES) lds = NH_LDS_BYTES;
  const int tr = nh_tile_rows(max_n, kmax);
  const int tiles = (kmax + tr - 1) / tr;                     // (no slide has more: the tiles grow with n and K)
  hipLaunchKernelGGL(nh_counts_kernel, dim3(tiles, 1, S), dim3(NH_THREADS), (size_t)lds, st, off, koff, order, start, k,
                     (long long)rows, max_n, kmax, nbr16, kw, static_cast<const unsigned short*>(nullptr), 1, count,
                     static_cast<unsigned long long*>(nullptr));
  MCL_CHECK_LAUNCH();
  if (!table) return MCL_OK;
  if (hipMemsetAsync(stats, 0, plane * 4 * 8, st) != hipSuccess) return (int)hipGetLastError();
  int Z = (NH_TARGET_BLOCKS + tiles * S - 1) / (tiles * S);
  const int zcap = (n_perms + NH_MIN_PERMS - 1) / NH_MIN_PERMS;
  if (Z > zcap) Z = zcap;
  if (Z > 65535) Z = 65535;
  if (Z < 1) Z = 1;
  hipLaunchKernelGGL(nh_counts_kernel, dim3(tiles, Z, S), dim3(NH_THREADS), (size_t)lds, st, off, koff, order, start, k,
                     (long long)rows, max_n, kmax, nbr16, kw, static_cast<const unsigned short*>(table), n_perms, count,
                     reinterpret_cast<unsigned long long*>(stats));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int64_t mcl_cooccur_workspace_bytes(int64_t rows) {
  if (rows < 2 || rows > (int64_t)NH_MAX_S * NH_MAX_N) return -1;
  return rows * 16 + 8;
}

extern "C" int mcl_cooccur_counts(const double* coords, const int64_t* offsets, const int32_t* order, const int32_t* start,
                                  const int32_t* k, int32_t S, int64_t rows, int32_t max_n, int32_t kmax,
                                  const double* radii_sq, int32_t T, void* work, int32_t* pairs, int32_t* status,
                                  mcl_stream_t stream) {
  if (!coords || !offsets || !order || !start || !k || !radii_sq || !work || !pairs || !status) return MCL_EINVAL;
  if (!nh_shape_ok(S, rows, max_n, kmax) || T < 1) return MCL_EINVAL;
  if (T > NH_MAX_T || !nh_limits_ok(S, max_n, kmax, T)) return MCL_EUNSUPPORTED;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  double* sorted = static_cast<double*>(work);
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(pairs, 0, (size_t)S * T * kmax * kmax * 4, st) != hipSuccess) return (int)hipGetLastError();
  const int tiles = (max_n + CC_TILE - 1) / CC_TILE;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cc_counts_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              NH_MAX_K * NH_MAX_T * 4);
  }
  hipLaunchKernelGGL(cc_gather_kernel, dim3(tiles, S), dim3(NH_C_THREADS), 0, st, coords, off, order, start, k,
                     (long long)rows, max_n, kmax, sorted, status);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_counts_kernel, dim3(tiles, tiles, S), dim3(CC_TILE), (size_t)kmax * T * 4, st, sorted, off, start, k, (long long)rows,
                     max_n, kmax, radii_sq, T, pairs);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_cooccur_scores(const int32_t* k, int32_t S, int32_t kmax, int32_t T, int32_t* pairs, double* occ,
                                  mcl_stream_t stream) {
  if (!k || !pairs || !occ || S < 1 || kmax < 1 || T < 1) return MCL_EINVAL;
  if (T > NH_MAX_T || S > NH_MAX_S || kmax > NH_MAX_K || (long long)S * T * kmax * kmax > NH_MAX_TOTAL)
    return MCL_EUNSUPPORTED;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(cc_prefix_kernel, dim3((kmax * kmax + NH_C_THREADS - 1) / NH_C_THREADS, S), dim3(NH_C_THREADS), 0, st,
                     kmax, T, pairs);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_scores_kernel, dim3(T, S), dim3(NH_C_THREADS), 0, st, kmax, T, k, pairs, occ);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
