// Ligand-receptor permutation test between spot groups (squidpy.gr.ligrec, the CellPhoneDB test), for every slide of an
// evaluation per call (DESIGN 6.19 states the arithmetic, tests/ligrec_reference.py restates it in numpy).  Slide s owns rows
// offsets[s] .. offsets[s + 1] of x (rows, G) and labels (rows,); its KEPT spots (label >= 0) in the stable order by
// (label, spot) are order[offsets[s] + j], j < n; group c owns the positions start[c] .. start[c + 1] of that order.
//
//   lr_prepare_kernel   one workgroup per slide: validates the labels (one outside -1 .. K - 1 is counted and dropped),
//                       counts the groups, and writes order by one wave per group walking the slide in ascending spot order
//                       (ballot + prefix count: stable, no sort).  lr_scan_kernel: the offsets of the kept spots.
//   lr_means_kernel     THE HOT PATH.  A workgroup takes one slide and C of the used gene columns -- as many as its LDS holds,
//                       1, 2, 4 or 8 --, gathers them in sorted order into LDS once (column-interleaved fp64) and walks its
//                       share of a chunk of permutations: a wave takes one (permutation, group), lane l reads pi[start + t]
//                       for t = l, l + 64, ... through the uint16 table of mcl_spatial_permutations, gathers the C values of
//                       that spot from LDS and adds them; the 64 lanes are combined by the halving tree, the C columns
//                       sharing its upper levels (lr_tree_total).  Without a table
//                       (pi = identity) the same code writes the observed sum, nnz, mean and frac.
//   lr_observed_kernel  one workgroup per (slide, interaction): picks the member of a complex with the lowest mean over the
//                       kept spots, then the observed means and the defined mask of every ordered group pair.
//   lr_count_kernel     one workgroup per (slide, interaction): stages the permuted group means of the two genes for a tile
//                       of permutations in LDS; a thread owns (c1, c2) and adds its comparisons into the int32 count.
//
// THE FIXED ORDER of a group sum over a segment of m spots: lane l of 64 adds the values at segment positions l, l + 64, ...
// in ascending order, starting from 0; the lanes are combined by the halving tree p[l] += p[l + o], o = 32, 16, ... 1.  It is
// a function of m alone.  Every sum is rounded separately.  No floating-point atomics, no workgroup waits for another: a
// slide inside a batch is bit-identical to the same slide alone.
#include "common.h"

namespace {

constexpr int LR_MAX_N = 16384;          // spots per slide: the uint16 permutation tables of csrc/spatial.hip
constexpr int LR_MAX_K = 255;            // groups per slide: a byte per spot in lr_prepare_kernel, 255 = dropped
constexpr int LR_MAX_G = 16384;
constexpr int LR_MAX_S = 32767;
constexpr int LR_MAX_PERMS = 65535;
constexpr int LR_MAX_I = 65535;          // interactions: grid.x
constexpr long long LR_MAX_CELLS = 1ll << 24;        // I * kmax^2 per slide
constexpr long long LR_MAX_TOTAL = (1ll << 31) - 1;  // S * I * kmax^2
constexpr int LR_THREADS = 1024;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_CMAX = 8;
constexpr int LR_X_BYTES = 155648;       // LDS for the gathered columns (152 KiB of the 160)
constexpr int LR_O_THREADS = 256;
constexpr int LR_STAGE = 2048;           // doubles per gene staged by lr_count_kernel: 2 x 16 KiB
constexpr int LR_STATUS = 4;             // config, labels out of range, non-finite x, negative x
constexpr long long LR_CHUNK_BYTES = 256ll << 20;    // the permuted means of one chunk
constexpr int LR_TARGET_BLOCKS = 1024;   // workgroups a launch of the hot kernel aims at (4 per CU)

__host__ __device__ inline int lr_columns(int n) {
  const int c = LR_X_BYTES / (8 * (n < 1 ? 1 : n));
  return c >= 8 ? 8 : c >= 4 ? 4 : c >= 2 ? 2 : 1;
}

inline long long lr_chunk(long long S, long long kmax, long long U, long long P) {
  long long c = LR_CHUNK_BYTES / (S * kmax * U * 8);
  if (c > P) c = P;
  return c < 1 ? 1 : c;
}

// The halving tree over the 64 lanes for W columns at once.  At a level that still holds more than one column the lanes with
// bit o set keep the upper half of the columns and hand the lower half to their partner, the others the reverse: every lane
// adds its own value of a column and its partner's (lanes l and l ^ o: the two numbers p[l] += p[l + o] adds), so each
// column's total is the stated tree's, bit for bit, at 1 + W / 2 + ... shuffles a level instead of W.  Every lane returns
// the total of column lr_lane_column<W>(lane).
template <int W>
__device__ __forceinline__ double lr_tree_total(const double* v, int lane, int o) {
#pragma clang fp contract(off)
  if constexpr (W == 1) {
    double a = v[0];
    for (; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
    return a;
  } else {
    constexpr int H = W / 2;
    const bool hi = (lane & o) != 0;
    double nv[H];
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const double keep = hi ? v[j + H] : v[j], send = hi ? v[j] : v[j + H];
      nv[j] = keep + __shfl_xor(send, o, 64);
    }
    return lr_tree_total<H>(nv, lane, o >> 1);
  }
}
template <int W>
__device__ __forceinline__ int lr_lane_column(int lane) {
  int col = 0, o = 32;
#pragma unroll
  for (int w = W; w > 1; w >>= 1, o >>= 1) col += (lane & o) ? w / 2 : 0;
  return col;
}

// ---------------------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(LR_THREADS) void lr_prepare_kernel(
    const long long* __restrict__ offsets, const int* __restrict__ labels, const int* __restrict__ kk, long long rows,
    int max_n, int kmax, int* __restrict__ order, int* __restrict__ start, int* __restrict__ status) {
  __shared__ unsigned char lab_s[LR_MAX_N];
  __shared__ int cnt_s[LR_MAX_K + 1];
  __shared__ int start_s[LR_MAX_K + 2];
  __shared__ int bad_s;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int K = kk[s];
  int* st = start + (long long)s * (kmax + 1);
  if (ns == 0 || K < 1 || K > kmax) {
    for (int c = tid; c <= kmax; c += LR_THREADS) st[c] = 0;
    if (tid == 0) status[LR_STATUS * s] = 1;
    return;
  }
  for (int c = tid; c <= LR_MAX_K; c += LR_THREADS) cnt_s[c] = 0;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < ns; i += LR_THREADS) {
    const int l = labels[r0 + i];
    bad += l < -1 || l >= K;
    const int code = (l >= 0 && l < K) ? l : 255;
    lab_s[i] = (unsigned char)code;
    if (code != 255) atomicAdd(&cnt_s[code], 1);
  }
  if (bad) atomicAdd(&bad_s, bad);
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int c = 0; c < K; ++c) {
      start_s[c] = run;
      run += cnt_s[c];
    }
    start_s[K] = run;
    if (bad_s) status[LR_STATUS * s + 1] = bad_s;
  }
  __syncthreads();
  const int n = start_s[K];
  for (int c = tid; c <= kmax; c += LR_THREADS) st[c] = c <= K ? start_s[c] : n;
  int* ord = order + r0;
  for (int c = wave; c < K; c += LR_WAVES) {
    int run = start_s[c];
    for (int base = 0; base < ns; base += 64) {
      const int i = base + lane;
      const bool match = i < ns && lab_s[i] == c;
      const unsigned long long mask = __ballot(match);
      if (match) ord[run + (int)lanes_below(mask)] = i;
      run += __popcll(mask);
    }
  }
  for (int j = n + tid; j < ns; j += LR_THREADS) ord[j] = -1;
}

__global__ void lr_scan_kernel(int S, int kmax, const int* __restrict__ start, long long* __restrict__ koff) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long run = 0;
  koff[0] = 0;
  for (int s = 0; s < S; ++s) {
    run += start[(long long)s * (kmax + 1) + kmax];
    koff[s + 1] = run;
  }
}

// ------------------------------------------------------------------------------------------------------ group means
template <typename T, int C>
__global__ __launch_bounds__(LR_THREADS) void lr_means_kernel(
    const T* __restrict__ x, long long ld, const long long* __restrict__ offsets, const long long* __restrict__ koff,
    const int* __restrict__ order, const int* __restrict__ start, const int* __restrict__ kk, long long rows, int G,
    int max_n, int kmax, const int* __restrict__ used, int U, const unsigned short* __restrict__ table, int P, int p0,
    int pc, int pcap, double* __restrict__ sum_out, int* __restrict__ nnz_out, double* __restrict__ mean_out,
    double* __restrict__ frac_out, double* __restrict__ pmean, int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char lr_lds[];
  __shared__ int start_s[LR_MAX_K + 2];
  __shared__ int nonfinite_s, negative_s;
  double* xs = reinterpret_cast<double*>(lr_lds);            // [n][C]: sorted position j, column q
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long r0;
  const int ns = segment_rows(offsets, s, rows, 2, max_n, &r0);
  const int K = kk[s];
  if (ns == 0 || K < 1 || K > kmax) return;
  const int* st = start + (long long)s * (kmax + 1);
  const int n = st[K];
  if (n < 0 || n > ns || lr_columns(n) != C) return;
  const int u0 = blockIdx.x * C;
  if (u0 >= U) return;
  const int cc = min(C, U - u0);
  for (int c = tid; c <= K; c += LR_THREADS) start_s[c] = min(max(st[c], 0), n);
  if (tid == 0) { nonfinite_s = 0; negative_s = 0; }
  __syncthreads();

  // the gather: sorted position j takes spot order[j]; a column past U reads the tile's last one
  const int* ord = order + r0;
  const int total = n * C;
  int nf = 0, ng = 0;
  for (int e = tid; e < total; e += LR_THREADS) {
    const int j = e / C, q = e - j * C;
    const int r = min(max(ord[j], 0), ns - 1);
    const int col = min(max(used[u0 + (q < cc ? q : cc - 1)], 0), G - 1);
    const double v = ldd(x + (r0 + (long long)r) * ld + col);
    if (q < cc) {
      nf += !isfinite(v);
      ng += v < 0.0;
    }
    xs[e] = v;
  }
  if (!table && blockIdx.z == 0) {
    if (nf) atomicAdd(&nonfinite_s, nf);
    if (ng) atomicAdd(&negative_s, ng);
  }
  __syncthreads();
  if (!table && blockIdx.z == 0 && tid == 0) {
    if (nonfinite_s) atomicAdd(&status[LR_STATUS * s + 2], nonfinite_s);
    if (negative_s) atomicAdd(&status[LR_STATUS * s + 3], negative_s);
  }

  // a slide of one kept spot has no table (mcl_spatial_permutations needs two rows): its only permutation is the identity
  const unsigned short* tb = (table && n >= 2) ? table + koff[s] * P : nullptr;
  const int Z = gridDim.z, z = blockIdx.z;
  const int mine = pc > z ? (pc - z + Z - 1) / Z : 0;         // the local permutations z, z + Z, ... of this chunk
  const int items = mine * K;
  const int nm1 = n - 1;
  for (int item = wave; item < items; item += LR_WAVES) {
    const int lp = z + Z * (item / K), c = item % K;
    const int a = start_s[c], m = start_s[c + 1] - a;
    const unsigned short* pi = tb ? tb + (long long)(p0 + lp) * n + a : nullptr;
    double acc[C];
    int cnt[C];
#pragma unroll
    for (int q = 0; q < C; ++q) { acc[q] = 0.0; cnt[q] = 0; }
    for (int t = lane; t < m; t += 256) {
      int r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tt = t + 64 * u;
        r[u] = tt < m ? (pi ? min((int)pi[tt], nm1) : a + tt) : -1;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (r[u] >= 0) {
          const double* row = xs + r[u] * C;
#pragma unroll
          for (int q = 0; q < C; ++q) {
            const double v = row[q];
            acc[q] = acc[q] + v;
            cnt[q] += v > 0.0;
          }
        }
      }
    }
    // every lane ends with the total of its column q; the first lane of each group of 64 / C lanes writes it
    const int q = lr_lane_column<C>(lane);
    const double tot = lr_tree_total<C>(acc, lane, 32);
    const bool writer = (lane & (64 / C - 1)) == 0 && q < cc;
    const double size = (double)m;
    if (table) {
      if (writer) pmean[(((long long)s * pcap + lp) * U + u0 + q) * kmax + c] = tot / size;
    } else {
      int nz = 0;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        const int cj = wave_sum(cnt[j]);
        if (j == q) nz = cj;
      }
      if (writer) {
        const long long o = ((long long)s * kmax + c) * U + u0 + q;
        sum_out[o] = tot;
        nnz_out[o] = nz;
        mean_out[o] = tot / size;
        frac_out[o] = (double)nz / size;
      }
    }
  }
  // the groups past K of a slide with fewer groups than kmax: NaN means, as an empty group
  if (!table && z == 0) {
    for (int e = tid; e < (kmax - K) * cc; e += LR_THREADS) {
      const int c = K + e / cc, q = e % cc;
      const long long o = ((long long)s * kmax + c) * U + u0 + q;
      sum_out[o] = 0.0;
      nnz_out[o] = 0;
      mean_out[o] = NAN;
      frac_out[o] = NAN;
    }
  }
}

// --------------------------------------------------------------------------------------------------------- observed
__global__ __launch_bounds__(LR_O_THREADS) void lr_observed_kernel(
    int I, int kmax, int U, const int* __restrict__ kk, const int* __restrict__ start, const double* __restrict__ sum,
    const int* __restrict__ nnz, const double* __restrict__ mean, const int* __restrict__ moff,
    const int* __restrict__ members, double threshold, int* __restrict__ pairs, double* __restrict__ means,
    int* __restrict__ defined, int* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ int pick_s[2];
  const int i = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int K = min(max(kk[s], 0), kmax);
  const int* st = start + (long long)s * (kmax + 1);
  if (tid < 2) {
    const int m0 = moff[2 * i + tid], m1 = moff[2 * i + tid + 1];
    int best = min(max(members[m0], 0), U - 1);
    if (m1 - m0 > 1) {                                       // a complex: the member of lowest mean over the kept spots
      const double nd = (double)st[kmax];
      double bestv = 0.0;
      for (int m = m0; m < m1; ++m) {
        const int u = min(max(members[m], 0), U - 1);
        double tot = 0.0;
        for (int c = 0; c < K; ++c) tot = tot + sum[((long long)s * kmax + c) * U + u];
        const double mv = tot / nd;
        if (m == m0 || mv < bestv) { best = u; bestv = mv; }
      }
    }
    pick_s[tid] = best;
    pairs[((long long)s * I + i) * 2 + tid] = best;
  }
  __syncthreads();
  const int ia = pick_s[0], ib = pick_s[1];
  for (int e = tid; e < kmax * kmax; e += LR_O_THREADS) {
    const int c1 = e / kmax, c2 = e - c1 * kmax;
    const long long o = ((long long)s * I + i) * kmax * kmax + e;
    double mv = NAN;
    int def = 0;
    if (c1 < K && c2 < K) {
      const long long oa = ((long long)s * kmax + c1) * U + ia, ob = ((long long)s * kmax + c2) * U + ib;
      const double m1 = mean[oa], m2 = mean[ob];
      const bool pos = m1 > 0.0 && m2 > 0.0;
      if (!isnan(m1) && !isnan(m2)) mv = pos ? (m1 + m2) / 2.0 : 0.0;
      const double s1 = (double)(st[c1 + 1] - st[c1]), s2 = (double)(st[c2 + 1] - st[c2]);
      const bool e1 = (double)nnz[oa] >= threshold * s1, e2 = (double)nnz[ob] >= threshold * s2;
      def = pos && e1 && e2;
    }
    means[o] = mv;
    defined[o] = def;
    count[o] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------ count
__global__ __launch_bounds__(LR_O_THREADS) void lr_count_kernel(
    int I, int kmax, int U, const int* __restrict__ kk, const double* __restrict__ mean, const int* __restrict__ pairs,
    const double* __restrict__ pmean, int pcap, int pc, int* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ double a_s[LR_STAGE], b_s[LR_STAGE];
  const int i = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int K = min(max(kk[s], 0), kmax);
  if (K < 1) return;
  const int ia = min(max(pairs[((long long)s * I + i) * 2], 0), U - 1);
  const int ib = min(max(pairs[((long long)s * I + i) * 2 + 1], 0), U - 1);
  const int PT = LR_STAGE / K;                               // permutations per tile: >= 8
  for (int t0 = 0; t0 < pc; t0 += PT) {
    const int np = min(PT, pc - t0);
    for (int e = tid; e < np * K; e += LR_O_THREADS) {
      const int p = e / K, c = e - p * K;
      const long long base = ((long long)s * pcap + t0 + p) * U;
      a_s[e] = pmean[(base + ia) * kmax + c];
      b_s[e] = pmean[(base + ib) * kmax + c];
    }
    __syncthreads();
    for (int e = tid; e < K * K; e += LR_O_THREADS) {
      const int c1 = e / K, c2 = e - c1 * K;
      const double m1 = mean[((long long)s * kmax + c1) * U + ia], m2 = mean[((long long)s * kmax + c2) * U + ib];
      const double obs = (m1 + m2) / 2.0;
      int cnt = 0;
      for (int p = 0; p < np; ++p) cnt += (a_s[p * K + c1] + b_s[p * K + c2]) / 2.0 >= obs;
      count[((long long)s * I + i) * kmax * kmax + c1 * kmax + c2] += cnt;
    }
    __syncthreads();
  }
}

inline bool lr_shape_ok(int32_t S, int64_t rows, int32_t max_n, int32_t kmax) {
  return S >= 1 && S <= LR_MAX_S && max_n >= 2 && rows >= 2 && rows <= (int64_t)S * max_n && kmax >= 1;
}
inline bool lr_limits_ok(int32_t max_n, int32_t kmax) { return max_n <= LR_MAX_N && kmax <= LR_MAX_K; }

template <typename T, int C>
int lr_launch_means(const void* x, int64_t ld, const int64_t* offsets, const int64_t* koff, const int32_t* order,
                    const int32_t* start, const int32_t* kk, int S, int64_t rows, int G, int max_n, int kmax,
                    const int32_t* used, int U, const unsigned short* table, int P, int p0, int pc, int pcap, double* sum,
                    int32_t* nnz, double* mean, double* frac, double* pmean, int32_t* status, hipStream_t st) {
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lr_means_kernel<T, C>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, LR_X_BYTES);
  }
  const int tiles = (U + C - 1) / C;
  int Z = 1;
  if (table) {
    Z = (LR_TARGET_BLOCKS + tiles * S - 1) / (tiles * S);
    if (Z > pc) Z = pc;
    if (Z > 64) Z = 64;
    if (Z < 1) Z = 1;
  }
  long long lds = (long long)max_n * C * 8;
  if (lds > LR_X_BYTES) lds = LR_X_BYTES;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL((lr_means_kernel<T, C>), dim3(tiles, S, Z), dim3(LR_THREADS), (size_t)lds, st,
                     static_cast<const T*>(x), (long long)ld, reinterpret_cast<const long long*>(offsets),
                     reinterpret_cast<const long long*>(koff), order, start, kk, (long long)rows, G, max_n, kmax, used, U,
                     table, P, p0, pc, pcap, sum, nnz, mean, frac, pmean, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

template <typename T>
int lr_launch_means_all(int cmask, const void* x, int64_t ld, const int64_t* offsets, const int64_t* koff,
                        const int32_t* order, const int32_t* start, const int32_t* kk, int S, int64_t rows, int G,
                        int max_n, int kmax, const int32_t* used, int U, const unsigned short* table, int P, int p0, int pc,
                        int pcap, double* sum, int32_t* nnz, double* mean, double* frac, double* pmean, int32_t* status,
                        hipStream_t st) {
  int rc = MCL_OK;
#define LR_ONE(C)                                                                                                      \
  if (rc == MCL_OK && (cmask >> C) & 1)                                                                                \
    rc = lr_launch_means<T, C>(x, ld, offsets, koff, order, start, kk, S, rows, G, max_n, kmax, used, U, table, P, p0, \
                               pc, pcap, sum, nnz, mean, frac, pmean, status, st)
  LR_ONE(1); LR_ONE(2); LR_ONE(4); LR_ONE(8);
  static_assert(LR_CMAX == 8, "one launch per column count");
#undef LR_ONE
  return rc;
}

}  // namespace

extern "C" int32_t mcl_ligrec_columns(int32_t n) { return (n < 0 || n > LR_MAX_N) ? -1 : lr_columns(n); }

extern "C" int32_t mcl_ligrec_chunk(int32_t S, int32_t kmax, int32_t U, int32_t n_perms) {
  if (S < 1 || S > LR_MAX_S || kmax < 1 || kmax > LR_MAX_K || U < 1 || U > LR_MAX_G || n_perms < 1 ||
      n_perms > LR_MAX_PERMS)
    return -1;
  return (int32_t)lr_chunk(S, kmax, U, n_perms);
}

extern "C" int64_t mcl_ligrec_workspace_bytes(int32_t S, int32_t kmax, int32_t U, int32_t n_perms) {
  const int32_t chunk = mcl_ligrec_chunk(S, kmax, U, n_perms);
  if (chunk < 0) return -1;
  return (int64_t)S * chunk * kmax * U * 8 + 8;
}

extern "C" int mcl_ligrec_prepare(const int64_t* offsets, const int32_t* labels, const int32_t* k, int32_t S, int64_t rows,
                                  int32_t max_n, int32_t kmax, int32_t* order, int32_t* start, int64_t* kept_offsets,
                                  int32_t* status, mcl_stream_t stream) {
  if (!offsets || !labels || !k || !order || !start || !kept_offsets || !status) return MCL_EINVAL;
  if (!lr_shape_ok(S, rows, max_n, kmax)) return MCL_EINVAL;
  if (!lr_limits_ok(max_n, kmax)) return MCL_EUNSUPPORTED;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(status, 0, (size_t)S * LR_STATUS * 4, st) != hipSuccess) return (int)hipGetLastError();
  hipLaunchKernelGGL(lr_prepare_kernel, dim3(S), dim3(LR_THREADS), 0, st, reinterpret_cast<const long long*>(offsets),
                     labels, k, (long long)rows, max_n, kmax, order, start, status);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(lr_scan_kernel, dim3(1), dim3(64), 0, st, S, kmax, start, reinterpret_cast<long long*>(kept_offsets));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_ligrec_group_means(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets,
                                      const int64_t* kept_offsets, const int32_t* order, const int32_t* start,
                                      const int32_t* k, int32_t S, int64_t rows, int32_t G, int32_t max_n, int32_t kmax,
                                      const int32_t* used, int32_t U, int32_t column_mask, const void* table,
                                      int32_t n_perms, int32_t p0, int32_t pc, int32_t chunk, double* sum, int32_t* nnz,
                                      double* mean, double* frac, double* perm_means, int32_t* status, mcl_stream_t stream) {
  if (!x || !offsets || !kept_offsets || !order || !start || !k || !used || !status) return MCL_EINVAL;
  if (!lr_shape_ok(S, rows, max_n, kmax) || G < 1 || U < 1 || U > G || ld < G || (dtype != 0 && dtype != 1) ||
      (column_mask & ~0x116) || !column_mask)
    return MCL_EINVAL;
  if (!lr_limits_ok(max_n, kmax) || G > LR_MAX_G) return MCL_EUNSUPPORTED;
  if (table) {
    if (!perm_means || n_perms < 1 || n_perms > LR_MAX_PERMS || p0 < 0 || pc < 1 || p0 + pc > n_perms || pc > chunk ||
        chunk > lr_chunk(S, kmax, U, n_perms))
      return MCL_EINVAL;
  } else if (!sum || !nnz || !mean || !frac) {
    return MCL_EINVAL;
  } else {
    n_perms = 1; p0 = 0; pc = 1; chunk = 1;                 // the observed pass: the identity, once
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned short* tb = static_cast<const unsigned short*>(table);
  return dtype == 0 ? lr_launch_means_all<float>(column_mask, x, ld, offsets, kept_offsets, order, start, k, S, rows, G,
                                                 max_n, kmax, used, U, tb, n_perms, p0, pc, chunk, sum, nnz, mean, frac,
                                                 perm_means, status, st)
                    : lr_launch_means_all<double>(column_mask, x, ld, offsets, kept_offsets, order, start, k, S, rows, G,
                                                  max_n, kmax, used, U, tb, n_perms, p0, pc, chunk, sum, nnz, mean, frac,
                                                  perm_means, status, st);
}

static bool lr_cells_ok(int32_t S, int32_t I, int32_t kmax) {
  if (S < 1 || S > LR_MAX_S || I < 1 || I > LR_MAX_I || kmax < 1 || kmax > LR_MAX_K) return false;
  const long long cells = (long long)I * kmax * kmax;
  return cells <= LR_MAX_CELLS && cells * S <= LR_MAX_TOTAL;
}

extern "C" int mcl_ligrec_observed(int32_t S, int32_t I, int32_t kmax, int32_t U, const int32_t* k, const int32_t* start,
                                   const double* sum, const int32_t* nnz, const double* mean,
                                   const int32_t* member_offsets, const int32_t* members, double threshold, int32_t* pairs,
                                   double* means, int32_t* defined, int32_t* count, mcl_stream_t stream) {
  if (!k || !start || !sum || !nnz || !mean || !member_offsets || !members || !pairs || !means || !defined || !count)
    return MCL_EINVAL;
  if (U < 1 || !(threshold >= 0.0 && threshold <= 1.0) || S < 1 || I < 1 || kmax < 1) return MCL_EINVAL;
  if (!lr_cells_ok(S, I, kmax) || U > LR_MAX_G) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(lr_observed_kernel, dim3(I, S), dim3(LR_O_THREADS), 0, static_cast<hipStream_t>(stream), I, kmax, U, k,
                     start, sum, nnz, mean, member_offsets, members, threshold, pairs, means, defined, count);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_ligrec_count(int32_t S, int32_t I, int32_t kmax, int32_t U, const int32_t* k, const double* mean,
                                const int32_t* pairs, const double* perm_means, int32_t chunk, int32_t pc, int32_t* count,
                                mcl_stream_t stream) {
  if (!k || !mean || !pairs || !perm_means || !count) return MCL_EINVAL;
  if (U < 1 || chunk < 1 || pc < 1 || pc > chunk || S < 1 || I < 1 || kmax < 1) return MCL_EINVAL;
  if (!lr_cells_ok(S, I, kmax) || U > LR_MAX_G || chunk > LR_MAX_PERMS) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(lr_count_kernel, dim3(I, S), dim3(LR_O_THREADS), 0, static_cast<hipStream_t>(stream), I, kmax, U, k,
                     mean, pairs, perm_means, chunk, pc, count);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
