// The spot neighbourhood graph (scanpy's sc.pp.neighbors with umap-learn's weights, exact at every size) for every segment
// (slide) of a row-stacked matrix; the arithmetic is the one DESIGN 6.11 states.  Everything is fp64, there are no
// floating-point atomics, and no result depends on the order in which workgroups or lanes arrive: a segment inside a batch
// is bit-identical to the same segment alone, and a run to its repeat.
//
//   mcl_knn_exact            nb_knn_kernel: one workgroup per row; the row's n_s squared distances are computed once into
//                            LDS; an exact radix select over the key (bits of d^2, j) -- eight 8-bit digits of d^2, two of
//                            j -- finds the (k-1)-th smallest other row, ties by index; the k-1 winners are gathered and
//                            rank-sorted in LDS.
//   mcl_knn_smooth           nb_smooth_kernel: one wave per row; lanes hold the row, exp() runs in parallel, the sum runs in
//                            index order in every lane (the lanes agree on every branch without a barrier).
//                            nb_floor_kernel: one workgroup per segment; the segment's mean distance in a fixed order, the
//                            floor of the rows without a positive distance.
//   mcl_knn_connectivities   phase 0: nb_indegree_kernel (integer atomics), nb_scan_kernel, nb_reverse_kernel (the reverse
//                            edges slotted by integer atomics; their order inside a row is arbitrary and never shows),
//                            nb_union_kernel<false> (the row's weights scattered by column into LDS, counted),
//                            nb_indptr_kernel.  phase 1: nb_union_kernel<true>: the same LDS row, compacted in column order,
//                            so every CSR row is ascending whatever the atomics did.
//
// Segments ride on grid.y; a segment the launch was not sized for is skipped; an index outside its segment is ignored.
#include "common.h"

namespace {

constexpr int NB_MAX_D = 64;
constexpr int NB_MAX_N = 16384;                 // one row of distances in LDS: 128 KiB of the 160 KiB
constexpr int NB_MAX_K = 256;
constexpr int NB_MAX_S = 65535;                 // grid.y
constexpr int NB_THREADS = 256;
constexpr int NB_SMOOTH_STEPS = 64;             // umap-learn's n_iter
constexpr double NB_SMOOTH_TOL = 1e-5;          // SMOOTH_K_TOLERANCE
constexpr double NB_MIN_SCALE = 1e-3;           // MIN_K_DIST_SCALE
constexpr int NB_SLOTS = NB_MAX_K / 64;         // entries of a row a lane holds

// Exclusive prefix of v over the 256 threads in thread order and, in *total, the sum.  `ws` holds 4 ints; two barriers.
__device__ __forceinline__ int nb_block_scan(int v, int* ws, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int t = ws[w];
    before += w < wave ? t : 0;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

// one count per matching lane into hist[digit]; a wave whose matching lanes agree on the digit (the leading bytes of the
// distances of a row nearly always do) adds once.  Called by whole waves.
__device__ __forceinline__ void nb_hist_add(int* hist, bool match, int digit) {
  const unsigned long long act = __ballot(match);
  if (act == 0) return;
  const int first = __ffsll((long long)act) - 1;
  const int d0 = __shfl(digit, first, 64);
  const unsigned long long same = __ballot(match && digit == d0);
  if (same == act) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], __popcll(act));
  } else if (match) {
    atomicAdd(&hist[digit], 1);
  }
}

// ------------------------------------------------------------------------------------------------------------- kNN
// dynamic LDS: dist[max_n] doubles | xi[64] doubles | wkey[256] u64 | widx[256] int | hist[256] int | misc[8] int
template <typename T>
__global__ __launch_bounds__(NB_THREADS) void nb_knn_kernel(const T* __restrict__ x, long long ld, int D,
                                                            const long long* __restrict__ off, int max_n, long long rows,
                                                            int k, int* __restrict__ out_idx, double* __restrict__ out_dist) {
  extern __shared__ __attribute__((aligned(16))) char nb_smem[];
  double* dist = reinterpret_cast<double*>(nb_smem);
  double* xi = dist + max_n;
  u64* wkey = reinterpret_cast<u64*>(xi + NB_MAX_D);
  int* widx = reinterpret_cast<int*>(wkey + NB_MAX_K);
  int* hist = widx + NB_MAX_K;
  int* misc = hist + NB_THREADS;               // 0..3 scan, 4 digit, 5 rank left, 6 winners
  long long o;
  int n;
  if (!segment_span(off, blockIdx.y, k, max_n, rows, &o, &n)) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= n) return;
  if (tid < D) xi[tid] = (double)x[(o + i) * ld + tid];
  if (tid == 0) misc[6] = 0;
  __syncthreads();
  for (int j = tid; j < n; j += NB_THREADS) dist[j] = ts_sqdist(xi, x + (o + j) * ld, D);
  __syncthreads();
  // the other row of ascending rank k - 2 under (bits of d^2, j): d^2 >= +0, so the bits order as the values do
  u64 prefix = 0, mask = 0;
  int jprefix = 0, jmask = 0, want = k - 2;
  for (int pass = 0; pass < 10; ++pass) {
    const int shift = pass < 8 ? 56 - 8 * pass : (pass == 8 ? 8 : 0);
    hist[tid] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += NB_THREADS) {
      const int j = base + tid;
      bool match = j < n && j != i;
      int digit = 0;
      if (match) {
        const u64 key = (u64)__double_as_longlong(dist[j]);
        match = (key & mask) == prefix && (j & jmask) == jprefix;
        digit = pass < 8 ? (int)((key >> shift) & 255) : (j >> shift) & 255;
      }
      nb_hist_add(hist, match, digit);
    }
    __syncthreads();
    const int h = hist[tid];
    int total;
    const int before = nb_block_scan(h, misc, &total);
    if (want >= before && want < before + h) {   // one thread: want < the matching rows by construction
      misc[4] = tid;
      misc[5] = want - before;
    }
    __syncthreads();
    if (pass < 8) {
      prefix |= (u64)misc[4] << shift;
      mask |= 0xFFull << shift;
    } else {
      jprefix |= misc[4] << shift;
      jmask |= 0xFF << shift;
    }
    want = misc[5];
    __syncthreads();
  }
  // the k - 1 rows at or below (prefix, jprefix), in arrival order
  for (int j = tid; j < n; j += NB_THREADS) {
    if (j == i) continue;
    const u64 key = (u64)__double_as_longlong(dist[j]);
    if (key < prefix || (key == prefix && j <= jprefix)) {
      const int slot = atomicAdd(&misc[6], 1);
      if (slot < NB_MAX_K) {
        wkey[slot] = key;
        widx[slot] = j;
      }
    }
  }
  __syncthreads();
  const int m = misc[6] < k - 1 ? misc[6] : k - 1;
  int* oi = out_idx + (o + i) * k;
  double* od = out_dist + (o + i) * k;
  if (tid == 0) {
    oi[0] = i;
    od[0] = 0.0;
  }
  if (tid < m) {
    const u64 key = wkey[tid];
    const int j = widx[tid];
    int rank = 0;
    for (int u = 0; u < m; ++u) {
      const u64 ku = wkey[u];
      rank += (ku < key || (ku == key && widx[u] < j)) ? 1 : 0;
    }
    oi[1 + rank] = j;
    od[1 + rank] = sqrt(__longlong_as_double((long long)key));
  }
}

// ---------------------------------------------------------------------------------------------------------- smoothing
// sum of e[1 .. k-1] in index order, the same in every lane; lane l holds entry 64 c + l in e[c]
__device__ __forceinline__ double nb_ordered_sum(const double (&e)[NB_SLOTS], int first, int k) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < NB_SLOTS; ++c) {
    if (64 * c >= k) break;
    for (int l = 0; l < 64; ++l) {
      const int j = 64 * c + l;
      const double v = __shfl(e[c], l, 64);
      if (j >= first && j < k) s += v;
    }
  }
  return s;
}

// one wave per row: rho, the search for sigma, the row's own floor; rowsum[row] = the sum of the row's k distances
__global__ __launch_bounds__(NB_THREADS) void nb_smooth_kernel(const double* __restrict__ dist, long long rows, int k,
                                                               double target, double* __restrict__ rho_out,
                                                               double* __restrict__ sigma_out,
                                                               double* __restrict__ rowsum) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                       // a whole wave
  const double* d = dist + row * k;
  double dl[NB_SLOTS], e[NB_SLOTS];
  double rho = INFINITY;
#pragma unroll
  for (int c = 0; c < NB_SLOTS; ++c) {
    const int j = 64 * c + lane;
    dl[c] = j < k ? d[j] : 0.0;
    if (dl[c] > 0.0) rho = fmin(rho, dl[c]);
  }
  rho = wave_min(rho);
  if (rho == INFINITY) rho = 0.0;
  const double total = nb_ordered_sum(dl, 0, k);
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int step = 0; step < NB_SMOOTH_STEPS; ++step) {
#pragma unroll
    for (int c = 0; c < NB_SLOTS; ++c) {
      const double t = dl[c] - rho;
      e[c] = t > 0.0 ? exp(-(t / mid)) : 1.0;
    }
    const double psum = nb_ordered_sum(e, 1, k);   // the same in every lane
    if (fabs(psum - target) < NB_SMOOTH_TOL) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  if (rho > 0.0) mid = fmax(mid, NB_MIN_SCALE * (total / (double)k));
  if (lane == 0) {
    rho_out[row] = rho;
    sigma_out[row] = mid;
    rowsum[row] = total;
  }
}

// one workgroup per segment: the mean of its (n_s, k) distances (threads stride the row sums, butterfly, the four waves in
// order), then the floor of the rows without a positive distance
__global__ __launch_bounds__(NB_THREADS) void nb_floor_kernel(const long long* __restrict__ off, int max_n, long long rows,
                                                              int k, const double* __restrict__ rowsum,
                                                              const double* __restrict__ rho,
                                                              double* __restrict__ sigma) {
  __shared__ double red[4];
  long long o;
  int n;
  if (!segment_span(off, blockIdx.x, k, max_n, rows, &o, &n)) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += NB_THREADS) s += rowsum[o + i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const double mean = (((red[0] + red[1]) + red[2]) + red[3]) / ((double)n * (double)k);
  for (int i = threadIdx.x; i < n; i += NB_THREADS)
    if (!(rho[o + i] > 0.0)) sigma[o + i] = fmax(sigma[o + i], NB_MIN_SCALE * mean);
}

// ----------------------------------------------------------------------------------------------------- connectivities
// the directed weight of j in row i's list at distance d
__device__ __forceinline__ double nb_weight(double d, double rho, double sigma, bool self) {
  if (self) return 0.0;
  const double t = d - rho;
  if (t <= 0.0 || sigma == 0.0) return 1.0;
  return exp(-(t / sigma));
}

// mix (a + b - a b) + (1 - mix) a b, every product and sum rounded on its own as numpy's elementwise arithmetic does
__device__ __forceinline__ double nb_combine(double a, double b, double mix) {
#pragma clang fp contract(off)
  const double prod = a * b;
  const double uni = (a + b) - prod;
  const double l = mix * uni;
  const double r = (1.0 - mix) * prod;
  return l + r;
}

// the workspace of mcl_knn_connectivities, in bytes from its start
struct nb_work {
  double* rev_w;      // rows * k: the weight of every reverse edge
  int* rev_src;       // rows * k: its source row
  int* indeg;         // rows
  int* cursor;        // rows: the slots handed out, then the entries of every CSR row
  int* rev_ptr;       // rows: where a row's reverse edges begin, from its segment's off[s] * k
};
__host__ __device__ inline nb_work nb_carve(void* work, long long rows, int k) {
  nb_work w;
  w.rev_w = static_cast<double*>(work);
  w.rev_src = reinterpret_cast<int*>(w.rev_w + rows * k);
  w.indeg = w.rev_src + rows * k;
  w.cursor = w.indeg + rows;
  w.rev_ptr = w.cursor + rows;
  return w;
}

// one workgroup per row, thread t its t-th neighbour: the in-degree of the neighbour
__global__ __launch_bounds__(NB_THREADS) void nb_indegree_kernel(const int* __restrict__ idx,
                                                                 const long long* __restrict__ off, int max_n,
                                                                 long long rows, int k, int* __restrict__ indeg) {
  long long o;
  int n;
  if (!segment_span(off, blockIdx.y, k, max_n, rows, &o, &n)) return;
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= n || t >= k) return;
  const int j = idx[(o + i) * k + t];
  if (j == i || j < 0 || j >= n) return;
  atomicAdd(&indeg[o + j], 1);
}

// one workgroup per segment: out[i] = the sum of in[0 .. i) over the segment's rows
__global__ __launch_bounds__(NB_THREADS) void nb_scan_kernel(const long long* __restrict__ off, int max_n, long long rows,
                                                             int k, const int* __restrict__ in, int* __restrict__ out) {
  __shared__ int ws[4];
  long long o;
  int n;
  if (!segment_span(off, blockIdx.x, k, max_n, rows, &o, &n)) return;
  int carry = 0;
  for (int base = 0; base < n; base += NB_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < n ? in[o + i] : 0;
    int total;
    const int before = nb_block_scan(v, ws, &total);
    if (i < n) out[o + i] = carry + before;
    carry += total;
  }
}

// every directed edge i -> j lands in j's reverse list with its weight; the slot is whichever the atomic hands out
__global__ __launch_bounds__(NB_THREADS) void nb_reverse_kernel(const int* __restrict__ idx, const double* __restrict__ dist,
                                                                const double* __restrict__ rho,
                                                                const double* __restrict__ sigma,
                                                                const long long* __restrict__ off, int max_n,
                                                                long long rows, int k, nb_work w) {
  long long o;
  int n;
  if (!segment_span(off, blockIdx.y, k, max_n, rows, &o, &n)) return;
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= n || t >= k) return;
  const int j = idx[(o + i) * k + t];
  if (j == i || j < 0 || j >= n) return;
  const int slot = atomicAdd(&w.cursor[o + j], 1);
  const long long at = o * k + w.rev_ptr[o + j] + slot;
  if (slot >= w.indeg[o + j] || at >= (o + n) * k) return;    // cannot happen after nb_indegree_kernel on the same lists
  w.rev_src[at] = i;
  w.rev_w[at] = nb_weight(dist[(o + i) * k + t], rho[o + i], sigma[o + i], false);
}

// One workgroup per row i.  val[j] (dynamic LDS, n_s doubles) becomes the symmetric weight of (i, j) or -1 where there is
// no edge: the reverse edges give b, the row's own list a, their union the entries.  FILL = false counts the entries that
// are not 0; FILL = true writes them in column order from where indptr says.
template <bool FILL>
__global__ __launch_bounds__(NB_THREADS) void nb_union_kernel(const int* __restrict__ idx, const double* __restrict__ dist,
                                                              const double* __restrict__ rho,
                                                              const double* __restrict__ sigma,
                                                              const long long* __restrict__ off, int max_n, long long rows,
                                                              int k, double mix, nb_work w,
                                                              const long long* __restrict__ indptr,
                                                              const long long* __restrict__ nnz_off, long long nnz_total,
                                                              int* __restrict__ indices, double* __restrict__ data) {
  extern __shared__ __attribute__((aligned(16))) char nb_smem[];
  double* val = reinterpret_cast<double*>(nb_smem);
  int* ws = reinterpret_cast<int*>(val + max_n);
  long long o;
  int n;
  const int s = blockIdx.y;
  if (!segment_span(off, s, k, max_n, rows, &o, &n)) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= n) return;
  for (int j = tid; j < n; j += NB_THREADS) val[j] = -1.0;
  __syncthreads();
  const int deg = min(w.indeg[o + i], n);
  const long long at = o * k + w.rev_ptr[o + i];
  const bool in_range = at >= o * k && at + deg <= (o + n) * k;
  if (in_range)
    for (int t = tid; t < deg; t += NB_THREADS) {
      const int j = w.rev_src[at + t];
      if (j >= 0 && j < n && j != i) val[j] = w.rev_w[at + t];
    }
  __syncthreads();
  int mine = -1;
  double both = 0.0;
  if (tid < k) {
    const int j = idx[(o + i) * k + tid];
    if (j >= 0 && j < n && j != i) {
      const double a = nb_weight(dist[(o + i) * k + tid], rho[o + i], sigma[o + i], false);
      const double b = val[j];
      mine = j;
      both = nb_combine(a, b < 0.0 ? 0.0 : b, mix);
    }
  }
  __syncthreads();
  if (in_range)
    for (int t = tid; t < deg; t += NB_THREADS) {
      const int j = w.rev_src[at + t];
      if (j >= 0 && j < n && j != i) val[j] = nb_combine(0.0, w.rev_w[at + t], mix);
    }
  __syncthreads();
  if (mine >= 0) val[mine] = both;
  __syncthreads();
  long long base = 0;
  if (FILL) base = nnz_off[s] + indptr[o + s + i];
  int carry = 0;
  for (int j0 = 0; j0 < n; j0 += NB_THREADS) {
    const int j = j0 + tid;
    const double v = j < n ? val[j] : -1.0;
    const int keep = (v != -1.0 && v != 0.0) ? 1 : 0;
    int total;
    const int before = nb_block_scan(keep, ws, &total);
    if (FILL && keep) {
      const long long p = base + carry + before;
      if (p >= 0 && p < nnz_total) {
        indices[p] = j;
        data[p] = v;
      }
    }
    carry += total;
  }
  if (!FILL && tid == 0) w.cursor[o + i] = carry;
}

// one workgroup per segment: indptr of its CSR (n_s + 1 entries from off[s] + s) and its nnz
__global__ __launch_bounds__(NB_THREADS) void nb_indptr_kernel(const long long* __restrict__ off, int max_n, long long rows,
                                                               int k, const int* __restrict__ count,
                                                               long long* __restrict__ indptr, long long* __restrict__ nnz) {
  __shared__ int ws[4];
  long long o;
  int n;
  const int s = blockIdx.x;
  if (!segment_span(off, s, k, max_n, rows, &o, &n)) {
    if (threadIdx.x == 0) nnz[s] = -1;
    return;
  }
  long long carry = 0;
  for (int base = 0; base < n; base += NB_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < n ? count[o + i] : 0;
    int total;
    const int before = nb_block_scan(v, ws, &total);
    if (i < n) indptr[o + s + i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    indptr[o + s + n] = carry;
    nnz[s] = carry;
  }
}

int nb_limits(int S, long long rows, int min_n, int max_n, int k) {
  if (S <= 0 || rows <= 0) return MCL_EINVAL;
  if (S > NB_MAX_S || max_n > NB_MAX_N || k > NB_MAX_K) return MCL_EUNSUPPORTED;
  if (k < 2 || min_n < 2 || min_n < k || min_n > max_n || rows < (long long)S * min_n || rows > (long long)S * max_n)
    return MCL_EINVAL;
  return MCL_OK;
}

}  // namespace

extern "C" {

int64_t mcl_knn_workspace_bytes(int32_t rows, int32_t k) {
  if (rows <= 0 || k < 2 || k > NB_MAX_K) return 0;
  // the larger of mcl_knn_smooth's (rows doubles) and mcl_knn_connectivities' (nb_carve)
  return (int64_t)rows * k * (8 + 4) + (int64_t)rows * 3 * 4 + 16;
}

int mcl_knn_exact(const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets, int32_t S, int32_t rows,
                  int32_t min_n, int32_t max_n, int32_t k, int32_t* knn_indices, double* knn_distances,
                  mcl_stream_t stream) {
  if (!x || !offsets || !knn_indices || !knn_distances || D <= 0 || ld < D || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (D > NB_MAX_D) return MCL_EUNSUPPORTED;
  const int rc = nb_limits(S, rows, min_n, max_n, k);
  if (rc != MCL_OK) return rc;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  constexpr size_t fixed = NB_MAX_D * 8 + NB_MAX_K * (8 + 4) + NB_THREADS * 4 + 8 * 4;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nb_knn_kernel<float>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NB_MAX_N * 8 + fixed);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nb_knn_kernel<double>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NB_MAX_N * 8 + fixed);
  }
  MCL_CLEAR_ERROR();
  const size_t lds = (size_t)max_n * 8 + fixed;
  if (dtype == 0)
    hipLaunchKernelGGL(nb_knn_kernel<float>, dim3(max_n, S), dim3(NB_THREADS), lds, st, (const float*)x, (long long)ld, D,
                       off, max_n, (long long)rows, k, knn_indices, knn_distances);
  else
    hipLaunchKernelGGL(nb_knn_kernel<double>, dim3(max_n, S), dim3(NB_THREADS), lds, st, (const double*)x, (long long)ld,
                       D, off, max_n, (long long)rows, k, knn_indices, knn_distances);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_knn_smooth(const double* knn_distances, const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n,
                   int32_t max_n, int32_t k, void* work, double* rho, double* sigma, mcl_stream_t stream) {
  if (!knn_distances || !offsets || !work || !rho || !sigma) return MCL_EINVAL;
  const int rc = nb_limits(S, rows, min_n, max_n, k);
  if (rc != MCL_OK) return rc;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  double* rowsum = static_cast<double*>(work);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(nb_smooth_kernel, dim3(ceil_div(rows, 4)), dim3(NB_THREADS), 0, st, knn_distances, (long long)rows, k,
                     log2((double)k), rho, sigma, rowsum);
  hipLaunchKernelGGL(nb_floor_kernel, dim3(S), dim3(NB_THREADS), 0, st, off, max_n, (long long)rows, k, rowsum, rho, sigma);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_knn_connectivities(const int32_t* knn_indices, const double* knn_distances, const double* rho, const double* sigma,
                           const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n, int32_t k,
                           double set_op_mix_ratio, int32_t phase, void* work, int64_t* indptr, int64_t* nnz,
                           const int64_t* nnz_offsets, int64_t nnz_total, int32_t* indices, double* data,
                           mcl_stream_t stream) {
  if (!knn_indices || !knn_distances || !rho || !sigma || !offsets || !work || !indptr || (phase != 0 && phase != 1) ||
      !(set_op_mix_ratio >= 0.0 && set_op_mix_ratio <= 1.0))
    return MCL_EINVAL;
  if (phase == 0 ? !nnz : (!nnz_offsets || !indices || !data || nnz_total < 0)) return MCL_EINVAL;
  const int rc = nb_limits(S, rows, min_n, max_n, k);
  if (rc != MCL_OK) return rc;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const nb_work w = nb_carve(work, rows, k);
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nb_union_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NB_MAX_N * 8 + 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nb_union_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NB_MAX_N * 8 + 16);
  }
  MCL_CLEAR_ERROR();
  const size_t lds = (size_t)max_n * 8 + 16;
  const dim3 per_row(max_n, S);
  if (phase == 0) {
    if (hipMemsetAsync(w.indeg, 0, (size_t)rows * 2 * sizeof(int), st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(nb_indegree_kernel, per_row, dim3(NB_THREADS), 0, st, knn_indices, off, max_n, (long long)rows, k,
                       w.indeg);
    hipLaunchKernelGGL(nb_scan_kernel, dim3(S), dim3(NB_THREADS), 0, st, off, max_n, (long long)rows, k, w.indeg, w.rev_ptr);
    hipLaunchKernelGGL(nb_reverse_kernel, per_row, dim3(NB_THREADS), 0, st, knn_indices, knn_distances, rho, sigma, off,
                       max_n, (long long)rows, k, w);
    MCL_CHECK_LAUNCH();
    hipLaunchKernelGGL(nb_union_kernel<false>, per_row, dim3(NB_THREADS), lds, st, knn_indices, knn_distances, rho, sigma,
                       off, max_n, (long long)rows, k, set_op_mix_ratio, w, (const long long*)nullptr,
                       (const long long*)nullptr, 0ll, (int*)nullptr, (double*)nullptr);
    hipLaunchKernelGGL(nb_indptr_kernel, dim3(S), dim3(NB_THREADS), 0, st, off, max_n, (long long)rows, k, w.cursor,
                       reinterpret_cast<long long*>(indptr), reinterpret_cast<long long*>(nnz));
  } else {
    hipLaunchKernelGGL(nb_union_kernel<true>, per_row, dim3(NB_THREADS), lds, st, knn_indices, knn_distances, rho, sigma,
                       off, max_n, (long long)rows, k, set_op_mix_ratio, w, reinterpret_cast<const long long*>(indptr),
                       reinterpret_cast<const long long*>(nnz_offsets), (long long)nnz_total, indices, data);
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // extern "C"
