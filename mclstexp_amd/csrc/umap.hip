// The UMAP layout of the spot neighbourhood graph (scanpy's sc.tl.umap on the connectivities of csrc/neighbors.hip) for every
// segment (slide) of a batch; the arithmetic is the one DESIGN 6.12 states: one Jacobi step per epoch -- every gradient of
// epoch n is taken at the positions at the start of epoch n -- and negative samples that are a pure function of (seed,
// epoch, vertex, entry rank, sample number).  Everything is fp64, there are no floating-point atomics (integer atomics count
// the samples), no workgroup waits on another, and no result depends on the order in which workgroups or lanes arrive: a
// segment inside a batch is bit-identical to the same segment alone, and a run to its repeat.
//
//   mcl_umap_prepare   um_wmax_kernel: one workgroup per segment, the largest valid weight.  um_schedule_kernel: one thread
//                      per stored entry: live, eps, epn and the two running values next, nneg; each a single IEEE operation.
//   mcl_umap_init      um_init_pca_kernel: one workgroup per segment, the largest |x| of the first two columns, then the
//                      scaled copy.  um_init_random_kernel: one thread per vertex.
//   mcl_umap_epochs    um_epoch_kernel, one launch per epoch, back to back: one wave per vertex, lanes stride the row's
//                      entries; a lane adds its entries' contributions in entry order (the attraction, then that entry's
//                      samples in sample order), the 64 partials are summed by an xor butterfly (offsets 32, 16, .. 1: one
//                      fixed tree, the same bits in every lane), and y + alpha * sum goes to the OTHER position buffer.  The
//                      lane that owns an entry advances its next / nneg in place.  A segment whose epochs are over copies
//                      its positions across, so both buffers hold its last ones.
//
// Segments ride on grid.y; a segment the launch was not sized for is skipped; a column outside its segment is ignored.
#include <float.h>
#include "common.h"

namespace {

constexpr int UM_MAX_N = 16384;
constexpr int UM_MAX_S = 65535;                 // grid.y
constexpr int UM_MAX_EPOCHS = 5000;
constexpr int UM_MAX_RATE = 64;
constexpr int UM_MAX_DRAWS = 4096;              // never met on a valid schedule (at most 2 R draws per activation)
constexpr int UM_THREADS = 256;
constexpr int UM_WAVES = UM_THREADS / 64;

struct um_work {
  double* eps;        // nnz: epochs per attraction of the entry, wmax / w
  double* epn;        // nnz: epochs per negative sample, eps / R
  double* next;       // nnz: the epoch of the entry's next attraction
  double* nneg;       // nnz: the epoch of its next negative sample
  double* wmax;       // S
  unsigned char* live;  // nnz
};
__host__ __device__ inline um_work um_carve(void* work, long long nnz, int S) {
  um_work w;
  w.eps = static_cast<double*>(work);
  w.epn = w.eps + nnz;
  w.next = w.epn + nnz;
  w.nneg = w.next + nnz;
  w.wmax = w.nneg + nnz;
  w.live = reinterpret_cast<unsigned char*>(w.wmax + S);
  return w;
}

// ---- the schedule: every value one IEEE fp64 operation, no contraction (the restatement's bits)
__device__ __forceinline__ void um_schedule(double w, double wmax, int n_epochs, int rate, bool* live, double* eps,
                                            double* epn) {
#pragma clang fp contract(off)
  const double thr = wmax / (double)n_epochs;
  *live = w >= thr;
  *eps = wmax / w;
  *epn = *eps / (double)rate;
}
__device__ __forceinline__ int um_draws(double nf, double nneg, double epn) {
#pragma clang fp contract(off)
  const double gap = nf - nneg;
  const double t = gap / epn;
  if (!(t >= 1.0)) return 0;
  return t < (double)UM_MAX_DRAWS ? (int)t : UM_MAX_DRAWS;
}
__device__ __forceinline__ double um_advance(double v, int q, double step) {
#pragma clang fp contract(off)
  const double prod = (double)q * step;
  return v + prod;
}
__device__ __forceinline__ double um_alpha(double alpha, int epoch, int n_epochs) {
#pragma clang fp contract(off)
  const double frac = (double)epoch / (double)n_epochs;
  const double left = 1.0 - frac;
  return alpha * left;
}
__device__ __forceinline__ double um_step(double y, double alpha, double sum) {
#pragma clang fp contract(off)
  const double move = alpha * sum;
  return y + move;
}

__device__ __forceinline__ double um_clip(double v) { return fmin(fmax(v, -4.0), 4.0); }

// ----------------------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(UM_THREADS) void um_wmax_kernel(const double* __restrict__ data,
                                                             const long long* __restrict__ nnz_off, long long nnz_total,
                                                             um_work w, long long* __restrict__ counters) {
  __shared__ double red[UM_WAVES];
  const int s = blockIdx.x;
  long long base, count;
  double m = 0.0;
  if (segment_entries(nnz_off, s, nnz_total, &base, &count))
    for (long long e = threadIdx.x; e < count; e += UM_THREADS) {
      const double v = data[base + e];
      if (valid_weight(v)) m = fmax(m, v);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));   // wave_max(m) written out: a call changes this kernel's code
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    w.wmax[s] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    counters[2 * s] = 0;
    counters[2 * s + 1] = 0;
  }
}

__global__ __launch_bounds__(UM_THREADS) void um_schedule_kernel(const double* __restrict__ data,
                                                                 const long long* __restrict__ nnz_off, long long nnz_total,
                                                                 const int* __restrict__ n_epochs, int rate, um_work w) {
  const int s = blockIdx.y;
  long long base, count;
  if (!segment_entries(nnz_off, s, nnz_total, &base, &count)) return;
  const int n_ep = n_epochs[s];
  const bool runs = n_ep >= 1 && n_ep <= UM_MAX_EPOCHS;
  const double wmax = w.wmax[s];
  for (long long e = (long long)blockIdx.x * UM_THREADS + threadIdx.x; e < count; e += (long long)gridDim.x * UM_THREADS) {
    const double v = data[base + e];
    bool live = false;
    double eps = 0.0, epn = 0.0;
    if (runs && valid_weight(v)) um_schedule(v, wmax, n_ep, rate, &live, &eps, &epn);
    w.live[base + e] = live ? 1 : 0;
    w.eps[base + e] = eps;
    w.epn[base + e] = epn;
    w.next[base + e] = eps;
    w.nneg[base + e] = epn;
  }
}

// -------------------------------------------------------------------------------------------------------------- init
// y = x[:, :2] * (10 / max |x[:, :2]|) per segment; all zeros stay zeros
template <typename T>
__global__ __launch_bounds__(UM_THREADS) void um_init_pca_kernel(const T* __restrict__ x, long long ld,
                                                                 const long long* __restrict__ off, int max_n,
                                                                 long long rows, double* __restrict__ Y) {
#pragma clang fp contract(off)
  __shared__ double red[UM_WAVES];
  long long o;
  int n;
  if (!segment_span(off, blockIdx.x, 2, max_n, rows, &o, &n)) return;
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += UM_THREADS) {
    const T* r = x + (o + i) * ld;
    m = fmax(m, fmax(fabs((double)r[0]), fabs((double)r[1])));
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) m = fmax(m, __shfl_xor(m, sh, 64));   // wave_max(m) written out, as in um_wmax_kernel
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double scale = m > 0.0 ? 10.0 / m : 1.0;
  for (int i = threadIdx.x; i < n; i += UM_THREADS) {
    const T* r = x + (o + i) * ld;
    Y[2 * (o + i)] = (double)r[0] * scale;
    Y[2 * (o + i) + 1] = (double)r[1] * scale;
  }
}

// y_ic = 20 ((h >> 11) 2^-53) - 10, h = mix(mix(seed0 ^ i) ^ c), seed0 = mix(seed ^ ~0)
__global__ __launch_bounds__(UM_THREADS) void um_init_random_kernel(const long long* __restrict__ off, int max_n,
                                                                    long long rows, u64 seed0, double* __restrict__ Y) {
#pragma clang fp contract(off)
  long long o;
  int n;
  if (!segment_span(off, blockIdx.y, 2, max_n, rows, &o, &n)) return;
  const int i = blockIdx.x * UM_THREADS + threadIdx.x;
  if (i >= n) return;
  const u64 hi = mix64(seed0 ^ (u64)i);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const u64 h = mix64(hi ^ (u64)c);
    const double u = (double)(h >> 11) * 0x1p-53;
    const double t = 20.0 * u;
    Y[2 * (o + i) + c] = t - 10.0;
  }
}

// ------------------------------------------------------------------------------------------------------------- epoch
struct um_args {
  const long long* indptr;
  const int* indices;
  const long long* off;
  const long long* nnz_off;
  const int* n_epochs;
  long long* counters;
  um_work w;
  long long rows, nnz_total;
  double a, b, gamma, alpha;
  u64 seed0;          // mix(seed)
  int max_n, rate;
};

__global__ __launch_bounds__(UM_THREADS) void um_epoch_kernel(um_args A, int epoch, const double2* __restrict__ Ysrc,
                                                              double2* __restrict__ Ydst) {
  const int s = blockIdx.y;
  long long o;
  int n;
  if (!segment_span(A.off, s, 2, A.max_n, A.rows, &o, &n)) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * UM_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;                                   // a whole wave
  const double2 yi = Ysrc[o + i];
  const int n_ep = A.n_epochs[s];
  long long base = 0, cap = 0, lo = 0, hi = 0;
  bool ok = n_ep >= 1 && n_ep <= UM_MAX_EPOCHS && epoch < n_ep && segment_entries(A.nnz_off, s, A.nnz_total, &base, &cap);
  if (ok) {
    lo = A.indptr[o + s + i];
    hi = A.indptr[o + s + i + 1];
    ok = lo >= 0 && lo <= hi && hi <= cap;
  }
  if (!ok) {                                            // the segment is over (or its row is not one): keep the position
    if (lane == 0) Ydst[o + i] = yi;
    return;
  }
  const u64 hrow = mix64(mix64(A.seed0 ^ (u64)epoch) ^ (u64)i);
  const double nf = (double)epoch;
  const double a = A.a, b = A.b;
  const double att = -2.0 * a * b, rep = 2.0 * A.gamma * b;
  double s0 = 0.0, s1 = 0.0;
  int taken = 0, drawn = 0;
  for (long long r = lo + lane; r < hi; r += 64) {
    const long long e = base + r;
    if (!A.w.live[e]) continue;
    const double nx = A.w.next[e];
    if (!(nx <= nf)) continue;
    const int j = A.indices[e];
    if (j < 0 || j >= n) continue;
    const double2 yj = Ysrc[o + j];
    {
      const double d0 = yi.x - yj.x, d1 = yi.y - yj.y;
      const double d2 = d0 * d0 + d1 * d1;
      if (d2 > 0.0) {
        const double pw = exp(b * log(d2));
        const double c = att * (pw / d2) / (a * pw + 1.0);
        s0 += 2.0 * um_clip(c * d0);
        s1 += 2.0 * um_clip(c * d1);
      }
    }
    int q = 0;
    double epn = 0.0, nneg = 0.0;
    if (A.rate > 0) {
      epn = A.w.epn[e];
      nneg = A.w.nneg[e];
      q = um_draws(nf, nneg, epn);
    }
    const u64 hent = mix64(hrow ^ (u64)(r - lo));         // the entry's rank in its row
    for (int p = 0; p < q; ++p) {
      const u64 h = mix64(hent ^ (u64)p);
      const int k = (int)(((h >> 32) * (u64)n) >> 32);   // < n
      const double2 yk = Ysrc[o + k];
      const double d0 = yi.x - yk.x, d1 = yi.y - yk.y;
      const double d2 = d0 * d0 + d1 * d1;
      if (d2 > 0.0) {
        const double pw = exp(b * log(d2));
        const double c = rep / ((0.001 + d2) * (a * pw + 1.0));
        s0 += um_clip(c * d0);
        s1 += um_clip(c * d1);
      }
    }
    A.w.next[e] = um_advance(nx, 1, A.w.eps[e]);
    if (A.rate > 0) A.w.nneg[e] = um_advance(nneg, q, epn);
    taken += 1;
    drawn += q;
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  taken = wave_sum(taken);
  drawn = wave_sum(drawn);
  if (lane == 0) {
    const double alpha = um_alpha(A.alpha, epoch, n_ep);
    double2 y;
    y.x = um_step(yi.x, alpha, s0);
    y.y = um_step(yi.y, alpha, s1);
    Ydst[o + i] = y;
    if (taken) atomicAdd(reinterpret_cast<u64*>(A.counters + 2 * s), (u64)taken);
    if (drawn) atomicAdd(reinterpret_cast<u64*>(A.counters + 2 * s + 1), (u64)drawn);
  }
}

int um_limits(int S, long long rows, int min_n, int max_n) {
  if (S <= 0 || rows <= 0) return MCL_EINVAL;
  if (S > UM_MAX_S || max_n > UM_MAX_N || min_n < 2) return MCL_EUNSUPPORTED;
  if (min_n > max_n || rows < (long long)S * min_n || rows > (long long)S * max_n) return MCL_EINVAL;
  return MCL_OK;
}

bool um_finite(double v) { return v == v && v <= DBL_MAX && v >= -DBL_MAX; }

}  // namespace

extern "C" {

int64_t mcl_umap_workspace_bytes(int64_t nnz_total, int32_t S) {
  if (nnz_total < 0 || S <= 0 || S > UM_MAX_S) return 0;
  return nnz_total * (4 * 8 + 1) + (int64_t)S * 8 + 16;
}

int mcl_umap_prepare(const double* data, const int64_t* nnz_offsets, const int32_t* n_epochs, int32_t S, int64_t nnz_total,
                     int64_t max_nnz, int32_t max_epochs, int32_t negative_sample_rate, void* work, int64_t* counters,
                     mcl_stream_t stream) {
  if (!data || !nnz_offsets || !n_epochs || !work || !counters || S <= 0 || nnz_total < 0 || max_nnz < 0 ||
      max_nnz > nnz_total)
    return MCL_EINVAL;
  if (S > UM_MAX_S || max_epochs < 1 || max_epochs > UM_MAX_EPOCHS || negative_sample_rate < 0 ||
      negative_sample_rate > UM_MAX_RATE)
    return MCL_EUNSUPPORTED;
  hipStream_t st = mcl_stream(stream);
  const long long* noff = reinterpret_cast<const long long*>(nnz_offsets);
  const um_work w = um_carve(work, nnz_total, S);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(um_wmax_kernel, dim3(S), dim3(UM_THREADS), 0, st, data, noff, (long long)nnz_total, w,
                     reinterpret_cast<long long*>(counters));
  const int blocks = max_nnz > 0 ? (ceil_div(max_nnz, UM_THREADS) < 4096 ? ceil_div(max_nnz, UM_THREADS) : 4096) : 1;
  hipLaunchKernelGGL(um_schedule_kernel, dim3(blocks, S), dim3(UM_THREADS), 0, st, data, noff, (long long)nnz_total,
                     n_epochs, negative_sample_rate, w);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_umap_init(int32_t mode, const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets, int32_t S,
                  int32_t rows, int32_t min_n, int32_t max_n, uint64_t seed, double* Y, mcl_stream_t stream) {
  if (!offsets || !Y || (mode != 0 && mode != 1)) return MCL_EINVAL;
  if (mode == 0 && (!x || D < 2 || ld < D || (dtype != 0 && dtype != 1))) return MCL_EINVAL;
  const int rc = um_limits(S, rows, min_n, max_n);
  if (rc != MCL_OK) return rc;
  hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  if (mode == 1)
    hipLaunchKernelGGL(um_init_random_kernel, dim3(ceil_div(max_n, UM_THREADS), S), dim3(UM_THREADS), 0, st, off, max_n,
                       (long long)rows, mix64((u64)seed ^ ~0ull), Y);
  else if (dtype == 0)
    hipLaunchKernelGGL(um_init_pca_kernel<float>, dim3(S), dim3(UM_THREADS), 0, st, (const float*)x, (long long)ld, off,
                       max_n, (long long)rows, Y);
  else
    hipLaunchKernelGGL(um_init_pca_kernel<double>, dim3(S), dim3(UM_THREADS), 0, st, (const double*)x, (long long)ld, off,
                       max_n, (long long)rows, Y);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_umap_epochs(int32_t first, int32_t count, const int64_t* indptr, const int32_t* indices, const int64_t* offsets,
                    const int64_t* nnz_offsets, const int32_t* n_epochs, int32_t S, int32_t rows, int32_t min_n,
                    int32_t max_n, int64_t nnz_total, int32_t max_epochs, double a, double b, double gamma, double alpha,
                    int32_t negative_sample_rate, uint64_t seed, void* work, double* Y0, double* Y1, int64_t* counters,
                    mcl_stream_t stream) {
  if (!indptr || !indices || !offsets || !nnz_offsets || !n_epochs || !work || !Y0 || !Y1 || Y0 == Y1 || !counters ||
      nnz_total < 0 || first < 0 || count < 0)
    return MCL_EINVAL;
  if (max_epochs < 1 || max_epochs > UM_MAX_EPOCHS || negative_sample_rate < 0 || negative_sample_rate > UM_MAX_RATE ||
      !um_finite(a) || !um_finite(b) || !um_finite(gamma) || !um_finite(alpha) || !(a > 0.0) || !(b > 0.0))
    return MCL_EUNSUPPORTED;
  const int rc = um_limits(S, rows, min_n, max_n);
  if (rc != MCL_OK) return rc;
  if ((long long)first + count > max_epochs) return MCL_EINVAL;
  hipStream_t st = mcl_stream(stream);
  um_args A;
  A.indptr = reinterpret_cast<const long long*>(indptr);
  A.indices = indices;
  A.off = reinterpret_cast<const long long*>(offsets);
  A.nnz_off = reinterpret_cast<const long long*>(nnz_offsets);
  A.n_epochs = n_epochs;
  A.counters = reinterpret_cast<long long*>(counters);
  A.w = um_carve(work, nnz_total, S);
  A.rows = rows;
  A.nnz_total = nnz_total;
  A.a = a;
  A.b = b;
  A.gamma = gamma;
  A.alpha = alpha;
  A.seed0 = mix64((u64)seed);
  A.max_n = max_n;
  A.rate = negative_sample_rate;
  MCL_CLEAR_ERROR();
  const dim3 grid(ceil_div(max_n, UM_WAVES), S);
  for (int n = first; n < first + count; ++n) {         // epoch n reads the buffer of its parity and writes the other
    const double2* src = reinterpret_cast<const double2*>(n & 1 ? Y1 : Y0);
    double2* dst = reinterpret_cast<double2*>(n & 1 ? Y0 : Y1);
    hipLaunchKernelGGL(um_epoch_kernel, grid, dim3(UM_THREADS), 0, st, A, n, src, dst);
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // extern "C"
