// Spots as non-negative mixtures of cell-type signatures: b_i = argmin over b >= 0 of || x_i - S^T b ||_2 for every spot of an
// evaluation per call (what a scipy.optimize.nnls loop over the spots computes; DESIGN 6.21 states the arithmetic,
// tests/deconv_reference.py restates it in numpy).  S is (T, G), T <= 64 types over G <= 16384 genes; everything is fp64, no
// floating-point atomics, every sum runs in an order that depends on G and T alone, and no workgroup reads what another
// wrote: a spot's outputs are bit-identical alone, anywhere in a batch and in a row-permuted batch.
//
//   nn_gram_kernel      one workgroup: A = S S^T (the upper triangle summed over g ascending out of LDS chunks, mirrored),
//                       then the Cholesky factor of the full A in LDS.  status[0] = 1 + the first type whose pivot is not
//                       above T eps A_jj, status[1] = 1 + the first type with a non-finite signature entry (0: none).
//   nn_products_kernel  c = x S^T and q = x . x on v_mfma_f64_16x16x4_f64: one wave = 16 spots x every tile of 16 types, so
//                       x is read once; operands masked on load, G walked 16 columns a step in index order (slot lk of
//                       MFMA t4 holds column j0 + 4 lk + t4, the layout of harmony.hip's hm_dist_kernel).  q: every lane sums
//                       the squares of its own columns, the four lanes of a spot are added in lane order.
//   nn_solve_kernel     THE HOT KERNEL.  Lawson-Hanson's active-set method on the normal equations (A, c_i), one wave per
//                       spot.  A sits in LDS once per workgroup; every wave keeps the Cholesky factor of the passive block
//                       A_PP as a packed triangle in LDS (row p at p (p + 1) / 2) and the passive list beside it.  Lane j
//                       holds c_j, b_j, w_j and the position of type j in the list (index space); lane p holds the type at
//                       position p and 1 / L_pp (position space).  Triangular solves are column sweeps: the pivot element
//                       is broadcast by v_readlane, the lanes behind it subtract their multiple.  No barrier after the
//                       staging: waves take spots of a grid-strided list and finish after different numbers of steps.
//   nn_residual_kernel  one wave per spot: rnorm = || x - S^T b || from x itself (lanes stride the genes, the types with
//                       b != 0 ascending, one butterfly), r2 = 1 - rnorm^2 / q, proportions = b / sum b, dominant = argmax.
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NN_MAX_T = 64;
constexpr int NN_MAX_G = 16384;
constexpr long long NN_MAX_CELLS = (1ll << 31) - 1;   // rows T
constexpr int NN_LDS_BYTES = 155648;                  // dynamic LDS of nn_solve_kernel at the most (152 KiB of the 160)
constexpr int NN_MAX_WAVES = 16;
constexpr int NN_WGS_PER_CU = 8;                      // workgroups of the solve a launch aims at per CU
constexpr int NN_GRAM_THREADS = 1024;
constexpr int NN_GRAM_CHUNK = 32;
constexpr int NN_GRAM_OWN = 3;                        // pairs (i <= j) a thread owns: 2080 / 1024 rounded up

__host__ __device__ inline int nn_tri(int T) { return T * (T + 1) / 2; }
// doubles a wave owns in LDS: the packed triangle and the passive list (T ints)
__host__ __device__ inline int nn_wave_doubles(int T) { return nn_tri(T) + (T + 1) / 2; }
__host__ __device__ inline int nn_waves(int T) {
  const int w = (NN_LDS_BYTES - T * T * 8) / (nn_wave_doubles(T) * 8);
  return w > NN_MAX_WAVES ? NN_MAX_WAVES : w;
}

// lane ``src`` (wave-uniform) of v in every lane
__device__ __forceinline__ double nn_bcast(double v, int src) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

// ------------------------------------------------------------------------------------------------------------- gram
__global__ __launch_bounds__(NN_GRAM_THREADS) void nn_gram_kernel(const double* __restrict__ S, int T, int G,
                                                                  double* __restrict__ A, double* __restrict__ L,
                                                                  int* __restrict__ status) {
  __shared__ double s_s[NN_MAX_T][NN_GRAM_CHUNK + 1];
  __shared__ double a_s[NN_MAX_T * NN_MAX_T];
  __shared__ double diag_s[NN_MAX_T];
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  const int pairs = nn_tri(T);
  int pi[NN_GRAM_OWN], pj[NN_GRAM_OWN];
  double acc[NN_GRAM_OWN];
#pragma unroll
  for (int u = 0; u < NN_GRAM_OWN; ++u) {                      // pair e of the upper triangle, row by row
    int i = 0, rem = tid + u * NN_GRAM_THREADS;
    if (rem >= pairs) rem = 0;
    while (rem >= T - i) {
      rem -= T - i;
      ++i;
    }
    pi[u] = i;
    pj[u] = i + rem;
    acc[u] = 0.0;
  }
  if (tid == 0) bad_s = NN_MAX_T;
  __syncthreads();
  for (int g0 = 0; g0 < G; g0 += NN_GRAM_CHUNK) {
    for (int e = tid; e < T * NN_GRAM_CHUNK; e += NN_GRAM_THREADS) {
      const int t = e / NN_GRAM_CHUNK, gg = e % NN_GRAM_CHUNK;
      const double v = g0 + gg < G ? S[(long long)t * G + g0 + gg] : 0.0;
      if (!isfinite(v)) atomicMin(&bad_s, t);
      s_s[t][gg] = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NN_GRAM_OWN; ++u) {
      if (tid + u * NN_GRAM_THREADS >= pairs) continue;
      for (int gg = 0; gg < NN_GRAM_CHUNK; ++gg) acc[u] = fma(s_s[pi[u]][gg], s_s[pj[u]][gg], acc[u]);   // (the tail adds 0 0)
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < NN_GRAM_OWN; ++u) {
    if (tid + u * NN_GRAM_THREADS >= pairs) continue;
    a_s[pi[u] * T + pj[u]] = acc[u];
    a_s[pj[u] * T + pi[u]] = acc[u];
  }
  __syncthreads();
  for (int e = tid; e < T * T; e += NN_GRAM_THREADS) A[e] = a_s[e];
  if (tid < T) diag_s[tid] = a_s[tid * T + tid];
  const int bad = bad_s;
  if (tid == 0) status[1] = bad < NN_MAX_T ? bad + 1 : 0;
  int fail = 0;
  if (bad == NN_MAX_T) {
    __syncthreads();
    for (int k = 0; k < T; ++k) {                              // right-looking, in place in the lower triangle
      const double d = a_s[k * T + k];
      if (!(d > (double)T * DBL_EPSILON * diag_s[k])) {        // (uniform: every thread read the same word)
        fail = k + 1;
        break;
      }
      __syncthreads();
      const double root = sqrt(d);
      if (tid == 0) a_s[k * T + k] = root;
      for (int i = k + 1 + tid; i < T; i += NN_GRAM_THREADS) a_s[i * T + k] = a_s[i * T + k] / root;
      __syncthreads();
      const int rest = T - k - 1;
      for (int e = tid; e < rest * rest; e += NN_GRAM_THREADS) {
        const int i = k + 1 + e / rest, j = k + 1 + e % rest;
        if (j <= i) a_s[i * T + j] = fma(-a_s[i * T + k], a_s[j * T + k], a_s[i * T + j]);
      }
      __syncthreads();
    }
  }
  if (tid == 0) status[0] = fail;
  for (int e = tid; e < T * T; e += NN_GRAM_THREADS) L[e] = (e % T <= e / T) ? a_s[e] : 0.0;
}

// --------------------------------------------------------------------------------------------------------- products
template <typename X, int NKT>
__global__ __launch_bounds__(256) void nn_products_kernel(const X* __restrict__ x, long long ld, long long rows, int G,
                                                          const double* __restrict__ S, int T, double* __restrict__ c,
                                                          double* __restrict__ q, unsigned* __restrict__ status) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const long long i0 = ((long long)blockIdx.x * 4 + wv) * 16;
  if (i0 >= rows) return;
  const long long n = i0 + lm;
  const bool okn = n < rows;
  const X* xr = x + (okn ? n : rows - 1) * ld;
  const double* sr[NKT];
  f64x4 acc[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int k = t * 16 + lm;
    sr[t] = S + (long long)(k < T ? k : T - 1) * G;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  double qp = 0.0;
  bool bad = false;
  for (int j0 = 0; j0 < G; j0 += 16) {
    double a[4];
    int jc[4];
    bool ok[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int j = j0 + 4 * lk + t4;
      ok[t4] = j < G;
      jc[t4] = ok[t4] ? j : G - 1;
      const double v = ldd(xr + jc[t4]);
      a[t4] = (ok[t4] && okn) ? v : 0.0;
      bad |= !isfinite(a[t4]);
      qp = fma(a[t4], a[t4], qp);
    }
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {
        const double v = sr[t][jc[t4]];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t4], ok[t4] ? v : 0.0, acc[t], 0, 0, 0);
      }
  }
  const double q0 = __shfl(qp, lm, 64), q1 = __shfl(qp, lm + 16, 64), q2 = __shfl(qp, lm + 32, 64),
               q3 = __shfl(qp, lm + 48, 64);
  if (lk == 0 && okn) q[n] = ((q0 + q1) + q2) + q3;
  if (bad) atomicMax(status, 0xFFFFFFFFu - (unsigned)n);      // (a masked row holds zeros: never bad)
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const long long row = i0 + lk + 4 * qi;
      const int col = t * 16 + lm;
      if (row < rows && col < T) c[row * T + col] = acc[t][qi];
    }
}

// ------------------------------------------------------------------------------------------------------------ solve
// The state of one spot, spread over the wave.  Index space: lane j < T.  Position space: lane p < m.
struct nn_state {
  int m;          // passive indices (uniform)
  int pos;        // index space: the position of type ``lane`` in the passive list, -1 outside it
  int pidx;       // position space: the type at position ``lane``
  double rdiag;   // position space: 1 / L[lane][lane]
};

// Type j enters at position m: row m of the factor is the forward substitution L l = A[P, j], its pivot A_jj - l . l summed
// in position order.  False (nothing changed) where the pivot is not above T eps A_jj.
__device__ __forceinline__ bool nn_append(const double* a_s, double* tri, int* plist, int T, int lane, int j, nn_state& s) {
  const int m = s.m;
  double r = lane < m ? a_s[j * T + s.pidx] : 0.0;
  const double ajj = a_s[j * T + j];
  double d = ajj, lrow = 0.0;
  for (int k = 0; k < m; ++k) {
    const double lk = nn_bcast(r * s.rdiag, k);
    d = fma(-lk, lk, d);
    if (lane == k) lrow = lk;
    if (lane > k && lane < m) r = fma(-tri[lane * (lane + 1) / 2 + k], lk, r);
  }
  if (!(d > (double)T * DBL_EPSILON * ajj)) return false;
  const double root = sqrt(d);
  const int base = m * (m + 1) / 2;
  if (lane < m) tri[base + lane] = lrow;
  if (lane == m) {
    tri[base + m] = root;
    s.rdiag = 1.0 / root;
    s.pidx = j;
    plist[m] = j;
  }
  if (lane == j) s.pos = m;
  s.m = m + 1;
  wave_sync();
  return true;
}

// z with A_PP z = c_P, returned in index space (0 outside P)
__device__ __forceinline__ double nn_passive_solve(const double* tri, int lane, double cj, const nn_state& s) {
  const int m = s.m;
  double y = __shfl(cj, s.pidx, 64);
  if (lane >= m) y = 0.0;
  for (int k = 0; k < m; ++k) {
    const double yk = nn_bcast(y * s.rdiag, k);
    if (lane == k) y = yk;
    if (lane > k && lane < m) y = fma(-tri[lane * (lane + 1) / 2 + k], yk, y);
  }
  for (int k = m - 1; k >= 0; --k) {
    const double zk = nn_bcast(y * s.rdiag, k);
    if (lane == k) y = zk;
    if (lane < k) y = fma(-tri[k * (k + 1) / 2 + lane], zk, y);
  }
  const double z = __shfl(y, s.pos < 0 ? 0 : s.pos, 64);
  return s.pos < 0 ? 0.0 : z;
}

__global__ __launch_bounds__(NN_MAX_WAVES * 64) void nn_solve_kernel(const double* __restrict__ A,
                                                                     const double* __restrict__ c, long long rows, int T,
                                                                     int waves, double* __restrict__ coef,
                                                                     int* __restrict__ n_iter,
                                                                     unsigned char* __restrict__ converged) {
  extern __shared__ __align__(16) unsigned char nn_lds[];
  double* a_s = reinterpret_cast<double*>(nn_lds);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* tri = a_s + T * T + wv * nn_wave_doubles(T);
  int* plist = reinterpret_cast<int*>(tri + nn_tri(T));
  for (int e = threadIdx.x; e < T * T; e += blockDim.x) a_s[e] = A[e];
  __syncthreads();                                             // the only barrier: spots take different numbers of steps
  const bool live = lane < T;
  const int cap = 3 * T;
  for (long long row = (long long)blockIdx.x * waves + wv; row < rows; row += (long long)gridDim.x * waves) {
    const double cj = live ? c[row * T + lane] : 0.0;
    const double tol = 10.0 * (double)T * DBL_EPSILON * wave_max(fabs(cj));
    double b = 0.0, w = cj;
    nn_state s = {0, -1, 0, 0.0};
    int it = 0;
    bool conv = true;
    while (s.m < T) {
      const double cand = (live && s.pos < 0) ? w : -INFINITY;
      const double mx = wave_max(cand);
      if (!(mx > tol)) break;
      const int j = __ffsll((unsigned long long)__ballot(cand == mx)) - 1;   // ties: the smaller index
      if (!nn_append(a_s, tri, plist, T, lane, j, s)) {
        conv = false;
        break;
      }
      bool first = true, rejected = false;
      for (;;) {
        if (it >= cap) {
          conv = false;
          break;
        }
        ++it;
        const double z = nn_passive_solve(tri, lane, cj, s);
        if (first && !(nn_bcast(z, j) > 0.0)) {                // Lawson and Hanson: the entering index steps back out
          s.m -= 1;
          if (lane == j) {
            s.pos = -1;
            w = 0.0;
          }
          rejected = true;
          break;
        }
        first = false;
        const bool in_p = s.pos >= 0;
        if (wave_min(in_p ? z : INFINITY) > 0.0) {
          b = in_p ? z : 0.0;
          break;
        }
        const double ratio = (in_p && z <= 0.0) ? b / (b - z) : INFINITY;
        const double alpha = wave_min(ratio);
        if (!(alpha <= 1.0)) {                                 // (a NaN solution: A is not what the gram call passed)
          conv = false;
          break;
        }
        b = in_p ? fma(alpha, z - b, b) : 0.0;
        const bool leave = in_p && (b <= 0.0 || ratio == alpha);   // the index that set alpha sits on the boundary: exactly 0
        if (leave) b = 0.0;
        // position space: which positions go, where the others land
        const int lp = __shfl((int)leave, s.pidx, 64);
        const bool had = lane < s.m;
        const unsigned long long keep = __ballot(had && !lp), gone = __ballot(had && lp);
        const int first_gone = __ffsll(gone) - 1;
        const int landing = (int)lanes_below(keep);
        if (had && !lp) plist[landing] = s.pidx;
        const int np = __shfl(landing, s.pos < 0 ? 0 : s.pos, 64);
        if (in_p) s.pos = leave ? -1 : np;
        const int m2 = __popcll(keep);
        wave_sync();
        if (lane < m2) s.pidx = plist[lane];
        wave_sync();
        s.m = first_gone;                                      // rows ahead of the first removed position stand
        bool okf = true;
        for (int p = first_gone; p < m2 && okf; ++p)
          okf = nn_append(a_s, tri, plist, T, lane, __builtin_amdgcn_readlane(s.pidx, p), s);
        if (!okf) {
          conv = false;
          break;
        }
        if (s.m == 0) break;
      }
      if (!conv) break;
      if (rejected) continue;
      double acc = cj;                                         // w = c - A b over the types with b != 0, ascending
      unsigned long long nz = __ballot(b != 0.0);
      while (nz) {
        const int i = __ffsll(nz) - 1;
        nz &= nz - 1;
        const double bi = nn_bcast(b, i);
        if (live) acc = fma(-a_s[i * T + lane], bi, acc);
      }
      w = acc;
    }
    if (live) coef[row * T + lane] = b;
    if (lane == 0) {
      n_iter[row] = it;
      converged[row] = conv ? 1 : 0;
    }
  }
}

// --------------------------------------------------------------------------------------------------------- residual
template <typename X>
__global__ __launch_bounds__(256) void nn_residual_kernel(const X* __restrict__ x, long long ld, long long rows, int G,
                                                          const double* __restrict__ S, int T,
                                                          const double* __restrict__ coef, const double* __restrict__ q,
                                                          double* __restrict__ rnorm, double* __restrict__ r2,
                                                          double* __restrict__ prop, int* __restrict__ dominant) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bool live = lane < T;
  const double b = live ? coef[row * T + lane] : 0.0;
  const unsigned long long nz = __ballot(b != 0.0);
  const X* xr = x + row * ld;
  double ss = 0.0;
  for (int g = lane; g < G; g += 64) {
    double pred = 0.0;
    for (unsigned long long mk = nz; mk; mk &= mk - 1) {
      const int t = __ffsll(mk) - 1;
      pred = fma(S[(long long)t * G + g], nn_bcast(b, t), pred);
    }
    const double r = ldd(xr + g) - pred;
    ss = fma(r, r, ss);
  }
  ss = wave_sum(ss);
  double tot = 0.0;
  for (unsigned long long mk = nz; mk; mk &= mk - 1) tot += nn_bcast(b, __ffsll(mk) - 1);
  const double p = tot > 0.0 ? b / tot : 0.0;
  const double top = wave_max(live ? p : 0.0);
  const int dom = tot > 0.0 ? __ffsll((unsigned long long)__ballot(live && p == top)) - 1 : -1;
  if (live) prop[row * T + lane] = p;
  if (lane == 0) {
    const double qq = q[row];
    rnorm[row] = sqrt(ss);
    r2[row] = qq == 0.0 ? NAN : 1.0 - ss / qq;
    dominant[row] = dom;
  }
}

inline bool nn_shape_ok(int64_t rows, int32_t G, int32_t T) { return rows >= 1 && G >= 1 && T >= 1; }
inline bool nn_limits_ok(int64_t rows, int32_t G, int32_t T) {
  return T <= NN_MAX_T && G >= T && G <= NN_MAX_G && (long long)rows * T <= NN_MAX_CELLS;
}

}  // namespace

extern "C" int32_t mcl_nnls_solve_waves(int32_t T) { return (T < 1 || T > NN_MAX_T) ? -1 : nn_waves(T); }

extern "C" int mcl_nnls_gram(const double* S, int32_t T, int32_t G, double* A, double* L, int32_t* status,
                             mcl_stream_t stream) {
  if (!S || !A || !L || !status || !nn_shape_ok(1, G, T)) return MCL_EINVAL;
  if (!nn_limits_ok(1, G, T)) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(nn_gram_kernel, dim3(1), dim3(NN_GRAM_THREADS), 0, mcl_stream(stream), S, T, G, A, L, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

template <typename X>
static int nn_launch_products(const X* x, int64_t ld, int64_t rows, int32_t G, const double* S, int32_t T, double* c,
                              double* q, unsigned* status, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(rows, 64)), block(256);
  const long long r = rows;
  switch ((T + 15) / 16) {
    case 1: hipLaunchKernelGGL((nn_products_kernel<X, 1>), grid, block, 0, st, x, (long long)ld, r, G, S, T, c, q, status); break;
    case 2: hipLaunchKernelGGL((nn_products_kernel<X, 2>), grid, block, 0, st, x, (long long)ld, r, G, S, T, c, q, status); break;
    case 3: hipLaunchKernelGGL((nn_products_kernel<X, 3>), grid, block, 0, st, x, (long long)ld, r, G, S, T, c, q, status); break;
    default: hipLaunchKernelGGL((nn_products_kernel<X, 4>), grid, block, 0, st, x, (long long)ld, r, G, S, T, c, q, status); break;
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_nnls_products(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, const double* S,
                                 int32_t T, double* c, double* q, int32_t* status, mcl_stream_t stream) {
  if (!x || !S || !c || !q || !status || !nn_shape_ok(rows, G, T) || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (!nn_limits_ok(rows, G, T)) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(status, 0, 4, st) != hipSuccess) return (int)hipGetLastError();
  unsigned* word = reinterpret_cast<unsigned*>(status);
  return dtype == 0 ? nn_launch_products(static_cast<const float*>(x), ld, rows, G, S, T, c, q, word, st)
                    : nn_launch_products(static_cast<const double*>(x), ld, rows, G, S, T, c, q, word, st);
}

extern "C" int mcl_nnls_solve(const double* A, const double* c, int64_t rows, int32_t T, double* coef, int32_t* n_iter,
                              void* converged, mcl_stream_t stream) {
  if (!A || !c || !coef || !n_iter || !converged || !nn_shape_ok(rows, T, T)) return MCL_EINVAL;
  if (!nn_limits_ok(rows, T, T)) return MCL_EUNSUPPORTED;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nn_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              NN_LDS_BYTES);
  }
  const int waves = nn_waves(T);
  const size_t lds = ((size_t)T * T + (size_t)waves * nn_wave_doubles(T)) * 8;
  long long blocks = (rows + waves - 1) / waves;
  const long long most = (long long)mcl_cu_count() * NN_WGS_PER_CU;
  if (blocks > most) blocks = most;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(nn_solve_kernel, dim3((unsigned)blocks), dim3(waves * 64), lds, mcl_stream(stream), A, c,
                     (long long)rows, T, waves, coef, n_iter, static_cast<unsigned char*>(converged));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_nnls_residual(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, const double* S,
                                 int32_t T, const double* coef, const double* q, double* rnorm, double* r2,
                                 double* proportions, int32_t* dominant, mcl_stream_t stream) {
  if (!x || !S || !coef || !q || !rnorm || !r2 || !proportions || !dominant || !nn_shape_ok(rows, G, T) || ld < G ||
      (dtype != 0 && dtype != 1))
    return MCL_EINVAL;
  if (!nn_limits_ok(rows, G, T)) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
  MCL_CLEAR_ERROR();
  if (dtype == 0)
    hipLaunchKernelGGL(nn_residual_kernel<float>, grid, block, 0, st, static_cast<const float*>(x), (long long)ld,
                       (long long)rows, G, S, T, coef, q, rnorm, r2, proportions, dominant);
  else
    hipLaunchKernelGGL(nn_residual_kernel<double>, grid, block, 0, st, static_cast<const double*>(x), (long long)ld,
                       (long long)rows, G, S, T, coef, q, rnorm, r2, proportions, dominant);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
