// The k <= 64 leading eigenpairs of S symmetric fp64 matrices (m_s <= 4096) per call: the direct, dsyevx-shaped method of
// DESIGN 6.14, restated line by line in tests/eig_reference.py.  Everything is fp64, there is no floating-point atomic and
// no workgroup waits for another: every dependency is a launch boundary.  Every sum runs in an order that depends only on
// the slide's own m and k, so a slide inside a batch is bit-identical to the same slide alone; a slide with fewer steps
// than the batch's largest has nothing to do in the trailing launches and leaves at once.
//
//   mcl_sym_eig_top     eig_setup_kernel            prefix sums of m, validation of every m_s (an invalid call certifies NaN)
//     stage 1 (a)       per column j = 0 .. m - 2, three launches:
//                         eig_house_kernel   (S)            the dlarfg reflector of column j (read as row j: A is exactly
//                                                           symmetric), v into row and column j, d_j, e_j, tau_j
//                         eig_symv_kernel    (n / 8, S)     p = tau S v, S = the trailing n x n block, n = m - j - 1:
//                                                           one streaming read of the block (8 n^2 bytes)
//                         eig_rank2_kernel   (n / 8, S)     w = p - (tau / 2)(p^T v) v (the dot recomputed by every
//                                                           workgroup in one fixed order), S_ab -= v_a w_b + w_a v_b: one
//                                                           read and one write of the block (16 n^2 bytes)
//     stage 2 (b)       eig_bisect_kernel  (S)      |T|, pivmin, the k largest eigenvalues by bisection on the Sturm count,
//                                                   one lane each; their perturbed copies and Gram-Schmidt groups
//             (c)       eig_factor_kernel  (S)      dgttrf of T - lambda_i I, one lane each; the hashed start vectors
//                       3 x eig_solve_kernel (S) + eig_ortho_kernel (S): dgtts2, then group-wise MGS (twice) and norm
//             (d)       eig_cert_kernel    (k, S) + eig_cert_reduce_kernel (S): residual / |T| and max |Z^T Z - I|
//     stage 4 (e, f)    eig_back_kernel    (k, S)   z <- H_0 .. H_{m-3} z with the column in LDS, then the sign rule
#include <float.h>

#include "common.h"

namespace {

constexpr int EG_THREADS = 256;
constexpr int EG_MAX_M = 4096;
constexpr int EG_MAX_K = 64;
constexpr int EG_WROWS = 2;          // rows of the trailing block per wave
constexpr int EG_ROWS = 4 * EG_WROWS;   // ... per workgroup.  A single slide of order 3467 then fills the chip with 1733 waves
                                     // (6.8 per CU), each with 8 matrix loads of 512 bytes in flight: 28 KB per CU
constexpr int EG_BISECT = 128;       // halvings at most
constexpr int EG_ITERS = 3;          // inverse iterations
constexpr double EG_EPS = 0x1p-52;
constexpr double EG_PERT = 10.0;     // dstein: eigenvalues closer than 10 eps |T| are pushed apart
constexpr double EG_ORTOL = 1e-3;    // dstein: consecutive eigenvalues within 1e-3 |T| share a group

// the workspace, carved on the host; per-slide vectors sit at moff[s] (doubles), per-slide (m, k) panels at moff[s] * k
struct EigWork {
  long long* moff;       // S + 1
  int* mv;               // S: m_s, or 0 for every slide of a call whose sizes are invalid
  double* scal;          // S x 2: |T|, pivmin
  double* lamp;          // S x k: the shifts of the solves
  int* gst;              // S x k: first column of the Gram-Schmidt group
  double* certp;         // S x k x 2
  double *d, *e, *tau, *p, *v;      // sum_m each
  double *z, *dl, *dd, *du, *du2;   // sum_m * k each, element (r, i) at r * k + i
  unsigned char* sw;     // sum_m * k: row interchanged in dgttrf
};

__host__ long long eig_work_doubles(long long S, long long sum_m, long long k) {
  return (S + 1) + (S + 1) / 2 + 2 * S + S * k + (S * k + 1) / 2 + 2 * S * k + 5 * sum_m + 5 * sum_m * k +
         (sum_m * k + 7) / 8;
}

__host__ EigWork eig_carve(void* work, long long S, long long sum_m, long long k) {
  EigWork w;
  double* q = static_cast<double*>(work);
  w.moff = reinterpret_cast<long long*>(q), q += S + 1;
  w.mv = reinterpret_cast<int*>(q), q += (S + 1) / 2;
  w.scal = q, q += 2 * S;
  w.lamp = q, q += S * k;
  w.gst = reinterpret_cast<int*>(q), q += (S * k + 1) / 2;
  w.certp = q, q += 2 * S * k;
  w.d = q, q += sum_m;
  w.e = q, q += sum_m;
  w.tau = q, q += sum_m;
  w.p = q, q += sum_m;
  w.v = q, q += sum_m;
  w.z = q, q += sum_m * k;
  w.dl = q, q += sum_m * k;
  w.dd = q, q += sum_m * k;
  w.du = q, q += sum_m * k;
  w.du2 = q, q += sum_m * k;
  w.sw = reinterpret_cast<unsigned char*>(q);
  return w;
}

// start value of element (row, column) in [-1, 1): independent of the slide
__device__ __forceinline__ double eg_start(int r, int c) {
  const u64 h = mix64(((u64)(unsigned)r << 32) | (u64)(unsigned)c);
  return (double)(h >> 11) * 0x1p-52 - 1.0;
}

// ------------------------------------------------------------------------------------------------------------- setup
__global__ __launch_bounds__(EG_THREADS) void eig_setup_kernel(const int* __restrict__ m, int S, int max_m, int k,
                                                               long long sum_m, long long* __restrict__ moff,
                                                               int* __restrict__ mv) {
  __shared__ long long part[EG_THREADS];
  __shared__ int bad_any;
  const int tid = threadIdx.x;
  const int chunk = (S + EG_THREADS - 1) / EG_THREADS;
  const int b = min(tid * chunk, S), e = min(b + chunk, S);
  if (tid == 0) bad_any = 0;
  __syncthreads();
  long long sum = 0;
  int bad = 0;
  for (int s = b; s < e; ++s) {
    const int ms = m[s];
    bad |= (ms < 1 || ms > max_m || k > ms);
    sum += bad ? 0 : ms;
  }
  part[tid] = sum;
  if (bad) atomicOr(&bad_any, 1);
  __syncthreads();
  long long run = 0, total = 0;
  for (int t = 0; t < EG_THREADS; ++t) {
    if (t == tid) run = total;
    total += part[t];
  }
  const bool ok = !bad_any && total == sum_m;
  for (int s = b; s < e; ++s) {
    moff[s] = ok ? run : 0;
    mv[s] = ok ? m[s] : 0;
    run += ok ? m[s] : 0;
  }
  if (tid == 0) moff[S] = ok ? total : 0;
}

// --------------------------------------------------------------------------------------- (a) Householder tridiagonalisation
// column j's reflector (dlarfg): x = A[j+1:, j] read as the row A[j, j+1:], alpha = x_0, beta = -copysign(hypot(alpha,
// |x[1:]|), alpha), tau = (beta - alpha) / beta, v = x / (alpha - beta), v_0 = 1; |x[1:]| = 0: tau = 0, e_j = alpha.
__global__ __launch_bounds__(EG_THREADS) void eig_house_kernel(double* __restrict__ a, const long long* __restrict__ aoff,
                                                               int j, EigWork w) {
  __shared__ double slot[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1 || (j > ms - 2 && !(j == 0 && ms == 1))) return;
  double* A = a + aoff[s];
  const long long o = w.moff[s];
  if (ms == 1) {
    if (tid == 0) w.d[o] = A[0];
    return;
  }
  const int n = ms - j - 1;
  double* row = A + (long long)j * ms + j + 1;
  const double alpha = row[0];              // read by every thread before the barrier: thread 0 stores v_0 = 1 there
  double ss = 0.0;
  for (int i = 1 + tid; i < n; i += EG_THREADS) ss += row[i] * row[i];
  ss = block_sum4<false>(ss, slot);
  const double xnorm = sqrt(ss);
  if (tid == 0) {
    w.d[o + j] = A[(long long)j * ms + j];
    if (j == ms - 2) w.d[o + ms - 1] = A[(long long)(ms - 1) * ms + ms - 1];
  }
  if (xnorm == 0.0) {
    if (tid == 0) {
      w.e[o + j] = alpha;
      w.tau[o + j] = 0.0;
    }
    return;
  }
  const double beta = -copysign(hypot(alpha, xnorm), alpha);
  const double scale = alpha - beta;
  for (int i = tid; i < n; i += EG_THREADS) {
    const double vi = i == 0 ? 1.0 : row[i] / scale;
    w.v[o + i] = vi;
    row[i] = vi;
    A[(long long)(j + 1 + i) * ms + j] = vi;
  }
  if (tid == 0) {
    w.e[o + j] = beta;
    w.tau[o + j] = (beta - alpha) / beta;
  }
}

// p = tau S v: a wave owns EG_WROWS rows of the trailing block, its lanes stride over the columns (512 contiguous bytes per
// load and row), four column steps at a time into four partial sums per row so that 4 EG_WROWS loads are in flight per
// lane; the partials close as (0 + 1) + (2 + 3), the row sums with the butterfly.
__global__ __launch_bounds__(EG_THREADS) void eig_symv_kernel(const double* __restrict__ a,
                                                              const long long* __restrict__ aoff, int j, EigWork w) {
  const int s = blockIdx.y;
  const int ms = w.mv[s];
  if (j > ms - 3) return;
  const long long o = w.moff[s];
  const double t = w.tau[o + j];
  if (t == 0.0) return;
  const int n = ms - j - 1;
  const int lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * EG_ROWS + (threadIdx.x >> 6) * EG_WROWS;
  if (r0 >= n) return;
  const double* base = a + aoff[s] + (long long)(j + 1) * ms + j + 1;
  const double* v = w.v + o;
  const double* row[EG_WROWS];
#pragma unroll
  for (int q = 0; q < EG_WROWS; ++q) row[q] = base + (long long)min(r0 + q, n - 1) * ms;
  double acc[EG_WROWS][4];
#pragma unroll
  for (int q = 0; q < EG_WROWS; ++q)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[q][u] = 0.0;
  int c = lane;
  for (; c + 192 < n; c += 256) {
    double vc[4], x[EG_WROWS][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      vc[u] = v[c + 64 * u];
#pragma unroll
      for (int q = 0; q < EG_WROWS; ++q) x[q][u] = row[q][c + 64 * u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < EG_WROWS; ++q) acc[q][u] = fma(x[q][u], vc[u], acc[q][u]);
  }
  for (int u = 0; c < n; c += 64, ++u) {      // the ragged end: at most three steps, partial u as in the full groups
    const double vc = v[c];
#pragma unroll
    for (int q = 0; q < EG_WROWS; ++q) {
      const double x = row[q][c];
      if (u == 0) acc[q][0] = fma(x, vc, acc[q][0]);
      else if (u == 1) acc[q][1] = fma(x, vc, acc[q][1]);
      else acc[q][2] = fma(x, vc, acc[q][2]);
    }
  }
#pragma unroll
  for (int q = 0; q < EG_WROWS; ++q) {
    const double sum = wave_sum((acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3]));
    if (lane == 0 && r0 + q < n) w.p[o + r0 + q] = t * sum;
  }
}

// w = p - (tau / 2)(p^T v) v, S_ab -= v_a w_b + w_a v_b.  The two products are rounded separately and added, so element
// (a, b) and element (b, a) receive the same bits: the block stays exactly symmetric.
__global__ __launch_bounds__(EG_THREADS) void eig_rank2_kernel(double* __restrict__ a, const long long* __restrict__ aoff,
                                                               int j, EigWork w) {
#pragma clang fp contract(off)
  __shared__ double slot[4];
  const int s = blockIdx.y;
  const int ms = w.mv[s];
  if (j > ms - 3) return;
  const long long o = w.moff[s];
  const double t = w.tau[o + j];
  if (t == 0.0) return;
  const int n = ms - j - 1;
  if ((int)blockIdx.x * EG_ROWS >= n) return;
  const double* v = w.v + o;
  const double* p = w.p + o;
  double dot = 0.0;
  for (int c = threadIdx.x; c < n; c += EG_THREADS) dot += p[c] * v[c];
  dot = block_sum4<false>(dot, slot);
  const double half = 0.5 * t * dot;
  const int lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * EG_ROWS + (threadIdx.x >> 6) * EG_WROWS;
  if (r0 >= n) return;
  double* base = a + aoff[s] + (long long)(j + 1) * ms + j + 1;
  double* row[EG_WROWS];
  double va[EG_WROWS], wa[EG_WROWS];
#pragma unroll
  for (int q = 0; q < EG_WROWS; ++q) {
    const int r = min(r0 + q, n - 1);
    row[q] = base + (long long)r * ms;
    va[q] = v[r];
    wa[q] = p[r] - half * va[q];
  }
#pragma unroll 4
  for (int c = lane; c < n; c += 64) {
    const double vb = v[c];
    const double wb = p[c] - half * vb;
#pragma unroll
    for (int q = 0; q < EG_WROWS; ++q) {
      if (r0 + q < n) {
        const double t1 = va[q] * wb, t2 = wa[q] * vb;
        row[q][c] = row[q][c] - (t1 + t2);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ (b) eigenvalues of T
// Lane i bisects for the i-th largest eigenvalue on the dstebz Sturm count (q <- d_r - x - e_{r-1}^2 / q, |q| < pivmin ->
// -pivmin) from the Gershgorin interval widened by 2 m eps |T| + 2 pivmin; an interval that no longer splits in fp64 ends
// the loop early.  Then lane 0 walks the eigenvalues once: the shifts of the solves (closer than 10 eps |T| to the
// predecessor: pushed apart by that much) and the Gram-Schmidt groups (gaps <= 1e-3 |T|).
__global__ __launch_bounds__(64) void eig_bisect_kernel(int k, double* __restrict__ evals, EigWork w) {
  __shared__ double lam_s[EG_MAX_K];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1) return;
  const long long o = w.moff[s];
  const double* d = w.d + o;
  const double* e = w.e + o;
  double gl = DBL_MAX, gu = -DBL_MAX, e2max = 0.0;
  for (int r = lane; r < ms; r += 64) {
    const double lo = r > 0 ? fabs(e[r - 1]) : 0.0, hi = r < ms - 1 ? fabs(e[r]) : 0.0;
    gl = fmin(gl, d[r] - (lo + hi));
    gu = fmax(gu, d[r] + (lo + hi));
    e2max = fmax(e2max, hi * hi);
  }
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) {   // wave_min / wave_max written out: three calls change this kernel's code
    gl = fmin(gl, __shfl_xor(gl, x, 64));
    gu = fmax(gu, __shfl_xor(gu, x, 64));
    e2max = fmax(e2max, __shfl_xor(e2max, x, 64));
  }
  const double tn = fmax(fabs(gl), fabs(gu));
  const double pivmin = DBL_MIN * fmax(1.0, e2max);
  if (lane == 0) {
    w.scal[2 * s] = tn;
    w.scal[2 * s + 1] = pivmin;
  }
  double lam = 0.0;
  if (tn != 0.0 && lane < k) {
    const double widen = 2.0 * ms * EG_EPS * tn + 2.0 * pivmin;
    double lo = gl - widen, hi = gu + widen;
    const int want = ms - 1 - lane;
    for (int it = 0; it < EG_BISECT; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (!(mid > lo && mid < hi)) break;
      double q = d[0] - mid;
      if (fabs(q) < pivmin) q = -pivmin;
      int count = q < 0.0;
      for (int r = 1; r < ms; ++r) {
        const double er = e[r - 1];
        q = d[r] - mid - er * er / q;
        if (fabs(q) < pivmin) q = -pivmin;
        count += q < 0.0;
      }
      if (count > want) hi = mid; else lo = mid;
    }
    lam = 0.5 * (lo + hi);
  }
  if (lane < k) {
    evals[(long long)s * k + lane] = lam;
    lam_s[lane] = lam;
  }
  __syncthreads();
  if (lane == 0) {
    double* lp = w.lamp + (long long)s * k;
    int* gs = w.gst + (long long)s * k;
    const double pert = EG_PERT * EG_EPS * tn, ortol = EG_ORTOL * tn;
    double prev = lam_s[0];
    int g = 0;
    lp[0] = prev;
    gs[0] = 0;
    for (int i = 1; i < k; ++i) {
      double cur = lam_s[i];
      if (!(lam_s[i - 1] - cur <= ortol)) g = i;
      if (prev - cur < pert) cur = prev - pert;
      lp[i] = cur;
      gs[i] = g;
      prev = cur;
    }
  }
}

// ----------------------------------------------------------------------------------------------- (c) eigenvectors of T
__device__ __forceinline__ double eg_floor_pivot(double p, double floor) {
  return fabs(p) < floor ? copysign(floor, p) : p;
}

// Lane i: dgttrf of T - shift_i I (partial pivoting; a pivot below eps |T| in magnitude becomes +-eps |T|), and the
// normalised start vector of column i.  |T| = 0: the first k unit vectors, and nothing else runs for the slide.
__global__ __launch_bounds__(64) void eig_factor_kernel(int k, EigWork w) {
  const int s = blockIdx.x, i = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1 || i >= k) return;
  const long long o = w.moff[s];
  const double tn = w.scal[2 * s];
  double* z = w.z + o * k + i;
  if (tn == 0.0) {
    for (int r = 0; r < ms; ++r) z[(long long)r * k] = r == i ? 1.0 : 0.0;
    return;
  }
  double ss = 0.0;
  for (int r = 0; r < ms; ++r) {
    const double x = eg_start(r, i);
    ss += x * x;
  }
  const double nrm = sqrt(ss);
  for (int r = 0; r < ms; ++r) z[(long long)r * k] = eg_start(r, i) / nrm;

  const double* d = w.d + o;
  const double* e = w.e + o;
  double* dl = w.dl + o * k + i;
  double* dd = w.dd + o * k + i;
  double* du = w.du + o * k + i;
  double* du2 = w.du2 + o * k + i;
  unsigned char* sw = w.sw + o * k + i;
  const double shift = w.lamp[(long long)s * k + i];
  const double floor = EG_EPS * tn;
  double cur = d[0] - shift;                 // dd[r] as eliminated so far
  double up = ms > 1 ? e[0] : 0.0;           // du[r] as eliminated so far
  for (int r = 0; r < ms - 1; ++r) {
    const double sub = e[r];
    const double nxt = d[r + 1] - shift;
    const double up1 = r < ms - 2 ? e[r + 1] : 0.0;
    const bool swap = fabs(cur) < fabs(sub);
    const double piv = eg_floor_pivot(swap ? sub : cur, floor);
    const double fact = (swap ? cur : sub) / piv;
    const long long q = (long long)r * k;
    dd[q] = piv;
    dl[q] = fact;
    du[q] = swap ? nxt : up;
    sw[q] = swap ? 1 : 0;
    cur = swap ? up - fact * nxt : nxt - fact * up;
    if (r < ms - 2) du2[q] = swap ? up1 : 0.0;
    up = swap ? -fact * up1 : up1;
  }
  dd[(long long)(ms - 1) * k] = eg_floor_pivot(cur, floor);
}

// Lane i: dgtts2 (no transpose) of column i against its own factorisation, in place
__global__ __launch_bounds__(64) void eig_solve_kernel(int k, EigWork w) {
  const int s = blockIdx.x, i = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1 || i >= k || w.scal[2 * s] == 0.0) return;
  const long long o = w.moff[s];
  double* b = w.z + o * k + i;
  const double* dl = w.dl + o * k + i;
  const double* dd = w.dd + o * k + i;
  const double* du = w.du + o * k + i;
  const double* du2 = w.du2 + o * k + i;
  const unsigned char* sw = w.sw + o * k + i;
  double top = b[0];
  for (int r = 0; r < ms - 1; ++r) {
    const long long q = (long long)r * k;
    const double bot = b[q + k];
    const bool swap = sw[q] != 0;
    b[q] = swap ? bot : top;
    top = swap ? top - dl[q] * bot : bot - dl[q] * top;
  }
  double x1 = top / dd[(long long)(ms - 1) * k];      // b[r + 1]
  b[(long long)(ms - 1) * k] = x1;
  if (ms == 1) return;
  long long q = (long long)(ms - 2) * k;
  double x0 = (b[q] - du[q] * x1) / dd[q];            // b[r]
  b[q] = x0;
  for (int r = ms - 3; r >= 0; --r) {
    q = (long long)r * k;
    const double x = (b[q] - du[q] * x0 - du2[q] * x1) / dd[q];
    b[q] = x;
    x1 = x0;
    x0 = x;
  }
}

// One workgroup per slide, columns in order: column i is orthogonalised twice by modified Gram-Schmidt against the
// finished columns of its group, then normalised.  A thread keeps its rows of column i (r = tid + 256 t) in registers.
__global__ __launch_bounds__(EG_THREADS) void eig_ortho_kernel(int k, EigWork w) {
  __shared__ double slot[2][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1 || w.scal[2 * s] == 0.0) return;
  double* z = w.z + w.moff[s] * k;
  const int* gs = w.gst + (long long)s * k;
  constexpr int PER = EG_MAX_M / EG_THREADS;
  int turn = 0;
  for (int i = 0; i < k; ++i) {
    double y[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int r = tid + t * EG_THREADS;
      y[t] = r < ms ? z[(long long)r * k + i] : 0.0;
    }
    const int g0 = gs[i];
    for (int pass = 0; pass < 2; ++pass)
      for (int c = g0; c < i; ++c) {
        double zc[PER];
        double dot = 0.0;
#pragma unroll
        for (int t = 0; t < PER; ++t) {
          const int r = tid + t * EG_THREADS;
          zc[t] = r < ms ? z[(long long)r * k + c] : 0.0;
          dot = fma(zc[t], y[t], dot);
        }
        dot = block_sum4<false>(dot, slot[turn]);
        turn ^= 1;
#pragma unroll
        for (int t = 0; t < PER; ++t) y[t] -= dot * zc[t];
      }
    double ss = 0.0;
#pragma unroll
    for (int t = 0; t < PER; ++t) ss = fma(y[t], y[t], ss);
    ss = block_sum4<false>(ss, slot[turn]);
    turn ^= 1;
    const double nrm = sqrt(ss);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
      const int r = tid + t * EG_THREADS;
      if (r < ms) z[(long long)r * k + i] = y[t] / nrm;      // read again by this thread only: its own rows
    }
  }
}

// ------------------------------------------------------------------------------------------------------ (d) certificate
// Workgroup (a, s): |T z_a - lambda_a z_a|_2 / |T| and max_b |z_a^T z_b - delta_ab| over b >= a (wave w takes b = a + w,
// a + w + 4, ...).
__global__ __launch_bounds__(EG_THREADS) void eig_cert_kernel(int k, const double* __restrict__ evals, EigWork w) {
  __shared__ double dev_s[4];
  const int s = blockIdx.y, ca = blockIdx.x;
  const int ms = w.mv[s];
  if (ms < 1) return;
  double* out = w.certp + ((long long)s * k + ca) * 2;
  const double tn = w.scal[2 * s];
  if (tn == 0.0) {
    if (threadIdx.x == 0) out[0] = out[1] = 0.0;
    return;
  }
  const long long o = w.moff[s];
  const double* z = w.z + o * k;
  const double* d = w.d + o;
  const double* e = w.e + o;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double dev = 0.0;
  for (int cb = ca + wv; cb < k; cb += 4) {
    double dot = 0.0;
    for (int r = lane; r < ms; r += 64) dot = fma(z[(long long)r * k + ca], z[(long long)r * k + cb], dot);
    dot = wave_sum(dot);
    dev = fmax(dev, fabs(dot - (cb == ca ? 1.0 : 0.0)));
  }
  double res = 0.0;
  if (wv == 0) {
    const double lam = evals[(long long)s * k + ca];
    for (int r = lane; r < ms; r += 64) {
      double t = (d[r] - lam) * z[(long long)r * k + ca];
      if (r > 0) t += e[r - 1] * z[(long long)(r - 1) * k + ca];
      if (r < ms - 1) t += e[r] * z[(long long)(r + 1) * k + ca];
      res = fma(t, t, res);
    }
    res = wave_sum(res);
  }
  if (lane == 0) dev_s[wv] = dev;
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = sqrt(res) / tn;
    out[1] = fmax(fmax(dev_s[0], dev_s[1]), fmax(dev_s[2], dev_s[3]));
  }
}

__global__ __launch_bounds__(64) void eig_cert_reduce_kernel(int k, double* __restrict__ cert, EigWork w) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int ms = w.mv[s];
  double r = 0.0, dv = 0.0;
  if (ms >= 1 && lane < k) {
    r = w.certp[((long long)s * k + lane) * 2];
    dv = w.certp[((long long)s * k + lane) * 2 + 1];
  }
  // a NaN anywhere must survive the maximum: fmax drops it, so it is carried as a flag
  int nan = (r != r) || (dv != dv);
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) {   // wave_max written out: calls beside the flag's loop change this kernel's code
    r = fmax(r, __shfl_xor(r, x, 64));
    dv = fmax(dv, __shfl_xor(dv, x, 64));
    nan |= __shfl_xor(nan, x, 64);
  }
  if (lane == 0) {
    const double bad = __longlong_as_double(0x7FF8000000000000ll);
    cert[2 * s] = (ms < 1 || nan) ? bad : r;
    cert[2 * s + 1] = (ms < 1 || nan) ? bad : dv;
  }
}

// ---------------------------------------------------------------------------------- (e) back-transformation, (f) sign
// Workgroup (c, s): column c of Z in LDS, z[j+1:] -= tau_j v_j (v_j^T z[j+1:]) for j = m - 3 .. 0 (v_j = row j of A right
// of the diagonal, v_0 = 1 stored).  A thread owns the elements q = tid (mod 256) through every step, so one barrier (the
// sum's) separates the steps.  Then the vector is scaled by +-1 so that its component of largest magnitude (ties: the
// lowest index) is positive, and written row-major (m, k) at evec_offsets[s].
__global__ __launch_bounds__(EG_THREADS) void eig_back_kernel(const double* __restrict__ a,
                                                              const long long* __restrict__ aoff, int k,
                                                              double* __restrict__ evecs,
                                                              const long long* __restrict__ eoff, EigWork w) {
  __shared__ double zl[EG_MAX_M];
  __shared__ double slot[2][4];
  __shared__ double best_v[4];
  __shared__ int best_i[4];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int ms = w.mv[s];
  if (ms < 1) return;
  const long long o = w.moff[s];
  const double* A = a + aoff[s];
  const double* z = w.z + o * k;
  const double* tau = w.tau + o;
  for (int r = tid; r < ms; r += EG_THREADS) zl[r] = z[(long long)r * k + c];
  __syncthreads();
  int turn = 0;
  for (int j = ms - 3; j >= 0; --j) {
    const double t = tau[j];
    if (t == 0.0) continue;
    const double* v = A + (long long)j * ms;         // v[q] pairs with zl[q], q = j + 1 .. m - 1
    const int q0 = j + 1 + ((tid - (j + 1)) & (EG_THREADS - 1));
    double dot = 0.0;
    for (int q = q0; q < ms; q += EG_THREADS) dot = fma(v[q], zl[q], dot);
    dot = block_sum4<false>(dot, slot[turn]);
    turn ^= 1;
    const double f = t * dot;
    for (int q = q0; q < ms; q += EG_THREADS) zl[q] -= f * v[q];
  }
  __syncthreads();
  double bv = -1.0;
  int bi = 0;
  for (int r = tid; r < ms; r += EG_THREADS) {
    const double x = fabs(zl[r]);
    if (x > bv) bv = x, bi = r;
  }
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) {
    const double ov = __shfl_xor(bv, x, 64);
    const int oi = __shfl_xor(bi, x, 64);
    if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
  }
  if ((tid & 63) == 0) best_v[tid >> 6] = bv, best_i[tid >> 6] = bi;
  __syncthreads();
  bv = best_v[0], bi = best_i[0];
#pragma unroll
  for (int q = 1; q < 4; ++q)
    if (best_v[q] > bv || (best_v[q] == bv && best_i[q] < bi)) bv = best_v[q], bi = best_i[q];
  const double sign = zl[bi] < 0.0 ? -1.0 : 1.0;
  double* out = evecs + eoff[s];
  for (int r = tid; r < ms; r += EG_THREADS) out[(long long)r * k + c] = sign * zl[r];
}

}  // namespace

// --------------------------------------------------------------------------------------------------------- entry points
static int eig_check_sizes(int32_t S, int32_t max_m, int64_t sum_m, int32_t k) {
  if (S < 1 || max_m < 1 || k < 1 || k > max_m || sum_m < S || sum_m > (int64_t)S * max_m) return MCL_EINVAL;
  if (S > 65535 || max_m > EG_MAX_M || k > EG_MAX_K) return MCL_EUNSUPPORTED;
  return MCL_OK;
}

extern "C" int64_t mcl_sym_eig_workspace_bytes(int32_t S, int32_t max_m, int64_t sum_m, int32_t k) {
  const int rc = eig_check_sizes(S, max_m, sum_m, k);
  if (rc != MCL_OK) return rc;
  return 8 * eig_work_doubles(S, sum_m, k);
}

extern "C" int mcl_sym_eig_top(double* a, const int64_t* a_offsets, const int32_t* m, int32_t S, int32_t max_m,
                               int64_t sum_m, int32_t k, int32_t stages, double* evals, double* evecs,
                               const int64_t* evec_offsets, double* cert, void* work, mcl_stream_t stream) {
  if (!a || !a_offsets || !m || !evals || !evecs || !evec_offsets || !cert || !work) return MCL_EINVAL;
  if (stages < 1 || stages > 7) return MCL_EINVAL;
  const int rc = eig_check_sizes(S, max_m, sum_m, k);
  if (rc != MCL_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const long long* aoff = reinterpret_cast<const long long*>(a_offsets);
  const long long* eoff = reinterpret_cast<const long long*>(evec_offsets);
  const EigWork w = eig_carve(work, S, sum_m, k);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(eig_setup_kernel, dim3(1), dim3(EG_THREADS), 0, st, m, S, max_m, k, (long long)sum_m, w.moff, w.mv);
  MCL_CHECK_LAUNCH();
  if (stages & 1) {
    for (int j = 0; j <= (max_m >= 2 ? max_m - 2 : 0); ++j) {
      hipLaunchKernelGGL(eig_house_kernel, dim3(S), dim3(EG_THREADS), 0, st, a, aoff, j, w);
      if (j <= max_m - 3) {
        const int nb = (max_m - j - 1 + EG_ROWS - 1) / EG_ROWS;
        hipLaunchKernelGGL(eig_symv_kernel, dim3(nb, S), dim3(EG_THREADS), 0, st, (const double*)a, aoff, j, w);
        hipLaunchKernelGGL(eig_rank2_kernel, dim3(nb, S), dim3(EG_THREADS), 0, st, a, aoff, j, w);
      }
    }
    MCL_CHECK_LAUNCH();
  }
  if (stages & 2) {
    hipLaunchKernelGGL(eig_bisect_kernel, dim3(S), dim3(64), 0, st, k, evals, w);
    hipLaunchKernelGGL(eig_factor_kernel, dim3(S), dim3(64), 0, st, k, w);
    for (int it = 0; it < EG_ITERS; ++it) {
      hipLaunchKernelGGL(eig_solve_kernel, dim3(S), dim3(64), 0, st, k, w);
      hipLaunchKernelGGL(eig_ortho_kernel, dim3(S), dim3(EG_THREADS), 0, st, k, w);
    }
    hipLaunchKernelGGL(eig_cert_kernel, dim3(k, S), dim3(EG_THREADS), 0, st, k, (const double*)evals, w);
    hipLaunchKernelGGL(eig_cert_reduce_kernel, dim3(S), dim3(64), 0, st, k, cert, w);
    MCL_CHECK_LAUNCH();
  }
  if (stages & 4) {
    hipLaunchKernelGGL(eig_back_kernel, dim3(k, S), dim3(EG_THREADS), 0, st, (const double*)a, aoff, k, evecs, eoff, w);
    MCL_CHECK_LAUNCH();
  }
  return MCL_OK;
}
