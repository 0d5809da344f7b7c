// Expression as non-negative gene programs: X ~ W H with W, H >= 0 by scikit-learn's multiplicative-update solver
// (non_negative_factorization(solver="mu"), Frobenius and Kullback-Leibler loss), every row segment (slide) times every
// start of a call at once.  DESIGN 6.24 states the arithmetic, tests/nmf_reference.py restates it in numpy.  A problem p =
// segment j * n_init + start s; W is (n_init, rows, k), H is (segments * n_init, k, G).  Everything is fp64 (x may be fp32:
// converted on load), there is no floating-point atomic, and every sum runs in an order that depends on the segment's rows,
// G and k alone: a segment's factors are bit-identical alone and inside a stacked call, a start's alone and beside others.
//
//   nm_check_kernel     one wave per row: status = 0xFFFFFFFF - the first row that holds a negative or non-finite value.
//   nm_hht_kernel       H H^T (k, k) per problem on the MFMA: 16 waves split the genes, their sums are added in wave order.
//   nm_axis_sum_kernel  rowsum(H) or colsum(W) per problem: 16 strided partial sums per component, added in order.
//   nm_update_w_kernel  THE ROW PASS.  One workgroup = 16 rows: X H^T (or Q H^T for KL) on v_mfma_f64_16x16x4_f64 as
//                       deconv.hip's nn_products_kernel walks it, the genes split over the four waves and their sums added in
//                       wave order; W (H H^T) on the same MFMA, then W <- W o (numerator / denominator).
//                       KL: Q = X / max(W H, EPSILON) is formed tile by tile on the MFMA inside the pass and turned into
//                       the A operand through a wave-private LDS tile; it is never written to memory.
//   nm_wh_kernel        the stop rule's error from X itself.  One workgroup = 16 rows, the genes split over its four waves:
//                       W H tile by tile on the MFMA, the divergence terms summed per wave.
//   nm_atb_kernel       THE COLUMN PASS.  W^T B over one run of NM_RUN rows of a segment (a quarter per wave, added in wave
//                       order), B = X or W, or for KL the ratio Q formed in registers (the MFMA's result layout of W H is the
//                       B operand of W^T Q): the partial of that run.  The runs are added in run order by nm_update_h_kernel.
//   nm_update_h_kernel  H <- H o (numerator / denominator) for 32 genes: sums the run partials, (W^T W) H out of LDS.
//   nm_decide_kernel    adds the tile errors in tile order, takes sklearn's stop decision, freezes the problem.
//   nm_scale_h_kernel / nm_usage_kernel   programs = H / rowsum(H), usage = W o rowsum(H), dominant = argmax.
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NM_MAX_K = 64;
constexpr int NM_MAX_G = 16384;
constexpr int NM_MAX_PROBLEMS = 65535;
constexpr long long NM_MAX_CELLS = (1ll << 31) - 1;   // rows k
// Rows of one column-pass partial.  512: per-run partials, added by the H update (the shipped form).  A variant built with
// -DNM_RUN_ROWS=16384 (tools/build_variant.sh) is the other schedule-independent form at the benchmarked shapes: one
// workgroup per 16 columns walks every row tile of the segment with the accumulators resident (DESIGN 6.24 records both).
#ifndef NM_RUN_ROWS
#define NM_RUN_ROWS 512
#endif
constexpr int NM_RUN = NM_RUN_ROWS;
constexpr int NM_TILE = 16;                           // rows of a wave
constexpr int NM_HCHUNK = 32;                         // genes a workgroup of the H update / of H H^T stages
constexpr int NM_RECORD = 8;                          // doubles of a problem's record
constexpr double NM_EPSILON = 1.1920928955078125e-07; // sklearn's EPSILON = float32 eps

// problem p -> (segment, start, first row, rows); 0 rows where the offsets do not fit the launch
__device__ __forceinline__ int nm_problem(const long long* __restrict__ offsets, int p, int n_init, long long rows, int max_n,
                                          int* s, long long* r0) {
  *s = p % n_init;
  return segment_rows(offsets, p / n_init, rows, 1, max_n, r0);
}

// ------------------------------------------------------------------------------------------------------------ check
template <typename X>
__global__ __launch_bounds__(256) void nm_check_kernel(const X* __restrict__ x, long long ld, long long rows, int G,
                                                       unsigned* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const X* xr = x + row * ld;
  bool bad = false;
  for (int g = lane; g < G; g += 64) {
    const double v = ldd(xr + g);
    bad |= !(v >= 0.0 && v <= DBL_MAX);
  }
  if (__ballot(bad) != 0ull && lane == 0) atomicMax(status, 0xFFFFFFFFu - (unsigned)row);
}

// -------------------------------------------------------------------------------------------------------------- HHt
// One workgroup per (problem, 16 x 16 tile of H H^T): wave w of 16 sums the products of its own run of genes (the same run
// whatever the tile) on the MFMA; wave 0 adds the 16 sums in wave order.
__global__ __launch_bounds__(1024) void nm_hht_kernel(const double* __restrict__ H, int k, int G,
                                                      const int* __restrict__ active, double* __restrict__ hht) {
  __shared__ double red[15][4][64];
  const int p = blockIdx.y;
  if (!active[p]) return;
  const int nkt = (k + 15) / 16;
  const int ta = blockIdx.x / nkt, tb = blockIdx.x % nkt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const double* Hp = H + (long long)p * k * G;
  const int a = ta * 16 + lm, b = tb * 16 + lm;
  const bool oka = a < k, okb = b < k;
  const double* ha = Hp + (long long)(oka ? a : k - 1) * G;
  const double* hb = Hp + (long long)(okb ? b : k - 1) * G;
  const int span = ((G + 15) / 16 + 15) / 16 * 16;            // genes of a wave: a multiple of 16
  const int g_lo = wv * span, g_hi = g_lo + span < G ? g_lo + span : G;
  f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int j0 = g_lo; j0 < g_hi; j0 += 16) {
    double va[4], vb[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int g = j0 + 4 * t4 + lk;
      const bool ok = g < G;
      const int gc = ok ? g : G - 1;
      const double x = ha[gc], y = hb[gc];
      va[t4] = (ok && oka) ? x : 0.0;
      vb[t4] = (ok && okb) ? y : 0.0;
    }
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[t4], vb[t4], acc, 0, 0, 0);
  }
  if (wv > 0) {
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) red[wv - 1][qi][lane] = acc[qi];
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    double t = acc[qi];
#pragma unroll
    for (int w = 0; w < 15; ++w) t += red[w][qi][lane];
    const int row = ta * 16 + lk + 4 * qi, col = tb * 16 + lm;
    if (row < k && col < k) hht[(long long)p * k * k + row * k + col] = t;
  }
}

// --------------------------------------------------------------------------------------------------------- axis sum
// mode 0: out[p][a] = sum over g of H[p][a][g]; mode 1: out[p][a] = sum over the segment's rows of W[s][row][a]
__global__ __launch_bounds__(1024) void nm_axis_sum_kernel(const double* __restrict__ M, int mode,
                                                           const long long* __restrict__ offsets, int n_init, long long rows,
                                                           int G, int k, int max_n, const int* __restrict__ active,
                                                           int ignore_active, double* __restrict__ out) {
  __shared__ double part[16][NM_MAX_K];
  const int p = blockIdx.x, a = threadIdx.x & 63, q = threadIdx.x >> 6;
  if (!ignore_active && !active[p]) return;
  int s;
  long long r0;
  const int n_seg = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  if (n_seg == 0) return;
  const double* base = mode == 0 ? M + (long long)p * k * G : M + ((long long)s * rows + r0) * k;
  const long long sa = mode == 0 ? G : 1, sj = mode == 0 ? 1 : k;
  const int n = mode == 0 ? G : n_seg;
  const int ac = a < k ? a : k - 1;
  double acc = 0.0;
  for (int j = q; j < n; j += 16) acc += base[ac * sa + j * sj];
  part[q][a] = acc;
  __syncthreads();
  if (q == 0 && a < k) {
    double t = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += part[u][a];
    out[(long long)p * k + a] = t;
  }
}

// --------------------------------------------------------------------------------------------------------- row pass
// aux: H H^T (p, k, k) for Frobenius, rowsum(H) (p, k) for KL.  KL: the operand of the long product is not x but the ratio
// Q = x / max(WH, EPSILON), formed per 16 x 16 tile on the MFMA (W rows in registers, H streamed), which leaves it in the
// result layout; a wave-private LDS tile turns it into the A operand.  Q never reaches memory.
template <typename X, int NKT, bool KL>
__global__ __launch_bounds__(256) void nm_update_w_kernel(const X* __restrict__ x, long long ld,
                                                          const long long* __restrict__ offsets, int n_init, long long rows,
                                                          int G, int k, int max_n, double* __restrict__ W,
                                                          const double* __restrict__ H, const double* __restrict__ aux,
                                                          const int* __restrict__ active) {
  const int p = blockIdx.y;
  if (!active[p]) return;
  int s;
  long long r0;
  const int n = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.x * NM_TILE;                         // the four waves share 16 rows and split the genes
  if (i0 >= n) return;
  __shared__ double red[3][NKT * 4][64];
  __shared__ double qs[KL ? 4 : 1][16][17];
  double* Wp = W + ((long long)s * rows + r0) * k;
  const double* Hp = H + (long long)p * k * G;
  const int il = i0 + lm;
  const bool okn = il < n;
  const X* xs = x + r0 * ld;
  const X* xr = xs + (long long)(okn ? il : n - 1) * ld;
  const double* wr = Wp + (long long)(okn ? il : n - 1) * k;
  const double* sr[NKT];
  int ac[NKT];
  f64x4 acc[NKT], den[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int a = t * 16 + lm;
    ac[t] = a < k ? a : k - 1;
    sr[t] = Hp + (long long)ac[t] * G;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    den[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  // the old W of the elements this lane writes, and the denominator W (H H^T), both ahead of the long loop's stores
  double wold[NKT][4];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int row = i0 + lk + 4 * qi;
      wold[t][qi] = Wp[(long long)(row < n ? row : n - 1) * k + ac[t]];
    }
  double wa[KL ? 4 * NKT : 1];                                // KL: this lane's row of W, the A operand of W H
  if (KL) {
#pragma unroll
    for (int st = 0; st < 4 * NKT; ++st) {
      const int b = 4 * st + lk;
      const double v = wr[b < k ? b : k - 1];
      wa[KL ? st : 0] = (b < k && okn) ? v : 0.0;
    }
  }
  if (!KL && wv == 0) {
    const double* hht = aux + (long long)p * k * k;
    for (int b0 = 0; b0 < k; b0 += 4) {
      const int b = b0 + lk;
      const int bc = b < k ? b : k - 1;
      const double wv_ = wr[bc];
      const double a_op = (b < k && okn) ? wv_ : 0.0;
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const double hv = hht[bc * k + ac[t]];
        den[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_op, (b < k && t * 16 + lm < k) ? hv : 0.0, den[t], 0, 0, 0);
      }
    }
  }
  const int span = ((G + 15) / 16 + 3) / 4 * 16;              // genes of a wave: a multiple of 16
  const int g_lo = wv * span, g_hi = g_lo + span < G ? g_lo + span : G;
  for (int j0 = g_lo; j0 < g_hi; j0 += 16) {
    double a[4];
    int jc[4];
    bool ok[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int j = j0 + 4 * lk + t4;
      ok[t4] = j < G;
      jc[t4] = ok[t4] ? j : G - 1;
      if (!KL) {
        const double v = ldd(xr + jc[t4]);
        a[t4] = (ok[t4] && okn) ? v : 0.0;
      }
    }
    if (KL) {
      const int g = j0 + lm;
      const bool okg = g < G;
      const int gc = okg ? g : G - 1;
      double xv[4];
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const int row = i0 + lk + 4 * qi;
        xv[qi] = ldd(xs + (long long)(row < n ? row : n - 1) * ld + gc);
      }
      f64x4 wh = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int st = 0; st < 4 * NKT; ++st) {
        const int b = 4 * st + lk;
        const double hv = Hp[(long long)(b < k ? b : k - 1) * G + gc];
        wh = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[KL ? st : 0], (b < k && okg) ? hv : 0.0, wh, 0, 0, 0);
      }
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const int row = i0 + lk + 4 * qi;
        const double whc = wh[qi] < NM_EPSILON ? NM_EPSILON : wh[qi];
        const double q = xv[qi] / whc;
        qs[KL ? wv : 0][lk + 4 * qi][lm] = (row < n && okg) ? q : 0.0;
      }
      wave_sync();
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) a[t4] = qs[KL ? wv : 0][lm][4 * lk + t4];
      wave_sync();
    }
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {
        const double v = sr[t][jc[t4]];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t4], ok[t4] ? v : 0.0, acc[t], 0, 0, 0);
      }
  }
  if (wv > 0) {
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) red[wv - 1][t * 4 + qi][lane] = acc[t][qi];
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const double hs = KL ? aux[(long long)p * k + ac[t]] : 0.0;
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int row = i0 + lk + 4 * qi;
      const int col = t * 16 + lm;
      acc[t][qi] = ((acc[t][qi] + red[0][t * 4 + qi][lane]) + red[1][t * 4 + qi][lane]) + red[2][t * 4 + qi][lane];
      double d = KL ? hs : den[t][qi];
      if (d == 0.0) d = NM_EPSILON;
      const double wn = wold[t][qi] * (acc[t][qi] / d);
      if (row < n && col < k) Wp[(long long)row * k + col] = wn;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- W H
// The wave's divergence terms into err_part[p][tile][wave][2]: Frobenius { sum (x - WH)^2, 0 }, KL { sum over x > EPSILON of
// x log(x / max(WH, EPSILON)), sum over x > EPSILON of x }.
template <typename X, int NKT>
__global__ __launch_bounds__(256) void nm_wh_kernel(const X* __restrict__ x, long long ld,
                                                    const long long* __restrict__ offsets, int n_init, long long rows, int G,
                                                    int k, int max_n, int kl, const double* __restrict__ W,
                                                    const double* __restrict__ H, const int* __restrict__ active,
                                                    int ignore_active, double* __restrict__ err_part, int tiles_max) {
  const int p = blockIdx.y;
  if (!ignore_active && !active[p]) return;
  int s;
  long long r0;
  const int n = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int tile = blockIdx.x;                                 // the four waves share 16 rows and split the genes
  const int i0 = tile * NM_TILE;
  if (i0 >= n) return;
  const double* Wp = W + ((long long)s * rows + r0) * k;
  const double* Hp = H + (long long)p * k * G;
  const X* xs = x + r0 * ld;
  const int il = i0 + lm;
  const bool okn = il < n;
  const double* wr = Wp + (long long)(okn ? il : n - 1) * k;
  double wa[4 * NKT];
#pragma unroll
  for (int st = 0; st < 4 * NKT; ++st) {
    const int b = 4 * st + lk;
    const double v = wr[b < k ? b : k - 1];
    wa[st] = (b < k && okn) ? v : 0.0;
  }
  double e1 = 0.0, e2 = 0.0;
  const int span = ((G + 15) / 16 + 3) / 4 * 16;              // genes of a wave: a multiple of 16
  const int g_lo = wv * span, g_hi = g_lo + span < G ? g_lo + span : G;
  for (int g0 = g_lo; g0 < g_hi; g0 += 16) {
    const int g = g0 + lm;
    const bool okg = g < G;
    const int gc = okg ? g : G - 1;
    double xv[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int row = i0 + lk + 4 * qi;
      xv[qi] = ldd(xs + (long long)(row < n ? row : n - 1) * ld + gc);
    }
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int st = 0; st < 4 * NKT; ++st) {
      const int b = 4 * st + lk;
      const double hv = Hp[(long long)(b < k ? b : k - 1) * G + gc];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[st], (b < k && okg) ? hv : 0.0, acc, 0, 0, 0);
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int row = i0 + lk + 4 * qi;
      const bool okx = row < n && okg;
      const double wh = acc[qi];
      if (kl) {
        const double whc = wh < NM_EPSILON ? NM_EPSILON : wh;
        if (okx && xv[qi] > NM_EPSILON) {
          e1 += xv[qi] * log(xv[qi] / whc);
          e2 += xv[qi];
        }
      } else if (okx) {
        const double d = xv[qi] - wh;
        e1 = fma(d, d, e1);
      }
    }
  }
  e1 = wave_sum(e1);
  e2 = wave_sum(e2);
  if (lane == 0) {
    err_part[(((long long)p * tiles_max + tile) * 4 + wv) * 2] = e1;
    err_part[(((long long)p * tiles_max + tile) * 4 + wv) * 2 + 1] = e2;
  }
}

// ------------------------------------------------------------------------------------------------------ column pass
// part[p][run][a][c] = sum over the run's rows i of W[s][i][a] B[s][i][c], c < N: B = X (N = G) or W itself (N = k).  KL: B is
// the ratio Q = x / max(WH, EPSILON) of the rows and columns at hand, formed on the MFMA from W's rows and the 16 columns of
// H this workgroup keeps in registers; its result layout IS the B operand of W^T Q, so Q never leaves the registers.
template <typename B, int NKT, bool KL>
__global__ __launch_bounds__(256) void nm_atb_kernel(const double* __restrict__ W, const B* __restrict__ Bm, long long ldb,
                                                     long long b_start_stride, int N, const long long* __restrict__ offsets,
                                                     int n_init, long long rows, int k, int max_n,
                                                     const int* __restrict__ active, double* __restrict__ part, int runs_max,
                                                     const double* __restrict__ H) {
  const int p = blockIdx.z;
  if (!active[p]) return;
  int s;
  long long r0;
  const int n = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int run = blockIdx.x;
  const int i_lo = run * NM_RUN;
  const int c0 = blockIdx.y * 16;                              // the four waves share 16 columns and split the run's rows
  if (i_lo >= n || c0 >= N) return;
  __shared__ double red[3][NKT * 4][64];
  const int i_hi = i_lo + NM_RUN < n ? i_lo + NM_RUN : n;
  const int w_lo = i_lo + wv * (NM_RUN / 4), w_hi = w_lo + NM_RUN / 4 < i_hi ? w_lo + NM_RUN / 4 : i_hi;
  const double* Wp = W + ((long long)s * rows + r0) * k;
  const B* Bp = Bm + (long long)s * b_start_stride + r0 * ldb;
  const int c = c0 + lm;
  const bool okc = c < N;
  const int cc = okc ? c : N - 1;
  int ac[NKT];
  bool oka[NKT];
  f64x4 acc[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int a = t * 16 + lm;
    oka[t] = a < k;
    ac[t] = oka[t] ? a : k - 1;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  double hb[KL ? 4 * NKT : 1];                                // KL: the B operand of W H, this lane's column of H
  if (KL) {
    const double* Hp = H + (long long)p * k * N;
#pragma unroll
    for (int st = 0; st < 4 * NKT; ++st) {
      const int b = 4 * st + lk;
      const double v = Hp[(long long)(b < k ? b : k - 1) * N + cc];
      hb[KL ? st : 0] = (b < k && okc) ? v : 0.0;
    }
  }
  for (int i0 = w_lo; i0 < w_hi; i0 += 16) {
    double bv[4], av[4][NKT];
    f64x4 wh = f64x4{0.0, 0.0, 0.0, 0.0};
    if (KL) {
      const int ir = i0 + lm;
      const double* wr = Wp + (long long)(ir < w_hi ? ir : i_hi - 1) * k;
#pragma unroll
      for (int st = 0; st < 4 * NKT; ++st) {
        const int b = 4 * st + lk;
        const double w = wr[b < k ? b : k - 1];
        wh = __builtin_amdgcn_mfma_f64_16x16x4f64((b < k && ir < w_hi) ? w : 0.0, hb[KL ? st : 0], wh, 0, 0, 0);
      }
    }
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int i = i0 + 4 * t4 + lk;
      const bool ok = i < w_hi;
      const long long ic = ok ? i : i_hi - 1;
      const double v = ldd(Bp + ic * ldb + cc);
      if (KL) {                                                // register t4 of W H holds row i0 + 4 t4 + lk, column c
        const double whc = wh[t4] < NM_EPSILON ? NM_EPSILON : wh[t4];
        const double q = v / whc;
        bv[t4] = (ok && okc) ? q : 0.0;
      } else {
        bv[t4] = (ok && okc) ? v : 0.0;
      }
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const double w = Wp[ic * k + ac[t]];
        av[t4][t] = (ok && oka[t]) ? w : 0.0;
      }
    }
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
      for (int t = 0; t < NKT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t4][t], bv[t4], acc[t], 0, 0, 0);
  }
  if (wv > 0) {
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) red[wv - 1][t * 4 + qi][lane] = acc[t][qi];
  }
  __syncthreads();
  if (wv != 0) return;
  double* out = part + ((long long)p * runs_max + run) * k * N;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int a = t * 16 + lk + 4 * qi;
      const double v = ((acc[t][qi] + red[0][t * 4 + qi][lane]) + red[1][t * 4 + qi][lane]) + red[2][t * 4 + qi][lane];
      if (a < k && okc) out[(long long)a * N + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ X-shared fused pass
// The Frobenius iteration's row pass and column pass as ONE launch that reads X once for up to SB starts (built with
// -DNM_FUSED -DNM_RUN_ROWS=128; measured against the two-pass form in DESIGN 6.24).  A workgroup of 4 waves owns a tile of 128
// rows of one segment and a batch of SB starts.  Phase A: wave w walks the genes for its two 16-row tiles in turn; the x operand of a
// 16-gene step is loaded once and serves every start's X H^T.  Then W (H H^T), the W update, the new rows to memory and to
// LDS.  Phase C: the waves take 16-gene chunks in turn; the 128 x 16 fragment of x sits in 32 registers per lane and serves
// every start's W^T X from the W rows in LDS; W^T W of the tile likewise.  The tile's partials go where nm_atb_kernel's runs
// of 128 rows would put them, so nm_update_h_kernel adds them in tile order.
#ifdef NM_FUSED
static_assert(NM_RUN_ROWS == 128, "the fused pass writes one partial per 128-row tile");
template <typename X, int NKT, int SB>
__global__ __launch_bounds__(256) void nm_fused_kernel(const X* __restrict__ x, long long ld,
                                                       const long long* __restrict__ offsets, int n_init, long long rows,
                                                       int G, int k, int max_n, double* __restrict__ W,
                                                       const double* __restrict__ H, const double* __restrict__ hht_all,
                                                       const int* __restrict__ active, double* __restrict__ wtx_part,
                                                       double* __restrict__ wtw_part, int runs_max) {
  extern __shared__ __align__(16) double nf_w[];               // [SB][128][k + 1]
  const int seg = blockIdx.y, s0 = blockIdx.z * SB, tile = blockIdx.x;
  long long r0;
  const int n = segment_rows(offsets, seg, rows, 1, max_n, &r0);
  const int t0 = tile * 128;
  if (t0 >= n) return;
  bool act[SB];
  int sc[SB];
  bool any = false;
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) {
    sc[sb] = s0 + sb < n_init ? s0 + sb : n_init - 1;
    act[sb] = s0 + sb < n_init && active[seg * n_init + sc[sb]] != 0;
    any |= act[sb];
  }
  if (!any) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int ws = k + 1;
  int ac[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) ac[t] = t * 16 + lm < k ? t * 16 + lm : k - 1;
  for (int half = 0; half < 2; ++half) {                      // a wave owns two 16-row tiles, one after the other
  const int rt = wv * 2 + half;
  const int i0 = t0 + rt * 16;
  const int il = i0 + lm;
  const bool okn = il < n;
  const X* xr = x + (r0 + (okn ? il : n - 1)) * ld;
  // ---- phase A: X H^T of every start from one read of the x operand
  f64x4 acc[SB][NKT];
#pragma unroll
  for (int sb = 0; sb < SB; ++sb)
#pragma unroll
    for (int t = 0; t < NKT; ++t) acc[sb][t] = f64x4{0.0, 0.0, 0.0, 0.0};
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
    }
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      if (!act[sb]) continue;
      const double* Hp = H + (long long)(seg * n_init + sc[sb]) * k * G;
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
          const double v = Hp[(long long)ac[t] * G + jc[t4]];
          acc[sb][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t4], ok[t4] ? v : 0.0, acc[sb][t], 0, 0, 0);
        }
    }
  }
  // ---- the W update of the wave's 16 rows, start by start
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) {
    if (!act[sb]) continue;
    const int p = seg * n_init + sc[sb];
    double* Wp = W + ((long long)sc[sb] * rows + r0) * k;
    const double* wr = Wp + (long long)(okn ? il : n - 1) * k;
    const double* hht = hht_all + (long long)p * k * k;
    double* wl = nf_w + (long long)sb * 128 * ws;
    f64x4 den[NKT];
    double wold[NKT][4];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      den[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const int row = i0 + lk + 4 * qi;
        wold[t][qi] = Wp[(long long)(row < n ? row : n - 1) * k + ac[t]];
      }
    }
    for (int b0 = 0; b0 < k; b0 += 4) {
      const int b = b0 + lk;
      const int bc = b < k ? b : k - 1;
      const double wv_ = wr[bc];
      const double a_op = (b < k && okn) ? wv_ : 0.0;
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const double hv = hht[bc * k + ac[t]];
        den[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_op, (b < k && t * 16 + lm < k) ? hv : 0.0, den[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const int row = i0 + lk + 4 * qi, col = t * 16 + lm;
        double d = den[t][qi];
        if (d == 0.0) d = NM_EPSILON;
        const double wn = wold[t][qi] * (acc[sb][t][qi] / d);
        if (col < k) {
          wl[(rt * 16 + lk + 4 * qi) * ws + col] = row < n ? wn : 0.0;
          if (row < n) Wp[(long long)row * k + col] = wn;
        }
      }
  }
  }
  __syncthreads();
  // ---- phase C: the tile's W^T X (16 genes at a time, the x fragment in registers for every start) and W^T W
  for (int c0 = wv * 16; c0 < G; c0 += 4 * 16) {
    const int c = c0 + lm;
    const bool okc = c < G;
    const int cc = okc ? c : G - 1;
    double xv[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) {
      const int row = t0 + 4 * t + lk;
      const double v = ldd(x + (r0 + (row < n ? row : n - 1)) * ld + cc);
      xv[t] = (row < n && okc) ? v : 0.0;
    }
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      if (!act[sb]) continue;
      const double* wl = nf_w + (long long)sb * 128 * ws;
      f64x4 out[NKT];
#pragma unroll
      for (int t = 0; t < NKT; ++t) out[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < 32; ++t)
#pragma unroll
        for (int tt = 0; tt < NKT; ++tt) {
          const double w = wl[(4 * t + lk) * ws + ac[tt]];
          out[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(tt * 16 + lm < k ? w : 0.0, xv[t], out[tt], 0, 0, 0);
        }
      double* dst = wtx_part + ((long long)(seg * n_init + sc[sb]) * runs_max + tile) * k * G;
#pragma unroll
      for (int tt = 0; tt < NKT; ++tt)
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
          const int a = tt * 16 + lk + 4 * qi;
          if (a < k && okc) dst[(long long)a * G + c] = out[tt][qi];
        }
    }
  }
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) {
    if (!act[sb]) continue;
    const double* wl = nf_w + (long long)sb * 128 * ws;
    double* dst = wtw_part + ((long long)(seg * n_init + sc[sb]) * runs_max + tile) * k * k;
    for (int e = wv; e < NKT * NKT; e += 4) {
      const int ta = e / NKT, tb = e % NKT;
      const int ca = ta * 16 + lm, cb = tb * 16 + lm;
      f64x4 out = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < 32; ++t) {
        const double wa = wl[(4 * t + lk) * ws + (ca < k ? ca : k - 1)];
        const double wb = wl[(4 * t + lk) * ws + (cb < k ? cb : k - 1)];
        out = __builtin_amdgcn_mfma_f64_16x16x4f64(ca < k ? wa : 0.0, cb < k ? wb : 0.0, out, 0, 0, 0);
      }
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const int a = ta * 16 + lk + 4 * qi;
        if (a < k && cb < k) dst[a * k + cb] = out[qi];
      }
    }
  }
}
#endif

// --------------------------------------------------------------------------------------------------------- H update
__global__ __launch_bounds__(256) void nm_update_h_kernel(const double* __restrict__ wtx_part,
                                                          const double* __restrict__ wtw_part,
                                                          const double* __restrict__ wsum,
                                                          const long long* __restrict__ offsets, int n_init, long long rows,
                                                          int G, int k, int max_n, int kl, int runs_max,
                                                          const int* __restrict__ active, double* __restrict__ H) {
  __shared__ double wtw_s[NM_MAX_K * NM_MAX_K];
  __shared__ double h_s[NM_MAX_K][NM_HCHUNK + 1];
  const int p = blockIdx.y, tid = threadIdx.x;
  if (!active[p]) return;
  int s;
  long long r0;
  const int n = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  if (n == 0) return;
  const int nruns = (n + NM_RUN - 1) / NM_RUN;
  const int g0 = blockIdx.x * NM_HCHUNK;
  double* Hp = H + (long long)p * k * G;
  if (!kl) {
    const double* wp = wtw_part + (long long)p * runs_max * k * k;
    for (int e = tid; e < k * k; e += 256) {
      double t = 0.0;
      for (int r = 0; r < nruns; ++r) t += wp[(long long)r * k * k + e];
      wtw_s[e] = t;
    }
  }
  for (int e = tid; e < k * NM_HCHUNK; e += 256) {
    const int a = e / NM_HCHUNK, gg = e % NM_HCHUNK;
    const int g = g0 + gg;
    const double v = Hp[(long long)a * G + (g < G ? g : G - 1)];
    h_s[a][gg] = g < G ? v : 0.0;
  }
  __syncthreads();
  const double* xp = wtx_part + (long long)p * runs_max * k * G;
  for (int e = tid; e < k * NM_HCHUNK; e += 256) {
    const int a = e / NM_HCHUNK, gg = e % NM_HCHUNK;
    const int g = g0 + gg;
    const int gc = g < G ? g : G - 1;
    double num = 0.0;
    for (int r = 0; r < nruns; ++r) num += xp[((long long)r * k + a) * G + gc];
    double d;
    if (kl) {
      d = wsum[(long long)p * k + a];
      if (d == 0.0) d = 1.0;
    } else {
      d = 0.0;
      for (int b = 0; b < k; ++b) d = fma(wtw_s[a * k + b], h_s[b][gg], d);
    }
    if (d == 0.0) d = NM_EPSILON;
    double hn = h_s[a][gg] * (num / d);
    if (kl && hn < DBL_EPSILON) hn = 0.0;
    if (g < G) Hp[(long long)a * G + g] = hn;
  }
}

// ----------------------------------------------------------------------------------------------------------- decide
// record[p]: { error at init, previous error, last error, n_iter, converged, final error, 0, 0 }.  phase 0: the error at
// init; 1: the check of iteration ``it``; 2: the final error (frozen problems too).
__global__ __launch_bounds__(64) void nm_decide_kernel(const double* __restrict__ err_part, int tiles_max,
                                                       const long long* __restrict__ offsets, int n_init, long long rows,
                                                       int max_n, int k, int kl, const double* __restrict__ wsum,
                                                       const double* __restrict__ hsum, int phase, int it, double tol,
                                                       int max_iter, int* __restrict__ active, double* __restrict__ record,
                                                       double* __restrict__ history, int hist_len) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (phase == 1 && !active[p]) return;
  int s;
  long long r0;
  const int n = nm_problem(offsets, p, n_init, rows, max_n, &s, &r0);
  if (n == 0) return;
  const int tiles = (n + NM_TILE - 1) / NM_TILE * 4;           // a partial per wave of a tile
  const double* ep = err_part + (long long)p * tiles_max * 8;
  double e1 = 0.0, e2 = 0.0;
  for (int t = lane; t < tiles; t += 64) {
    e1 += ep[2 * t];
    e2 += ep[2 * t + 1];
  }
  e1 = wave_sum(e1);
  e2 = wave_sum(e2);
  double err;
  if (kl) {
    const double pr = lane < k ? wsum[(long long)p * k + lane] * hsum[(long long)p * k + lane] : 0.0;
    const double sum_wh = wave_sum(pr);
    double res = e1 + (sum_wh - e2);
    res = res > 0.0 ? res : 0.0;
    err = sqrt(2.0 * res);
  } else {
    err = sqrt(e1);
  }
  if (lane != 0) return;
  double* rec = record + (long long)p * NM_RECORD;
  if (phase == 0) {
    rec[0] = err;
    rec[1] = err;
    rec[2] = err;
    rec[3] = (double)max_iter;
    rec[4] = 0.0;
    rec[5] = err;
    rec[6] = 0.0;
    rec[7] = 0.0;
    if (hist_len > 0) history[(long long)p * hist_len] = err;
  } else if (phase == 1) {
    rec[2] = err;
    const int slot = it / 10;
    if (slot < hist_len) history[(long long)p * hist_len + slot] = err;
    if ((rec[1] - err) / rec[0] < tol) {
      active[p] = 0;
      rec[3] = (double)it;
      rec[4] = it < max_iter ? 1.0 : 0.0;
    } else {
      rec[1] = err;
    }
  } else {
    rec[5] = err;
  }
}

// --------------------------------------------------------------------------------------------------------- programs
__global__ __launch_bounds__(256) void nm_scale_h_kernel(const double* __restrict__ H, const double* __restrict__ hsum, int G,
                                                         int k, double* __restrict__ programs) {
  const int g = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y, j = blockIdx.z;
  if (g >= G) return;
  const long long e = ((long long)j * k + a) * G + g;
  const double hs = hsum[(long long)j * k + a];
  programs[e] = hs > 0.0 ? H[e] / hs : 0.0;
}

__global__ __launch_bounds__(256) void nm_usage_kernel(const double* __restrict__ W, const double* __restrict__ hsum,
                                                       const long long* __restrict__ offsets, long long rows, int k, int max_n,
                                                       double* __restrict__ usage, int* __restrict__ dominant) {
  const int j = blockIdx.y, lane = threadIdx.x & 63;
  long long r0;
  const int n = segment_rows(offsets, j, rows, 1, max_n, &r0);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long long row = r0 + i;
  const bool live = lane < k;
  const int lc = live ? lane : k - 1;
  const double w = W[row * k + lc], hs = hsum[(long long)j * k + lc];
  const double u = live ? w * hs : 0.0;
  const double top = wave_max(u);
  const int dom = top > 0.0 ? __ffsll((unsigned long long)__ballot(live && u == top)) - 1 : -1;
  if (live) usage[row * k + lane] = u;
  if (lane == 0) dominant[row] = dom;
}

// ------------------------------------------------------------------------------------------------------------- host
struct nm_plan {
  int runs_max, tiles_max;
  long long hht, hsum, wsum, wtw, wtx, errp, total;      // offsets in doubles
};

inline bool nm_shape_ok(int64_t rows, int32_t G, int32_t k, int32_t S, int32_t n_init, int32_t max_n) {
  return rows >= 1 && G >= 1 && k >= 1 && S >= 1 && n_init >= 1 && max_n >= 1 && max_n <= rows;
}
inline bool nm_limits_ok(int64_t rows, int32_t G, int32_t k, int32_t S, int32_t n_init) {
  return k <= NM_MAX_K && G <= NM_MAX_G && (long long)S * n_init <= NM_MAX_PROBLEMS && (long long)rows * k <= NM_MAX_CELLS;
}

inline nm_plan nm_make_plan(int64_t rows, int32_t G, int32_t k, int32_t S, int32_t n_init, int32_t max_n, int32_t kl) {
  nm_plan pl;
  const long long P = (long long)S * n_init;
  pl.runs_max = (max_n + NM_RUN - 1) / NM_RUN;
  pl.tiles_max = (max_n + NM_TILE - 1) / NM_TILE;
  long long at = 0;
  pl.hht = at;
  at += P * k * k;
  pl.hsum = at;
  at += P * k;
  pl.wsum = at;
  at += P * k;
  pl.wtw = at;
  at += kl ? 0 : P * pl.runs_max * k * k;
  pl.wtx = at;
  at += P * pl.runs_max * k * G;
  pl.errp = at;
  at += P * pl.tiles_max * 8;
  pl.total = at;
  return pl;
}

struct nm_args {
  const void* x;
  long long ld;
  int dtype;
  const long long* offsets;
  int S, n_init;
  long long rows;
  int G, k, max_n, kl;
  double *W, *H, *work;
  int* active;
};

template <typename X, bool KL>
void nm_launch_update_w(const nm_args& a, const X* x, const double* aux, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.max_n, NM_TILE), (unsigned)(a.S * a.n_init)), block(256);
#define NM_UW(NKT)                                                                                                       \
  hipLaunchKernelGGL((nm_update_w_kernel<X, NKT, KL>), grid, block, 0, st, x, a.ld, a.offsets, a.n_init, a.rows, a.G, a.k, \
                     a.max_n, a.W, (const double*)a.H, aux, (const int*)a.active)
  switch ((a.k + 15) / 16) {
    case 1: NM_UW(1); break;
    case 2: NM_UW(2); break;
    case 3: NM_UW(3); break;
    default: NM_UW(4); break;
  }
#undef NM_UW
}

template <typename B, bool KL>
void nm_launch_atb(const nm_args& a, const B* Bm, long long ldb, long long b_start_stride, int N, double* part,
                   const nm_plan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.runs_max, (unsigned)ceil_div(N, 16), (unsigned)(a.S * a.n_init)), block(256);
#define NM_ATB(NKT)                                                                                                          \
  hipLaunchKernelGGL((nm_atb_kernel<B, NKT, KL>), grid, block, 0, st, (const double*)a.W, Bm, ldb, b_start_stride, N, a.offsets, \
                     a.n_init, a.rows, a.k, a.max_n, (const int*)a.active, part, pl.runs_max, (const double*)a.H)
  switch ((a.k + 15) / 16) {
    case 1: NM_ATB(1); break;
    case 2: NM_ATB(2); break;
    case 3: NM_ATB(3); break;
    default: NM_ATB(4); break;
  }
#undef NM_ATB
}

template <typename X>
void nm_launch_wh(const nm_args& a, const X* x, int ignore_active, const nm_plan& pl, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.max_n, NM_TILE), (unsigned)(a.S * a.n_init)), block(256);
#define NM_WH(NKT)                                                                                                          \
  hipLaunchKernelGGL((nm_wh_kernel<X, NKT>), grid, block, 0, st, x, a.ld, a.offsets, a.n_init, a.rows, a.G, a.k, a.max_n, a.kl, \
                     (const double*)a.W, (const double*)a.H, (const int*)a.active, ignore_active, a.work + pl.errp, pl.tiles_max)
  switch ((a.k + 15) / 16) {
    case 1: NM_WH(1); break;
    case 2: NM_WH(2); break;
    case 3: NM_WH(3); break;
    default: NM_WH(4); break;
  }
#undef NM_WH
}

void nm_launch_axis_sum(const nm_args& a, int mode, int ignore_active, double* out, hipStream_t st) {
  hipLaunchKernelGGL(nm_axis_sum_kernel, dim3((unsigned)(a.S * a.n_init)), dim3(1024), 0, st,
                     mode == 0 ? (const double*)a.H : (const double*)a.W, mode, a.offsets, a.n_init, a.rows, a.G, a.k, a.max_n,
                     (const int*)a.active, ignore_active, out);
}

#ifdef NM_FUSED
template <typename X, int NKT, int SB>
void nm_launch_fused_as(const nm_args& a, const X* x, const nm_plan& pl, hipStream_t st) {
  const size_t lds = (size_t)SB * 128 * (a.k + 1) * 8;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nm_fused_kernel<X, NKT, SB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, SB * 128 * (NKT * 16 + 1) * 8);
  }
  const dim3 grid((unsigned)pl.runs_max, (unsigned)a.S, (unsigned)ceil_div(a.n_init, SB)), block(256);
  hipLaunchKernelGGL((nm_fused_kernel<X, NKT, SB>), grid, block, lds, st, x, a.ld, a.offsets, a.n_init, a.rows, a.G, a.k,
                     a.max_n, a.W, (const double*)a.H, (const double*)(a.work + pl.hht), (const int*)a.active, a.work + pl.wtx,
                     a.work + pl.wtw, pl.runs_max);
}
// four starts share a read of x where their W rows fit the LDS (k <= 32), two beyond
template <typename X>
void nm_launch_fused(const nm_args& a, const X* x, const nm_plan& pl, hipStream_t st) {
  switch ((a.k + 15) / 16) {
    case 1: nm_launch_fused_as<X, 1, 4>(a, x, pl, st); break;
    case 2: nm_launch_fused_as<X, 2, 4>(a, x, pl, st); break;
    case 3: nm_launch_fused_as<X, 3, 2>(a, x, pl, st); break;
    default: nm_launch_fused_as<X, 4, 2>(a, x, pl, st); break;
  }
}
#endif

// one multiplicative-update iteration of every live problem
template <typename X>
void nm_enqueue_step(const nm_args& a, const X* x, int update_h, bool first, const nm_plan& pl, hipStream_t st) {
  const int P = a.S * a.n_init;
  double* w = a.work;
  if (a.kl) {
    if (update_h || first) nm_launch_axis_sum(a, 0, 0, w + pl.hsum, st);
    nm_launch_update_w<X, true>(a, x, (const double*)(w + pl.hsum), st);
    if (!update_h) return;
    nm_launch_atb<X, true>(a, x, a.ld, 0ll, a.G, w + pl.wtx, pl, st);
    nm_launch_axis_sum(a, 1, 0, w + pl.wsum, st);
  } else {
    if (update_h || first)
      hipLaunchKernelGGL(nm_hht_kernel, dim3((unsigned)(((a.k + 15) / 16) * ((a.k + 15) / 16)), (unsigned)P), dim3(1024), 0, st,
                         (const double*)a.H, a.k, a.G, (const int*)a.active, w + pl.hht);
#ifdef NM_FUSED
    if (update_h) {
      nm_launch_fused(a, x, pl, st);
    } else {
      nm_launch_update_w<X, false>(a, x, (const double*)(w + pl.hht), st);
      return;
    }
#else
    nm_launch_update_w<X, false>(a, x, (const double*)(w + pl.hht), st);
    if (!update_h) return;
    nm_launch_atb<X, false>(a, x, a.ld, 0ll, a.G, w + pl.wtx, pl, st);
    nm_launch_atb<double, false>(a, (const double*)a.W, (long long)a.k, a.rows * (long long)a.k, a.k, w + pl.wtw, pl, st);
#endif
  }
  hipLaunchKernelGGL(nm_update_h_kernel, dim3((unsigned)ceil_div(a.G, NM_HCHUNK), (unsigned)P), dim3(256), 0, st,
                     (const double*)(w + pl.wtx), (const double*)(w + pl.wtw), (const double*)(w + pl.wsum), a.offsets,
                     a.n_init, a.rows, a.G, a.k, a.max_n, a.kl, pl.runs_max, (const int*)a.active, a.H);
}

inline bool nm_args_ok(const nm_args& a) {
  return a.x && a.offsets && a.W && a.H && a.work && a.active && a.ld >= a.G && (a.dtype == 0 || a.dtype == 1) &&
         (a.kl == 0 || a.kl == 1) && nm_shape_ok(a.rows, a.G, a.k, a.S, a.n_init, a.max_n);
}

}  // namespace

extern "C" int64_t mcl_nmf_workspace_bytes(int64_t rows, int32_t G, int32_t k, int32_t S, int32_t n_init, int32_t max_n,
                                           int32_t loss) {
  if (!nm_shape_ok(rows, G, k, S, n_init, max_n) || !nm_limits_ok(rows, G, k, S, n_init) || (loss != 0 && loss != 1)) return -1;
  return nm_make_plan(rows, G, k, S, n_init, max_n, loss).total * 8;
}

extern "C" int mcl_nmf_check(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, int32_t* status,
                             mcl_stream_t stream) {
  if (!x || !status || rows < 1 || G < 1 || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (G > NM_MAX_G || rows > NM_MAX_CELLS) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  if (hipMemsetAsync(status, 0, 4, st) != hipSuccess) return (int)hipGetLastError();
  unsigned* word = reinterpret_cast<unsigned*>(status);
  const dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
  if (dtype == 0)
    hipLaunchKernelGGL(nm_check_kernel<float>, grid, block, 0, st, static_cast<const float*>(x), (long long)ld,
                       (long long)rows, G, word);
  else
    hipLaunchKernelGGL(nm_check_kernel<double>, grid, block, 0, st, static_cast<const double*>(x), (long long)ld,
                       (long long)rows, G, word);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_nmf_steps(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t n_init,
                             int64_t rows, int32_t G, int32_t k, int32_t max_n, int32_t loss, int32_t update_h, double* W,
                             double* H, double* work, int32_t* active, int32_t n_steps, mcl_stream_t stream) {
  const nm_args a = {x, (long long)ld, dtype, reinterpret_cast<const long long*>(offsets), S, n_init, (long long)rows, G, k,
                     max_n, loss, W, H, work, active};
  if (!nm_args_ok(a) || n_steps < 0 || (update_h != 0 && update_h != 1)) return MCL_EINVAL;
  if (!nm_limits_ok(rows, G, k, S, n_init)) return MCL_EUNSUPPORTED;
  const nm_plan pl = nm_make_plan(rows, G, k, S, n_init, max_n, loss);
  const hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  for (int i = 0; i < n_steps; ++i) {
    if (dtype == 0)
      nm_enqueue_step(a, static_cast<const float*>(x), update_h, i == 0, pl, st);
    else
      nm_enqueue_step(a, static_cast<const double*>(x), update_h, i == 0, pl, st);
    MCL_CHECK_LAUNCH();
  }
  return MCL_OK;
}

extern "C" int mcl_nmf_error(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t n_init,
                             int64_t rows, int32_t G, int32_t k, int32_t max_n, int32_t loss, const double* W,
                             const double* H, double* work, int32_t* active, int32_t phase, int32_t it, double tol,
                             int32_t max_iter, double* record, double* history, int32_t hist_len, mcl_stream_t stream) {
  const nm_args a = {x, (long long)ld, dtype, reinterpret_cast<const long long*>(offsets), S, n_init, (long long)rows, G, k,
                     max_n, loss, const_cast<double*>(W), const_cast<double*>(H), work, active};
  if (!nm_args_ok(a) || !record || phase < 0 || phase > 2 || it < 0 || max_iter < 0 || hist_len < 0 ||
      (hist_len > 0 && !history) || !(tol >= 0.0))
    return MCL_EINVAL;
  if (!nm_limits_ok(rows, G, k, S, n_init)) return MCL_EUNSUPPORTED;
  const nm_plan pl = nm_make_plan(rows, G, k, S, n_init, max_n, loss);
  const hipStream_t st = mcl_stream(stream);
  const int ignore = phase != 1;
  MCL_CLEAR_ERROR();
  if (dtype == 0)
    nm_launch_wh(a, static_cast<const float*>(x), ignore, pl, st);
  else
    nm_launch_wh(a, static_cast<const double*>(x), ignore, pl, st);
  if (loss) {
    nm_launch_axis_sum(a, 0, ignore, work + pl.hsum, st);
    nm_launch_axis_sum(a, 1, ignore, work + pl.wsum, st);
  }
  hipLaunchKernelGGL(nm_decide_kernel, dim3((unsigned)(S * n_init)), dim3(64), 0, st, (const double*)(work + pl.errp),
                     pl.tiles_max, a.offsets, n_init, (long long)rows, max_n, k, loss, (const double*)(work + pl.wsum),
                     (const double*)(work + pl.hsum), phase, it, tol, max_iter, active, record, history, hist_len);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_nmf_programs(const double* W, const double* H, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                                int32_t k, int32_t max_n, double* hsum, double* programs, double* usage, int32_t* dominant,
                                mcl_stream_t stream) {
  if (!W || !H || !offsets || !hsum || !programs || !usage || !dominant || !nm_shape_ok(rows, G, k, S, 1, max_n))
    return MCL_EINVAL;
  if (!nm_limits_ok(rows, G, k, S, 1)) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(nm_axis_sum_kernel, dim3((unsigned)S), dim3(1024), 0, st, H, 0, off, 1, (long long)rows, G, k, max_n,
                     (const int*)nullptr, 1, hsum);
  hipLaunchKernelGGL(nm_scale_h_kernel, dim3((unsigned)ceil_div(G, 256), (unsigned)k, (unsigned)S), dim3(256), 0, st, H,
                     (const double*)hsum, G, k, programs);
  hipLaunchKernelGGL(nm_usage_kernel, dim3((unsigned)ceil_div(max_n, 4), (unsigned)S), dim3(256), 0, st, W,
                     (const double*)hsum, off, (long long)rows, k, max_n, usage, dominant);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
