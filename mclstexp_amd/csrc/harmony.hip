// Harmony batch correction of expression matrices (BLEEP's preprocess.ipynb, last cell: harmonypy.run_harmony on the
// concatenated hvg_matrix.npy of the slides).  The arithmetic is the one DESIGN 6.9 states; cells are rows (Z is N x d),
// everything is fp64, no floating-point atomics, no kernel waits on another workgroup, and every summation order is a
// function of the shapes alone: two runs are bit-identical.
//
//   mcl_harmony_normalize     hm_normalize_kernel: row / row max, then / L2 norm (or the L2 norm alone); optional fp64 copy
//   mcl_harmony_centroids     hm_centroid_kernel: out (M x d) = A^T X over N on v_mfma_f64_16x16x4_f64, the A operand formed
//                             on load (R, R masked by batch -> the correction's M_k, or one-hot labels -> Lloyd sums); N is
//                             cut into fixed slices merged in slice order (hm_merge_kernel); optional row normalisation
//   mcl_harmony_dist          hm_dist_kernel: D = 2 (1 - Zc Y^T) (or the product itself), one wave = 16 cells x all centres
//   mcl_harmony_softmax       hm_softmax_kernel: exp(-D / sigma - row max), optionally / row sum
//   mcl_harmony_moments       hm_block_sums_kernel over all cells: E = (sum_n R) Pr, O = per-batch sums
//   mcl_harmony_update_block  per block: hm_block_sums_kernel (-), hm_block_cells_kernel, hm_block_sums_kernel (+)
//   mcl_harmony_objective     hm_objective_kernel + hm_objective_final_kernel: three doubles
//   mcl_harmony_ridge         hm_ridge_kernel: Gauss-Jordan with partial pivoting of the (B+1)^2 systems in LDS, W = A^-1 M
//   mcl_harmony_apply         hm_apply_kernel: Z_corr = Z - sum_k R[n,k] W[k, b(n)+1, :], MFMA, A masked by batch on load
//   mcl_harmony_lloyd         the hard k-means that seeds Y: gather, then (product, hm_label_kernel, one-hot sums,
//                             hm_lloyd_mean_kernel) per iteration, rows normalised at the end
//
// v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register q of lane l is
// D[(l >> 4) + 4 q][l & 15].  Tails follow DESIGN 4.0g (7): the address is clamped, the value masked at the use.
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int HM_MAX_K = 128;
constexpr int HM_MAX_B = 31;
constexpr int HM_MAX_D = 1 << 22;   // columns ride on grid.y (64 or 256 per workgroup)
constexpr int HM_SUM_THREADS = 128;

// batch[n] and order[i] come from the caller: an entry outside its range is read as the nearest valid one (clamp_index)

// ------------------------------------------------------------------------------------------------------- normalise
// one wave per row; lanes stride the columns, fixed butterfly
template <typename T>
__global__ __launch_bounds__(256) void hm_normalize_kernel(const T* z, long long ld, int N, int d,
                                                           int by_max, double* z64, double* zc) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const T* zr = z + (long long)n * ld;
  double mx = 1.0;
  if (by_max) {   // numpy's max: a NaN anywhere in the row makes the maximum NaN (fmax alone would drop it)
    mx = -INFINITY;
    bool nan = false;
    for (int j = lane; j < d; j += 64) {
      const double v = (double)zr[j];
      nan |= v != v;
      mx = fmax(mx, v);
    }
    mx = wave_max(mx);
    if (__any(nan)) mx = NAN;
  }
  double ss = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double v = (double)zr[j] / mx;
    ss = fma(v, v, ss);
  }
  ss = wave_sum(ss);
  const double nrm = sqrt(ss);
  for (int j = lane; j < d; j += 64) {
    const double x = (double)zr[j];
    if (z64) z64[(long long)n * d + j] = x;
    zc[(long long)n * d + j] = (x / mx) / nrm;
  }
}

// ------------------------------------------------------------------------------------------- centroids: A^T X over N
// MODE 0: A[m][n] = R[n][m] (M = K).  MODE 1: m = k G + g, A = R[n][k] [g == 0 or batch[n] == g - 1] (M = K G, G = B + 1).
// MODE 2: A = [labels[n] == m].
template <int MODE>
__device__ __forceinline__ double hm_a_operand(const double* __restrict__ R, int K, int nc, int k, int g, int bn,
                                               int ln) {
  if (MODE == 2) return ln == k ? 1.0 : 0.0;
  const double v = R[(long long)nc * K + k];
  if (MODE == 1) return (g == 0 || bn == g - 1) ? v : 0.0;
  return v;
}

// One workgroup = one 64 x 64 block of the output for one slice of N, one wave = a 32 x 32 quarter as 2 x 2 MFMA tiles.
template <int MODE>
__global__ __launch_bounds__(256) void hm_centroid_kernel(const double* __restrict__ R, const int* __restrict__ labels,
                                                          const double* __restrict__ X, const int* __restrict__ batch,
                                                          int N, int K, int d, int G, int slice_len,
                                                          double* __restrict__ out) {
  const int M = K * G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = blockIdx.y * 64 + (w >> 1) * 32, j0 = blockIdx.x * 64 + (w & 1) * 32;
  const int lm = lane & 15, lk = lane >> 4;
  const int n_lo = blockIdx.z * slice_len;
  const int n_hi = n_lo + slice_len < N ? n_lo + slice_len : N;
  const int m0 = i0 + lm, m1 = i0 + 16 + lm;
  const bool okm0 = m0 < M, okm1 = m1 < M;
  const int m0c = okm0 ? m0 : M - 1, m1c = okm1 ? m1 : M - 1;
  const int k0 = m0c / G, g0 = m0c % G, k1 = m1c / G, g1 = m1c % G;
  const int ja = j0 + lm, jb = j0 + 16 + lm;
  const int jac = ja < d ? ja : d - 1, jbc = jb < d ? jb : d - 1;
  f64x4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
#pragma unroll 2
  for (int nb = n_lo; nb < n_hi; nb += 4) {
    const int n = nb + lk;
    const bool okn = n < n_hi;
    const int nc = okn ? n : n_hi - 1;
    const int bn = MODE == 1 ? batch[nc] : 0;
    const int ln = MODE == 2 ? labels[nc] : 0;
    double a0 = hm_a_operand<MODE>(R, K, nc, k0, g0, bn, ln);
    double a1 = hm_a_operand<MODE>(R, K, nc, k1, g1, bn, ln);
    double b0 = X[(long long)nc * d + jac];
    double b1 = X[(long long)nc * d + jbc];
    a0 = (okn && okm0) ? a0 : 0.0;
    a1 = (okn && okm1) ? a1 : 0.0;
    b0 = okn ? b0 : 0.0;
    b1 = okn ? b1 : 0.0;
    acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
    acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
  }
  double* o = out + (long long)blockIdx.z * M * d;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int di = lk + 4 * q;
    const double v[2][2] = {{acc00[q], acc01[q]}, {acc10[q], acc11[q]}};
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const int i = i0 + 16 * ti + di, j = j0 + 16 * tj + lm;
        if (i < M && j < d) o[(long long)i * d + j] = v[ti][tj];
      }
  }
}

// out[e] = part[0][e] + part[1][e] + ... in slice order
__global__ __launch_bounds__(256) void hm_merge_kernel(const double* __restrict__ part, int slices, long long MD,
                                                       double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MD) return;
  double a = part[e];
  for (int s = 1; s < slices; ++s) a += part[(long long)s * MD + e];
  out[e] = a;
}

// ---------------------------------------------------------------------------------------------- D = 2 (1 - Zc Y^T)
// One wave = 16 cells x NKT tiles of 16 centres; the d loop takes 16 columns per step: slot lk of MFMA t4 holds column
// j0 + 4 lk + t4, so that the four lanes of a row read 128 contiguous bytes of it.
template <int NKT>
__global__ __launch_bounds__(64) void hm_dist_kernel(const double* __restrict__ Zc, const double* __restrict__ Y, int N,
                                                     int K, int d, int raw, double* __restrict__ D) {
  const int lane = threadIdx.x;
  const int lm = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.x * 16;
  const int n = i0 + lm;
  const double* zr = Zc + (long long)(n < N ? n : N - 1) * d;
  const double* yr[NKT];
  f64x4 acc[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int k = t * 16 + lm;
    yr[t] = Y + (long long)(k < K ? k : K - 1) * d;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  for (int j0 = 0; j0 < d; j0 += 16) {
    double a[4];
    int jc[4];
    bool ok[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int j = j0 + 4 * lk + t4;
      ok[t4] = j < d;
      jc[t4] = ok[t4] ? j : d - 1;
      const double v = zr[jc[t4]];
      a[t4] = ok[t4] ? v : 0.0;
    }
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {
        const double v = yr[t][jc[t4]];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t4], ok[t4] ? v : 0.0, acc[t], 0, 0, 0);
      }
  }
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = i0 + lk + 4 * q, col = t * 16 + lm;
      if (row < N && col < K) D[(long long)row * K + col] = raw ? acc[t][q] : 2.0 * (1.0 - acc[t][q]);
    }
}

// ------------------------------------------------------------------------------------------------------- soft-max
// one wave per cell, K <= 128: lane holds centres lane and lane + 64
__global__ __launch_bounds__(256) void hm_softmax_kernel(const double* __restrict__ D, int N, int K, double sigma,
                                                         int normalize, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const double* dr = D + (long long)n * K;
  const int ka = lane, kb = lane + 64;
  const double va = ka < K ? -dr[ka] / sigma : -INFINITY;
  const double vb = kb < K ? -dr[kb] / sigma : -INFINITY;
  const double mx = wave_max(fmax(va, vb));
  double ea = ka < K ? exp(va - mx) : 0.0, eb = kb < K ? exp(vb - mx) : 0.0;
  if (normalize) {
    const double s = wave_sum(ea + eb);
    ea /= s;
    eb /= s;
  }
  if (ka < K) out[(long long)n * K + ka] = ea;
  if (kb < K) out[(long long)n * K + kb] = eb;
}

// ------------------------------------------------------------------------------------------- block sums and E / O
// One workgroup per centre k: sums over the cells order[start .. start + len) (order NULL: the cells themselves) of R[n][k],
// in total and per batch, each thread over its strided cells in index order, then a fixed tree.  mode -1 / +1: E and O
// take the sums off / on; mode 0: they are set from them.
__global__ __launch_bounds__(HM_SUM_THREADS) void hm_block_sums_kernel(const double* __restrict__ R,
                                                                       const int* __restrict__ batch,
                                                                       const int* __restrict__ order, int start, int len,
                                                                       int N, int K, int B, const double* __restrict__ Pr,
                                                                       int mode, double* E, double* O) {
  __shared__ double sh[HM_MAX_B + 1][HM_SUM_THREADS];
  const int tid = threadIdx.x, k = blockIdx.x;
  for (int b = 0; b <= B; ++b) sh[b][tid] = 0.0;
  double tot = 0.0;
  for (int i = tid; i < len; i += HM_SUM_THREADS) {
    const int n = order ? clamp_index(order[start + i], N) : start + i;
    const double v = R[(long long)n * K + k];
    tot += v;
    sh[clamp_index(batch[n], B)][tid] += v;
  }
  sh[B][tid] = tot;
  __syncthreads();
  for (int h = HM_SUM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h)
      for (int b = 0; b <= B; ++b) sh[b][tid] += sh[b][tid + h];
    __syncthreads();
  }
  if (tid < B) {
    const double e = sh[B][0] * Pr[tid], o = sh[tid][0];
    const long long at = (long long)k * B + tid;
    if (mode == 0) {
      E[at] = e;
      O[at] = o;
    } else if (mode < 0) {
      E[at] -= e;
      O[at] -= o;
    } else {
      E[at] += e;
      O[at] += o;
    }
  }
}

// one wave per cell of the block: R[n][k] = S[n][k] ((E[k][b] + 1) / (O[k][b] + 1))^theta_b, row / its L1 norm
__global__ __launch_bounds__(256) void hm_block_cells_kernel(double* __restrict__ R, const double* __restrict__ S,
                                                             const int* __restrict__ batch,
                                                             const int* __restrict__ order, int start, int len, int N,
                                                             int K, int B, const double* __restrict__ theta,
                                                             const double* __restrict__ E, const double* __restrict__ O) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= len) return;
  const int n = clamp_index(order[start + i], N);
  const int b = clamp_index(batch[n], B);
  const double th = theta[b];
  const int ka = lane, kb = lane + 64;
  const int kac = ka < K ? ka : K - 1, kbc = kb < K ? kb : K - 1;
  double ra = S[(long long)n * K + kac] * pow((E[(long long)kac * B + b] + 1.0) / (O[(long long)kac * B + b] + 1.0), th);
  double rb = S[(long long)n * K + kbc] * pow((E[(long long)kbc * B + b] + 1.0) / (O[(long long)kbc * B + b] + 1.0), th);
  ra = ka < K ? ra : 0.0;
  rb = kb < K ? rb : 0.0;
  const double s = wave_sum(fabs(ra) + fabs(rb));
  if (ka < K) R[(long long)n * K + ka] = ra / s;
  if (kb < K) R[(long long)n * K + kb] = rb / s;
}

// ------------------------------------------------------------------------------------------------------ objective
// partial[wg][3]: a workgroup takes 64 cells, a wave 16 of them in order; lanes hold centres lane and lane + 64
__global__ __launch_bounds__(256) void hm_objective_kernel(const double* __restrict__ R, const double* __restrict__ D,
                                                           const int* __restrict__ batch, const double* __restrict__ E,
                                                           const double* __restrict__ O,
                                                           const double* __restrict__ theta, int N, int K, int B,
                                                           double* __restrict__ partial) {
  __shared__ double sh[4][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double t1 = 0.0, t2 = 0.0, t3 = 0.0;
  for (int r = 0; r < 16; ++r) {
    const int n = blockIdx.x * 64 + w * 16 + r;
    if (n >= N) break;
    const int b = clamp_index(batch[n], B);
    const double th = theta[b];
    for (int k = lane; k < K; k += 64) {
      const double rv = R[(long long)n * K + k];
      t1 = fma(rv, D[(long long)n * K + k], t1);
      const double x = rv * log(rv);
      t2 += isfinite(x) ? x : 0.0;
      t3 += rv * th * log((O[(long long)k * B + b] + 1.0) / (E[(long long)k * B + b] + 1.0));
    }
  }
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  t3 = wave_sum(t3);
  if (lane == 0) {
    sh[w][0] = t1;
    sh[w][1] = t2;
    sh[w][2] = t3;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    partial[(long long)blockIdx.x * 3 + c] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
  }
}

__global__ __launch_bounds__(256) void hm_objective_final_kernel(const double* __restrict__ partial, int nwg, double sigma,
                                                                 double* __restrict__ out3) {
  __shared__ double sh[3][256];
  const int tid = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < nwg; i += 256)
    for (int c = 0; c < 3; ++c) a[c] += partial[(long long)i * 3 + c];
  for (int c = 0; c < 3; ++c) sh[c][tid] = a[c];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
      for (int c = 0; c < 3; ++c) sh[c][tid] += sh[c][tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    out3[0] = sh[0][0];
    out3[1] = sigma * sh[1][0];
    out3[2] = sigma * sh[2][0];
  }
}

// ---------------------------------------------------------------------------------------------------------- ridge
// grid (K, column chunks of 256): every workgroup inverts A_k = arrow(O[k]) + diag(0, lambda) ((B+1)^2 <= 32^2) in LDS by
// Gauss-Jordan with partial pivoting (ties: the lowest row), then W[k][i][j] = sum_l inv[i][l] M[k][l][j], row 0 zeroed.
__global__ __launch_bounds__(256) void hm_ridge_kernel(const double* __restrict__ O, const double* __restrict__ M,
                                                       const double* __restrict__ lamb, int K, int B, int d,
                                                       double* __restrict__ W) {
  __shared__ double aug[HM_MAX_B + 1][2 * (HM_MAX_B + 1) + 1];
  __shared__ double fac[HM_MAX_B + 1];
  __shared__ int piv;
  const int tid = threadIdx.x, k = blockIdx.x;
  const int n1 = B + 1, n2 = 2 * n1;
  const double* ok = O + (long long)k * B;
  for (int e = tid; e < n1 * n2; e += 256) {
    const int r = e / n2, c = e % n2;
    double v = 0.0;
    if (c >= n1) {
      v = (c - n1 == r) ? 1.0 : 0.0;
    } else if (r == 0 && c == 0) {
      for (int b = 0; b < B; ++b) v += ok[b];
    } else if (r == 0) {
      v = ok[c - 1];
    } else if (c == 0) {
      v = ok[r - 1];
    } else if (r == c) {
      v = ok[r - 1] + lamb[r - 1];
    }
    aug[r][c] = v;
  }
  __syncthreads();
  for (int c = 0; c < n1; ++c) {
    if (tid == 0) {
      int p = c;
      double best = fabs(aug[c][c]);
      for (int r = c + 1; r < n1; ++r)
        if (fabs(aug[r][c]) > best) {
          best = fabs(aug[r][c]);
          p = r;
        }
      piv = p;
    }
    __syncthreads();
    const int p = piv;
    if (p != c && tid < n2) {
      const double t = aug[c][tid];
      aug[c][tid] = aug[p][tid];
      aug[p][tid] = t;
    }
    __syncthreads();
    const double pv = aug[c][c];
    if (tid < n1) fac[tid] = aug[tid][c];
    __syncthreads();
    if (tid < n2) aug[c][tid] /= pv;
    __syncthreads();
    for (int e = tid; e < n1 * n2; e += 256) {
      const int r = e / n2, t = e % n2;
      if (r != c) aug[r][t] -= fac[r] * aug[c][t];
    }
    __syncthreads();
  }
  const int j = blockIdx.y * 256 + tid;
  if (j >= d) return;
  const double* mk = M + (long long)k * n1 * d + j;
  double* wk = W + (long long)k * n1 * d + j;
  wk[0] = 0.0;
  for (int i = 1; i < n1; ++i) {
    double a = 0.0;
    for (int l = 0; l < n1; ++l) a = fma(aug[i][n1 + l], mk[(long long)l * d], a);
    wk[(long long)i * d] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------- apply
// One wave = 16 cells x 64 columns.  The reduction runs over (batch b, centre k): A[n][(b, k)] = R[n][k] [batch[n] == b],
// B[(b, k)][j] = W[k][b + 1][j]; a batch none of the wave's 16 cells belongs to adds exact zeros and is skipped.
__global__ __launch_bounds__(64) void hm_apply_kernel(const double* __restrict__ Z, const double* __restrict__ R,
                                                      const double* __restrict__ W, const int* __restrict__ batch, int N,
                                                      int K, int B, int d, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const int lm = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 64;   // cells on grid.x: no 65535 limit on N
  const int n = i0 + lm;
  const bool okn = n < N;
  const int nc = okn ? n : N - 1;
  const int bn = okn ? batch[nc] : -1;
  const double* rr = R + (long long)nc * K;
  int jc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + lm;
    jc[t] = j < d ? j : d - 1;
  }
  const int n1 = B + 1;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < B; ++b) {
    if (!__any(bn == b)) continue;   // wave-uniform
    for (int kb = 0; kb < K; kb += 4) {
      const int k = kb + lk;
      const bool okk = k < K;
      const int kc = okk ? k : K - 1;
      const double rv = rr[kc];
      const double a = (okk && bn == b) ? rv : 0.0;
      const double* wr = W + ((long long)kc * n1 + b + 1) * d;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double wv = wr[jc[t]];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, okk ? wv : 0.0, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = i0 + lk + 4 * q, col = j0 + 16 * t + lm;
      if (row < N && col < d) out[(long long)row * d + col] = Z[(long long)row * d + col] - acc[t][q];
    }
}

// ---------------------------------------------------------------------------------------------------------- Lloyd
__global__ __launch_bounds__(256) void hm_gather_kernel(const double* __restrict__ Zc, const int* __restrict__ rows, int N,
                                                        int d, double* __restrict__ Y) {
  int r = rows[blockIdx.x];
  r = r < 0 ? 0 : (r >= N ? N - 1 : r);
  for (int j = threadIdx.x; j < d; j += 256) Y[(long long)blockIdx.x * d + j] = Zc[(long long)r * d + j];
}

// label = the centre of largest product (ties: the lowest centre); one wave per cell
__global__ __launch_bounds__(256) void hm_label_kernel(const double* __restrict__ P, int N, int K, int* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double best = -INFINITY;
  int idx = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const double v = P[(long long)n * K + k];
    if (v > best) {
      best = v;
      idx = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) {
      best = ov;
      idx = oi;
    }
  }
  if (lane == 0) labels[n] = idx < K ? idx : 0;
}

// Y[k] = sums[k] / count(labels == k); an emptied centre keeps its row
__global__ __launch_bounds__(256) void hm_lloyd_mean_kernel(const double* __restrict__ sums, const int* __restrict__ labels,
                                                            int N, int d, double* __restrict__ Y) {
  __shared__ int cnt;
  const int k = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  __syncthreads();
  int c = 0;
  for (int n = tid; n < N; n += 256) c += labels[n] == k;
  atomicAdd(&cnt, c);   // integer: exact in any order
  __syncthreads();
  const int total = cnt;
  if (total == 0) return;
  for (int j = tid; j < d; j += 256) Y[(long long)k * d + j] = sums[(long long)k * d + j] / (double)total;
}

// ------------------------------------------------------------------------------------------------------ host side
// the cut of N for an M x d output: a function of the shapes alone
inline void hm_slices(int N, int M, int d, int* slices, int* slice_len) {
  const long long tiles = (long long)ceil_div(M, 64) * ceil_div(d, 64);
  long long want = (1024 + tiles - 1) / tiles;
  const long long most = ceil_div(N, 256);
  if (want > most) want = most;
  if (want < 1) want = 1;
  int len = ceil_div(N, want);
  len = (len + 3) / 4 * 4;
  *slice_len = len;
  *slices = ceil_div(N, len);
}

inline int hm_limits(long long N, int K, int B) {
  if (K > HM_MAX_K || B > HM_MAX_B || N * (long long)K >= (1ll << 31)) return MCL_EUNSUPPORTED;
  return MCL_OK;
}

template <int MODE>
int hm_centroids_launch(const double* R, const int* labels, const double* X, const int* batch, int N, int K, int d, int G,
                        double* work, double* out, hipStream_t st) {
  const int M = K * G;
  int slices, len;
  hm_slices(N, M, d, &slices, &len);
  double* dst = slices == 1 ? out : work;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_centroid_kernel<MODE>, dim3(ceil_div(d, 64), ceil_div(M, 64), slices), dim3(256), 0, st, R, labels, X,
                     batch, N, K, d, G, len, dst);
  MCL_CHECK_LAUNCH();
  if (slices > 1) {
    const long long MD = (long long)M * d;
    hipLaunchKernelGGL(hm_merge_kernel, dim3(ceil_div(MD, 256)), dim3(256), 0, st, work, slices, MD, out);
    MCL_CHECK_LAUNCH();
  }
  return MCL_OK;
}

int hm_normalize_launch(const void* z, long long ld, int dtype, int N, int d, int by_max, double* z64, double* zc,
                        hipStream_t st) {
  MCL_CLEAR_ERROR();
  if (dtype == 0)
    hipLaunchKernelGGL(hm_normalize_kernel<float>, dim3(ceil_div(N, 4)), dim3(256), 0, st, (const float*)z, ld, N, d, by_max,
                       z64, zc);
  else
    hipLaunchKernelGGL(hm_normalize_kernel<double>, dim3(ceil_div(N, 4)), dim3(256), 0, st, (const double*)z, ld, N, d,
                       by_max, z64, zc);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int hm_dist_launch(const double* Zc, const double* Y, int N, int K, int d, int raw, double* D, hipStream_t st) {
  MCL_CLEAR_ERROR();
  const dim3 grid(ceil_div(N, 16)), block(64);
  switch (ceil_div(K, 16)) {
#define HM_DIST_CASE(T) \
  case T: hipLaunchKernelGGL(hm_dist_kernel<T>, grid, block, 0, st, Zc, Y, N, K, d, raw, D); break;
    HM_DIST_CASE(1) HM_DIST_CASE(2) HM_DIST_CASE(3) HM_DIST_CASE(4) HM_DIST_CASE(5) HM_DIST_CASE(6) HM_DIST_CASE(7)
    HM_DIST_CASE(8)
#undef HM_DIST_CASE
    default: return MCL_EUNSUPPORTED;
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // namespace

extern "C" {

int64_t mcl_harmony_workspace_doubles(int32_t N, int32_t K, int32_t d, int32_t B) {
  if (N <= 0 || K <= 0 || d <= 0 || B <= 0) return 0;
  long long most = 0;
  for (int G : {1, B + 1}) {
    int slices, len;
    hm_slices(N, K * G, d, &slices, &len);
    const long long need = slices > 1 ? (long long)slices * K * G * d : 0;
    if (need > most) most = need;
  }
  const long long obj = 3ll * ceil_div(N, 64);
  return most > obj ? most : obj;
}

int mcl_harmony_normalize(const void* z, int64_t ld, int32_t dtype, int32_t N, int32_t d, int32_t divide_by_max,
                          double* z64, double* zc, mcl_stream_t stream) {
  if (!z || !zc || N <= 0 || d <= 0 || ld < d || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  return hm_normalize_launch(z, ld, dtype, N, d, divide_by_max, z64, zc, mcl_stream(stream));
}

int mcl_harmony_centroids(const double* R, const double* X, const int32_t* batch, int32_t N, int32_t K, int32_t d,
                          int32_t B, int32_t normalize, double* work, double* out, mcl_stream_t stream) {
  if (!R || !X || !work || !out || N <= 0 || K <= 0 || d <= 0 || B < 0 || (B > 0 && !batch)) return MCL_EINVAL;
  if (hm_limits(N, K, B) != MCL_OK) return MCL_EUNSUPPORTED;
  hipStream_t st = mcl_stream(stream);
  const int rc = B > 0 ? hm_centroids_launch<1>(R, nullptr, X, batch, N, K, d, B + 1, work, out, st)
                       : hm_centroids_launch<0>(R, nullptr, X, nullptr, N, K, d, 1, work, out, st);
  if (rc != MCL_OK || !normalize) return rc;
  return hm_normalize_launch(out, d, 1, K * (B > 0 ? B + 1 : 1), d, 0, nullptr, out, st);
}

int mcl_harmony_dist(const double* Zc, const double* Y, int32_t N, int32_t K, int32_t d, int32_t raw, double* D,
                     mcl_stream_t stream) {
  if (!Zc || !Y || !D || N <= 0 || K <= 0 || d <= 0) return MCL_EINVAL;
  if (hm_limits(N, K, 0) != MCL_OK) return MCL_EUNSUPPORTED;
  return hm_dist_launch(Zc, Y, N, K, d, raw, D, mcl_stream(stream));
}

int mcl_harmony_softmax(const double* D, int32_t N, int32_t K, double sigma, int32_t normalize, double* out,
                        mcl_stream_t stream) {
  if (!D || !out || N <= 0 || K <= 0 || !(sigma > 0.0)) return MCL_EINVAL;
  if (hm_limits(N, K, 0) != MCL_OK) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_softmax_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, mcl_stream(stream), D, N, K, sigma, normalize,
                     out);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_harmony_moments(const double* R, const int32_t* batch, int32_t N, int32_t K, int32_t B, const double* Pr, double* E,
                        double* O, mcl_stream_t stream) {
  if (!R || !batch || !Pr || !E || !O || N <= 0 || K <= 0 || B <= 0) return MCL_EINVAL;
  if (hm_limits(N, K, B) != MCL_OK) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_block_sums_kernel, dim3(K), dim3(HM_SUM_THREADS), 0, mcl_stream(stream), R, batch,
                     (const int*)nullptr, 0, N, N, K, B, Pr, 0, E, O);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_harmony_update_block(double* R, const double* S, const int32_t* batch, const int32_t* order, int32_t N, int32_t K,
                             int32_t B, int32_t n_blocks, int32_t block_lo, int32_t block_hi, const double* theta,
                             const double* Pr, double* E, double* O, mcl_stream_t stream) {
  if (!R || !S || !batch || !order || !theta || !Pr || !E || !O || N <= 0 || K <= 0 || B <= 0 || n_blocks <= 0 ||
      n_blocks > N || block_lo < 0 || block_hi > n_blocks || block_lo > block_hi)
    return MCL_EINVAL;
  if (hm_limits(N, K, B) != MCL_OK) return MCL_EUNSUPPORTED;
  hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  const int base = N / n_blocks, extra = N % n_blocks;   // numpy.array_split: the first `extra` blocks hold one more
  for (int blk = block_lo; blk < block_hi; ++blk) {
    const int start = blk * base + (blk < extra ? blk : extra);
    const int len = base + (blk < extra ? 1 : 0);
    hipLaunchKernelGGL(hm_block_sums_kernel, dim3(K), dim3(HM_SUM_THREADS), 0, st, R, batch, order, start, len, N, K, B, Pr, -1,
                       E, O);
    hipLaunchKernelGGL(hm_block_cells_kernel, dim3(ceil_div(len, 4)), dim3(256), 0, st, R, S, batch, order, start, len, N, K, B,
                       theta, E, O);
    hipLaunchKernelGGL(hm_block_sums_kernel, dim3(K), dim3(HM_SUM_THREADS), 0, st, R, batch, order, start, len, N, K, B, Pr, 1,
                       E, O);
    MCL_CHECK_LAUNCH();
  }
  return MCL_OK;
}

int mcl_harmony_objective(const double* R, const double* D, const int32_t* batch, const double* E, const double* O,
                          const double* theta, int32_t N, int32_t K, int32_t B, double sigma, double* work, double* out3,
                          mcl_stream_t stream) {
  if (!R || !D || !batch || !E || !O || !theta || !work || !out3 || N <= 0 || K <= 0 || B <= 0) return MCL_EINVAL;
  if (hm_limits(N, K, B) != MCL_OK) return MCL_EUNSUPPORTED;
  hipStream_t st = mcl_stream(stream);
  const int nwg = ceil_div(N, 64);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_objective_kernel, dim3(nwg), dim3(256), 0, st, R, D, batch, E, O, theta, N, K, B, work);
  hipLaunchKernelGGL(hm_objective_final_kernel, dim3(1), dim3(256), 0, st, work, nwg, sigma, out3);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_harmony_ridge(const double* O, const double* M, const double* lamb, int32_t K, int32_t B, int32_t d, double* W,
                      mcl_stream_t stream) {
  if (!O || !M || !lamb || !W || K <= 0 || B <= 0 || d <= 0) return MCL_EINVAL;
  if (hm_limits(1, K, B) != MCL_OK || d > HM_MAX_D) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_ridge_kernel, dim3(K, ceil_div(d, 256)), dim3(256), 0, mcl_stream(stream), O, M, lamb, K, B, d, W);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_harmony_apply(const double* Z, const double* R, const double* W, const int32_t* batch, int32_t N, int32_t K,
                      int32_t B, int32_t d, double* out, mcl_stream_t stream) {
  if (!Z || !R || !W || !batch || !out || N <= 0 || K <= 0 || B <= 0 || d <= 0) return MCL_EINVAL;
  if (hm_limits(N, K, B) != MCL_OK || d > HM_MAX_D) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_apply_kernel, dim3(ceil_div(N, 16), ceil_div(d, 64)), dim3(64), 0, mcl_stream(stream), Z, R, W, batch, N,
                     K, B, d, out);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_harmony_lloyd(const double* Zc, int32_t N, int32_t K, int32_t d, const int32_t* seed_rows, int32_t iters,
                      int32_t* labels, double* products, double* sums, double* work, double* Y, mcl_stream_t stream) {
  if (!Zc || !seed_rows || !labels || !products || !sums || !work || !Y || N <= 0 || K <= 0 || d <= 0 || iters < 0 || K > N)
    return MCL_EINVAL;
  if (hm_limits(N, K, 0) != MCL_OK) return MCL_EUNSUPPORTED;
  hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hm_gather_kernel, dim3(K), dim3(256), 0, st, Zc, seed_rows, N, d, Y);
  MCL_CHECK_LAUNCH();
  for (int it = 0; it < iters; ++it) {
    int rc = hm_dist_launch(Zc, Y, N, K, d, 1, products, st);
    if (rc != MCL_OK) return rc;
    hipLaunchKernelGGL(hm_label_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, st, products, N, K, labels);
    MCL_CHECK_LAUNCH();
    rc = hm_centroids_launch<2>(nullptr, labels, Zc, nullptr, N, K, d, 1, work, sums, st);
    if (rc != MCL_OK) return rc;
    hipLaunchKernelGGL(hm_lloyd_mean_kernel, dim3(K), dim3(256), 0, st, sums, labels, N, d, Y);
    MCL_CHECK_LAUNCH();
  }
  return hm_normalize_launch(Y, d, 1, K, d, 0, nullptr, Y, st);
}

}  // extern "C"
