// Spatial-domain clustering of predicted expression (the reference's cluster(), /root/reference/utils.py:67-79, the last
// number of its tutorial): PCA -> k-means -> ARI / NMI against the pathologist's labels, for S slides (row segments) per call.
// Everything is fp64, floating-point sums are atomics-free and every reduction order depends only on the segment's own
// shape, so a slide computed inside a batch is bit-identical to the same slide computed alone.
//
//   mcl_pca_gram        pca_mean_kernel (column means) + pca_gram_kernel: the centred Gram matrix in its smaller form,
//                       Xc^T Xc (G x G) when n_s >= G ("primal"), else Xc Xc^T (n_s x n_s) ("dual"), on
//                       v_mfma_f64_16x16x4_f64; the lower triangle of 64x64 blocks is computed and mirrored.
//   (host, or device)   the leading eigenpairs of that one symmetric matrix per segment: numpy.linalg.eigh on the host by
//                       default, mcl_sym_eig_top (csrc/eig.hip) on request -- then the Gram matrices stay on the device.
//   mcl_pca_project     pca_loadings_kernel + pca_sign_kernel + pca_scores_kernel: the scores Xc V (primal) or U sqrt(lambda)
//                       (dual), each component's sign fixed so that its loading of largest magnitude is positive.
//   mcl_kmeans          kmeans_kernel, grid (restart, segment): one workgroup runs one whole Lloyd problem (seeding, the
//                       iteration, the final assignment, the inertia) inside one launch; kmeans_select_kernel keeps the
//                       restart of lowest inertia per segment.
//   mcl_cluster_scores  cluster_scores_kernel: contingency table in LDS, ARI (pair-confusion form) and NMI (arithmetic).
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int KM_THREADS = 256;
constexpr int KM_MAX = 64;          // D <= 64, K <= 64
constexpr int CS_THREADS = 256;
constexpr int CS_VALUES = 1024;     // label values in [0, 1024)
constexpr int CS_TABLE = 12288;     // distinct(a) * distinct(b) entries of the contingency table held in LDS

// ------------------------------------------------------------------------------------------------------------- PCA
// column means: lane = column, the four waves stride over the segment's rows, combined wave 0 + 1 + 2 + 3
template <typename T>
__global__ __launch_bounds__(256) void pca_mean_kernel(const T* __restrict__ x, long long ld,
                                                       const long long* __restrict__ offsets, int G,
                                                       double* __restrict__ mean) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int g = blockIdx.x * 64 + lane;
  const int gc = g < G ? g : G - 1;
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  double a = 0.0;
  for (long long r = r0 + w; r < r1; r += 4) a += ldd(x + r * ld + gc);
  part[w][lane] = a;
  __syncthreads();
  if (w == 0 && g < G) {
    a = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    mean[(long long)s * G + g] = a / (double)(r1 - r0);
  }
}

// element (k, m) of the centred operand: primal (n_s >= G) k = row, m = column; dual k = column, m = row.  Indices past
// the matrix read a clamped address and count as zero.
template <typename T>
__device__ __forceinline__ double gram_operand(const T* __restrict__ xs, long long ld, const double* __restrict__ mu,
                                               bool primal, int k, int m, int K, int M) {
  const bool ok = k < K && m < M;
  const int kc = k < K ? k : K - 1, mc = m < M ? m : M - 1;
  const int row = primal ? kc : mc, col = primal ? mc : kc;
  const double v = ldd(xs + (long long)row * ld + col) - mu[col];
  return ok ? v : 0.0;
}

// One workgroup = one 64x64 block (bi >= bj) of the segment's M x M Gram matrix, one wave = one 32x32 quarter of it as
// 2 x 2 MFMA tiles; the K loop runs in index order, so the sums do not depend on the launch.
// v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register q of lane l is
// D[(l >> 4) + 4 q][l & 15]  (not the layout of the other MFMA shapes).
template <typename T>
__global__ __launch_bounds__(256) void pca_gram_kernel(const T* __restrict__ x, long long ld,
                                                       const long long* __restrict__ offsets, int G,
                                                       const double* __restrict__ mean,
                                                       const long long* __restrict__ gram_offsets,
                                                       double* __restrict__ gram) {
  const int s = blockIdx.z;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const bool primal = n >= G;
  const int M = primal ? G : n, K = primal ? n : G;
  if (bi * 64 >= M) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = bi * 64 + (w >> 1) * 32, j0 = bj * 64 + (w & 1) * 32;
  const int lm = lane & 15, lk = lane >> 4;
  const T* xs = x + r0 * ld;
  const double* mu = mean + (long long)s * G;
  f64x4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + lk;
    const double a0 = gram_operand(xs, ld, mu, primal, k, i0 + lm, K, M);
    const double a1 = gram_operand(xs, ld, mu, primal, k, i0 + 16 + lm, K, M);
    const double b0 = gram_operand(xs, ld, mu, primal, k, j0 + lm, K, M);
    const double b1 = gram_operand(xs, ld, mu, primal, k, j0 + 16 + lm, K, M);
    acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
    acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
  }
  double* out = gram + gram_offsets[s];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int di = lk + 4 * q;
    const double v[2][2] = {{acc00[q], acc01[q]}, {acc10[q], acc11[q]}};
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const int i = i0 + 16 * ti + di, j = j0 + 16 * tj + lm;
        if (i < M && j <= i) {   // the lower triangle, mirrored: the output is exactly symmetric
          out[(long long)i * M + j] = v[ti][tj];
          out[(long long)j * M + i] = v[ti][tj];
        }
      }
  }
}

// loadings (G, C) per segment, up to a positive factor per component: primal V itself, dual Xc^T U
template <typename T>
__global__ __launch_bounds__(256) void pca_loadings_kernel(const T* __restrict__ x, long long ld,
                                                           const long long* __restrict__ offsets, int G, int C,
                                                           const double* __restrict__ mean,
                                                           const double* __restrict__ evec,
                                                           const long long* __restrict__ evec_offsets,
                                                           double* __restrict__ loadings) {
  const int s = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const double* V = evec + evec_offsets[s];
  double* L = loadings + (long long)s * G * C;
  if (n >= G) {
    for (int c = 0; c < C; ++c) L[(long long)g * C + c] = V[(long long)g * C + c];
    return;
  }
  const double mu = mean[(long long)s * G + g];
  const T* xc = x + r0 * ld + g;
  for (int c = 0; c < C; ++c) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) a = fma(ldd(xc + (long long)i * ld) - mu, V[(long long)i * C + c], a);
    L[(long long)g * C + c] = a;
  }
}

// sign[s][c] = +-1 so that the loading of largest magnitude (ties: the lowest gene) becomes positive
__global__ __launch_bounds__(256) void pca_sign_kernel(const double* __restrict__ loadings, int G, int C,
                                                       double* __restrict__ sign) {
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double* L = loadings + (long long)s * G * C;
  for (int c = 0; c < C; ++c) {
    double best = -1.0;
    int idx = 0x7fffffff;
    for (int g = tid; g < G; g += 256) {
      const double a = fabs(L[(long long)g * C + c]);
      if (a > best) { best = a; idx = g; }
    }
    bv[tid] = best; bi[tid] = idx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) {
        const double ov = bv[tid + h];
        const int oi = bi[tid + h];
        if (ov > bv[tid] || (ov == bv[tid] && oi < bi[tid])) { bv[tid] = ov; bi[tid] = oi; }
      }
      __syncthreads();
    }
    const int top = bi[0] < G ? bi[0] : 0;   // (no finite loading at all: row 0)
    if (tid == 0) sign[(long long)s * C + c] = L[(long long)top * C + c] < 0.0 ? -1.0 : 1.0;
    __syncthreads();
  }
}

// one wave per row: primal z[i][c] = sign_c sum_g (x[i][g] - mean[g]) V[g][c] (lanes stride the genes, fixed butterfly);
// dual z[i][c] = sign_c sqrt(lambda_c) U[i][c]
template <typename T>
__global__ __launch_bounds__(256) void pca_scores_kernel(const T* __restrict__ x, long long ld,
                                                         const long long* __restrict__ offsets, int G, int C,
                                                         const double* __restrict__ mean, const double* __restrict__ evec,
                                                         const long long* __restrict__ evec_offsets,
                                                         const double* __restrict__ eval, const double* __restrict__ sign,
                                                         double* __restrict__ z) {
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const int i = blockIdx.x * 4 + w;
  if (i >= n) return;
  const double* V = evec + evec_offsets[s];
  const double* sg = sign + (long long)s * C;
  double* zr = z + (r0 + i) * C;
  if (n < G) {
    if (lane < C) zr[lane] = sg[lane] * sqrt(fmax(eval[(long long)s * C + lane], 0.0)) * V[(long long)i * C + lane];
    return;
  }
  const T* xr = x + (r0 + i) * ld;
  const double* mu = mean + (long long)s * G;
  for (int c = 0; c < C; ++c) {
    double a = 0.0;
    for (int g = lane; g < G; g += 64) a = fma(ldd(xr + g) - mu[g], V[(long long)g * C + c], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);   // wave_sum(a) written out: a call changes this kernel's code
    if (lane == 0) zr[c] = sg[c] * a;
  }
}

// ----------------------------------------------------------------------------------------------------------- k-means
// the counter-based generator of csrc/step_misc.hip's dropout (mix64), keyed by (seed, segment, restart, draw)
__device__ __forceinline__ double km_uniform(unsigned long long seed, int seg, int r, int draw) {
  unsigned long long h = mix64(seed ^ mix64((unsigned long long)(unsigned)seg));
  h = mix64(h ^ (unsigned long long)(unsigned)r);
  h = mix64(h ^ (unsigned long long)(unsigned)draw);
  return (double)(h >> 32) * (1.0 / 4294967296.0);   // 32 random bits: u * total < total also after rounding
}

__device__ __forceinline__ double km_sqdist(const double* __restrict__ p, const double* c, int D) {
  double a = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = p[d] - c[d];
    a = fma(t, t, a);
  }
  return a;
}

// sum of one value per thread in a fixed tree; every thread gets the result
__device__ __forceinline__ double km_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

struct KmShared {
  double cen[KM_MAX * KM_MAX];   // centres (K, D)
  double red[KM_THREADS];        // partials of the fixed-order reductions
  int redi[KM_THREADS];
  int cnt[KM_MAX];
  int moved_row[KM_MAX];         // relocation of emptied clusters: the row that moved and the label it had
  int moved_old[KM_MAX];
  int pick;
  double pick_base, pick_target;
};

// nearest centre of every point (ties: lowest centre), its squared distance into dist[], counts by LDS integer atomics;
// returns whether any label changed (block-wide)
__device__ __forceinline__ int km_assign(KmShared& sh, const double* __restrict__ zs, long long ld, int n, int D, int K,
                                         int* lab, double* dist) {
  const int tid = threadIdx.x;
  if (tid < KM_MAX) sh.cnt[tid] = 0;
  __syncthreads();
  int changed = 0;
  for (int i = tid; i < n; i += KM_THREADS) {
    const double* p = zs + (long long)i * ld;
    double best = km_sqdist(p, sh.cen, D);
    int bk = 0;
    for (int k = 1; k < K; ++k) {
      const double d2 = km_sqdist(p, sh.cen + k * D, D);
      if (d2 < best) { best = d2; bk = k; }
    }
    changed |= lab[i] != bk;
    lab[i] = bk;
    dist[i] = best;
    atomicAdd(&sh.cnt[bk], 1);
  }
  return __syncthreads_or(changed);
}

// the row of largest dist[] (ties: lowest row), for every thread
__device__ __forceinline__ int km_argmax(KmShared& sh, const double* dist, int n) {
  const int tid = threadIdx.x;
  double best = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = tid; i < n; i += KM_THREADS) {
    const double v = dist[i];
    if (v > best) { best = v; idx = i; }
  }
  __syncthreads();
  sh.red[tid] = best; sh.redi[tid] = idx;
  __syncthreads();
  for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double ov = sh.red[tid + h];
      const int oi = sh.redi[tid + h];
      if (ov > sh.red[tid] || (ov == sh.red[tid] && oi < sh.redi[tid])) { sh.red[tid] = ov; sh.redi[tid] = oi; }
    }
    __syncthreads();
  }
  const int r = sh.redi[0] < n ? sh.redi[0] : 0;   // (nothing comparable, NaN input: row 0)
  __syncthreads();
  return r;
}

// sum over the rows [lo, hi) of column d of the points whose label is k (k < 0: every point; sq: squared deviation from mu)
__device__ __forceinline__ double km_colsum(const double* __restrict__ zs, long long ld, const int* lab, int lo,
                                            int hi, int d, int k, bool sq, double mu) {
  double a = 0.0;
  for (int i = lo; i < hi; ++i) {
    double v = zs[(long long)i * ld + d];
    if (sq) v = (v - mu) * (v - mu);
    a += (k < 0 || lab[i] == k) ? v : 0.0;
  }
  return a;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int D, const int* __restrict__ ks,
    int k_max, int R, const long long* __restrict__ seeds, unsigned long long seed, int seg_base, double tol, int max_iter,
    long long rows, long long* __restrict__ seeds_out, int* labels_all, double* __restrict__ centers_all,
    double* __restrict__ inertia_all, int* __restrict__ n_iter_all, double* work) {
  __shared__ KmShared sh;
  const int tid = threadIdx.x;
  const int r = blockIdx.x, s = blockIdx.y;
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const int K = ks[s];
  const long long sr = (long long)s * R + r;
  int* lab = labels_all + (long long)r * rows + r0;
  double* dist = work + (long long)r * rows + r0;
  double* cen_out = centers_all + sr * k_max * D;
  long long* sd_out = seeds_out + sr * k_max;
  if (K < 1 || K > k_max || K > n) {   // not a k-means problem: flagged, never selected over a valid restart
    if (tid == 0) { inertia_all[sr] = NAN; n_iter_all[sr] = -1; }
    for (int i = tid; i < n; i += KM_THREADS) lab[i] = -1;
    return;
  }
  const double* zs = z + r0 * ld;
  const int KD = K * D;
  // (column, chunk) and (centre, column, chunk) reductions: P chunks of rows per sum, merged in chunk order
  const int Pd = KM_THREADS / D, lend = (n + Pd - 1) / Pd;

  // ---- tol scaled by the mean per-column variance (sklearn's _tolerance): two passes, fixed order
  double tol_abs;
  {
    const int d = tid % D, c = tid / D;
    const bool act = c < Pd;
    const int lo = min(n, c * lend), hi = min(n, lo + lend);
    __syncthreads();
    sh.red[tid] = act ? km_colsum(zs, ld, lab, lo, hi, d, -1, false, 0.0) : 0.0;
    __syncthreads();
    double mu = 0.0;
    for (int q = 0; q < Pd; ++q) mu += sh.red[q * D + d];
    mu /= (double)n;
    __syncthreads();
    sh.red[tid] = act ? km_colsum(zs, ld, lab, lo, hi, d, -1, true, mu) : 0.0;
    __syncthreads();
    double var = 0.0;
    if (tid < D) {
      for (int q = 0; q < Pd; ++q) var += sh.red[q * D + tid];
      var /= (double)n;
    }
    tol_abs = tol * (km_block_sum(tid < D ? var : 0.0, sh.red) / (double)D);
  }

  // ---- seeding
  for (int i = tid; i < n; i += KM_THREADS) lab[i] = -1;
  if (seeds != nullptr) {
    for (int e = tid; e < KD; e += KM_THREADS) {
      const int k = e / D, d = e - k * D;
      long long row = seeds[sr * k_max + k];
      row = row < 0 ? 0 : (row >= n ? n - 1 : row);
      sh.cen[e] = zs[row * ld + d];
      if (d == 0) sd_out[k] = row;
    }
    __syncthreads();
  } else {
    // k-means++ (one candidate per centre): the first centre uniform, each next one sampled with probability
    // proportional to the squared distance to the nearest centre so far, through a fixed-order prefix sum
    const int lenp = (n + KM_THREADS - 1) / KM_THREADS;
    const int plo = min(n, tid * lenp), phi = min(n, plo + lenp);
    for (int j = 0; j < K; ++j) {
      const double u = km_uniform(seed, seg_base + s, r, j);
      int row;
      if (j == 0) {
        row = min(n - 1, (int)(u * (double)n));
      } else {
        double cs = 0.0;
        for (int i = plo; i < phi; ++i) cs += dist[i];
        __syncthreads();
        sh.red[tid] = cs;
        __syncthreads();
        if (tid == 0) {
          double total = 0.0;
          for (int t = 0; t < KM_THREADS; ++t) total += sh.red[t];
          const double target = u * total;
          double base = 0.0, last_base = 0.0;
          int pick = -1, last = -1;
          for (int t = 0; t < KM_THREADS; ++t) {
            const double v = sh.red[t];
            if (v > 0.0) {
              last = t;
              last_base = base;
              if (base + v > target) { pick = t; break; }
            }
            base += v;
          }
          if (pick < 0) { pick = last; base = last_base; }   // rounding at the far end: the last chunk with mass
          sh.pick = pick;                                     // (-1: every point coincides with a centre)
          sh.pick_base = base;
          sh.pick_target = target;
          sh.redi[0] = min(n - 1, (int)(u * (double)n));
        }
        __syncthreads();
        if (tid == sh.pick) {   // the chunk's owner repeats its own sum: the same order, so the crossing lies inside
          double run = 0.0;
          int found = -1, lastm = plo;
          for (int i = plo; i < phi; ++i) {
            const double v = dist[i];
            run += v;
            if (v > 0.0) {
              lastm = i;
              if (sh.pick_base + run > sh.pick_target) { found = i; break; }
            }
          }
          sh.redi[0] = found >= 0 ? found : lastm;
        }
        __syncthreads();
        row = sh.redi[0];
        __syncthreads();
      }
      if (tid < D) sh.cen[j * D + tid] = zs[(long long)row * ld + tid];
      if (tid == 0) sd_out[j] = row;
      __syncthreads();
      for (int i = tid; i < n; i += KM_THREADS) {
        const double d2 = km_sqdist(zs + (long long)i * ld, sh.cen + j * D, D);
        dist[i] = j == 0 ? d2 : fmin(dist[i], d2);
      }
      __syncthreads();
    }
  }

  // ---- Lloyd (sklearn's algorithm="lloyd"): assign, update, stop on unchanged labels or a small centre shift
  const int Pk = KD <= KM_THREADS / 2 ? KM_THREADS / KD : 1;
  const int lenk = (n + Pk - 1) / Pk;
  int it = 0;
  bool strict = false;
  while (it < max_iter) {
    const int changed = km_assign(sh, zs, ld, n, D, K, lab, dist);
    // emptied clusters take, in turn, the point farthest from its own centre (ties: lowest row)
    int n_moved = 0;
    for (int k = 0; k < K; ++k) {
      if (sh.cnt[k] != 0) continue;   // LDS value, the same for every thread
      const int f = km_argmax(sh, dist, n);
      if (tid == 0) {
        const int o = lab[f];
        sh.moved_row[n_moved] = f;
        sh.moved_old[n_moved] = o;
        lab[f] = k;
        dist[f] = -1.0;
        sh.cnt[k] = 1;
        sh.cnt[o] -= 1;
      }
      ++n_moved;
      __syncthreads();
    }
    // per-centre column sums -> means, in place; the squared shift of every coordinate summed in a fixed tree
    double shift = 0.0;
    if (Pk > 1) {
      const int e = tid % KD, c = tid / KD;
      const int k = e / D, d = e - k * D;
      const int lo = min(n, c * lenk), hi = min(n, lo + lenk);
      sh.red[tid] = c < Pk ? km_colsum(zs, ld, lab, lo, hi, d, k, false, 0.0) : 0.0;
      __syncthreads();
      if (tid < KD) {
        double a = 0.0;
        for (int q = 0; q < Pk; ++q) a += sh.red[q * KD + tid];
        if (sh.cnt[k] > 0) {
          const double v = a * (1.0 / (double)sh.cnt[k]);
          const double df = v - sh.cen[tid];
          sh.cen[tid] = v;
          shift = df * df;
        }
      }
    } else {
      for (int e = tid; e < KD; e += KM_THREADS) {
        const int k = e / D, d = e - k * D;
        const double a = km_colsum(zs, ld, lab, 0, n, d, k, false, 0.0);
        if (sh.cnt[k] > 0) {
          const double v = a * (1.0 / (double)sh.cnt[k]);
          const double df = v - sh.cen[e];
          sh.cen[e] = v;
          shift = fma(df, df, shift);
        }
      }
    }
    const double shift_tot = km_block_sum(shift, sh.red);
    if (tid == 0)
      for (int m = 0; m < n_moved; ++m) lab[sh.moved_row[m]] = sh.moved_old[m];   // the labels stay the assignment's
    __syncthreads();
    ++it;
    if (!changed) { strict = true; break; }
    if (shift_tot <= tol_abs) break;
  }
  if (!strict) (void)km_assign(sh, zs, ld, n, D, K, lab, dist);   // labels consistent with the final centres

  double part = 0.0;
  for (int i = tid; i < n; i += KM_THREADS) part += km_sqdist(zs + (long long)i * ld, sh.cen + lab[i] * D, D);
  const double inertia = km_block_sum(part, sh.red);
  for (int e = tid; e < KD; e += KM_THREADS) cen_out[e] = sh.cen[e];
  if (tid == 0) { inertia_all[sr] = inertia; n_iter_all[sr] = it; }
}

// per segment: the restart of lowest inertia (ties: lowest r) and its labels / centres / inertia / n_iter
__global__ __launch_bounds__(256) void kmeans_select_kernel(const long long* __restrict__ offsets, int D, int k_max, int R,
                                                            long long rows, const int* __restrict__ labels_all,
                                                            const double* __restrict__ centers_all,
                                                            const double* __restrict__ inertia_all,
                                                            const int* __restrict__ n_iter_all, int* __restrict__ labels,
                                                            double* __restrict__ centers, double* __restrict__ inertia,
                                                            int* __restrict__ n_iter, int* __restrict__ restart) {
  const int s = blockIdx.x, tid = threadIdx.x;
  int best = 0;
  double bv = inertia_all[(long long)s * R];
  for (int r = 1; r < R; ++r) {
    const double v = inertia_all[(long long)s * R + r];
    if (v < bv || (isnan(bv) && !isnan(v))) { bv = v; best = r; }
  }
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  for (long long i = r0 + tid; i < r1; i += 256) labels[i] = labels_all[(long long)best * rows + i];
  const int KD = k_max * D;
  for (int e = tid; e < KD; e += 256) centers[(long long)s * KD + e] = centers_all[((long long)s * R + best) * KD + e];
  if (tid == 0) {
    inertia[s] = bv;
    n_iter[s] = n_iter_all[(long long)s * R + best];
    restart[s] = best;
  }
}

// ------------------------------------------------------------------------------------------------------- ARI / NMI
// a: the reference labelling ("true"), b: the clustering.  Both scores are symmetric in (a, b).
__global__ __launch_bounds__(CS_THREADS) void cluster_scores_kernel(const int* __restrict__ a, const int* __restrict__ b,
                                                                    const long long* __restrict__ offsets,
                                                                    double* __restrict__ out) {
  __shared__ int table[CS_TABLE];
  __shared__ int ida[CS_VALUES], idb[CS_VALUES];   // presence, then the dense class id of every label value
  __shared__ double red[CS_THREADS];
  __shared__ long long redl[CS_THREADS];
  __shared__ int na_s, nb_s, bad_s;
  const int tid = threadIdx.x, s = blockIdx.x;
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const int* la = a + r0;
  const int* lb = b + r0;
  for (int v = tid; v < CS_VALUES; v += CS_THREADS) { ida[v] = 0; idb[v] = 0; }
  if (tid == 0) bad_s = 0;
  __syncthreads();
  for (int i = tid; i < n; i += CS_THREADS) {
    const int va = la[i], vb = lb[i];
    if (va < 0 || va >= CS_VALUES || vb < 0 || vb >= CS_VALUES) bad_s = 1;
    else { ida[va] = 1; idb[vb] = 1; }
  }
  __syncthreads();
  if (tid == 0) {   // dense ids in value order
    int c = 0;
    for (int v = 0; v < CS_VALUES; ++v) { const int p = ida[v]; ida[v] = p ? c : -1; c += p; }
    na_s = c;
    c = 0;
    for (int v = 0; v < CS_VALUES; ++v) { const int p = idb[v]; idb[v] = p ? c : -1; c += p; }
    nb_s = c;
  }
  __syncthreads();
  const int na = na_s, nb = nb_s;
  double* o = out + 2 * (long long)s;
  if (bad_s || n < 1 || (long long)na * nb > CS_TABLE) {   // outside the documented domain: NaN, nothing out of bounds
    if (tid == 0) { o[0] = NAN; o[1] = NAN; }
    return;
  }
  const int cells = na * nb;
  for (int e = tid; e < cells; e += CS_THREADS) table[e] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += CS_THREADS) atomicAdd(&table[ida[la[i]] * nb + idb[lb[i]]], 1);
  __syncthreads();

  // integer sums: sum n_ij^2, sum_i a_i^2, sum_j b_j^2 (fixed tree; integer addition is exact anyway)
  long long ssq = 0, sa2 = 0, sb2 = 0;
  for (int e = tid; e < cells; e += CS_THREADS) ssq += (long long)table[e] * table[e];
  // row / column totals into ida / idb (their id role is over)
  __syncthreads();
  for (int i = tid; i < na; i += CS_THREADS) {
    int t = 0;
    for (int j = 0; j < nb; ++j) t += table[i * nb + j];
    ida[i] = t;
    sa2 += (long long)t * t;
  }
  for (int j = tid; j < nb; j += CS_THREADS) {
    int t = 0;
    for (int i = 0; i < na; ++i) t += table[i * nb + j];
    idb[j] = t;
    sb2 += (long long)t * t;
  }
  long long tot[3];
  const long long loc[3] = {ssq, sa2, sb2};
  for (int q = 0; q < 3; ++q) {
    __syncthreads();
    redl[tid] = loc[q];
    __syncthreads();
    for (int h = CS_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) redl[tid] += redl[tid + h];
      __syncthreads();
    }
    tot[q] = redl[0];
  }
  __syncthreads();

  // mutual information and the two entropies (natural log), sklearn's term order; fixed tree
  const double dn = (double)n, logn = log(dn);
  double mi = 0.0, ha = 0.0, hb = 0.0;
  for (int e = tid; e < cells; e += CS_THREADS) {
    const int v = table[e];
    if (v == 0) continue;
    const int i = e / nb, j = e - i * nb;
    const double nm = (double)v / dn;
    const double outer = (double)((long long)ida[i] * (long long)idb[j]);
    const double log_outer = -log(outer) + logn + logn;
    const double t = nm * (log((double)v) - logn) + nm * log_outer;
    mi += fabs(t) < 2.220446049250313e-16 ? 0.0 : t;
  }
  for (int i = tid; i < na; i += CS_THREADS) ha -= ((double)ida[i] / dn) * (log((double)ida[i]) - logn);
  for (int j = tid; j < nb; j += CS_THREADS) hb -= ((double)idb[j] / dn) * (log((double)idb[j]) - logn);
  double ftot[3];
  const double floc[3] = {mi, ha, hb};
  for (int q = 0; q < 3; ++q) {
    __syncthreads();
    red[tid] = floc[q];
    __syncthreads();
    for (int h = CS_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    ftot[q] = red[0];
  }
  if (tid != 0) return;

  // ARI, sklearn's pair_confusion_matrix: a = "true", b = "pred"
  const long long nn = (long long)n;
  const long long tp = tot[0] - nn, fp = tot[2] - tot[0], fn = tot[1] - tot[0], tn = nn * nn - fp - fn - tot[0];
  double ari = 1.0;
  if (fn != 0 || fp != 0) ari = 2.0 * (double)(tp * tn - fn * fp) / (double)((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn));
  // NMI, average_method="arithmetic"
  double nmi;
  if (na == 1 && nb == 1) {
    nmi = 1.0;
  } else {
    const double m = (na == 1 || nb == 1) ? 0.0 : fmax(ftot[0], 0.0);   // a single class on one side: MI = 0
    const double norm = 0.5 * ((na == 1 ? 0.0 : ftot[1]) + (nb == 1 ? 0.0 : ftot[2]));
    nmi = (m == 0.0 || !(norm > 0.0)) ? 0.0 : m / norm;
  }
  o[0] = ari;
  o[1] = nmi;
}

}  // namespace

// --------------------------------------------------------------------------------------------------------- entry points
extern "C" int mcl_pca_gram(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t G,
                            int32_t max_rows, const int64_t* gram_offsets, double* mean, double* gram,
                            mcl_stream_t stream) {
  if (!x || !offsets || !gram_offsets || !mean || !gram) return MCL_EINVAL;
  if (S < 1 || G < 1 || max_rows < 1 || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (S > 65535) return MCL_EUNSUPPORTED;   // grid.y / grid.z
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* goff = reinterpret_cast<const long long*>(gram_offsets);
  const int M = max_rows < G ? max_rows : G;
  const int nb = (M + 63) / 64;
  MCL_CLEAR_ERROR();
  if (dtype == 0) {
    hipLaunchKernelGGL((pca_mean_kernel<float>), dim3((G + 63) / 64, S), dim3(256), 0, st, static_cast<const float*>(x),
                       (long long)ld, off, G, mean);
    hipLaunchKernelGGL((pca_gram_kernel<float>), dim3(nb, nb, S), dim3(256), 0, st, static_cast<const float*>(x),
                       (long long)ld, off, G, (const double*)mean, goff, gram);
  } else {
    hipLaunchKernelGGL((pca_mean_kernel<double>), dim3((G + 63) / 64, S), dim3(256), 0, st, static_cast<const double*>(x),
                       (long long)ld, off, G, mean);
    hipLaunchKernelGGL((pca_gram_kernel<double>), dim3(nb, nb, S), dim3(256), 0, st, static_cast<const double*>(x),
                       (long long)ld, off, G, (const double*)mean, goff, gram);
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_pca_project(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t G,
                               int32_t max_rows, int32_t n_comps, const double* mean, const double* evec,
                               const int64_t* evec_offsets, const double* eval, double* loadings, double* sign, double* z,
                               mcl_stream_t stream) {
  if (!x || !offsets || !mean || !evec || !evec_offsets || !eval || !loadings || !sign || !z) return MCL_EINVAL;
  if (S < 1 || G < 1 || max_rows < 1 || n_comps < 1 || ld < G || (dtype != 0 && dtype != 1)) return MCL_EINVAL;
  if (n_comps > KM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long* eoff = reinterpret_cast<const long long*>(evec_offsets);
  MCL_CLEAR_ERROR();
  if (dtype == 0)
    hipLaunchKernelGGL((pca_loadings_kernel<float>), dim3((G + 255) / 256, S), dim3(256), 0, st,
                       static_cast<const float*>(x), (long long)ld, off, G, n_comps, mean, evec, eoff, loadings);
  else
    hipLaunchKernelGGL((pca_loadings_kernel<double>), dim3((G + 255) / 256, S), dim3(256), 0, st,
                       static_cast<const double*>(x), (long long)ld, off, G, n_comps, mean, evec, eoff, loadings);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(pca_sign_kernel, dim3(S), dim3(256), 0, st, (const double*)loadings, G, n_comps, sign);
  MCL_CHECK_LAUNCH();
  if (dtype == 0)
    hipLaunchKernelGGL((pca_scores_kernel<float>), dim3((max_rows + 3) / 4, S), dim3(256), 0, st,
                       static_cast<const float*>(x), (long long)ld, off, G, n_comps, mean, evec, eoff, eval,
                       (const double*)sign, z);
  else
    hipLaunchKernelGGL((pca_scores_kernel<double>), dim3((max_rows + 3) / 4, S), dim3(256), 0, st,
                       static_cast<const double*>(x), (long long)ld, off, G, n_comps, mean, evec, eoff, eval,
                       (const double*)sign, z);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_kmeans(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                          const int32_t* k, int32_t k_max, int32_t R, const int64_t* seeds, uint64_t seed,
                          int32_t segment_base, double tol, int32_t max_iter, int64_t* seeds_out, int32_t* labels_all,
                          double* centers_all, double* inertia_all, int32_t* n_iter_all, double* work, int32_t* labels,
                          double* centers, double* inertia, int32_t* n_iter, int32_t* restart, mcl_stream_t stream) {
  if (!z || !offsets || !k || !seeds_out || !labels_all || !centers_all || !inertia_all || !n_iter_all || !work ||
      !labels || !centers || !inertia || !n_iter || !restart)
    return MCL_EINVAL;
  if (S < 1 || rows < 1 || D < 1 || k_max < 1 || R < 1 || ld < D || max_iter < 1 || !(tol >= 0.0)) return MCL_EINVAL;
  if (D > KM_MAX || k_max > KM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(kmeans_kernel, dim3(R, S), dim3(KM_THREADS), 0, st, z, (long long)ld, off, D, (const int*)k, k_max, R,
                     reinterpret_cast<const long long*>(seeds), (unsigned long long)seed, segment_base, tol, max_iter,
                     (long long)rows, reinterpret_cast<long long*>(seeds_out), labels_all, centers_all, inertia_all,
                     n_iter_all, work);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_select_kernel, dim3(S), dim3(256), 0, st, off, D, k_max, R, (long long)rows,
                     (const int*)labels_all, (const double*)centers_all, (const double*)inertia_all,
                     (const int*)n_iter_all, labels, centers, inertia, n_iter, restart);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_cluster_scores(const int32_t* labels_a, const int32_t* labels_b, const int64_t* offsets, int32_t S,
                                  int32_t max_rows, double* scores, mcl_stream_t stream) {
  if (!labels_a || !labels_b || !offsets || !scores || S < 1 || max_rows < 1) return MCL_EINVAL;
  if (max_rows > 50000) return MCL_EUNSUPPORTED;   // the pair counts (~ n^4 in the products) stay inside int64
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(cluster_scores_kernel, dim3(S), dim3(CS_THREADS), 0, mcl_stream(stream), labels_a, labels_b,
                     reinterpret_cast<const long long*>(offsets), scores);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
