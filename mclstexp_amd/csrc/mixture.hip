// Gaussian mixtures of PCA scores: EM as sklearn's GaussianMixture states it, for S slides (row segments) x R
// models per call, covariance_type full / tied / diag / spherical.  Everything is fp64 with contraction off (an a * b + c
// is two roundings, as in numpy), there are no floating-point atomics and every sum runs in one fixed order that depends
// on the segment's own shape alone: a slide inside a batch is bit-identical to the same slide alone.
//
//   mcl_gmm_fit      gmm_fit_kernel, grid (model, segment): one workgroup runs one whole EM problem (the M-step from
//                    the initial labels, the E / M iteration, the stopping rule, the final E-step) inside one launch; no
//                    workgroup waits for another.  Parameters sit in the per-model output arrays, log_resp / resp and the
//                    moment sums in the caller's workspace.
//   mcl_gmm_select   per segment the model of highest lower bound (ties: lowest r), its labels / resp / parameters, BIC, AIC.
//   mcl_gmm_predict  the E-step alone (the device function of the fit) under given parameters.
//   mcl_gmm_mstep    the M-step alone from given log-responsibilities (the device function of the fit).
//
// The sums over rows (n_k, means, scatter matrices) and the E-step's triangular product (x - mu_k) P_k run on
// v_mfma_f64_16x16x4_f64 with operands masked on load and the contraction index ascending.  The Cholesky factor of a
// covariance is right-looking in LDS, its inverse one forward substitution per column; a non-positive (or NaN) pivot sets
// the status word of that (model, segment) and ends that problem: an ordinary return.
#include "mixture_device.h"
#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(GM_THREADS) void gmm_fit_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int D, const int* __restrict__ ks,
    int k_max, int R, int type, const int* __restrict__ init_labels, double tol, int max_iter, double reg, long long rows,
    void* work, int* labels_all, double* weights_all, double* means_all, double* cov_all, double* prec_all,
    double* lower_bound_all, double* score_all, int* n_iter_all, int* converged_all, int* status_all) {
  __shared__ GmShared sh;
  const int tid = threadIdx.x;
  const int r = blockIdx.x, s = blockIdx.y;
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  const int K = ks[s];
  const long long sr = (long long)s * R + r;
  const long long csz = gm_cov_size(type, k_max, D);
  int* lab = labels_all + (long long)r * rows + r0;
  if (nl < 1 || nl > GM_MAX_ROWS || r0 < 0 || r0 + nl > rows || K < 1 || K > k_max || K > nl) {   // not a mixture problem
    if (tid == 0) {
      lower_bound_all[sr] = NAN; score_all[sr] = NAN; n_iter_all[sr] = 0; converged_all[sr] = 0; status_all[sr] = 2;
    }
    if (nl >= 1 && r0 >= 0 && r0 + nl <= rows)
      for (long long i = tid; i < nl; i += GM_THREADS) lab[i] = -1;
    return;
  }
  const GmWork wk = gm_work(work, rows, R, k_max);
  GmModel m;
  m.n = (int)nl; m.D = D; m.K = K; m.KS = k_max; m.type = type;
  m.x = z + r0 * ld; m.ld = ld;
  m.w = weights_all + sr * k_max;
  m.mu = means_all + sr * k_max * D;
  m.cov = cov_all + sr * csz;
  m.pc = prec_all + sr * csz;
  m.lr = wk.lr + ((long long)r * rows + r0) * k_max;
  m.lse = wk.lse + (long long)r * rows + r0;
  m.mom = wk.mom + sr * k_max * (2 * D + 1);
  const int n = m.n;

  // sklearn's _initialize(X, resp) with one-hot responsibilities (a label outside 0 .. K - 1: a row of zeros)
  const int* il = init_labels + (long long)r * rows + r0;
  for (long long e = tid; e < (long long)n * K; e += GM_THREADS) {
    const long long i = e / K;
    const int k = (int)(e - i * K);
    m.lr[i * k_max + k] = il[i] == k ? 1.0 : 0.0;
  }
  __syncthreads();
  int fail = gm_mstep(sh, m, reg, false, true);
  double lb = -INFINITY;
  int it = 0, conv = 0;
  while (!fail && it < max_iter) {
    const double prev = lb;
    lb = gm_estep(sh, m, nullptr, nullptr);
    fail = gm_mstep(sh, m, reg, true, false);
    ++it;
    if (fail) break;
    if (fabs(lb - prev) < tol) { conv = 1; break; }
  }
  if (fail) {   // sklearn raises "ill-defined empirical covariance" here
    if (tid == 0) {
      lower_bound_all[sr] = NAN; score_all[sr] = NAN; n_iter_all[sr] = it; converged_all[sr] = 0; status_all[sr] = 1;
    }
    for (int i = tid; i < n; i += GM_THREADS) lab[i] = -1;
    return;
  }
  const double score = gm_estep(sh, m, lab, nullptr);   // labels and log_resp under the final parameters
  if (tid == 0) {
    lower_bound_all[sr] = lb; score_all[sr] = score; n_iter_all[sr] = it; converged_all[sr] = conv; status_all[sr] = 0;
  }
}

// per segment: the model of highest lower bound (ties: lowest r; a failed model has NaN and never wins over a valid one)
__global__ __launch_bounds__(256) void gmm_select_kernel(
    const long long* __restrict__ offsets, int D, const int* __restrict__ ks, int k_max, int R, int type, long long rows,
    const void* work, const int* __restrict__ labels_all, const double* __restrict__ weights_all,
    const double* __restrict__ means_all, const double* __restrict__ cov_all, const double* __restrict__ prec_all,
    const double* __restrict__ lower_bound_all, const double* __restrict__ score_all, const int* __restrict__ n_iter_all,
    const int* __restrict__ converged_all, const int* __restrict__ status_all, int* __restrict__ labels,
    double* __restrict__ resp, double* __restrict__ weights, double* __restrict__ means, double* __restrict__ cov,
    double* __restrict__ prec, double* __restrict__ lower_bound, int* __restrict__ n_iter, int* __restrict__ converged,
    int* __restrict__ status, double* __restrict__ bic, double* __restrict__ aic, int* __restrict__ restart) {
  const int s = blockIdx.x, tid = threadIdx.x;
  int best = 0;
  double bv = lower_bound_all[(long long)s * R];
  for (int r = 1; r < R; ++r) {
    const double v = lower_bound_all[(long long)s * R + r];
    if (v > bv || (isnan(bv) && !isnan(v))) { bv = v; best = r; }
  }
  const long long sb = (long long)s * R + best;
  const int st = status_all[sb];
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  const int K = ks[s];
  if (st != 2) {
    const GmWork wk = gm_work(const_cast<void*>(work), rows, R, k_max);
    const double* lr = wk.lr + (long long)best * rows * k_max;
    for (long long i = r0 + tid; i < r1; i += 256) {
      labels[i] = labels_all[(long long)best * rows + i];
      for (int k = 0; k < k_max; ++k) resp[i * k_max + k] = (st == 0 && k < K) ? exp(lr[i * k_max + k]) : (st == 0 ? 0.0 : NAN);
    }
  }
  const long long csz = gm_cov_size(type, k_max, D);
  for (int e = tid; e < k_max; e += 256) weights[(long long)s * k_max + e] = weights_all[sb * k_max + e];
  for (int e = tid; e < k_max * D; e += 256) means[(long long)s * k_max * D + e] = means_all[sb * k_max * D + e];
  for (long long e = tid; e < csz; e += 256) {
    cov[(long long)s * csz + e] = cov_all[sb * csz + e];
    prec[(long long)s * csz + e] = prec_all[sb * csz + e];
  }
  if (tid == 0) {
    const double n = (double)(r1 - r0), score = score_all[sb];
    const double covp = type == GM_FULL ? (double)K * D * (D + 1) / 2.0 : type == GM_TIED ? (double)D * (D + 1) / 2.0
                      : type == GM_DIAG ? (double)K * D : (double)K;
    const double p = (double)(long long)(covp + (double)D * K + (double)K - 1.0);
    lower_bound[s] = bv;
    n_iter[s] = n_iter_all[sb];
    converged[s] = converged_all[sb];
    status[s] = st;
    restart[s] = best;
    bic[s] = ((-2.0 * score) * n) + p * log(n);
    aic[s] = ((-2.0 * score) * n) + 2.0 * p;
  }
}

__global__ __launch_bounds__(GM_THREADS) void gmm_predict_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int D, const int* __restrict__ ks,
    int k_max, int type, long long rows, const double* weights, const double* means, const double* prec,
    double* log_prob_norm, double* log_resp, double* resp, int* labels, double* score) {
  __shared__ GmShared sh;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  const int K = ks[s];
  if (nl < 1 || nl > GM_MAX_ROWS || r0 < 0 || r0 + nl > rows || K < 1 || K > k_max) {
    if (tid == 0) score[s] = NAN;
    return;
  }
  const long long csz = gm_cov_size(type, k_max, D);
  GmModel m;
  m.n = (int)nl; m.D = D; m.K = K; m.KS = k_max; m.type = type;
  m.x = z + r0 * ld; m.ld = ld;
  m.w = const_cast<double*>(weights) + (long long)s * k_max;
  m.mu = const_cast<double*>(means) + (long long)s * k_max * D;
  m.cov = nullptr;
  m.pc = const_cast<double*>(prec) + (long long)s * csz;
  m.lr = log_resp + r0 * k_max;
  m.lse = log_prob_norm + r0;
  m.mom = nullptr;
  const double sc = gm_estep(sh, m, labels + r0, resp + r0 * k_max);
  if (tid == 0) score[s] = sc;
}

__global__ __launch_bounds__(GM_THREADS) void gmm_mstep_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int D, const int* __restrict__ ks,
    int k_max, int type, long long rows, const double* __restrict__ log_resp, double reg, void* work, double* weights,
    double* means, double* cov, double* prec, int* status) {
  __shared__ GmShared sh;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  const int K = ks[s];
  if (nl < 1 || nl > GM_MAX_ROWS || r0 < 0 || r0 + nl > rows || K < 1 || K > k_max) {
    if (tid == 0) status[s] = 2;
    return;
  }
  const GmWork wk = gm_work(work, rows, 1, k_max);
  const long long csz = gm_cov_size(type, k_max, D);
  GmModel m;
  m.n = (int)nl; m.D = D; m.K = K; m.KS = k_max; m.type = type;
  m.x = z + r0 * ld; m.ld = ld;
  m.w = weights + (long long)s * k_max;
  m.mu = means + (long long)s * k_max * D;
  m.cov = cov + (long long)s * csz;
  m.pc = prec + (long long)s * csz;
  m.lr = wk.lr + r0 * k_max;
  m.lse = wk.lse + r0;
  m.mom = wk.mom + (long long)s * k_max * (2 * D + 1);
  for (long long e = tid; e < nl * K; e += GM_THREADS) {
    const long long i = e / K, k = e - i * K;
    m.lr[i * k_max + k] = log_resp[(r0 + i) * k_max + k];
  }
  __syncthreads();
  const int fail = gm_mstep(sh, m, reg, true, false);
  if (tid == 0) status[s] = fail;
}

bool gm_shape_ok(int32_t S, int64_t rows, int32_t D, int32_t k_max, int32_t type) {
  return S >= 1 && rows >= 1 && D >= 1 && k_max >= 1 && type >= GM_FULL && type <= GM_SPHERICAL;
}

// -------------------------------------------------------------------------------------------------- cluster validity
// Silhouette, Calinski-Harabasz and Davies-Bouldin of a labelling.  cv_sort_kernel: the kept rows of a slide in cluster
// order (dense cluster ids in label-value order, rows ascending inside a cluster: a stable counting sort).
// cv_pair_kernel: one thread per row walks every kept row in that order, staged through LDS, so every (row, cluster)
// distance sum runs over the cluster's rows ascending.  cv_scores_kernel: centroids and the three scores per slide.
constexpr int CV_THREADS = 256;
constexpr int CV_VALUES = 1024;   // label values in [0, 1024)
constexpr int CV_TILE = 64;       // rows staged per LDS tile of the pair pass

struct CvWork {
  double* dcen;   // (rows): distance of the row at a sorted position to its centroid
  double* cen;    // (rows, D): centroid of dense cluster c of slide s at row offsets[s] + c
  int* order;     // (rows): sorted position -> row of the slide
  int* scid;      // (rows): dense cluster id at a sorted position
  int* cid;       // (rows): dense cluster id of a row, -1 dropped
  int* start;     // (S, 1025): first sorted position of every dense cluster
  int* info;      // (S, 4): clusters, kept rows, valid
};
__host__ __device__ inline long long cv_work_bytes(long long rows, int S, int D) {
  const long long b = 8 * (rows + rows * D) + 4 * (3 * rows + (long long)S * (CV_VALUES + 1 + 4));
  return (b + 7) / 8 * 8;
}
__host__ __device__ inline CvWork cv_work(void* work, long long rows, int S, int D) {
  CvWork wk;
  wk.dcen = static_cast<double*>(work);
  wk.cen = wk.dcen + rows;
  wk.order = reinterpret_cast<int*>(wk.cen + rows * D);
  wk.scid = wk.order + rows;
  wk.cid = wk.scid + rows;
  wk.start = wk.cid + rows;
  wk.info = wk.start + (long long)S * (CV_VALUES + 1);
  return wk;
}

__global__ __launch_bounds__(CV_THREADS) void cv_sort_kernel(const long long* __restrict__ offsets,
                                                             const int* __restrict__ labels, long long rows, int S, int D,
                                                             void* work) {
  __shared__ int cnt[CV_VALUES], dense[CV_VALUES], base[CV_VALUES], lab[CV_THREADS];
  __shared__ int bad_s, valid_s;
  const int tid = threadIdx.x, s = blockIdx.x;
  const CvWork wk = cv_work(work, rows, S, D);
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  int* info = wk.info + 4 * s;
  if (nl < 2 || nl > GM_MAX_ROWS || r0 < 0 || r0 + nl > rows) {
    if (tid == 0) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 1; }
    return;
  }
  const int n = (int)nl;
  const int* ls = labels + r0;
  for (int v = tid; v < CV_VALUES; v += CV_THREADS) cnt[v] = 0;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  for (int i = tid; i < n; i += CV_THREADS) {
    const int l = ls[i];
    if (l < -1 || l >= CV_VALUES) bad_s = 1;
    else if (l >= 0) atomicAdd(&cnt[l], 1);
  }
  __syncthreads();
  if (tid == 0) {   // dense ids in value order, the first sorted position of every cluster
    int* start = wk.start + (long long)s * (CV_VALUES + 1);
    int c = 0, pos = 0;
    for (int v = 0; v < CV_VALUES; ++v) {
      if (cnt[v] > 0) { dense[v] = c; start[c] = pos; base[v] = pos; pos += cnt[v]; ++c; }
    }
    start[c] = pos;
    const int valid = !bad_s && c >= 2 && c <= pos - 1;
    info[0] = c; info[1] = pos; info[2] = valid; info[3] = bad_s;
    valid_s = valid;
  }
  __syncthreads();
  if (!valid_s) return;
  for (int b0 = 0; b0 < n; b0 += CV_THREADS) {
    const int i = b0 + tid;
    const int l = i < n ? ls[i] : -1;
    lab[tid] = l;
    __syncthreads();
    if (l >= 0) {
      int rank = 0;
      for (int t = 0; t < tid; ++t) rank += lab[t] == l;
      const int pos = base[l] + rank;
      wk.order[r0 + pos] = i;
      wk.scid[r0 + pos] = dense[l];
      wk.cid[r0 + i] = dense[l];
    } else if (i < n) {
      wk.cid[r0 + i] = -1;
    }
    __syncthreads();
    if (l >= 0) atomicAdd(&base[l], 1);
    __syncthreads();
  }
}

// DB: D rounded up to the register width of a row; columns past D hold zeros on both sides and add 0.0 to a sum
template <int DB>
__global__ __launch_bounds__(CV_THREADS) void cv_pair_kernel(const double* __restrict__ z, long long ld,
                                                             const long long* __restrict__ offsets, long long rows, int S,
                                                             int D, void* work, double* __restrict__ silhouette) {
  __shared__ double tile[CV_TILE * DB];
  __shared__ int tcid[CV_TILE];
  __shared__ int start[CV_VALUES + 1];
  const int tid = threadIdx.x, s = blockIdx.y;
  const CvWork wk = cv_work(work, rows, S, D);
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  if (nl < 2 || nl > GM_MAX_ROWS || r0 < 0 || r0 + nl > rows) return;
  const int n = (int)nl;
  if ((long long)blockIdx.x * CV_THREADS >= n) return;
  const int i = blockIdx.x * CV_THREADS + tid;
  const int* info = wk.info + 4 * s;
  const int ncl = info[0], nkept = info[1];
  if (!info[2]) {
    if (i < n) silhouette[r0 + i] = NAN;
    return;
  }
  for (int c = tid; c <= ncl; c += CV_THREADS) start[c] = wk.start[(long long)s * (CV_VALUES + 1) + c];
  const int own = i < n ? wk.cid[r0 + i] : -1;
  double xi[DB];
  {
    const double* xr = z + (r0 + (i < n ? i : n - 1)) * ld;
#pragma unroll
    for (int d = 0; d < DB; ++d) xi[d] = d < D ? xr[d < D ? d : 0] : 0.0;
  }
  double a = 0.0, b = INFINITY, acc = 0.0;
  int cur = -1, own_cnt = 1;
  for (int p0 = 0; p0 < nkept; p0 += CV_TILE) {
    __syncthreads();
    for (int e = tid; e < CV_TILE * DB; e += CV_THREADS) {
      const int jr = e / DB, d = e - jr * DB, p = p0 + jr;
      tile[e] = (p < nkept && d < D) ? z[(r0 + wk.order[r0 + p]) * ld + d] : 0.0;
    }
    if (tid < CV_TILE) tcid[tid] = p0 + tid < nkept ? wk.scid[r0 + p0 + tid] : -2;
    __syncthreads();
    const int jn = min(CV_TILE, nkept - p0);
    for (int jr = 0; jr < jn; ++jr) {
      const int c = tcid[jr];
      if (c != cur) {   // the same branch in every thread: all walk the same rows
        if (cur >= 0) {
          const int cn = start[cur + 1] - start[cur];
          if (cur == own) { a = cn > 1 ? acc / (double)(cn - 1) : 0.0; own_cnt = cn; }
          else b = fmin(b, acc / (double)cn);
        }
        cur = c;
        acc = 0.0;
      }
      const double* xj = tile + jr * DB;
      double sq = 0.0;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const double df = xi[d] - xj[d];
        sq += df * df;
      }
      acc += sqrt(sq);
    }
  }
  if (cur >= 0) {
    const int cn = start[cur + 1] - start[cur];
    if (cur == own) { a = cn > 1 ? acc / (double)(cn - 1) : 0.0; own_cnt = cn; }
    else b = fmin(b, acc / (double)cn);
  }
  if (i < n) {
    double sv = NAN;
    if (own >= 0) {
      sv = (b - a) / fmax(a, b);
      if (own_cnt == 1 || isnan(sv)) sv = 0.0;
    }
    silhouette[r0 + i] = sv;
  }
}

__global__ __launch_bounds__(CV_THREADS) void cv_scores_kernel(const double* __restrict__ z, long long ld,
                                                               const long long* __restrict__ offsets, long long rows, int S,
                                                               int D, void* work, const double* __restrict__ silhouette,
                                                               double* __restrict__ scores) {
  __shared__ double red[CV_THREADS];
  __shared__ double mean[GM_MAX];
  __shared__ double sc[CV_VALUES];
  const int tid = threadIdx.x, s = blockIdx.x;
  const CvWork wk = cv_work(work, rows, S, D);
  double* out = scores + 3 * (long long)s;
  const int* info = wk.info + 4 * s;
  if (!info[2]) {
    if (tid == 0) { out[0] = NAN; out[1] = NAN; out[2] = NAN; }
    return;
  }
  const long long r0 = offsets[s];
  const int n = (int)(offsets[s + 1] - r0);
  const int ncl = info[0], nkept = info[1];
  const int* start = wk.start + (long long)s * (CV_VALUES + 1);
  const int* order = wk.order + r0;
  const int* scid = wk.scid + r0;
  double* cen = wk.cen + r0 * D;
  double* dcen = wk.dcen + r0;
  const double* zs = z + r0 * ld;
  for (int e = tid; e < ncl * D; e += CV_THREADS) {
    const int c = e / D, d = e - c * D;
    double acc = 0.0;
    for (int p = start[c]; p < start[c + 1]; ++p) acc += zs[(long long)order[p] * ld + d];
    cen[e] = acc / (double)(start[c + 1] - start[c]);
  }
  for (int d = 0; d < D; ++d) {
    double part = 0.0;
    for (int p = tid; p < nkept; p += CV_THREADS) part += zs[(long long)order[p] * ld + d];
    const double tot = gm_block_sum(part, red);
    if (tid == 0) mean[d] = tot / (double)nkept;
  }
  __syncthreads();
  double part = 0.0;
  for (int p = tid; p < nkept; p += CV_THREADS) {
    const double* xr = zs + (long long)order[p] * ld;
    const double* cc = cen + scid[p] * D;
    double sq = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = xr[d] - cc[d];
      sq += df * df;
    }
    dcen[p] = sqrt(sq);
    part += sq;
  }
  const double intra = gm_block_sum(part, red);
  part = 0.0;
  for (int c = tid; c < ncl; c += CV_THREADS) {
    double sq = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = cen[c * D + d] - mean[d];
      sq += df * df;
    }
    part += (double)(start[c + 1] - start[c]) * sq;
  }
  const double extra = gm_block_sum(part, red);
  double any_s = 0.0;
  for (int c = tid; c < ncl; c += CV_THREADS) {
    double acc = 0.0;
    for (int p = start[c]; p < start[c + 1]; ++p) acc += dcen[p];
    const double v = acc / (double)(start[c + 1] - start[c]);
    sc[c] = v;
    if (v > 1e-8) any_s = 1.0;
  }
  any_s = gm_block_sum(any_s, red);
  part = 0.0;
  double any_d = 0.0;
  for (int c = tid; c < ncl; c += CV_THREADS) {
    double best = 0.0;   // the cluster against itself: distance 0 counts as infinite
    for (int j = 0; j < ncl; ++j) {
      double sq = 0.0;
      for (int d = 0; d < D; ++d) {
        const double df = cen[c * D + d] - cen[j * D + d];
        sq += df * df;
      }
      const double dist = sqrt(sq);
      if (dist > 1e-8) any_d = 1.0;
      if (dist != 0.0) best = fmax(best, (sc[c] + sc[j]) / dist);
    }
    part += best;
  }
  const double db_sum = gm_block_sum(part, red);
  any_d = gm_block_sum(any_d, red);
  part = 0.0;
  for (int i = tid; i < n; i += CV_THREADS) part += wk.cid[r0 + i] >= 0 ? silhouette[r0 + i] : 0.0;
  const double sil = gm_block_sum(part, red);
  if (tid == 0) {
    out[0] = sil / (double)nkept;
    out[1] = intra == 0.0 ? 1.0 : (extra * (double)(nkept - ncl)) / (intra * ((double)ncl - 1.0));
    out[2] = (any_s == 0.0 || any_d == 0.0) ? 0.0 : db_sum / (double)ncl;
  }
}

}  // namespace

// --------------------------------------------------------------------------------------------------------- entry points
extern "C" int64_t mcl_gmm_workspace_bytes(int64_t rows, int32_t S, int32_t R, int32_t D, int32_t k_max) {
  if (rows < 1 || S < 1 || R < 1 || D < 1 || D > GM_MAX || k_max < 1 || k_max > GM_MAX) return -1;
  return 8 * gm_work_doubles(rows, S, R, D, k_max);
}

extern "C" int mcl_gmm_fit(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                           const int32_t* k, int32_t k_max, int32_t R, int32_t covariance_type,
                           const int32_t* init_labels, double tol, int32_t max_iter, double reg_covar, void* work,
                           int64_t work_bytes, int32_t* labels_all, double* weights_all, double* means_all,
                           double* covariances_all, double* precisions_cholesky_all, double* lower_bound_all,
                           double* score_all, int32_t* n_iter_all, int32_t* converged_all, int32_t* status_all,
                           mcl_stream_t stream) {
  if (!z || !offsets || !k || !init_labels || !work || !labels_all || !weights_all || !means_all || !covariances_all ||
      !precisions_cholesky_all || !lower_bound_all || !score_all || !n_iter_all || !converged_all || !status_all)
    return MCL_EINVAL;
  if (!gm_shape_ok(S, rows, D, k_max, covariance_type) || R < 1 || ld < D || max_iter < 1 || !(tol >= 0.0) ||
      !(reg_covar >= 0.0))
    return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  if (work_bytes < 8 * gm_work_doubles(rows, S, R, D, k_max)) return MCL_EWORKSPACE;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(gmm_fit_kernel, dim3(R, S), dim3(GM_THREADS), 0, mcl_stream(stream), z, (long long)ld,
                     reinterpret_cast<const long long*>(offsets), D, (const int*)k, k_max, R, covariance_type,
                     (const int*)init_labels, tol, max_iter, reg_covar, (long long)rows, work, labels_all, weights_all,
                     means_all, covariances_all, precisions_cholesky_all, lower_bound_all, score_all, n_iter_all,
                     converged_all, status_all);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_gmm_select(const int64_t* offsets, int32_t S, int64_t rows, int32_t D, const int32_t* k, int32_t k_max,
                              int32_t R, int32_t covariance_type, const void* work, int64_t work_bytes,
                              const int32_t* labels_all, const double* weights_all, const double* means_all,
                              const double* covariances_all, const double* precisions_cholesky_all,
                              const double* lower_bound_all, const double* score_all, const int32_t* n_iter_all,
                              const int32_t* converged_all, const int32_t* status_all, int32_t* labels, double* resp,
                              double* weights, double* means, double* covariances, double* precisions_cholesky,
                              double* lower_bound, int32_t* n_iter, int32_t* converged, int32_t* status, double* bic,
                              double* aic, int32_t* restart, mcl_stream_t stream) {
  if (!offsets || !k || !work || !labels_all || !weights_all || !means_all || !covariances_all ||
      !precisions_cholesky_all || !lower_bound_all || !score_all || !n_iter_all || !converged_all || !status_all ||
      !labels || !resp || !weights || !means || !covariances || !precisions_cholesky || !lower_bound || !n_iter ||
      !converged || !status || !bic || !aic || !restart)
    return MCL_EINVAL;
  if (!gm_shape_ok(S, rows, D, k_max, covariance_type) || R < 1) return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  if (work_bytes < 8 * gm_work_doubles(rows, S, R, D, k_max)) return MCL_EWORKSPACE;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(gmm_select_kernel, dim3(S), dim3(256), 0, mcl_stream(stream),
                     reinterpret_cast<const long long*>(offsets), D, (const int*)k, k_max, R, covariance_type,
                     (long long)rows, work, (const int*)labels_all, weights_all, means_all, covariances_all,
                     precisions_cholesky_all, lower_bound_all, score_all, (const int*)n_iter_all,
                     (const int*)converged_all, (const int*)status_all, labels, resp, weights, means, covariances,
                     precisions_cholesky, lower_bound, n_iter, converged, status, bic, aic, restart);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_gmm_predict(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                               const int32_t* k, int32_t k_max, int32_t covariance_type, const double* weights,
                               const double* means, const double* precisions_cholesky, double* log_prob_norm,
                               double* log_resp, double* resp, int32_t* labels, double* score, mcl_stream_t stream) {
  if (!z || !offsets || !k || !weights || !means || !precisions_cholesky || !log_prob_norm || !log_resp || !resp ||
      !labels || !score)
    return MCL_EINVAL;
  if (!gm_shape_ok(S, rows, D, k_max, covariance_type) || ld < D) return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(gmm_predict_kernel, dim3(S), dim3(GM_THREADS), 0, mcl_stream(stream), z, (long long)ld,
                     reinterpret_cast<const long long*>(offsets), D, (const int*)k, k_max, covariance_type, (long long)rows,
                     weights, means, precisions_cholesky, log_prob_norm, log_resp, resp, labels, score);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_gmm_mstep(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                             const int32_t* k, int32_t k_max, int32_t covariance_type, const double* log_resp,
                             double reg_covar, void* work, int64_t work_bytes, double* weights, double* means,
                             double* covariances, double* precisions_cholesky, int32_t* status, mcl_stream_t stream) {
  if (!z || !offsets || !k || !log_resp || !work || !weights || !means || !covariances || !precisions_cholesky || !status)
    return MCL_EINVAL;
  if (!gm_shape_ok(S, rows, D, k_max, covariance_type) || ld < D || !(reg_covar >= 0.0)) return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  if (work_bytes < 8 * gm_work_doubles(rows, S, 1, D, k_max)) return MCL_EWORKSPACE;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(gmm_mstep_kernel, dim3(S), dim3(GM_THREADS), 0, mcl_stream(stream), z, (long long)ld,
                     reinterpret_cast<const long long*>(offsets), D, (const int*)k, k_max, covariance_type, (long long)rows,
                     log_resp, reg_covar, work, weights, means, covariances, precisions_cholesky, status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int64_t mcl_cluster_validity_workspace_bytes(int64_t rows, int32_t S, int32_t D) {
  if (rows < 1 || S < 1 || D < 1 || D > GM_MAX) return -1;
  return cv_work_bytes(rows, S, D);
}

extern "C" int mcl_cluster_validity(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                                    const int32_t* labels, void* work, int64_t work_bytes, double* silhouette,
                                    double* scores, mcl_stream_t stream) {
  if (!z || !offsets || !labels || !work || !silhouette || !scores) return MCL_EINVAL;
  if (S < 1 || rows < 1 || D < 1 || ld < D) return MCL_EINVAL;
  if (D > GM_MAX || S > 65535) return MCL_EUNSUPPORTED;
  if (work_bytes < cv_work_bytes(rows, S, D)) return MCL_EWORKSPACE;
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const long long max_n = rows < GM_MAX_ROWS ? rows : GM_MAX_ROWS;
  const dim3 grid((unsigned)((max_n + CV_THREADS - 1) / CV_THREADS), S);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(cv_sort_kernel, dim3(S), dim3(CV_THREADS), 0, st, off, (const int*)labels, (long long)rows, S, D, work);
  MCL_CHECK_LAUNCH();
  if (D <= 16)
    hipLaunchKernelGGL((cv_pair_kernel<16>), grid, dim3(CV_THREADS), 0, st, z, (long long)ld, off, (long long)rows, S, D,
                       work, silhouette);
  else
    hipLaunchKernelGGL((cv_pair_kernel<64>), grid, dim3(CV_THREADS), 0, st, z, (long long)ld, off, (long long)rows, S, D,
                       work, silhouette);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(cv_scores_kernel, dim3(S), dim3(CV_THREADS), 0, st, z, (long long)ld, off, (long long)rows, S, D, work,
                     (const double*)silhouette, scores);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
