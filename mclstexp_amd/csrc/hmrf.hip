// Potts-HMRF mixtures on the spot lattice: the Gaussian mixture of csrc/mixture.hip with a Potts prior on the
// labels over the fixed-width neighbour list of csrc/spatial.hip, fitted by EM with the mean-field approximation of Celeux,
// Forbes and Peyrard (2003) in synchronous sweeps: during iteration t the neighbours' memberships are the responsibilities
// of iteration t - 1.  Everything is fp64 with contraction off, there are no floating-point atomics and every sum runs in
// one fixed order that depends on the slide's own shape alone: a slide inside a batch is bit-identical to the same slide
// alone.  The E-step's two passes, the M-step and the block sum are the mixture's own (mixture_device.h).
//
//   mcl_hmrf_fit        hmrf_fit_kernel, grid (start, slide): one workgroup runs one whole problem inside one launch; no
//                       workgroup waits for another.  The workspace begins with the mixture's, so mcl_gmm_select picks the
//                       start of highest lower bound; the field (R, rows, k_max) follows it.
//   mcl_hmrf_estep      one E-step (the device function of the fit) under given parameters and previous responsibilities.
//   mcl_label_refine    one synchronous round of neighbourhood majority relabelling.
//   mcl_edge_agreement  per slide the weight of the kept neighbour pairs that share a label, and the weight of all of them.
//
// The field pass: element (i, k) of a slide goes to thread (i K + k) mod 256, so the lanes of a wave read the K
// responsibilities of one neighbour as one contiguous run (several rows per wave for small K).  A neighbour index outside
// the slide is clamped for the load and masked at the use: the slot counts as pruned and bit 4 of the status is set.
#include "mixture_device.h"
#pragma clang fp contract(off)

namespace {

constexpr int HM_MAX_ROWS = 16384;   // the lattice's
constexpr int HM_MAX_KW = 64;
constexpr int HM_BAD_INDEX = 4;
constexpr int RF_THREADS = 128;      // label_refine_kernel: 64 staged labels per thread in 32 KiB of LDS

struct HmGraph {   // one slide's part of the neighbour list
  const int* nbr;     // (n, kw) segment-local
  const double* w;    // (n, kw); 0 marks a pruned slot
  int kw;
};

// fld[i][k] = sum over slots c ascending with w_ic != 0 of w_ic q[nbr_ic][k]: a running sum from 0.0, product then add.
// q: (n, KS) responsibilities.  Returns (this thread) whether a kept slot held an index outside 0 .. n - 1.
__device__ __forceinline__ int hm_field(const HmGraph& g, int n, int K, int KS, const double* q, double* fld) {
  int bad = 0;
  const int kw = g.kw;
  for (int e = threadIdx.x; e < n * K; e += GM_THREADS) {   // n K <= 16384 x 64
    const int i = e / K, k = e - i * K;
    const int* nb = g.nbr + (long long)i * kw;
    const double* wr = g.w + (long long)i * kw;
    double f = 0.0;
    for (int c = 0; c < kw; ++c) {
      const int j = nb[c];
      const double wv = wr[c];
      const bool in = j >= 0 && j < n;
      const double qv = q[(long long)(in ? j : 0) * KS + k];   // loaded whatever the slot holds, used where it is kept
      if (wv != 0.0) {
        if (in) f += wv * qv;
        else bad = 1;
      }
    }
    fld[(long long)i * KS + k] = f;
  }
  return bad;
}

struct HmWork {
  GmWork gm;
  double* field;   // (R, rows, k_max)
};
__host__ __device__ inline long long hm_work_doubles(long long rows, int S, int R, int D, int k_max) {
  return gm_work_doubles(rows, S, R, D, k_max) + (long long)R * rows * k_max;
}
__host__ __device__ inline HmWork hm_work(void* work, long long rows, int S, int R, int D, int k_max) {
  HmWork wk;
  wk.gm = gm_work(work, rows, R, k_max);
  wk.field = static_cast<double*>(work) + gm_work_doubles(rows, S, R, D, k_max);
  return wk;
}

// csz, the doubles of one problem's covariances, is gm_cov_size(type, k_max, D) formed on the host and passed to both kernels:
// with that ladder over the type inside hmrf_estep_kernel the compiler left the 64-bit row stride k_max unwritten on the
// spherical path, and the field pass loaded q[j * k_max + k] from a wild address.
//
// one E-step of the HMRF: the field of q (read before the density pass overwrites lr, which may be q itself), the density
// pass, the coupled finalisation.  Returns the mean of lse - za; *bad is or-ed by the threads that met a bad index.
__device__ __forceinline__ double hm_estep(GmShared& sh, const GmModel& m, const HmGraph& g, double beta, const double* q,
                                           double* fld, int* lab, double* resp, double* za, int* bad) {
  if (hm_field(g, m.n, m.K, m.KS, q, fld)) *bad = 1;
  __syncthreads();
  gm_density(sh, m);
  return gm_finalise(sh, m, lab, resp, fld, beta, za);
}

__global__ __launch_bounds__(GM_THREADS) void hmrf_fit_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int S, int D,
    const int* __restrict__ ks, int k_max, int R, int type, const int* __restrict__ init_labels,
    const int* __restrict__ nbr, const double* __restrict__ wgt, int kw, const double* __restrict__ beta, double tol,
    int max_iter, double reg, long long rows, long long csz, void* work, int* labels_all, double* weights_all,
    double* means_all, double* cov_all, double* prec_all, double* lower_bound_all, double* score_all, int* n_iter_all,
    int* converged_all, int* status_all) {
  __shared__ GmShared sh;
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  const int r = blockIdx.x, s = blockIdx.y;
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  const int K = ks[s];
  const double b = beta[s];
  const long long sr = (long long)s * R + r;
  int* lab = labels_all + (long long)r * rows + r0;
  if (nl < 1 || nl > HM_MAX_ROWS || r0 < 0 || r0 + nl > rows || K < 1 || K > k_max || K > nl || !(b >= 0.0) ||
      !(b < INFINITY)) {   // not a problem
    if (tid == 0) {
      lower_bound_all[sr] = NAN; score_all[sr] = NAN; n_iter_all[sr] = 0; converged_all[sr] = 0; status_all[sr] = 2;
    }
    if (nl >= 1 && r0 >= 0 && r0 + nl <= rows)
      for (long long i = tid; i < nl; i += GM_THREADS) lab[i] = -1;
    return;
  }
  const HmWork wk = hm_work(work, rows, S, R, D, k_max);
  GmModel m;
  m.n = (int)nl; m.D = D; m.K = K; m.KS = k_max; m.type = type;
  m.x = z + r0 * ld; m.ld = ld;
  m.w = weights_all + sr * k_max;
  m.mu = means_all + sr * k_max * D;
  m.cov = cov_all + sr * csz;
  m.pc = prec_all + sr * csz;
  m.lr = wk.gm.lr + ((long long)r * rows + r0) * k_max;
  m.lse = wk.gm.lse + (long long)r * rows + r0;
  m.mom = wk.gm.mom + sr * k_max * (2 * D + 1);
  double* fld = wk.field + ((long long)r * rows + r0) * k_max;
  HmGraph g;
  g.nbr = nbr + r0 * kw; g.w = wgt + r0 * kw; g.kw = kw;
  const int n = m.n;
  if (tid == 0) bad_s = 0;

  // q0: one-hot in the start's labels (a label outside 0 .. K - 1: a row of zeros); theta1 its M-step, as the mixture's
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
    lb = hm_estep(sh, m, g, b, m.lr, fld, nullptr, nullptr, nullptr, &bad_s);   // lr holds q of the iteration before
    fail = gm_mstep(sh, m, reg, true, false);
    ++it;
    if (fail) break;
    if (fabs(lb - prev) < tol) { conv = 1; break; }
  }
  __syncthreads();
  const int bad = bad_s ? HM_BAD_INDEX : 0;
  if (fail) {
    if (tid == 0) {
      lower_bound_all[sr] = NAN; score_all[sr] = NAN; n_iter_all[sr] = it; converged_all[sr] = 0; status_all[sr] = 1 | bad;
    }
    for (int i = tid; i < n; i += GM_THREADS) lab[i] = -1;
    return;
  }
  // labels, log_resp and the field of the last q under the final parameters
  const double score = hm_estep(sh, m, g, b, m.lr, fld, lab, nullptr, nullptr, &bad_s);
  if (tid == 0) {
    lower_bound_all[sr] = lb; score_all[sr] = score; n_iter_all[sr] = it; converged_all[sr] = conv; status_all[sr] = bad;
  }
}

__global__ __launch_bounds__(GM_THREADS) void hmrf_estep_kernel(
    const double* __restrict__ z, long long ld, const long long* __restrict__ offsets, int D, const int* __restrict__ ks,
    int k_max, int type, long long rows, long long csz, const double* weights, const double* means, const double* prec,
    const double* __restrict__ resp_prev, const int* __restrict__ nbr, const double* __restrict__ wgt, int kw,
    const double* __restrict__ beta, double* field, double* log_resp, double* resp, int* labels, double* log_prob_norm,
    double* log_prior_norm, double* score, int* status) {
  __shared__ GmShared sh;
  __shared__ int bad_s;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long r0 = offsets[s];
  const long long nl = offsets[s + 1] - r0;
  const int K = ks[s];
  const double b = beta[s];
  if (nl < 1 || nl > HM_MAX_ROWS || r0 < 0 || r0 + nl > rows || K < 1 || K > k_max || !(b >= 0.0) || !(b < INFINITY)) {
    if (tid == 0) { score[s] = NAN; status[s] = 2; }
    return;
  }
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
  HmGraph g;
  g.nbr = nbr + r0 * kw; g.w = wgt + r0 * kw; g.kw = kw;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  const double sc = hm_estep(sh, m, g, b, resp_prev + r0 * k_max, field + r0 * k_max, labels + r0, resp + r0 * k_max,
                             log_prior_norm + r0, &bad_s);
  if (tid == 0) { score[s] = sc; status[s] = bad_s ? HM_BAD_INDEX : 0; }
}

// One synchronous round of majority relabelling; one thread per spot, the kept neighbours' labels staged in LDS (one
// column per thread) and counted pairwise, so no label range is needed.
__global__ __launch_bounds__(RF_THREADS) void label_refine_kernel(
    const long long* __restrict__ offsets, long long rows, const int* __restrict__ labels, const int* __restrict__ nbr,
    const double* __restrict__ wgt, int kw, int* __restrict__ out, int* __restrict__ changed) {
  __shared__ int nl[HM_MAX_KW][RF_THREADS];
  __shared__ int count_s;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long r0 = offsets[s];
  const long long nrows = offsets[s + 1] - r0;
  if (tid == 0) count_s = 0;
  __syncthreads();
  if (nrows < 1 || nrows > HM_MAX_ROWS || r0 < 0 || r0 + nrows > rows) {
    if (tid == 0) changed[s] = -1;
    return;
  }
  const int n = (int)nrows;
  const int* ls = labels + r0;
  int mine = 0;
  for (int i = tid; i < n; i += RF_THREADS) {
    const int l = ls[i];
    const int* nb = nbr + (r0 + i) * kw;
    const double* wr = wgt + (r0 + i) * kw;
    int m = 0;
    for (int c = 0; c < kw; ++c) {
      const int j = nb[c];
      const double wv = wr[c];
      const bool in = j >= 0 && j < n;
      const int lj = ls[in ? j : 0];
      if (wv != 0.0 && in && lj >= 0) nl[m++][tid] = lj;
    }
    int res = l;
    if (l >= 0) {
      int own = 1, top = l;
      for (int c = 0; c < m; ++c) own += nl[c][tid] == l;
      int top_n = own;
      for (int c = 0; c < m; ++c) {
        const int lc = nl[c][tid];
        int cnt = lc == l;
        for (int d = 0; d < m; ++d) cnt += nl[d][tid] == lc;
        if (cnt > top_n || (cnt == top_n && lc < top)) { top_n = cnt; top = lc; }
      }
      if (2 * own < m && 2 * top_n > m) res = top;
    }
    out[r0 + i] = res;
    mine += res != l;
  }
  if (mine) atomicAdd(&count_s, mine);
  __syncthreads();
  if (tid == 0) changed[s] = count_s;
}

// out[s] = (sum_i sum_c w_ic [l_i = l_nbr], sum_i sum_c w_ic) over the kept slots whose two labels are >= 0: slots ascending
// within a row, the rows in gm_block_sum's order
__global__ __launch_bounds__(GM_THREADS) void edge_agreement_kernel(
    const long long* __restrict__ offsets, long long rows, const int* __restrict__ labels, const int* __restrict__ nbr,
    const double* __restrict__ wgt, int kw, double* __restrict__ out) {
  __shared__ double red[GM_THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long r0 = offsets[s];
  const long long nrows = offsets[s + 1] - r0;
  if (nrows < 1 || nrows > HM_MAX_ROWS || r0 < 0 || r0 + nrows > rows) {
    if (tid == 0) { out[2 * s] = NAN; out[2 * s + 1] = NAN; }
    return;
  }
  const int n = (int)nrows;
  const int* ls = labels + r0;
  double agree = 0.0, total = 0.0;
  for (int i = tid; i < n; i += GM_THREADS) {
    const int l = ls[i];
    const int* nb = nbr + (r0 + i) * kw;
    const double* wr = wgt + (r0 + i) * kw;
    double a = 0.0, t = 0.0;
    for (int c = 0; c < kw; ++c) {
      const int j = nb[c];
      const double wv = wr[c];
      const bool in = j >= 0 && j < n;
      const int lj = ls[in ? j : 0];
      if (wv != 0.0 && in && l >= 0 && lj >= 0) {
        t += wv;
        if (lj == l) a += wv;
      }
    }
    agree += a;
    total += t;
  }
  const double sa = gm_block_sum(agree, red);
  const double st = gm_block_sum(total, red);
  if (tid == 0) { out[2 * s] = sa; out[2 * s + 1] = st; }
}

bool hm_shape_ok(int32_t S, int64_t rows, int32_t D, int32_t k_max, int32_t type, int32_t kw) {
  return S >= 1 && rows >= 1 && D >= 1 && k_max >= 1 && type >= GM_FULL && type <= GM_SPHERICAL && kw >= 1;
}

}  // namespace

// --------------------------------------------------------------------------------------------------------- entry points
extern "C" int64_t mcl_hmrf_workspace_bytes(int64_t rows, int32_t S, int32_t R, int32_t D, int32_t k_max) {
  if (rows < 1 || S < 1 || R < 1 || D < 1 || D > GM_MAX || k_max < 1 || k_max > GM_MAX) return -1;
  return 8 * hm_work_doubles(rows, S, R, D, k_max);
}

extern "C" int mcl_hmrf_fit(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                            const int32_t* k, int32_t k_max, int32_t R, int32_t covariance_type,
                            const int32_t* init_labels, const int32_t* nbr, const double* w, int32_t kw, const double* beta,
                            double tol, int32_t max_iter, double reg_covar, void* work, int64_t work_bytes,
                            int32_t* labels_all, double* weights_all, double* means_all, double* covariances_all,
                            double* precisions_cholesky_all, double* lower_bound_all, double* score_all,
                            int32_t* n_iter_all, int32_t* converged_all, int32_t* status_all, mcl_stream_t stream) {
  if (!z || !offsets || !k || !init_labels || !nbr || !w || !beta || !work || !labels_all || !weights_all || !means_all ||
      !covariances_all || !precisions_cholesky_all || !lower_bound_all || !score_all || !n_iter_all || !converged_all ||
      !status_all)
    return MCL_EINVAL;
  if (!hm_shape_ok(S, rows, D, k_max, covariance_type, kw) || R < 1 || ld < D || max_iter < 1 || !(tol >= 0.0) ||
      !(reg_covar >= 0.0))
    return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || kw > HM_MAX_KW || S > 65535) return MCL_EUNSUPPORTED;
  if (work_bytes < 8 * hm_work_doubles(rows, S, R, D, k_max)) return MCL_EWORKSPACE;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hmrf_fit_kernel, dim3(R, S), dim3(GM_THREADS), 0, mcl_stream(stream), z, (long long)ld,
                     reinterpret_cast<const long long*>(offsets), S, D, (const int*)k, k_max, R, covariance_type,
                     (const int*)init_labels, (const int*)nbr, w, kw, beta, tol, max_iter, reg_covar, (long long)rows,
                     gm_cov_size(covariance_type, k_max, D), work, labels_all, weights_all, means_all, covariances_all,
                     precisions_cholesky_all, lower_bound_all, score_all, n_iter_all, converged_all, status_all);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_hmrf_estep(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                              const int32_t* k, int32_t k_max, int32_t covariance_type, const double* weights,
                              const double* means, const double* precisions_cholesky, const double* resp_prev,
                              const int32_t* nbr, const double* w, int32_t kw, const double* beta, double* field,
                              double* log_resp, double* resp, int32_t* labels, double* log_prob_norm,
                              double* log_prior_norm, double* score, int32_t* status, mcl_stream_t stream) {
  if (!z || !offsets || !k || !weights || !means || !precisions_cholesky || !resp_prev || !nbr || !w || !beta || !field ||
      !log_resp || !resp || !labels || !log_prob_norm || !log_prior_norm || !score || !status)
    return MCL_EINVAL;
  if (!hm_shape_ok(S, rows, D, k_max, covariance_type, kw) || ld < D) return MCL_EINVAL;
  if (D > GM_MAX || k_max > GM_MAX || kw > HM_MAX_KW || S > 65535) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(hmrf_estep_kernel, dim3(S), dim3(GM_THREADS), 0, mcl_stream(stream), z, (long long)ld,
                     reinterpret_cast<const long long*>(offsets), D, (const int*)k, k_max, covariance_type, (long long)rows,
                     gm_cov_size(covariance_type, k_max, D), weights, means, precisions_cholesky, resp_prev,
                     (const int*)nbr, w, kw, beta, field, log_resp, resp, labels, log_prob_norm, log_prior_norm, score,
                     status);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_label_refine(const int64_t* offsets, int32_t S, int64_t rows, const int32_t* labels, const int32_t* nbr,
                                const double* w, int32_t kw, int32_t* labels_out, int32_t* changed, mcl_stream_t stream) {
  if (!offsets || !labels || !nbr || !w || !labels_out || !changed) return MCL_EINVAL;
  if (S < 1 || rows < 1 || kw < 1 || labels == labels_out) return MCL_EINVAL;
  if (kw > HM_MAX_KW || S > 65535) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(label_refine_kernel, dim3(S), dim3(RF_THREADS), 0, mcl_stream(stream),
                     reinterpret_cast<const long long*>(offsets), (long long)rows, (const int*)labels, (const int*)nbr, w, kw,
                     labels_out, changed);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_edge_agreement(const int64_t* offsets, int32_t S, int64_t rows, const int32_t* labels,
                                  const int32_t* nbr, const double* w, int32_t kw, double* sums, mcl_stream_t stream) {
  if (!offsets || !labels || !nbr || !w || !sums) return MCL_EINVAL;
  if (S < 1 || rows < 1 || kw < 1) return MCL_EINVAL;
  if (kw > HM_MAX_KW || S > 65535) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(edge_agreement_kernel, dim3(S), dim3(GM_THREADS), 0, mcl_stream(stream),
                     reinterpret_cast<const long long*>(offsets), (long long)rows, (const int*)labels, (const int*)nbr, w, kw,
                     sums);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
