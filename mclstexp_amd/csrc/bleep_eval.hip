// BLEEP's prediction methods and scoring protocol (/root/reference/baselines/Bleep/BLEEP_inference.ipynb, cells 5 and 7):
// the three ways it turns the cosine top-k into a prediction (simple / average / weighted_average), its scoring block
// (correlation across cells, highly expressed genes by sum, highly variable genes by variance, marker genes, the maximum gene
// correlation) and the normalisation of the gene-gene-correlation matrices.  The per-gene Pearson r itself is
// mcl_expr_metrics' (eval_metrics.hip) and the Gram matrix behind the gene-gene correlation is mcl_pca_gram's (cluster.hip).
//
//   knn_combine_kernel       one workgroup per query: neighbour ids and fp64 weights in LDS, squared distances by wave, then a
//                            thread owns a column (or four adjacent ones: 16-byte loads where the rows allow them) and the k
//                            neighbour rows stream past it, 8 loads in flight, fp64 accumulation
//   cell_pearson_kernel      one wave per row, two passes over its G genes, fp64
//   truth_gene_stats_kernel  grid (ceil(G/64), S), lane = gene: column sums and population variances, two passes, fp64
//   bleep_summary_kernel     one workgroup per segment: the n_top genes by sum and by variance (exact rank by counting, equal
//                            values to the HIGHER gene index: the tail of a stable argsort) and the seven summaries
//   corr_from_gram_kernel    elementwise
// No floating-point atomics; every reduction order depends only on the problem's own shape (k, dim, G, the segment's length):
// a segment scored inside a batch is bit-identical to the same segment scored alone.
#include "common.h"
#include "stats.h"

namespace {

// ------------------------------------------------------------------------------------------------------ mcl_knn_combine
constexpr int KC_THREADS = 256;
constexpr int KC_INFLIGHT = 8;               // neighbour rows loaded before the first is consumed
constexpr int KC_MAX_LDS = (60000 / 8) * 12; // k doubles + k ints at the largest k the entry point takes
enum { KC_FIRST = 0, KC_MEAN = 1, KC_BLEEP_EXP = 2 };

template <int V>
struct kc_vec {
  typedef float type __attribute__((ext_vector_type(V)));
};
template <>
struct kc_vec<1> {
  typedef float type;
};
template <int V>
__device__ __forceinline__ float kc_elem(const typename kc_vec<V>::type& v, int e) { return v[e]; }
template <>
__device__ __forceinline__ float kc_elem<1>(const float& v, int) { return v; }

// dst[c] = sum_j w_j src[nbr_j, c] / tot for the columns [c0, c0 + V * nvec): a thread owns V adjacent columns, the k rows
// stream past it.  Per column the sum runs over four interleaved partial sums (j mod 4), combined (a0 + a1) + (a2 + a3): the
// same order whatever V is.  A trip past k repeats row k-1 and adds an exact zero.
template <int V>
__device__ __forceinline__ void kc_columns(const float* __restrict__ src, long long ld, int c0, int nvec,
                                           const int* nbr, const double* wgt, int k, bool weighted, double tot,
                                           float* __restrict__ dst) {
  typedef typename kc_vec<V>::type vec_t;
  for (int i = threadIdx.x; i < nvec; i += KC_THREADS) {
    const int c = c0 + i * V;
    double a[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < V; ++e) a[u][e] = 0.0;
    for (int j0 = 0; j0 < k; j0 += KC_INFLIGHT) {
      vec_t v[KC_INFLIGHT];
      double w[KC_INFLIGHT];
#pragma unroll
      for (int u = 0; u < KC_INFLIGHT; ++u) {
        const int j = min(j0 + u, k - 1);
        v[u] = *reinterpret_cast<const vec_t*>(src + (long long)nbr[j] * ld + c);
        w[u] = weighted ? wgt[j] : 1.0;
      }
#pragma unroll
      for (int u = 0; u < KC_INFLIGHT; ++u) {
        const bool ok = j0 + u < k;
#pragma unroll
        for (int e = 0; e < V; ++e) a[u & 3][e] += ok ? w[u] * (double)kc_elem<V>(v[u], e) : 0.0;
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) dst[c + e] = (float)(((a[0][e] + a[1][e]) + (a[2][e] + a[3][e])) / tot);
  }
}

__global__ __launch_bounds__(KC_THREADS) void knn_combine_kernel(
    const float* __restrict__ spot_key, long long ldk, const float* __restrict__ expression_key, long long lde,
    const float* __restrict__ query, long long ldq, const long long* __restrict__ indices, int k, int dim, int genes,
    int mode, float* __restrict__ emb_pred, float* __restrict__ expr_pred) {
  extern __shared__ unsigned char smem[];
  double* wgt = reinterpret_cast<double*>(smem);   // k
  int* nbr = reinterpret_cast<int*>(wgt + k);       // k
  __shared__ double red[KC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = blockIdx.x;

  if (mode == KC_FIRST) {  // the best match's rows, moved as they are
    const long long n0 = indices[(long long)qi * k];
    if (emb_pred)
      for (int c = tid; c < dim; c += KC_THREADS) emb_pred[(long long)qi * dim + c] = spot_key[n0 * ldk + c];
    if (expr_pred)
      for (int c = tid; c < genes; c += KC_THREADS) expr_pred[(long long)qi * genes + c] = expression_key[n0 * lde + c];
    return;
  }

  for (int j = tid; j < k; j += KC_THREADS) nbr[j] = (int)indices[(long long)qi * k + j];
  __syncthreads();
  double tot = (double)k;
  if (mode == KC_BLEEP_EXP) {
    // d_j = sum (key[idx_j] - q)^2 on the un-normalised embeddings; w_j = exp(-(d_j - d_0 + 1)), d_0 = the best COSINE match's
    const float* q = query + (long long)qi * ldq;
    for (int j = wave; j < k; j += KC_THREADS / 64) {
      const float* r = spot_key + (long long)nbr[j] * ldk;
      double acc = 0.0;
      for (int c = lane; c < dim; c += 64) {
        const double d = (double)r[c] - (double)q[c];
        acc = fma(d, d, acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) wgt[j] = acc;
    }
    __syncthreads();
    const double d0 = wgt[0];
    __syncthreads();
    tot = 0.0;
    for (int j = tid; j < k; j += KC_THREADS) {
      const double w = exp(-(wgt[j] - d0 + 1.0));
      wgt[j] = w;
      tot += w;
    }
    tot = wave_sum(tot);
    if (lane == 0) red[wave] = tot;
    __syncthreads();
    tot = 0.0;
#pragma unroll
    for (int w = 0; w < KC_THREADS / 64; ++w) tot += red[w];
  }
  const bool weighted = mode == KC_BLEEP_EXP;

  for (int pass = 0; pass < 2; ++pass) {
    const float* src = pass ? expression_key : spot_key;
    const long long ld = pass ? lde : ldk;
    const int cols = pass ? genes : dim;
    float* dst = pass ? expr_pred + (long long)qi * genes : emb_pred + (long long)qi * dim;
    if ((pass ? expr_pred : emb_pred) == nullptr) continue;
    // 16-byte loads need every row to start on a 16-byte boundary
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<unsigned long long>(src) & 15ull) == 0);
    const int nv = vec ? cols / 4 : 0;
    if (nv) kc_columns<4>(src, ld, 0, nv, nbr, wgt, k, weighted, tot, dst);
    kc_columns<1>(src, ld, nv * 4, cols - nv * 4, nbr, wgt, k, weighted, tot, dst);
  }
}

// ----------------------------------------------------------------------------------------------------- mcl_cell_pearson
template <typename TP, typename TT>
__global__ __launch_bounds__(256) void cell_pearson_kernel(const TP* __restrict__ pred, long long ldp,
                                                           const TT* __restrict__ tru, long long ldt, long long rows, int G,
                                                           double* __restrict__ r_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TP* p = pred + row * ldp;
  const TT* t = tru + row * ldt;
  double sp = 0.0, st = 0.0;
  double pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
  for (int g = lane; g < G; g += 64) {
    const double pv = ldd(p + g), tv = ldd(t + g);
    sp += pv;
    st += tv;
    pmin = fmin(pmin, pv); pmax = fmax(pmax, pv);
    tmin = fmin(tmin, tv); tmax = fmax(tmax, tv);
  }
  sp = wave_sum(sp);
  st = wave_sum(st);
  pmin = wave_min(pmin); pmax = wave_max(pmax);
  tmin = wave_min(tmin); tmax = wave_max(tmax);
  const double pm = sp / (double)G, tm = st / (double)G;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int g = lane; g < G; g += 64) {
    const double dp = ldd(p + g) - pm, dt = ldd(t + g) - tm;
    sxy = fma(dp, dt, sxy);
    sxx = fma(dp, dp, sxx);
    syy = fma(dt, dt, syy);
  }
  sxy = wave_sum(sxy);
  sxx = wave_sum(sxx);
  syy = wave_sum(syy);
  if (lane == 0) {
    const bool constant = (pmin == pmax) || (tmin == tmax);
    const double r = sxy / (sqrt(sxx) * sqrt(syy));
    r_out[row] = constant ? NAN : fmin(fmax(r, -1.0), 1.0);   // np.corrcoef clips
  }
}

template <typename TP, typename TT>
void launch_cell_pearson(const void* pred, long long ldp, const void* tru, long long ldt, long long rows, int G, double* r,
                         hipStream_t st) {
  hipLaunchKernelGGL((cell_pearson_kernel<TP, TT>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                     static_cast<const TP*>(pred), ldp, static_cast<const TT*>(tru), ldt, rows, G, r);
}

// ---------------------------------------------------------------------------------------------------- mcl_bleep_summary
constexpr int GS_WAVES = 4;
constexpr int GS_UNROLL = 4;      // rows per wave per trip
constexpr int BS_THREADS = 256;

// np.sum(true, axis=0) and np.var(true, axis=0) of one segment: lane = gene, the waves stride over the rows
template <typename TT>
__global__ __launch_bounds__(GS_WAVES * 64) void truth_gene_stats_kernel(const TT* __restrict__ tru, long long ldt,
                                                                         const long long* __restrict__ offsets, int G,
                                                                         double* __restrict__ sum_out,
                                                                         double* __restrict__ var_out) {
  __shared__ double part[GS_WAVES][64];
  __shared__ double mean_s[64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int g = blockIdx.x * 64 + lane;
  const int gc = g < G ? g : G - 1;  // lanes past G load column G-1 and store nothing
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  const long long last = r1 - 1;
  const TT* tc = tru + gc;
  constexpr int STEP = GS_WAVES * GS_UNROLL;
  const double n = (double)(r1 - r0);

  double st = 0.0;
  for (long long base = r0 + w; base < r1; base += STEP) {
    double tv[GS_UNROLL];
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) tv[u] = ldd(tc + min(base + (long long)u * GS_WAVES, last) * ldt);
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) st += (base + (long long)u * GS_WAVES < r1) ? tv[u] : 0.0;
  }
  part[w][lane] = st;
  __syncthreads();
  if (w == 0) {
    for (int v = 1; v < GS_WAVES; ++v) st += part[v][lane];   // fixed order: wave 0 + 1 + 2 + 3
    mean_s[lane] = st / n;
  }
  __syncthreads();
  const double tm = mean_s[lane];
  double sq = 0.0;
  for (long long base = r0 + w; base < r1; base += STEP) {
    double tv[GS_UNROLL];
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) tv[u] = ldd(tc + min(base + (long long)u * GS_WAVES, last) * ldt);
#pragma unroll
    for (int u = 0; u < GS_UNROLL; ++u) {
      const double d = (base + (long long)u * GS_WAVES < r1) ? tv[u] - tm : 0.0;
      sq = fma(d, d, sq);
    }
  }
  part[w][lane] = sq;
  __syncthreads();
  if (w == 0 && g < G) {
    for (int v = 1; v < GS_WAVES; ++v) sq += part[v][lane];
    sum_out[(long long)s * G + g] = st;
    var_out[(long long)s * G + g] = sq / n;
  }
}

__global__ __launch_bounds__(BS_THREADS) void bleep_summary_kernel(
    const long long* __restrict__ offsets, int G, int n_top, const double* __restrict__ r_gene_all,
    const double* __restrict__ r_cell, const int* __restrict__ markers, int n_markers,
    const double* __restrict__ gene_sum, const double* __restrict__ gene_var, long long* __restrict__ top_sum_all,
    long long* __restrict__ top_var_all, double* __restrict__ summary) {
  __shared__ stats::top_lds<BS_THREADS> L;
  __shared__ double red[8][BS_THREADS];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const double* rr = r_gene_all + (long long)s * G;
  long long* top_sum = top_sum_all + (long long)s * n_top;
  long long* top_var = top_var_all + (long long)s * n_top;
  // equal values to the HIGHER gene index; a rank that no gene reaches (non-finite values only) stays -1
  for (int i = tid; i < n_top; i += BS_THREADS) top_sum[i] = -1;
  stats::top_select<stats::DESCENDING_HIGH>(gene_sum + (long long)s * G, G, n_top, top_sum, L);
  for (int i = tid; i < n_top; i += BS_THREADS) top_var[i] = -1;
  stats::top_select<stats::DESCENDING_HIGH>(gene_var + (long long)s * G, G, n_top, top_var, L);

  // per-thread strided sums, then a fixed LDS tree
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  double a_cell = 0.0, n_cell = 0.0, n_gene = 0.0, mx = -INFINITY, a_heg = 0.0, a_hvg = 0.0, a_mark = 0.0;
  for (long long i = r0 + tid; i < r1; i += BS_THREADS) {
    const double v = r_cell[i];
    if (!isnan(v)) {
      a_cell += v;
      n_cell += 1.0;
    }
  }
  for (int g = tid; g < G; g += BS_THREADS) {
    const double v = rr[g];
    if (!isnan(v)) {
      n_gene += 1.0;
      mx = fmax(mx, v);
    }
  }
  for (int i = tid; i < n_top; i += BS_THREADS) {  // NaN propagates (np.mean)
    const long long h = top_sum[i], v = top_var[i];
    a_heg += (h >= 0 && h < G) ? rr[h] : NAN;
    a_hvg += (v >= 0 && v < G) ? rr[v] : NAN;
  }
  for (int i = tid; i < n_markers; i += BS_THREADS) {
    const int m = markers[i];
    a_mark += (m >= 0 && m < G) ? rr[m] : NAN;
  }
  red[0][tid] = a_cell; red[1][tid] = n_cell; red[2][tid] = n_gene; red[3][tid] = mx;
  red[4][tid] = a_heg; red[5][tid] = a_hvg; red[6][tid] = a_mark;
  __syncthreads();
  for (int h = BS_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int q = 0; q < 7; ++q)
        red[q][tid] = (q == 3) ? fmax(red[q][tid], red[q][tid + h]) : red[q][tid] + red[q][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* out = summary + 7 * (long long)s;
    const double nc = red[1][0], ng = red[2][0];
    out[0] = nc > 0.0 ? red[0][0] / nc : NAN;      // np.mean of an empty array
    out[1] = nc;
    out[2] = ng;
    out[3] = ng > 0.0 ? red[3][0] : NAN;
    out[4] = red[4][0] / n_top;
    out[5] = red[5][0] / n_top;
    out[6] = n_markers > 0 ? red[6][0] / n_markers : NAN;
  }
}

// --------------------------------------------------------------------------------------------------- mcl_corr_from_gram
__global__ __launch_bounds__(256) void corr_from_gram_kernel(const double* __restrict__ gram, int m, double* __restrict__ corr) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)m * m) return;
  const int i = (int)(e / m), j = (int)(e % m);
  const double gi = gram[(long long)i * m + i], gj = gram[(long long)j * m + j];
  const double c = gram[e] / sqrt(gi) / sqrt(gj);            // np.corrcoef: c / stddev[:, None] / stddev[None, :]
  corr[e] = (gi == 0.0 || gj == 0.0) ? NAN : fmin(fmax(c, -1.0), 1.0);
}

inline bool dtype_ok(int32_t d) { return d == 0 || d == 1; }

}  // namespace

extern "C" int mcl_knn_combine(const float* spot_key, int64_t ldk, const float* expression_key, int64_t lde,
                               const float* query, int64_t ldq, const int64_t* indices, int n_query, int k, int dim,
                               int genes, int mode, float* emb_pred, float* expr_pred, mcl_stream_t stream) {
  if (n_query == 0) return MCL_OK;
  if (!spot_key || !query || !indices || n_query < 0 || k <= 0 || dim <= 0 || ldk < dim || ldq < dim)
    return MCL_EINVAL;
  if ((expr_pred != nullptr) && (!expression_key || genes <= 0 || lde < genes)) return MCL_EINVAL;
  if (mode != KC_FIRST && mode != KC_MEAN && mode != KC_BLEEP_EXP) return MCL_EUNSUPPORTED;
  if ((size_t)k * 8 > 60000) return MCL_EUNSUPPORTED;
  static mcl_device_once attr_once;
  if (auto attr_guard = attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_combine_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, KC_MAX_LDS);
  }
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(knn_combine_kernel, dim3(n_query), dim3(KC_THREADS), (size_t)k * 12, mcl_stream(stream), spot_key,
                     (long long)ldk, expr_pred ? expression_key : nullptr, (long long)lde, query, (long long)ldq,
                     reinterpret_cast<const long long*>(indices), k, dim, genes, mode, emb_pred, expr_pred);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_cell_pearson(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                                int32_t true_dtype, int64_t rows, int32_t G, double* r_cell, mcl_stream_t stream) {
  if (rows == 0) return MCL_OK;
  if (!pred || !truth || !r_cell || rows < 0 || G < 1 || ld_pred < G || ld_true < G) return MCL_EINVAL;
  if (!dtype_ok(pred_dtype) || !dtype_ok(true_dtype)) return MCL_EINVAL;
  if ((rows + 3) / 4 > 0x7FFFFFFFLL) return MCL_EUNSUPPORTED;  // grid.x
  const hipStream_t st = mcl_stream(stream);
  MCL_CLEAR_ERROR();
  if (pred_dtype == 0 && true_dtype == 0)
    launch_cell_pearson<float, float>(pred, ld_pred, truth, ld_true, rows, G, r_cell, st);
  else if (pred_dtype == 0)
    launch_cell_pearson<float, double>(pred, ld_pred, truth, ld_true, rows, G, r_cell, st);
  else if (true_dtype == 0)
    launch_cell_pearson<double, float>(pred, ld_pred, truth, ld_true, rows, G, r_cell, st);
  else
    launch_cell_pearson<double, double>(pred, ld_pred, truth, ld_true, rows, G, r_cell, st);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_bleep_summary(const void* truth, int64_t ld_true, int32_t true_dtype, const int64_t* offsets, int32_t S,
                                 int32_t G, int32_t n_top, const double* r_gene, const double* r_cell,
                                 const int32_t* markers, int32_t n_markers, double* gene_sum, double* gene_var,
                                 int64_t* top_sum, int64_t* top_var, double* summary, mcl_stream_t stream) {
  if (S == 0) return MCL_OK;
  if (!truth || !offsets || !r_gene || !r_cell || !gene_sum || !gene_var || !top_sum || !top_var || !summary)
    return MCL_EINVAL;
  if (S < 0 || G < 1 || n_top < 1 || n_top > G || ld_true < G || !dtype_ok(true_dtype)) return MCL_EINVAL;
  if (n_markers < 0 || (n_markers > 0 && !markers)) return MCL_EINVAL;
  if (S > 65535 || G > 1048576) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  const dim3 grid((G + 63) / 64, S);
  if (true_dtype == 0)
    hipLaunchKernelGGL(truth_gene_stats_kernel<float>, grid, dim3(GS_WAVES * 64), 0, st, static_cast<const float*>(truth),
                       (long long)ld_true, off, G, gene_sum, gene_var);
  else
    hipLaunchKernelGGL(truth_gene_stats_kernel<double>, grid, dim3(GS_WAVES * 64), 0, st,
                       static_cast<const double*>(truth), (long long)ld_true, off, G, gene_sum, gene_var);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(bleep_summary_kernel, dim3(S), dim3(BS_THREADS), 0, st, off, G, n_top, r_gene, r_cell,
                     reinterpret_cast<const int*>(markers), n_markers, gene_sum, gene_var,
                     reinterpret_cast<long long*>(top_sum), reinterpret_cast<long long*>(top_var), summary);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_corr_from_gram(const double* gram, int32_t m, double* corr, mcl_stream_t stream) {
  if (m == 0) return MCL_OK;
  if (!gram || !corr || m < 0) return MCL_EINVAL;
  if (m > 32768) return MCL_EUNSUPPORTED;
  MCL_CLEAR_ERROR();
  const long long blocks = ((long long)m * m + 255) / 256;
  hipLaunchKernelGGL(corr_from_gram_kernel, dim3((unsigned)blocks), dim3(256), 0, mcl_stream(stream), gram, m, corr);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
