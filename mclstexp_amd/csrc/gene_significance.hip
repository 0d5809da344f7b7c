// Gene-level significance of expression predictions: the second output of the reference's get_R (utils.py:52-65,
// scipy.stats.pearsonr's two-sided p-value) and the table tutorial.ipynb's third cell builds on it (genes x slides of
// -log10 p, its skipna row mean, the genes sorted by that mean, the best slide of every gene).
//
// scipy's p is 2 * I_x(a, a) with a = n / 2 - 1, x = (1 - |r|) / 2 (the beta(a, a) distribution of r on [-1, 1]).  Here
// log p is evaluated directly, so -log10 p stays finite where p itself underflows fp64:
//   log p = log 2 + [lgamma(2a) - 2 lgamma(a) + a log x + a log1p(-x) - log a] + log cf(a, a, x)
// cf = the continued fraction of the incomplete beta function by the modified Lentz recurrence; x <= 1/2 =
// (a + 1) / (2a + 2) always, the side from which it converges.
//
// Three launches in two entry points, all fp64, deterministic and atomics-free; no workgroup hands data to another inside
// a launch:
//   pearson_pvalue_kernel  grid (ceil(G/256), S): one lane per (slide, gene), lane = gene (a row's loads coalesce); every
//                          element is a function of (r, n) alone: a slide inside a batch is bit-identical to it alone.
//   gene_row_kernel        one lane per gene, slides walked in index order: skipna mean, count, first row maximum.
//   gene_order_kernel      gridded over genes: the exact descending rank of every gene by counting against all G means
//                          (staged through LDS in tiles), ties to the lower gene index, NaN means last.
#include "common.h"
#include "stats.h"
#include "betacf.h"   // log_betacf_sym, CF_MAX_ITER

namespace {

constexpr int PV_THREADS = 256;
constexpr int RANK_THREADS = 256;
constexpr int MAX_GENES = 1048576;

__global__ __launch_bounds__(PV_THREADS) void pearson_pvalue_kernel(const double* __restrict__ r_all,
                                                                    const long long* __restrict__ offsets, int G,
                                                                    double* __restrict__ p_out,
                                                                    double* __restrict__ nl_out) {
  const int s = blockIdx.y;
  const int g = blockIdx.x * PV_THREADS + threadIdx.x;
  if (g >= G) return;
  const long long n = offsets[s + 1] - offsets[s];
  const long long o = (long long)s * G + g;
  const double r = r_all[o];
  double p, nl;
  if (isnan(r) || n < 2) {
    p = NAN; nl = NAN;
  } else if (n == 2) {                 // scipy: two points always correlate perfectly, p = 1
    p = 1.0; nl = 0.0;
  } else if (fabs(r) >= 1.0) {
    p = 0.0; nl = INFINITY;
  } else {
    const double a = 0.5 * (double)n - 1.0;
    const double x = 0.5 * (1.0 - fabs(r));
    const double pre = lgamma(2.0 * a) - 2.0 * lgamma(a) + a * log(x) + a * log1p(-x) - log(a);
    double lp = stats::LN2 + pre + log_betacf_sym(a, x);
    lp = lp > 0.0 ? 0.0 : lp;          // p <= 1 (rounding at r ~ 0); NaN passes through
    nl = 0.0 - lp / stats::LN10;
    p = exp(lp);
  }
  p_out[o] = p;
  nl_out[o] = nl;
}

__global__ __launch_bounds__(RANK_THREADS) void gene_row_kernel(const double* __restrict__ nl,
                                                                const double* __restrict__ r, int S, int G,
                                                                double* __restrict__ mean, int* __restrict__ n_defined,
                                                                int* __restrict__ best_slide,
                                                                double* __restrict__ best_value,
                                                                double* __restrict__ best_r) {
  const int g = blockIdx.x * RANK_THREADS + threadIdx.x;
  if (g >= G) return;
  double sum = 0.0, best = NAN;
  int cnt = 0, arg = -1;
  for (int s = 0; s < S; ++s) {
    const double v = nl[(long long)s * G + g];
    if (isnan(v)) continue;
    sum += v;
    ++cnt;
    if (arg < 0 || v > best) {         // strict: the first slide that attains the maximum (pandas idxmax)
      best = v;
      arg = s;
    }
  }
  mean[g] = cnt ? sum / (double)cnt : NAN;
  n_defined[g] = cnt;
  best_slide[g] = arg;
  best_value[g] = best;
  best_r[g] = arg >= 0 ? r[(long long)arg * G + g] : NAN;
}

// (mj, gj) sorts before (m, g): descending mean, NaN last, equal keys by ascending gene index
__device__ __forceinline__ int sorts_before(double mj, int gj, double m, int g) {
  const bool nj = isnan(mj), nm = isnan(m);
  if (nj || nm) return (!nj && nm) || (nj && nm && gj < g);
  return (mj > m) || (mj == m && gj < g);
}

// (the counting loop is written out in every kernel that has it: stats.h says why it holds no shared form)
__global__ __launch_bounds__(RANK_THREADS) void gene_order_kernel(const double* __restrict__ mean, int G,
                                                                  long long* __restrict__ order) {
  __shared__ double tile[RANK_THREADS];
  const int g = blockIdx.x * RANK_THREADS + threadIdx.x;
  const double m = mean[g < G ? g : G - 1];
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += RANK_THREADS) {
    const int j = j0 + threadIdx.x;
    tile[threadIdx.x] = mean[j < G ? j : G - 1];
    __syncthreads();
    const int cnt = min(RANK_THREADS, G - j0);
    for (int k = 0; k < cnt; ++k) rank += sorts_before(tile[k], j0 + k, m, g);
    __syncthreads();
  }
  if (g < G) order[rank] = g;          // the ranks are a permutation of 0 .. G-1: every slot is written once
}

}  // namespace

extern "C" int mcl_pearson_pvalue(const double* r, const int64_t* offsets, int32_t S, int32_t G, double* p,
                                  double* neglog10p, mcl_stream_t stream) {
  if (!r || !offsets || !p || !neglog10p) return MCL_EINVAL;
  if (S < 1 || G < 1) return MCL_EINVAL;
  if (S > 65535 || G > MAX_GENES) return MCL_EUNSUPPORTED;  // grid.y; the gene bound of the preprocessing entry points
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(pearson_pvalue_kernel, dim3((G + PV_THREADS - 1) / PV_THREADS, S), dim3(PV_THREADS), 0,
                     mcl_stream(stream), r, reinterpret_cast<const long long*>(offsets), G, p, neglog10p);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

extern "C" int mcl_gene_rank(const double* neglog10p, const double* r, int32_t S, int32_t G, int32_t top_n, double* mean,
                             int32_t* n_defined, int64_t* order, int32_t* best_slide, double* best_value, double* best_r,
                             mcl_stream_t stream) {
  if (!neglog10p || !r || !mean || !n_defined || !order || !best_slide || !best_value || !best_r) return MCL_EINVAL;
  if (S < 1 || G < 1 || top_n < 1 || top_n > G) return MCL_EINVAL;
  if (S > 65535 || G > MAX_GENES) return MCL_EUNSUPPORTED;
  const hipStream_t st = mcl_stream(stream);
  const int blocks = (G + RANK_THREADS - 1) / RANK_THREADS;
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(gene_row_kernel, dim3(blocks), dim3(RANK_THREADS), 0, st, neglog10p, r, S, G, mean, n_defined,
                     best_slide, best_value, best_r);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gene_order_kernel, dim3(blocks), dim3(RANK_THREADS), 0, st, mean, G,
                     reinterpret_cast<long long*>(order));
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
