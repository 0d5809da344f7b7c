// Scoring of expression predictions (the closing block of /root/reference/evel_her2st.py:196-226, evel_cscc.py:226-261,
// evel_visium.py:212-244 with utils.py:52-65 get_R): per-gene Pearson r, the 50 highest-expressed genes (HEG), their mean r,
// the mean r over the non-NaN genes (HVG), MSE and MAE -- for S folds (row segments) in one call.
//
// Two launches, both deterministic and atomics-free; no workgroup hands data to another inside a launch:
//   expr_gene_stats_kernel  grid (ceil(G/64), S), 4 waves.  Lane = gene (a wave's loads of a row are coalesced), the waves
//                           stride over the segment's rows (4 rows in flight per wave per trip, loads from clamped row
//                           indices, the tail masked at the use).  Pass 1: sums of p, t, (t-p)^2, |t-p| and min / max of
//                           p and t; the four waves' partials are combined through LDS in wave order; pass 2 re-reads the
//                           segment for the centred sums S_pt, S_pp, S_tt.  fp64 throughout.
//   expr_summary_kernel     one workgroup per segment: the top-n_heg genes by true mean (exact rank by counting, ties to the
//                           lower gene index) and the fixed-order block reductions of the summary row.
// Every reduction order depends only on (segment length, G, n_heg): a fold scored inside a batch is bit-identical to the
// same fold scored alone.
#include "common.h"

namespace {

constexpr int STAT_WAVES = 4;
constexpr int STAT_UNROLL = 4;     // rows per wave per trip
constexpr int SUM_THREADS = 256;
// stats.h's TOP_SAMPLE / TOP_CAP for the top-n written out in expr_summary_kernel (the reason stands at heg_beats)
constexpr int HEG_SAMPLE = 256;    // genes in the sample that sets the candidate threshold
constexpr int HEG_CAP = 2048;      // candidates ranked in LDS; more -> ranked against all G means in global memory

// writes r, true_mean and the per-gene mean squared / absolute error (work[s][0][g], work[s][1][g])
template <typename TP, typename TT>
__global__ __launch_bounds__(STAT_WAVES * 64) void expr_gene_stats_kernel(
    const TP* __restrict__ pred, long long ldp, const TT* __restrict__ tru, long long ldt,
    const long long* __restrict__ offsets, int G, double* __restrict__ r_out, double* __restrict__ tmean_out,
    double* __restrict__ work) {
  __shared__ double part[8][STAT_WAVES][64];
  __shared__ double mean_s[2][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int g = blockIdx.x * 64 + lane;
  const int gc = g < G ? g : G - 1;  // lanes past G load column G-1 and store nothing
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  const long long last = r1 - 1;
  const TP* pc = pred + gc;
  const TT* tc = tru + gc;
  constexpr int STEP = STAT_WAVES * STAT_UNROLL;

  // ---- pass 1: sums, error sums, extremes.  A clamped row repeats row r1-1: harmless for min / max, masked for sums.
  double sp = 0.0, st = 0.0, se = 0.0, sa = 0.0;
  double pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
  for (long long base = r0 + w; base < r1; base += STEP) {
    double pv[STAT_UNROLL], tv[STAT_UNROLL];
#pragma unroll
    for (int u = 0; u < STAT_UNROLL; ++u) {
      const long long row = min(base + (long long)u * STAT_WAVES, last);
      pv[u] = ldd(pc + row * ldp);
      tv[u] = ldd(tc + row * ldt);
    }
#pragma unroll
    for (int u = 0; u < STAT_UNROLL; ++u) {
      const bool ok = base + (long long)u * STAT_WAVES < r1;
      const double d = tv[u] - pv[u];
      pmin = fmin(pmin, pv[u]); pmax = fmax(pmax, pv[u]);
      tmin = fmin(tmin, tv[u]); tmax = fmax(tmax, tv[u]);
      sp += ok ? pv[u] : 0.0;
      st += ok ? tv[u] : 0.0;
      se += ok ? d * d : 0.0;
      sa += ok ? fabs(d) : 0.0;
    }
  }
  part[0][w][lane] = sp; part[1][w][lane] = st; part[2][w][lane] = se; part[3][w][lane] = sa;
  part[4][w][lane] = pmin; part[5][w][lane] = pmax; part[6][w][lane] = tmin; part[7][w][lane] = tmax;
  __syncthreads();
  const double n = (double)(r1 - r0);
  bool constant = false;
  double tmean = 0.0;
  if (w == 0) {
    for (int v = 1; v < STAT_WAVES; ++v) {  // fixed order: wave 0 + wave 1 + wave 2 + wave 3
      sp += part[0][v][lane]; st += part[1][v][lane]; se += part[2][v][lane]; sa += part[3][v][lane];
      pmin = fmin(pmin, part[4][v][lane]); pmax = fmax(pmax, part[5][v][lane]);
      tmin = fmin(tmin, part[6][v][lane]); tmax = fmax(tmax, part[7][v][lane]);
    }
    constant = (pmin == pmax) || (tmin == tmax);
    tmean = st / n;
    mean_s[0][lane] = sp / n;
    mean_s[1][lane] = tmean;
  }
  __syncthreads();

  // ---- pass 2: centred sums (the one-pass sum-of-squares form cancels on sparse, low-variance columns)
  const double pm = mean_s[0][lane], tm = mean_s[1][lane];
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (long long base = r0 + w; base < r1; base += STEP) {
    double pv[STAT_UNROLL], tv[STAT_UNROLL];
#pragma unroll
    for (int u = 0; u < STAT_UNROLL; ++u) {
      const long long row = min(base + (long long)u * STAT_WAVES, last);
      pv[u] = ldd(pc + row * ldp);
      tv[u] = ldd(tc + row * ldt);
    }
#pragma unroll
    for (int u = 0; u < STAT_UNROLL; ++u) {
      const bool ok = base + (long long)u * STAT_WAVES < r1;
      const double dp = ok ? pv[u] - pm : 0.0;
      const double dt = ok ? tv[u] - tm : 0.0;
      sxy = fma(dp, dt, sxy);
      sxx = fma(dp, dp, sxx);
      syy = fma(dt, dt, syy);
    }
  }
  part[0][w][lane] = sxy; part[1][w][lane] = sxx; part[2][w][lane] = syy;
  __syncthreads();
  if (w == 0 && g < G) {
    for (int v = 1; v < STAT_WAVES; ++v) {
      sxy += part[0][v][lane]; sxx += part[1][v][lane]; syy += part[2][v][lane];
    }
    double r = sxy / (sqrt(sxx) * sqrt(syy));
    r = constant ? NAN : fmin(fmax(r, -1.0), 1.0);  // scipy.stats.pearsonr: NaN for a constant input, clipped
    const long long o = (long long)s * G + g;
    r_out[o] = r;
    tmean_out[o] = tmean;
    work[2 * (long long)s * G + g] = se / n;
    work[(2 * (long long)s + 1) * G + g] = sa / n;
  }
}

// (mj, gj) before (m, g): descending mean, equal means by ascending gene index.  With HEG_SAMPLE / HEG_CAP and steps 1 - 3
// of expr_summary_kernel this is stats.h's top_select<DESCENDING> written out: through the call the kernel's code changes
// (5512 -> 5676 bytes; 34 VGPRs, 90 SGPRs, 37912 bytes of LDS either way) and mcl_expr_metrics at 8 folds x 785 genes takes
// 47.9 - 48.6 us against 45.1 - 45.8 us.  heg[] arrives uninitialised (torch.empty) and is not prefilled: a rank stays
// unfilled only where means are non-finite, and the summary turns an entry outside [0, G) into NaN
__device__ __forceinline__ int heg_beats(double mj, int gj, double m, int g) { return (mj > m) || (mj == m && gj < g); }

__global__ __launch_bounds__(SUM_THREADS) void expr_summary_kernel(const double* __restrict__ r_all,
                                                                   const double* __restrict__ tmean_all,
                                                                   const double* __restrict__ work, int G, int n_heg,
                                                                   long long* __restrict__ heg_all,
                                                                   double* __restrict__ summary) {
  __shared__ double smp_m[HEG_SAMPLE];
  __shared__ int smp_g[HEG_SAMPLE];
  __shared__ double cand_m[HEG_CAP];
  __shared__ int cand_g[HEG_CAP];
  __shared__ double red[5][SUM_THREADS];
  __shared__ int wave_cnt[SUM_THREADS / 64];
  __shared__ double thr_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int s = blockIdx.x;
  const double* m = tmean_all + (long long)s * G;
  const double* rr = r_all + (long long)s * G;
  const double* mse_g = work + 2 * (long long)s * G;
  const double* mae_g = mse_g + G;
  long long* heg = heg_all + (long long)s * n_heg;

  // 1. threshold T = the n_heg-th largest mean of an evenly strided sample: the full set's n_heg-th largest is >= T, so
  //    every HEG gene has a mean >= T (T = -inf when the sample holds fewer than n_heg genes)
  const int ns = min(G, HEG_SAMPLE);
  if (tid == 0) thr_s = -INFINITY;
  if (tid < ns) {
    const int gs = (int)(((long long)tid * G) / ns);
    smp_m[tid] = m[gs];
    smp_g[tid] = gs;
  }
  __syncthreads();
  if (n_heg <= ns && tid < ns) {
    const double mt = smp_m[tid];
    const int gt = smp_g[tid];
    int rank = 0;
    for (int j = 0; j < ns; ++j) rank += heg_beats(smp_m[j], smp_g[j], mt, gt);
    if (rank == n_heg - 1) thr_s = mt;
  }
  __syncthreads();
  const double T = thr_s;

  // 2. candidates (mean >= T) compacted in gene order: ballot + a prefix over the waves, no atomics
  int count = 0;
  for (int g0 = 0; g0 < G; g0 += SUM_THREADS) {
    const int g = g0 + tid;
    const double mg = m[g < G ? g : G - 1];
    const bool f = g < G && mg >= T;
    const unsigned long long b = __ballot(f);
    if (lane == 0) wave_cnt[w] = __builtin_popcountll(b);
    __syncthreads();
    int before = count;
    for (int v = 0; v < w; ++v) before += wave_cnt[v];
    if (f) {
      const int pos = before + (int)lanes_below(b);
      if (pos < HEG_CAP) {
        cand_m[pos] = mg;
        cand_g[pos] = g;
      }
    }
    for (int v = 0; v < SUM_THREADS / 64; ++v) count += wave_cnt[v];
    __syncthreads();
  }

  // 3. exact rank of every candidate among the candidates (a non-candidate is strictly below every candidate)
  if (count <= HEG_CAP) {
    for (int c = tid; c < count; c += SUM_THREADS) {
      const double mc = cand_m[c];
      const int gc = cand_g[c];
      int rank = 0;
      for (int j = 0; j < count; ++j) rank += heg_beats(cand_m[j], cand_g[j], mc, gc);
      if (rank < n_heg) heg[rank] = gc;
    }
  } else {
    for (int g = tid; g < G; g += SUM_THREADS) {
      const double mg = m[g];
      if (!(mg >= T)) continue;
      int rank = 0;
      for (int j = 0; j < G; ++j) rank += heg_beats(m[j], j, mg, g);
      if (rank < n_heg) heg[rank] = g;
    }
  }
  __syncthreads();  // heg[] is read back below

  // 4. summary: per-thread strided sums, then a fixed LDS tree
  double a_heg = 0.0, a_hvg = 0.0, a_nv = 0.0, a_mse = 0.0, a_mae = 0.0;
  for (int i = tid; i < n_heg; i += SUM_THREADS) {  // NaN propagates (np.mean)
    const long long h = heg[i];
    a_heg += (h >= 0 && h < G) ? rr[h] : NAN;       // (a rank left unfilled only by non-finite means)
  }
  for (int g = tid; g < G; g += SUM_THREADS) {
    const double v = rr[g];
    if (!isnan(v)) {
      a_hvg += v;
      a_nv += 1.0;
    }
    a_mse += mse_g[g];
    a_mae += mae_g[g];
  }
  red[0][tid] = a_heg; red[1][tid] = a_hvg; red[2][tid] = a_nv; red[3][tid] = a_mse; red[4][tid] = a_mae;
  __syncthreads();
  for (int h = SUM_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* out = summary + 5 * (long long)s;
    const double nv = red[2][0];
    out[0] = red[0][0] / n_heg;
    out[1] = nv > 0.0 ? red[1][0] / nv : NAN;  // np.mean of an empty array
    out[2] = red[3][0] / G;
    out[3] = red[4][0] / G;
    out[4] = nv;
  }
}

template <typename TP, typename TT>
void launch_stats(const void* pred, long long ldp, const void* tru, long long ldt, const long long* offsets, int S, int G,
                  double* r, double* tmean, double* work, hipStream_t st) {
  hipLaunchKernelGGL((expr_gene_stats_kernel<TP, TT>), dim3((G + 63) / 64, S), dim3(STAT_WAVES * 64), 0, st,
                     static_cast<const TP*>(pred), ldp, static_cast<const TT*>(tru), ldt, offsets, G, r, tmean, work);
}

}  // namespace

extern "C" int mcl_expr_metrics(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                                int32_t true_dtype, const int64_t* offsets, int32_t S, int32_t G, int32_t n_heg, double* r,
                                double* true_mean, int64_t* heg, double* summary, double* work, mcl_stream_t stream) {
  if (!pred || !truth || !offsets || !r || !true_mean || !heg || !summary || !work) return MCL_EINVAL;
  if (S < 1 || G < 1 || n_heg < 1 || n_heg > G || ld_pred < G || ld_true < G) return MCL_EINVAL;
  if ((pred_dtype != 0 && pred_dtype != 1) || (true_dtype != 0 && true_dtype != 1)) return MCL_EINVAL;
  if (S > 65535) return MCL_EUNSUPPORTED;  // grid.y
  const hipStream_t st = mcl_stream(stream);
  const long long* off = reinterpret_cast<const long long*>(offsets);
  MCL_CLEAR_ERROR();
  if (pred_dtype == 0 && true_dtype == 0)
    launch_stats<float, float>(pred, ld_pred, truth, ld_true, off, S, G, r, true_mean, work, st);
  else if (pred_dtype == 0)
    launch_stats<float, double>(pred, ld_pred, truth, ld_true, off, S, G, r, true_mean, work, st);
  else if (true_dtype == 0)
    launch_stats<double, float>(pred, ld_pred, truth, ld_true, off, S, G, r, true_mean, work, st);
  else
    launch_stats<double, double>(pred, ld_pred, truth, ld_true, off, S, G, r, true_mean, work, st);
  MCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(expr_summary_kernel, dim3(S), dim3(SUM_THREADS), 0, st, r, true_mean, work, G, n_heg,
                     reinterpret_cast<long long*>(heg), summary);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}
