// Deterministic Leiden on the connectivities CSR of csrc/neighbors.hip (scanpy's sc.tl.leiden, RBConfiguration quality) for
// every segment (slide) of a batch; the arithmetic is the one DESIGN 6.13 states and tests/leiden_reference.py restates.
//
// Weights are fixed point: q = rint(w 2^e), e = 61 - ex - ceil(log2(nnz_s)) with the segment's largest weight below 2^ex, so
// every sum of weights (k_i, tot_c, k_ic, in_c, 2m <= 2^61) is an exact int64 and no order of summation, and no arrival order
// of an integer atomic, changes a bit.  Floating point enters only where converted integers are combined (gains, the
// well-connectedness tests, Q): one IEEE fp64 operation at a time, uncontracted, and the one fp64 sum (over communities, in
// Q) runs in a fixed order.  There are no floating-point atomics, no workgroup waits on another, a segment inside a batch is
// bit-identical to the same segment alone, and a run to its repeat.
//
//   mcl_leiden_init           ld_prepare (a workgroup per segment: wmax, e, the state record), ld_quantise (a wave per row:
//                             q, k_i, the start labels), ld_m2, then the tally and Q of the start partition.
//   mcl_leiden_move_sweeps    per sweep ld_zero_move, ld_sweep (one wave per vertex; k_ic in a wave-private LDS hash table
//                             with integer atomics for rows of up to LD_CUT entries, a dense int64 accumulator in the workspace
//                             that the row's wave owns for longer rows), ld_tally_move, ld_q_move (Q in the fixed order, and
//                             the acceptance: on the device, in the segment's state record).
//   mcl_leiden_refine_rounds  per round ld_zero_refine, ld_propose (the same two paths), ld_commit, ld_tally_refine, ld_q_refine.
//   mcl_leiden_aggregate      ld_agg_number (prefix sums in index order), ld_agg_map, ld_agg_rows twice (count, fill: the
//                             merged row lands in the dense accumulator and is read back in column order), ld_agg_indptr.
//   mcl_leiden_finish         labels of the original vertices, canonical ids, the renumbering by size.
//
// Segments ride on grid.y; a finished segment returns at once from every later launch.
#include <float.h>
#include <limits.h>
#include "common.h"

namespace {

constexpr int LD_MAX_N = 16384;
constexpr int LD_MAX_S = 65535;                 // grid.y
constexpr int LD_CUT = 512;                     // rows longer than this take the dense path
constexpr int LD_SLOTS = 1024;                  // hash slots per wave: at most LD_CUT keys, load <= 1/2
constexpr int LD_DENSE = 256;                   // waves of the dense path, each owning max_n int64 of the workspace
constexpr int LD_THREADS = 256;

// per-segment state record: 128 bytes, read by the host between batches of launches (mclstexp_amd/leiden.py: STATE)
enum { F_N, F_SHIFT, F_CUR, F_RCUR, F_PARITY, F_FAILS, F_MOVE_DONE, F_REF_DONE, F_FINISHED, F_LEVEL_ACC, F_SWEEPS, F_ACCEPTED,
       F_ROUNDS, F_LEVELS, F_PHASE, F_ERROR, F_N_NEXT, F_MAX_ROW, F_N0, F_CLUSTERS, F_COUNT = 24 };
struct ld_state {
  double Q, QR;
  long long m2, in_new;
  int f[F_COUNT];
};
static_assert(sizeof(ld_state) == 128, "state record");

struct ld_work {
  ld_state* st;                 // S
  long long* q0;                // nnz
  long long* ipL[2];            // rows + S
  long long* qL[2];             // nnz + rows
  long long* kk[2];             // rows
  long long* tot[2];
  long long* totR[2];
  long long* ext[2];
  long long* dense;             // LD_DENSE * max_n
  int* ixL[2];                  // nnz + rows
  int* P[2];
  int* R[2];
  int* size[2];
  int* target;
  int* flag;
  int* node_of;
  int* rank;
  int* orig;
  int* rowcnt;
  int* first;
  int* raw;
};
__host__ __device__ inline long long ld_pad(long long v) { return (v + 1) & ~1ll; }      // int arrays in 8-byte units
__host__ __device__ inline ld_work ld_carve(void* work, long long rows, long long nnz, int S, int max_n, long long* bytes) {
  ld_work w;
  char* p = static_cast<char*>(work);
  auto take = [&](long long n, int width) { char* r = p; p += ld_pad(n) * width; return r; };
  w.st = reinterpret_cast<ld_state*>(take((long long)S * 16, 8));
  w.q0 = reinterpret_cast<long long*>(take(nnz, 8));
  for (int a = 0; a < 2; ++a) w.ipL[a] = reinterpret_cast<long long*>(take(rows + S, 8));
  for (int a = 0; a < 2; ++a) w.qL[a] = reinterpret_cast<long long*>(take(nnz + rows, 8));
  for (int a = 0; a < 2; ++a) w.kk[a] = reinterpret_cast<long long*>(take(rows, 8));
  for (int a = 0; a < 2; ++a) w.tot[a] = reinterpret_cast<long long*>(take(rows, 8));
  for (int a = 0; a < 2; ++a) w.totR[a] = reinterpret_cast<long long*>(take(rows, 8));
  for (int a = 0; a < 2; ++a) w.ext[a] = reinterpret_cast<long long*>(take(rows, 8));
  w.dense = reinterpret_cast<long long*>(take((long long)LD_DENSE * max_n, 8));
  for (int a = 0; a < 2; ++a) w.ixL[a] = reinterpret_cast<int*>(take(nnz + rows, 4));
  for (int a = 0; a < 2; ++a) w.P[a] = reinterpret_cast<int*>(take(rows, 4));
  for (int a = 0; a < 2; ++a) w.R[a] = reinterpret_cast<int*>(take(rows, 4));
  for (int a = 0; a < 2; ++a) w.size[a] = reinterpret_cast<int*>(take(rows, 4));
  int** singles[] = {&w.target, &w.flag, &w.node_of, &w.rank, &w.orig, &w.rowcnt, &w.first, &w.raw};
  for (int** q : singles) *q = reinterpret_cast<int*>(take(rows, 4));
  *bytes = (long long)(p - static_cast<char*>(work));
  return w;
}

struct ld_args {
  const long long* indptr;      // the caller's CSR: level 0 is read in place
  const int* indices;
  const long long* off;
  const long long* nnz_off;
  ld_work w;
  long long rows, nnz_total;
  double gamma;
  int S, max_n, level;
};

// ---------------------------------------------------------------------------------------------------------- helpers
// segment_span and segment_entries (device.h) with A's fields read inside the test, not ahead of it: a call to either
// reads them first and changes the code of this file's kernels
__device__ __forceinline__ bool ld_segment(const ld_args& A, int s, long long* o, int* n0) {
  const long long lo = A.off[s], len = A.off[s + 1] - lo;
  if (lo < 0 || len < 2 || len > A.max_n || lo + len > A.rows) return false;
  *o = lo;
  *n0 = (int)len;
  return true;
}
// where the entries of segment s live at the level, and how many fit
__device__ __forceinline__ bool ld_entries(const ld_args& A, int s, long long o, int n0, int level, long long* base,
                                           long long* cap) {
  const long long lo = A.nnz_off[s], len = A.nnz_off[s + 1] - lo;
  if (lo < 0 || len < 0 || lo + len > A.nnz_total) return false;
  *base = level == 0 ? lo : lo + o;
  *cap = level == 0 ? len : len + n0;
  return true;
}
// one of a pair of buffers (a select: an array of pointers indexed at run time would live in scratch)
template <typename T>
__device__ __forceinline__ T* ld_sel(T* first, T* second, int which) { return which ? second : first; }
struct ld_graph {
  const long long* ip;
  const int* ix;
  const long long* qw;
  const long long* kk;
};
__device__ __forceinline__ ld_graph ld_level(const ld_args& A, int level) {
  ld_graph g;
  g.ip = level == 0 ? A.indptr : ld_sel(A.w.ipL[0], A.w.ipL[1], level & 1);
  g.ix = level == 0 ? A.indices : ld_sel(A.w.ixL[0], A.w.ixL[1], level & 1);
  g.qw = level == 0 ? A.w.q0 : ld_sel(A.w.qL[0], A.w.qL[1], level & 1);
  g.kk = ld_sel(A.w.kk[0], A.w.kk[1], level & 1);
  return g;
}
// the absolute entry range of row i; empty where the row pointers do not fit
__device__ __forceinline__ void ld_row(const ld_graph& g, long long o, int s, int i, long long base, long long cap,
                                       long long* lo, long long* hi) {
  const long long a = g.ip[o + s + i], b = g.ip[o + s + i + 1];
  const bool ok = a >= 0 && a <= b && b <= cap;
  *lo = ok ? base + a : 0;
  *hi = ok ? base + b : 0;
}

__device__ __forceinline__ void ld_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ((gamma a) b) / 2m: each operation rounded once
__device__ __forceinline__ double ld_penalty(double gamma, long long a, long long b, double m2) {
#pragma clang fp contract(off)
  const double ga = gamma * (double)a;
  const double gab = ga * (double)b;
  return gab / m2;
}
__device__ __forceinline__ double ld_gain(long long kic, double pen) {
#pragma clang fp contract(off)
  return (double)kic - pen;
}

// the candidate of largest gain, ties to the smaller id, over the wave
__device__ __forceinline__ void ld_better(double g, int c, double* bg, int* bc) {
  if (g > *bg || (g == *bg && c < *bc)) {
    *bg = g;
    *bc = c;
  }
}
__device__ __forceinline__ void ld_wave_best(double* bg, int* bc) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double og = __shfl_xor(*bg, o, 64);
    const int oc = __shfl_xor(*bc, o, 64);
    ld_better(og, oc, bg, bc);
  }
}

__device__ __forceinline__ void ld_phase() {      // one wave per workgroup: orders its lanes' traffic to the workspace
  __threadfence();
  __syncthreads();
}

// k_ic accumulators of one wave.  The hash table lives in LDS (keys -1 when empty); the dense one in the workspace, all zero
// between vertices.  Integer atomics only: the sums are exact, so arrival order changes nothing.
struct ld_hash {
  int* keys;
  unsigned long long* vals;
  __device__ __forceinline__ void clear(int lane) {
    for (int t = lane; t < LD_SLOTS; t += 64) {
      keys[t] = -1;
      vals[t] = 0ull;
    }
  }
  __device__ __forceinline__ void add(int c, long long q) {
    unsigned slot = ((unsigned)c * 0x9E3779B1u) >> 22;                  // 10 bits
    for (int probe = 0; probe < LD_SLOTS; ++probe) {
      const int prev = atomicCAS(&keys[slot], -1, c);
      if (prev == -1 || prev == c) {
        atomicAdd(&vals[slot], (unsigned long long)q);
        return;
      }
      slot = (slot + 1) & (LD_SLOTS - 1);
    }
  }
  __device__ __forceinline__ long long get(int c) const {
    unsigned slot = ((unsigned)c * 0x9E3779B1u) >> 22;
    for (int probe = 0; probe < LD_SLOTS; ++probe) {
      const int key = keys[slot];
      if (key == c) return (long long)vals[slot];
      if (key == -1) return 0;
      slot = (slot + 1) & (LD_SLOTS - 1);
    }
    return 0;
  }
  __device__ __forceinline__ void drop(int) {}
  __device__ __forceinline__ void phase() const { __syncthreads(); }      // LDS only: the barrier orders it
};
static_assert(LD_SLOTS == 1024, "the hash takes the top 10 bits");
struct ld_dense {
  long long* acc;               // n entries, ids below n
  __device__ __forceinline__ void clear(int) {}
  __device__ __forceinline__ void add(int c, long long q) { ld_add(acc + c, q); }
  __device__ __forceinline__ long long get(int c) const {
    return __hip_atomic_load(acc + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void drop(int c) { __hip_atomic_store(acc + c, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void phase() const { ld_phase(); }
};

// ---------------------------------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(LD_THREADS) void ld_prepare_kernel(ld_args A, const double* __restrict__ data,
                                                                const int* __restrict__ active) {
  __shared__ double red[LD_THREADS / 64];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o = 0, base = 0, cap = 0;
  int n0 = 0;
  const bool ok = ld_segment(A, s, &o, &n0) && ld_entries(A, s, o, n0, 0, &base, &cap);
  double m = 0.0;
  if (ok)
    for (long long e = threadIdx.x; e < cap; e += LD_THREADS) {
      const double v = data[base + e];
      if (valid_weight(v)) m = fmax(m, v);
    }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) m = fmax(m, __shfl_xor(m, sh, 64));   // wave_max(m) written out: a call changes this kernel's code
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  int ex = 0, bits = 0;
  if (m > 0.0) (void)frexp(m, &ex);
  while (cap > 1 && (1ll << bits) < cap) ++bits;
  st->Q = 0.0;
  st->QR = 0.0;
  st->m2 = 0;
  st->in_new = 0;
  for (int t = 0; t < F_COUNT; ++t) st->f[t] = 0;
  st->f[F_N] = st->f[F_N0] = ok ? n0 : 0;
  st->f[F_SHIFT] = 61 - ex - bits;
  const bool runs = ok && m > 0.0 && (!active || active[s] != 0);
  st->f[F_FINISHED] = runs ? 0 : 1;
  st->f[F_MOVE_DONE] = st->f[F_REF_DONE] = runs ? 0 : 1;
  if (!ok) st->f[F_ERROR] = 2;
}

// one wave per row: q of its entries, k_i, the start label, the identity maps
__global__ __launch_bounds__(64) void ld_quantise_kernel(ld_args A, const double* __restrict__ data,
                                                         const int* __restrict__ partition) {
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  long long o, base, cap;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || i >= n0 || !ld_entries(A, s, o, n0, 0, &base, &cap)) return;
  const ld_graph g = ld_level(A, 0);
  long long lo, hi;
  ld_row(g, o, s, i, base, cap, &lo, &hi);
  const int shift = A.w.st[s].f[F_SHIFT];
  long long sum = 0;
  for (long long e = lo + lane; e < hi; e += 64) {
    const double v = data[e];
    const int j = A.indices[e];
    long long q = 0;
    if (valid_weight(v) && j >= 0 && j < n0 && j != i) q = (long long)rint(ldexp(v, shift));
    A.w.q0[e] = q;
    sum += q;
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    A.w.kk[0][o + i] = sum;
    int p = partition ? partition[o + i] : i;
    if (p < 0 || p >= n0) p = i;
    A.w.P[0][o + i] = p;
    A.w.orig[o + i] = i;
  }
}

__global__ __launch_bounds__(LD_THREADS) void ld_m2_kernel(ld_args A) {
  __shared__ long long red[LD_THREADS / 64];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0)) return;
  long long sum = 0;
  for (int i = threadIdx.x; i < n0; i += LD_THREADS) sum += A.w.kk[0][o + i];
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    st->m2 = red[0] + red[1] + red[2] + red[3];
    if (st->m2 <= 0) st->f[F_FINISHED] = st->f[F_MOVE_DONE] = st->f[F_REF_DONE] = 1;
  }
}

// ------------------------------------------------------------------------------------------------------ local moving
// mode 0: the move phase (skips a segment whose phase is over); 1: the start of a level; buffer = cur ^ 1 or cur
__device__ __forceinline__ bool ld_move_live(const ld_state* st, int begin) {
  return !st->f[F_FINISHED] && (begin || !st->f[F_MOVE_DONE]);
}

__global__ __launch_bounds__(LD_THREADS) void ld_zero_move_kernel(ld_args A, int begin) {
  const int s = blockIdx.y, i = blockIdx.x * LD_THREADS + threadIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_move_live(st, begin)) return;
  if (i >= st->f[F_N]) return;
  const int buf = begin ? st->f[F_CUR] : st->f[F_CUR] ^ 1;
  ld_sel(A.w.tot[0], A.w.tot[1], buf)[o + i] = 0;
  if (i == 0) st->in_new = 0;
}

template <typename ACC>
__device__ __forceinline__ void ld_decide(const ld_args& A, const ld_graph& g, ACC acc, long long o, int n, int i, int lane,
                                          long long lo, long long hi, const ld_state* st) {
  const int cur = st->f[F_CUR];
  const int* P = ld_sel(A.w.P[0], A.w.P[1], cur) + o;
  const long long* tot = ld_sel(A.w.tot[0], A.w.tot[1], cur) + o;
  const int own = P[i];
  const long long ki = g.kk[o + i];
  const double m2 = (double)st->m2;
  acc.clear(lane);
  acc.phase();
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    const long long q = g.qw[e];
    if (q == 0 || j == i || j < 0 || j >= n) continue;
    acc.add(P[j], q);
  }
  acc.phase();
  double bg = -HUGE_VAL;
  int bc = INT_MAX;
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    const long long q = g.qw[e];
    if (q == 0 || j == i || j < 0 || j >= n) continue;
    const int c = P[j];
    if (c == own) continue;
    ld_better(ld_gain(acc.get(c), ld_penalty(A.gamma, ki, tot[c], m2)), c, &bg, &bc);
  }
  const long long kown = acc.get(own);
  ld_wave_best(&bg, &bc);
  acc.phase();
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    if (j >= 0 && j < n) acc.drop(P[j]);
  }
  if (lane == 0) {
    int to = own;
    if (bc != INT_MAX) {
#pragma clang fp contract(off)
      const double stay = ld_gain(kown, ld_penalty(A.gamma, ki, tot[own] - ki, m2));
      const double diff = bg - stay;
      if (diff > 0.0 && (st->f[F_PARITY] ? bc > own : bc < own)) to = bc;
    }
    ld_sel(A.w.P[0], A.w.P[1], cur ^ 1)[o + i] = to;
  }
}

// rows of up to LD_CUT entries: one wave (one workgroup) per vertex
__global__ __launch_bounds__(64) void ld_sweep_kernel(ld_args A) {
  __shared__ int keys[LD_SLOTS];
  __shared__ unsigned long long vals[LD_SLOTS];
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o, base, cap, lo, hi;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_move_live(st, 0) || i >= st->f[F_N]) return;
  if (!ld_entries(A, s, o, n0, A.level, &base, &cap)) return;
  const ld_graph g = ld_level(A, A.level);
  ld_row(g, o, s, i, base, cap, &lo, &hi);
  if (hi - lo > LD_CUT) return;                          // ld_sweep_long_kernel's
  ld_hash acc{keys, vals};
  ld_decide(A, g, acc, o, st->f[F_N], i, lane, lo, hi, st);
}

// longer rows: LD_DENSE waves walk every segment's vertices; wave b owns dense[b * max_n ..]
__global__ __launch_bounds__(64) void ld_sweep_long_kernel(ld_args A) {
  const int lane = threadIdx.x;
  ld_dense acc{A.w.dense + (long long)blockIdx.x * A.max_n};
  const ld_graph g = ld_level(A, A.level);
  for (int s = 0; s < A.S; ++s) {
    const ld_state* st = A.w.st + s;
    long long o, base, cap, lo, hi;
    int n0;
    if (!ld_segment(A, s, &o, &n0) || !ld_move_live(st, 0) || !ld_entries(A, s, o, n0, A.level, &base, &cap)) continue;
    const int n = st->f[F_N];
    for (int i = blockIdx.x; i < n; i += LD_DENSE) {
      ld_row(g, o, s, i, base, cap, &lo, &hi);
      if (hi - lo <= LD_CUT) continue;
      ld_decide(A, g, acc, o, n, i, lane, lo, hi, st);
      ld_phase();
    }
  }
}

// tot and the inside weight of label buffer `buf`: a wave per vertex, integer atomics
__global__ __launch_bounds__(64) void ld_tally_move_kernel(ld_args A, int begin) {
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  ld_state* st = A.w.st + s;
  long long o, base, cap, lo, hi;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_move_live(st, begin) || i >= st->f[F_N]) return;
  if (!ld_entries(A, s, o, n0, A.level, &base, &cap)) return;
  const int n = st->f[F_N];
  const int buf = begin ? st->f[F_CUR] : st->f[F_CUR] ^ 1;
  const int* P = ld_sel(A.w.P[0], A.w.P[1], buf) + o;
  const ld_graph g = ld_level(A, A.level);
  ld_row(g, o, s, i, base, cap, &lo, &hi);
  const int own = P[i];
  long long in = 0;
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    if (j >= 0 && j < n && P[j] == own) in += g.qw[e];
  }
  in = wave_sum(in);
  if (lane == 0) {
    ld_add(ld_sel(A.w.tot[0], A.w.tot[1], buf) + o + own, g.kk[o + i]);
    if (in) ld_add(&st->in_new, in);
  }
}

// Q = in / 2m - gamma sum_c (tot_c / 2m)^2: partial t adds c = t, t + 256, .. in order, then p[t] += p[t + o], o = 128 .. 1
__device__ __forceinline__ double ld_quality(const long long* tot, int n, long long in, long long m2i, double gamma,
                                             double* part) {
#pragma clang fp contract(off)
  const double m2 = (double)m2i;
  double acc = 0.0;
  for (int c = threadIdx.x; c < n; c += LD_THREADS) {
    const double t = (double)tot[c] / m2;
    const double sq = t * t;
    acc = acc + sq;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = LD_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + o];
    __syncthreads();
  }
  const double inside = (double)in / m2;
  const double pen = gamma * part[0];
  return inside - pen;
}

__global__ __launch_bounds__(LD_THREADS) void ld_q_move_kernel(ld_args A, int begin, int max_sweeps) {
  __shared__ double part[LD_THREADS];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_move_live(st, begin)) return;      // uniform over the workgroup
  const int buf = begin ? st->f[F_CUR] : st->f[F_CUR] ^ 1;
  const double Q = ld_quality(ld_sel(A.w.tot[0], A.w.tot[1], buf) + o, st->f[F_N], st->in_new, st->m2, A.gamma, part);
  if (threadIdx.x != 0) return;
  if (begin) {
    st->Q = Q;
    st->f[F_PARITY] = st->f[F_FAILS] = st->f[F_MOVE_DONE] = st->f[F_LEVEL_ACC] = st->f[F_PHASE] = 0;
    return;
  }
  st->f[F_SWEEPS] += 1;
  st->f[F_PHASE] += 1;
  if (Q > st->Q) {
    st->Q = Q;
    st->f[F_CUR] ^= 1;
    st->f[F_FAILS] = 0;
    st->f[F_ACCEPTED] += 1;
    st->f[F_LEVEL_ACC] += 1;
  } else {
    st->f[F_FAILS] += 1;
  }
  st->f[F_PARITY] ^= 1;
  if (st->f[F_FAILS] >= 2) {
    st->f[F_MOVE_DONE] = 1;
  } else if (st->f[F_PHASE] >= max_sweeps) {
    st->f[F_MOVE_DONE] = 1;
    st->f[F_ERROR] = 1;
  }
}

// -------------------------------------------------------------------------------------------------------- refinement
__device__ __forceinline__ bool ld_ref_live(const ld_state* st, int begin) {
  return !st->f[F_FINISHED] && (begin || !st->f[F_REF_DONE]);
}

__global__ __launch_bounds__(LD_THREADS) void ld_zero_refine_kernel(ld_args A, int begin) {
  const int s = blockIdx.y, i = blockIdx.x * LD_THREADS + threadIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, begin)) return;
  if (i >= st->f[F_N]) return;
  if (begin) {
    A.w.R[0][o + i] = i;
    if (i == 0) st->f[F_RCUR] = 0;
  }
  const int buf = begin ? 0 : st->f[F_RCUR] ^ 1;
  ld_sel(A.w.totR[0], A.w.totR[1], buf)[o + i] = 0;
  ld_sel(A.w.ext[0], A.w.ext[1], buf)[o + i] = 0;
  ld_sel(A.w.size[0], A.w.size[1], buf)[o + i] = 0;
  A.w.flag[o + i] = 0;
  if (i == 0) st->in_new = 0;
}

template <typename ACC>
__device__ __forceinline__ void ld_propose(const ld_args& A, const ld_graph& g, ACC acc, long long o, int n, int i, int lane,
                                           long long lo, long long hi, const ld_state* st) {
  const int rc = st->f[F_RCUR];
  const int* P = ld_sel(A.w.P[0], A.w.P[1], st->f[F_CUR]) + o;
  const int* R = ld_sel(A.w.R[0], A.w.R[1], rc) + o;
  const long long* totR = ld_sel(A.w.totR[0], A.w.totR[1], rc) + o;
  const long long* ext = ld_sel(A.w.ext[0], A.w.ext[1], rc) + o;
  const int* size = ld_sel(A.w.size[0], A.w.size[1], rc) + o;
  const int S = P[i], r = R[i];
  if (size[r] != 1) {                                   // only a vertex that is still alone may move (uniform over the wave)
    if (lane == 0) A.w.target[o + i] = -1;
    return;
  }
  const long long ki = g.kk[o + i], totS = ld_sel(A.w.tot[0], A.w.tot[1], st->f[F_CUR])[o + S];
  const double m2 = (double)st->m2;
  acc.clear(lane);
  acc.phase();
  long long kS = 0;
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    const long long q = g.qw[e];
    if (q == 0 || j == i || j < 0 || j >= n || P[j] != S) continue;
    acc.add(R[j], q);
    kS += q;
  }
  kS = wave_sum(kS);
  acc.phase();
  double bg = -HUGE_VAL;
  int bc = INT_MAX;
  if ((double)kS >= ld_penalty(A.gamma, ki, totS - ki, m2)) {
    for (long long e = lo + lane; e < hi; e += 64) {
      const int j = g.ix[e];
      const long long q = g.qw[e];
      if (q == 0 || j == i || j < 0 || j >= n || P[j] != S) continue;
      const int c = R[j];
      if (c == r) continue;
      const long long tc = totR[c];
      if (!((double)ext[c] >= ld_penalty(A.gamma, tc, totS - tc, m2))) continue;
      if (!(size[c] > 1 || c < r)) continue;
      const double gain = ld_gain(acc.get(c), ld_penalty(A.gamma, ki, tc, m2));
      if (gain > 0.0) ld_better(gain, c, &bg, &bc);
    }
  }
  ld_wave_best(&bg, &bc);
  acc.phase();
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    if (j >= 0 && j < n) acc.drop(R[j]);
  }
  if (lane == 0) {
    A.w.target[o + i] = bc == INT_MAX ? -1 : bc;
    if (bc != INT_MAX) A.w.flag[o + bc] = 1;             // a plain idempotent store
  }
}

__global__ __launch_bounds__(64) void ld_propose_kernel(ld_args A) {
  __shared__ int keys[LD_SLOTS];
  __shared__ unsigned long long vals[LD_SLOTS];
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o, base, cap, lo, hi;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, 0) || i >= st->f[F_N]) return;
  if (!ld_entries(A, s, o, n0, A.level, &base, &cap)) return;
  const ld_graph g = ld_level(A, A.level);
  ld_row(g, o, s, i, base, cap, &lo, &hi);
  if (hi - lo > LD_CUT) return;
  ld_hash acc{keys, vals};
  ld_propose(A, g, acc, o, st->f[F_N], i, lane, lo, hi, st);
}

__global__ __launch_bounds__(64) void ld_propose_long_kernel(ld_args A) {
  const int lane = threadIdx.x;
  ld_dense acc{A.w.dense + (long long)blockIdx.x * A.max_n};
  const ld_graph g = ld_level(A, A.level);
  for (int s = 0; s < A.S; ++s) {
    const ld_state* st = A.w.st + s;
    long long o, base, cap, lo, hi;
    int n0;
    if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, 0) || !ld_entries(A, s, o, n0, A.level, &base, &cap)) continue;
    const int n = st->f[F_N];
    for (int i = blockIdx.x; i < n; i += LD_DENSE) {
      ld_row(g, o, s, i, base, cap, &lo, &hi);
      if (hi - lo <= LD_CUT) continue;
      ld_propose(A, g, acc, o, n, i, lane, lo, hi, st);
      ld_phase();
    }
  }
}

// a lone vertex that some proposal of this round targets stays where it is
__global__ __launch_bounds__(LD_THREADS) void ld_commit_kernel(ld_args A) {
  const int s = blockIdx.y, i = blockIdx.x * LD_THREADS + threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, 0) || i >= st->f[F_N]) return;
  const int rc = st->f[F_RCUR];
  const int t = A.w.target[o + i];
  ld_sel(A.w.R[0], A.w.R[1], rc ^ 1)[o + i] = (t >= 0 && !A.w.flag[o + i]) ? t : ld_sel(A.w.R[0], A.w.R[1], rc)[o + i];
}

__global__ __launch_bounds__(64) void ld_tally_refine_kernel(ld_args A, int begin) {
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  ld_state* st = A.w.st + s;
  long long o, base, cap, lo, hi;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, begin) || i >= st->f[F_N]) return;
  if (!ld_entries(A, s, o, n0, A.level, &base, &cap)) return;
  const int n = st->f[F_N];
  const int buf = begin ? 0 : st->f[F_RCUR] ^ 1;
  const int* P = ld_sel(A.w.P[0], A.w.P[1], st->f[F_CUR]) + o;
  const int* R = ld_sel(A.w.R[0], A.w.R[1], buf) + o;
  const ld_graph g = ld_level(A, A.level);
  ld_row(g, o, s, i, base, cap, &lo, &hi);
  const int r = R[i], S = P[i];
  long long in = 0, out = 0;
  for (long long e = lo + lane; e < hi; e += 64) {
    const int j = g.ix[e];
    if (j < 0 || j >= n) continue;
    const long long q = g.qw[e];
    if (R[j] == r) in += q;
    else if (P[j] == S) out += q;
  }
  in = wave_sum(in);
  out = wave_sum(out);
  if (lane == 0) {
    ld_add(ld_sel(A.w.totR[0], A.w.totR[1], buf) + o + r, g.kk[o + i]);
    atomicAdd(ld_sel(A.w.size[0], A.w.size[1], buf) + o + r, 1);
    if (out) ld_add(ld_sel(A.w.ext[0], A.w.ext[1], buf) + o + r, out);
    if (in) ld_add(&st->in_new, in);
  }
}

__global__ __launch_bounds__(LD_THREADS) void ld_q_refine_kernel(ld_args A, int begin, int max_rounds) {
  __shared__ double part[LD_THREADS];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || !ld_ref_live(st, begin)) return;
  const int buf = begin ? 0 : st->f[F_RCUR] ^ 1;
  const double Q = ld_quality(ld_sel(A.w.totR[0], A.w.totR[1], buf) + o, st->f[F_N], st->in_new, st->m2, A.gamma, part);
  if (threadIdx.x != 0) return;
  if (begin) {
    st->QR = Q;
    st->f[F_REF_DONE] = st->f[F_PHASE] = 0;
    return;
  }
  st->f[F_ROUNDS] += 1;
  st->f[F_PHASE] += 1;
  if (Q > st->QR) {
    st->QR = Q;
    st->f[F_RCUR] ^= 1;
    if (st->f[F_PHASE] >= max_rounds) {
      st->f[F_REF_DONE] = 1;
      st->f[F_ERROR] = 1;
    }
  } else {
    st->f[F_REF_DONE] = 1;
  }
}

// ------------------------------------------------------------------------------------------------------- aggregation
// exclusive prefix sums of v[0 .. n) in index order by one workgroup: thread t owns a contiguous chunk; returns the total
template <typename F, typename G>
__device__ __forceinline__ long long ld_block_scan(int n, F value, G store, long long* part) {
  const int chunk = (n + LD_THREADS - 1) / LD_THREADS;
  const int lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += value(i);
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int t = 0; t < LD_THREADS; ++t) {
      const long long v = part[t];
      part[t] = run;
      run += v;
    }
    part[LD_THREADS] = run;
  }
  __syncthreads();
  long long run = part[threadIdx.x];
  for (int i = lo; i < hi; ++i) {
    store(i, run);
    run += value(i);
  }
  return part[LD_THREADS];
}

// refined communities become nodes, numbered in order of their id; decides whether the segment is finished
__global__ __launch_bounds__(LD_THREADS) void ld_agg_number_kernel(ld_args A, int max_levels) {
  __shared__ long long part[LD_THREADS + 1];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || st->f[F_FINISHED]) return;
  const int n = st->f[F_N];
  const int* size = ld_sel(A.w.size[0], A.w.size[1], st->f[F_RCUR]) + o;
  int* rank = A.w.rank + o;
  const long long total = ld_block_scan(n, [&](int i) { return (long long)(size[i] > 0); },
                                        [&](int i, long long v) { rank[i] = (int)v; }, part);
  if (threadIdx.x != 0) return;
  st->f[F_LEVELS] += 1;
  st->f[F_N_NEXT] = (int)total;
  if (st->f[F_LEVEL_ACC] == 0 && total == n) {
    st->f[F_FINISHED] = 1;
  } else if (A.level + 1 >= max_levels) {
    st->f[F_FINISHED] = 1;
    st->f[F_ERROR] = 1;
  }
}

__global__ __launch_bounds__(LD_THREADS) void ld_agg_zero_kernel(ld_args A) {
  const int s = blockIdx.y, i = blockIdx.x * LD_THREADS + threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || st->f[F_FINISHED] || i >= st->f[F_N]) return;
  ld_sel(A.w.kk[0], A.w.kk[1], (A.level + 1) & 1)[o + i] = 0;
  A.w.first[o + i] = INT_MAX;
}

__global__ __launch_bounds__(LD_THREADS) void ld_agg_map_kernel(ld_args A) {
  const int s = blockIdx.y, i = blockIdx.x * LD_THREADS + threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || st->f[F_FINISHED] || i >= st->f[F_N]) return;
  const int node = A.w.rank[o + ld_sel(A.w.R[0], A.w.R[1], st->f[F_RCUR])[o + i]];
  A.w.node_of[o + i] = node;
  ld_add(ld_sel(A.w.kk[0], A.w.kk[1], (A.level + 1) & 1) + o + node, ld_sel(A.w.kk[0], A.w.kk[1], A.level & 1)[o + i]);
  atomicMin(A.w.first + o + ld_sel(A.w.P[0], A.w.P[1], st->f[F_CUR])[o + i], node);
}

// the merged row of every node: LD_DENSE waves; a wave gathers its node's members' rows into its dense accumulator and reads
// it back in column order.  fill = 0 counts the row's entries, fill = 1 writes them behind the row pointer.
__global__ __launch_bounds__(64) void ld_agg_rows_kernel(ld_args A, int fill) {
  const int lane = threadIdx.x;
  long long* acc = A.w.dense + (long long)blockIdx.x * A.max_n;
  const ld_graph g = ld_level(A, A.level);
  const int nb = (A.level + 1) & 1;
  for (int s = 0; s < A.S; ++s) {
    const ld_state* st = A.w.st + s;
    long long o, base, cap, nbase, ncap;
    int n0;
    if (!ld_segment(A, s, &o, &n0) || st->f[F_FINISHED] || !ld_entries(A, s, o, n0, A.level, &base, &cap)) continue;
    (void)ld_entries(A, s, o, n0, 1, &nbase, &ncap);
    const int n = st->f[F_N], nn = st->f[F_N_NEXT];
    const int* node_of = A.w.node_of + o;
    for (int a = blockIdx.x; a < nn; a += LD_DENSE) {
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        if (i < n && node_of[i] == a) {
          long long lo, hi;
          ld_row(g, o, s, i, base, cap, &lo, &hi);
          for (long long e = lo; e < hi; ++e) {
            const int j = g.ix[e];
            const long long q = g.qw[e];
            if (q != 0 && j >= 0 && j < n) ld_add(acc + node_of[j], q);
          }
        }
      }
      ld_phase();
      long long at = fill ? ld_sel(A.w.ipL[0], A.w.ipL[1], nb)[o + s + a] : 0;
      int count = 0;
      for (int c0 = 0; c0 < nn; c0 += 64) {
        const int c = c0 + lane;
        const long long v = c < nn ? __hip_atomic_load(acc + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const unsigned long long mask = __ballot(v != 0);
        if (v != 0) {
          __hip_atomic_store(acc + c, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (fill) {
            const long long pos = at + count + __popcll(mask & ((1ull << lane) - 1ull));
            if (pos < ncap) {
              ld_sel(A.w.ixL[0], A.w.ixL[1], nb)[nbase + pos] = c;
              ld_sel(A.w.qL[0], A.w.qL[1], nb)[nbase + pos] = v;
            }
          }
        }
        count += __popcll(mask);
      }
      if (!fill && lane == 0) A.w.rowcnt[o + a] = count;
      ld_phase();
    }
  }
}

// row pointers of the next level (prefix sums in index order), its start labels, the map of the original vertices, the state
__global__ __launch_bounds__(LD_THREADS) void ld_agg_indptr_kernel(ld_args A) {
  __shared__ long long part[LD_THREADS + 1];
  __shared__ int longest[LD_THREADS / 64];
  const int s = blockIdx.x;
  ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || st->f[F_FINISHED]) return;
  const int n = st->f[F_N], nn = st->f[F_N_NEXT], nb = (A.level + 1) & 1;
  const int* rowcnt = A.w.rowcnt + o;
  long long* ip = ld_sel(A.w.ipL[0], A.w.ipL[1], nb) + o + s;
  const long long total = ld_block_scan(nn, [&](int a) { return (long long)rowcnt[a]; },
                                        [&](int a, long long v) { ip[a] = v; }, part);
  int m = 0;
  for (int a = threadIdx.x; a < nn; a += LD_THREADS) m = max(m, rowcnt[a]);
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) m = max(m, __shfl_xor(m, sh, 64));   // an int maximum: device.h has none
  if ((threadIdx.x & 63) == 0) longest[threadIdx.x >> 6] = m;
  // the start labels of the next level: the smallest node of the vertex's community; founders carry their node's
  const int cur = st->f[F_CUR];
  for (int i = threadIdx.x; i < n; i += LD_THREADS)
    if (ld_sel(A.w.R[0], A.w.R[1], st->f[F_RCUR])[o + i] == i) ld_sel(A.w.P[0], A.w.P[1], cur ^ 1)[o + A.w.rank[o + i]] = A.w.first[o + ld_sel(A.w.P[0], A.w.P[1], cur)[o + i]];
  for (int v = threadIdx.x; v < n0; v += LD_THREADS) A.w.orig[o + v] = A.w.node_of[o + A.w.orig[o + v]];
  __syncthreads();
  if (threadIdx.x != 0) return;
  ip[nn] = total;
  st->f[F_MAX_ROW] = max(max(longest[0], longest[1]), max(longest[2], longest[3]));
}

// after the rows are filled: the segment moves to its next level
__global__ __launch_bounds__(LD_THREADS) void ld_agg_done_kernel(ld_args A) {
  const int s = blockIdx.x * LD_THREADS + threadIdx.x;
  if (s >= A.S) return;
  ld_state* st = A.w.st + s;
  if (st->f[F_FINISHED]) return;
  st->f[F_N] = st->f[F_N_NEXT];
  st->f[F_CUR] ^= 1;
}

// ------------------------------------------------------------------------------------------------------------ finish
// source 0: the community of every original vertex (P[cur][orig]); 1: its refined community at level 0 (R[rcur])
__global__ __launch_bounds__(LD_THREADS) void ld_finish_raw_kernel(ld_args A, int source, const int* __restrict__ active,
                                                                   int stage, int* __restrict__ canon) {
  const int s = blockIdx.y, v = blockIdx.x * LD_THREADS + threadIdx.x;
  const ld_state* st = A.w.st + s;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || v >= n0 || (active && !active[s])) return;
  if (stage == 0) {
    A.w.first[o + v] = INT_MAX;
  } else if (stage == 1) {
    int c = v;
    if (st->m2 > 0) c = source ? ld_sel(A.w.R[0], A.w.R[1], st->f[F_RCUR])[o + v] : ld_sel(A.w.P[0], A.w.P[1], st->f[F_CUR])[o + A.w.orig[o + v]];
    if (c < 0 || c >= n0) c = v;
    A.w.raw[o + v] = c;
    atomicMin(A.w.first + o + c, v);
  } else {
    canon[o + v] = A.w.first[o + A.w.raw[o + v]];
  }
}

// canonical ids (the smallest member) to labels by descending size, ties to the smaller smallest member
__global__ __launch_bounds__(LD_THREADS) void ld_finish_rank_kernel(ld_args A, int stage, const int* __restrict__ canon,
                                                                    int* __restrict__ labels, int* __restrict__ n_clusters) {
  const int s = blockIdx.y, v = blockIdx.x * LD_THREADS + threadIdx.x;
  long long o;
  int n0;
  if (!ld_segment(A, s, &o, &n0) || v >= n0) return;
  int* size = A.w.size[0] + o;
  if (stage == 0) {
    size[v] = 0;
    if (v == 0) n_clusters[s] = 0;
  } else if (stage == 1) {
    int c = canon[o + v];
    if (c < 0 || c >= n0) c = v;
    atomicAdd(size + c, 1);
    if (c == v) atomicAdd(n_clusters + s, 1);
  } else if (stage == 2) {
    const int mine = size[v];
    if (mine == 0) return;
    int before = 0;
    for (int u = 0; u < n0; ++u) {
      const int other = size[u];
      before += (other > mine || (other == mine && u < v)) ? 1 : 0;
    }
    A.w.rank[o + v] = before;
  } else {
    int c = canon[o + v];
    if (c < 0 || c >= n0) c = v;
    labels[o + v] = A.w.rank[o + c];
  }
}

bool ld_finite(double v) { return v == v && v <= DBL_MAX && v >= -DBL_MAX; }

// the checks every launching entry point shares, and the argument block of its kernels
int ld_make(const int64_t* indptr, const int32_t* indices, const int64_t* offsets, const int64_t* nnz_offsets, int32_t S,
            int32_t rows, int32_t max_n, int64_t nnz_total, double gamma, int32_t level, void* work, ld_args* A) {
  if (!indptr || !indices || !offsets || !nnz_offsets || !work || S <= 0 || rows <= 0 || nnz_total < 0 || level < 0)
    return MCL_EINVAL;
  if (!ld_finite(gamma) || !(gamma > 0.0)) return MCL_EINVAL;
  if (S > LD_MAX_S || max_n > LD_MAX_N || max_n < 2) return MCL_EUNSUPPORTED;
  if (rows < 2ll * S || rows > (long long)S * max_n) return MCL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(work) & 7) != 0) return MCL_EINVAL;
  long long bytes;
  A->indptr = reinterpret_cast<const long long*>(indptr);
  A->indices = indices;
  A->off = reinterpret_cast<const long long*>(offsets);
  A->nnz_off = reinterpret_cast<const long long*>(nnz_offsets);
  A->w = ld_carve(work, rows, nnz_total, S, max_n, &bytes);
  A->rows = rows;
  A->nnz_total = nnz_total;
  A->gamma = gamma;
  A->S = S;
  A->max_n = max_n;
  A->level = level;
  return MCL_OK;
}

void ld_level_begin(const ld_args& A, int n_cur, hipStream_t st) {
  const dim3 per_vertex(ceil_div(n_cur, LD_THREADS), A.S), per_wave(n_cur, A.S);
  hipLaunchKernelGGL(ld_zero_move_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, 1);
  hipLaunchKernelGGL(ld_tally_move_kernel, per_wave, dim3(64), 0, st, A, 1);
  hipLaunchKernelGGL(ld_q_move_kernel, dim3(A.S), dim3(LD_THREADS), 0, st, A, 1, 0);
}

}  // namespace

extern "C" {

int64_t mcl_leiden_workspace_bytes(int64_t rows, int64_t nnz_total, int32_t S, int32_t max_n) {
  if (rows <= 0 || nnz_total < 0 || S <= 0 || S > LD_MAX_S || max_n < 2 || max_n > LD_MAX_N) return -1;
  long long bytes = 0;
  (void)ld_carve(nullptr, rows, nnz_total, S, max_n, &bytes);
  return bytes + 16;
}

int mcl_leiden_init(const int64_t* indptr, const int32_t* indices, const double* data, const int64_t* offsets,
                    const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total, double resolution,
                    const int32_t* partition, const int32_t* active, void* work, mcl_stream_t stream) {
  ld_args A;
  const int rc = ld_make(indptr, indices, offsets, nnz_offsets, S, rows, max_n, nnz_total, resolution, 0, work, &A);
  if (rc != MCL_OK) return rc;
  if (!data) return MCL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MCL_CLEAR_ERROR();
  (void)hipMemsetAsync(A.w.dense, 0, (size_t)LD_DENSE * max_n * 8, st);
  hipLaunchKernelGGL(ld_prepare_kernel, dim3(S), dim3(LD_THREADS), 0, st, A, data, active);
  hipLaunchKernelGGL(ld_quantise_kernel, dim3(max_n, S), dim3(64), 0, st, A, data, partition);
  hipLaunchKernelGGL(ld_m2_kernel, dim3(S), dim3(LD_THREADS), 0, st, A);
  ld_level_begin(A, max_n, st);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_leiden_move_sweeps(int32_t count, int32_t level, int32_t n_cur, int32_t long_rows, int32_t max_sweeps,
                           const int64_t* indptr, const int32_t* indices, const int64_t* offsets, const int64_t* nnz_offsets,
                           int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total, double resolution, void* work,
                           mcl_stream_t stream) {
  ld_args A;
  const int rc = ld_make(indptr, indices, offsets, nnz_offsets, S, rows, max_n, nnz_total, resolution, level, work, &A);
  if (rc != MCL_OK) return rc;
  if (count < 0 || n_cur < 1 || n_cur > max_n || max_sweeps < 1) return MCL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_vertex(ceil_div(n_cur, LD_THREADS), S), per_wave(n_cur, S);
  MCL_CLEAR_ERROR();
  for (int t = 0; t < count; ++t) {
    hipLaunchKernelGGL(ld_zero_move_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, 0);
    hipLaunchKernelGGL(ld_sweep_kernel, per_wave, dim3(64), 0, st, A);
    if (long_rows) hipLaunchKernelGGL(ld_sweep_long_kernel, dim3(LD_DENSE), dim3(64), 0, st, A);
    hipLaunchKernelGGL(ld_tally_move_kernel, per_wave, dim3(64), 0, st, A, 0);
    hipLaunchKernelGGL(ld_q_move_kernel, dim3(S), dim3(LD_THREADS), 0, st, A, 0, max_sweeps);
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_leiden_refine_rounds(int32_t begin, int32_t count, int32_t level, int32_t n_cur, int32_t long_rows,
                             int32_t max_rounds, const int64_t* indptr, const int32_t* indices, const int64_t* offsets,
                             const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total,
                             double resolution, void* work, mcl_stream_t stream) {
  ld_args A;
  const int rc = ld_make(indptr, indices, offsets, nnz_offsets, S, rows, max_n, nnz_total, resolution, level, work, &A);
  if (rc != MCL_OK) return rc;
  if (count < 0 || n_cur < 1 || n_cur > max_n || max_rounds < 1) return MCL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_vertex(ceil_div(n_cur, LD_THREADS), S), per_wave(n_cur, S);
  MCL_CLEAR_ERROR();
  if (begin) {
    hipLaunchKernelGGL(ld_zero_refine_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, 1);
    hipLaunchKernelGGL(ld_tally_refine_kernel, per_wave, dim3(64), 0, st, A, 1);
    hipLaunchKernelGGL(ld_q_refine_kernel, dim3(S), dim3(LD_THREADS), 0, st, A, 1, 0);
  }
  for (int t = 0; t < count; ++t) {
    hipLaunchKernelGGL(ld_zero_refine_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, 0);
    hipLaunchKernelGGL(ld_propose_kernel, per_wave, dim3(64), 0, st, A);
    if (long_rows) hipLaunchKernelGGL(ld_propose_long_kernel, dim3(LD_DENSE), dim3(64), 0, st, A);
    hipLaunchKernelGGL(ld_commit_kernel, per_vertex, dim3(LD_THREADS), 0, st, A);
    hipLaunchKernelGGL(ld_tally_refine_kernel, per_wave, dim3(64), 0, st, A, 0);
    hipLaunchKernelGGL(ld_q_refine_kernel, dim3(S), dim3(LD_THREADS), 0, st, A, 0, max_rounds);
  }
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_leiden_aggregate(int32_t level, int32_t n_cur, int32_t max_levels, const int64_t* indptr, const int32_t* indices,
                         const int64_t* offsets, const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n,
                         int64_t nnz_total, double resolution, void* work, mcl_stream_t stream) {
  ld_args A;
  const int rc = ld_make(indptr, indices, offsets, nnz_offsets, S, rows, max_n, nnz_total, resolution, level, work, &A);
  if (rc != MCL_OK) return rc;
  if (n_cur < 1 || n_cur > max_n || max_levels < 1) return MCL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_vertex(ceil_div(n_cur, LD_THREADS), S);
  MCL_CLEAR_ERROR();
  hipLaunchKernelGGL(ld_agg_number_kernel, dim3(S), dim3(LD_THREADS), 0, st, A, max_levels);
  hipLaunchKernelGGL(ld_agg_zero_kernel, per_vertex, dim3(LD_THREADS), 0, st, A);
  hipLaunchKernelGGL(ld_agg_map_kernel, per_vertex, dim3(LD_THREADS), 0, st, A);
  hipLaunchKernelGGL(ld_agg_rows_kernel, dim3(LD_DENSE), dim3(64), 0, st, A, 0);
  hipLaunchKernelGGL(ld_agg_indptr_kernel, dim3(S), dim3(LD_THREADS), 0, st, A);
  hipLaunchKernelGGL(ld_agg_rows_kernel, dim3(LD_DENSE), dim3(64), 0, st, A, 1);
  hipLaunchKernelGGL(ld_agg_done_kernel, dim3(ceil_div(S, LD_THREADS)), dim3(LD_THREADS), 0, st, A);
  A.level = level + 1;                                   // Q of the start partition of the next level
  ld_level_begin(A, n_cur, st);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

int mcl_leiden_finish(int32_t source, int32_t final_labels, const int32_t* active, const int64_t* indptr,
                      const int32_t* indices, const int64_t* offsets, const int64_t* nnz_offsets, int32_t S, int32_t rows,
                      int32_t max_n, int64_t nnz_total, void* work, int32_t* canonical, int32_t* labels, int32_t* n_clusters,
                      mcl_stream_t stream) {
  ld_args A;
  const int rc = ld_make(indptr, indices, offsets, nnz_offsets, S, rows, max_n, nnz_total, 1.0, 0, work, &A);
  if (rc != MCL_OK) return rc;
  if (!canonical || (source != 0 && source != 1) || (final_labels && (!labels || !n_clusters))) return MCL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_vertex(ceil_div(max_n, LD_THREADS), S);
  MCL_CLEAR_ERROR();
  if (!final_labels)
    for (int stage = 0; stage < 3; ++stage)
      hipLaunchKernelGGL(ld_finish_raw_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, source, active, stage, canonical);
  else
    for (int stage = 0; stage < 4; ++stage)
      hipLaunchKernelGGL(ld_finish_rank_kernel, per_vertex, dim3(LD_THREADS), 0, st, A, stage, canonical, labels, n_clusters);
  MCL_CHECK_LAUNCH();
  return MCL_OK;
}

}  // extern "C"
