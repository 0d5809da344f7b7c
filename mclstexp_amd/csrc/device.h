// Device types and helpers shared by the gfx950 kernels (included from common.h).  A helper that rounds or loads
// differently from the ones here keeps a name of its own in its file (gemm.hip f2bf_rne_finite: no inf / NaN handling;
// dense_block.hip bn_relu_chunk_f4; the buffer descriptors c0_rsrc / raw_rsrc; spatial.hip sp_slide_rows).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

typedef unsigned short bf16_t;                                   // bf16 bits
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));        // MFMA bf16 operand
typedef short v4s __attribute__((ext_vector_type(4)));           // ds_read_b64_tr_b16 result
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));         // the non-temporal builtins reject HIP's float4 class
typedef float f32x16 __attribute__((ext_vector_type(16)));       // 32x32 MFMA accumulator
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // 16-byte chunk; buffer descriptor
typedef unsigned long long u64;

#define MCL_LDSP(p) ((__attribute__((address_space(3))) void*)(p))
#define MCL_GLBP(p) ((const __attribute__((address_space(1))) void*)(p))

// ---- bf16 <-> fp32.  pack_bf16 / f2bf / round_bf16 round to nearest even in hardware (v_cvt_pk_bf16_f32).
__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));  // v_cvt_pk_bf16_f32 (RNE)
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack_bf16(f, 0.0f) & 0xFFFFu); }
__device__ __forceinline__ float round_bf16(float v) { return bf_lo(pack_bf16(v, 0.0f)); }
// round to nearest even in software (inf / NaN truncated), in the low 16 bits of the result
__device__ __forceinline__ unsigned f2bf_rne(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7F800000u) == 0x7F800000u) return u >> 16;   // inf / nan: truncate
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

// one 16-byte chunk = 8 bf16 channels
__device__ __forceinline__ void unpack8(uint4 v, float (&f)[8]) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf_lo(w[i]);
    f[2 * i + 1] = bf_hi(w[i]);
  }
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // pack_bf16 written out: a call to it here changes the code of pool.hip's kernels
    const f32x2 v = {f[2 * i], f[2 * i + 1]};
    w[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// a = relu(x*sc + sh) on one 16-byte chunk (8 channels)
__device__ __forceinline__ uint4 bn_relu_chunk(uint4 v, const float (&sc)[8], const float (&sh)[8]) {
  unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = fmaxf(fmaf(bf_lo(w[i]), sc[2 * i], sh[2 * i]), 0.0f);
    const float hi = fmaxf(fmaf(bf_hi(w[i]), sc[2 * i + 1], sh[2 * i + 1]), 0.0f);
    w[i] = pack_bf16(lo, hi);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// an fp32 / fp64 / integer element as fp64: the load of the kernels that take their input in either width
template <typename T>
__device__ __forceinline__ double ldd(const T* p) { return (double)*p; }

// ---- lanes
// number of set bits of ``mask`` below this lane
__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// sum over the 32 lanes of each half-wave by DPP (5 VALU instructions, no LDS); the total lands in lanes 16..31 / 48..63
__device__ __forceinline__ float half_wave_sum(float x) {
#define MCL_DPP_ADD(ctrl, rmask)                                                                              \
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, rmask, 0xF, false))
  MCL_DPP_ADD(0xB1, 0xF);     // quad_perm [1,0,3,2]
  MCL_DPP_ADD(0x4E, 0xF);     // quad_perm [2,3,0,1]
  MCL_DPP_ADD(0x141, 0xF);    // row_half_mirror
  MCL_DPP_ADD(0x140, 0xF);    // row_mirror: every lane of a 16-lane row holds the row sum
  MCL_DPP_ADD(0x142, 0xA);    // row_bcast15 into rows 1 and 3: + the sum of the row below
#undef MCL_DPP_ADD
  return x;
}

// 64-lane butterfly reductions: every lane returns the wave's sum / maximum / minimum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// the sum over a 256-thread workgroup in a fixed order: the butterfly inside each wave, then waves 0 + 1 + 2 + 3.  Every
// thread returns the same value.  ``red`` holds 4 doubles.  LEAD: a barrier ahead of the store, so that ``red`` may still be
// being read from the reduction before; without it callers alternate two slots.
template <bool LEAD>
__device__ __forceinline__ double block_sum4(double v, double* red) {
  v = wave_sum(v);
  if (LEAD) __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the lane id, made opaque to the compiler: everything derived from it is recomputed where it is used instead of being
// hoisted out of the loop into live registers
__device__ __forceinline__ int opaque_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}
// LDS written by some lanes of a wave is read by others: the hardware runs a wave's LDS instructions in order, this keeps the
// compiler from moving them across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- order-preserving bit patterns: a < b <=> order_key(a) < order_key(b), -0.0 just below +0.0; a NaN with the sign bit
// clear sorts above +inf (as torch.topk treats it).  key_value is the inverse.
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned u = __float_as_uint(f);
  return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  return __uint_as_float(u);
}
__device__ __forceinline__ u64 order_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// ---- segments: the rows (spots of a slide) and stored entries a workgroup owns, read from device-resident offsets
// rows of segment s, first row in *r0_out (always written); 0 where the offsets break what the launch was sized by
// (min_n .. max_n rows each, ``rows`` in all): nothing is read or written then
__device__ __forceinline__ int segment_rows(const long long* __restrict__ offsets, int s, long long rows, int min_n,
                                            int max_n, long long* r0_out) {
  const long long r0 = offsets[s], r1 = offsets[s + 1];
  *r0_out = r0;
  if (r0 < 0 || r1 - r0 < min_n || r1 > rows || r1 - r0 > max_n) return 0;
  return (int)(r1 - r0);
}
// the same check for the kernels that test it as a condition: first row and rows of segment s, written only where it
// holds (segment_rows in their place changes their code).  A segment has 2 rows at the least, whatever min_n says: the two
// terms stand apart because max(2, min_n) changes the code of neighbors.hip, whose min_n is the k of the launch
__device__ __forceinline__ bool segment_span(const long long* off, int s, int min_n, int max_n, long long rows, long long* o,
                                             int* n) {
  const long long lo = off[s], len = off[s + 1] - lo;
  if (lo < 0 || len < 2 || len < min_n || len > max_n || lo + len > rows) return false;
  *o = lo;
  *n = (int)len;
  return true;
}
// the stored entries of segment s: false where nnz_off does not fit nnz_total
__device__ __forceinline__ bool segment_entries(const long long* nnz_off, int s, long long nnz_total, long long* base,
                                                long long* count) {
  const long long lo = nnz_off[s], len = nnz_off[s + 1] - lo;
  if (lo < 0 || len < 0 || lo + len > nnz_total) return false;
  *base = lo;
  *count = len;
  return true;
}
// a stored graph weight that counts: positive and finite
__device__ __forceinline__ bool valid_weight(double w) { return w > 0.0 && w <= DBL_MAX; }
// an index the caller supplied, read as the nearest one in [0, n)
__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// the splitmix64 step: the counter-based generator of every stage that draws
__host__ __device__ __forceinline__ u64 mix64(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- LDS-DMA: every lane fetches 16 (glds4: 4) bytes; the wave's bytes land lane-linear at the wave-uniform LDS byte
// address ``dst`` (M0) -- no VGPR round trip.  Inline asm on purpose: hipcc cannot prove that a DMA into one LDS buffer
// does not alias the LDS being read from another and would drain vmcnt(0) -- the whole prefetch -- mid-tile.  Hidden from
// its bookkeeping, the DMA is covered by the caller's explicit vmcnt + barrier.
__device__ __forceinline__ void glds16(const void* src, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(dst)
               : "memory");
}
// saddr form: wave-uniform 64-bit base in SGPRs + per-lane 32-bit byte offset
// (M0 is not saved / restored here: nothing else in its callers, gemm_bf16.hip and infonce_fused.hip, uses it -- checked
// in the ISA -- and the two extra s_mov per piece are issue slots of a lone wave.)
// The "m0" clobber draws hipcc's "inline asm clobber list contains reserved registers: m0" at every use.
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0"
               :
               : "s"(sbase), "v"(voff), "s"(dst)
               : "memory", "m0");
}
__device__ __forceinline__ void glds4(const void* src, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(dst)
               : "memory");
}
// buffer form: every lane fetches 16 bytes at its own 32-bit byte offset ``voff`` from the buffer descriptor ``rsrc``.  A
// chunk beyond the descriptor's num_records is out of range: it lands in LDS as ZEROS and touches no memory (checked on
// MI355X), so ragged tiles need no branch.
__device__ __forceinline__ void buffer_lds16(u32x4 rsrc, unsigned voff, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(dst)
               : "memory");
}
