/*
 * mclstexp_hip.h -- C ABI of libmclstexp_hip.so: hand-written gfx950 (MI355X) kernels for the
 * contrastive training hot path of mclSTExp.
 *
 * The reference (ZhicengShi/mclSTExp) has no native code and no FFI: every entry point below
 * replaces the ATen dispatch behind one call site of /root/reference/model.py or train.py, cited
 * per function.  Conventions:
 *   - plain pointers + sizes only; every buffer is caller-owned DEVICE memory (the Python host
 *     passes torch tensors' data_ptr()); the library never allocates, frees or retains pointers;
 *   - every call only ENQUEUES work on the caller's stream (hipStream_t passed as void*); no host
 *     synchronisation, no global mutable state; safe from one host thread per device;
 *   - return 0 on success, a positive hipError_t if a launch failed, a negative MCL_E* code for a
 *     rejected argument.  No exceptions cross the ABI.
 *   - all matrices are fp32 row-major with explicit leading dimensions (elements, not bytes);
 *     G (genes) need not be a multiple of anything: tails are masked in-kernel.
 */
#ifndef MCLSTEXP_HIP_H
#define MCLSTEXP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_ABI_VERSION 13

#define MCL_OK 0
#define MCL_EINVAL (-1)       /* null pointer / non-positive size / inconsistent arguments */
#define MCL_EUNSUPPORTED (-2) /* valid but not implemented (e.g. head_dim != 64) */
#define MCL_EWORKSPACE (-3)   /* workspace too small (see the *_workspace_bytes query) */

typedef void* mcl_stream_t; /* hipStream_t */

int mcl_abi_version(void);
const char* mcl_error_string(int code);

/* ---------------------------------------------------------------- GEMM (K3, K5, K6, K7, K8 contractions)
 * C[b] = epilogue( alpha * A[b] (M x K) * B[b] (K x N) ), fp32 in HBM.
 * Element (m,k) of A is A[b*sAb + m*sAm + k*sAk]; element (k,n) of B is B[b*sBb + k*sBk + n*sBn];
 * exactly one of (sAm,sAk) and one of (sBk,sBn) must be 1.  This single strided form covers
 *   y = x W^T      nn.Linear forward      model.py:23,27,43,45,155,157   (A k-contig, B k-contig)
 *   dx = dy W      nn.Linear backward-data                              (A k-contig, B n-contig)
 *   dW = dy^T x    nn.Linear backward-weight                            (A m-contig, B n-contig)
 *   q k^T, attn v  einsum model.py:53,55 batched over heads (b = head, strided views of qkv)
 *   S = E_spot E_img^T / T                model.py:242
 * Epilogue, in order:  v = alpha*acc ; v += bias[n] ; if pre_out: pre_out[m,n] = v ;
 *   GELU: v = gelu_erf(v) (nn.GELU, model.py:25,156) ; GELU_BWD: v *= gelu_erf'(aux[m,n]) ;
 *   v += resid[m,n] (residual, model.py:67,68,165) ; ACCUM: v += C[m,n] ; C[m,n] = v.
 * compute: MCL_COMPUTE_F32 = v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate);
 *          MCL_COMPUTE_BF16 = operands rounded to bf16 at LDS staging, v_mfma_f32_32x32x16_bf16.
 */
#define MCL_EPI_GELU 1
#define MCL_EPI_GELU_BWD 2
#define MCL_EPI_ACCUM 4
#define MCL_COMPUTE_F32 0
#define MCL_COMPUTE_BF16 1

typedef struct mcl_gemm_args {
  uint32_t struct_size;  /* ABI 8: sizeof(mcl_gemm_args) AS THE CALLER COMPILED / DECLARED IT.  The struct travels by pointer and
                            has grown (ABI 7 appended the flt_* block): mcl_gemm copies min(struct_size, its own sizeof) bytes and
                            reads every field beyond the caller's size as zero / NULL, so a binding written against a shorter
                            layout stays valid; a size below the end of `workspace` (the ABI-6 fields) is MCL_EINVAL.  */
  int32_t M, N, K, batch;
  const float* A; int64_t sAm, sAk, sAb;
  const float* B; int64_t sBk, sBn, sBb;
  float* C; int64_t ldc, sCb;
  float alpha;
  int32_t flags;         /* MCL_EPI_* */
  const float* bias;     /* [N] or NULL */
  const float* resid; int64_t ldr, sRb;  /* NULL or (M,N) per batch */
  float* pre_out; int64_t ldp;           /* NULL or (M,N): pre-activation store (batch must be 1) */
  const float* aux; int64_t ldaux;       /* (M,N) for MCL_EPI_GELU_BWD (batch must be 1) */
  int32_t compute;       /* MCL_COMPUTE_* */
  int32_t ksplit;        /* 0 / 1: one pass.  > 1: K is cut into that many slices whose fp32 partials go to
                            `workspace` and a second launch adds them in fixed order and applies the epilogue
                            (deterministic; for skinny problems such as the spot path's M = batch of 128 spots) */
  float* workspace;      /* >= mcl_gemm_workspace_floats(M, N, batch, ksplit) floats when ksplit > 1, else unused */
  /* ABI 7: threshold FILTER instead of the C store (fused similarity + top-k, /root/reference/evel_her2st.py:74-84).
   * flt_thr != NULL: nothing is written to C (may be NULL); every product alpha * (A B)[i][j] >= flt_thr[i] is appended to row i's
   * candidate list: pos = atomic flt_cnt[i]++ (zero on entry), flt_val[i * flt_cap + pos] = value, flt_idx[...] = j when
   * pos < flt_cap (flt_cnt keeps counting past the capacity: the caller sees the overflow).  batch 1, no split-K, no epilogue. */
  const float* flt_thr; int32_t* flt_cnt; float* flt_val; int32_t* flt_idx; int32_t flt_cap;
  /* Reserved (ABI 9 - 10: split-K in one launch, measured slower and removed at ABI 11).  Ignored: split-K always merges the
   * slices in a second launch, and the array, if any, is neither read nor written. */
  uint32_t* counters;
} mcl_gemm_args;

int mcl_gemm(const mcl_gemm_args* args, mcl_stream_t stream);
/* sizeof(mcl_gemm_args) of THIS library build and the smallest struct_size it accepts (the fields up to `workspace`): a binding
 * in a language without the header (ctypes, cgo, JNI) checks its own struct declaration against these at load time. */
uint32_t mcl_gemm_args_size(void);
uint32_t mcl_gemm_args_min_size(void);
/* Slices that give a problem with few 64x64 output tiles ~256 workgroups (1 = do not split). */
int32_t mcl_gemm_auto_ksplit(int32_t M, int32_t N, int32_t K, int32_t batch);
int64_t mcl_gemm_workspace_floats(int32_t M, int32_t N, int32_t batch, int32_t ksplit);
/* n <= 4 independent problems as ONE launch (a layer's backward: its weight gradients and its data gradient are a few dozen
 * 64x64 tiles each).  `args`: an array of mcl_gemm_args, args[0].struct_size bytes apart, every element with the same
 * struct_size.  Each problem keeps its own layouts and epilogue; results are bit-identical to n separate mcl_gemm calls.
 * Restrictions: compute MCL_COMPUTE_F32, batch 1, ksplit <= 1, no filter epilogue -> MCL_EUNSUPPORTED otherwise.           */
int mcl_gemm_group(const mcl_gemm_args* args, int32_t n, mcl_stream_t stream);

/* ---------------------------------------------------------------- K7 ProjectionHead (model.py:151-168), projection_dim = 256
 * Forward as ONE launch, exact fp32 (csrc/proj_head.hip):
 *     p = x Wp^T + bp ;  a = gelu(p) ;  z = a Wf^T + bf + p ;  e = LayerNorm(z; gamma, beta, eps)      (dropout p = 0)
 * x (M, D) row stride ldx; Wp (256, D) row stride ldwp; Wf (256, 256) row stride ldwf; bp, bf, gamma, beta (256).
 * Outputs, all dense (M, 256) / (M): e, and for the backward p, a, z, mean, rstd.  The first product is cut into `ksplit`
 * K slices over the grid (mcl_proj_head_ksplit(M, D) recommends; 1..16); the last workgroup to arrive at a block of 16 rows adds
 * the slices in slice order (bit-reproducible) and finishes the rows.  ws: >= mcl_proj_head_ws_floats(M, ksplit) floats;
 * counters: ceil(M / 16) uint32, ZERO before the first call and left zero by every call -- one counter array per concurrently
 * running call.  16-byte aligned: e, p, a, z, ws, bp, gamma, beta.
 * Backward, row-local part as ONE launch:
 *     dz = LayerNorm'(de) ;  dp = (dz Wf) * gelu'(p) + dz ;  dgamma = sum_rows de * xhat, dbeta = sum_rows de,
 *     dbf = sum_rows dz, dbp = sum_rows dp     (bit i of accumulate_mask: output i of (dgamma, dbeta, dbf, dbp) is added to --
 *     the parameter's .grad -- instead of overwritten; a NULL output is skipped; sums over row blocks in block order).
 * dz, dp dense (M, 256); ws >= ceil(M / 16) * 1024 floats; counter: ONE zero uint32, as above.  The remaining three products
 * (dWf = dz^T a, dWp = dp^T x, dx = dp Wp) are plain problems for mcl_gemm_group.                                              */
int32_t mcl_proj_head_ksplit(int32_t M, int32_t D);
int64_t mcl_proj_head_ws_floats(int32_t M, int32_t ksplit);
int mcl_proj_head_fwd(const float* x, int64_t ldx, int32_t M, int32_t D, const float* wp, int64_t ldwp, const float* bp,
                      const float* wf, int64_t ldwf, const float* bf, const float* gamma, const float* beta, float eps,
                      float* e, float* p, float* a, float* z, float* mean, float* rstd, float* ws, uint32_t* counters,
                      int32_t ksplit, mcl_stream_t stream);
int mcl_proj_head_bwd_rows(const float* de, int64_t ldde, int32_t M, const float* z, const float* mean, const float* rstd,
                           const float* gamma, const float* p, const float* wf, int64_t ldwf, float* dz, float* dp,
                           float* dgamma, float* dbeta, float* dbf, float* dbp, int32_t accumulate_mask, float* ws,
                           uint32_t* counter, mcl_stream_t stream);

/* ---------------------------------------------------------------- K1 position-embedding add
 * model.py:230-235:  out[b,:] = expr[b,:] + X[(long)pos[b,0],:] + Y[(long)pos[b,1],:]
 * (tables model.py:204-205, 65536 rows).  (long) truncates toward zero.  ix/iy (int32, B) receive
 * the indices for the backward.  Indices outside [0,n_rows) are clamped and *err_flag (device int,
 * may be NULL) is set to 1 -- nn.Embedding would raise.                                        */
int mcl_pos_embed_add_fwd(const float* expr, int64_t ld_expr, const float* pos /*(B,2)*/,
                          const float* x_table, const float* y_table, int64_t ld_table, int32_t n_rows,
                          float* out, int64_t ld_out, int32_t* ix, int32_t* iy, int32_t* err_flag,
                          int32_t B, int32_t G, mcl_stream_t stream);

/* Backward of the gather (autograd of nn.Embedding, dense in the reference: two (65536,G) grads).
 * Row-sparse, deterministic: slot b is "owner" iff no b' < b has idx[b'] == idx[b]; then
 * row_grad[b,:] = sum_{b'>=b, idx[b']==idx[b]} d_out[b',:] (ascending b') and owner_idx[b] = idx[b];
 * otherwise owner_idx[b] = -1 and row_grad[b,:] is untouched.                                   */
int mcl_embed_rowgrad(const float* d_out, int64_t ld_dout, const int32_t* idx, int32_t* owner_idx,
                      float* row_grad, int64_t ld_rg, int32_t B, int32_t G, mcl_stream_t stream);

/* Dense scatter of owner rows: table_grad[owner_idx[b],:] (+)= row_grad[b,:] for owners
 * (accumulate != 0 adds, else overwrites).  For drop-in use with a stock dense optimizer.      */
int mcl_embed_scatter_rows(const int32_t* owner_idx, const float* row_grad, int64_t ld_rg, float* table_grad,
                           int64_t ld_table, int32_t B, int32_t G, int32_t accumulate, mcl_stream_t stream);

/* ---------------------------------------------------------------- K2 LayerNorm (model.py:13,17,158,166)
 * y = (x-mean)*rstd*gamma + beta over the last dim (biased variance, eps inside the sqrt).
 * mean/rstd (rows) are saved for the backward.                                                */
int mcl_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y, int64_t ldy,
                      float* mean, float* rstd, int32_t rows, int32_t cols, float eps, mcl_stream_t stream);
/* dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) (+ dx_add if non-NULL: the residual branch's gradient,
 * may alias dx), g = dy*gamma.  dgamma/dbeta (cols) are OVERWRITTEN with the column sums over rows (accumulate_params != 0:
 * added to).  ABI 9: dgamma == dbeta == NULL computes dx alone (the parameter gradients then belong to a grouped
 * mcl_colred_group launch).                                                                              */
int mcl_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                      const float* mean, const float* rstd, const float* dx_add, int64_t ldadd, float* dx,
                      int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate_params, int32_t rows, int32_t cols,
                      mcl_stream_t stream);

/* Fused attention core of the spot Transformer (/root/reference/model.py:49-57), head dimension 64, fp32 on the matrix cores
 * (v_mfma_f32_32x32x2_f32), no (heads, B, B) tensor in HBM.  qkv: (B, 3*heads*64) fp32, row stride ld, columns q | k | v,
 * head-major inside each; out: (B, heads*64), row stride ldo; lse: (heads, B) row log-sum-exp of the scaled scores (all the
 * backward needs beside qkv and out).  Backward: dqkv (B, 3*heads*64, row stride ldq) from dout (row stride ldo, as out);
 * dvec: (heads, B) fp32 scratch.  One launch forward, two backward (the unfused sequence: 3 + 5).  16-byte aligned bases,
 * strides multiples of 4 floats; dim_head != 64 -> MCL_EUNSUPPORTED (callers keep the GEMM + softmax path for it).      */
int mcl_attention_fwd(const float* qkv, int64_t ld, int32_t B, int32_t heads, int32_t dim_head, float scale, float* out,
                      int64_t ldo, float* lse, mcl_stream_t stream);
int mcl_attention_bwd(const float* qkv, int64_t ld, int32_t B, int32_t heads, int32_t dim_head, float scale, const float* out,
                      const float* dout, int64_t ldo, const float* lse, float* dvec, float* dqkv, int64_t ldq,
                      mcl_stream_t stream);
/* The same core over nseq independent sequences of B tokens each (ABI 7): rows sequence-major, lse / dvec (nseq, heads, B).
 * The fp32 ("reference numerics") ViT image encoder runs it with one sequence per image (/root/reference/model.py:104-116:
 * timm's Attention inside vit_base_patch{16,32}_224, T = 197 / 50 tokens). */
int mcl_attention_batched_fwd(const float* qkv, int64_t ld, int32_t B, int32_t nseq, int32_t heads, int32_t dim_head, float scale,
                              float* out, int64_t ldo, float* lse, mcl_stream_t stream);
int mcl_attention_batched_bwd(const float* qkv, int64_t ld, int32_t B, int32_t nseq, int32_t heads, int32_t dim_head, float scale,
                              const float* out, const float* dout, int64_t ldo, const float* lse, float* dvec, float* dqkv,
                              int64_t ldq, mcl_stream_t stream);
/* ---------------------------------------------------------------- K4 attention softmax (model.py:53-54)
 * In place over n_rows rows of length cols (row stride ld):  p = softmax(scale * s).           */
int mcl_softmax_rows_fwd(float* s, int64_t ld, int32_t n_rows, int32_t cols, float scale, mcl_stream_t stream);
/* In place on dp:  ds = scale * p * (dp - sum_j dp_j p_j).                                     */
int mcl_softmax_rows_bwd(const float* p, float* dp, int64_t ld, int32_t n_rows, int32_t cols, float scale,
                         mcl_stream_t stream);

/* ---------------------------------------------------------------- bias gradient
 * out[n] = sum_m x[m,n]  (nn.Linear bias backward).                                           */
int mcl_colsum(const float* x, int64_t ldx, float* out, int32_t rows, int32_t cols, int32_t accumulate, mcl_stream_t stream);
/* n <= 6 column reductions over the same number of rows (<= 1024) as ONE launch -- a Transformer layer's bias gradients and
 * LayerNorm parameter gradients (model.py:13,17,23,27,45).  Host arrays of n entries.  x[i] == NULL: out0[i][c] (+)= sum_r a[i][r, c]
 * (mcl_colsum).  x[i] != NULL: out0[i][c] (+)= sum_r a[i][r, c] * (x[i][r, c] - mean[i][r]) * rstd[i][r] and out1[i][c] (+)=
 * sum_r a[i][r, c] (the dgamma / dbeta of mcl_layernorm_bwd, which computes dx alone when its dgamma and dbeta are both NULL).
 * accumulate[i] != 0: +=.  Per problem bit-identical to the separate launches.                                              */
int mcl_colred_group(int32_t n, const float* const* a, const int64_t* lda, const float* const* x, const int64_t* ldx,
                     const float* const* mean, const float* const* rstd, float* const* out0, float* const* out1,
                     const int32_t* cols, const int32_t* accumulate, int32_t rows, mcl_stream_t stream);
/* ABI 7: the two column reductions above for MANY rows (the fp32 ViT's 6 400 - 25 216 token rows).  With a workspace of
 * mcl_rowred_workspace_floats(rows, cols) floats and rows > 1024 the rows are reduced in 128-row chunks on a 2-D grid and the
 * chunk partials added in chunk order by a second launch (deterministic); otherwise exactly the calls above. */
int64_t mcl_rowred_workspace_floats(int32_t rows, int32_t cols);
int mcl_colsum_ws(const float* x, int64_t ldx, float* out, int32_t rows, int32_t cols, int32_t accumulate, float* workspace,
                  mcl_stream_t stream);
int mcl_layernorm_bwd_ws(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, const float* mean,
                         const float* rstd, const float* dx_add, int64_t ldadd, float* dx, int64_t lddx, float* dgamma,
                         float* dbeta, int32_t accumulate_params, int32_t rows, int32_t cols, float* workspace, mcl_stream_t stream);

/* ---------------------------------------------------------------- f4: soft-target contrastive loss, elementwise middle (ABI 7)
 * /root/reference/baselines/Bleep/models.py:34-43,66-76,228-234.  Given S = E_s E_i^T / T, the soft targets Tg (row softmax),
 * the row / column log-sum-exp of S (mcl_infonce_lse) and the column sums of Tg (mcl_colsum), ONE pass writes
 * dS = c (softmax_row(S) + softmax_col(S) tcol - 2 Tg), dA = -c (logsoftmax_row(S) + logsoftmax_col(S)) and, per row, the loss
 * partial loss_rows[i] = -c sum_j Tg_ij (logsoftmax_row + logsoftmax_col)_ij (their sum is the loss; c = 1 / (2B)).  All (B, B)
 * row-major fp32.  mcl_symmetrize: out = (a + a^T) / 2 (out != a). */
int mcl_soft_clip_mid(const float* S, const float* Tg, const float* lse_row, const float* lse_col, const float* tcol, int32_t B,
                      float c, float* dS, float* dA, float* loss_rows, mcl_stream_t stream);
int mcl_symmetrize(const float* a, int32_t B, float* out, mcl_stream_t stream);

/* ---------------------------------------------------------------- K8 symmetric InfoNCE (model.py:242-247)
 * Works on a logits strip S (R x C, already divided by T): this rank's rows are global rows
 * [row0,row0+R) and its columns are global columns [col0,col0+C); the target (identity) entry of
 * local (i,j) is at row0+i == col0+j.
 *
 * mcl_infonce_lse: row_lse[i] = LSE_j S_ij (if row_lse != NULL) and col_lse[j] = LSE_i S_ij (if
 * col_lse != NULL), max-subtracted.                                                            */
int mcl_infonce_lse(const float* S, int64_t ldS, int32_t R, int32_t C, float* row_lse, float* col_lse,
                    mcl_stream_t stream);
/* loss_sum[0] (+)= sum_i (row_lse[i] - S_ii)  and  loss_sum[1] (+)= sum_j (col_lse[j] - S_jj) over
 * the target entries present in this strip; n_diag = how many to visit starting at local
 * (di0, dj0).  The reference's loss is (loss_sum[0]+loss_sum[1]) / (2*B_glob).                 */
int mcl_infonce_loss(const float* S, int64_t ldS, const float* row_lse, const float* col_lse,
                     int32_t di0, int32_t dj0, int32_t n_diag, int32_t use_rows, int32_t use_cols,
                     float* loss_sum, mcl_stream_t stream);
/* dS_ij = coef * (exp(S_ij-row_lse[i]) + exp(S_ij-col_lse[j]) - 2*[row0+i == col0+j]), written to
 * dS (may alias S).  coef = 1/(2*B_glob*T) folds the temperature of model.py:242.              */
/* loss_out[0] = (sum_t (row_lse[t] - S[t][t]) + sum_t (col_lse[t] - S[t][t])) / denom over the n diagonal entries: the
 * scalar of /root/reference/model.py:244-247 in ONE launch (mcl_infonce_loss accumulates the two sums for the strip form
 * and leaves the final add / divide to the caller).                                                                    */
int mcl_infonce_loss_mean(const float* S, int64_t ldS, const float* row_lse, const float* col_lse, int32_t n, float denom,
                          float* loss_out, mcl_stream_t stream);
int mcl_infonce_dlogits(const float* S, int64_t ldS, const float* row_lse, const float* col_lse, int32_t R,
                        int32_t C, int32_t row0, int32_t col0, float coef, float* dS, int64_t lddS,
                        mcl_stream_t stream);

/* ---------------------------------------------------------------- K8 fused InfoNCE (model.py:242-247), bf16 MFMA
 * The same loss without ever writing the logits to HBM (flash-attention-shaped; csrc/infonce_fused.hip).
 * a: (R, dim) and b: (C, dim) bf16 with row strides lda / ldb (elements, multiples of 8; bases 16-byte
 * aligned), dim == 256 (projection_dim); S = a b^T * inv_temp.
 * The positive pair of local row r is column r + diag_off (data parallel: rank * B_loc).  Calling with (a, b)
 * = (E_spot, E_img) gives the row direction of the symmetric loss, with (E_img, E_spot) the column direction.
 *
 * mcl_infonce_fused_lse:  lse[r] = log sum_c exp(S[r,c]);  diag[r] = S[r, r+diag_off] (written where that
 *   column exists; diag may be NULL).
 * mcl_infonce_fused_grad: dA[r,:] = coef * sum_c (exp(S[r,c]-lse_a[r]) + exp(S[r,c]-lse_b[c])
 *                                                - 2*[c == r+diag_off]) * b[c,:]      (fp32, (R, dim) contiguous)
 *   i.e. d loss / d a with coef = inv_temp / (2*B_glob): the closed-form backward of model.py:244-247.
 * workspace: mcl_infonce_fused_workspace_bytes(R, C, dim) bytes of device memory, 16-byte aligned.       */
int64_t mcl_infonce_fused_workspace_bytes(int32_t R, int32_t C, int32_t dim);
int mcl_infonce_fused_lse(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t R, int32_t C, int32_t dim,
                          int32_t diag_off, float inv_temp, float* lse, float* diag, void* workspace, int64_t ws_bytes,
                          mcl_stream_t stream);
int mcl_infonce_fused_grad(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t R, int32_t C, int32_t dim,
                           int32_t diag_off, float inv_temp, const float* lse_a, const float* lse_b, float coef, float* dA,
                           void* workspace, int64_t ws_bytes, mcl_stream_t stream);
/* y (bf16, row stride ldy) = round-to-nearest-even(x (fp32, row stride ldx)); cols % 8 == 0.             */
int mcl_cast_f32_to_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t cols,
                         mcl_stream_t stream);

/* ---- ViT image encoder on bf16 (csrc/gemm_bf16.hip, csrc/vit_ops.hip; /root/reference/model.py:104-116).
 * mcl_gemm_bf16: C[b] = epilogue(alpha * A[b] B[b]) with fp32 accumulation on the bf16 MFMA; per-operand storage flags
 * (bit 0: A stored reduction-major [K][M]; bit 1: B stored reduction-major [K][N]; default: A [M][K], B [N][K]),
 * bit 2: exact-erf GELU (pre_out != NULL also stores the pre-activation; with bit 5: stores gelu'(pre-activation) instead),
 * bit 3: multiply by gelu'(aux), bit 6: multiply by aux itself (aux = the derivative stored through bit 5), bit 4: fp32
 * output.  Two-level batch: problem bi = (bi / batch2, bi % batch2) with strides (s?b, s?b2) -- (image, head) for the
 * attention products.  bias [N] fp32, resid [M][N] bf16 (outer-batch stride sRb, 0 = broadcast).  Leading dimensions multiples of 8 (bf16) /
 * 4 (fp32 C); ragged M, N, K allowed; bf16 C needs ldc >= round_up(N, 8).  ksplit > 1 (fp32 output, batch 1, no
 * epilogue): the K range is split over workgroups, fp32 slabs in `workspace` (mcl_gemm_bf16_workspace_floats) are
 * merged in fixed order into C (accumulate != 0: +=) -- the weight-gradient form, deterministic.
 * ABI 11: flags bits 7-8 choose among the kernels that apply to the problem (for tests and A/B runs; production passes 0):
 * 0 auto (the pipelined kernel for bf16 output, the staggered one for fp32), 1 the lockstep kernel only, 2 the lockstep or
 * the staggered kernel, never the pipelined one, 3 the pipelined kernel wherever it applies (fp32 output included).  A
 * value never forces a kernel onto a problem it does not apply to (the staggered kernel: interior 256 x 256 tiles only; the
 * pipelined one: also K ranges of >= 128).  The lockstep and staggered kernels agree bit for bit, the pipelined one too
 * except for one bf16 ulp on the GELU epilogues.                                                                         */
int64_t mcl_gemm_bf16_workspace_floats(int32_t M, int64_t ldc, int32_t ksplit);
int mcl_gemm_bf16(const void* A, int64_t lda, int64_t sAb, const void* B, int64_t ldb, int64_t sBb, void* C, int64_t ldc,
                  int64_t sCb, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t batch2, int64_t sAb2, int64_t sBb2,
                  int64_t sCb2, float alpha, int32_t flags,
                  const float* bias, const void* resid, int64_t ldr, int64_t sRb, const void* aux, int64_t ldaux,
                  void* pre_out, int64_t ldp, int32_t ksplit, float* workspace, int32_t accumulate, mcl_stream_t stream);
/* LayerNorm over the last dimension D (multiple of 8, <= 1024) on bf16 rows, fp32 affine parameters and statistics. */
int mcl_ln_bf16_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, float* mean,
                    float* rstd, int64_t rows, int32_t D, float eps, mcl_stream_t stream);
/* dx = LayerNorm backward (+ dx_add); dgamma / dbeta (accumulate != 0: +=) merged deterministically.               */
int64_t mcl_colred_workspace_floats(int64_t rows, int32_t D);
int mcl_ln_bf16_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma, const float* mean,
                    const float* rstd, const void* dx_add, int64_t ldadd, void* dx, int64_t lddx, float* workspace,
                    float* dgamma, float* dbeta, int32_t accumulate, int64_t rows, int32_t D, mcl_stream_t stream);
/* out[c] (+)= sum over rows of a bf16 (rows, D) matrix (bias gradients), deterministic; D % 4 == 0, D <= 3072.      */
int mcl_colsum_bf16(const void* x, int64_t ldx, int64_t rows, int32_t D, float* workspace, float* out, int32_t accumulate,
                    mcl_stream_t stream);
/* Row softmax in place on bf16 scores (row length n <= 256, row stride ld; padding columns are zeroed) and its
 * backward in place on dP: dS = P * (dP - sum P dP) * scale.                                                        */
int mcl_softmax_bf16_fwd(void* s, int64_t ld, int64_t rows, int32_t n, mcl_stream_t stream);
int mcl_softmax_bf16_bwd(const void* P, void* dP, int64_t ld, int64_t rows, int32_t n, float scale, mcl_stream_t stream);
/* Fused attention core of the ViT encoder (csrc/vit_attention.hip; replaces the reference's timm Attention.forward core,
 * /root/reference/model.py:104-116 -> timm vision_transformer.Attention: softmax(q k^T scale) v per image and head), bf16,
 * head dimension 64, T <= 224 tokens, no (B heads, T, T) tensor in HBM.  qkv (B, T, 3 heads 64) bf16 as the qkv linear
 * writes it; o / dout (B, T, heads 64) bf16; lse, dsum (B heads, T) fp32 (dsum is scratch written by the backward);
 * dqkv (B, T, 3 heads 64) bf16, every element written.  T > 224 -> MCL_EUNSUPPORTED (callers keep the GEMM + softmax path). */
int mcl_vit_attn_fwd(const void* qkv, void* o, float* lse, int32_t B, int32_t T, int32_t heads, float scale, mcl_stream_t stream);
int mcl_vit_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, float* dsum, void* dqkv, int32_t B,
                     int32_t T, int32_t heads, float scale, mcl_stream_t stream);
/* ---- the ViT's token assembly and token mean on own kernels (csrc/glue.hip; timm VisionTransformer.forward_features behind
 * /root/reference/model.py:104-116).  x / dx: (B, T, D) with T = patches + 1, row 0 of an image = the class token; dtype 0 = fp32,
 * 1 = bf16; cls (D), pos (T*D) fp32 parameters.
 *   mcl_vit_patchify_tokens  mcl_vit_patchify with (lead_zero_row) one zero row in front of every image's patches -- the (B, T, K)
 *                            token matrix whose row 0 carries no patch -- and (out_f32) an fp32 result;
 *   mcl_vit_cls_row          x[b][0] = cls + pos[0]                        (the patch rows come from the patch GEMM's epilogue)
 *   mcl_vit_assemble_f32     x[b][0] = cls + pos[0] ; x[b][t] = tok[b*(T-1) + t-1] + pos[t]          (fp32 path)
 *   mcl_vit_tokens_extract   dtok[b*(T-1) + t-1] = dx[b][t], t >= 1
 *   mcl_vit_token_mean_fwd   feat[b] = mean over t >= 1 of x[b][t]  (fp32, token order)              (global_pool = 'avg')
 *   mcl_vit_token_mean_bwd   dx[b][0] = 0 ; dx[b][t >= 1] = dfeat[b] / (T - 1)
 *   mcl_vit_pos_grad         dpos[t] (+)= sum_b dx[b][t] (batch order) ; dcls (+)= its t = 0 row (NULL: skipped);
 *                            accumulate: bit 0 adds into dpos, bit 1 adds into dcls
 *   mcl_vit_zero_cls_rows    dx[b][0] = 0                                   (before the patch-embedding bias gradient)        */
int mcl_vit_patchify_tokens(const float* img, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int32_t B, int32_t H, int32_t W,
                            int32_t p, void* out, int32_t lead_zero_row, int32_t out_f32, mcl_stream_t stream);
int mcl_vit_cls_row(const float* cls, const float* pos, void* x, int32_t B, int32_t T, int32_t D, int32_t dtype,
                    mcl_stream_t stream);
int mcl_vit_assemble_f32(const float* tok, const float* cls, const float* pos, float* x, int32_t B, int32_t T, int32_t D,
                         mcl_stream_t stream);
int mcl_vit_tokens_extract(const void* dx, void* dtok, int32_t B, int32_t T, int32_t D, int32_t dtype, mcl_stream_t stream);
int mcl_vit_token_mean_fwd(const void* x, float* feat, int32_t B, int32_t T, int32_t D, int32_t dtype, mcl_stream_t stream);
int mcl_vit_token_mean_bwd(const float* dfeat, void* dx, int32_t B, int32_t T, int32_t D, int32_t dtype, mcl_stream_t stream);
int mcl_vit_pos_grad(const void* dx, float* dpos, float* dcls, int32_t B, int32_t T, int32_t D, int32_t dtype,
                     int32_t accumulate, mcl_stream_t stream);
int mcl_vit_zero_cls_rows(void* dx, int32_t B, int32_t T, int32_t D, int32_t dtype, mcl_stream_t stream);
/* 4-D strided copy of an fp32 source, element strides on both sides: dst[i . d] (+)= src[i . a], i over (n0, n1, n2, n3); dst fp32
 * (dst_dtype 0) or bf16 (1).  Packs a Conv2d weight of any memory format into the (c, iy, ix) column order of the patch GEMM
 * (with the cast), and adds a contiguous weight gradient into a .grad that has the parameter's own strides.               */
int mcl_strided4_f32(const float* src, int32_t n0, int32_t n1, int32_t n2, int32_t n3, int64_t a0, int64_t a1, int64_t a2,
                     int64_t a3, void* dst, int64_t d0, int64_t d1, int64_t d2, int64_t d3, int32_t dst_dtype, int32_t accumulate,
                     mcl_stream_t stream);
/* 2-D copy with row strides in BYTES (a channel slice of a channels-last buffer -> dense rows, or back); 2-byte granularity. */
int mcl_copy_rows(const void* src, int64_t ld_src_bytes, void* dst, int64_t ld_dst_bytes, int64_t rows, int64_t row_bytes,
                  mcl_stream_t stream);
/* wf[ci][ky][kx][co] = w[co][k-1-ky][k-1-kx][ci]: the weight of the "same" convolution that IS the backward-data pass of a
 * stride-1 convolution (w: (Co, k, k, Ci) storage = a channels-last Conv2d weight); dtype 0 fp32 / 1 bf16.                  */
int mcl_weight_rot180(const void* w, void* wf, int32_t Co, int32_t k, int32_t Ci, int32_t dtype, mcl_stream_t stream);
/* Patch extraction for the patch-embedding GEMM: out[(b, py, px)][c*p*p + iy*p + ix] (bf16) from an fp32 image
 * addressed by element strides (sb, sc, sy, sx): NCHW or channels-last.                                            */
int mcl_vit_patchify(const float* img, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int32_t B, int32_t H, int32_t W,
                     int32_t p, void* out_bf16, mcl_stream_t stream);

/* ---- fp8 (OCP e4m3) similarity contraction for the InfoNCE (csrc/infonce_fp8.hip; BASELINE configs[4]).
 * mcl_quant_e4m3_rows: per row one power-of-two scale 2^e (smallest with max|x| <= 448 * 2^e); q = e4m3_rne(x 2^-e),
 * scale byte = e + 127 (E8M0, what v_mfma_scale_f32_32x32x64_f8f6f4 consumes); optionally the dequantised copy in
 * bf16 (exactly representable).  x (rows, 256) fp32 row stride ldx; q (rows, 256) bytes row stride ldq; scale bytes
 * with byte stride ld_scale; deq (rows, 256) bf16 row stride ldd or NULL.  cols must be 256.                       */
int mcl_quant_e4m3_rows(const float* x, int64_t ldx, int32_t rows, int32_t cols, void* q, int64_t ldq, void* scale,
                        int64_t ld_scale, void* deq_bf16, int64_t ldd, mcl_stream_t stream);
int mcl_dequant_e4m3_rows(const void* q, int64_t ldq, const void* scale, int64_t ld_scale, int32_t rows, int32_t cols,
                          void* deq_bf16, int64_t ldd, mcl_stream_t stream);
/* lse[r] = log sum_c exp(inv_temp * sum_k (a8[r][k] 2^(sa[r]-127)) (b8[c][k] 2^(sb[c]-127))), logits never in HBM,
 * fp8 MFMA with hardware block scales, fp32 accumulate and statistics.  a8 (R, 256), b8 (C, 256) e4m3 bytes, row
 * strides multiples of 16.  workspace: mcl_infonce_fp8_workspace_bytes(R, C).                                      */
int64_t mcl_infonce_fp8_workspace_bytes(int32_t R, int32_t C);
int mcl_infonce_fp8_lse(const void* a8, int64_t lda, const void* scale_a, int64_t ld_sa, const void* b8, int64_t ldb,
                        const void* scale_b, int64_t ld_sb, int32_t R, int32_t C, int32_t dim, float inv_temp, float* lse,
                        void* workspace, int64_t ws_bytes, mcl_stream_t stream);
/* diag[r] = inv_temp * a[r] . b[r + diag_off] on bf16 rows (rows whose partner lies outside [0, C) are left untouched) */
int mcl_infonce_rowdot_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t R, int32_t C, int32_t dim,
                            int32_t diag_off, float inv_temp, float* diag, mcl_stream_t stream);

/* ---------------------------------------------------------------- K10 DenseNet BatchNorm(+ReLU), channels-last
 * Train-mode nn.BatchNorm2d (+ nn.ReLU) of the torchvision DenseNet-121 feature extractor that
 * model.py:75-76 wraps, on NHWC activations viewed as (S = B*H*W rows) x (C channels) with a row stride
 * ld (elements) -- so a dense layer reads its input as a channel slice of the block's concat buffer in
 * place (no torch.cat), per-channel statistics are computed once per produced feature map, and the
 * data gradient is accumulated in place.  dtype: 0 = fp32, 1 = bf16 activations; statistics and affine
 * parameters are fp32.  C must be a multiple of 4 (fp32) / 8 (bf16), bases 16-byte aligned.
 * workspace: mcl_bn_workspace_floats(S, C, dtype) floats.                                        */
int64_t mcl_bn_workspace_floats(int64_t S, int32_t C, int32_t dtype);
/* mean/var (biased)/rstd = 1/sqrt(var+eps) per channel; if copy_out != NULL also copies x there
 * (used to place a produced feature map into its slice of the concat buffer in the same pass).  */
int mcl_bn_stats(const void* x, int64_t ld, int64_t S, int32_t C, int32_t dtype, void* copy_out, int64_t ld_out,
                 float* workspace, float eps, float* mean, float* var, float* rstd, mcl_stream_t stream);
/* y = relu?( (x-mean)*rstd*gamma + beta ) */
int mcl_bn_act_fwd(const void* x, int64_t ldx, int64_t S, int32_t C, int32_t dtype, const float* gamma,
                   const float* beta, const float* mean, const float* rstd, int32_t relu, void* y, int64_t ldy,
                   mcl_stream_t stream);
/* g = dy*[y>0] (or dy); dgamma (+)= sum g*xhat; dbeta (+)= sum g  (accumulate_params != 0 adds into the
 * given buffers -- the parameters' .grad views of the flat optimizer bucket -- instead of overwriting);
 * dx (+)= gamma*rstd*(g - mean(g) - xhat*mean(g*xhat))   (accumulate != 0: read-modify-write of dx) */
int mcl_bn_act_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, int64_t S, int32_t C, int32_t dtype,
                   const float* gamma, const float* beta, const float* mean, const float* rstd, int32_t relu,
                   float* workspace, float* dgamma, float* dbeta, int32_t accumulate_params, void* dx, int64_t lddx,
                   int32_t accumulate, mcl_stream_t stream);

/* DenseNet bottleneck 1x1 convolution with both BatchNorms folded in (torchvision _DenseLayer norm1/relu1/conv1 +
 * norm2's statistics):   z[s][n] = sum_k relu(x[s][k]*g[k]*rstd[k] + beta[k] - mean[k]*g[k]*rstd[k]) * W[n][k],
 * n < 128;  zmean/zvar (biased)/zrstd = batch statistics of the bf16-rounded z.  x: (S, K) bf16 row stride ldx
 * (a channel slice of the block's concat buffer), W: (128, K) bf16 contiguous, z: (S, 128) bf16 row stride ldz.
 * K % 8 == 0, K <= 1024.  workspace: mcl_dense_conv1x1_workspace_floats(S) floats.  zmean = zvar = zrstd = NULL:
 * no statistics (inference, where mean/rstd are the running statistics of norm1 and norm2 uses its own).       */
int64_t mcl_dense_conv1x1_workspace_floats(int64_t S);
int mcl_dense_conv1x1_fwd(const void* x, int64_t ldx, int64_t S, int32_t K, const float* gamma, const float* beta,
                          const float* mean, const float* rstd, const void* W, void* z, int64_t ldz, float* workspace,
                          float eps, float* zmean, float* zvar, float* zrstd, mcl_stream_t stream);

/* DenseNet growth 3x3 convolution (pad 1, 128 -> 32) with both BatchNorms folded in (torchvision _DenseLayer
 * norm2/relu2/conv2 + the statistics of the new feature map), written straight into the concat buffer:
 *   y[p][co] = sum_{ky,kx,ci} relu(bn2(z))[p + (ky-1)*W + (kx-1)][ci] * W2[co][ky][kx][ci]   (zero outside the image)
 * z: (S, 128) bf16 contiguous NHWC pixels (S = B*H*W), W2: (32, 3, 3, 128) bf16 (a channels-last (32,128,3,3)
 * weight), out: bf16 with row stride ldo (the block buffer's channel slice), ymean/yvar (biased)/yrstd = batch
 * statistics of the bf16-rounded y (all three NULL: none, inference).  workspace:
 * mcl_dense_conv3x3_workspace_floats(S) floats.                                                           */
int64_t mcl_dense_conv3x3_workspace_floats(int64_t S);
int mcl_dense_conv3x3_fwd(const void* z, int64_t S, int32_t H, int32_t W, const float* gamma, const float* beta,
                          const float* mean, const float* rstd, const void* W2, void* out, int64_t ldo,
                          float* workspace, float eps, float* ymean, float* yvar, float* yrstd, mcl_stream_t stream);

/* Weight gradient of that 3x3 convolution: dW2[co][ky][kx][ci] (+)= sum_p dy[p][co] * relu(bn2(z))[p + tap][ci], the
 * normalised input recomputed from z on the fly; dW2: (32, 3, 3, 128) fp32 contiguous (the channels-last parameter's
 * .grad).  dy: (S, 32) bf16 row stride lddy; z: (S, 128) bf16 contiguous.  No atomics: every pixel group stores its fp32
 * partial (32 x 1152) in the workspace and a merge launch adds the partials in fixed order -> dW (accumulate_w != 0: +=).
 * Bit-reproducible.  workspace: mcl_dense_conv3x3_wrw_workspace_floats(S) floats.                                  */
int64_t mcl_dense_conv3x3_wrw_workspace_floats(int64_t S);
int mcl_dense_conv3x3_wrw_det(const void* dy, int64_t lddy, const void* z, int64_t S, int32_t H, int32_t W,
                              const float* gamma, const float* beta, const float* mean, const float* rstd,
                              float* workspace, float* dW, int32_t accumulate_w, mcl_stream_t stream);

/* Backward of a dense layer's head x -> norm1 -> relu1 -> conv1 (1x1) -> z with respect to x, fused (csrc/dense_bwd.hip):
 *   da = dz W1 ; g = da*[bn1(x) > 0] ; dgamma (+)= sum g*xhat ; dbeta (+)= sum g ;
 *   gbuf[s, :C] += gamma*rstd*(g - mean(g) - xhat*mean(g*xhat))
 * without materialising da (both passes recompute dz W1 on the matrix cores).  dz: (S, 128) bf16 contiguous, W1:
 * (128, C) bf16 contiguous, x and gbuf: (S, C) bf16 channel slices with row strides ldx / ldg.  accumulate_params
 * != 0 adds dgamma/dbeta into the given buffers (the parameters' .grad views).  C % 8 == 0.
 * workspace: mcl_dense_bn1_bwd_workspace_floats(S, C) floats.                                              */
int64_t mcl_dense_bn1_bwd_workspace_floats(int64_t S, int32_t C);
int mcl_dense_bn1_bwd(const void* dz, const void* W1, int32_t C, const void* x, int64_t ldx, int64_t S,
                      const float* gamma, const float* beta, const float* mean, const float* rstd, float* workspace,
                      float* dgamma, float* dbeta, int32_t accumulate_params, void* gbuf, int64_t ldg,
                      mcl_stream_t stream);

/* Round 6 -- two consecutive layers' dx passes as ONE pass over the channels both read (the BatchNorm-1 backward of the 56 x 56 /
 * 28 x 28 dense blocks re-reads and re-writes the block's whole growing gradient buffer once per layer: O(L^2) bytes).
 *   mcl_dense_bn1_dx_window  mcl_dense_bn1_dx restricted to the channel window [c0, c0 + nc) of the layer's C input channels
 *                            (c0 % 8 == 0): layer l's term on the 32 channels layer l-1 produced, which layer l-1's 3x3
 *                            backward consumes next;
 *   mcl_dense_bn1_dx_pair    gbuf[:, 0:C] += term_A + term_B for layer A = l (input C + 32 channels: W1A rows are ldwA long) and
 *                            layer B = l - 1 (input C channels), x and gbuf read once, gbuf written once; both dz W1 products
 *                            recomputed on the matrix cores; the two deltas are added in fp32 and rounded to bf16 once.
 * Operands as mcl_dense_bn1_dx (coef = that layer's mcl_dense_bn1_wrw output).                                             */
int mcl_dense_bn1_dx_window(const void* dz, const void* W1, int32_t C, int32_t c0, int32_t nc, const void* x, int64_t ldx,
                            int64_t S, const float* gamma, const float* beta, const float* mean, const float* rstd,
                            const float* coef, void* gbuf, int64_t ldg, mcl_stream_t stream);
int mcl_dense_bn1_dx_pair(const void* dzA, const void* W1A, int32_t ldwA, const float* gammaA, const float* betaA,
                          const float* coefA, const void* dzB, const void* W1B, const float* gammaB, const float* betaB,
                          const float* coefB, int32_t C, const void* x, int64_t ldx, int64_t S, const float* mean,
                          const float* rstd, void* gbuf, int64_t ldg, mcl_stream_t stream);

/* Deterministic replacement of the reduce launch of mcl_dense_bn1_bwd AND of the bottleneck weight gradient
 * (csrc/wrw_fused.hip): one pass over (dz, x) forms the Gram matrices R = dz^T mask and Qx = dz^T (mask*x) and from
 * them  dW1 (+)= dz^T relu(bn1(x))  [accumulate_w != 0: += into the parameter's fp32 .grad (128, C) contiguous],
 * dgamma / dbeta (+)= the BatchNorm-backward sums, and coef_out[2c] = mean(g), coef_out[2c+1] = mean(g*xhat) for
 * mcl_dense_bn1_dx.  Slab partials go through the workspace and are merged in fixed order: no atomics,
 * bit-reproducible.  Same operand layouts as mcl_dense_bn1_bwd.  workspace: mcl_wrw_workspace_floats(S, 128, C). */
int64_t mcl_wrw_workspace_floats(int64_t S, int32_t M, int32_t N);
int mcl_dense_bn1_wrw(const void* dz, const void* W1, int32_t C, const void* x, int64_t ldx, int64_t S,
                      const float* gamma, const float* beta, const float* mean, const float* rstd, float* workspace,
                      float* dW, int32_t accumulate_w, float* dgamma, float* dbeta, int32_t accumulate_params,
                      float* coef_out, mcl_stream_t stream);
/* The dx pass of mcl_dense_bn1_bwd alone, with the two per-channel means supplied (coef: 2*C floats).       */
int mcl_dense_bn1_dx(const void* dz, const void* W1, int32_t C, const void* x, int64_t ldx, int64_t S,
                     const float* gamma, const float* beta, const float* mean, const float* rstd, const float* coef,
                     void* gbuf, int64_t ldg, mcl_stream_t stream);
/* Single-pass form of mcl_dense_bn1_bwd for the latency-bound small maps.  dx = gamma*rstd*(g - mean g - xhat*mean(g*xhat)) is
 * linear in the two means, and the statistics (mean, rstd) of a concat-buffer channel are the same for every layer of a dense
 * block.  ONE kernel adds gamma*rstd*g into gbuf, reduces the two sums (no separate reduce pass over dz and x) and, when
 * have_prev != 0, subtracts on the same elements the mean terms of the PREVIOUS pass  kprev[c] = gamma*rstd*(mean g, mean g*xhat)
 * (2*C_total floats, [c][2]); its finalize adds dgamma / dbeta and overwrites kprev[0 .. C) with this layer's terms.  Every
 * layer's mean terms thus reach the channels the next layer reads one pass late, and mcl_dense_bn1_fix applies them to the
 * channels [c0, c0 + nc) the next pass does not cover (c0, nc multiples of 8):  gbuf[s][c] -= K1[c] + K2[c]*xhat[s][c].
 * workspace: mcl_dense_bn1_bwd_workspace_floats(S, C).  Replaces the same torch sequence as mcl_dense_bn1_bwd
 * (/root/reference/model.py:75-76 via torchvision _DenseLayer).                                                        */
int mcl_dense_bn1_dx_sums(const void* dz, const void* W1, int32_t C, const void* x, int64_t ldx, int64_t S,
                          const float* gamma, const float* beta, const float* mean, const float* rstd, float* workspace,
                          float* dgamma, float* dbeta, int32_t accumulate_params, float* kprev, int32_t have_prev, void* gbuf,
                          int64_t ldg, mcl_stream_t stream);
int mcl_dense_bn1_fix(const void* x, int64_t ldx, void* gbuf, int64_t ldg, int64_t S, int32_t c0, int32_t nc,
                      const float* mean, const float* rstd, const float* kacc, mcl_stream_t stream);
/* Deterministic 1x1 weight gradient dW[M][N] (+)= dz[S][M]^T a'[S][N]: a' = a (gamma..rstd NULL: transition
 * convolutions) or relu(BatchNorm(a)) recomputed in registers (all four given) -- the atomics-free form of
 * mcl_conv1x1_wrw_bf16.  workspace: mcl_wrw_workspace_floats(S, min(M,128), N).                                 */
int mcl_conv1x1_wrw_det(const void* dz, int64_t ldz, const void* a, int64_t lda, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* workspace, float* dW, int32_t accumulate_w,
                        int64_t S, int32_t M, int32_t N, mcl_stream_t stream);

/* Backward of a dense layer's tail z -> norm2 -> relu2 -> conv2 (3x3, pad 1, 128 -> 32) with respect to z, fused:
 *   da2 = conv3x3 backward-data of dy ; g2 = da2*[bn2(z) > 0] ; dgamma2 (+)= sum g2*zhat ; dbeta2 (+)= sum g2 ;
 *   dz = gamma2*rstd2*(g2 - mean(g2) - zhat*mean(g2*zhat)).
 * dy: (S, 32) bf16 row stride lddy (the gradient buffer's channel slice, read in place); W2: (32, 3, 3, 128) bf16;
 * z: (S, 128) bf16 contiguous NHWC pixels; g2 (scratch) and dz: (S, 128) bf16 contiguous.
 * workspace: mcl_dense_conv3x3_bwd_workspace_floats(S) floats.                                            */
int64_t mcl_dense_conv3x3_bwd_workspace_floats(int64_t S);
int mcl_dense_conv3x3_bwd(const void* dy, int64_t lddy, int64_t S, int32_t H, int32_t W, const void* W2, const void* z,
                          const float* gamma, const float* beta, const float* mean, const float* rstd, float* workspace,
                          float* dgamma, float* dbeta, int32_t accumulate_params, void* g2, void* dz, mcl_stream_t stream);
/* mcl_dense_conv3x3_bwd with mcl_dense_bn1_fix folded into the dy staging (single-pass BatchNorm-1 backward, maps narrower
 * than 17 pixels): dy' = dy - (K1 + K2*xhat) on the layer's 32 output channels (xfix: those channels of the concat buffer,
 * row stride ldxf; fmean / frstd: their statistics; fk: [32][2] mean terms of the previous pass), used for the data
 * gradient and written to dyc (S x 32 bf16 contiguous) for mcl_dense_conv3x3_wrw_det.  Bit-identical to the two launches. */
int mcl_dense_conv3x3_bwd_fix(const void* dy, int64_t lddy, int64_t S, int32_t H, int32_t W, const void* W2, const void* z,
                              const float* gamma, const float* beta, const float* mean, const float* rstd, float* workspace,
                              float* dgamma, float* dbeta, int32_t accumulate_params, void* g2, void* dz, const void* xfix,
                              int64_t ldxf, const float* fmean, const float* frstd, const float* fk, void* dyc,
                              mcl_stream_t stream);

/* Pooling layers of the DenseNet stem / transitions on channels-last bf16 (C % 8 == 0, 16-byte aligned, dense NHWC).
 * mcl_avgpool2_nhwc_bf16: AvgPool2d(2, 2); backward == 0: x (N,H,W,C) -> y (N,H/2,W/2,C); backward != 0: x is dy
 *   (N,H/2,W/2,C) and y receives dx (N,H,W,C) = dy/4.  H, W even.
 * mcl_maxpool3s2_*: MaxPool2d(3, stride 2, padding 1); the forward also records idx (one byte per output element:
 *   window position of the first maximum in row-major order, ATen's tie rule); the backward GATHERS dy through it:
 *   deterministic, no atomics.                                                                             */
int mcl_avgpool2_nhwc_bf16(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t backward,
                           mcl_stream_t stream);
int mcl_maxpool3s2_nhwc_bf16_fwd(const void* x, void* y, void* idx, int32_t N, int32_t H, int32_t W, int32_t C,
                                 mcl_stream_t stream);
int mcl_maxpool3s2_nhwc_bf16_bwd(const void* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                 mcl_stream_t stream);
/* the same with dy addressed through a row stride (elements per pooled pixel): the channel slice [:C] of a wider gradient
 * buffer is read in place (no contiguous copy of the first dense block's input gradient).                             */
int mcl_maxpool3s2_nhwc_bf16_bwd_ld(const void* idx, const void* dy, int64_t lddy, void* dx, int32_t N, int32_t H, int32_t W,
                                    int32_t C, mcl_stream_t stream);

/* DenseNet transition (torchvision _Transition: norm -> relu -> conv1x1 -> AvgPool2d(2,2)) with the pool moved in
 * front of the (linear, per-pixel) convolution:  p = avgpool2x2(relu(bn(x))), bf16 NHWC, x (N*H*W, C) with row stride
 * ldx, p (N*H/2*W/2, C) with row stride ldy; H, W even.  The convolution then runs on p (mcl_dense_conv1x1_fwd with an
 * identity prologue), a quarter of the pixels.
 * Backward: dp = gradient of p (pooled rows, row stride lddp); every pixel receives dp[pooled pixel]/4 through the
 * relu mask and the full train-mode BatchNorm backward: dgamma/dbeta (accumulated into when accumulate_params != 0)
 * and dx (written, row stride lddx).  workspace: mcl_bn_workspace_floats(N*H*W, C, 1) floats.                  */
int mcl_bn_act_avgpool_fwd(const void* x, int64_t ldx, int32_t N, int32_t H, int32_t W, int32_t C, const float* gamma,
                           const float* beta, const float* mean, const float* rstd, void* y, int64_t ldy,
                           mcl_stream_t stream);
int mcl_bn_act_avgpool_bwd(const void* dp, int64_t lddp, const void* x, int64_t ldx, int32_t N, int32_t H, int32_t W,
                           int32_t C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                           float* workspace, float* dgamma, float* dbeta, int32_t accumulate_params, void* dx,
                           int64_t lddx, mcl_stream_t stream);
/* DenseNet stem convolution conv0 (7x7, stride 2, pad 3, 3 -> 64; torchvision densenet121.features.conv0) with the
 * batch statistics of its output for norm0:  x (N,H,W,3) bf16 NHWC contiguous, Wt (64,7,7,3) bf16 (a channels-last
 * (64,3,7,7) weight), y (N,H/2,W/2,64) bf16 NHWC; mean/var (biased)/rstd of the bf16-rounded y (all three NULL:
 * none).  H % 4 == 0, W % 8 == 0, W <= 256.  workspace: mcl_conv0_workspace_floats(N, H, W) floats.            */
int64_t mcl_conv0_workspace_floats(int32_t N, int32_t H, int32_t W);
int mcl_conv0_fwd(const void* x, int32_t N, int32_t H, int32_t W, const void* Wt, void* y, float* workspace, float eps,
                  float* mean, float* var, float* rstd, mcl_stream_t stream);
/* Weight gradient of conv0: dW (64,7,7,3) fp32 (the channels-last parameter's .grad) (+)= sum_p dy[p] (x) patch(x)[p].
 * dy: (N,H/2,W/2,64) bf16 NHWC contiguous.  H % 4 == 0, W % 8 == 0, W <= 256.  workspace:
 * mcl_conv0_wrw_workspace_floats floats -- per-workgroup partials merged in fixed order (deterministic);
 * accumulate_w != 0 adds into dW, else overwrites.                                                              */
int64_t mcl_conv0_wrw_workspace_floats(int32_t N, int32_t H, int32_t W);
int mcl_conv0_wrw(const void* x, int32_t N, int32_t H, int32_t W, const void* dy, float* workspace, float* dW,
                  int32_t accumulate_w, mcl_stream_t stream);

/* DenseNet stem tail norm0 -> relu0 -> pool0 (MaxPool2d(3, 2, 1)) in one pass over the conv0 output x (N,H,W,C) bf16
 * NHWC contiguous: y (N,OH,OW,C) = maxpool(relu(bn(x))), idx = arg-max byte per pooled element (ky*3+kx, first maximum
 * in window order).  Backward: mcl_maxpool3s2_nhwc_bf16_bwd(idx, dy) followed by mcl_bn_act_bwd(relu = 1) on x
 * (fusing the gather into both BatchNorm-backward passes was measured slower: 388 us vs 217 us at 128 x 112^2 x 64). */
int mcl_bn_act_maxpool_fwd(const void* x, int32_t N, int32_t H, int32_t W, int32_t C, const float* gamma,
                           const float* beta, const float* mean, const float* rstd, void* y, void* idx,
                           mcl_stream_t stream);
/* dst[i] += (float)src[i], i < n, in storage order (src_dtype 0 = fp32, 1 = bf16): adds a low-precision
 * weight gradient into the fp32 .grad view of the flat optimizer bucket (both dense, identical strides). */
int mcl_accum_into_f32(float* dst, const void* src, int64_t n, int32_t src_dtype, mcl_stream_t stream);

/* ---------------------------------------------------------------- the last pieces of the step (csrc/step_misc.hip)
 * mcl_bn_gap_fwd: the tail of the DenseNet feature extractor, norm5 -> adaptive_avg_pool2d((1,1)) -> flatten
 *   (/root/reference/model.py:81-85; no ReLU): out[b][c] = gamma*rstd*(mean_hw x[b][hw][c] - mean[c]) + beta, fp32 (B, C);
 *   x = (B, HW, C) bf16 rows of stride ldx; xmean (B, C) fp32 (may be NULL) receives the raw pooled means for the backward.
 * mcl_bn_gap_bwd: from g = dL/dout (B, C) fp32: dgamma / dbeta (accumulate_params != 0: +=), coef (2C floats of scratch:
 *   the two BatchNorm-backward means) and dx (B, HW, C) bf16 = gamma*rstd*(g/HW - mean(dy) - xhat*mean(dy*xhat)) -- the
 *   train-mode BatchNorm backward with dy = g/HW broadcast over the map.  Deterministic (fixed-order sums over B).
 * mcl_bn_running_update: nn.BatchNorm2d's bookkeeping for n layers (HOST arrays of n device pointers / values):
 *   running_mean.lerp_(mean, momentum); running_var.lerp_(var * factor, momentum)  (factor = count / (count - 1): unbiased);
 *   num_batches_tracked += 1 (entries may be NULL).  The pointer table travels by value in the kernel arguments, 64 layers
 *   per launch.
 * mcl_image_to_bf16_nhwc: y (B, H, W, C) bf16 contiguous = x[b*sb + c*sc + y*sy + x*sx] (fp32, element strides): the
 *   ``image.to(bf16).contiguous(channels_last)`` in front of the stem for NCHW and channels-last inputs alike.
 * mcl_fill_zero: bytes (a multiple of 4, p 4-byte aligned) of zeros written by a kernel -- not hipMemsetAsync: a memset
 *   node inside the captured step graph cost the step its two-lane execution (measured).                              */
int mcl_bn_gap_fwd(const void* x, int64_t ldx, int32_t B, int32_t HW, int32_t C, const float* gamma, const float* beta,
                   const float* mean, const float* rstd, float* out, float* xmean, mcl_stream_t stream);
int mcl_bn_gap_bwd(const float* g, const float* xmean, const void* x, int64_t ldx, int32_t B, int32_t HW, int32_t C,
                   const float* gamma, const float* mean, const float* rstd, float* coef, float* dgamma, float* dbeta,
                   int32_t accumulate_params, void* dx, int64_t lddx, mcl_stream_t stream);
/* eval mode (evel_her2st.py:48-50: model.eval()): rstd_out[k][c] = 1 / sqrt(running_var[k][c] + eps[k]) for n BatchNorm
 * layers (HOST arrays of n device pointers / values), 64 layers per launch. */
int mcl_bn_eval_rstd(int32_t n, const float* const* running_var, float* const* rstd_out, const int32_t* C, const float* eps,
                     mcl_stream_t stream);
int mcl_bn_running_update(int32_t n, float* const* running_mean, float* const* running_var, const float* const* mean,
                          const float* const* var, int64_t* const* num_batches_tracked, const int32_t* C,
                          const float* factor, const float* momentum, mcl_stream_t stream);
int mcl_image_to_bf16_nhwc(const float* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int32_t B, int32_t C, int32_t H,
                           int32_t W, void* y, mcl_stream_t stream);
int mcl_fill_zero(void* p, int64_t bytes, mcl_stream_t stream);
/* nn.Dropout(p) / nn.GELU() / the residual add of the dropout > 0 path (model.py:25-29,156,164-165; never active in the
 * reference, model.py:217) as own elementwise kernels on contiguous fp32.  mcl_dropout_fwd: mask byte = 1 where kept (a
 * counter-based generator of (seed, element index): reproducible per seed), y = kept ? x / (1 - p) : 0; mcl_dropout_bwd:
 * dx = mask ? dy / (1 - p) : 0.  mcl_gelu_f32: out = dy ? dy * gelu'(x) : gelu(x) (exact erf form).                       */
int mcl_dropout_fwd(const float* x, float* y, void* mask, int64_t n, float p, uint64_t seed, mcl_stream_t stream);
int mcl_dropout_bwd(const float* dy, const void* mask, float* dx, int64_t n, float p, mcl_stream_t stream);
int mcl_gelu_f32(const float* x, const float* dy, float* out, int64_t n, mcl_stream_t stream);
int mcl_add_f32(const float* a, const float* b, float* y, int64_t n, mcl_stream_t stream);
/* debug: buf[idx] (uint64) = the GPU wall clock (100 MHz) when the stream reaches this point (MCL_STAMPS=1 timelines). */
int mcl_stamp(void* buf, int32_t idx, mcl_stream_t stream);
/* ya[i] = a[i] * s[0] (i < na), yb[i] = b[i] * s[0] (i < nb): a loss gradient scaled by autograd's upstream scalar (a
 * DEVICE value: no host read) for both embedding gradients in one launch.                                             */
int mcl_scale2_f32(const float* a, int64_t na, const float* b, int64_t nb, const float* s, float* ya, float* yb,
                   mcl_stream_t stream);

/* ---------------------------------------------------------------- generic convolution lowering + pooling, fp32 AND bf16
 * (csrc/im2col.hip, csrc/pool_generic.hip; dtype 0 = fp32, 1 = bf16).  For the shapes the specialised DenseNet kernels do not
 * cover: fp32 activations (the reference-numerics mode of the backbone, /root/reference/model.py:72-85) and the ResNet
 * encoders (/root/reference/model.py:88-148).  A convolution is im2col + this library's GEMM (mcl_gemm / mcl_gemm_bf16):
 *   mcl_im2col_nhwc: cols[(n,oy,ox)][(ky,kx,c)] = x[n][oy*stride-pad+ky][ox*stride-pad+kx][c] (0 outside); x rows of stride
 *     ldx (a channel slice is read in place); cols (N*OH*OW, KH*KW*C) contiguous; the column order is the storage order of a
 *     channels-last weight (C_out, kh, kw, C_in).
 *   mcl_col2im_nhwc: the transpose (backward-data): dx[n][y][x][c] (+)= the sum of the columns that reference the pixel, as a
 *     gather in fixed tap order (deterministic); dx rows of stride lddx.
 *   mcl_maxpool3s2_nhwc_{fwd,bwd}_any: MaxPool2d(3, 2, 1) with ATen's first-maximum tie rule, idx = one byte per element.
 *   mcl_avgpool2_nhwc_any: AvgPool2d(2, 2) (floor on odd maps) forward / backward.
 *   mcl_gap_nhwc_{fwd,bwd}: adaptive_avg_pool2d((1,1)) + flatten -> (B, C) fp32, and its backward g/HW broadcast.
 *   mcl_add_relu: y = relu(a + b) (backward != 0: y = a * [b > 0] with a = dy, b = the forward output).                 */
int mcl_im2col_nhwc(const void* x, int64_t ldx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t KH, int32_t KW,
                    int32_t stride, int32_t pad, int32_t dtype, void* cols, mcl_stream_t stream);
int mcl_col2im_nhwc(const void* dcols, int32_t N, int32_t H, int32_t W, int32_t C, int32_t KH, int32_t KW, int32_t stride,
                    int32_t pad, int32_t dtype, void* dx, int64_t lddx, int32_t accumulate, mcl_stream_t stream);
int mcl_maxpool3s2_nhwc_fwd_any(const void* x, void* y, void* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                                mcl_stream_t stream);
int mcl_maxpool3s2_nhwc_bwd_any(const void* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                int32_t dtype, mcl_stream_t stream);
int mcl_avgpool2_nhwc_any(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t backward, int32_t dtype,
                          mcl_stream_t stream);
int mcl_gap_nhwc_fwd(const void* x, int64_t ldx, int32_t B, int32_t HW, int32_t C, int32_t dtype, float* out,
                     mcl_stream_t stream);
int mcl_gap_nhwc_bwd(const float* g, int32_t B, int32_t HW, int32_t C, int32_t dtype, void* dx, mcl_stream_t stream);
/* backward: 0 = y = relu(a + b); 1 = dx = dy*[y > 0] (a = dy, b = forward output); 2 = y = a + b (gradient of a tensor with
 * two consumers: the fork in front of a residual block). */
int mcl_add_relu(const void* a, const void* b, void* y, int64_t n, int32_t backward, int32_t dtype, mcl_stream_t stream);

/* ---------------------------------------------------------------- a whole dense block, forward, 7 x 7 maps (ABI 6)
 * torchvision _DenseBlock (/root/reference/model.py:75-76: densenet121(...).features.denseblock4) in train mode as ONE
 * persistent launch: replaces, per layer, mcl_dense_conv1x1_fwd + mcl_dense_conv3x3_fwd (and their statistics finalize
 * launches) on H = W = 7 maps.  One workgroup per image (B <= compute units, all resident); the batch statistics are
 * exchanged in-launch (two all-to-all seams per layer, write-through stores + flags, fixed-order merges: deterministic).
 *   buf        (B, 7, 7, Ct) bf16 NHWC concat buffer, Ct = C0 + 32*L <= 1024; channels [0, C0) hold the block input on entry,
 *              channels [C0, Ct) are written;
 *   layer_ptrs HOST array of 10*L pointers, per layer: norm1.weight, norm1.bias (fp32 [C_in]), conv1 weight PACKED by
 *              mcl_dense_block_pack_w1 (bf16, 128*C_in elements in the kernel's MFMA-fragment streaming order),
 *              norm2.weight, norm2.bias (fp32 [128]), conv2 weight (bf16 [32][3][3][128]), z out (bf16 (B, 7, 7, 128), saved
 *              for the backward), norm2 batch mean / biased var / rstd out (fp32 [128] each);
 *   mean / var / rstd  fp32 [Ct] batch statistics of the concat channels: [0, C0) given (mean, rstd read), [C0, Ct) written;
 *   workspace  mcl_dense_block_fwd_workspace_bytes(B, L) bytes, 256-byte aligned; err_flag: device int32, set to 1 if a seam
 *              wait timed out (results invalid; never hangs).  The HOST must read it at its next synchronisation and discard
 *              the step (mclstexp_amd.ops.check_device_errors raises SeamTimeoutError);
 *   max_spins  bound of every seam poll loop (0 = the default, 2^19 polls ~ 0.5 s); a test passes 1 to force the timeout path;
 *   stamps     NULL, or a device buffer of B*L*8 uint64 that the launch fills with in-kernel phase stamps (100 MHz wall
 *              clock) per image and layer -- per call: the library keeps no state between calls.
 * Algorithmic bytes: the block input read once, z and the new channels written once (+ the weights).                      */
/* conv1 weights (bf16 [128][C_in_l], C_in_l = C0 + 32*l, k-contiguous rows) of the L layers -> the packed order (same sizes);
 * w1_ptrs / out_ptrs: HOST arrays of L device pointers.  One launch; run it whenever the weights have changed. */
int mcl_dense_block_pack_w1(const void* const* w1_ptrs, void* const* out_ptrs, int32_t L, int32_t C0, mcl_stream_t stream);
int64_t mcl_dense_block_fwd_workspace_bytes(int32_t B, int32_t L);
int mcl_dense_block_fwd(void* buf, int32_t B, int32_t H, int32_t W, int32_t Ct, int32_t C0, int32_t L,
                        const void* const* layer_ptrs, float eps1, float eps2, float* mean, float* var, float* rstd,
                        void* workspace, int32_t* err_flag, uint32_t max_spins, void* stamps, mcl_stream_t stream);

/* The same dense block BACKWARD (7 x 7 maps) as one persistent launch: replaces, per layer, mcl_dense_conv3x3_bwd_fix and
 * mcl_dense_bn1_dx_sums (+ their finalize launches and bn2_dz) with the same arithmetic; the two weight gradients of a layer
 * stay mcl_dense_conv3x3_wrw_det / mcl_conv1x1_wrw_det on the dz / dyc tensors this launch writes.
 *   buf        the forward's concat buffer (B, 7, 7, Ct) bf16;  gbuf: the block's gradient buffer, same shape: read whole,
 *              channels [0, C0) (the gradient of the block input) written back;
 *   layer_ptrs HOST array of 15*L pointers, per layer: norm1.weight, norm1.bias, conv1 weight packed by
 *              mcl_dense_block_pack_bwd (w1t), norm2.weight, norm2.bias, conv2 weight packed (w2t), z (forward, (B,7,7,128)),
 *              norm2 batch mean, norm2 batch rstd, dz out (B,7,7,128), dyc out (B,7,7,32: the gradient of the layer's output as
 *              consumed), then the fp32 gradients of norm1.weight, norm1.bias, norm2.weight, norm2.bias (ACCUMULATED into);
 *   mean / rstd  fp32 [Ct] batch statistics of the concat channels (forward);
 *   workspace  mcl_dense_block_bwd_workspace_bytes(B, L) bytes, 256-byte aligned; err_flag / max_spins / stamps as in the forward. */
int mcl_dense_block_pack_bwd(const void* const* w1_ptrs, const void* const* w2_ptrs, void* const* w1t_ptrs,
                             void* const* w2t_ptrs, int32_t L, int32_t C0, mcl_stream_t stream);
int64_t mcl_dense_block_bwd_workspace_bytes(int32_t B, int32_t L);
int mcl_dense_block_bwd(const void* buf, void* gbuf, int32_t B, int32_t H, int32_t W, int32_t Ct, int32_t C0, int32_t L,
                        const void* const* layer_ptrs, const float* mean, const float* rstd, void* workspace,
                        int32_t* err_flag, uint32_t max_spins, void* stamps, mcl_stream_t stream);

/* ---------------------------------------------------------------- K9 Adam with L2 weight decay
 * torch.optim.Adam(lr, betas, eps, weight_decay) as used by train.py:118-120, one fused pass:
 *   g += wd*p ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ;
 *   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),   bc1 = 1-b1^t, bc2 = 1-b2^t (host-computed).
 * Hyper-parameters are doubles (Python floats in torch.optim) and rounded to fp32 once, so that
 * 1-beta matches torch's double-computed constant.
 * Flat fp32 buffers of n elements (28 B/element of HBM traffic).                               */
int mcl_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, double bc1, double bc2, mcl_stream_t stream);
/* Same update for an embedding table (n_rows x cols, contiguous) whose data gradient is row-sparse:
 * g = wd*p + (row_slot[r] >= 0 ? row_grad[row_slot[r],:] : 0).  24 B/element: the dense zero
 * gradient of the reference (model.py:204-205 under autograd) is never materialised.
 * row_slot (n_rows int32) maps table row -> slot in row_grad or -1.                            */
int mcl_adam_table_step(float* p, float* m, float* v, int32_t n_rows, int32_t cols, const int32_t* row_slot,
                        const float* row_grad, int64_t ld_rg, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double bc1, double bc2, mcl_stream_t stream);

/* Graph-replayable Adam: the step counter (one int64) and the derived constants (8 floats) live on the device.
 * mcl_adam_consts_update advances the counter and refreshes the constants (one thread, double arithmetic, rounded once
 * as the host-constant entry points do); the _dev kernels read them, so nothing step-dependent is baked into a launch
 * and the whole optimizer step can sit inside a captured HIP graph.  `hyper` = DEVICE pointer to 5 doubles
 * {lr, beta1, beta2, eps, weight_decay}: the host refreshes them with an ordinary copy between replays, so an LR schedule
 * (torch.optim.lr_scheduler / a manual param_groups edit) is honoured by a captured step (ABI 2; ABI 1 took them by value
 * and froze them into the graph).                                                                                     */
int mcl_adam_consts_update(int64_t* step, float* consts, const double* hyper, mcl_stream_t stream);
int mcl_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* consts, mcl_stream_t stream);
int mcl_adam_table_step_dev(float* p, float* m, float* v, int32_t n_rows, int32_t cols, const int32_t* row_slot,
                            const float* row_grad, int64_t ld_rg, const float* consts, mcl_stream_t stream);
/* mcl_adam_step_dev with a bf16 shadow: additionally stores round-to-nearest-even(p) into shadow_bf16[i] (the flat low-
 * precision weight copy the backbone kernels read), so no separate cast pass over the parameters runs after the step. */
int mcl_adam_step_dev_shadow(float* p, const float* g, float* m, float* v, int64_t n, const float* consts,
                             void* shadow_bf16, mcl_stream_t stream);
/* Lazy-exact position-table Adam (ABI 6).  Replaces, for the two (65536, G) tables of /root/reference/model.py:204-205 under
 * /root/reference/train.py:118-120, the dense pass above: with L2 weight decay every row moves on every step, but a row
 * without a data gradient follows a recurrence in its own (p, m, v) and the step constants only.  Each row carries a
 * "valid through step" stamp (row_step, n_rows int32, 0 = initial state); a row is brought up to date by replaying its missed
 * steps in registers -- the same fp32 operation sequence as the dense kernel, with the constants those steps used, kept in a
 * ring `hist` of hist_len (power of two) x 8 floats that mcl_adam_consts_update_hist fills (slot = step & (hist_len - 1)) --
 * so the result is bit-identical to running mcl_adam_table_step_dev on every step.  The caller guarantees that no row is
 * more than hist_len - 1 steps behind (materialise in time).  One entry point, three uses; `step` = device step counter:
 *   catch-up of gathered rows (forward): pos != NULL ((n_owner, 2) fp32 positions; table 0 takes column 0, table 1 column 1);
 *       rows are advanced through *step; duplicates are resolved inside (first spot naming a row owns it);
 *   step with data gradients: owner0/owner1 (n_owner int32: row index or -1, as mcl_embed_rowgrad writes them) and
 *       row_grad0/row_grad1 ((n_owner, cols) fp32, leading dimension ld_rg); *step is the step being applied (already advanced
 *       by mcl_adam_consts_update_hist): rows are replayed through *step - 1, then updated with g = wd*p + row_grad;
 *   materialise: pos, owner*, row_grad* all NULL and n_owner == n_rows: every row is advanced through *step.
 * Table 1 is optional (p1 == NULL).  Algorithmic bytes: 24 B x touched rows x cols (+ the gradient rows).                */
int mcl_adam_consts_update_hist(int64_t* step, float* consts, const double* hyper, float* hist, int32_t hist_len,
                                mcl_stream_t stream);
int mcl_adam_table_lazy(float* p0, float* m0, float* v0, int32_t* row_step0, float* p1, float* m1, float* v1,
                        int32_t* row_step1, int32_t n_rows, int32_t cols, const float* pos, const int32_t* owner0,
                        const int32_t* owner1, int32_t n_owner, const float* row_grad0, const float* row_grad1, int64_t ld_rg,
                        const int64_t* step, const float* hist, int32_t hist_len, mcl_stream_t stream);
/* row_slot maintenance: set row_slot[owner_idx[b]] = b for owners (fill != 0) or back to -1.    */
int mcl_row_slot_update(int32_t* row_slot, const int32_t* owner_idx, int32_t B, int32_t fill, mcl_stream_t stream);

/* ---------------------------------------------------------------- inference-time retrieval
 * Replaces, on the device, the reference's find_matches() + weighting loop:
 *   evel_her2st.py:74-84,174-187 (top 200, L1 distance), evel_cscc.py:74-84,197-215 (top 600, values returned,
 *   L2 distance), evel_visium.py:94-104,193-205 (top 200, L2 distance).
 * mcl_l2_normalize_rows: y[r,:] = x[r,:] / max(||x[r,:]||_2, 1e-12)   (F.normalize(p=2, dim=-1)).
 *   The similarity matrix itself is mcl_gemm(query_n, key_n^T) with MCL_COMPUTE_F32.
 * mcl_topk_rows: torch.topk(sim, k) along each row of sim (rows x n, leading dimension ld): values (rows x k) best
 *   first and int64 indices; exact selection (radix select on the fp32 bit patterns), equal values ordered by
 *   ascending index.  k <= mcl_topk_rows_max_k() (2048), k <= n.
 * mcl_knn_weighted_average: per query i with neighbours idx = indices[i,:] (k of them):
 *     a_j = || spot_key[idx_j,:] - query[i,:] ||_ord   (ord = 1 or 2, UN-normalised embeddings, fp32)
 *     w_j = a_j^-2 / sum_j a_j^-2
 *     emb_pred[i,:]  = sum_j w_j spot_key[idx_j,:]        (n_query x dim,   may be NULL)
 *     expr_pred[i,:] = sum_j w_j expression_key[idx_j,:]  (n_query x genes, may be NULL)
 *   (np.average(..., weights=w)); the weighted sums accumulate in fp64.  An exact match (a_j = 0) yields a NaN row,
 *   as numpy's inf/inf does.                                                                     */
int mcl_l2_normalize_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int32_t rows, int32_t dim,
                          mcl_stream_t stream);
int mcl_topk_rows_max_k(void);
int mcl_topk_rows(const float* sim, int64_t ld, int32_t rows, int32_t n, int32_t k, float* values, int64_t* indices,
                  mcl_stream_t stream);
/* top-k of CANDIDATE LISTS (mcl_gemm's threshold filter): row i holds n (value, original column) pairs in arbitrary order, unused
 * slots -inf.  Returns the original columns, equal values ordered by original column like mcl_topk_rows.  A row whose k-th value is
 * an exact tie that would have to be cut by original column sets tie_flag[i] = 1 (its output is then unspecified: recompute that
 * row with mcl_topk_rows on the materialised similarities). */
int mcl_topk_rows_indexed(const float* cand_val, int64_t ld, const int32_t* cand_idx, int64_t ld_idx, int rows, int n, int k,
                          float* values, int64_t* indices, int32_t* tie_flag, mcl_stream_t stream);
int mcl_knn_weighted_average(const float* spot_key, int64_t ldk, const float* expression_key, int64_t lde,
                             const float* query, int64_t ldq, const int64_t* indices, int32_t n_query, int32_t k,
                             int32_t dim, int32_t genes, int32_t ord, float* emb_pred, float* expr_pred,
                             mcl_stream_t stream);

/* ---------------------------------------------------------------- scoring of expression predictions
 * Replaces, on the device, the closing block of the reference's evaluation scripts for ALL folds at once:
 *   evel_her2st.py:196-226, evel_cscc.py:226-261, evel_visium.py:212-244 and utils.py:52-65 (get_R, dim=1).
 * pred, truth: rows x G, leading dimensions ld_pred / ld_true (elements), dtype codes 0 = fp32, 1 = fp64, each its own.
 * offsets: S + 1 int64 row offsets IN DEVICE MEMORY, one segment (fold) per pair; preconditions the caller checks (the
 *   library cannot read them before launching): offsets[0] >= 0, strictly increasing, every segment >= 2 rows
 *   (scipy.stats.pearsonr raises below 2), offsets[S] <= the rows of both matrices.  Inputs are finite.
 * Per segment s, all fp64 (row-major, gene g at [s * G + g]):
 *   r[S x G]          Pearson r of pred[:, g] against truth[:, g] over the segment (scipy.stats.pearsonr as get_R calls it):
 *                     NaN when either column is exactly constant over the segment, otherwise clipped to [-1, 1];
 *   true_mean[S x G]  mean of truth[:, g] over the segment;
 *   heg[S x n_heg]    int64: the n_heg genes with the largest true_mean, best first, equal means by ascending gene index
 *                     (np.argsort(mean)[::-1][:50], evel_her2st.py:201-202);
 *   summary[S x 5]    { heg_pcc = mean of r over heg (NaN propagates, np.mean), hvg_pcc = mean of r over the non-NaN genes
 *                     (evel_her2st.py:209-213; NaN if there are none), mse = mean over genes of the per-gene mean of
 *                     (truth - pred)^2, mae = the same with |truth - pred| (sklearn's uniform average over outputs),
 *                     n_valid = the number of non-NaN r };
 *   work              2 * S * G doubles of scratch (the per-gene errors).
 * fp64 accumulation in two passes (means, then centred sums); no atomics: the reduction order depends only on
 * (segment length, G, n_heg), so a segment scored inside a batch is bit-identical to the same segment scored alone.
 * 1 <= n_heg <= G; S <= 65535.                                                                                    */
int mcl_expr_metrics(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                     int32_t true_dtype, const int64_t* offsets, int32_t S, int32_t G, int32_t n_heg, double* r,
                     double* true_mean, int64_t* heg, double* summary, double* work, mcl_stream_t stream);

/* ---------------------------------------------------------------- gene significance (csrc/gene_significance.hip; added
 * under ABI 13: new entry points only).  The second output of get_R (utils.py:52-65: scipy.stats.pearsonr's two-sided
 * p-value per gene) and the gene table of tutorial.ipynb's third cell.  All fp64, deterministic, no atomics.
 *
 * mcl_pearson_pvalue: r (S x G) as mcl_expr_metrics writes it, offsets[S + 1] the same device-resident int64 segment
 *   boundaries; n = the segment's length, a = n / 2 - 1.  Per element, into p and neglog10p (both S x G):
 *     r NaN (or n < 2)  -> both NaN;
 *     n == 2            -> p = 1, neglog10p = 0 (scipy's rule);
 *     |r| >= 1          -> p = 0, neglog10p = +inf;
 *     otherwise         log p = log 2 + log I_x(a, a), x = (1 - |r|) / 2: the prefactor lgamma(2a) - 2 lgamma(a) + a log x
 *                       + a log1p(-x) - log a plus the log of the continued fraction (modified Lentz, at most 1000 trips;
 *                       an element that has not converged by then is NaN, never a wrong number), clamped at 0;
 *                       neglog10p = -log p / ln 10 -- evaluated in log space, so it stays finite where p underflows;
 *                       p = exp(log p), which underflows to 0 as scipy's does.
 *   Every element depends on (r, n) alone: a segment inside a batch is bit-identical to the same segment alone.
 * mcl_gene_rank: neglog10p and r (S x G).  Per gene g, slides walked in index order:
 *     mean[g]        the mean of neglog10p[:, g] over its non-NaN entries (pandas mean(axis=1), skipna): NaN if there is
 *                    none, +inf if one of them is +inf;
 *     n_defined[g]   how many entries are not NaN;
 *     best_slide[g]  the first slide that attains the maximum over the non-NaN entries (pandas idxmax), -1 if none;
 *     best_value[g], best_r[g]   neglog10p and r at that slide (NaN if none);
 *   then order[G] int64: order[k] = the gene of rank k by descending mean -- exact rank by counting, equal means by
 *   ascending gene index, NaN means last.  The order is always full; top_n (1 <= top_n <= G) is how many leading
 *   entries the caller means to read and changes no result.
 * Both: S <= 65535 and G <= 1048576, MCL_EUNSUPPORTED beyond.                                                       */
int mcl_pearson_pvalue(const double* r, const int64_t* offsets, int32_t S, int32_t G, double* p, double* neglog10p,
                       mcl_stream_t stream);
int mcl_gene_rank(const double* neglog10p, const double* r, int32_t S, int32_t G, int32_t top_n, double* mean,
                  int32_t* n_defined, int64_t* order, int32_t* best_slide, double* best_value, double* best_r,
                  mcl_stream_t stream);

/* ---------------------------------------------------------------- BLEEP's prediction methods and scoring protocol
 * (csrc/bleep_eval.hip; added under ABI 13: new entry points only).  baselines/Bleep/BLEEP_inference.ipynb, cell 5 (the
 * three prediction methods and the scoring block) and cell 7 (the gene-gene-correlation matrices).  No floating-point
 * atomics; every reduction order depends only on the problem's own shape, so a segment scored inside a batch is
 * bit-identical to the same segment scored alone.
 *
 * mcl_knn_combine: arguments, NULL rules and the k * 8 <= 60000 limit of mcl_knn_weighted_average; fp32 in and out.  Per
 *   query i with neighbours idx = indices[i,:], by mode:
 *     0 FIRST      emb_pred[i,:] = spot_key[idx_0,:], expr_pred[i,:] = expression_key[idx_0,:], bit for bit (method "simple");
 *     1 MEAN       np.average(rows idx, axis=0)                                                  (method "average");
 *     2 BLEEP_EXP  d_j = sum_c (spot_key[idx_j,c] - query[i,c])^2, w_j = exp(-(d_j - d_0 + 1)), np.average(rows idx, axis=0,
 *                  weights=w) (method "weighted_average").  d_0 belongs to the best COSINE match, not to the nearest
 *                  neighbour, so an exponent can be positive; w_0 = exp(-1) keeps the weight sum above zero.
 *   d_j, the weights, their sum and the column sums are fp64 (the notebook: fp32 distances and weights); the result is
 *   rounded to fp32 once.  Any other mode: MCL_EUNSUPPORTED.  Rows are read with 16-byte loads where the matrix's base is
 *   16-byte aligned and its leading dimension a multiple of 4, else element by element.
 * mcl_cell_pearson: r_cell[i] = Pearson r of pred[i,:] against truth[i,:] over the G genes (np.corrcoef(...)[0, 1]) for
 *   every row: two passes, fp64; NaN when either row is exactly constant, otherwise clipped to [-1, 1].  dtype codes as in
 *   mcl_expr_metrics.  rows == 0 is MCL_OK.
 * mcl_bleep_summary: truth (rows x G), offsets[S + 1] device-resident as in mcl_expr_metrics, r_gene (S x G) as
 *   mcl_expr_metrics writes it, r_cell (rows) as mcl_cell_pearson writes it, markers: n_markers device int32 gene indices in
 *   [0, G) (the caller checks them; NULL when n_markers == 0).  Per segment s:
 *     gene_sum[S x G], gene_var[S x G]   np.sum / np.var (population variance) of the truth's columns, two passes, fp64;
 *     top_sum, top_var [S x n_top] int64  the n_top genes of largest sum / variance, best first, exact rank by counting, equal
 *                                        values to the HIGHER gene index first: np.argsort(kind="stable")[-n_top:][::-1];
 *     summary[S x 7]   { cell_mean = mean of the segment's non-NaN r_cell (NaN if none), n_cells_valid, n_genes_valid = the
 *                      number of non-NaN r_gene, max_r over them (NaN if none), heg_mean = mean of r_gene over top_sum (NaN
 *                      propagates, np.mean), hvg_mean = the same over top_var, marker_mean = the same over markers (NaN when
 *                      n_markers == 0) }.
 *   1 <= n_top <= G; S <= 65535 and G <= 1048576, MCL_EUNSUPPORTED beyond.  S == 0 is MCL_OK.
 * mcl_corr_from_gram: gram (m x m, row-major, dense) = a centred Gram matrix Xc^T Xc as mcl_pca_gram writes its primal form;
 *   corr[i,j] = gram[i,j] / sqrt(gram[i,i]) / sqrt(gram[j,j]) clipped to [-1, 1] (np.corrcoef), NaN where gram[i,i] or
 *   gram[j,j] is 0 (a constant column).  m <= 32768.                                                                 */
int mcl_knn_combine(const float* spot_key, int64_t ldk, const float* expression_key, int64_t lde, const float* query,
                    int64_t ldq, const int64_t* indices, int32_t n_query, int32_t k, int32_t dim, int32_t genes,
                    int32_t mode, float* emb_pred, float* expr_pred, mcl_stream_t stream);
int mcl_cell_pearson(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                     int32_t true_dtype, int64_t rows, int32_t G, double* r_cell, mcl_stream_t stream);
int mcl_bleep_summary(const void* truth, int64_t ld_true, int32_t true_dtype, const int64_t* offsets, int32_t S, int32_t G,
                      int32_t n_top, const double* r_gene, const double* r_cell, const int32_t* markers, int32_t n_markers,
                      double* gene_sum, double* gene_var, int64_t* top_sum, int64_t* top_var, double* summary,
                      mcl_stream_t stream);
int mcl_corr_from_gram(const double* gram, int32_t m, double* corr, mcl_stream_t stream);

/* ---------------------------------------------------------------- spatial-domain clustering (ABI 12; csrc/cluster.hip)
 * The reference's cluster() (utils.py:67-79): PCA -> k-means -> ARI / NMI against given labels, for S slides per call.
 * Common contract: row-stacked row-major device matrices, offsets[S + 1] device-resident int64 with offsets[0] = 0, every
 * segment non-empty; S <= 65535; all results fp64; floating-point sums are atomics-free and their order depends only on
 * the segment's own shape: a segment computed inside a batch is bit-identical to the same segment computed alone.
 *
 * mcl_pca_gram: x (rows, G), leading dimension ld >= G, dtype 0 = float32 / 1 = float64.  Per segment s of n_s rows:
 *   mean[s * G + g] = the column means, and at gram[gram_offsets[s]] the centred Gram matrix in its smaller form, row-major
 *   m_s x m_s with m_s = min(n_s, G): Xc^T Xc when n_s >= G ("primal"), else Xc Xc^T ("dual"); fp64 accumulation on
 *   v_mfma_f64_16x16x4_f64 in index order; full matrix, exactly symmetric.  gram_offsets[S + 1] (device int64) are element
 *   offsets, gram_offsets[s + 1] - gram_offsets[s] >= m_s^2.  max_rows = the largest n_s (sizes the grid).
 * mcl_pca_project: the top n_comps <= 64 eigenpairs of that matrix, found on the host or by mcl_sym_eig_top (whose outputs
 *   have this layout): evec at evec_offsets[s] (device int64
 *   element offsets) row-major (m_s, n_comps), eval[s * n_comps + c] the eigenvalues, best first.  Writes the scores
 *   z (rows, n_comps): primal Xc V, dual U sqrt(lambda) -- sklearn's PCA.fit_transform -- with each component's sign chosen
 *   so that its loading of largest magnitude (ties: the lowest column) is positive (sklearn >= 1.5's svd_flip on V);
 *   sign[s * n_comps + c] = +-1 is that factor; loadings: S * G * n_comps doubles of scratch.  n_s >= G decides primal / dual
 *   exactly as in mcl_pca_gram.
 * mcl_kmeans: z (rows, D) fp64, leading dimension ld; k[s] (device int32) clusters in segment s, 1 <= k[s] <= min(k_max, n_s)
 *   (otherwise that segment reports inertia NaN, n_iter -1, labels -1); D <= 64 and k_max <= 64, MCL_EUNSUPPORTED beyond.
 *   Grid (restart r < R, segment s): one workgroup runs one whole Lloyd problem in one launch.  Seeding: seeds != NULL:
 *   seeds[(s * R + r) * k_max + j] (device int64) is the row, inside the segment, of initial centre j; seeds == NULL:
 *   k-means++ with one candidate per centre (first centre uniform, then D^2 sampling through a fixed-order prefix sum) from
 *   a counter-based generator keyed by (seed, segment_base + s, r, draw) -- NOT NumPy's stream.  seeds_out gets the rows
 *   used, same layout.  Iteration = sklearn's algorithm="lloyd": nearest centre by squared Euclidean distance (ties: lowest
 *   centre), means; an emptied cluster takes the point farthest from its own centre (ties: lowest row); stop when no label
 *   changed, or when sum ||c_new - c_old||^2 <= tol * mean_d var(z[:, d]), or after max_iter iterations; then one final
 *   assignment unless the labels were already stable; inertia from the final labels and centres.
 *   Per restart: labels_all (R, rows) int32, centers_all (S, R, k_max, D), inertia_all (S, R), n_iter_all (S, R) int32;
 *   work: R * rows doubles of scratch.  A second launch picks per segment the restart of lowest inertia (ties: lowest r):
 *   labels (rows) int32, centers (S, k_max, D), inertia (S), n_iter (S) int32, restart (S) int32.
 * mcl_cluster_scores: labels_a ("true") and labels_b (rows) int32, values in [0, 1024), distinct(a) * distinct(b) <= 12288
 *   per segment (else that segment scores NaN); max_rows = the largest n_s <= 50000 (pair counts stay inside int64),
 *   MCL_EUNSUPPORTED beyond.  scores[2 s] = adjusted Rand index in sklearn's pair-confusion form (1.0 when fn = fp = 0),
 *   scores[2 s + 1] = normalized mutual information, average_method="arithmetic", natural log (1.0 when both labellings
 *   have one class, 0.0 when only one has, MI clamped at 0).  Contingency table in LDS by integer atomics.             */
int mcl_pca_gram(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t G, int32_t max_rows,
                 const int64_t* gram_offsets, double* mean, double* gram, mcl_stream_t stream);
int mcl_pca_project(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t G,
                    int32_t max_rows, int32_t n_comps, const double* mean, const double* evec, const int64_t* evec_offsets,
                    const double* eval, double* loadings, double* sign, double* z, mcl_stream_t stream);
int mcl_kmeans(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D, const int32_t* k,
               int32_t k_max, int32_t R, const int64_t* seeds, uint64_t seed, int32_t segment_base, double tol,
               int32_t max_iter, int64_t* seeds_out, int32_t* labels_all, double* centers_all, double* inertia_all,
               int32_t* n_iter_all, double* work, int32_t* labels, double* centers, double* inertia, int32_t* n_iter,
               int32_t* restart, mcl_stream_t stream);
int mcl_cluster_scores(const int32_t* labels_a, const int32_t* labels_b, const int64_t* offsets, int32_t S,
                       int32_t max_rows, double* scores, mcl_stream_t stream);

/* ---------------------------------------------------------------- count tables -> HVGs -> expression matrices (ABI 13;
 * csrc/preprocess.hip).  The reference's hvg_her2st.py / hvg_cscc.py / hvg_visium.py for S slides per call.
 * Slide set (all five arrays DEVICE-resident, the caller checks them; the library cannot before launching): slides[s] the
 *   row-major (rows[s], ncols[s]) count matrix of slide s, leading dimension ld[s] >= ncols[s] (elements), every slide of the
 *   one dtype (0 = float32, 1 = int32); row_offsets[S + 1] int64 = the running sum of rows (row_offsets[0] = 0).
 *   2 <= rows[s] <= 50000 = max_rows' bound, S <= 65535, 2 <= G <= 1048576 (MCL_EUNSUPPORTED beyond).
 * mcl_hvg_stats: colmaps NULL (gene g is column g of every slide, ncols[s] >= G) or (S, G) int32, colmaps[s * G + g] = the
 *   column of shared gene g in slide s (an entry outside [0, ncols[s]) is read as the nearest valid column and reported).
 *   Per slide, what scanpy computes for normalize_total(target_sum=None), log1p, highly_variable_genes(flavor="seurat",
 *   n_bins=20, n_top_genes), all fp64, the fp32 log1p / expm1 round trip left out:
 *     target_sum[s]                 the median of the positive library sizes s_i = sum_g c_ig (NaN if there is none);
 *     x_ig = c_ig / f_i             f_i = s_i / target_sum, 1 where that is 0;
 *     means[s * G + g]              log1p(mean), mean = sum_i x_ig / n with an exact 0 replaced by 1e-12;
 *     dispersions[s * G + g]        log(var / mean), var = (E[x^2] - mean^2) n / (n - 1), a ratio of exactly 0 -> NaN;
 *     mean_bin[s * G + g]           0 .. 19: pandas.cut(means, 20) (numpy.linspace edges, the lowest lowered by 0.1 % of the
 *                                   range, intervals closed on the right);
 *     dispersions_norm[s * G + g]   (dispersions - bin mean) / bin std (ddof = 1) over the bin's non-NaN dispersions; a bin
 *                                   with fewer than two of them takes std = its mean and mean = 0; IEEE results for std = 0;
 *     cutoff[s]                     the min(n_top_genes, number of non-NaN)-th largest non-NaN dispersions_norm;
 *     highly_variable[s * G + g]    1 where nan_to_num(dispersions_norm) >= cutoff, else 0 (ties all pass; NaN genes pass
 *                                   when cutoff <= 0, as in scanpy);
 *     status[s]                     0, or bits: 1 the means are all equal or not finite (outputs: NaN / 0; pandas' widening
 *                                   of a flat range is not reproduced), 2 no positive library size, 4 no non-NaN
 *                                   dispersions_norm, 8 a column map entry out of range.
 *   work: row_offsets[S] doubles (the size factors).  Four launches, no floating-point atomics, every summation order a
 *   function of (rows[s], G) alone: a slide inside a batch is bit-identical to the slide alone, run to run.
 * mcl_hvg_pool: highly_variable (S, G) -> union_out / intersection_out (G) bytes, then union_out[extra[j]] = 1 for the
 *   n_extra int32 gene indices (hvg_her2st.py:64; indices outside [0, G) are ignored).
 * mcl_expression_matrices: sel (S, K) int32 = the columns of slide s to keep, in output order.  For slide s writes at
 *   out + K * row_offsets[s] the (K, rows[s]) row-major fp32 matrix log10(c / rowsum * rescale + 1), rowsum over the K kept
 *   columns only -- scprep.transform.log(scprep.normalize.library_size_normalize(.)) of the subset, transposed into the
 *   layout of preprocessed_matrix.npy; an all-zero spot stays zero as in mcl_log_library_size_normalize.  K <= 1048576. */
int mcl_hvg_stats(const void* const* slides, const int64_t* ld, const int32_t* rows, const int32_t* ncols,
                  const int64_t* row_offsets, int32_t dtype, const int32_t* colmaps, int32_t S, int32_t G,
                  int32_t max_rows, int32_t n_top_genes, double* work, double* means, double* dispersions,
                  double* dispersions_norm, int32_t* mean_bin, uint8_t* highly_variable, double* cutoff,
                  double* target_sum, int32_t* status, mcl_stream_t stream);
int mcl_hvg_pool(const uint8_t* highly_variable, int32_t S, int32_t G, const int32_t* extra, int32_t n_extra,
                 uint8_t* union_out, uint8_t* intersection_out, mcl_stream_t stream);
int mcl_expression_matrices(const void* const* slides, const int64_t* ld, const int32_t* rows, const int32_t* ncols,
                            const int64_t* row_offsets, int32_t dtype, const int32_t* sel, int32_t S, int32_t K,
                            int32_t max_rows, float rescale, float* out, mcl_stream_t stream);

/* ---------------------------------------------------------------- Harmony batch correction (ABI 13, entry points added;
 * csrc/harmony.hip).  BLEEP's preprocess.ipynb, last cell: harmonypy.run_harmony on the slides' concatenated hvg_matrix.npy.
 * The arithmetic is stated in DESIGN 6.9.  Common contract: cells are rows; Z, Zc, Z_corr (N, d), R, S, D (N, K),
 * Y (K, d), E, O (K, B) are dense row-major fp64 device matrices; batch[n] in [0, B) and order[] (a permutation of
 * 0 .. N - 1) are device int32 the caller has checked (an entry out of range is read as the nearest valid one); theta,
 * lamb, Pr are B device doubles.  K <= 128, B <= 31, N * K < 2^31 (and d <= 2^22 in mcl_harmony_ridge and
 * mcl_harmony_apply): MCL_EUNSUPPORTED beyond.  No floating-point atomics,
 * no kernel waits on another workgroup, every summation order is a function of the shapes alone: bit-identical run to run.
 *
 * mcl_harmony_workspace_doubles: the doubles `work` must hold for (N, K, d, B) in every entry point below that takes it.
 * mcl_harmony_normalize: z (N, d), leading dimension ld, dtype 0 = float32 / 1 = float64.  zc = the rows of z divided by
 *   their own maximum (divide_by_max != 0; a zero maximum gives NaN, a negative one flips the sign, as harmonypy does) and
 *   then by their L2 norm; a NaN anywhere in a row makes its maximum NaN (numpy's max), so the whole row becomes NaN.
 *   z64 (may be NULL) = z converted to fp64.  zc may be z itself when z is dense fp64.
 * mcl_harmony_centroids: out = A X reduced over the N cells on v_mfma_f64_16x16x4_f64, N cut into slices fixed by the
 *   shapes and merged in slice order.  B == 0: out (K, d) = R^T X, normalize != 0 then L2-normalises its rows (step 2a).
 *   B > 0: out (K, B + 1, d): row (k, 0) = sum_n R[n][k] X[n], row (k, b + 1) the same over the cells of batch b (the
 *   correction's M_k), the operand formed on load.
 * mcl_harmony_dist: D = 2 (1 - Zc Y^T) (raw != 0: the product itself), reduced over d in index order on the same MFMA.
 * mcl_harmony_softmax: out[n][k] = exp(-D[n][k] / sigma - max_k(-D[n][k] / sigma)); normalize != 0: divided by its row sum.
 * mcl_harmony_moments: E[k][b] = (sum_n R[n][k]) Pr[b], O[k][b] = sum_{n in b} R[n][k].
 * mcl_harmony_update_block: step 2d for the blocks [block_lo, block_hi) of numpy.array_split(order, n_blocks), in order:
 *   the block's sums of R leave E and O, R[n][k] = S[n][k] ((E[k][b] + 1) / (O[k][b] + 1))^theta[b] divided by the row's L1
 *   norm, the new sums enter E and O.  Three launches per block; block sums by a fixed tree.
 * mcl_harmony_objective: out3 = { sum R D, sigma sum R log R (a non-finite term counts 0),
 *   sigma sum R[n][k] theta[b(n)] log((O[k][b(n)] + 1) / (E[k][b(n)] + 1)) }.
 * mcl_harmony_ridge: M (K, B + 1, d) from mcl_harmony_centroids.  A_k = arrow(O[k]) + diag(0, lamb) is inverted by
 *   Gauss-Jordan with partial pivoting; W (K, B + 1, d) = A_k^-1 M_k with row (k, 0) set to 0.
 * mcl_harmony_apply: out[n] = Z[n] - sum_k R[n][k] W[k][batch[n] + 1]; out must not be Z.
 * mcl_harmony_lloyd: the hard k-means that seeds Y when no centroids are given: Y = the rows seed_rows[K] of Zc, then iters
 *   times: label = argmax_k Zc Y^T (ties: the lowest centre), Y[k] = the mean of its cells (an emptied centre keeps its
 *   row); finally the rows of Y are L2-normalised.  labels (N) int32, products (N, K), sums (K, d): scratch / results.   */
int64_t mcl_harmony_workspace_doubles(int32_t N, int32_t K, int32_t d, int32_t B);
int mcl_harmony_normalize(const void* z, int64_t ld, int32_t dtype, int32_t N, int32_t d, int32_t divide_by_max,
                          double* z64, double* zc, mcl_stream_t stream);
int mcl_harmony_centroids(const double* R, const double* X, const int32_t* batch, int32_t N, int32_t K, int32_t d,
                          int32_t B, int32_t normalize, double* work, double* out, mcl_stream_t stream);
int mcl_harmony_dist(const double* Zc, const double* Y, int32_t N, int32_t K, int32_t d, int32_t raw, double* D,
                     mcl_stream_t stream);
int mcl_harmony_softmax(const double* D, int32_t N, int32_t K, double sigma, int32_t normalize, double* out,
                        mcl_stream_t stream);
int mcl_harmony_moments(const double* R, const int32_t* batch, int32_t N, int32_t K, int32_t B, const double* Pr, double* E,
                        double* O, mcl_stream_t stream);
int mcl_harmony_update_block(double* R, const double* S, const int32_t* batch, const int32_t* order, int32_t N, int32_t K,
                             int32_t B, int32_t n_blocks, int32_t block_lo, int32_t block_hi, const double* theta,
                             const double* Pr, double* E, double* O, mcl_stream_t stream);
int mcl_harmony_objective(const double* R, const double* D, const int32_t* batch, const double* E, const double* O,
                          const double* theta, int32_t N, int32_t K, int32_t B, double sigma, double* work, double* out3,
                          mcl_stream_t stream);
int mcl_harmony_ridge(const double* O, const double* M, const double* lamb, int32_t K, int32_t B, int32_t d, double* W,
                      mcl_stream_t stream);
int mcl_harmony_apply(const double* Z, const double* R, const double* W, const int32_t* batch, int32_t N, int32_t K,
                      int32_t B, int32_t d, double* out, mcl_stream_t stream);
int mcl_harmony_lloyd(const double* Zc, int32_t N, int32_t K, int32_t d, const int32_t* seed_rows, int32_t iters,
                      int32_t* labels, double* products, double* sums, double* work, double* Y, mcl_stream_t stream);

/* ---------------------------------------------------------------- exact t-SNE in two dimensions (ABI 13, entry points added;
 * csrc/tsne.hip).  sklearn.manifold.TSNE(method="exact"), degrees of freedom 1, for every segment (slide) of a row-stacked
 * matrix; the arithmetic is stated in DESIGN 6.10.  Common contract: offsets (S + 1) and pair_offsets (S + 1, the running
 * sum of n_s^2) are device int64 the caller has checked; rows = offsets[S], min_n / max_n the smallest / largest n_s and
 * pairs = pair_offsets[S] are the caller's statement of them, by which the launches are sized (a segment that does not fit
 * them is skipped).  P holds one dense (n_s, n_s) fp64 matrix per segment at pair_offsets[s]; Y, grad, update, gains are
 * dense (rows, 2) fp64, 16-byte aligned.  seg_params (S, 5) device doubles: exaggeration, momentum, learning rate, active
 * (0: the segment is skipped by mcl_tsne_gradient and mcl_tsne_update), reset (!= 0: update and gains are read as 0 and 1).
 * 2 <= n_s <= 16384, pairs <= 2^31, S <= 65535, D <= 64: MCL_EUNSUPPORTED beyond.  fp64 throughout, no floating-point
 * atomics, no kernel waits on another workgroup, every summation order is a function of n_s alone: a segment inside a
 * batch is bit-identical to the same segment alone.
 *
 * mcl_tsne_workspace_doubles: the doubles `work` must hold for (rows, S) in the entry points below.
 * mcl_tsne_affinities: x (rows, D), leading dimension ld, dtype 0 = float32 / 1 = float64.  d_ij = sum_k (x_ik - x_jk)^2
 *   in index order without contraction (float32_distances != 0: rounded to float32 and back, sklearn's arithmetic), the
 *   per-row precision search of sklearn's _binary_search_perplexity (perplexity < min_n), P = max((C + C^T) / sum, eps)
 *   with a zero diagonal.  beta (rows): the precision each row's conditional distribution was made with.
 * mcl_tsne_gradient: grad_i = 4 (sum_j p'_ij w_ij (y_i - y_j) - (sum_j w_ij^2 (y_i - y_j)) / sum Q), p' = exaggeration p,
 *   w_ij = 1 / (1 + |y_i - y_j|^2), sum Q over i != j.  want_kl != 0: kl[s] = sum p' log(max(p', eps) sum Q / w).
 * mcl_tsne_update: gain += 0.2 where update * grad < 0, else *= 0.8, floored at 0.01; update = momentum update -
 *   learning rate gain grad; Y += update; grad_norm2[s] = the squared norm of gain * grad.                              */
int64_t mcl_tsne_workspace_doubles(int32_t rows, int32_t S);
int mcl_tsne_affinities(const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets,
                        const int64_t* pair_offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n, int64_t pairs,
                        double perplexity, int32_t float32_distances, double* work, double* P, double* beta,
                        mcl_stream_t stream);
int mcl_tsne_gradient(const double* P, const int64_t* pair_offsets, const double* Y, const int64_t* offsets, int32_t S,
                      int32_t rows, int32_t min_n, int32_t max_n, int64_t pairs, const double* seg_params, int32_t want_kl,
                      double* work, double* grad, double* kl, mcl_stream_t stream);
int mcl_tsne_update(const double* grad, const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n,
                    const double* seg_params, double* Y, double* update, double* gains, double* grad_norm2,
                    mcl_stream_t stream);

/* ---------------------------------------------------------------- the spot neighbourhood graph (ABI 13, entry points added;
 * csrc/neighbors.hip).  scanpy's sc.pp.neighbors with umap-learn's weights, exact at every size, for every segment (slide)
 * of a row-stacked matrix; the arithmetic is stated in DESIGN 6.11.  Common contract: offsets (S + 1) is device int64 the
 * caller has checked; rows = offsets[S], min_n / max_n the smallest / largest n_s are the caller's statement of them, by
 * which the launches are sized (a segment that does not fit them is skipped).  k = n_neighbors counts the row itself.
 * 2 <= k <= 256, k <= n_s, 2 <= n_s <= 16384, S <= 65535, D <= 64: MCL_EUNSUPPORTED beyond the upper limits, MCL_EINVAL
 * below the lower ones.  fp64 throughout, no floating-point atomics, no result depends on the order workgroups arrive in:
 * a segment inside a batch is bit-identical to the same segment alone.
 *
 * mcl_knn_workspace_bytes: the bytes `work` must hold for (rows, k) in mcl_knn_smooth and mcl_knn_connectivities (8-byte
 *   aligned; the two phases of mcl_knn_connectivities share its contents).
 * mcl_knn_exact: x (rows, D), leading dimension ld, dtype 0 = float32 / 1 = float64.  d2_ij = sum_c (x_ic - x_jc)^2 in index
 *   order without contraction.  knn_indices (rows, k) int32, segment-local: position 0 is the row itself at distance 0,
 *   positions 1 .. k-1 the other rows in ascending (d2, j); knn_distances (rows, k) = sqrt(d2).
 * mcl_knn_smooth: umap-learn's smooth_knn_dist(n_iter 64, local_connectivity 1, bandwidth 1) per row: rho (rows) the
 *   smallest positive distance or 0, sigma (rows) the bisection's last mid after the floors 1e-3 x the row's / the
 *   segment's mean distance.
 * mcl_knn_connectivities: the directed weights (0 for the row itself, 1 where d - rho <= 0 or sigma == 0, else
 *   exp(-(d - rho) / sigma)), united as w = mix (a + b - a b) + (1 - mix) a b, as one CSR per segment without the diagonal
 *   and without zeros, columns ascending.  phase 0: fills work, writes indptr (rows + S int64: segment s holds n_s + 1
 *   entries from offsets[s] + s, starting at 0) and nnz (S int64; -1 for a skipped segment).  phase 1, after phase 0 on
 *   the same arguments and work: nnz_offsets (S + 1 device int64, the running sum of nnz) places segment s in indices
 *   (int32) and data (fp64), each of nnz_total entries; nothing is written beyond them.                                  */
int64_t mcl_knn_workspace_bytes(int32_t rows, int32_t k);
int mcl_knn_exact(const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets, int32_t S, int32_t rows,
                  int32_t min_n, int32_t max_n, int32_t k, int32_t* knn_indices, double* knn_distances,
                  mcl_stream_t stream);
int mcl_knn_smooth(const double* knn_distances, const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n,
                   int32_t max_n, int32_t k, void* work, double* rho, double* sigma, mcl_stream_t stream);
int mcl_knn_connectivities(const int32_t* knn_indices, const double* knn_distances, const double* rho, const double* sigma,
                           const int64_t* offsets, int32_t S, int32_t rows, int32_t min_n, int32_t max_n, int32_t k,
                           double set_op_mix_ratio, int32_t phase, void* work, int64_t* indptr, int64_t* nnz,
                           const int64_t* nnz_offsets, int64_t nnz_total, int32_t* indices, double* data,
                           mcl_stream_t stream);

/* ---------------------------------------------------------------- the UMAP layout of that graph (ABI 13, entry points added;
 * csrc/umap.hip).  scanpy's sc.tl.umap on the connectivities CSR of mcl_knn_connectivities for every segment (slide); the
 * arithmetic is stated in DESIGN 6.12: one Jacobi step per epoch (every gradient of epoch n at the positions at its start),
 * negative samples a pure function of (seed, epoch, vertex, entry rank, sample number).  Common contract: offsets (S + 1),
 * nnz_offsets (S + 1) device int64 and n_epochs (S) device int32 the caller has checked; rows, min_n, max_n, nnz_total =
 * nnz_offsets[S], max_nnz (the most entries of one segment) and max_epochs (the largest n_epochs) are the caller's statement
 * of them, by which the launches are sized (a segment that does not fit them is skipped; a column outside its segment is
 * ignored; a weight that is not positive and finite is never sampled).  indptr / indices / data as mcl_knn_connectivities
 * leaves them: exactly symmetric, no diagonal, columns ascending.  Positions are dense (rows, 2) fp64, 16-byte aligned.
 * 2 <= n_s <= 16384, S <= 65535, 1 <= n_epochs <= 5000, 0 <= negative_sample_rate <= 64, a, b, gamma, alpha finite and
 * a, b > 0: MCL_EUNSUPPORTED otherwise.  fp64 throughout, no floating-point atomics (integer atomics count the samples), no
 * workgroup waits on another: a segment inside a batch is bit-identical to the same segment alone.
 *
 * mcl_umap_workspace_bytes: the bytes `work` must hold (8-byte aligned); it carries the schedule from mcl_umap_prepare
 *   through every mcl_umap_epochs call of one layout.
 * mcl_umap_prepare: per segment wmax = its largest weight; per stored entry live = w >= wmax / n_epochs, eps = wmax / w,
 *   epn = eps / negative_sample_rate, next = eps, nneg = epn, each a single IEEE operation.  Zeroes counters (S, 2).
 * mcl_umap_init: mode 0: Y = the first two columns of x (rows, D >= 2; leading dimension ld, dtype 0 = float32 / 1 =
 *   float64) times 10 / (the segment's largest absolute value in them); mode 1: y_ic = 20 ((h >> 11) 2^-53) - 10 with
 *   h = mix(mix(mix(seed ^ ~0) ^ i) ^ c), mix the splitmix64 step (x is not read).
 * mcl_umap_epochs: epochs first .. first + count - 1, one launch each, enqueued back to back.  Epoch n reads Y0 when n is
 *   even and Y1 when it is odd and writes the other; a segment with n >= n_epochs[s] copies its positions across, so after
 *   epoch n every segment's current positions are in the buffer of parity n + 1.  The same work, counters and arguments as
 *   in mcl_umap_prepare; every epoch exactly once, in order.  counters[s] = (attractions taken, negative samples drawn). */
int64_t mcl_umap_workspace_bytes(int64_t nnz_total, int32_t S);
int mcl_umap_prepare(const double* data, const int64_t* nnz_offsets, const int32_t* n_epochs, int32_t S, int64_t nnz_total,
                     int64_t max_nnz, int32_t max_epochs, int32_t negative_sample_rate, void* work, int64_t* counters,
                     mcl_stream_t stream);
int mcl_umap_init(int32_t mode, const void* x, int64_t ld, int32_t dtype, int32_t D, const int64_t* offsets, int32_t S,
                  int32_t rows, int32_t min_n, int32_t max_n, uint64_t seed, double* Y, mcl_stream_t stream);
int mcl_umap_epochs(int32_t first, int32_t count, const int64_t* indptr, const int32_t* indices, const int64_t* offsets,
                    const int64_t* nnz_offsets, const int32_t* n_epochs, int32_t S, int32_t rows, int32_t min_n,
                    int32_t max_n, int64_t nnz_total, int32_t max_epochs, double a, double b, double gamma, double alpha,
                    int32_t negative_sample_rate, uint64_t seed, void* work, double* Y0, double* Y1, int64_t* counters,
                    mcl_stream_t stream);

/* ---------------------------------------------------------------- deterministic Leiden on that graph (ABI 13, entry points
 * added; csrc/leiden.hip).  scanpy's sc.tl.leiden (RBConfigurationVertexPartition on the connectivities) for every segment
 * (slide); the algorithm is the one DESIGN 6.13 states: Jacobi sweeps of local moving and Jacobi rounds of refinement, each
 * accepted only if Q rose strictly, aggregation, levels.  Weights are fixed point (q = rint(w 2^e) per segment), so every
 * sum of weights is an exact int64 and integer atomics change no bit; fp64 only in gains, tests and Q, no floating-point
 * atomics; a segment inside a batch is bit-identical to the same segment alone.  Common contract: indptr / indices / data /
 * offsets / nnz_offsets as mcl_umap_epochs takes them; rows, max_n, nnz_total the caller's statement of them; 2 <= n_s <=
 * 16384, S <= 65535 (MCL_EUNSUPPORTED otherwise); resolution finite and > 0.  `work` holds mcl_leiden_workspace_bytes bytes,
 * 8-byte aligned, and carries one clustering from mcl_leiden_init to mcl_leiden_finish; it begins with S state records of
 * 128 bytes (two doubles Q, Q of the refinement; two int64 2m, scratch; 24 int32: n, shift, label buffer, refined buffer,
 * parity, fails, move phase done, refinement done, finished, sweeps accepted at the level, sweeps, accepted sweeps, rounds,
 * levels, steps of the phase, error, next n, longest row, n at level 0), which the host reads between batches of launches.
 *
 * mcl_leiden_init: level 0 of one iteration: q, k_i, 2m, labels = partition (device int32 ids below n_s; NULL: every vertex
 *   alone), Q of that partition.  A segment with active[s] == 0 (active may be NULL) or with 2m = 0 is finished at once.
 * mcl_leiden_move_sweeps: `count` sweeps at `level` (n_cur: the most nodes of a segment there; long_rows: some row exceeds
 *   512 entries, so the dense path is launched too).  A phase ends after two consecutive sweeps that did not raise Q;
 *   max_sweeps sweeps without that end set the record's error.
 * mcl_leiden_refine_rounds: begin != 0 starts the refinement of the current partition (every node alone), then `count` rounds.
 * mcl_leiden_aggregate: refined communities become the nodes of level + 1, which starts from the partition of local moving;
 *   a segment whose level accepted no sweep and merged nothing is finished; level + 1 == max_levels unfinished is an error.
 * mcl_leiden_finish: final_labels == 0: canonical[v] = the smallest vertex of v's community (source 0) or of its refined
 *   community at level 0 (source 1), for the segments with active[s] != 0; final_labels != 0: labels = canonical ids
 *   renumbered by descending size, ties to the smaller id, and n_clusters (S). */
int64_t mcl_leiden_workspace_bytes(int64_t rows, int64_t nnz_total, int32_t S, int32_t max_n);
int mcl_leiden_init(const int64_t* indptr, const int32_t* indices, const double* data, const int64_t* offsets,
                    const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total, double resolution,
                    const int32_t* partition, const int32_t* active, void* work, mcl_stream_t stream);
int mcl_leiden_move_sweeps(int32_t count, int32_t level, int32_t n_cur, int32_t long_rows, int32_t max_sweeps,
                           const int64_t* indptr, const int32_t* indices, const int64_t* offsets, const int64_t* nnz_offsets,
                           int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total, double resolution, void* work,
                           mcl_stream_t stream);
int mcl_leiden_refine_rounds(int32_t begin, int32_t count, int32_t level, int32_t n_cur, int32_t long_rows,
                             int32_t max_rounds, const int64_t* indptr, const int32_t* indices, const int64_t* offsets,
                             const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n, int64_t nnz_total,
                             double resolution, void* work, mcl_stream_t stream);
int mcl_leiden_aggregate(int32_t level, int32_t n_cur, int32_t max_levels, const int64_t* indptr, const int32_t* indices,
                         const int64_t* offsets, const int64_t* nnz_offsets, int32_t S, int32_t rows, int32_t max_n,
                         int64_t nnz_total, double resolution, void* work, mcl_stream_t stream);
int mcl_leiden_finish(int32_t source, int32_t final_labels, const int32_t* active, const int64_t* indptr,
                      const int32_t* indices, const int64_t* offsets, const int64_t* nnz_offsets, int32_t S, int32_t rows,
                      int32_t max_n, int64_t nnz_total, void* work, int32_t* canonical, int32_t* labels, int32_t* n_clusters,
                      mcl_stream_t stream);

/* ---------------------------------------------------------------- leading eigenpairs of symmetric matrices (ABI 13, entry
 * points added; csrc/eig.hip).  The k <= 64 largest eigenvalues and their eigenvectors of S dense symmetric fp64 matrices
 * per call, by the direct method DESIGN 6.14 states: Householder tridiagonalisation, bisection on the Sturm count, block
 * inverse iteration, back-transformation.  fp64 throughout, no floating-point atomics, no workgroup waits for another;
 * every sum's order depends only on the slide's own m and k: a slide inside a batch is bit-identical to the same slide
 * alone.  a: slide s is row-major m_s x m_s at a[a_offsets[s]] (device int64 element offsets, the layout mcl_pca_gram
 * writes), exactly symmetric, both triangles; it is OVERWRITTEN (reflectors and the reduced blocks).  m[S] device int32;
 * max_m and sum_m: the caller's statement of the largest and the sum of them.  1 <= m_s <= max_m <= 4096, 1 <= k <= 64,
 * S <= 65535 (MCL_EUNSUPPORTED beyond), k <= max_m and S <= sum_m <= S max_m (MCL_EINVAL otherwise); k <= every m_s and
 * the stated sum are checked on the device: a call that breaks them computes nothing and certifies NaN for every slide.
 * evals[s * k + i]: descending.  evecs: row-major (m_s, k) at evecs[evec_offsets[s]] (device int64), the layout
 * mcl_pca_project reads; each vector is scaled by +-1 so that its component of largest magnitude (ties: the lowest index)
 * is positive.  cert[2 s] = max_i |T z_i - lambda_i z_i|_2 / |T|, cert[2 s + 1] = max |Z^T Z - I| of the tridiagonal
 * problem, computed on the device.  work: mcl_sym_eig_workspace_bytes bytes, 8-byte aligned; it carries the call from one
 * stage to the next.  stages: bit 0 the tridiagonalisation, bit 1 eigenvalues, vectors of T and the certificate, bit 2 the
 * back-transformation and the sign; 7 runs all, and a caller that times the stages passes 1, 2, 4 in that order with the
 * same arguments.  Enqueues about 3 max_m launches and never synchronises. */
int64_t mcl_sym_eig_workspace_bytes(int32_t S, int32_t max_m, int64_t sum_m, int32_t k);
int mcl_sym_eig_top(double* a, const int64_t* a_offsets, const int32_t* m, int32_t S, int32_t max_m, int64_t sum_m,
                    int32_t k, int32_t stages, double* evals, double* evecs, const int64_t* evec_offsets, double* cert,
                    void* work, mcl_stream_t stream);

/* ---------------------------------------------------------------- marker genes of spot groups (ABI 13, entry points added;
 * csrc/markers.hip).  scanpy's sc.tl.rank_genes_groups(adata, groupby, reference="rest") for every slide of an evaluation
 * per call: Wilcoxon rank-sum and Welch t (DESIGN 6.15 states the arithmetic).  Common contract: x row-stacked (rows, G),
 * dtype 0 = fp32 / 1 = fp64, row stride ld >= G; offsets: S + 1 device int64 slide boundaries; labels: rows device int32,
 * within slide s in [0, k[s]) or -1 (the row is dropped from everything); k: S device int32.  max_n, kmax, groups_total:
 * the caller's statement of the largest slide, the largest k and sum k.  2 <= n_s <= max_n <= 16384, 1 <= k[s] <= kmax <=
 * 255, G <= 16384, S <= 65535, S <= groups_total <= S kmax: anything else is MCL_EINVAL before a launch; the device checks
 * offsets, k and labels against the statements, and a slide that breaks them is skipped and counted in status.  Group g of
 * slide s is group row sum_{s' < s} k[s'] + g of every (groups_total, G) output.  work: mcl_marker_workspace_bytes bytes,
 * 8-byte aligned; mcl_marker_stats fills it and the three other calls read it, so they follow it on the same stream with
 * the same S, rows, G, kmax, groups_total.  fp64 and exact int64, no floating-point atomics, deterministic; a slide inside
 * a batch is bit-identical to the same slide alone.
 *
 * mcl_marker_stats: group_sizes (groups_total), n_valid (S): rows with a label >= 0; per (group row, gene): mean and
 *   variance (ddof 1, NaN below two rows) of the group and of the rest, the fraction and the count of x != 0 of both;
 *   status[2 s] = non-finite values among the kept rows of slide s, status[2 s + 1] = labels outside [-1, k[s]) plus one if
 *   the slide's offsets or k break the statements.
 * mcl_marker_rank_sums: rank_sums2 (groups_total, G) = sum over the group's rows of twice the tie-averaged rank among the
 *   slide's kept rows (-0.0 ties with +0.0); tie_terms (S, G) = sum over tie runs of t^3 - t.  Exact int64.
 * mcl_marker_test: method 0 Wilcoxon (tie_correct != 0: the variance is scaled by 1 - T / (N^3 - N)), 1 Welch t, 2 Welch t
 *   with the rest's variance over the group's size; scores, pvals, neglog10_pvals (log space: finite where pvals is 0),
 *   logfoldchanges = log2((expm1(mean) + 1e-9) / (expm1(mean_rest) + 1e-9)).  rank_sums2 / tie_terms may be NULL for 1, 2.
 * mcl_marker_rank_adjust: pvals_adj (groups_total, G) = Benjamini-Hochberg over the G genes of a group row, in gene order;
 *   names (groups_total, n_genes) = the genes by descending score (rankby_abs != 0: |score|), equal scores by gene index,
 *   and the five columns gathered in that order. */
int64_t mcl_marker_workspace_bytes(int64_t rows, int64_t groups_total, int32_t S, int32_t G);
int mcl_marker_stats(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, const int32_t* labels,
                     const int32_t* k, int32_t S, int64_t rows, int32_t G, int32_t max_n, int32_t kmax,
                     int64_t groups_total, void* work, int32_t* group_sizes, int32_t* n_valid, double* mean_g,
                     double* var_g, double* mean_r, double* var_r, double* pts_g, double* pts_r, int32_t* nnz_g,
                     int32_t* nnz_r, int32_t* status, mcl_stream_t stream);
int mcl_marker_rank_sums(const void* x, int64_t ld, int32_t dtype, const int32_t* labels, int32_t S, int64_t rows,
                         int32_t G, int32_t max_n, int32_t kmax, int64_t groups_total, void* work, int64_t* rank_sums2,
                         int64_t* tie_terms, mcl_stream_t stream);
int mcl_marker_test(int32_t method, int32_t tie_correct, int32_t S, int64_t rows, int32_t G, int32_t kmax,
                    int64_t groups_total, const void* work, const int32_t* group_sizes, const double* mean_g,
                    const double* var_g, const double* mean_r, const double* var_r, const int64_t* rank_sums2,
                    const int64_t* tie_terms, double* scores, double* pvals, double* neglog10_pvals,
                    double* logfoldchanges, mcl_stream_t stream);
int mcl_marker_rank_adjust(int32_t S, int64_t rows, int32_t G, int32_t kmax, int64_t groups_total, int32_t n_genes,
                           int32_t rankby_abs, void* work, const double* scores, const double* pvals,
                           const double* neglog10_pvals, const double* logfoldchanges, double* pvals_adj, int64_t* names,
                           double* top_scores, double* top_pvals, double* top_pvals_adj, double* top_neglog10_pvals,
                           double* top_logfoldchanges, mcl_stream_t stream);

/* ---------------------------------------------------------------- spatial autocorrelation (csrc/spatial.hip)
 * Moran's I and Geary's C of every gene on the spot lattice graph of every slide, the analytic moments under normality and
 * a permutation test.  Slide s owns rows offsets[s] .. offsets[s + 1] (device int64, S + 1 entries) of every row-stacked
 * array; S, rows and max_n are the caller's statement of them: 2 <= n_s <= max_n <= 16384, 1 <= k <= 64, G <= 16384,
 * n_perms <= 65535, S <= 65535 (mcl_spatial_moments: 32767): anything else is MCL_EINVAL before a launch; a slide whose
 * offsets break the statements is skipped and counted in status.  The graph is a fixed-width list: nbr (rows, k) int32
 * segment-local, w (rows, k) fp64 (0 = a pruned slot), deg (rows,) = kept slots; consts (S, 3) = S0, S1, S2.  fp64, every
 * sum over the rows of a slide in one fixed order that depends on n alone, no floating-point atomics, deterministic; a slide
 * inside a batch is bit-identical to the same slide alone.
 *
 * mcl_spatial_workspace_bytes: hist_slots = k + 1 and n_perms = 0 for mcl_spatial_lattice; hist_slots = 0 for the
 *   permutation table, which is uint16 (n_perms, n_s) per slide at element offset n_perms * offsets[s].
 * mcl_spatial_columns: the gene columns a workgroup of mcl_spatial_stats takes for a slide of n rows (1 .. 6).
 * mcl_spatial_lattice: given = 0: knn_indices / knn_distances are the (rows, k + 1) lists of mcl_knn_exact over the
 *   coordinates (position 0 the row itself); needs n_s >= k + 1; prune 0 keeps all k, 1 keeps d <= mean + population std of
 *   the row's k distances, 2 keeps d <= 2; kept edges weigh 1, or 1 / deg with row_standardise.  given != 0: nbr and w are
 *   inputs and are validated; deg and consts are outputs either way.  status (S, 6): offsets broken, indices out of range,
 *   weights negative or non-finite, neighbours listed twice, rows that are not binary, rows that are not row-standardised;
 *   consts are NaN for a slide that is refused.
 * mcl_spatial_permutations: fills the table: permutation p of a slide of n rows is a function of (seed, p, n) alone.
 * mcl_spatial_stats: stat (2, S, n_perms, G): Moran's I, then Geary's C, of x (rows, G; dtype 0 fp32, 1 fp64; row stride
 *   ld) with row i taking the value of row table[p][i].  table = NULL: the identity, n_perms = 1, and mean / den (S, G) are
 *   written: the observed statistic, from the same code.  column_mask: bit c set = launch the c-column kernel (the caller
 *   sets the bits mcl_spatial_columns gives for its slides).  status (S,): non-finite values of x (accumulated).
 * mcl_spatial_moments: z, p (two_tailed != 0: both tails) and -log10 p (log space) under normality, and the
 *   Benjamini-Hochberg adjustment over the G genes of a (statistic, slide); all (2, S, G); prank / scratch: (2, S, G) scratch.
 * mcl_spatial_perm_summary: per (statistic, slide, gene) over the n_perms sims: count = #(sims >= stat) folded to the smaller
 *   tail, pval_sim = (count + 1) / (n_perms + 1), mean and population variance summed over p ascending, and the normal p of
 *   (stat - mean) / sqrt(var). */
int64_t mcl_spatial_workspace_bytes(int64_t rows, int32_t hist_slots, int32_t n_perms);
int32_t mcl_spatial_columns(int32_t n);
int mcl_spatial_lattice(const int32_t* knn_indices, const double* knn_distances, const int64_t* offsets, int32_t S,
                        int64_t rows, int32_t max_n, int32_t k, int32_t prune, int32_t row_standardise, int32_t given,
                        void* work, int32_t* nbr, double* w, int32_t* deg, double* consts, int32_t* status, mcl_stream_t stream);
int mcl_spatial_permutations(const int64_t* offsets, int32_t S, int64_t rows, int32_t max_n, int32_t n_perms,
                             uint64_t seed, void* work, mcl_stream_t stream);
int mcl_spatial_stats(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                      int32_t max_n, int32_t k, int32_t column_mask, const int32_t* nbr, const double* w,
                      const double* consts, const void* table, int32_t n_perms, double* mean, double* den, double* stat,
                      int32_t* status, mcl_stream_t stream);
int mcl_spatial_moments(const int64_t* offsets, int32_t S, int64_t rows, int32_t G, int32_t max_n, const double* consts,
                        const double* stat, int32_t two_tailed, int32_t* prank, double* scratch, double* z_norm,
                        double* pval_norm, double* neglog10_pval_norm, double* pval_norm_adj, mcl_stream_t stream);
int mcl_spatial_perm_summary(int32_t S, int32_t G, int32_t n_perms, const double* stat, const double* sims,
                             int32_t two_tailed, int32_t* count, double* pval_sim, double* pval_z_sim, double* mean_sim,
                             double* var_sim, mcl_stream_t stream);

/* ---------------------------------------------------------------- Gaussian mixtures (csrc/mixture.hip)
 * EM as sklearn's GaussianMixture states it, for S slides x R models per call.  Slide s owns rows offsets[s] ..
 * offsets[s + 1] (device int64, S + 1 entries) of z (rows, D) fp64, row stride ld, and has k[s] components (device int32),
 * 1 <= k[s] <= min(k_max, n_s), 1 <= n_s <= 50000; D <= 64 and k_max <= 64, MCL_EUNSUPPORTED beyond.  covariance_type:
 * 0 full, 1 tied, 2 diag, 3 spherical; covariances and precisions_cholesky hold, per model, (k_max, D, D), (D, D),
 * (k_max, D) or (k_max) doubles (full / tied: the upper-triangular factor P with P^T P = the precision).  fp64, no
 * floating-point atomics, every sum in one fixed order that depends on the slide's own shape alone: a slide inside a batch
 * is bit-identical to the same slide alone.  One workgroup runs one whole (model, slide) problem; none waits for another.
 *
 * mcl_gmm_workspace_bytes: the workspace of mcl_gmm_fit / mcl_gmm_select (R models) and of mcl_gmm_mstep (R = 1).
 * mcl_gmm_fit: init_labels (R, rows) int32 are one-hot responsibilities (sklearn's _initialize), then E / M steps until
 *   |change of lower_bound| < tol or max_iter, then one more E-step: labels_all (R, rows), the parameters (S, R, ...),
 *   lower_bound_all / score_all (S, R): the mean log-likelihood of the last iteration's E-step / under the final parameters.
 *   status_all (S, R): 0 ok; 1 a covariance was not positive definite (sklearn raises "ill-defined empirical covariance":
 *   lower bound NaN, labels -1, the problem ends there); 2 the slide's shape or k breaks the statements above.
 * mcl_gmm_select: per slide the model of highest lower bound (ties: lowest r; NaN never wins): its labels (rows), resp
 *   (rows, k_max) = exp(log_resp), parameters (S, ...), n_iter, converged, status, restart, and bic / aic with sklearn's
 *   parameter counts.
 * mcl_gmm_predict: the E-step of the fit under given parameters (S, ...): log_prob_norm (rows) = score_samples, log_resp and
 *   resp (rows, k_max), labels (argmax, ties to the lowest k), score (S) = the mean of log_prob_norm.
 * mcl_gmm_mstep: the M-step of the fit from given log_resp (rows, k_max): weights = n_k / sum n_k, means, covariances
 *   (+ reg_covar on the diagonal), precisions_cholesky; status (S) as above.
 * mcl_cluster_validity: z as above with D <= 64, labels (rows) int32 in [0, 1024) or -1 = the row is dropped, 2 <= n_s <=
 *   50000.  silhouette (rows): sklearn's silhouette_samples (Euclidean; 0 for a row alone in its cluster, NaN for a dropped
 *   row); scores (S, 3): the mean silhouette over the kept rows, the Calinski-Harabasz and the Davies-Bouldin score, NaN
 *   all three when the slide has fewer than 2 or more than kept - 1 non-empty clusters (or a label out of range).  work:
 *   mcl_cluster_validity_workspace_bytes.  Every (row, cluster) distance sum runs over the cluster's rows ascending. */
int64_t mcl_gmm_workspace_bytes(int64_t rows, int32_t S, int32_t R, int32_t D, int32_t k_max);
int mcl_gmm_fit(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                const int32_t* k, int32_t k_max, int32_t R, int32_t covariance_type, const int32_t* init_labels,
                double tol, int32_t max_iter, double reg_covar, void* work, int64_t work_bytes, int32_t* labels_all,
                double* weights_all, double* means_all, double* covariances_all, double* precisions_cholesky_all,
                double* lower_bound_all, double* score_all, int32_t* n_iter_all, int32_t* converged_all,
                int32_t* status_all, mcl_stream_t stream);
int mcl_gmm_select(const int64_t* offsets, int32_t S, int64_t rows, int32_t D, const int32_t* k, int32_t k_max, int32_t R,
                   int32_t covariance_type, const void* work, int64_t work_bytes, const int32_t* labels_all,
                   const double* weights_all, const double* means_all, const double* covariances_all,
                   const double* precisions_cholesky_all, const double* lower_bound_all, const double* score_all,
                   const int32_t* n_iter_all, const int32_t* converged_all, const int32_t* status_all, int32_t* labels,
                   double* resp, double* weights, double* means, double* covariances, double* precisions_cholesky,
                   double* lower_bound, int32_t* n_iter, int32_t* converged, int32_t* status, double* bic, double* aic,
                   int32_t* restart, mcl_stream_t stream);
int mcl_gmm_predict(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                    const int32_t* k, int32_t k_max, int32_t covariance_type, const double* weights, const double* means,
                    const double* precisions_cholesky, double* log_prob_norm, double* log_resp, double* resp,
                    int32_t* labels, double* score, mcl_stream_t stream);
int mcl_gmm_mstep(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D, const int32_t* k,
                  int32_t k_max, int32_t covariance_type, const double* log_resp, double reg_covar, void* work,
                  int64_t work_bytes, double* weights, double* means, double* covariances, double* precisions_cholesky,
                  int32_t* status, mcl_stream_t stream);
int64_t mcl_cluster_validity_workspace_bytes(int64_t rows, int32_t S, int32_t D);
int mcl_cluster_validity(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                         const int32_t* labels, void* work, int64_t work_bytes, double* silhouette, double* scores,
                         mcl_stream_t stream);

/* ---------------------------------------------------------------- Potts-HMRF mixtures (csrc/hmrf.hip)
 * The mixture above with a Potts prior on the labels over a fixed-width neighbour list: nbr (rows, kw) int32, indices local
 * to the slide, w (rows, kw) fp64 with 0 marking a pruned slot (what mcl_spatial_lattice writes), kw <= 64, and one coupling
 * beta[s] >= 0 per slide (device fp64).  Mean-field EM in synchronous sweeps: the field of iteration t,
 * f_ik = sum over the kept slots c ascending of w_ic q[nbr_ic][k], reads the responsibilities q of iteration t - 1; the
 * E-step normalises the mixture's weighted log prob + (beta f).  Shapes and limits as the mixture's, with n_s <= 16384.  A
 * kept slot whose index lies outside 0 .. n_s - 1 counts as pruned and sets bit 4 (value 4) of the status.
 *
 * mcl_hmrf_workspace_bytes: the workspace of mcl_hmrf_fit.  It begins with the one mcl_gmm_workspace_bytes describes, so
 *   mcl_gmm_select reads it as it is; the field (R, rows, k_max) of every start's final E-step follows at byte
 *   mcl_gmm_workspace_bytes(rows, S, R, D, k_max).
 * mcl_hmrf_fit: mcl_gmm_fit with the graph and beta.  lower_bound_all / score_all (S, R): the mean over the rows of
 *   lse_i - za_i (the mean-field pseudo-log-likelihood; za the log-sum-exp of log w_k + (beta f_ik)) of the last iteration /
 *   under the final parameters; the bic / aic mcl_gmm_select derives from score_all are pseudo-likelihood criteria.
 *   status_all: 0, 1, 2 as mcl_gmm_fit (2 also for a beta that is negative or not finite), bit 4 as above.
 * mcl_hmrf_estep: one E-step under given parameters (S, ...) and previous responsibilities resp_prev (rows, k_max): field,
 *   log_resp, resp (rows, k_max), labels (argmax, ties to the lowest k), log_prob_norm = lse and log_prior_norm = za (rows),
 *   score (S) = the mean of lse - za, status (S).
 * mcl_label_refine: one synchronous round of majority relabelling.  For a spot with label l >= 0: over its kept slots
 *   whose neighbour's label is >= 0 (m of them) and the spot itself, own = the count of l, top = the label of largest
 *   count (ties: the smallest label); the spot takes top iff 2 own < m and 2 count(top) > m.  -1 stays -1.  Every decision
 *   reads labels; labels_out (rows) must not alias it; changed (S): the spots whose label changed.
 * mcl_edge_agreement: sums (S, 2): sum_i sum_c w_ic [l_i = l_nbr] and sum_i sum_c w_ic, both over the kept slots whose two
 *   labels are >= 0; slots ascending within a row, rows summed per thread t, t + 256, ... and then in a binary tree. */
int64_t mcl_hmrf_workspace_bytes(int64_t rows, int32_t S, int32_t R, int32_t D, int32_t k_max);
int mcl_hmrf_fit(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                 const int32_t* k, int32_t k_max, int32_t R, int32_t covariance_type, const int32_t* init_labels,
                 const int32_t* nbr, const double* w, int32_t kw, const double* beta, double tol, int32_t max_iter,
                 double reg_covar, void* work, int64_t work_bytes, int32_t* labels_all, double* weights_all,
                 double* means_all, double* covariances_all, double* precisions_cholesky_all, double* lower_bound_all,
                 double* score_all, int32_t* n_iter_all, int32_t* converged_all, int32_t* status_all, mcl_stream_t stream);
int mcl_hmrf_estep(const double* z, int64_t ld, const int64_t* offsets, int32_t S, int64_t rows, int32_t D,
                   const int32_t* k, int32_t k_max, int32_t covariance_type, const double* weights, const double* means,
                   const double* precisions_cholesky, const double* resp_prev, const int32_t* nbr, const double* w,
                   int32_t kw, const double* beta, double* field, double* log_resp, double* resp, int32_t* labels,
                   double* log_prob_norm, double* log_prior_norm, double* score, int32_t* status, mcl_stream_t stream);
int mcl_label_refine(const int64_t* offsets, int32_t S, int64_t rows, const int32_t* labels, const int32_t* nbr,
                     const double* w, int32_t kw, int32_t* labels_out, int32_t* changed, mcl_stream_t stream);
int mcl_edge_agreement(const int64_t* offsets, int32_t S, int64_t rows, const int32_t* labels, const int32_t* nbr,
                       const double* w, int32_t kw, double* sums, mcl_stream_t stream);

/* ---------------------------------------------------------------- ligand-receptor permutation test (csrc/ligrec.hip)
 * squidpy.gr.ligrec / CellPhoneDB: group means of the ligand and receptor genes under permutations of the group labels.
 * Slide s owns rows offsets[s] .. offsets[s + 1] (device int64, S + 1 entries) of x (rows, G; dtype 0 fp32, 1 fp64; row
 * stride ld) and labels (rows,) int32 in -1 .. k[s] - 1 (-1: the spot is dropped; k device int32 per slide, <= kmax).
 * 2 <= n_s <= max_n <= 16384 (the limit of mcl_spatial_permutations, whose tables it reads), kmax <= 255, G <= 16384,
 * n_perms <= 65535, S <= 32767, I <= 65535, I kmax^2 <= 2^24 and S I kmax^2 < 2^31: MCL_EUNSUPPORTED beyond, MCL_EINVAL for a
 * malformed call.  The KEPT spots n of a slide (label >= 0) may number 0 or 1: mcl_spatial_permutations then skips the slide
 * (it gets no table), and a slide of one kept spot takes the identity as its only permutation, a slide of none has NaN
 * means and no defined entry.  fp64, every group sum in one fixed order
 * that depends on the group's size alone, no floating-point atomics; a slide inside a batch is bit-identical to the same slide
 * alone.  status (S, 4): offsets or k broken, labels outside -1 .. k - 1 (dropped), non-finite x, negative x (the last two
 * counted over the kept spots of the used columns).
 *
 * mcl_ligrec_columns: the used gene columns (1, 2, 4 or 8) a workgroup of mcl_ligrec_group_means takes for n kept spots.
 * mcl_ligrec_chunk: the permutations per chunk: as many as keep perm_means within 256 MiB, at most n_perms.
 * mcl_ligrec_workspace_bytes: the bytes of perm_means, (S, chunk, U, kmax) fp64.
 * mcl_ligrec_prepare: order (rows,): the kept spots of slide s (segment-local) in the stable order by (label, spot) at
 *   offsets[s] .. + n, -1 behind them; start (S, kmax + 1): group c owns positions start[c] .. start[c + 1] of that order
 *   (start[c] = n for c >= k[s]); kept_offsets (S + 1,): the running sum of n: the offsets to hand to
 *   mcl_spatial_permutations, whose table then holds (n_perms, n) uint16 per slide at element n_perms * kept_offsets[s].
 * mcl_ligrec_group_means: used (U,) int32: the ascending distinct gene columns of the interactions.  column_mask: bit c set
 *   = launch the c-column kernel (the bits mcl_ligrec_columns gives for the slides' n).  table = NULL: the identity, once:
 *   writes sum, nnz (count of values > 0), mean = sum / size and frac = nnz / size, all (S, kmax, U) (an empty group: NaN
 *   mean and frac).  Otherwise permutations p0 .. p0 + pc - 1 (pc <= chunk) of the table: group c receives the spots
 *   order[table[p][j]], start[c] <= j < start[c + 1]; perm_means[s][p - p0][u][c] is its mean.
 * mcl_ligrec_observed: side t of interaction i lists the used-column indices members[member_offsets[2 i + t] ..
 *   member_offsets[2 i + t + 1]) ascending; of a complex the member of lowest mean over the kept spots is taken (sum over
 *   the groups ascending / n; ties: the first).  pairs (S, I, 2): the choice.  means, defined, count (S, I, kmax, kmax):
 *   (m1 + m2) / 2 where both group means are > 0, else 0 (NaN with an empty or absent group); defined = both > 0 and both
 *   nnz >= threshold * size; count = 0.
 * mcl_ligrec_count: count[s][i][c1][c2] += the permutations p < pc of perm_means with
 *   (m1' + m2') / 2 >= (m1 + m2) / 2; one thread owns an element.                                                          */
int32_t mcl_ligrec_columns(int32_t n);
int32_t mcl_ligrec_chunk(int32_t S, int32_t kmax, int32_t U, int32_t n_perms);
int64_t mcl_ligrec_workspace_bytes(int32_t S, int32_t kmax, int32_t U, int32_t n_perms);
int mcl_ligrec_prepare(const int64_t* offsets, const int32_t* labels, const int32_t* k, int32_t S, int64_t rows,
                       int32_t max_n, int32_t kmax, int32_t* order, int32_t* start, int64_t* kept_offsets, int32_t* status,
                       mcl_stream_t stream);
int mcl_ligrec_group_means(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, const int64_t* kept_offsets,
                           const int32_t* order, const int32_t* start, const int32_t* k, int32_t S, int64_t rows, int32_t G,
                           int32_t max_n, int32_t kmax, const int32_t* used, int32_t U, int32_t column_mask,
                           const void* table, int32_t n_perms, int32_t p0, int32_t pc, int32_t chunk, double* sum,
                           int32_t* nnz, double* mean, double* frac, double* perm_means, int32_t* status, mcl_stream_t stream);
int mcl_ligrec_observed(int32_t S, int32_t I, int32_t kmax, int32_t U, const int32_t* k, const int32_t* start,
                        const double* sum, const int32_t* nnz, const double* mean, const int32_t* member_offsets,
                        const int32_t* members, double threshold, int32_t* pairs, double* means, int32_t* defined,
                        int32_t* count, mcl_stream_t stream);
int mcl_ligrec_count(int32_t S, int32_t I, int32_t kmax, int32_t U, const int32_t* k, const double* mean,
                     const int32_t* pairs, const double* perm_means, int32_t chunk, int32_t pc, int32_t* count,
                     mcl_stream_t stream);

/* ---------------------------------------------------------------- arrangement of spot groups (ABI 13, entry points added;
 * csrc/nhood.hip).  squidpy.gr.nhood_enrichment / interaction_matrix / co_occurrence: which groups sit next to
 * which on the spot lattice under permutations of the group labels, and which lie within a radius of which.  offsets, labels,
 * k, order, start and kept_offsets are those of mcl_ligrec_prepare, whose status (S, 4) these entry points extend: [2]
 * counts the kept neighbour slots whose index lies outside the slide (they count as pruned), [3] the kept spots with a
 * non-finite coordinate.  2 <= n_s <= max_n <= 16384, kmax <= 255, kw <= 64, n_perms <= 65535, T <= 64, S <= 32767, S kmax^2
 * and S T kmax^2 < 2^31: MCL_EUNSUPPORTED beyond, MCL_EINVAL for a malformed call.  Everything is an integer count (and three
 * fp64 divisions): bit-reproducible, a slide inside a batch is bit-identical to the same slide alone.
 *
 * mcl_nhood_tile_rows: the source groups a workgroup of mcl_nhood_counts takes for a slide of n rows and K groups:
 *   (155648 - 2 ceil16(n)) / (32 K), at least 1, at most K.  mcl_nhood_staged: 1 when the slide's uint16 neighbour list
 *   (2 n kw bytes) fits in LDS beside them, 0 when it is read through L2.
 * mcl_nhood_workspace_bytes: the bytes of work: the uint16 neighbour list.
 * mcl_nhood_counts: nbr (rows, kw) int32 slide-local, w (rows, kw) fp64, 0 = pruned.  count (S, kmax, kmax) int32:
 *   count[c1][c2] = #(spot i, slot c) with w != 0, both ends kept, label(i) = c1, label(nbr) = c2.  table = NULL (n_perms 0):
 *   that alone.  Otherwise the (n_perms, n) uint16 tables of mcl_spatial_permutations at element n_perms * kept_offsets[s]:
 *   under permutation p the spot order[table[p][j]] belongs to the group that owns position j; stats (S, 4, kmax, kmax)
 *   int64: sum of count_p, sum of count_p^2, #(count_p >= count), #(count_p <= count).
 * mcl_cooccur_workspace_bytes: the bytes of work: the coordinates of the kept spots in sorted order.
 * mcl_cooccur_counts: coords (rows, 2) fp64, radii_sq (S, T) fp64 ascending.  pairs (S, T, kmax, kmax) int32: the ordered
 *   pairs i != j of kept spots with label(i) = c1, label(j) = c2 whose FIRST t with d2 <= radii_sq[t] is t; d2 = dx dx + dy dy,
 *   every product and the sum rounded separately.
 * mcl_cooccur_scores: pairs becomes its running sum over t in place; occ (S, T, kmax, kmax) fp64 = (pairs / row) / (col /
 *   tot) with row, col, tot the sums of pairs[t] over c2, c1 and both; NaN where a denominator is 0 or a group is absent. */
int32_t mcl_nhood_tile_rows(int32_t n, int32_t kmax);
int32_t mcl_nhood_staged(int32_t n, int32_t kmax, int32_t kw);
int64_t mcl_nhood_workspace_bytes(int64_t rows, int32_t kw);
int mcl_nhood_counts(const int64_t* offsets, const int64_t* kept_offsets, const int32_t* order, const int32_t* start,
                     const int32_t* k, int32_t S, int64_t rows, int32_t max_n, int32_t kmax, const int32_t* nbr,
                     const double* w, int32_t kw, const void* table, int32_t n_perms, void* work, int32_t* count,
                     int64_t* stats, int32_t* status, mcl_stream_t stream);
int64_t mcl_cooccur_workspace_bytes(int64_t rows);
int mcl_cooccur_counts(const double* coords, const int64_t* offsets, const int32_t* order, const int32_t* start,
                       const int32_t* k, int32_t S, int64_t rows, int32_t max_n, int32_t kmax, const double* radii_sq,
                       int32_t T, void* work, int32_t* pairs, int32_t* status, mcl_stream_t stream);
int mcl_cooccur_scores(const int32_t* k, int32_t S, int32_t kmax, int32_t T, int32_t* pairs, double* occ, mcl_stream_t stream);

/* ---------------------------------------------------------------- spots as mixtures of signatures (ABI 13, entry points
 * added; csrc/deconv.hip).  b_i = argmin over b >= 0 of || x_i - S^T b ||_2 for every spot: what a
 * scipy.optimize.nnls loop computes.  S (T, G) fp64 dense; x (rows, G) fp32 (dtype 0) or fp64 (dtype 1) with the leading
 * dimension ld >= G.  1 <= T <= 64, T <= G <= 16384, rows T < 2^31: MCL_EUNSUPPORTED beyond, MCL_EINVAL for a malformed call.
 * fp64 throughout, no floating-point atomics, every sum in an order that depends on G and T alone: a spot's outputs are
 * bit-identical alone, anywhere in a batch and in a row-permuted batch.
 *
 * mcl_nnls_solve_waves: the spots (one wave each) a workgroup of mcl_nnls_solve takes at a time:
 *   (155648 - 8 T^2) / (8 (T (T + 1) / 2 + ceil(T / 2))), at most 16 (7 at T = 64).
 * mcl_nnls_gram: A (T, T) = S S^T, the upper triangle summed over g ascending and mirrored; L (T, T) the lower Cholesky
 *   factor of A (zeros above the diagonal).  status[0] = 1 + the first type whose pivot is not above T eps A_jj (L is
 *   unfinished then), status[1] = 1 + the first type with a NaN or Inf in its signature (no factor then); 0 = none.
 * mcl_nnls_products: c (rows, T) = x S^T and q (rows,) = x . x on the fp64 MFMA, x read once.  status[0] = 0, or
 *   2^32 - 1 - r as an unsigned word for the first row r that holds a non-finite entry.
 * mcl_nnls_solve: Lawson-Hanson's active-set method on (A, c_i), one wave per spot: from b = 0, P empty, w = c; the
 *   largest w_j outside P enters (ties: the smaller j) until P is full or that w_j <= 10 T eps max|c_i|; A_PP z = c_P by the
 *   Cholesky factor of A_PP, a row appended per entering index and recomputed from the first removed position on; z_P > 0
 *   is accepted, else b steps to the boundary (alpha = min b_j / (b_j - z_j) over z_j <= 0) and every index with b_j <= 0
 *   leaves with b_j = 0 exactly; an entering index whose own z_j <= 0 leaves at once with w_j = 0.  At most 3 T solves:
 *   beyond, or where a pivot of A_PP is not above T eps A_jj, the spot keeps its last feasible iterate with converged = 0.
 *   coef (rows, T) fp64, n_iter (rows,) int32 (the solves), converged (rows,) uint8.
 * mcl_nnls_residual: rnorm (rows,) = || x_i - S^T b_i ||_2 summed from x itself, r2 = 1 - rnorm^2 / q (NaN where q = 0),
 *   proportions (rows, T) = coef / sum(coef) (a zero row where the sum is 0), dominant (rows,) int32 = its argmax (ties:
 *   the smaller index; -1 for a zero row). */
int32_t mcl_nnls_solve_waves(int32_t T);
int mcl_nnls_gram(const double* S, int32_t T, int32_t G, double* A, double* L, int32_t* status, mcl_stream_t stream);
int mcl_nnls_products(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, const double* S, int32_t T,
                      double* c, double* q, int32_t* status, mcl_stream_t stream);
int mcl_nnls_solve(const double* A, const double* c, int64_t rows, int32_t T, double* coef, int32_t* n_iter,
                   void* converged, mcl_stream_t stream);
int mcl_nnls_residual(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, const double* S, int32_t T,
                      const double* coef, const double* q, double* rnorm, double* r2, double* proportions,
                      int32_t* dominant, mcl_stream_t stream);

/* ---------------------------------------------------------------- local spatial statistics (ABI 13, entry points added;
 * csrc/hotspot.hip).  Local Moran's I_i, Getis-Ord Gi*, quadrant and hot / cold spot label of every (spot,
 * column pair) with a conditional permutation test, on the graph mcl_spatial_lattice writes (nbr, w (rows, k); a slot with
 * w = 0 is pruned; the kept slots of a row share one weight).  Slide s owns rows offsets[s] .. offsets[s + 1] (device int64,
 * S + 1 entries); 2 <= n_s <= max_n <= 16384, 1 <= k <= 64, G <= 16384, M <= 16384 pairs, n_perms <= 65535, S <= 65535:
 * anything else is MCL_EINVAL before a launch.  pairs (M, 2) device int32: (held column a, lagged column b); a == b is the
 * univariate case.  x (rows, G), dtype 0 fp32 / 1 fp64, row stride ld.  Per-(spot, pair) arrays are (rows, M).  status
 * (S, 4), zeroed by the caller: offsets that break the statements, non-finite values of x, pair columns outside 0 .. G - 1,
 * replayed draws that do not fit the graph.  fp64, no contraction, no floating-point atomics, deterministic; a slide inside
 * a batch is bit-identical to the same slide alone.
 *
 * mcl_hotspot_columns: the lagged columns a workgroup of mcl_hotspot_permute takes for a slide of n rows (1 .. 6).
 * mcl_hotspot_table_bytes: the draw table: uint16 (n_perms, n_s, k) per slide at element offset n_perms * k * offsets[s].
 * mcl_hotspot_moments: mean and den = sum (x - mean)^2 (2, S, M) of the held (plane 0) and the lagged (plane 1) column of
 *   every pair in the fixed row order of mcl_spatial_stats (bit-equal to its mean / den); a constant column has den = 0.
 * mcl_hotspot_draws: materialises the draws: entry (p, i, t) is the t-th of the d_i = min(kept slots, n - 1) distinct spots
 *   other than i drawn for spot i in draw p, a function of (seed, p, i, n, d_i) alone; slots t >= d_i hold 0xFFFF.
 * mcl_hotspot_permute: lag (rows, M) = sum of the centred lagged column over the kept slots in slot order; with n_perms > 0
 *   the same sum over each draw in draw order: count_ge / count_le = #(L^p >= / <= L), sum1 = sum L^p, sum2 = sum (L^p)^2 over
 *   p ascending.  table = NULL: the draws are generated in the kernel from seed; else they are read from the table.
 *   deg / wbar (rows,): kept slots and their common weight.  column_mask: bit c set = launch the c-column kernel.
 * mcl_hotspot_finalise: local_i = (n - 1) z_a (wbar lag) / den_a (a != b: / sqrt(den_a den_b)); quadrant int8 1 HH, 2 LH,
 *   3 LL, 4 HL, 0 where a sign is zero; gi_z = (z + lag) / (sqrt(den / n) sqrt((d + 1)(n - d - 1) / (n - 1))) (a == b only,
 *   NaN at n = d + 1), its one-tailed normal p and -log10 p in log space; with n_perms > 0 pval_sim = (min(count_ge,
 *   count_le) + 1) / (n_perms + 1), mean_sim / var_sim / z_sim of the sims of local_i, cluster int8 = quadrant where
 *   pval_sim <= alpha else 0.  A constant column: NaN in every floating output, 0 in quadrant and cluster. */
int32_t mcl_hotspot_columns(int32_t n);
int64_t mcl_hotspot_table_bytes(int64_t rows, int32_t k, int32_t n_perms);
int mcl_hotspot_moments(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                        int32_t max_n, const int32_t* pairs, int32_t M, double* mean, double* den, int32_t* status,
                        mcl_stream_t stream);
int mcl_hotspot_draws(const int64_t* offsets, int32_t S, int64_t rows, int32_t max_n, int32_t k, const double* w,
                      int32_t n_perms, uint64_t seed, void* table, mcl_stream_t stream);
int mcl_hotspot_permute(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                        int32_t max_n, int32_t k, int32_t column_mask, const int32_t* nbr, const double* w,
                        const int32_t* pairs, int32_t M, const double* mean, const double* den, const void* table,
                        int32_t n_perms, uint64_t seed, double* lag, int32_t* count_ge, int32_t* count_le, double* sum1,
                        double* sum2, int32_t* deg, double* wbar, int32_t* status, mcl_stream_t stream);
int mcl_hotspot_finalise(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G,
                         int32_t max_n, const int32_t* pairs, int32_t M, const double* mean, const double* den,
                         const int32_t* deg, const double* wbar, const double* lag, const int32_t* count_ge,
                         const int32_t* count_le, const double* sum1, const double* sum2, int32_t n_perms, double alpha,
                         double* local_i, void* quadrant, double* gi_z, double* gi_pval_norm, double* gi_neglog10_pval_norm,
                         double* pval_sim, double* mean_sim, double* var_sim, double* z_sim, void* cluster,
                         mcl_stream_t stream);

/* ---------------------------------------------------------------- rank agreement of predictions (csrc/rank.hip; added
 * under ABI 13: new entry points only).  Spearman's rho and Kendall's tau-b of pred against truth, the two other values of
 * ``func`` in the reference's get_R(data1, data2, dim, func) (utils.py:52-65), on both ``dim``s.  pred, truth: rows x G,
 * leading dimensions ld_pred / ld_true (elements), dtype codes 0 = fp32, 1 = fp64, each its own.
 *   axis 0 (genes, dim=1): problem (s, g) = column g over the rows offsets[s] .. offsets[s + 1] (device-resident int64, as
 *     for mcl_expr_metrics); S * G problems, problem index s * G + g; max_n = the largest segment (sizes the launch: a
 *     segment that is longer, shorter than 2 or leaves the rows sets status[3 s + 2] and keeps n = 0 in its problems).
 *   axis 1 (spots, dim=0): problem i = row i over the G genes; rows problems; offsets is not read (may be NULL), S = 1,
 *     max_n = G.
 * Limits: mcl_rank_max_elements(pred_dtype, true_dtype) elements per vector = 16384 when both sides are fp32, 8192 with an
 *   fp64 side (what the LDS plan of a workgroup holds; -1 for an unknown dtype code); G <= 16384; S <= 65535; MCL_EINVAL
 *   beyond.  mcl_rank_columns(n, ...) = the problems of n elements one workgroup takes (-1 outside 2 .. the limit).
 * mcl_rank_stats: ints[problems x 12] int64, exact: { n, Sxy = sum a_x a_y with a = twice the 1-based average rank (-0.0
 *   ties +0.0), then over the tie runs t of pred / truth: Tx, Ty = sum (t^3 - t); xtie, ytie = sum t(t-1)/2; x0, y0 = sum
 *   t(t-1)(t-2); x1, y1 = sum t(t-1)(2t+5); joint = the pairs i < j tied on both sides; s = sum_{i<j} sign(a_x[i] - a_x[j])
 *   sign(a_y[i] - a_y[j]) }.  joint and s are 0 when tau == 0 (the O(n^2) pair walk is skipped).
 *   status[S x 3] int32 (zeroed by the call): the non-finite values met, 0x7fffffff - the smallest problem index within
 *   the segment (gene; row for axis 1) that holds one, and the refused flag.  A non-finite value never faults; the
 *   outputs of its segment are then unspecified.
 * mcl_rank_finish: per problem, fp64 without contraction, NaN where n < 2 or a side is constant:
 *   rho = (n Sxy - n^2 (n+1)^2) / (sqrt(d_x) sqrt(d_y)), d = n (n^3 - n - T) / 3, clipped to [-1, 1]; exactly +-1 where
 *   numerator^2 = d_x d_y (perfect agreement, decided on the integers; the same rule for tau_b);
 *   tau_b = s / (sqrt(n0 - xtie) sqrt(n0 - ytie)), n0 = n (n-1) / 2, clipped; tau_p = erfc(|z| / sqrt 2), z = s / sqrt(var),
 *   var = (m (2n+5) - x1 - y1) / 18 + 2 xtie ytie / m + x0 y0 / (9 m (n-2)), m = n (n-1) (scipy.stats.kendalltau,
 *   method="asymptotic"); tau_neglog10p in log space, finite where tau_p underflows; both NaN at n < 3.  With tau == 0
 *   only rho is written (the tau pointers may be NULL).  Spearman's p is mcl_pearson_pvalue of rho.
 * mcl_rank_summary: rho, tau_b (S x G; tau_b may be NULL), heg (S x n_heg) as mcl_expr_metrics writes it -> summary[S x 5]
 *   = { heg_rho = mean of rho over heg (NaN propagates, np.mean), hvg_rho = mean over the non-NaN genes (NaN if none),
 *   heg_tau, hvg_tau (NaN without tau_b), n_valid }, every sum in gene-index order.                                  */
int32_t mcl_rank_max_elements(int32_t pred_dtype, int32_t true_dtype);
int32_t mcl_rank_columns(int32_t n, int32_t pred_dtype, int32_t true_dtype);
int mcl_rank_stats(const void* pred, int64_t ld_pred, int32_t pred_dtype, const void* truth, int64_t ld_true,
                   int32_t true_dtype, const int64_t* offsets, int32_t S, int64_t rows, int32_t G, int32_t max_n,
                   int32_t axis, int32_t tau, int64_t* ints, int32_t* status, mcl_stream_t stream);
int mcl_rank_finish(const int64_t* ints, int64_t problems, int32_t tau, double* rho, double* tau_b, double* tau_p,
                    double* tau_neglog10p, mcl_stream_t stream);
int mcl_rank_summary(const double* rho, const double* tau_b, const int64_t* heg, int32_t S, int32_t G, int32_t n_heg,
                     double* summary, mcl_stream_t stream);

/* ---------------------------------------------------------------- gene programs: batched NMF (csrc/nmf.hip)
 * X ~ W H with W, H >= 0 by scikit-learn's multiplicative-update solver (non_negative_factorization(solver="mu"), no
 * regularisation), for every row segment of a row-stacked x (rows, G; dtype 0 fp32 / 1 fp64, leading dimension ld >= G,
 * offsets device int64 [S + 1]) times every one of n_init starts per call.  Problem p = segment * n_init + start; W is
 * (n_init, rows, k), H is (S n_init, k, G), both fp64 and updated in place; active (S n_init) int32 is 1 for a problem that
 * still iterates (the caller sets it; a problem whose word is 0 is frozen: no kernel touches it).  loss: 0 Frobenius,
 * 1 Kullback-Leibler.  1 <= k <= 64, G <= 16384, S n_init <= 65535, rows k < 2^31: MCL_EUNSUPPORTED beyond (-1 from
 * mcl_nmf_workspace_bytes), MCL_EINVAL for a malformed call.  fp64 throughout, no floating-point atomics; every sum runs
 * in an order fixed by the segment's rows, G and k.  work holds mcl_nmf_workspace_bytes bytes (the same arguments).
 * mcl_nmf_check: status[0] = 0, or 0xFFFFFFFF - the first row of x that holds a negative or non-finite value.
 * mcl_nmf_steps: n_steps iterations.  Per iteration W <- W o (X H^T) / (W (H H^T)) then, where update_h, H <- H o (W^T X) /
 *   ((W^T W) H) from the new W (Frobenius); W <- W o ((X / WH) H^T) / rowsum(H), H <- H o (W^T (X / WH)) / colsum(W) and
 *   H < 2^-52 -> 0 (KL).  WH below EPSILON = 2^-23 is EPSILON, a zero denominator is EPSILON (colsum(W) = 0: 1).
 * mcl_nmf_error: error = sqrt(2 D(X | W H)) summed from x itself, and by phase: 0 the error at init; 1 the check of
 *   iteration it -- a live problem with (previous - error) / error_at_init < tol is frozen (active = 0, n_iter = it,
 *   converged = it < max_iter), else previous = error; 2 the final error of every problem.  record (S n_init, 8) fp64:
 *   { error at init, previous, last, n_iter, converged, final, 0, 0 }; history (S n_init, hist_len): slot it / 10.
 * mcl_nmf_programs: for one W (rows, k) and H (S, k, G): hsum = rowsum(H), programs = H / hsum (0 where hsum = 0),
 *   usage = W o hsum, dominant = argmax of usage (ties: the smaller index; -1 for a zero row).                            */
int64_t mcl_nmf_workspace_bytes(int64_t rows, int32_t G, int32_t k, int32_t S, int32_t n_init, int32_t max_n, int32_t loss);
int mcl_nmf_check(const void* x, int64_t ld, int32_t dtype, int64_t rows, int32_t G, int32_t* status, mcl_stream_t stream);
int mcl_nmf_steps(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t n_init, int64_t rows,
                  int32_t G, int32_t k, int32_t max_n, int32_t loss, int32_t update_h, double* W, double* H, double* work,
                  int32_t* active, int32_t n_steps, mcl_stream_t stream);
int mcl_nmf_error(const void* x, int64_t ld, int32_t dtype, const int64_t* offsets, int32_t S, int32_t n_init, int64_t rows,
                  int32_t G, int32_t k, int32_t max_n, int32_t loss, const double* W, const double* H, double* work,
                  int32_t* active, int32_t phase, int32_t it, double tol, int32_t max_iter, double* record, double* history,
                  int32_t hist_len, mcl_stream_t stream);
int mcl_nmf_programs(const double* W, const double* H, const int64_t* offsets, int32_t S, int64_t rows, int32_t G, int32_t k,
                     int32_t max_n, double* hsum, double* programs, double* usage, int32_t* dominant, mcl_stream_t stream);

/* ---------------------------------------------------------------- input pipeline on the GPU
 * mcl_patch_gather: the reference's per-spot patch extraction (dataset.py:226-231 PIL crop + transforms.ToTensor;
 *   dataset.py:330-336 numpy crop of the cv2 image + TenxDataset.transform) for a whole batch: image_u8 (Hs, Ws, 3)
 *   uint8 resident in HBM, centers_rc (N, 2) int32 (row, col), patch side 2r.  Source pixels outside the image read 0.
 *   ops (N bytes, may be NULL): bit 0 horizontal flip, bit 1 vertical flip, bits 2-3 = k: then a counter-clockwise
 *   rotation by k*90 degrees (TF.hflip -> TF.vflip -> TF.rotate(angle), angle = 90 k).  Values are divided by divisor
 *   (255: ToTensor's .div(255); 1: Tenx) and written as fp32 NCHW (N,3,2r,2r) and/or bf16 NHWC (N,2r,2r,3); either may be NULL.
 * mcl_log_library_size_normalize: out = log10(counts / rowsum(counts) * rescale + 1) (scprep.transform.log(
 *   scprep.normalize.library_size_normalize(.)), dataset.py:188-189; rescale 1e4); all-zero rows stay zero.      */
int mcl_patch_gather(const void* image_u8, int32_t Hs, int32_t Ws, const int32_t* centers_rc, int32_t N, int32_t r,
                     const void* ops, float divisor, float* out_nchw_f32, void* out_nhwc_bf16, mcl_stream_t stream);
int mcl_log_library_size_normalize(const float* counts, int64_t ldx, float* out, int64_t ldy, int32_t rows,
                                   int32_t cols, float rescale, mcl_stream_t stream);

/* HER2ST / cSCC training transform (/root/reference/dataset.py:63-68: ColorJitter(0.5,0.5,0.5), RandomHorizontalFlip,
 * RandomRotation(180), ToTensor) for a batch of patches cropped from the resident slide, with the random draws supplied:
 * params = N records of 16 32-bit words {order (2 bits per step: 0 brightness, 1 contrast, 2 saturation), hflip,
 * rot_mode (0 quarter turns / 1 affine), rot_k, brightness, contrast, saturation (float), a[6] = libImaging's 16.16
 * fixed-point affine coefficients, 3 pad}.  Bit-exact with PIL (ImageEnhance / Image.rotate NEAREST).  2r <= 232.   */
int mcl_her2st_train_patches(const void* image_u8, int32_t Hs, int32_t Ws, const int32_t* centers_rc, int32_t N, int32_t r,
                             const void* params, float divisor, float* out_nchw_f32, void* out_nhwc_bf16,
                             mcl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCLSTEXP_HIP_H */
