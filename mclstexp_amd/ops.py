"""Host-side launch wrappers and hand-derived autograd for the HIP kernels (C ABI via ctypes).

Every function here takes fp32 tensors resident on the GPU and enqueues kernels on torch's current
stream.  CPU tensors are rejected: there is no fallback path.  The backward passes are written out
kernel by kernel (the reference obtains them from autograd, train.py:38).

Reference call sites are cited per function (paths relative to /root/reference/).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import (COMPUTE_BF16, COMPUTE_F32, EPI_ACCUM, EPI_GELU, EPI_GELU_BWD, GemmArgs, call)

Tensor = torch.Tensor
LN_EPS = 1e-5

_compute_mode = COMPUTE_F32


def set_compute(mode: str) -> None:
    """'f32' (exact fp32 MFMA, reference numerics) or 'bf16' (bf16 MFMA operands, fp32 accumulate)."""
    global _compute_mode
    _compute_mode = {"f32": COMPUTE_F32, "fp32": COMPUTE_F32, "bf16": COMPUTE_BF16}[mode]


def get_compute() -> str:
    return "bf16" if _compute_mode == COMPUTE_BF16 else "f32"


class forced_compute:
    """``with forced_compute(COMPUTE_F32):`` -- every mcl_gemm inside runs in that mode whatever set_compute() says (the fp32
    "reference numerics" image encoders: /root/reference/model.py:104-116 computes in fp32)."""

    def __init__(self, mode: Optional[int]):
        self.mode = mode

    def __enter__(self):
        global _compute_mode
        self.old = _compute_mode
        if self.mode is not None:
            _compute_mode = self.mode

    def __exit__(self, *exc):
        global _compute_mode
        _compute_mode = self.old
        return False


_stream = _lib.current_stream            # (tests and tools that call the C ABI directly pass it)


def _chk(t: Tensor, name: str = "tensor") -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"mclstexp_amd: {name} is on {t.device}; the hot path runs only on the GPU "
                           "(HIP kernels, no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"mclstexp_amd: {name} must be float32, got {t.dtype}")
    return t


def _rowmajor(t: Tensor, name: str = "tensor") -> Tensor:
    """2-D view with unit stride along the last dim (makes a copy only if needed)."""
    _chk(t, name)
    if t.dim() != 2:
        raise RuntimeError(f"{name}: expected 2-D, got shape {tuple(t.shape)}")
    if t.stride(1) != 1 and t.shape[1] != 1:
        t = t.contiguous()
    if t.shape[1] == 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- GEMM
SPLIT_K = True


def gemm_raw(M: int, N: int, K: int, batch: int, A: Tensor, sAm: int, sAk: int, sAb: int, B: Tensor, sBk: int,
             sBn: int, sBb: int, Cmat: Tensor, ldc: int, sCb: int, alpha: float = 1.0, flags: int = 0,
             bias: Optional[Tensor] = None, resid: Optional[Tensor] = None, ldr: int = 0, sRb: int = 0,
             pre_out: Optional[Tensor] = None, ldp: int = 0, aux: Optional[Tensor] = None, ldaux: int = 0,
             a_off: int = 0, b_off: int = 0, c_off: int = 0, compute: Optional[int] = None, filt=None) -> None:
    """mcl_gemm with explicit strides; *_off are element offsets into A/B/C's storage views.  ``filt`` = (thr (M,), cnt (M,)
    int32 zeroed, cand_val (M, cap), cand_idx (M, cap) int32): nothing is stored to C (pass None); products >= thr[row] are
    appended to the row's candidate list (retrieval's fused similarity + top-k)."""
    a = _lib.gemm_args()
    a.M, a.N, a.K, a.batch = M, N, K, batch
    a.A, a.sAm, a.sAk, a.sAb = A.data_ptr() + 4 * a_off, sAm, sAk, sAb
    a.B, a.sBk, a.sBn, a.sBb = B.data_ptr() + 4 * b_off, sBk, sBn, sBb
    if filt is not None:
        thr, cnt, cval, cidx = filt
        a.flt_thr, a.flt_cnt, a.flt_val, a.flt_idx, a.flt_cap = thr.data_ptr(), cnt.data_ptr(), cval.data_ptr(), cidx.data_ptr(), cval.shape[1]
        a.C, a.ldc, a.sCb = None, N, 0
    else:
        a.C, a.ldc, a.sCb = Cmat.data_ptr() + 4 * c_off, ldc, sCb
    a.alpha, a.flags = alpha, flags
    a.bias = _p(bias)
    a.resid, a.ldr, a.sRb = _p(resid), ldr, sRb
    a.pre_out, a.ldp = _p(pre_out), ldp
    a.aux, a.ldaux = _p(aux), ldaux
    a.compute = _compute_mode if compute is None else compute
    ks = call("mcl_gemm_auto_ksplit", M, N, K, batch) if (SPLIT_K and filt is None) else 1
    if ks > 1:    # skinny problem (M = a batch of spots): K slices + fixed-order merge fill the chip
        ws = torch.empty(ks * batch * M * N, device=Cmat.device, dtype=torch.float32)
        a.ksplit, a.workspace = ks, ws.data_ptr()
    call("mcl_gemm", C.byref(a))


def linear_fwd(x: Tensor, W: Tensor, bias: Optional[Tensor] = None, gelu: bool = False,
               resid: Optional[Tensor] = None, save_pre: bool = False, alpha: float = 1.0
               ) -> Tuple[Tensor, Optional[Tensor]]:
    """y = epi(alpha * x W^T + b): nn.Linear forward (model.py:23,27,43,45,155,157) with the fused epilogue."""
    x, W = _rowmajor(x, "x"), _rowmajor(W, "W")
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K, (x.shape, W.shape)
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    pre = torch.empty((M, N), device=x.device, dtype=torch.float32) if save_pre else None
    if resid is not None:
        resid = _rowmajor(resid, "resid")
    gemm_raw(M, N, K, 1, x, x.stride(0), 1, 0, W, 1, W.stride(0), 0, y, N, 0, alpha, EPI_GELU if gelu else 0,
             bias, resid, resid.stride(0) if resid is not None else 0, 0, pre, N)
    return y, pre


def linear_bwd_data(dy: Tensor, W: Tensor, gelu_bwd_aux: Optional[Tensor] = None,
                    resid: Optional[Tensor] = None) -> Tensor:
    """dx = (dy W) [* gelu'(aux)] [+ resid]."""
    dy, W = _rowmajor(dy, "dy"), _rowmajor(W, "W")
    M, N = dy.shape
    K = W.shape[1]
    assert W.shape[0] == N
    dx = torch.empty((M, K), device=dy.device, dtype=torch.float32)
    flags = EPI_GELU_BWD if gelu_bwd_aux is not None else 0
    if resid is not None:
        resid = _rowmajor(resid, "resid")
    gemm_raw(M, K, N, 1, dy, dy.stride(0), 1, 0, W, W.stride(0), 1, 0, dx, K, 0, 1.0, flags, None, resid,
             resid.stride(0) if resid is not None else 0, 0, None, 0, gelu_bwd_aux,
             gelu_bwd_aux.stride(0) if gelu_bwd_aux is not None else 0)
    return dx


# When a weight already owns a dense fp32 .grad (FusedAdam's flat bucket, zeroed every step) its gradient GEMM adds
# straight into it and autograd gets None: no temporary, no AccumulateGrad add kernel (12 of them per spot-path step).
DIRECT_PARAM_GRADS = True


def _direct_grad_ok(p) -> bool:
    """Pure predicate (this path never creates a .grad).  A parameter with tensor / post-accumulate-grad hooks is excluded:
    the hooks fire from autograd's AccumulateGrad node, which a kernel-side accumulation never reaches."""
    if not getattr(p, "is_leaf", True):       # a view of a parameter (reshaped patch-embedding weight): autograd routes it
        return False
    g = getattr(p, "grad", None)
    if getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
        return False
    return (DIRECT_PARAM_GRADS and g is not None and g.dtype == torch.float32 and g.is_cuda and g.shape == p.shape
            and g.is_contiguous() and p.is_contiguous() and not g.requires_grad)


def linear_bwd_weight(dy: Tensor, x: Tensor, param: Optional[Tensor] = None) -> Optional[Tensor]:
    """dW = dy^T x  (N, K); with ``param`` (the weight Parameter) owning a dense .grad: param.grad += dW, returns None."""
    dy, x = _rowmajor(dy, "dy"), _rowmajor(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M
    if param is not None and param.shape == (N, K) and _direct_grad_ok(param):
        gemm_raw(N, K, M, 1, dy, 1, dy.stride(0), 0, x, x.stride(0), 1, 0, param.grad, K, 0, flags=EPI_ACCUM)
        return None
    dW = torch.empty((N, K), device=dy.device, dtype=torch.float32)
    gemm_raw(N, K, M, 1, dy, 1, dy.stride(0), 0, x, x.stride(0), 1, 0, dW, K, 0)
    return dW


def colsum(x: Tensor, param: Optional[Tensor] = None) -> Optional[Tensor]:
    """Column sums (nn.Linear bias gradient).  With ``param`` (the bias Parameter) owning a dense fp32 .grad the sums are
    ADDED straight into it and None is returned to autograd (no temporary, no AccumulateGrad add launch)."""
    x = _rowmajor(x, "x")
    ws = _rowred_ws(x.shape[0], x.shape[1], x.device)
    if param is not None and param.shape == (x.shape[1],) and _direct_grad_ok(param):
        call("mcl_colsum_ws", x, x.stride(0), param.grad, x.shape[0], x.shape[1], 1, ws)
        return None
    out = torch.empty((x.shape[1],), device=x.device, dtype=torch.float32)
    call("mcl_colsum_ws", x, x.stride(0), out, x.shape[0], x.shape[1], 0, ws)
    return out


def colred_group(sums, norms=()):
    """One launch for a layer's column reductions.  ``sums``: (x, bias Parameter or None) pairs -> bias gradients;
    ``norms``: (dy, x, mean, rstd, (weight, bias) Parameters) -> LayerNorm parameter gradients.  Returns (list of bias-gradient
    tensors, list of (dgamma, dbeta)) for autograd -- None where the sums went straight into the parameters' .grad."""
    a, lda, xs, ldx, mean, rstd, o0, o1, cols, acc = ([] for _ in range(10))
    out_s, out_n = [], []
    rows = None
    for x, q in sums:
        x = _rowmajor(x, "x")
        rows = x.shape[0] if rows is None else rows
        assert x.shape[0] == rows
        direct = q is not None and q.shape == (x.shape[1],) and _direct_grad_ok(q)
        t = q.grad if direct else torch.empty((x.shape[1],), device=x.device, dtype=torch.float32)
        out_s.append(None if direct else t)
        a.append(x.data_ptr()); lda.append(x.stride(0)); xs.append(None); ldx.append(0); mean.append(None); rstd.append(None)
        o0.append(t.data_ptr()); o1.append(None); cols.append(x.shape[1]); acc.append(direct)
    for dy, x, mu, rs, params in norms:
        dy, x = _rowmajor(dy, "dy"), _rowmajor(x, "x")
        rows = x.shape[0] if rows is None else rows
        assert x.shape[0] == rows and dy.shape == x.shape
        n = x.shape[1]
        direct = (params is not None and params[0].shape == (n,) and params[1].shape == (n,)
                  and _direct_grad_ok(params[0]) and _direct_grad_ok(params[1]))
        if direct:
            dg, db = params[0].grad, params[1].grad
        else:
            dg = torch.empty((n,), device=x.device, dtype=torch.float32)
            db = torch.empty((n,), device=x.device, dtype=torch.float32)
        out_n.append((None, None) if direct else (dg, db))
        a.append(dy.data_ptr()); lda.append(dy.stride(0)); xs.append(x.data_ptr()); ldx.append(x.stride(0))
        mean.append(mu.data_ptr()); rstd.append(rs.data_ptr())
        o0.append(dg.data_ptr()); o1.append(db.data_ptr()); cols.append(n); acc.append(direct)
    n = len(a)
    vp, i64, i32 = C.c_void_p * n, C.c_int64 * n, C.c_int32 * n
    call("mcl_colred_group", n, vp(*a), i64(*lda), vp(*xs), i64(*ldx),
         vp(*mean), vp(*rstd), vp(*o0), vp(*o1), i32(*cols), i32(*acc), rows)
    return out_s, out_n


def _rowred_ws(rows: int, cols: int, device) -> Optional[Tensor]:
    """Chunk-partial workspace of the many-row column reductions (None for the spot branch's few rows: the one-launch forms)."""
    if rows <= 1024:
        return None
    return torch.empty(call("mcl_rowred_workspace_floats", rows, cols), device=device, dtype=torch.float32)


# --------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = LN_EPS) -> Tuple[Tensor, Tensor, Tensor]:
    x = _rowmajor(x, "x")
    rows, cols = x.shape
    y = torch.empty((rows, cols), device=x.device, dtype=torch.float32)
    mean = torch.empty((rows,), device=x.device, dtype=torch.float32)
    rstd = torch.empty((rows,), device=x.device, dtype=torch.float32)
    call("mcl_layernorm_fwd", x, x.stride(0), _chk(gamma), _chk(beta), y, cols, mean, rstd, rows, cols, eps)
    return y, mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor,
                  dx_add: Optional[Tensor] = None, params: Optional[Tuple[Tensor, Tensor]] = None, dx_only: bool = False
                  ) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """``params`` = (weight, bias) Parameters: when both own a dense fp32 .grad, dgamma / dbeta are added straight into them
    and (dx, None, None) is returned.  ``dx_only``: the parameter gradients are left to a grouped launch (colred_group)."""
    dy, x = _rowmajor(dy, "dy"), _rowmajor(x, "x")
    rows, cols = x.shape
    dx = torch.empty((rows, cols), device=x.device, dtype=torch.float32)
    if dx_only:
        if dx_add is not None:
            dx_add = _rowmajor(dx_add, "dx_add")
        call("mcl_layernorm_bwd_ws", dy, dy.stride(0), x, x.stride(0), gamma, mean, rstd, dx_add,
             dx_add.stride(0) if dx_add is not None else 0, dx, cols, None, None, 0, rows, cols, None)
        return dx, None, None
    direct = (params is not None and params[0].shape == (cols,) and params[1].shape == (cols,)
              and _direct_grad_ok(params[0]) and _direct_grad_ok(params[1]))
    if direct:
        dg, db = params[0].grad, params[1].grad
    else:
        dg = torch.empty((cols,), device=x.device, dtype=torch.float32)
        db = torch.empty((cols,), device=x.device, dtype=torch.float32)
    if dx_add is not None:
        dx_add = _rowmajor(dx_add, "dx_add")
    call("mcl_layernorm_bwd_ws", dy, dy.stride(0), x, x.stride(0), gamma, mean, rstd, dx_add,
         dx_add.stride(0) if dx_add is not None else 0, dx, cols, dg, db, direct, rows, cols, _rowred_ws(rows, cols, x.device))
    return (dx, None, None) if direct else (dx, dg, db)


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dim (model.py:13,158)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        y, mean, rstd = layernorm_fwd(x2, gamma, beta, eps)
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shp = shp
        ctx.lparams = (gamma, beta)
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, mean, rstd = ctx.saved_tensors
        dx, dg, db = layernorm_bwd(dy.reshape(x2.shape), x2, gamma, mean, rstd, params=ctx.lparams)
        return dx.view(ctx.shp), dg, db, None


# --------------------------------------------------------------------------- attention core (v1: materialised P)
def _attention_fusable(qkv: Tensor, dim_head: int) -> bool:
    return (dim_head == 64 and qkv.dtype == torch.float32 and qkv.stride(1) == 1 and qkv.stride(0) % 4 == 0
            and qkv.data_ptr() % 16 == 0)


def attention_core_fwd(qkv: Tensor, heads: int, dim_head: int, nseq: int = 1) -> Tuple[Tensor, Tensor]:
    """model.py:52-56 on the (B, 3*h*d) to_qkv output: returns (out (B, h*d), aux) where aux is what the backward needs:
    the row log-sum-exp (h, B) of the fused kernel (csrc/attention.hip: head dimension 64, no (h, B, B) tensor in HBM), or
    the probabilities P (h, B, B) of the GEMM + softmax sequence (any head dimension, unaligned views).
    ``nseq`` > 1: the rows are nseq independent sequences of B / nseq tokens (the fp32 ViT, one sequence per image; fused
    kernel only)."""
    if _attention_fusable(qkv, dim_head):
        rows, inner = qkv.shape[0], heads * dim_head
        if rows % nseq:
            raise RuntimeError(f"attention: {rows} rows are not {nseq} sequences")
        T = rows // nseq
        out = torch.empty((rows, inner), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((nseq * heads, T), device=qkv.device, dtype=torch.float32)
        call("mcl_attention_batched_fwd", qkv, qkv.stride(0), T, nseq, heads, dim_head, dim_head ** -0.5, out, inner, lse)
        return out, lse
    if nseq != 1:
        raise RuntimeError("attention: several sequences need the fused kernel (head dimension 64, fp32, aligned rows)")
    return attention_core_fwd_unfused(qkv, heads, dim_head)


def attention_core_bwd(dout: Tensor, qkv: Tensor, out: Tensor, aux: Tensor, heads: int, dim_head: int, nseq: int = 1) -> Tensor:
    """Returns dqkv (B, 3*h*d); ``aux`` as returned by attention_core_fwd."""
    if aux.dim() == 3:
        return attention_core_bwd_unfused(dout, qkv, aux, heads, dim_head)
    rows, inner = qkv.shape[0], heads * dim_head
    T = rows // nseq
    dout = _rowmajor(dout, "dout")
    if dout.data_ptr() % 16 or dout.stride(0) != inner or out.stride(0) != inner:
        dout = dout.contiguous()
        out = out.contiguous()
    dqkv = torch.empty((rows, 3 * inner), device=qkv.device, dtype=torch.float32)
    dvec = torch.empty((nseq * heads, T), device=qkv.device, dtype=torch.float32)
    call("mcl_attention_batched_bwd", qkv, qkv.stride(0), T, nseq, heads,
         dim_head, dim_head ** -0.5, out, dout, inner, aux, dvec, dqkv, 3 * inner)
    return dqkv


def attention_core_fwd_unfused(qkv: Tensor, heads: int, dim_head: int) -> Tuple[Tensor, Tensor]:
    """The GEMM + softmax sequence: returns (out (B, h*d), P (h, B, B))."""
    B = qkv.shape[0]
    inner = heads * dim_head
    ld = qkv.stride(0)
    P = torch.empty((heads, B, B), device=qkv.device, dtype=torch.float32)
    # scores_h = q_h k_h^T
    gemm_raw(B, B, dim_head, heads, qkv, ld, 1, dim_head, qkv, 1, ld, dim_head, P, B, B * B, b_off=inner)
    call("mcl_softmax_rows_fwd", P, B, heads * B, B, dim_head ** -0.5)
    out = torch.empty((B, inner), device=qkv.device, dtype=torch.float32)
    # out_h = P_h v_h
    gemm_raw(B, dim_head, B, heads, P, B, 1, B * B, qkv, ld, 1, dim_head, out, inner, dim_head, b_off=2 * inner)
    return out, P


def attention_core_bwd_unfused(dout: Tensor, qkv: Tensor, P: Tensor, heads: int, dim_head: int) -> Tensor:
    """Returns dqkv (B, 3*h*d)."""
    B = qkv.shape[0]
    inner = heads * dim_head
    ld = qkv.stride(0)
    dout = _rowmajor(dout, "dout")
    ldo = dout.stride(0)
    dqkv = torch.empty((B, 3 * inner), device=qkv.device, dtype=torch.float32)
    ldq = 3 * inner
    # dV_h = P_h^T dO_h
    gemm_raw(B, dim_head, B, heads, P, 1, B, B * B, dout, ldo, 1, dim_head, dqkv, ldq, dim_head, c_off=2 * inner)
    # dP_h = dO_h v_h^T
    dP = torch.empty_like(P)
    gemm_raw(B, B, dim_head, heads, dout, ldo, 1, dim_head, qkv, 1, ld, dim_head, dP, B, B * B, b_off=2 * inner)
    call("mcl_softmax_rows_bwd", P, dP, B, heads * B, B, dim_head ** -0.5)
    # dq_h = dS_h k_h ; dk_h = dS_h^T q_h
    gemm_raw(B, dim_head, B, heads, dP, B, 1, B * B, qkv, ld, 1, dim_head, dqkv, ldq, dim_head, b_off=inner)
    gemm_raw(B, dim_head, B, heads, dP, 1, B, B * B, qkv, ld, 1, dim_head, dqkv, ldq, dim_head, c_off=inner)
    return dqkv


# --------------------------------------------------------------------------- attn_block (model.py:60-69)
# Round 6: a spot-branch layer's four weight gradients as one grouped launch, its bias gradients as another (A/B: 0 = separate).
GROUP_LAYER_GRADS = os.environ.get("MCL_GROUP_LAYER_GRADS", "1") != "0"


def _mode_of(compute):
    return _compute_mode if compute is None else compute


class AttnBlockFn(torch.autograd.Function):
    """One pre-norm Transformer layer:
        x1 = to_out(attn(LN1(x))) + x ;  x2 = W2 gelu(W1 LN2(x1) + b1) + b2 + x1
    The spot Transformer over the batch-as-sequence, model.py:66-69 (PreNorm 17, Attention 49-57, FeedForward 31-32; both
    dropouts p=0): ``bqkv`` None, one sequence.  The same arithmetic is a timm ViT block (model.py:104-116; qkv bias, LayerNorm
    eps 1e-6, one sequence per image): ``bqkv`` given, ``nseq`` = images, ``compute`` pins the GEMM mode (fp32)."""

    @staticmethod
    def forward(ctx, x, g1, be1, wqkv, wo, bo, g2, be2, w1, b1, w2, b2, heads, dim_head, bqkv=None, nseq=1, eps=LN_EPS,
                compute=None):
        with forced_compute(compute):
            x = _rowmajor(x, "x")
            u1, mean1, rstd1 = layernorm_fwd(x, g1, be1, eps)
            qkv, _ = linear_fwd(u1, wqkv, bqkv)
            o, P = attention_core_fwd(qkv, heads, dim_head, nseq)
            x1, _ = linear_fwd(o, wo, bo, resid=x)
            u2, mean2, rstd2 = layernorm_fwd(x1, g2, be2, eps)
            h, pre = linear_fwd(u2, w1, b1, gelu=True, save_pre=True)
            x2, _ = linear_fwd(h, w2, b2, resid=x1)
        ctx.save_for_backward(x, g1, wqkv, wo, g2, w1, w2, mean1, rstd1, u1, qkv, P, o, x1, mean2, rstd2, u2, pre, h)
        ctx.heads, ctx.dim_head, ctx.nseq, ctx.compute = heads, dim_head, nseq, compute
        ctx.wparams = (wqkv, wo, w1, w2)   # the Parameter objects themselves: their .grad may be written directly
        ctx.bparams = (bo, b1, b2, g1, be1, g2, be2, bqkv)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        (x, g1, wqkv, wo, g2, w1, w2, mean1, rstd1, u1, qkv, P, o, x1, mean2, rstd2, u2, pre, h) = ctx.saved_tensors
        p_qkv, p_o, p_1, p_2 = ctx.wparams
        q_bo, q_b1, q_b2, q_g1, q_be1, q_g2, q_be2, q_bqkv = ctx.bparams
        rows = x.shape[0]
        if (GROUP_LAYER_GRADS and _mode_of(ctx.compute) == COMPUTE_F32 and rows <= 1024
                and all(call("mcl_gemm_auto_ksplit", w.shape[0], w.shape[1], rows, 1) == 1 for w in (wqkv, wo, w1, w2))):
            # The spot branch (rows = one batch of spots): the data-gradient chain first, then the four weight gradients as ONE
            # grouped launch and the bias + LayerNorm parameter gradients as another -- 2 launches where they were 9 (K = rows <=
            # 255: none of them is a split-K problem; each result is bit-identical to its separate launch).
            with forced_compute(ctx.compute):
                dx2 = _rowmajor(dx2, "dx2")
                dpre = linear_bwd_data(dx2, w2, gelu_bwd_aux=pre)
                du2 = linear_bwd_data(dpre, w1)
                dx1, _, _ = layernorm_bwd(du2, x1, g2, mean2, rstd2, dx_add=dx2, dx_only=True)
                do = linear_bwd_data(dx1, wo)
                dqkv = attention_core_bwd(do, qkv, o, P, ctx.heads, ctx.dim_head, ctx.nseq)
                du1 = linear_bwd_data(dqkv, wqkv)
                dx, _, _ = layernorm_bwd(du1, x, g1, mean1, rstd1, dx_add=dx1, dx_only=True)
                probs, dws = [], []
                for dy_, x_, par in ((dx2, h, p_2), (dpre, u2, p_1), (dx1, o, p_o), (dqkv, u1, p_qkv)):
                    f, t = _wgrad_problem(_rowmajor(dy_, "dy"), x_, par, x.device)
                    probs.append(f)
                    dws.append(t)
                gemm_group(probs)
                dw2, dw1, dwo, dwqkv = dws
                items = [(dx2, q_b2), (dpre, q_b1), (dx1, q_bo)] + ([(dqkv, q_bqkv)] if q_bqkv is not None else [])
                sums, ((dg2, dbe2), (dg1, dbe1)) = colred_group(items, [(du2, x1, mean2, rstd2, (q_g2, q_be2)),
                                                                        (du1, x, mean1, rstd1, (q_g1, q_be1))])
                db2, db1, dbo = sums[:3]
                dbqkv = sums[3] if q_bqkv is not None else None
            return dx, dg1, dbe1, dwqkv, dwo, dbo, dg2, dbe2, dw1, db1, dw2, db2, None, None, dbqkv, None, None, None
        with forced_compute(ctx.compute):
            dx2 = _rowmajor(dx2, "dx2")
            # ff: x2 = h W2^T + b2 + x1
            dw2 = linear_bwd_weight(dx2, h, p_2)
            db2 = colsum(dx2, q_b2)
            dpre = linear_bwd_data(dx2, w2, gelu_bwd_aux=pre)
            dw1 = linear_bwd_weight(dpre, u2, p_1)
            db1 = colsum(dpre, q_b1)
            du2 = linear_bwd_data(dpre, w1)
            dx1, dg2, dbe2 = layernorm_bwd(du2, x1, g2, mean2, rstd2, dx_add=dx2, params=(q_g2, q_be2))
            # attn: x1 = o Wo^T + bo + x
            dwo = linear_bwd_weight(dx1, o, p_o)
            dbo = colsum(dx1, q_bo)
            do = linear_bwd_data(dx1, wo)
            dqkv = attention_core_bwd(do, qkv, o, P, ctx.heads, ctx.dim_head, ctx.nseq)
            dwqkv = linear_bwd_weight(dqkv, u1, p_qkv)
            dbqkv = colsum(dqkv, q_bqkv) if q_bqkv is not None else None
            du1 = linear_bwd_data(dqkv, wqkv)
            dx, dg1, dbe1 = layernorm_bwd(du1, x, g1, mean1, rstd1, dx_add=dx1, params=(q_g1, q_be1))
        return dx, dg1, dbe1, dwqkv, dwo, dbo, dg2, dbe2, dw1, db1, dw2, db2, None, None, dbqkv, None, None, None


class LinearFn(torch.autograd.Function):
    """y = x W^T + b over 2-D rows (the fp32 ViT's patch embedding: timm PatchEmbed's stride-p convolution is this product on
    the unfolded patches, model.py:104-116)."""

    @staticmethod
    def forward(ctx, x, w, b, compute=None):
        with forced_compute(compute):
            y, _ = linear_fwd(_rowmajor(x, "x"), w, b)
        ctx.save_for_backward(x, w)
        ctx.params = (w, b)
        ctx.compute = compute
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        pw, pb = ctx.params
        with forced_compute(ctx.compute):
            dy = _rowmajor(dy, "dy")
            dw = linear_bwd_weight(dy, x, pw)
            db = colsum(dy, pb) if pb is not None else None
            dx = linear_bwd_data(dy, w) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


# --------------------------------------------------------------------------- ProjectionHead (model.py:151-168)
# Round 6: the head as one forward launch (mcl_proj_head_fwd), one row-local backward launch (mcl_proj_head_bwd_rows) and one
# grouped launch for the three products over the batch rows (mcl_gemm_group) -- 3 launches where the epilogue-fused GEMMs + split-K
# merges + LayerNorm + column sums were 17.  fp32 compute mode and projection_dim = 256 only; MCL_FUSED_HEAD=0: the separate
# launches (A/B; same math, other summation order).
FUSED_HEAD = os.environ.get("MCL_FUSED_HEAD", "1") != "0"
HEAD_P = 256
_head_counters = {}


def _head_counter_words(owner: Tensor, n: int) -> Tensor:
    """The head kernels' arrival counters: zero before the first call, left zero by every call (csrc/proj_head.hip), one
    array per weight (two heads may run on two streams at once)."""
    key = (owner.device.index, owner.data_ptr())
    t = _head_counters.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1024), device=owner.device, dtype=torch.int32)
        call("mcl_fill_zero", t, t.numel() * 4)
        _head_counters[key] = t
    return t


def gemm_group(problems) -> None:
    """``problems``: up to four dicts of mcl_gemm_args fields (fp32, batch 1, no split-K) -> one launch."""
    n = len(problems)
    arr = (_lib.GemmArgs * n)()
    for i, kw in enumerate(problems):
        a = arr[i]
        a.struct_size = C.sizeof(_lib.GemmArgs)
        a.batch, a.alpha, a.compute = 1, 1.0, _lib.COMPUTE_F32
        for k, v in kw.items():
            setattr(a, k, v)
    call("mcl_gemm_group", arr, n)


def _fused_head_ok(x: Tensor, wp: Tensor, wf: Tensor, vecs=()) -> bool:
    return (FUSED_HEAD and _compute_mode == COMPUTE_F32 and wp.shape[0] == HEAD_P and tuple(wf.shape) == (HEAD_P, HEAD_P)
            and x.dim() == 2 and x.shape[0] > 0 and wp.stride(1) == 1 and wf.stride(1) == 1
            and all(v.is_contiguous() and v.data_ptr() % 16 == 0 for v in vecs))     # (bias / LayerNorm vectors: 16-byte loads)


def proj_head_fwd(x: Tensor, wp: Tensor, bp: Tensor, wf: Tensor, bf: Tensor, g: Tensor, be: Tensor, eps: float = LN_EPS):
    """(e, p, a, z, mean, rstd) of the projection head, one launch."""
    x = _rowmajor(x, "x")
    M, D = x.shape
    dev = x.device
    e, p, a, z = (torch.empty((M, HEAD_P), device=dev, dtype=torch.float32) for _ in range(4))
    mean = torch.empty((M,), device=dev, dtype=torch.float32)
    rstd = torch.empty((M,), device=dev, dtype=torch.float32)
    ks = int(os.environ.get("MCL_HEAD_KSPLIT", "0")) or call("mcl_proj_head_ksplit", M, D)
    ws = torch.empty(call("mcl_proj_head_ws_floats", M, ks), device=dev, dtype=torch.float32)
    cnt = _head_counter_words(wp, (M + 15) // 16 + 1)
    call("mcl_proj_head_fwd", x, x.stride(0), M, D, wp, wp.stride(0), bp, wf,
         wf.stride(0), bf, g, be, eps, e, p, a, z, mean, rstd, ws, cnt, ks)
    return e, p, a, z, mean, rstd


def proj_head_bwd_rows(de: Tensor, z: Tensor, mean: Tensor, rstd: Tensor, g: Tensor, p: Tensor, wf: Tensor, vec_params):
    """dz, dp and the four column sums (d gamma, d beta, d bf, d bp); ``vec_params`` = the four Parameters in that order: one
    that owns a dense fp32 .grad gets the sum added into it (None returned for it)."""
    de = _rowmajor(de, "de")
    M = de.shape[0]
    dev = de.device
    dz = torch.empty((M, HEAD_P), device=dev, dtype=torch.float32)
    dp = torch.empty((M, HEAD_P), device=dev, dtype=torch.float32)
    outs, ptrs, mask = [], [], 0
    for i, q in enumerate(vec_params):
        if q is not None and q.shape == (HEAD_P,) and _direct_grad_ok(q):
            outs.append(None)
            ptrs.append(q.grad.data_ptr())
            mask |= 1 << i
        else:
            t = torch.empty((HEAD_P,), device=dev, dtype=torch.float32)
            outs.append(t)
            ptrs.append(t.data_ptr())
    nrb = (M + 15) // 16
    ws = torch.empty(nrb * 4 * HEAD_P, device=dev, dtype=torch.float32)
    cnt = _head_counter_words(wf, nrb + 1)
    call("mcl_proj_head_bwd_rows", de, de.stride(0), M, z, mean, rstd, g, p, wf, wf.stride(0),
         dz, dp, ptrs[0], ptrs[1], ptrs[2], ptrs[3], mask, ws, cnt.data_ptr() + 4 * nrb)
    return dz, dp, outs


def _wgrad_problem(dy: Tensor, x: Tensor, param: Tensor, dev):
    """dW = dy^T x as a grouped-launch problem: (fields, tensor handed to autograd or None when it went into param.grad)."""
    M, N = dy.shape
    K = x.shape[1]
    f = dict(M=N, N=K, K=M, A=dy.data_ptr(), sAm=1, sAk=dy.stride(0), B=x.data_ptr(), sBk=x.stride(0), sBn=1)
    if param is not None and param.shape == (N, K) and _direct_grad_ok(param):
        f.update(C=param.grad.data_ptr(), ldc=K, flags=EPI_ACCUM)
        return f, None
    dW = torch.empty((N, K), device=dev, dtype=torch.float32)
    f.update(C=dW.data_ptr(), ldc=K)
    return f, dW


class ProjectionHeadFn(torch.autograd.Function):
    """p = x Wp^T + bp ; E = LN(gelu(p) Wf^T + bf + p)   (dropout p=0, model.py:164)."""

    @staticmethod
    def forward(ctx, x, wp, bp, wf, bf, g, be):
        x = _rowmajor(x, "x")
        ctx.fused = _fused_head_ok(x, wp, wf, (bp, bf, g, be))
        if ctx.fused:
            e, p, a, z, mean, rstd = proj_head_fwd(x, wp, bp, wf, bf, g, be)
            ctx.save_for_backward(x, wp, wf, g, p, a, z, mean, rstd)
            ctx.wparams = (wp, wf)
            ctx.bparams = (bp, bf, g, be)
            return e
        a, p = linear_fwd(x, wp, bp, gelu=True, save_pre=True)
        z, _ = linear_fwd(a, wf, bf, resid=p)
        e, mean, rstd = layernorm_fwd(z, g, be)
        ctx.save_for_backward(x, wp, wf, g, p, a, z, mean, rstd)
        ctx.wparams = (wp, wf)
        ctx.bparams = (bp, bf, g, be)
        return e

    @staticmethod
    def backward(ctx, de):
        x, wp, wf, g, p, a, z, mean, rstd = ctx.saved_tensors
        q_bp, q_bf, q_g, q_be = ctx.bparams
        if ctx.fused:
            dz, dp, (dg, dbe, dbf, dbp) = proj_head_bwd_rows(de, z, mean, rstd, g, p, wf, (q_g, q_be, q_bf, q_bp))
            f1, dwf = _wgrad_problem(dz, a, ctx.wparams[1], x.device)
            f2, dwp = _wgrad_problem(dp, x, ctx.wparams[0], x.device)
            probs, dx = [f1, f2], None
            if ctx.needs_input_grad[0]:
                dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
                probs.append(dict(M=x.shape[0], N=x.shape[1], K=HEAD_P, A=dp.data_ptr(), sAm=HEAD_P, sAk=1, B=wp.data_ptr(),
                                  sBk=wp.stride(0), sBn=1, C=dx.data_ptr(), ldc=x.shape[1]))
            gemm_group(probs)
            return dx, dwp, dbp, dwf, dbf, dg, dbe
        dz, dg, dbe = layernorm_bwd(_rowmajor(de, "de"), z, g, mean, rstd, params=(q_g, q_be))
        dwf = linear_bwd_weight(dz, a, ctx.wparams[1])
        dbf = colsum(dz, q_bf)
        dp = linear_bwd_data(dz, wf, gelu_bwd_aux=p, resid=dz)
        dwp = linear_bwd_weight(dp, x, ctx.wparams[0])
        dbp = colsum(dp, q_bp)
        dx = linear_bwd_data(dp, wp) if ctx.needs_input_grad[0] else None
        return dx, dwp, dbp, dwf, dbf, dg, dbe


# --------------------------------------------------------------------------- position embedding (model.py:230-235)
class RowSparseGrad:
    """Row-sparse gradient of an embedding table: ``rows[b]`` (B, G) is the summed gradient of table row
    ``owner_idx[b]`` where owner_idx[b] >= 0 (each touched table row appears exactly once)."""
    __slots__ = ("owner_idx", "rows")

    def __init__(self, owner_idx: Tensor, rows: Tensor):
        self.owner_idx, self.rows = owner_idx, rows

    def to_dense(self, n_rows: int) -> Tensor:
        G = self.rows.shape[1]
        dense = torch.zeros((n_rows, G), device=self.rows.device, dtype=torch.float32)
        call("mcl_embed_scatter_rows", self.owner_idx, self.rows, self.rows.stride(0), dense, G, self.rows.shape[0], G, 0)
        return dense


def embed_rowgrad(d_out: Tensor, idx: Tensor) -> RowSparseGrad:
    d_out = _rowmajor(d_out, "d_out")
    B, G = d_out.shape
    owner = torch.empty((B,), device=d_out.device, dtype=torch.int32)
    rows = torch.empty((B, G), device=d_out.device, dtype=torch.float32)
    call("mcl_embed_rowgrad", d_out, d_out.stride(0), idx, owner, rows, G, B, G)
    return RowSparseGrad(owner, rows)


# Device-side error words.  The kernels never raise in the middle of an enqueue-only step: a position outside [0, table rows)
# is clamped and flagged (word 0: nn.Embedding would raise IndexError), a persistent dense-block launch that gave up waiting at
# a BatchNorm seam flags word 1 (its results are invalid: csrc/dense_block.hip).  ``check_device_errors`` turns the words into
# exceptions at a point where the host synchronises anyway (train() does it with the loss.item() of its meter, TrainStep polls
# them without a sync); SURVEY 8(b): no exceptions cross the ABI, the Python wrapper raises.
ERR_POSITION, ERR_BLOCK_SEAM, _ERR_WORDS = 0, 1, 4
_err_words = {}


class SeamTimeoutError(RuntimeError):
    """A persistent dense-block kernel timed out at a BatchNorm seam: that step's activations / gradients are invalid."""


def device_error_words(device) -> Tensor:
    t = _err_words.get(device.index)
    if t is None:
        t = torch.zeros(_ERR_WORDS, device=device, dtype=torch.int32)
        _err_words[device.index] = t
    return t


def position_error_flag(device) -> Tensor:
    return device_error_words(device)[ERR_POSITION:ERR_POSITION + 1]


def block_seam_error_flag(device) -> Tensor:
    return device_error_words(device)[ERR_BLOCK_SEAM:ERR_BLOCK_SEAM + 1]


def raise_for_error_words(words, clear=None) -> None:
    """``words``: the host copy of a device's error words; ``clear``: called before raising (resets the device words)."""
    if not any(words):
        return
    if clear is not None:
        clear()
    if words[ERR_BLOCK_SEAM]:
        raise SeamTimeoutError(
            "a persistent dense-block launch (csrc/dense_block.hip) timed out waiting for the other images' BatchNorm records: "
            "its workgroups were not co-resident (GPU shared with another process, CU masking, a long concurrent kernel). "
            "The step that contained it produced invalid activations and gradients -- discard it; MCL_BLOCK_PERSIST=0 / "
            "MCL_BLOCK_PERSIST_BWD=0 select the per-layer kernels")
    if words[ERR_POSITION]:
        raise IndexError("index out of range in self: a batch held a position outside [0, 65536) "
                         "(the reference's nn.Embedding raises here, model.py:232-233)")


def check_device_errors(device=None) -> None:
    """Raises IndexError (a position outside the tables) / SeamTimeoutError (a persistent dense-block seam timed out) if any
    step since the last check flagged one (host sync)."""
    for idx, t in list(_err_words.items()):
        if device is not None and device.index != idx:
            continue
        raise_for_error_words(t.tolist(), t.zero_)


check_position_errors = check_device_errors      # the name train.py has used since round 1


class PosEmbedAddFn(torch.autograd.Function):
    """out = expr + x_table[pos[:,0].long()] + y_table[pos[:,1].long()].

    Backward never builds the reference's dense (65536, G) gradients unless asked: with
    ``sparse_sink`` (a dict) the upstream gradient and the two index vectors are handed over as
    ``sink['dout'|'ix'|'iy']`` for the fused table optimizer (which reduces them to touched rows) and
    the tables receive no ``.grad``; without it dense gradients are returned (stock-optimizer
    compatible)."""

    @staticmethod
    def forward(ctx, expr, pos, x_table, y_table, sparse_sink):
        expr = _rowmajor(expr, "expression")
        B, G = expr.shape
        if pos.is_cuda and pos.dtype != torch.float32:
            pos = pos.to(torch.float32)              # integer grid / pixel coordinates (nn.Embedding takes .long())
        pos = _chk(pos, "position").contiguous()
        if pos.shape != (B, 2):
            raise RuntimeError(f"position must be ({B}, 2), got {tuple(pos.shape)}")
        xt, yt = _chk(x_table, "x_embed.weight"), _chk(y_table, "y_embed.weight")
        assert xt.is_contiguous() and yt.is_contiguous() and xt.shape == yt.shape and xt.shape[1] == G
        out = torch.empty((B, G), device=expr.device, dtype=torch.float32)
        ix = torch.empty((B,), device=expr.device, dtype=torch.int32)
        iy = torch.empty((B,), device=expr.device, dtype=torch.int32)
        call("mcl_pos_embed_add_fwd", expr, expr.stride(0), pos, xt, yt, G,
             xt.shape[0], out, G, ix, iy, position_error_flag(expr.device), B, G)
        ctx.save_for_backward(ix, iy)
        ctx.n_rows = xt.shape[0]
        ctx.sink = sparse_sink
        return out

    @staticmethod
    def backward(ctx, dout):
        ix, iy = ctx.saved_tensors
        d_expr = dout if ctx.needs_input_grad[0] else None
        if ctx.sink is not None:
            # both tables share the same upstream gradient; the optimizer (or its data-parallel
            # exchange) reduces it to touched rows
            ctx.sink["dout"], ctx.sink["ix"], ctx.sink["iy"] = _rowmajor(dout, "dout"), ix, iy
            from . import densenet_fused as _dn
            _dn.stamp("spot backward done (its stream)")
            hook = ctx.sink.get("hook")
            if hook is not None:
                hook()          # FusedAdam._early_tables: update both tables now, on this (spot-branch) stream
                _dn.stamp("position tables updated (spot stream)")
            return d_expr, None, None, None, None
        gx = embed_rowgrad(dout, ix)
        gy = embed_rowgrad(dout, iy)
        return d_expr, None, gx.to_dense(ctx.n_rows), gy.to_dense(ctx.n_rows), None


# --------------------------------------------------------------------------- InfoNCE (model.py:242-247)
def infonce_fwd_bwd(e_spot: Tensor, e_img: Tensor, temperature: float, want_logits: bool = True
                    ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Single-device symmetric InfoNCE: returns (loss 0-d, dE_spot, dE_img, logits)."""
    es, ei = _rowmajor(e_spot, "spot_embeddings"), _rowmajor(e_img, "image_embeddings")
    B, P = es.shape
    assert ei.shape == (B, P)
    dev = es.device
    S = torch.empty((B, B), device=dev, dtype=torch.float32)
    gemm_raw(B, B, P, 1, es, es.stride(0), 1, 0, ei, 1, ei.stride(0), 0, S, B, 0, alpha=1.0 / temperature)
    lse = torch.empty((2, B), device=dev, dtype=torch.float32)
    call("mcl_infonce_lse", S, B, B, B, lse[0], lse[1])
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("mcl_infonce_loss_mean", S, B, lse[0], lse[1], B, 2.0 * B, loss)
    dS = torch.empty_like(S)
    call("mcl_infonce_dlogits", S, B, lse[0], lse[1], B, B, 0, 0, 1.0 / (2.0 * B * temperature), dS, B)
    d_es = torch.empty_like(es)
    d_ei = torch.empty_like(ei)
    if _compute_mode == COMPUTE_F32 and (not SPLIT_K or call("mcl_gemm_auto_ksplit", B, P, B, 1) == 1):
        # both gradient products as one launch (on the step's critical chain between loss and backward); bit-identical
        gemm_group([dict(M=B, N=P, K=B, A=dS.data_ptr(), sAm=B, sAk=1, B=ei.data_ptr(), sBk=ei.stride(0), sBn=1,
                         C=d_es.data_ptr(), ldc=P),                                # dE_s = dS E_i
                    dict(M=B, N=P, K=B, A=dS.data_ptr(), sAm=1, sAk=B, B=es.data_ptr(), sBk=es.stride(0), sBn=1,
                         C=d_ei.data_ptr(), ldc=P)])                               # dE_i = dS^T E_s
    else:
        gemm_raw(B, P, B, 1, dS, B, 1, 0, ei, ei.stride(0), 1, 0, d_es, P, 0)          # dE_s = dS E_i
        gemm_raw(B, P, B, 1, dS, 1, B, 0, es, es.stride(0), 1, 0, d_ei, P, 0)          # dE_i = dS^T E_s
    return loss, d_es, d_ei, (S if want_logits else None)


# --------------------------------------------------------------------------- fused InfoNCE (bf16 MFMA, no logits in HBM)
FUSED_DIM = 256
_fused_ws = {}


def _fused_workspace(R: int, C: int, device) -> Tensor:
    need = call("mcl_infonce_fused_workspace_bytes", R, C, FUSED_DIM)
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    w = _fused_ws.get(key)
    if w is None or w.numel() < need:
        w = torch.empty(max(int(need), 1 << 20), device=device, dtype=torch.uint8)
        _fused_ws[key] = w
    return w


def cast_bf16(x: Tensor) -> Tensor:
    """fp32 (rows, cols) -> contiguous bf16 copy (round to nearest even) on the HIP cast kernel."""
    x = _rowmajor(x, "x")
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    call("mcl_cast_f32_to_bf16", x, x.stride(0), y, y.stride(0), x.shape[0], x.shape[1])
    return y


def _bf16_rows(t: Tensor, name: str) -> Tensor:
    """2-D bf16 GPU tensor with unit column stride (a row stride is allowed: column slices of a wider buffer)."""
    if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or \
            t.data_ptr() % 16:
        raise RuntimeError(f"{name}: expected a 2-D bf16 GPU tensor with unit column stride, 16-byte aligned rows")
    if t.shape[1] != FUSED_DIM:
        raise RuntimeError(f"{name}: the fused InfoNCE kernel is built for projection_dim {FUSED_DIM}, "
                           f"got {t.shape[1]}")
    return t


def infonce_fused_lse(a16: Tensor, b16: Tensor, inv_t: float, diag_off: int = 0) -> Tuple[Tensor, Tensor]:
    """(lse (R,), diag (R,)) of S = a b^T * inv_t without materialising S (csrc/infonce_fused.hip)."""
    a16, b16 = _bf16_rows(a16, "a"), _bf16_rows(b16, "b")
    R, Cn = a16.shape[0], b16.shape[0]
    lse = torch.empty((R,), device=a16.device, dtype=torch.float32)
    diag = torch.zeros((R,), device=a16.device, dtype=torch.float32)
    ws = _fused_workspace(R, Cn, a16.device)
    call("mcl_infonce_fused_lse", a16, a16.stride(0), b16, b16.stride(0),
         R, Cn, FUSED_DIM, diag_off, inv_t, lse, diag, ws, ws.numel())
    return lse, diag


def infonce_fused_grad(a16: Tensor, b16: Tensor, inv_t: float, lse_a: Tensor, lse_b: Tensor, coef: float,
                       diag_off: int = 0) -> Tensor:
    """dA (R, 256) fp32 = coef * sum_c (exp(S-lse_a[r]) + exp(S-lse_b[c]) - 2[c == r+diag_off]) b[c]."""
    a16, b16 = _bf16_rows(a16, "a"), _bf16_rows(b16, "b")
    R, Cn = a16.shape[0], b16.shape[0]
    assert lse_a.shape == (R,) and lse_b.shape == (Cn,) and lse_a.is_contiguous() and lse_b.is_contiguous()
    dA = torch.empty((R, FUSED_DIM), device=a16.device, dtype=torch.float32)
    ws = _fused_workspace(R, Cn, a16.device)
    call("mcl_infonce_fused_grad", a16, a16.stride(0), b16, b16.stride(0), R, Cn,
         FUSED_DIM, diag_off, inv_t, _chk(lse_a), _chk(lse_b), coef, dA, ws, ws.numel())
    return dA


# Below this batch the flash-style kernels are launch-bound (12 small launches, 0.15 ms at B = 128 .. 1024) and the
# exact fp32 path (5 launches on a B x B matrix that fits L2) is faster AND more accurate: 0.083 ms at B = 128
# (profiles/r02_infonce_microbench.jsonl).  "fused" therefore means "never materialise the logits where that pays".
FUSED_MIN_BATCH = int(os.environ.get("MCL_FUSED_MIN_BATCH", "1024"))


def infonce_fused_fwd_bwd(e_spot: Tensor, e_img: Tensor, temperature: float, min_fused_batch: Optional[int] = None
                          ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Single-device symmetric InfoNCE on the fused bf16 kernels: (loss, dE_spot, dE_img, None).  Same closed
    form as ``infonce_fwd_bwd``; the embeddings are rounded to bf16 once, logits never reach HBM.  Batches below
    ``min_fused_batch`` (default FUSED_MIN_BATCH) take the exact fp32 kernels instead."""
    if e_spot.shape[0] < (FUSED_MIN_BATCH if min_fused_batch is None else min_fused_batch):
        loss, d_es, d_ei, _ = infonce_fwd_bwd(e_spot, e_img, temperature, want_logits=False)
        return loss, d_es, d_ei, None
    es16, ei16 = cast_bf16(e_spot), cast_bf16(e_img)
    B = es16.shape[0]
    inv_t = 1.0 / temperature
    rl, diag = infonce_fused_lse(es16, ei16, inv_t)
    cl, _ = infonce_fused_lse(ei16, es16, inv_t)
    loss = ((rl - diag).sum() + (cl - diag).sum()) / (2.0 * B)
    coef = inv_t / (2.0 * B)
    d_es = infonce_fused_grad(es16, ei16, inv_t, rl, cl, coef)
    d_ei = infonce_fused_grad(ei16, es16, inv_t, cl, rl, coef)
    return loss, d_es, d_ei, None


# --------------------------------------------------------------------------- fp8 similarity contraction (configs[4])
FP8_ROW = FUSED_DIM + 16        # packed row: 256 e4m3 bytes + the E8M0 scale byte, padded to a 16-byte multiple


def quant_e4m3(x: Tensor, want_deq: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """fp32 (rows, 256) -> (packed uint8 (rows, 272): e4m3 bytes [:256] + scale byte [256], bf16 dequantised copy).
    One power-of-two scale per row (csrc/infonce_fp8.hip); the dequantised values are exactly representable in bf16."""
    x = _rowmajor(x, "x")
    rows, cols = x.shape
    if cols != FUSED_DIM:
        raise RuntimeError(f"the fp8 InfoNCE kernels are built for projection_dim {FUSED_DIM}, got {cols}")
    packed = torch.zeros((rows, FP8_ROW), device=x.device, dtype=torch.uint8)
    deq = torch.empty((rows, cols), device=x.device, dtype=torch.bfloat16) if want_deq else None
    call("mcl_quant_e4m3_rows", x, x.stride(0), rows, cols, packed, FP8_ROW,
         packed.data_ptr() + FUSED_DIM, FP8_ROW, deq, cols if want_deq else 0)
    return packed, deq


def _fp8_rows(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or t.shape[1] != FP8_ROW or \
            t.stride(0) % 16 or t.data_ptr() % 16:
        raise RuntimeError(f"{name}: expected packed e4m3 rows (uint8, {FP8_ROW} columns, 16-byte aligned rows)")
    return t


def dequant_e4m3(packed: Tensor) -> Tensor:
    packed = _fp8_rows(packed, "packed")
    rows = packed.shape[0]
    deq = torch.empty((rows, FUSED_DIM), device=packed.device, dtype=torch.bfloat16)
    call("mcl_dequant_e4m3_rows", packed, packed.stride(0), packed.data_ptr() + FUSED_DIM,
         packed.stride(0), rows, FUSED_DIM, deq, FUSED_DIM)
    return deq


def infonce_fp8_lse(a8: Tensor, b8: Tensor, inv_t: float) -> Tensor:
    """lse (R,) of S = dequant(a8) dequant(b8)^T * inv_t on the fp8 MFMA (hardware block scales), S never in HBM."""
    a8, b8 = _fp8_rows(a8, "a8"), _fp8_rows(b8, "b8")
    R, Cn = a8.shape[0], b8.shape[0]
    need = call("mcl_infonce_fp8_workspace_bytes", R, Cn)
    ws = _fused_workspace(R, Cn, a8.device)
    if ws.numel() < need:
        ws = torch.empty(int(need), device=a8.device, dtype=torch.uint8)
    lse = torch.empty((R,), device=a8.device, dtype=torch.float32)
    call("mcl_infonce_fp8_lse", a8, a8.stride(0), a8.data_ptr() + FUSED_DIM, a8.stride(0), b8, b8.stride(0),
         b8.data_ptr() + FUSED_DIM, b8.stride(0), R, Cn, FUSED_DIM, inv_t, lse, ws, ws.numel())
    return lse


def infonce_rowdot(a16: Tensor, b16: Tensor, inv_t: float, diag_off: int = 0) -> Tensor:
    a16, b16 = _bf16_rows(a16, "a"), _bf16_rows(b16, "b")
    R, Cn = a16.shape[0], b16.shape[0]
    diag = torch.zeros((R,), device=a16.device, dtype=torch.float32)
    call("mcl_infonce_rowdot_bf16", a16, a16.stride(0), b16, b16.stride(0), R, Cn, FUSED_DIM, diag_off, inv_t, diag)
    return diag


def infonce_fp8_fwd_bwd(e_spot: Tensor, e_img: Tensor, temperature: float
                        ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Symmetric InfoNCE with the similarity contraction on e4m3 operands (per-row power-of-two scales): the row and
    column LSEs come from the fp8 MFMA kernel; the closed-form gradient runs the bf16 strip kernel on the dequantised
    embeddings, which are bit-exact bf16 images of the fp8 operands (so the probabilities it forms are normalised by
    exactly these LSEs).  Returns (loss, dE_spot, dE_img, None)."""
    s8, s16 = quant_e4m3(e_spot)
    i8, i16 = quant_e4m3(e_img)
    B = s8.shape[0]
    inv_t = 1.0 / temperature
    rl = infonce_fp8_lse(s8, i8, inv_t)
    cl = infonce_fp8_lse(i8, s8, inv_t)
    diag = infonce_rowdot(s16, i16, inv_t)
    loss = ((rl - diag).sum() + (cl - diag).sum()) / (2.0 * B)
    coef = inv_t / (2.0 * B)
    d_es = infonce_fused_grad(s16, i16, inv_t, rl, cl, coef)
    d_ei = infonce_fused_grad(i16, s16, inv_t, cl, rl, coef)
    return loss, d_es, d_ei, None


class InfoNCEFn(torch.autograd.Function):
    """loss = 0.5*[CE(S, I) + CE(S^T, I)], S = E_spot E_img^T / T.  Forward and backward are computed
    together (closed-form dS from the two LSE vectors); autograd's backward only scales by grad_output."""

    @staticmethod
    def forward(ctx, e_spot, e_img, temperature, stash, fused=False):
        if fused == "fp8":
            loss, d_es, d_ei, S = infonce_fp8_fwd_bwd(e_spot, e_img, temperature)
        elif fused:
            loss, d_es, d_ei, S = infonce_fused_fwd_bwd(e_spot, e_img, temperature)
        else:
            loss, d_es, d_ei, S = infonce_fwd_bwd(e_spot, e_img, temperature, want_logits=stash is not None)
        if stash is not None:
            stash["logits"] = S
        ctx.save_for_backward(d_es, d_ei)
        return loss

    @staticmethod
    def backward(ctx, gl):
        d_es, d_ei = ctx.saved_tensors
        ya, yb = scale_pair(d_es, d_ei, gl)
        return ya, yb, None, None, None


# --------------------------------------------------------------------------- dropout > 0 path (model.py:25-29,156,164-165)
_dropout_calls = 0


class DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in training mode on an own kernel (csrc/step_misc.hip): mask from a counter-based generator seeded by
    torch's seed and a per-call counter (reproducible under torch.manual_seed), one byte per element kept for the backward."""

    @staticmethod
    def forward(ctx, x, p):
        global _dropout_calls
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mclstexp_amd: dropout > 0 inside a HIP-graph capture would replay ONE frozen mask; run the "
                               "dropout > 0 configuration eagerly (engine.TrainStep(graphs=False))")
        x = _chk(x, "dropout input").contiguous()
        y = torch.empty_like(x)
        mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        _dropout_calls += 1
        seed = (torch.initial_seed() * 0x9E3779B1 + _dropout_calls) & 0xFFFFFFFFFFFFFFFF
        call("mcl_dropout_fwd", x, y, mask, x.numel(), float(p), seed)
        ctx.save_for_backward(mask)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("mcl_dropout_bwd", dy, mask, dx, dy.numel(), ctx.p)
        return dx, None


def gelu_bwd(dy: Tensor, pre: Tensor) -> Tensor:
    """dy * gelu'(pre) (exact erf form) in one own launch."""
    dy, pre = dy.contiguous(), pre.contiguous()
    out = torch.empty_like(dy)
    call("mcl_gelu_f32", pre, dy, out, dy.numel())
    return out


class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "gelu input").contiguous()
        y = torch.empty_like(x)
        call("mcl_gelu_f32", x, None, y, x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return gelu_bwd(dy, x)


class AddFn(torch.autograd.Function):
    """a + b (a residual join) as an own launch; the gradient passes through to both."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _chk(a, "a").contiguous(), _chk(b, "b").contiguous()
        assert a.shape == b.shape
        y = torch.empty_like(a)
        call("mcl_add_f32", a, b, y, a.numel())
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


# --------------------------------------------------------------------------- BLEEP soft-target CLIP loss (§8 f4)
def soft_clip_fwd_bwd(e_spot: Tensor, e_img: Tensor, temperature: float, targets_times_temperature: bool = False
                      ) -> Tuple[Tensor, Tensor, Tensor]:
    """(loss, dE_spot, dE_img) of the reference baseline's soft-target contrastive loss
    (/root/reference/baselines/Bleep/models.py:34-43, 66-76, 228-234), forward and backward in closed form on the
    same kernels as the exact InfoNCE path (fp32 MFMA GEMMs, row-softmax, row/column LSE); gradients flow through the
    soft targets as in the reference.

        S = E_s E_i^T / T,  Tg = softmax_rows(k (E_i E_i^T + E_s E_s^T)/2),  k = 1/T (CLIPModel) or T (CLIPModel_ViT)
        loss = -(1/2B) sum_ij Tg_ij (logsoftmax_row(S) + logsoftmax_col(S))_ij
    """
    es, ei = _rowmajor(e_spot, "spot_embeddings"), _rowmajor(e_img, "image_embeddings")
    B, P = es.shape
    assert ei.shape == (B, P)
    dev = es.device
    inv_t = 1.0 / temperature
    k = temperature if targets_times_temperature else inv_t
    S = torch.empty((B, B), device=dev, dtype=torch.float32)
    gemm_raw(B, B, P, 1, es, es.stride(0), 1, 0, ei, 1, ei.stride(0), 0, S, B, 0, alpha=inv_t, compute=COMPUTE_F32)
    Tg = torch.empty((B, B), device=dev, dtype=torch.float32)
    gemm_raw(B, B, P, 1, ei, ei.stride(0), 1, 0, ei, 1, ei.stride(0), 0, Tg, B, 0, alpha=0.5, compute=COMPUTE_F32)
    gemm_raw(B, B, P, 1, es, es.stride(0), 1, 0, es, 1, es.stride(0), 0, Tg, B, 0, alpha=0.5, flags=EPI_ACCUM,
             compute=COMPUTE_F32)
    call("mcl_softmax_rows_fwd", Tg, B, B, B, k)      # Tg in place
    lse = torch.empty((2, B), device=dev, dtype=torch.float32)
    call("mcl_infonce_lse", S, B, B, B, lse[0], lse[1])
    c = 1.0 / (2.0 * B)
    # the elementwise middle in one pass (csrc/soft_clip.hip): loss partials, dS, d loss / d Tg
    tcol = colsum(Tg)
    dS = torch.empty((B, B), device=dev, dtype=torch.float32)
    dA = torch.empty((B, B), device=dev, dtype=torch.float32)
    loss_rows = torch.empty((B, 1), device=dev, dtype=torch.float32)
    call("mcl_soft_clip_mid", S, Tg, lse[0], lse[1], tcol, B, c, dS, dA, loss_rows)
    loss = colsum(loss_rows)[0]
    # backward through the soft targets
    call("mcl_softmax_rows_bwd", Tg, dA, B, B, B, k)
    dsym = torch.empty((B, B), device=dev, dtype=torch.float32)  # A = (II + SS)/2 and both Gram matrices are symmetric
    call("mcl_symmetrize", dA, B, dsym)
    d_es = torch.empty_like(es)
    d_ei = torch.empty_like(ei)
    gemm_raw(B, P, B, 1, dS, B, 1, 0, ei, ei.stride(0), 1, 0, d_es, P, 0, alpha=inv_t, compute=COMPUTE_F32)
    gemm_raw(B, P, B, 1, dsym, B, 1, 0, es, es.stride(0), 1, 0, d_es, P, 0, flags=EPI_ACCUM, compute=COMPUTE_F32)
    gemm_raw(B, P, B, 1, dS, 1, B, 0, es, es.stride(0), 1, 0, d_ei, P, 0, alpha=inv_t, compute=COMPUTE_F32)
    gemm_raw(B, P, B, 1, dsym, B, 1, 0, ei, ei.stride(0), 1, 0, d_ei, P, 0, flags=EPI_ACCUM, compute=COMPUTE_F32)
    return loss, d_es, d_ei


def scale_pair(d_es: Tensor, d_ei: Tensor, gl: Tensor) -> Tuple[Tensor, Tensor]:
    """(d_es * gl, d_ei * gl) for autograd's upstream scalar ``gl`` (a DEVICE value: no host read) -- both embedding gradients in
    ONE own launch (mcl_scale2_f32); anything else (a host scalar, a non-fp32 gradient) is not a training-step shape and raises."""
    if not (gl.is_cuda and gl.numel() == 1 and d_es.dtype == d_ei.dtype == torch.float32):
        raise RuntimeError("loss backward: expected a one-element device gradient and fp32 embedding gradients")
    gl = gl.reshape(1).to(torch.float32)            # (no launch for the fp32 scalar autograd hands over)
    d_es, d_ei = d_es.contiguous(), d_ei.contiguous()
    ya, yb = torch.empty_like(d_es), torch.empty_like(d_ei)
    call("mcl_scale2_f32", d_es, d_es.numel(), d_ei, d_ei.numel(), gl, ya, yb)
    return ya, yb


class SoftClipLossFn(torch.autograd.Function):
    """loss = soft-target CLIP loss of (spot_embeddings, image_embeddings); backward from the closed form."""

    @staticmethod
    def forward(ctx, e_spot, e_img, temperature, targets_times_temperature):
        loss, d_es, d_ei = soft_clip_fwd_bwd(e_spot.detach(), e_img.detach(), temperature, targets_times_temperature)
        ctx.save_for_backward(d_es, d_ei)
        return loss

    @staticmethod
    def backward(ctx, g):
        d_es, d_ei = ctx.saved_tensors
        ya, yb = scale_pair(d_es, d_ei, g)          # own kernel (was two ATen multiplies: VERDICT r05 weak #12)
        return ya, yb, None, None
