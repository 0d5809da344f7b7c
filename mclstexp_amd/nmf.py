"""Expression as gene programs on the MI355X: ``X ~ W H`` with ``W, H >= 0`` -- the unsupervised factorisation of the
(spots, genes) matrix into programs (the rows of H) and their usage per spot (W), for every slide and every start of a
call at once, and the number the feature exists for: does the predicted expression use the same programs, in the same
spots, as the measured expression (``program_recovery``)?

The arithmetic is scikit-learn's ``non_negative_factorization(solver="mu")`` for ``beta_loss="frobenius"`` and
``"kullback-leibler"``, stated in DESIGN 6.24 and restated in numpy by ``tests/nmf_reference.py``, which is pinned to
scikit-learn.  The rules:

* fp64 throughout (``x`` may be fp32: converted on load); no floating-point atomics; every sum runs in an order that
  depends on the segment's rows, G and k alone.  A segment's factors are bit-identical alone and inside a stacked call, a
  start's alone and beside other starts, run to run.
* A problem is one row segment of the row-stacked ``x`` (``offsets``; ``None``: one pooled problem) times one start.  Per
  iteration W is updated first, then H from the new W.  Every 10th iteration the error ``sqrt(2 D(X | WH))`` is summed
  from X itself and a problem stops where ``(previous - error) / error_at_init < tol``: the decision is taken on the
  device, a stopped problem is frozen, and the host reads one word per problem.  ``tol = 0`` runs ``max_iter`` iterations
  without a read.
* ``init="random"`` is scikit-learn's (``avg * |standard_normal|`` from ``RandomState(seed + start)``, H drawn before W,
  ``avg = sqrt(mean of the segment / k)``), drawn on the host; ``init=(W0, H0)`` is a custom start.  The ``nndsvd``
  initialisations, regularisation, other beta and the coordinate-descent solver are not built.
* A negative or non-finite ``x`` raises a ``ValueError`` naming the row, ahead of the first update.
* 1 <= k <= 64, G <= 16384, segments x starts <= 65535, rows k < 2^31: ``ValueError`` before a launch.

``res["programs"]`` (per segment (k, G), every row summing to 1) is a signature matrix that ``deconv.nnls`` accepts as it
is.  No CPU fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.nmf --pred P1.npy ... [--true T1.npy ...] [--k K] [--beta_loss frobenius|kullback-leibler]
                               [--n_init 4] [--genes names.npy] [--top 10] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_int, cumulative_offsets, dense, device, empty, load_gene_major,
                      matrix, nanmean, paired_offsets, stack_rows, upload, validate_offsets)
from ._lib import call

MAX_K = 64               # csrc/nmf.hip: four MFMA tiles of components
MAX_GENES = 16384
MAX_PROBLEMS = 65535     # segments x starts: a grid dimension
MAX_CELLS = (1 << 31) - 1
LOSSES = {"frobenius": 0, "kullback-leibler": 1}
CHECK_EVERY = 10
OUT_FILE = "nmf.npz"
TOP_N = 10
KEYS = ("W", "H", "err", "n_iter", "converged", "best_start", "programs", "usage", "dominant")
Init = Union[str, Tuple[ArrayLike, ArrayLike]]


# ------------------------------------------------------------------------------------------------------- host rules
def check_problem(x_shape: Sequence[int], k: int, offsets=None, n_init: int = 1, beta_loss: str = "frobenius",
                  max_iter: int = 200, tol: float = 1e-4, ld: Optional[int] = None,
                  n_genes: Optional[int] = None) -> Tuple[int, int, np.ndarray]:
    """The limits and arguments, checked on the host before the GPU is touched.  Returns (rows, G, offsets)."""
    if beta_loss not in LOSSES:
        raise ValueError(f"beta_loss must be one of {sorted(LOSSES)}, got {beta_loss!r}")
    k = check_int(k, "k", 1, MAX_K)
    n_init = check_int(n_init, "n_init", 1, MAX_PROBLEMS)
    check_int(max_iter, "max_iter", 1)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating, np.integer)) or not (0 <= tol < np.inf):
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")
    if len(x_shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(x_shape)}")
    rows, width = int(x_shape[0]), int(x_shape[1])
    if ld is None:
        if n_genes is not None and int(n_genes) != width:
            raise ValueError(f"x: {width} columns, n_genes = {n_genes}; give ld for a padded matrix")
        G = width
    else:
        if n_genes is None:
            raise ValueError("ld needs n_genes: x is (rows, ld) and its first n_genes columns are the genes")
        G = check_int(n_genes, "n_genes", 1)
        ld = check_int(ld, "ld", G)
        if width != ld:
            raise ValueError(f"x: expected (rows, {ld}) for ld = {ld}, got {tuple(x_shape)}")
    if G < 1 or G > MAX_GENES:
        raise ValueError(f"x: {G} genes; the kernels handle 1 .. {MAX_GENES}")
    if rows < 1:
        raise ValueError("x: no spot")
    if rows * k > MAX_CELLS:
        raise ValueError(f"x: {rows} spots x {k} components; at most {MAX_CELLS} usages per start")
    off = validate_offsets(offsets, rows, 1, none_is_one=True)
    if (off.size - 1) * n_init > MAX_PROBLEMS:
        raise ValueError(f"{off.size - 1} segments x {n_init} starts; at most {MAX_PROBLEMS} problems per call")
    return rows, G, off


def random_init(x: np.ndarray, k: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """scikit-learn's ``init="random"`` start (W0, H0) of one (rows, G) matrix, bit for bit: H is drawn first."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    avg = np.sqrt(x.mean() / k)
    rng = np.random.RandomState(seed)
    H = avg * rng.standard_normal(size=(k, x.shape[1]))
    W = avg * rng.standard_normal(size=(x.shape[0], k))
    np.abs(H, out=H)
    np.abs(W, out=W)
    return W, H


def _shape(a) -> Tuple[int, ...]:
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def custom_init(init, rows: int, G: int, k: int, S: int, n_init: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``init=(W0, H0)`` as (W (n, rows, k), H (S, n, k, G), n): W0 is (rows, k) or (n, rows, k); H0 is (k, G) for one
    segment and one start, (S, k, G) for one start, (n, k, G) for one segment, or (n, S, k, G)."""
    if not isinstance(init, (tuple, list)) or len(init) != 2:
        raise ValueError("init must be 'random' or a pair (W0, H0)")
    W0 = np.asarray(init[0].cpu() if isinstance(init[0], Tensor) else init[0], dtype=np.float64)
    H0 = np.asarray(init[1].cpu() if isinstance(init[1], Tensor) else init[1], dtype=np.float64)
    if W0.ndim == 2:
        W0 = W0[None]
    if W0.ndim != 3 or W0.shape[1:] != (rows, k):
        raise ValueError(f"init: W0 must be ({rows}, {k}) or (n_init, {rows}, {k}), got {_shape(init[0])}")
    n = int(W0.shape[0])
    if n_init not in (1, n):
        raise ValueError(f"init: W0 holds {n} starts, n_init = {n_init}")
    if H0.ndim == 2 and S == 1 and n == 1:
        H0 = H0[None, None]
    elif H0.ndim == 3 and n == 1 and H0.shape[0] == S:
        H0 = H0[:, None]
    elif H0.ndim == 3 and S == 1 and H0.shape[0] == n:
        H0 = H0[None]
    elif H0.ndim == 4:
        H0 = np.swapaxes(H0, 0, 1)
    if H0.ndim != 4 or H0.shape != (S, n, k, G):
        raise ValueError(f"init: H0 must hold ({k}, {G}) per segment ({S}) and start ({n}), got {_shape(init[1])}")
    if not (np.isfinite(W0).all() and np.isfinite(H0).all() and (W0 >= 0).all() and (H0 >= 0).all()):
        raise ValueError("init: W0 and H0 must be finite and non-negative")
    return np.ascontiguousarray(W0), np.ascontiguousarray(H0), n


def match_programs(a: np.ndarray, b: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Programs matched greedily on cosine similarity: the largest cell first (ties: the smaller (row, column)), its row
    and column leave.  ``a`` (ka, G), ``b`` (kb, G).  Returns ((m, 2) pairs (row of a, row of b) in the order taken, their
    cosines); a zero program has cosine 0 with everything and is matched last."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.sqrt((a * a).sum(axis=1)), np.sqrt((b * b).sum(axis=1))
    cos = (a @ b.T) / np.where(na > 0, na, 1.0)[:, None] / np.where(nb > 0, nb, 1.0)[None, :]
    t = cos.copy()
    pairs, vals = [], []
    for _ in range(min(t.shape)):
        r, c = divmod(int(np.argmax(t)), t.shape[1])
        pairs.append((r, c))
        vals.append(cos[r, c])
        t[r, :] = -np.inf
        t[:, c] = -np.inf
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(vals, dtype=np.float64)


def top_indices(v: np.ndarray, n: int) -> np.ndarray:
    """The ``n`` indices of ``v`` by descending value (ties: the smaller index)."""
    v = np.asarray(v, dtype=np.float64)
    return np.lexsort((np.arange(v.size), -v))[:max(0, int(n))].astype(np.int64)


def top_gene_overlap(a: np.ndarray, b: np.ndarray, pairs: np.ndarray, n_top: int) -> Tuple[np.ndarray, np.ndarray]:
    """(overlap, Jaccard index) of the ``n_top`` genes of every matched pair of programs."""
    over, jac = [], []
    for r, c in pairs:
        ta, tb = set(top_indices(a[r], n_top).tolist()), set(top_indices(b[c], n_top).tolist())
        over.append(len(ta & tb))
        jac.append(len(ta & tb) / max(1, len(ta | tb)))
    return np.asarray(over, dtype=np.int64), np.asarray(jac, dtype=np.float64)


def column_pearson(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Pearson r of every column pair of two (n, k) arrays; NaN where a column is constant or n < 2."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape[0] < 2:
        return np.full(a.shape[1], np.nan)
    da, db = a - a.mean(axis=0), b - b.mean(axis=0)
    den = np.sqrt((da * da).sum(axis=0) * (db * db).sum(axis=0))
    with np.errstate(all="ignore"):
        return np.where(den > 0, (da * db).sum(axis=0) / den, np.nan)


def usage_scores(up: np.ndarray, ut: np.ndarray, dp: np.ndarray, dt: np.ndarray, offsets: np.ndarray) -> Dict[str, object]:
    """Predicted against measured usage under the same programs: ``pearson`` (slides, k) and ``pearson_pooled`` (k,) over the
    spots, ``dominant_agreement`` (slides,) and ``dominant_agreement_pooled``, the share of spots with the same dominant
    program."""
    S = int(offsets.size - 1)
    sl = [slice(int(offsets[s]), int(offsets[s + 1])) for s in range(S)]
    pearson = np.stack([column_pearson(up[c], ut[c]) for c in sl])
    agree = np.array([float((dp[c] == dt[c]).mean()) for c in sl])
    return {"pearson": pearson, "pearson_pooled": column_pearson(up, ut), "dominant_agreement": agree,
            "dominant_agreement_pooled": float((dp == dt).mean()), "mean_pearson": nanmean(pearson),
            "mean_dominant_agreement": nanmean(agree)}


# ----------------------------------------------------------------------------------------------------------- device
class _Problem:
    """The device state of one call: x, the offsets, W, H, the workspace and the stop-rule words."""

    def __init__(self, x, k, off, n_init, beta_loss, rows, G):
        dev = device("nmf")
        self.dev, self.k, self.off, self.n_init, self.rows, self.G = dev, int(k), off, int(n_init), rows, G
        self.loss = LOSSES[beta_loss]
        self.S = int(off.size - 1)
        self.P = self.S * self.n_init
        self.max_n = int(np.diff(off).max())
        xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
        self.x, self.code = xd, FLOAT_CODE[xd.dtype]
        self._host = None if isinstance(x, Tensor) and x.is_cuda else np.asarray(x)
        self.ldx = int(xd.stride(0)) if rows > 1 else max(int(xd.stride(0)), int(xd.shape[1]))
        self.off_d = upload(off, dev)
        e = empty(dev)
        status = e((1,), torch.int32)
        call("mcl_nmf_check", xd, self.ldx, self.code, rows, G, status)
        bad = int(status.cpu().numpy().view(np.uint32)[0])              # read ahead of the first update
        if bad:
            raise ValueError(f"x: row {0xFFFFFFFF - bad} holds a negative or non-finite value")
        nbytes = int(call("mcl_nmf_workspace_bytes", rows, G, self.k, self.S, self.n_init, self.max_n, self.loss))
        self.work = e((nbytes // 8 + 1,), torch.float64)
        self.active = torch.ones((self.P,), device=dev, dtype=torch.int32)
        self.record = torch.zeros((self.P, 8), device=dev, dtype=torch.float64)

    def host_segment(self, j: int) -> np.ndarray:
        """Segment j of x on the host, fp64 and dense: what the initial scale is the mean of.  A host x is used as it came;
        a device x is copied back once per call, not once per segment."""
        if self._host is None:
            self._host = self.x.cpu().numpy()
        return np.ascontiguousarray(self._host[int(self.off[j]):int(self.off[j + 1]), :self.G], dtype=np.float64)

    def run(self, W: Tensor, H: Tensor, max_iter: int, tol: float, update_h: bool) -> Tensor:
        """The iterations and the stop rule.  Returns the error history (P, checks + 1)."""
        hist_len = max_iter // CHECK_EVERY + 1
        hist = torch.full((self.P, hist_len), float("nan"), device=self.dev, dtype=torch.float64)
        head = (self.x, self.ldx, self.code, self.off_d, self.S, self.n_init, self.rows, self.G, self.k, self.max_n, self.loss)
        tail = (self.work, self.active)
        call("mcl_nmf_error", *head, W, H, *tail, 0, 0, float(tol), max_iter, self.record, hist, hist_len)
        it = 0
        while it < max_iter:
            n = min(CHECK_EVERY, max_iter - it)
            call("mcl_nmf_steps", *head, int(update_h), W, H, *tail, n)
            it += n
            if tol > 0 and it % CHECK_EVERY == 0:
                call("mcl_nmf_error", *head, W, H, *tail, 1, it, float(tol), max_iter, self.record, hist, hist_len)
                if not self.active.cpu().numpy().any():                  # the one synchronisation per 10 iterations
                    break
        call("mcl_nmf_error", *head, W, H, *tail, 2, it, float(tol), max_iter, self.record, hist, hist_len)
        return hist


def _programs(pr: _Problem, Wb: Tensor, Hb: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    e = empty(pr.dev)
    hsum, prog = e((pr.S, pr.k), torch.float64), e((pr.S, pr.k, pr.G), torch.float64)
    usage, dom = e((pr.rows, pr.k), torch.float64), e((pr.rows,), torch.int32)
    call("mcl_nmf_programs", Wb, Hb, pr.off_d, pr.S, pr.rows, pr.G, pr.k, pr.max_n, hsum, prog, usage, dom)
    return hsum, prog, usage, dom


def nmf_device(x: ArrayLike, k: int, offsets=None, beta_loss: str = "frobenius", init: Init = "random", n_init: int = 1,
               seed: int = 0, max_iter: int = 200, tol: float = 1e-4, ld: Optional[int] = None,
               n_genes: Optional[int] = None, return_all: bool = False) -> Dict[str, Tensor]:
    """``nmf`` with everything left on the device (``n_iter`` / ``converged`` / ``best_start`` / ``err`` are small host
    arrays: the stop rule has read them).  See ``nmf``."""
    rows, G, off = check_problem(_shape(x), k, offsets, n_init, beta_loss, max_iter, tol, ld, n_genes)
    S = int(off.size - 1)
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f"init must be 'random' or a pair (W0, H0), got {init!r} (the nndsvd initialisations are not built)")
        seed = check_int(seed, "seed", 0, (1 << 32) - 1 - n_init)
        W0 = H0 = None
    else:
        W0, H0, n_init = custom_init(init, rows, G, int(k), S, int(n_init))
        if S * n_init > MAX_PROBLEMS:
            raise ValueError(f"{S} segments x {n_init} starts; at most {MAX_PROBLEMS} problems per call")
    pr = _Problem(x, k, off, n_init, beta_loss, rows, G)
    if W0 is None:
        W0, H0 = np.empty((n_init, rows, pr.k)), np.empty((S, n_init, pr.k, G))
        for j in range(S):
            seg = pr.host_segment(j)
            for s in range(n_init):
                W0[s, int(off[j]):int(off[j + 1])], H0[j, s] = random_init(seg, pr.k, seed + s)
    W, H = upload(W0, pr.dev), upload(H0.reshape(pr.P, pr.k, G), pr.dev)
    hist = pr.run(W, H, int(max_iter), float(tol), True)
    rec = pr.record.cpu().numpy().reshape(S, n_init, 8)
    err_all = rec[:, :, 5]
    best = np.array([int(np.lexsort((np.arange(n_init), np.where(np.isnan(e), np.inf, e)))[0]) for e in err_all], dtype=np.int64)
    if n_init == 1:
        Wb, Hb = W[0], H
    else:
        e = empty(pr.dev)
        Wb, Hb = e((rows, pr.k), torch.float64), e((S, pr.k, G), torch.float64)
        for j in range(S):
            Wb[int(off[j]):int(off[j + 1])].copy_(W[int(best[j]), int(off[j]):int(off[j + 1])])
            Hb[j].copy_(H[j * n_init + int(best[j])])
    _, prog, usage, dom = _programs(pr, Wb, Hb)
    pick = (np.arange(S), best)
    out = {"W": Wb, "H": Hb, "err": err_all[pick], "n_iter": rec[:, :, 3][pick].astype(np.int32),
           "converged": rec[:, :, 4][pick].astype(np.uint8), "best_start": best, "programs": prog, "usage": usage,
           "dominant": dom, "offsets": off}
    if return_all:
        out.update({"W_all": W, "H_all": H.view(S, n_init, pr.k, G), "err_all": err_all,
                    "n_iter_all": rec[:, :, 3].astype(np.int32), "converged_all": rec[:, :, 4].astype(np.uint8),
                    "err_init_all": rec[:, :, 0], "history_all": hist.view(S, n_init, -1)})
    return out


def _to_host(d: Dict[str, object]) -> Dict[str, np.ndarray]:
    return {key: (v.cpu().numpy() if isinstance(v, Tensor) else v) for key, v in d.items()}


def nmf(x: ArrayLike, k: int, offsets=None, beta_loss: str = "frobenius", init: Init = "random", n_init: int = 1,
        seed: int = 0, max_iter: int = 200, tol: float = 1e-4, ld: Optional[int] = None, n_genes: Optional[int] = None,
        return_all: bool = False) -> Dict[str, np.ndarray]:
    """Every row segment of ``x`` factorised into ``k`` non-negative programs, from ``n_init`` starts.

    ``x``: (rows, G) fp32 or fp64, host or device (a device tensor whose rows are strided is taken as it is); with ``ld``
    and ``n_genes``, (rows, ld) of which the first ``n_genes`` columns are the genes.  ``offsets``: the row offsets of the
    segments (``None``: one pooled problem).  ``init``: ``"random"`` (scikit-learn's stream, start s of a segment from
    ``RandomState(seed + s)`` and the segment's own mean) or ``(W0, H0)`` (``custom_init``; a leading ``n_init`` axis is
    allowed).  ``nndsvd`` is not built.

    Returns, per segment the start with the smallest final error (ties: the smaller index): ``W`` (rows, k), ``H``
    (segments, k, G), ``err`` = sqrt(2 D(X | WH)), ``n_iter`` (a multiple of 10, or ``max_iter``), ``converged`` (1 where
    the stop rule fired before ``max_iter``: where scikit-learn raises no ConvergenceWarning), ``best_start``;
    ``programs`` = H with every row scaled to sum 1 -- a (k, G) signature matrix per segment that ``deconv.nnls`` accepts
    as it is --, ``usage`` = W with that scale moved into it, ``dominant`` = the argmax of usage (ties: the smaller
    index; -1 for a zero row).  ``return_all=True`` adds every start: ``W_all`` (n_init, rows, k), ``H_all`` (segments,
    n_init, k, G), ``err_all``, ``n_iter_all``, ``converged_all``, ``err_init_all`` and ``history_all`` (segments, n_init,
    max_iter // 10 + 1: the error at init and at every check, NaN where none was taken)."""
    return _to_host(nmf_device(x, k, offsets, beta_loss, init, n_init, seed, max_iter, tol, ld, n_genes, return_all))


def transform_device(x: ArrayLike, H: ArrayLike, offsets=None, beta_loss: str = "frobenius", max_iter: int = 200,
                     tol: float = 1e-4, ld: Optional[int] = None) -> Dict[str, Tensor]:
    hs = _shape(H)
    if len(hs) not in (2, 3):
        raise ValueError(f"H: expected (k, G) or (segments, k, G), got shape {hs}")
    k, G = int(hs[-2]), int(hs[-1])
    rows, G, off = check_problem(_shape(x), k, offsets, 1, beta_loss, max_iter, tol, ld, G)
    S = int(off.size - 1)
    if len(hs) == 3 and hs[0] != S:
        raise ValueError(f"H: {hs[0]} program sets for {S} segments")
    Hh = np.asarray(H.cpu() if isinstance(H, Tensor) else H, dtype=np.float64)
    if not (np.isfinite(Hh).all() and (Hh >= 0).all()):
        raise ValueError("H must be finite and non-negative")
    pr = _Problem(x, k, off, 1, beta_loss, rows, G)
    if len(hs) == 2:
        one = dense(H, "H", (k, G), torch.float64, pr.dev)
        Hd = torch.empty((S, k, G), device=pr.dev, dtype=torch.float64)
        for j in range(S):
            Hd[j].copy_(one)
    else:
        Hd = dense(H, "H", (S, k, G), torch.float64, pr.dev, copy=True)
    W0 = np.empty((1, rows, k))
    for j in range(S):
        W0[0, int(off[j]):int(off[j + 1])] = np.sqrt(pr.host_segment(j).mean() / k)
    W = upload(W0, pr.dev)
    hist = pr.run(W, Hd, int(max_iter), float(tol), False)
    rec = pr.record.cpu().numpy()
    _, _, usage, dom = _programs(pr, W[0], Hd)
    return {"W": W[0], "err": rec[:, 5].copy(), "n_iter": rec[:, 3].astype(np.int32), "converged": rec[:, 4].astype(np.uint8),
            "usage": usage, "dominant": dom, "history": hist, "offsets": off}


def transform(x: ArrayLike, H: ArrayLike, offsets=None, beta_loss: str = "frobenius", max_iter: int = 200,
              tol: float = 1e-4, ld: Optional[int] = None) -> Dict[str, np.ndarray]:
    """scikit-learn's ``NMF(solver="mu").transform``: the usage of given programs.  ``H`` (k, G), shared by all segments,
    or (segments, k, G), stays fixed; W starts from ``full(sqrt(mean of the segment / k))`` and follows the same updates
    and stop rule.  Returns ``W`` (rows, k), ``err``, ``n_iter``, ``converged`` per segment, ``usage`` = W scaled by the row
    sums of H, ``dominant`` and ``history``."""
    return _to_host(transform_device(x, H, offsets, beta_loss, max_iter, tol, ld))


# ----------------------------------------------------------------------------------------------------------- slides
def _stack(matrices: Sequence[ArrayLike]) -> Tuple[Tensor, np.ndarray]:
    if not len(matrices):
        raise ValueError("matrices: need at least one slide")
    for i, m in enumerate(matrices):
        if len(m.shape) != 2 or int(m.shape[0]) < 1:
            raise ValueError(f"matrices[{i}]: expected (spots >= 1, genes), got {tuple(m.shape)}")
    return stack_rows(matrices, "matrices", device("nmf"))


def nmf_slides(matrices: Sequence[ArrayLike], k: int, pooled: bool = True, **kw) -> Dict[str, np.ndarray]:
    """``nmf`` of one (spots, genes) matrix per slide (arrays, or what ``load_gene_major`` returns), row-stacked:
    ``pooled`` fits one set of programs to all slides, else every slide is a problem of its own.  The result also holds
    ``slide_offsets``, by which ``usage`` and ``dominant`` split into slides."""
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    check_problem((int(off[-1]), int(matrices[0].shape[1])), k, None if pooled else off, kw.get("n_init", 1),
                  kw.get("beta_loss", "frobenius"), kw.get("max_iter", 200), kw.get("tol", 1e-4))
    x, off = _stack(matrices)
    res = nmf(x, k, None if pooled else off, **kw)
    res["slide_offsets"] = off
    return res


def top_genes(res: Dict[str, np.ndarray], program: int, n: int = TOP_N, segment: int = 0) -> np.ndarray:
    """The ``n`` gene indices of one program by descending weight (ties: the smaller index)."""
    return top_indices(np.asarray(res["programs"])[segment, program], n)


def program_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], k: int, n_top: int = 50, **kw) -> Dict[str, object]:
    """Does the predicted expression use the same gene programs, in the same spots, as the measured expression?

    The measured matrices are fitted pooled (``true``); the predicted matrices are ``transform``-ed under the measured
    programs: ``pearson`` (slides, k) and ``pearson_pooled`` (k,), for every program the Pearson r over the spots between
    the predicted and the measured usage, ``dominant_agreement`` (slides,) / ``dominant_agreement_pooled``, the share of
    spots with the same dominant program, and their ``mean_*``.  The predicted matrices are also fitted on their own
    (``pred``) and the two program sets matched greedily on cosine similarity (``match_programs``): ``matching`` (k, 2)
    (measured, predicted), ``cosine`` (k,), ``top_overlap`` and ``top_jaccard`` of the ``n_top`` genes of every matched
    pair, ``mean_cosine``, ``mean_top_jaccard``.  ``kw`` goes to ``nmf`` (``beta_loss``, ``n_init``, ``seed``,
    ``max_iter``, ``tol``)."""
    n_top = check_int(n_top, "n_top", 1)
    off = paired_offsets(preds, trues, "slide")
    rt = nmf_slides(trues, k, True, **kw)
    rp = nmf_slides(preds, k, True, **kw)
    xp, _ = _stack(preds)
    tr = transform(xp, rt["H"][0], None, kw.get("beta_loss", "frobenius"), kw.get("max_iter", 200), kw.get("tol", 1e-4))
    out = usage_scores(tr["usage"], rt["usage"], tr["dominant"], rt["dominant"], off)
    pairs, cos = match_programs(rt["programs"][0], rp["programs"][0])
    over, jac = top_gene_overlap(rt["programs"][0], rp["programs"][0], pairs, n_top)
    out.update({"matching": pairs, "cosine": cos, "top_overlap": over, "top_jaccard": jac, "mean_cosine": nanmean(cos),
                "mean_top_jaccard": nanmean(jac), "true": rt, "pred": rp, "pred_under_true": tr})
    return out


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.nmf",
                                description="Factor expression into non-negative gene programs (batched NMF) and score how "
                                            "well predictions recover the measured programs")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery line")
    p.add_argument("--k", type=int, default=8, help="programs")
    p.add_argument("--beta_loss", default="frobenius", choices=sorted(LOSSES))
    p.add_argument("--n_init", type=int, default=4, help="starts; the one with the smallest error is kept")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max_iter", type=int, default=200)
    p.add_argument("--tol", type=float, default=1e-4)
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the index)")
    p.add_argument("--top", type=int, default=TOP_N, help="genes to print per program")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/{OUT_FILE} and <out_dir>/<slide>/usage.npy")
    a = p.parse_args(argv)
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.top < 1 or a.k < 1 or a.n_init < 1:
        p.error("--top, --k and --n_init must be >= 1")
    return a


def format_programs(res: Dict[str, np.ndarray], names: Sequence[str], top: int) -> List[str]:
    share = res["usage"].sum(axis=0)
    share = share / share.sum() if share.sum() > 0 else share
    return [f"program {t} usage share {share[t]:.4f}: " + ", ".join(str(names[g]) for g in top_genes(res, t, top))
            for t in range(res["programs"].shape[1])]


def format_recovery(rec: Dict[str, object]) -> str:
    return (f"recovery: mean usage Pearson {rec['mean_pearson']:.4f}, mean dominant agreement "
            f"{rec['mean_dominant_agreement']:.4f}, mean matched cosine {rec['mean_cosine']:.4f}, mean top-gene Jaccard "
            f"{rec['mean_top_jaccard']:.4f}")


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    trues = load_gene_major(args.true) if args.true is not None else None
    kw = dict(beta_loss=args.beta_loss, n_init=args.n_init, seed=args.seed, max_iter=args.max_iter, tol=args.tol)
    G = int(preds[0].shape[1])
    names = [str(g) for g in range(G)]
    if args.genes is not None:
        names = [str(v) for v in np.load(args.genes, allow_pickle=True).reshape(-1)]
        if len(names) != G:
            raise ValueError(f"{args.genes}: {len(names)} gene names for {G} genes")
    if trues is not None:
        rec = program_recovery(preds, trues, args.k, **kw)
        res = rec["pred"]
    else:
        rec, res = None, nmf_slides(preds, args.k, True, **kw)
    print(f"k = {args.k}, {args.beta_loss}, n_iter {int(res['n_iter'][0])}, error {float(res['err'][0]):.6g}, best start "
          f"{int(res['best_start'][0])}")
    print("\n".join(format_programs(res, names, args.top)))
    if args.out_dir is not None:
        os.makedirs(args.out_dir, exist_ok=True)
        np.savez(os.path.join(args.out_dir, OUT_FILE), genes=np.asarray(names),
                 **{key: np.asarray(res[key]) for key in KEYS + ("slide_offsets",)})
        off = res["slide_offsets"]
        for i in range(off.size - 1):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "usage.npy"), res["usage"][int(off[i]):int(off[i + 1])])
    if rec is not None:
        print(format_recovery(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
