"""Spots as mixtures of cell types on the MI355X: every spot of an evaluation as a non-negative combination of cell-type
(or domain) expression signatures, ``b_i = argmin over b >= 0 of || x_i - S^T b ||_2`` -- the NNLS baseline of the
deconvolution benchmarks, what a ``scipy.optimize.nnls`` loop over the spots computes -- for all slides per call, and the
number the feature exists for: does the predicted expression imply the same tissue composition as the measured expression
(``deconvolution_recovery``)?  The signatures are given, pooled from annotated slides (``signatures_from_groups``), or found
without labels: ``nmf.nmf(x, k)["programs"][segment]`` is a (T, G) signature matrix that ``nnls`` accepts as it is.

What is computed is stated in DESIGN 6.21 and restated in numpy by ``tests/deconv_reference.py``, which is pinned to
``scipy.optimize.nnls``.  Parity with SPOTlight, RCTD or cell2location is unpinned, and no signature set is shipped or
fetched.  The rules:

* fp64 throughout (``x`` may be fp32: converted on load); no floating-point atomics; every sum runs in an order that
  depends on G and T alone.  A spot's outputs are bit-identical whether it is alone in a call, anywhere in a batch, or in a
  batch whose rows were permuted, run to run.
* ``A = S S^T`` must be positive definite: the Cholesky pivots of A are checked on the device, and a type whose pivot is
  not above ``T eps A_jj`` (rank-deficient signatures, a zero signature row) or that holds a NaN / Inf raises a
  ``ValueError`` naming the type; a non-finite spot raises one naming the row.  Neither launches the solve.
* The solve is Lawson-Hanson's active-set method on the normal equations ``(A, c_i = S x_i)``: from ``b = 0``, ``P`` empty,
  ``w = c``; the largest ``w_j`` outside P enters (ties: the smaller index) until P is full or that ``w_j <= 10 T eps
  max|c_i|``; ``A_PP z = c_P`` by a Cholesky factor that grows a row per entering index; ``z_P > 0`` is accepted, else the
  iterate steps to the boundary (``alpha = min b_j / (b_j - z_j)`` over ``z_j <= 0``) and every index with ``b_j <= 0`` leaves
  P with ``b_j = 0`` exactly; an entering index that comes back with ``z_j <= 0`` leaves at once with ``w_j = 0``.  At most
  ``3 T`` inner solves (scipy's cap): a spot that reaches it keeps its last feasible iterate with ``converged = 0``.
* ``rnorm`` is summed from ``x`` itself in a second pass, not as ``q - 2 b.c + b^T A b``, which cancels where the fit is
  good.  ``r2 = 1 - rnorm^2 / (x.x)`` (NaN for a zero spot), ``proportions = coef / sum(coef)`` (a zero row where the sum
  is 0), ``dominant`` = its argmax (ties: the smaller index; -1 for a zero row).
* 1 <= T <= 64 types, T <= G <= 16384 genes, rows T < 2^31: ``ValueError`` before a launch.

No CPU fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.deconv --pred P1.npy ... (--signatures S.npy | --labels L1.npy ... --true T1.npy ...)
                                  [--types names.npy] [--true T1.npy ...] [--top 5] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import markers
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_int, cumulative_offsets, dense, device, empty, load_gene_major,
                      matrix, nanmean, paired_offsets, stack_rows, upload)
from ._lib import call

MAX_TYPES = 64           # csrc/deconv.hip: a lane per type
MAX_GENES = 16384
MAX_CELLS = (1 << 31) - 1
OUT_FILE = "deconv.npz"
TOP_N = 5
KEYS = ("coef", "rnorm", "r2", "n_iter", "converged", "proportions", "dominant")


# ------------------------------------------------------------------------------------------------------- host rules
def check_problem(x_shape: Sequence[int], s_shape: Sequence[int], ld: Optional[int] = None) -> Tuple[int, int, int]:
    """The limits, checked on the host before the GPU is touched.  Returns (rows, G, T)."""
    if len(s_shape) != 2:
        raise ValueError(f"signatures: expected a 2-D (types, genes) matrix, got shape {tuple(s_shape)}")
    T, G = int(s_shape[0]), int(s_shape[1])
    if T < 1 or T > MAX_TYPES:
        raise ValueError(f"signatures: {T} types; the kernel handles 1 .. {MAX_TYPES}")
    if G < T or G > MAX_GENES:
        raise ValueError(f"signatures: {G} genes for {T} types; the kernel handles T <= G <= {MAX_GENES}")
    if len(x_shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(x_shape)}")
    rows, width = int(x_shape[0]), int(x_shape[1])
    if ld is not None:
        ld = check_int(ld, "ld", G)
    if width != (G if ld is None else ld):
        raise ValueError(f"x: expected (rows, {G if ld is None else ld}) for {G} genes" +
                         ("" if ld is None else f" and ld = {ld}") + f", got {tuple(x_shape)}")
    if rows < 1:
        raise ValueError("x: no spot")
    if rows * T > MAX_CELLS:
        raise ValueError(f"x: {rows} spots x {T} types; at most {MAX_CELLS} coefficients per call")
    return rows, G, T


def _shape(a) -> Tuple[int, ...]:
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


# ----------------------------------------------------------------------------------------------------------- device
def nnls_device(x: ArrayLike, signatures: ArrayLike, ld: Optional[int] = None) -> Dict[str, Tensor]:
    """``nnls`` with everything left on the device: ``coef`` (rows, T) fp64, ``rnorm``, ``r2`` (rows,) fp64, ``n_iter``
    int32, ``converged`` uint8, ``proportions`` (rows, T) fp64, ``dominant`` int32, and the intermediates ``gram`` (T, T),
    ``cholesky`` (T, T), ``c`` (rows, T), ``q`` (rows,).  The one synchronisation is the read of the status words, ahead of
    the solve."""
    rows, G, T = check_problem(_shape(x), _shape(signatures), ld)
    dev = device("deconv")
    xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
    S = dense(signatures, "signatures", (T, G), torch.float64, dev)
    code, ldx = FLOAT_CODE[xd.dtype], int(xd.stride(0)) if rows > 1 else max(int(xd.stride(0)), int(xd.shape[1]))
    e = empty(dev)
    f64, i32 = torch.float64, torch.int32
    A, L, status = e((T, T), f64), e((T, T), f64), e((4,), i32)
    c, q = e((rows, T), f64), e((rows,), f64)
    call("mcl_nnls_gram", S, T, G, A, L, status[0:2])
    call("mcl_nnls_products", xd, ldx, code, rows, G, S, T, c, q, status[2:3])
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad[1]:
        raise ValueError(f"signatures: type {int(bad[1]) - 1} holds a non-finite value")
    if bad[0]:
        raise ValueError(f"signatures: type {int(bad[0]) - 1} is a combination of the types before it, or zero (its Cholesky "
                         f"pivot is not above T eps A_jj): S S^T must be positive definite")
    if bad[2]:
        raise ValueError(f"x: row {0xFFFFFFFF - int(bad[2:3].view(np.uint32)[0])} holds a non-finite value")
    coef, n_iter, conv = e((rows, T), f64), e((rows,), i32), e((rows,), torch.uint8)
    call("mcl_nnls_solve", A, c, rows, T, coef, n_iter, conv)
    rnorm, r2, prop, dom = e((rows,), f64), e((rows,), f64), e((rows, T), f64), e((rows,), i32)
    call("mcl_nnls_residual", xd, ldx, code, rows, G, S, T, coef, q, rnorm, r2, prop, dom)
    return {"coef": coef, "rnorm": rnorm, "r2": r2, "n_iter": n_iter, "converged": conv, "proportions": prop,
            "dominant": dom, "gram": A, "cholesky": L, "c": c, "q": q}


def nnls(x: ArrayLike, signatures: ArrayLike, ld: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Every row of ``x`` as a non-negative combination of the rows of ``signatures``.

    ``x``: (rows, G) fp32 or fp64, host or device (a device tensor whose rows are strided is taken as it is); with ``ld``,
    (rows, ld) of which the first G columns are the genes.  ``signatures``: (T, G).  Returns numpy arrays: ``coef`` (rows,
    T), ``rnorm``, ``r2`` (rows,), ``n_iter`` (the inner solves), ``converged`` (0 where the cap of 3 T solves was
    reached), ``proportions`` (rows, T) and ``dominant`` (rows,) int32."""
    d = nnls_device(x, signatures, ld)
    return {key: d[key].cpu().numpy() for key in KEYS}


# ------------------------------------------------------------------------------------------------------- signatures
def encode_pooled(labels: Sequence[Sequence], undetermined="undetermined") -> Tuple[List[np.ndarray], np.ndarray]:
    """One label vector per slide -> (int32 codes per slide, the names of the codes), the codes shared by all slides:
    integer vectors are group ids as they are (-1 stays -1, names 0 .. max), anything else is indexed into the sorted
    distinct labels of all slides with ``undetermined`` as -1.  A code no spot carries is a ``ValueError``."""
    arrs = [np.asarray(lab) for lab in labels]
    for i, a in enumerate(arrs):
        if a.ndim != 1:
            raise ValueError(f"labels[{i}]: expected a 1-D vector, got shape {a.shape}")
    if all(np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_ for a in arrs):
        if any((a < -1).any() for a in arrs):
            raise ValueError("labels: integer group ids must be >= -1 (-1: not part of the analysis)")
        K = max([int(a.max(initial=-1)) for a in arrs]) + 1
        names = np.arange(K)
        codes = [a.astype(np.int32) for a in arrs]
    else:
        arrs = [a.astype(str) for a in arrs]
        names = np.unique(np.concatenate([a[a != str(undetermined)] for a in arrs]))
        codes = []
        for a in arrs:
            keep = a != str(undetermined)
            cd = np.full(a.size, -1, dtype=np.int32)
            cd[keep] = np.searchsorted(names, a[keep]).astype(np.int32)
            codes.append(cd)
        K = int(names.size)
    if K < 1:
        raise ValueError("labels: no spot is left after dropping the undetermined ones")
    seen = np.zeros(K, dtype=bool)
    for cd in codes:
        seen[cd[cd >= 0]] = True
    if not seen.all():
        raise ValueError(f"labels: group {names[int(np.flatnonzero(~seen)[0])]!r} occurs on no slide")
    return codes, names


def pool_means(means: Sequence[np.ndarray], sizes: Sequence[np.ndarray]) -> np.ndarray:
    """The size-weighted mean over slides of per-slide group means (K, G) with group sizes (K,); a group absent from a
    slide contributes nothing."""
    tot = np.zeros(np.asarray(sizes[0]).shape, dtype=np.float64)
    acc = np.zeros(np.asarray(means[0]).shape, dtype=np.float64)
    for m, n in zip(means, sizes):
        n = np.asarray(n, dtype=np.float64)
        acc += np.where(n[:, None] > 0, np.asarray(m, dtype=np.float64) * n[:, None], 0.0)
        tot += n
    return acc / tot[:, None]


def signatures_from_groups(matrices: Sequence[ArrayLike], labels: Sequence[Sequence],
                           undetermined="undetermined") -> Tuple[np.ndarray, np.ndarray]:
    """(S (T, G), names): the mean profile of every label pooled over all slides given -- the measured matrices under the
    pathologist's annotation or any of this library's domain labels.  The per-slide group means and sizes are
    ``mcl_marker_stats``'; the pooling is a size-weighted mean on the host.  Spots labelled -1 (``undetermined``) are
    dropped; a label that occurs nowhere is a ``ValueError``."""
    if len(matrices) != len(labels) or not len(matrices):
        raise ValueError(f"need one label vector per slide and >= 1 slide; got {len(matrices)} and {len(labels)}")
    for i, (m, lab) in enumerate(zip(matrices, labels)):
        if len(m.shape) != 2 or m.shape[0] != len(lab):
            raise ValueError(f"slide {i}: matrix {tuple(m.shape)} and {len(lab)} labels do not match")
    codes, names = encode_pooled(labels, undetermined)
    K = int(names.size)
    if K > MAX_TYPES:
        raise ValueError(f"labels: {K} groups; at most {MAX_TYPES} signatures")
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    rows, G = int(off[-1]), int(matrices[0].shape[1])
    off, kk = markers.check_problem((rows, G), off, np.full(len(matrices), K))
    dev = device("deconv")
    xd, off = stack_rows(matrices, "matrices", dev)
    lab_d = markers.device_labels(np.concatenate(codes), rows, dev)
    S_n, KT = int(kk.size), int(kk.size) * K
    e = empty(dev)
    f64, i32 = torch.float64, torch.int32
    work = e((int(call("mcl_marker_workspace_bytes", rows, KT, S_n, G)) // 8 + 1,), f64)
    gsize, nvalid, status = e((KT,), i32), e((S_n,), i32), e((S_n, 2), i32)
    mg, vg, mr, vr, pg, pr = (e((KT, G), f64) for _ in range(6))
    zg, zr = e((KT, G), i32), e((KT, G), i32)
    call("mcl_marker_stats", xd, int(xd.stride(0)), FLOAT_CODE[xd.dtype], upload(off, dev), lab_d, upload(kk, dev), S_n,
         rows, G, int(np.diff(off).max()), K, KT, work, gsize, nvalid, mg, vg, mr, vr, pg, pr, zg, zr, status)
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad.any():
        s = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"matrices: slide {s} holds {int(bad[s, 0])} non-finite values" if bad[s, 0] else
                         f"labels: slide {s} holds {int(bad[s, 1])} group ids outside -1 .. {K - 1}")
    means, sizes = mg.cpu().numpy().reshape(S_n, K, G), gsize.cpu().numpy().reshape(S_n, K)
    return pool_means(list(means), list(sizes)), names


# ----------------------------------------------------------------------------------------------------------- slides
def deconvolve_slides(matrices: Sequence[ArrayLike], signatures: ArrayLike) -> List[Dict[str, np.ndarray]]:
    """``nnls`` of one (spots, genes) matrix per slide, from one call on the row-stacked matrix: one result dict per slide.
    Warns once with the number of spots that have ``converged == 0``.  A slide's ``dominant`` is a label vector that
    ``nhood.arrangement_slides`` and ``markers.marker_slides`` accept (-1: a spot that no signature explains)."""
    if not len(matrices):
        raise ValueError("matrices: need at least one slide")
    for i, m in enumerate(matrices):
        if len(m.shape) != 2 or int(m.shape[0]) < 1:
            raise ValueError(f"matrices[{i}]: expected (spots >= 1, genes), got {tuple(m.shape)}")
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    check_problem((int(off[-1]), int(matrices[0].shape[1])), _shape(signatures))
    dev = device("deconv")
    x, off = stack_rows(matrices, "matrices", dev)
    res = nnls(x, signatures)
    lost = int((res["converged"] == 0).sum())
    if lost:
        warnings.warn(f"deconv: {lost} of {int(off[-1])} spots reached the cap of 3 T inner solves (converged == 0); they "
                      f"keep their last feasible iterate", RuntimeWarning, stacklevel=2)
    return [{key: v[off[s]:off[s + 1]] for key, v in res.items()} for s in range(off.size - 1)]


def column_pearson(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Pearson r of every column pair of two (n, T) arrays; NaN where a column is constant or n < 2."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape[0] < 2:
        return np.full(a.shape[1], np.nan)
    da, db = a - a.mean(axis=0), b - b.mean(axis=0)
    den = np.sqrt((da * da).sum(axis=0) * (db * db).sum(axis=0))
    with np.errstate(all="ignore"):
        return np.where(den > 0, (da * db).sum(axis=0) / den, np.nan)


def recovery_scores(rp: Dict[str, np.ndarray], rt: Dict[str, np.ndarray]) -> Dict[str, object]:
    """``pearson`` (T,), ``dominant_agreement`` and ``rmse`` of one slide's predicted and measured results."""
    pp, pt = rp["proportions"], rt["proportions"]
    diff = pp - pt
    return {"pearson": column_pearson(pp, pt), "dominant_agreement": float((rp["dominant"] == rt["dominant"]).mean()),
            "rmse": float(np.sqrt((diff * diff).mean()))}


def deconvolution_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], signatures: ArrayLike) -> Dict[str, object]:
    """Does the predicted expression imply the same tissue composition as the measured expression?  Both are deconvolved
    with the same signatures.  Per slide: ``pearson`` (S, T), for every type the Pearson r over the spots between the
    predicted and the measured proportions (NaN where either is constant); ``dominant_agreement`` (S,), the share of spots
    whose ``dominant`` agrees; ``rmse`` (S,), over all proportions of the slide.  Averaged over the slides with
    ``nanmean``: ``mean_pearson_per_type`` (T,), ``mean_pearson`` (over every finite (slide, type)),
    ``mean_dominant_agreement``, ``mean_rmse``.  Also the two results ``pred`` / ``true``, whose ``dominant`` vectors are
    label vectors that ``nhood.arrangement_slides`` and ``markers.marker_slides`` accept."""
    paired_offsets(preds, trues, "slide")
    rp, rt = deconvolve_slides(preds, signatures), deconvolve_slides(trues, signatures)
    per = [recovery_scores(a, b) for a, b in zip(rp, rt)]
    pearson = np.stack([p["pearson"] for p in per])
    out = {"pearson": pearson, "dominant_agreement": np.array([p["dominant_agreement"] for p in per]),
           "rmse": np.array([p["rmse"] for p in per])}
    out.update({"mean_pearson_per_type": np.array([nanmean(pearson[:, t]) for t in range(pearson.shape[1])]),
                "mean_pearson": nanmean(pearson), "mean_dominant_agreement": nanmean(out["dominant_agreement"]),
                "mean_rmse": nanmean(out["rmse"]), "pred": rp, "true": rt})
    return out


def top_types(res: Sequence[Dict[str, np.ndarray]], slide: int, n: int = TOP_N) -> np.ndarray:
    """The ``n`` types of one slide by descending mean proportion (ties: the smaller index)."""
    mean = res[slide]["proportions"].mean(axis=0)
    return np.lexsort((np.arange(mean.size), -mean))[:max(0, int(n))].astype(np.int64)


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.deconv",
                                description="Deconvolve spots into proportions of cell-type signatures (batched NNLS) and "
                                            "score how well predictions recover the measured composition")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--signatures", default=None, help=".npy of (T, G) signatures")
    p.add_argument("--labels", default=None, nargs="+",
                   help="one label vector per slide: the signatures are the pooled group means of the --true matrices")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery line")
    p.add_argument("--types", default=None, help=".npy of T type names (default: the group labels, or the index)")
    p.add_argument("--top", type=int, default=TOP_N, help="types to print per slide")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if (a.signatures is None) == (a.labels is None):
        p.error("give either --signatures or --labels (with --true)")
    if a.labels is not None and a.true is None:
        p.error("--labels needs the --true matrices the signatures are pooled from")
    if a.labels is not None and len(a.labels) != len(a.pred):
        p.error(f"{len(a.labels)} --labels files for {len(a.pred)} --pred files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def format_slides(res: Sequence[Dict[str, np.ndarray]], names: Sequence[str], top: int) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        mean = r["proportions"].mean(axis=0)
        cells = [f"{names[t]} {mean[t]:.4f}" for t in top_types(res, s, top)]
        lines.append(f"slide {s} n = {r['coef'].shape[0]} mean r2 {nanmean(r['r2']):.4f} unassigned "
                     f"{int((r['dominant'] < 0).sum())}: " + ", ".join(cells))
    return lines


def format_recovery(rec: Dict[str, object]) -> List[str]:
    lines = [f"slide {s}: Pearson {nanmean(rec['pearson'][s]):.4f}, dominant agreement {rec['dominant_agreement'][s]:.4f}, "
             f"RMSE {rec['rmse'][s]:.4f}" for s in range(len(rec["rmse"]))]
    lines.append(f"recovery: mean Pearson {rec['mean_pearson']:.4f}, mean dominant agreement "
                 f"{rec['mean_dominant_agreement']:.4f}, mean RMSE {rec['mean_rmse']:.4f}")
    return lines


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    trues = load_gene_major(args.true) if args.true is not None else None
    if args.signatures is not None:
        S = np.load(args.signatures)
        names = [str(t) for t in range(S.shape[0])]
    else:
        labels = [np.load(f, allow_pickle=True).reshape(-1) for f in args.labels]
        S, cats = signatures_from_groups(trues, labels)
        names = [str(v) for v in cats]
    if args.types is not None:
        names = [str(v) for v in np.load(args.types, allow_pickle=True).reshape(-1)]
        if len(names) != S.shape[0]:
            raise ValueError(f"{args.types}: {len(names)} type names for {S.shape[0]} signatures")
    if trues is not None:
        rec = deconvolution_recovery(preds, trues, S)
        res = rec["pred"]
    else:
        rec, res = None, deconvolve_slides(preds, S)
    print("\n".join(format_slides(res, names, args.top)))
    if args.out_dir is not None:
        for i, r in enumerate(res):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, OUT_FILE), types=np.asarray(names), signatures=np.asarray(S, dtype=np.float64),
                     **{key: np.asarray(v) for key, v in r.items()})
    if rec is not None:
        print("\n".join(format_recovery(rec)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
