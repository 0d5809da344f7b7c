"""Marker genes of spot groups on the MI355X: what ``sc.tl.rank_genes_groups(adata, groupby, method=...)`` leaves in
``uns["rank_genes_groups"]`` (``reference="rest"``), for all slides of an evaluation per call, and the number the feature
exists for: do predicted expression values recover the marker genes of the measured ones (``marker_recovery``)?  The
groups are whatever labels a slide carries: ``cluster.cluster_slides`` domains, ``leiden.leiden`` communities, or the
pathologist's annotation (``undetermined`` spots are left out).

What is computed is stated in DESIGN 6.15 and restated in numpy by ``tests/markers_reference.py``; every piece scipy has
(``rankdata``, ``ranksums``, ``mannwhitneyu``, ``ttest_ind(equal_var=False)``, ``false_discovery_control``) is pinned to
scipy.  scanpy is not installed: parity with a scanpy release is unpinned.  Things to know:

* Methods ``"wilcoxon"`` (default; ``tie_correct`` as in scanpy), ``"t-test"`` (Welch) and ``"t-test_overestim_var"``.
* Rows labelled -1 are dropped from everything, exactly as if the slide had been subset first.
* Rank sums and tie terms are exact int64; ``-0.0`` ties with ``+0.0``.  A NaN statistic (an empty group, an empty rest, a
  constant column, a group of one spot under Welch) becomes score 0 and p = 1.
* ``neglog10_pvals`` is evaluated in log space and stays finite where ``pvals`` underflows to 0 (a real marker on a
  4000-spot slide has |z| > 38); ``pvals`` itself underflows as scipy's does.
* ``pvals_adj`` is Benjamini-Hochberg over the genes of a (slide, group).
* Genes go by descending score (``rankby_abs``: |score|); equal scores go by ascending gene index, an order scanpy's
  ``argpartition`` leaves open.
* 2 <= n_s <= 16384 spots per slide, k <= 255 groups, at most 16384 genes and 65535 slides: ``ValueError`` before a launch.
  A non-finite value or a label outside [-1, k) is counted on the device and raises ``ValueError`` after the first launch.

Bit-reproducible run to run, free of floating-point atomics; a slide inside a batch is bit-identical to the same slide
alone.  No CPU fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.markers --pred P1.npy ... --labels L1.npy ... [--true T1.npy ...] [--genes names.npy]
                                   [--method wilcoxon] [--tie_correct] [--top 50] --out_dir D
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import cluster
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_flag, cumulative_offsets, device, empty, load_gene_major, matrix,
                      stack_rows, upload, validate_offsets)
from ._lib import call

MAX_ROWS = 16384         # csrc/markers.hip: a column's keys and group bytes sit in LDS
MAX_GROUPS = 255
MAX_GENES = 16384
MAX_SLIDES = 65535
METHODS = {"wilcoxon": 0, "t-test": 1, "t-test_overestim_var": 2}
OUT_FILE = "markers.npz"
TOP_N = 50
ORDERED = ("names", "scores", "pvals", "pvals_adj", "neglog10_pvals", "logfoldchanges")
FULL = ("means", "vars", "means_rest", "vars_rest", "pts", "pts_rest")


# ------------------------------------------------------------------------------------------------------- host rules
def _check_options(method, tie_correct, n_genes, rankby_abs, G: int) -> int:
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    check_flag(tie_correct, "tie_correct")
    check_flag(rankby_abs, "rankby_abs")
    if n_genes is None:
        return G
    if isinstance(n_genes, bool) or not isinstance(n_genes, (int, np.integer)) or n_genes < 1:
        raise ValueError(f"n_genes must be a positive integer or None, got {n_genes!r}")
    return min(int(n_genes), G)


def check_k(k, S: int) -> np.ndarray:
    """``k`` as int32 per slide: an int stands for every slide; each 1 .. MAX_GROUPS."""
    kk = np.asarray(k)
    if kk.ndim == 0:
        kk = np.full(S, kk)
    if kk.shape != (S,) or not np.issubdtype(kk.dtype, np.integer):
        raise ValueError(f"k: expected {S} integers (one per slide), got {k!r}")
    if (kk < 1).any() or (kk > MAX_GROUPS).any():
        raise ValueError(f"every slide needs 1 .. {MAX_GROUPS} groups; k = {kk.tolist()}")
    return kk.astype(np.int32)


def device_labels(labels, rows: int, dev: torch.device) -> Tensor:
    """The group ids of ``rows`` spots as an int32 device tensor; a tensor must already be int32."""
    if isinstance(labels, Tensor):
        if labels.dtype != torch.int32 or tuple(labels.shape) != (rows,):
            raise ValueError(f"labels: a tensor must be int32 of shape ({rows},), got {labels.dtype} {tuple(labels.shape)}")
        return labels.contiguous().to(dev) if not labels.is_cuda else labels
    lab = np.asarray(labels)
    if lab.shape != (rows,) or not np.issubdtype(lab.dtype, np.integer) or lab.dtype == np.bool_:
        raise ValueError(f"labels: expected {rows} integer group ids (-1: not part of the analysis), got shape {lab.shape} "
                         f"dtype {lab.dtype}")
    if lab.size and (lab.min() < np.iinfo(np.int32).min or lab.max() > np.iinfo(np.int32).max):
        raise ValueError("labels: group ids must fit int32")
    return upload(lab.astype(np.int32), dev)


def infer_k(labels, offsets: np.ndarray) -> np.ndarray:
    """k per slide = the largest label + 1 (at least 1): what ``k=None`` means for host labels."""
    lab = np.asarray(labels)
    return np.array([max(1, int(lab[offsets[s]:offsets[s + 1]].max(initial=-1)) + 1) for s in range(offsets.size - 1)],
                    dtype=np.int64)


def check_problem(shape: Sequence[int], offsets, k, labels=None):
    """The limits, checked on the host before the GPU is touched.  Returns (offsets int64, k int32)."""
    if len(shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(shape)}")
    rows, G = int(shape[0]), int(shape[1])
    if G < 1 or G > MAX_GENES:
        raise ValueError(f"1 .. {MAX_GENES} genes per call, got {G}")
    off = validate_offsets(offsets, rows, min_rows=2, max_rows=MAX_ROWS, max_segments=MAX_SLIDES, none_is_one=True,
                           noun="slide")
    if k is None:
        if labels is None or isinstance(labels, Tensor):
            raise ValueError("k: needed when the labels are a device tensor")
        lab = np.asarray(labels)
        if lab.shape != (rows,) or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"labels: expected {rows} integer group ids, got shape {lab.shape} dtype {lab.dtype}")
        k = infer_k(lab, off)
    return off, check_k(k, off.size - 1)


# ----------------------------------------------------------------------------------------------------------- device
def rank_genes_groups_device(x: ArrayLike, labels, offsets: Optional[Sequence[int]] = None, k=None,
                             method: str = "wilcoxon", tie_correct: bool = False, n_genes: Optional[int] = None,
                             rankby_abs: bool = False) -> Dict[str, object]:
    """``rank_genes_groups`` with everything left on the device.  The per-group tensors are stacked over the slides: group
    g of slide s is row ``group_offsets[s] + g``.  Returns the ordered (sum k, n_genes) ``names`` (int64), ``scores``,
    ``pvals``, ``pvals_adj``, ``neglog10_pvals``, ``logfoldchanges``; the gene-order (sum k, G) ``means``, ``vars``,
    ``means_rest``, ``vars_rest``, ``pts``, ``pts_rest``, ``nnz``, ``nnz_rest``, ``rank_sums2``, ``full_scores``,
    ``full_pvals``, ``full_pvals_adj``, ``full_neglog10_pvals``, ``full_logfoldchanges``; ``tie_terms`` (S, G);
    ``group_sizes`` (sum k,), ``n_valid`` (S,); and the host ``offsets``, ``k``, ``group_offsets``.  The one read-back is the
    status word per slide."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    off, kk = check_problem(shape, offsets, k, labels)
    rows, G = int(shape[0]), int(shape[1])
    n_top = _check_options(method, tie_correct, n_genes, rankby_abs, G)
    dev = device("markers")
    xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
    lab_d = device_labels(labels, rows, dev)
    S, max_n, kmax = int(kk.size), int(np.diff(off).max()), int(kk.max())
    goff = cumulative_offsets(kk)
    KT = int(goff[-1])
    code, ld = FLOAT_CODE[xd.dtype], int(xd.stride(0))
    e = empty(dev)
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    work = e((int(call("mcl_marker_workspace_bytes", rows, KT, S, G)) // 8 + 1,), f64)
    off_d, k_d = upload(off, dev), upload(kk, dev)
    gsize, nvalid, status = e((KT,), i32), e((S,), i32), e((S, 2), i32)
    mg, vg, mr, vr, pg, pr = (e((KT, G), f64) for _ in range(6))
    zg, zr = e((KT, G), i32), e((KT, G), i32)
    call("mcl_marker_stats", xd, ld, code, off_d, lab_d, k_d, S, rows, G, max_n, kmax, KT, work, gsize, nvalid, mg, vg, mr,
         vr, pg, pr, zg, zr, status)
    R2, T = e((KT, G), i64), e((S, G), i64)
    # (the rank sums are part of the result for every method: they are what the tests pin exactly)
    call("mcl_marker_rank_sums", xd, ld, code, lab_d, S, rows, G, max_n, kmax, KT, work, R2, T)
    sc, pv, nl, lfc, adj = (e((KT, G), f64) for _ in range(5))
    call("mcl_marker_test", METHODS[method], int(bool(tie_correct)), S, rows, G, kmax, KT, work, gsize, mg, vg, mr, vr, R2,
         T, sc, pv, nl, lfc)
    names = e((KT, n_top), i64)
    o_sc, o_pv, o_adj, o_nl, o_lfc = (e((KT, n_top), f64) for _ in range(5))
    call("mcl_marker_rank_adjust", S, rows, G, kmax, KT, n_top, int(bool(rankby_abs)), work, sc, pv, nl, lfc, adj, names,
         o_sc, o_pv, o_adj, o_nl, o_lfc)
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad.any():
        s = int(np.flatnonzero(bad.any(axis=1))[0])
        if bad[s, 1]:
            raise ValueError(f"labels: slide {s} holds {int(bad[s, 1])} group ids outside -1 .. {int(kk[s]) - 1}")
        raise ValueError(f"x: slide {s} holds {int(bad[s, 0])} non-finite values")
    return {"names": names, "scores": o_sc, "pvals": o_pv, "pvals_adj": o_adj, "neglog10_pvals": o_nl,
            "logfoldchanges": o_lfc, "means": mg, "vars": vg, "means_rest": mr, "vars_rest": vr, "pts": pg, "pts_rest": pr,
            "nnz": zg, "nnz_rest": zr, "rank_sums2": R2, "tie_terms": T, "full_scores": sc, "full_pvals": pv,
            "full_pvals_adj": adj, "full_neglog10_pvals": nl, "full_logfoldchanges": lfc, "group_sizes": gsize,
            "n_valid": nvalid, "offsets": off, "k": kk, "group_offsets": goff}


def rank_genes_groups(x: ArrayLike, labels, offsets: Optional[Sequence[int]] = None, k=None, method: str = "wilcoxon",
                      tie_correct: bool = False, n_genes: Optional[int] = None,
                      rankby_abs: bool = False) -> List[Dict[str, np.ndarray]]:
    """Marker genes of every group of every slide against the rest of its slide.

    ``x``: row-stacked (rows, G), float32 or float64, host or device.  ``offsets``: the S + 1 slide boundaries (default: one
    slide).  ``labels``: (rows,) integers, within slide s in [0, k[s]), -1 = not part of the analysis.  ``k``: groups per
    slide (an int or S of them; default: the largest label + 1).  Returns one dict per slide of numpy arrays: the ordered
    (k, n_genes) ``names`` (int64 gene indices), ``scores``, ``pvals``, ``pvals_adj``, ``neglog10_pvals``,
    ``logfoldchanges``; the gene-order (k, G) ``means``, ``vars``, ``means_rest``, ``vars_rest``, ``pts``, ``pts_rest`` (and
    ``nnz``, ``nnz_rest``, ``rank_sums2``, the ``full_*`` columns); ``tie_terms`` (G,); ``group_sizes`` (k,); ``n_valid``."""
    d = rank_genes_groups_device(x, labels, offsets, k, method, tie_correct, n_genes, rankby_abs)
    goff = d["group_offsets"]
    host = {key: v.cpu().numpy() for key, v in d.items() if isinstance(v, Tensor)}
    out = []
    for s in range(goff.size - 1):
        a, b = int(goff[s]), int(goff[s + 1])
        one = {key: v[a:b] for key, v in host.items() if key not in ("tie_terms", "n_valid")}
        one["tie_terms"], one["n_valid"] = host["tie_terms"][s], int(host["n_valid"][s])
        out.append(one)
    return out


def encode_slides(labels: Sequence[Sequence], undetermined="undetermined"):
    """One label vector per slide -> (stacked int32 codes with -1 for ``undetermined``, k per slide, the sorted distinct
    labels per slide).  Integer vectors are taken as group ids as they are (-1 stays -1)."""
    codes, ks, cats = [], [], []
    for i, lab in enumerate(labels):
        a = np.asarray(lab)
        if a.ndim != 1:
            raise ValueError(f"labels[{i}]: expected a 1-D vector, got shape {a.shape}")
        if np.issubdtype(a.dtype, np.integer):
            codes.append(a.astype(np.int32))
            ks.append(max(1, int(a.max(initial=-1)) + 1))
            cats.append(np.arange(ks[-1]))
        else:
            idx, c, k = cluster.encode_labels(a, undetermined)
            full = np.full(a.size, -1, dtype=np.int32)
            full[idx] = c
            codes.append(full)
            ks.append(k)
            cats.append(np.unique(a[idx]))
    return np.concatenate(codes) if codes else np.zeros(0, np.int32), np.asarray(ks, dtype=np.int64), cats


def marker_slides(matrices: Sequence[ArrayLike], labels: Sequence[Sequence], undetermined="undetermined",
                  **kw) -> List[Dict[str, np.ndarray]]:
    """``rank_genes_groups`` of one (spots, genes) matrix and one label vector per slide.  String labels are encoded by
    ``cluster.encode_labels`` (sorted distinct values; ``undetermined`` becomes -1); every slide's dict also carries
    ``categories``, the label of each group."""
    if len(matrices) != len(labels) or not len(matrices):
        raise ValueError(f"need one label vector per slide and >= 1 slide; got {len(matrices)} and {len(labels)}")
    for i, (m, lab) in enumerate(zip(matrices, labels)):
        if len(m.shape) != 2 or m.shape[0] != len(lab):
            raise ValueError(f"slide {i}: matrix {tuple(m.shape)} and {len(lab)} labels do not match")
    codes, ks, cats = encode_slides(labels, undetermined)
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    check_problem((int(off[-1]), int(matrices[0].shape[1])), off, ks)
    dev = device("markers")
    x, off = stack_rows(matrices, "matrices", dev)
    res = rank_genes_groups(x, codes, off, ks, **kw)
    for r, c in zip(res, cats):
        r["categories"] = c
    return res


def top_markers(res: Sequence[Dict[str, np.ndarray]], slide: int, n: int = TOP_N) -> np.ndarray:
    """The distinct gene indices among the first ``n`` markers of every group of one slide, ascending: what
    ``bleep.score(..., markers=...)`` takes."""
    names = res[slide]["names"]
    return np.unique(names[:, :max(1, min(int(n), names.shape[1]))])


def recovery_table(pred_names: np.ndarray, true_names: np.ndarray):
    """Host set arithmetic on two (k, n_top) index arrays: overlap count and Jaccard index per group."""
    overlap = np.array([np.intersect1d(a, b).size for a, b in zip(pred_names, true_names)], dtype=np.int64)
    union = np.array([np.union1d(a, b).size for a, b in zip(pred_names, true_names)], dtype=np.int64)
    return overlap, overlap / union


def marker_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], labels: Sequence[Sequence],
                    n_top: int = TOP_N, **kw) -> Dict[str, object]:
    """Do the predicted values recover the marker genes of the measured ones?  The top ``n_top`` markers of every group are
    taken from the predicted and from the measured matrix under the same labels.  Returns ``overlap`` and ``jaccard`` (one
    (k,) array per slide), ``mean_overlap``, ``mean_jaccard`` (over all groups of all slides), ``n_top`` and the two
    results ``pred`` / ``true``."""
    if len(preds) != len(trues):
        raise ValueError(f"need one measured matrix per prediction; got {len(preds)} and {len(trues)}")
    for i, (p, t) in enumerate(zip(preds, trues)):
        if tuple(p.shape) != tuple(t.shape):
            raise ValueError(f"slide {i}: pred {tuple(p.shape)} and true {tuple(t.shape)} differ in shape")
    if isinstance(n_top, bool) or not isinstance(n_top, (int, np.integer)) or n_top < 1:
        raise ValueError(f"n_top must be a positive integer, got {n_top!r}")
    rp = marker_slides(preds, labels, n_genes=int(n_top), **kw)
    rt = marker_slides(trues, labels, n_genes=int(n_top), **kw)
    tables = [recovery_table(a["names"], b["names"]) for a, b in zip(rp, rt)]
    overlap, jaccard = [t[0] for t in tables], [t[1] for t in tables]
    return {"overlap": overlap, "jaccard": jaccard, "mean_overlap": float(np.concatenate(overlap).mean()),
            "mean_jaccard": float(np.concatenate(jaccard).mean()), "n_top": int(rp[0]["names"].shape[1]), "pred": rp,
            "true": rt}


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.markers",
                                description="Rank the marker genes of every spot group (sc.tl.rank_genes_groups) and score "
                                            "how well predictions recover the measured markers")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--labels", required=True, nargs="+",
                   help="one label vector per slide: leiden.npy as the Leiden CLI writes it, or an annotation array")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery table")
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the gene index)")
    p.add_argument("--method", default="wilcoxon", choices=sorted(METHODS))
    p.add_argument("--tie_correct", action="store_true")
    p.add_argument("--rankby_abs", action="store_true")
    p.add_argument("--top", type=int, default=TOP_N, help="markers per group to print and to score the recovery on")
    p.add_argument("--out_dir", required=True, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if len(a.labels) != len(a.pred):
        p.error(f"{len(a.labels)} --labels files for {len(a.pred)} --pred files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def format_markers(res: Sequence[Dict[str, np.ndarray]], genes: Optional[Sequence[str]], top: int) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        for g in range(r["names"].shape[0]):
            cells = [f"{genes[j] if genes is not None else j} ({r['scores'][g, i]:.3f}, {r['logfoldchanges'][g, i]:.3f})"
                     for i, j in enumerate(r["names"][g, :top])]
            lines.append(f"slide {s} group {r['categories'][g]} (n = {int(r['group_sizes'][g])}): " + ", ".join(cells))
    return lines


def format_recovery(rec: Dict[str, object]) -> List[str]:
    lines = []
    for s, (o, j) in enumerate(zip(rec["overlap"], rec["jaccard"])):
        for g in range(o.size):
            lines.append(f"slide {s} group {rec['pred'][s]['categories'][g]}: overlap {int(o[g])} / {rec['n_top']}, "
                         f"Jaccard {j[g]:.4f}")
    lines.append(f"mean overlap {rec['mean_overlap']:.4f} / {rec['n_top']}, mean Jaccard {rec['mean_jaccard']:.4f}")
    return lines


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    labels = [np.load(f, allow_pickle=True).reshape(-1) for f in args.labels]
    G = preds[0].shape[1]
    genes = None
    if args.genes is not None:
        genes = [str(v) for v in np.load(args.genes, allow_pickle=True).reshape(-1)]
        if len(genes) != G:
            raise ValueError(f"{args.genes}: {len(genes)} gene names for {G} genes")
    kw = dict(method=args.method, tie_correct=args.tie_correct, rankby_abs=args.rankby_abs)
    res = marker_slides(preds, labels, **kw)
    top = min(args.top, G)
    print("\n".join(format_markers(res, genes, top)))
    for i, r in enumerate(res):
        d = os.path.join(args.out_dir, str(i))
        os.makedirs(d, exist_ok=True)
        np.savez(os.path.join(d, OUT_FILE), **{key: np.asarray(v) for key, v in r.items()})
    if args.true is not None:
        trues = load_gene_major(args.true)
        print("\n".join(format_recovery(marker_recovery(preds, trues, labels, n_top=top, **kw))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
