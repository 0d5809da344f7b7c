"""Rank agreement of expression predictions on the MI355X: Spearman's rho and Kendall's tau-b per gene and per spot, the
two values of ``func`` the reference's ``get_R`` takes besides ``pearsonr``, on both of its ``dim``s.

Reference (paths relative to /root/reference/):
  get_R              utils.py:52-65: ``get_R(data1, data2, dim=1, func=pearsonr)``; ``dim=1`` correlates every gene over
                     the spots, ``dim=0`` every spot over the genes
  spearmanr          imported beside pearsonr by baselines/His2ST/predict.py:7, tutorial.ipynb, run_trained_models.ipynb
  scipy              ``scipy.stats.spearmanr`` (average ranks; p from Student's t, n - 2 degrees of freedom) and
                     ``scipy.stats.kendalltau(method="asymptotic")`` (tau-b; the normal approximation with tie corrections)

All slides are ranked by ONE ``mcl_rank_stats`` call (csrc/rank.hip: LDS bitonic sorts with tie runs, exact integer sums,
the O(n^2) pair walk for Kendall), finished by ``mcl_rank_finish``; Spearman's p is ``mcl_pearson_pvalue`` on rho.  Every
sum is an integer, so a slide inside a batch, alone, or with its rows permuted gives the same bits.  A vector holds at most
16384 elements when pred and true are both float32, 8192 when either is float64 (the LDS plan of one workgroup); at most
16384 genes, 65535 slides.  Kendall's exact small-sample p-value, tau-c, weighted tau and partial correlations are not
computed.  No CPU fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.rank --pred P1.npy ... --true T1.npy ... [--genes names.npy] [--no_tau] [--spots] [--top 7]
                                [--json OUT] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import evaluate, genes
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_flag, device, empty, json_value, matrix, nanmean, paired_offsets,
                      stack_rows, upload, validate_offsets, write_json)
from ._lib import call

N_HEG = evaluate.N_HEG
TOP_N = genes.TOP_N
MAX_ELEMENTS_F32 = 16384      # mcl_rank_max_elements(0, 0)
MAX_ELEMENTS_F64 = 8192       # with a float64 side
MAX_GENES = 16384
MAX_SLIDES = 65535
N_INTS = 12
INT_NAMES = ("n", "Sxy", "Tx", "Ty", "xtie", "ytie", "x0", "y0", "x1", "y1", "joint", "s")
AXES = {"genes": 0, "spots": 1}
SUMMARY_KEYS = ("heg_spearman", "hvg_spearman", "heg_kendall", "hvg_kendall")
_PVALUE_CHUNK = 1 << 20       # mcl_pearson_pvalue's column limit


def max_elements(pred_dtype: torch.dtype, true_dtype: torch.dtype) -> int:
    """The longest vector one call ranks for these input dtypes."""
    return MAX_ELEMENTS_F32 if pred_dtype == true_dtype == torch.float32 else MAX_ELEMENTS_F64


def check_limits(sizes: Sequence[int], G: int, pred_dtype: torch.dtype, true_dtype: torch.dtype, axis: str) -> None:
    """The limits of one call, checked on the host before anything is launched.  ``sizes``: the spots of every slide."""
    if axis not in AXES:
        raise ValueError(f"axis must be 'genes' or 'spots', got {axis!r}")
    for dt, name in ((pred_dtype, "pred"), (true_dtype, "true")):
        if dt not in FLOAT_CODE:
            raise ValueError(f"{name}: expected float32 or float64, got {dt}")
    lim = max_elements(pred_dtype, true_dtype)
    what = "float32 inputs" if lim == MAX_ELEMENTS_F32 else "a float64 input"
    if G < 1 or G > MAX_GENES:
        raise ValueError(f"{G} genes; a call ranks 1 .. {MAX_GENES}")
    if axis == "spots":
        if G < 2 or G > lim:
            raise ValueError(f"axis='spots' ranks vectors of G = {G} genes; 2 .. {lim} with {what}")
        return
    if len(sizes) > MAX_SLIDES:
        raise ValueError(f"at most {MAX_SLIDES} slides per call, got {len(sizes)}")
    for s, n in enumerate(sizes):
        if n < 2 or n > lim:
            raise ValueError(f"slide {s} has {n} spots; a vector holds 2 .. {lim} elements with {what}")


def _input(t: Tensor, name: str) -> None:
    if not isinstance(t, Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype not in FLOAT_CODE or \
            (t.stride(1) != 1 and t.shape[1] != 1) or t.stride(0) < t.shape[1]:
        raise RuntimeError(f"{name}: expected a row-major float32 / float64 device matrix")


def _spearman_p(rho: Tensor, offsets: Sequence[int]) -> Tuple[Tensor, Tensor]:
    """p and -log10 p of rho (S, G) for slides of ``offsets``' sizes: mcl_pearson_pvalue, in column chunks it takes."""
    S, G = rho.shape
    if G <= _PVALUE_CHUNK:
        return genes.pvalues_device(rho, offsets)
    e = empty(rho.device)
    p, nl = e((S, G), torch.float64), e((S, G), torch.float64)
    for lo in range(0, G, _PVALUE_CHUNK):                     # (only a one-slide row of more than 2^20 spots gets here)
        pc, nc = genes.pvalues_device(rho[:, lo:lo + _PVALUE_CHUNK].clone(), offsets)
        p[:, lo:lo + _PVALUE_CHUNK].copy_(pc)
        nl[:, lo:lo + _PVALUE_CHUNK].copy_(nc)
    return p, nl


def rank_device(pred: Tensor, true: Tensor, offsets: Optional[Sequence[int]], axis: str = "genes",
                tau: bool = True) -> Dict[str, Tensor]:
    """One ``mcl_rank_stats`` + ``mcl_rank_finish`` + ``mcl_pearson_pvalue`` on row-stacked device matrices (rows, G), each
    float32 or float64 with its own row stride.  ``axis="genes"``: one problem per (slide, gene) over the slide's spots,
    ``offsets`` the S + 1 slide boundaries (host integers; None = one slide); outputs are (S, G).  ``axis="spots"``: one
    problem per row over the G genes, ``offsets`` must be None; outputs are (rows,).  Device tensors: ``ints`` (..., 12) int64 (``INT_NAMES``),
    ``spearman``, ``spearman_pval``, ``spearman_neglog10_pval`` and, with ``tau``, ``kendall``, ``kendall_pval``,
    ``kendall_neglog10_pval`` (float64; NaN where a side is constant, Kendall's p also at n < 3).  A NaN or infinite input
    raises ``ValueError`` naming the slide (the row for ``axis="spots"``); the one synchronisation is that check."""
    tau = check_flag(tau, "tau")
    if axis not in AXES:
        raise ValueError(f"axis must be 'genes' or 'spots', got {axis!r}")
    if not isinstance(pred, Tensor) or not isinstance(true, Tensor) or pred.dim() != 2 or tuple(pred.shape) != tuple(true.shape):
        raise ValueError("pred and true must be 2-D matrices of one shape")
    rows, G = int(pred.shape[0]), int(pred.shape[1])
    if axis == "genes":
        off = validate_offsets(offsets, rows, 2, None, MAX_SLIDES, none_is_one=True, noun="slide")
        sizes = np.diff(off).tolist()
    else:
        if offsets is not None:
            raise ValueError("axis='spots' ranks every row on its own: offsets must be None")
        if rows < 1:
            raise ValueError("axis='spots' needs at least one row")
        off, sizes = np.array([0, G], dtype=np.int64), [G]
    check_limits(sizes, G, pred.dtype, true.dtype, axis)
    device("rank")
    _input(pred, "pred")
    _input(true, "true")
    S, max_n = len(sizes), int(max(sizes))
    problems = S * G if axis == "genes" else rows
    shape = (S, G) if axis == "genes" else (rows,)
    e = empty(pred.device)
    ints, status = e(shape + (N_INTS,), torch.int64), e((S, 3), torch.int32)
    off_d = upload(off, pred.device)
    call("mcl_rank_stats", pred, pred.stride(0), FLOAT_CODE[pred.dtype], true, true.stride(0), FLOAT_CODE[true.dtype],
         off_d, S, rows, G, max_n, AXES[axis], tau, ints, status)
    rho = e(shape, torch.float64)
    tb, tp, tnl = (e(shape, torch.float64) for _ in range(3)) if tau else (None, None, None)
    call("mcl_rank_finish", ints, problems, tau, rho, tb, tp, tnl)
    p, nl = _spearman_p(rho.view(S, -1), off)
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad[:, 2].any():
        raise ValueError(f"slide {int(np.flatnonzero(bad[:, 2])[0])}: offsets the device refuses")
    if bad[:, 0].any():
        s = int(np.flatnonzero(bad[:, 0])[0])
        where = f"slide {s}" if axis == "genes" else f"row {0x7fffffff - int(bad[s, 1])}"
        raise ValueError(f"pred / true: {where} holds non-finite values ({int(bad[:, 0].sum())} in the call)")
    out = {"ints": ints, "spearman": rho, "spearman_pval": p.view(shape), "spearman_neglog10_pval": nl.view(shape)}
    if tau:
        out.update(kendall=tb, kendall_pval=tp, kendall_neglog10_pval=tnl)
    return out


def _float_dtype(a: ArrayLike) -> torch.dtype:
    """The dtype ``a`` reaches the device with: its own when float32 / float64, else (host arrays only) float64."""
    if isinstance(a, Tensor):
        return a.dtype if a.dtype in FLOAT_CODE or a.is_cuda else torch.float64
    return torch.float32 if np.asarray(a).dtype == np.float32 else torch.float64


def _stacked_dtype(parts: Sequence[ArrayLike]) -> torch.dtype:
    """The dtype ``stack_rows`` gives these parts: their own when they share float32 / float64, else float64."""
    dts = {_float_dtype(p) for p in parts}
    dt = dts.pop() if len(dts) == 1 else torch.float64
    return dt if dt in FLOAT_CODE else torch.float64


def _host(d: Dict[str, Tensor]) -> Dict[str, np.ndarray]:
    return {k: v.cpu().numpy() for k, v in d.items()}


def score_folds(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], n_heg: int = N_HEG,
                tau: bool = True) -> Dict[str, object]:
    """Ranks every fold's (spots, genes) prediction against its ground truth in one call.  Returns ``folds``: per fold
    ``spearman`` (G,), ``spearman_pval``, ``spearman_neglog10_pval``, with ``tau`` also ``kendall``, ``kendall_pval``,
    ``kendall_neglog10_pval``; ``heg_spearman`` / ``heg_kendall``: the mean over the fold's ``heg_genes`` (the genes
    ``evaluate.score_folds`` names; a NaN among them makes it NaN, as its ``heg_pcc``), ``hvg_spearman`` /
    ``hvg_kendall``: the mean over the ``n_valid`` genes that are defined (the Kendall entries are NaN without ``tau``);
    and ``heg_spearman``, ``hvg_spearman``, ``heg_kendall``, ``hvg_kendall``: ``np.mean`` over the folds, as
    ``evaluate.score_folds`` reports its PCCs.  ``spearman`` and ``spearman_neglog10_pval`` stacked over the folds are the
    (S, G) matrices ``genes.rank_genes`` takes."""
    tau = check_flag(tau, "tau")
    offsets = paired_offsets(preds, trues, "fold")
    G = int(preds[0].shape[1])
    check_limits(np.diff(offsets).tolist(), G, _stacked_dtype(preds), _stacked_dtype(trues), "genes")
    n_heg = min(int(n_heg), G)
    if n_heg < 1:
        raise ValueError("n_heg must be >= 1")
    dev = device("rank")
    pred = stack_rows(preds, "preds", dev, convert_on_device=True)[0]
    true = stack_rows(trues, "trues", dev, convert_on_device=True)[0]
    heg = evaluate.metrics_device(pred, true, offsets, n_heg)["heg"]
    d = rank_device(pred, true, offsets, "genes", tau)
    S = len(preds)
    summary = empty(dev)((S, 5), torch.float64)
    call("mcl_rank_summary", d["spearman"], d.get("kendall"), heg, S, G, n_heg, summary)
    h, summ, heg_h = _host({k: v for k, v in d.items() if k != "ints"}), summary.cpu().numpy(), heg.cpu().numpy()
    folds = []
    for s in range(S):
        f: Dict[str, object] = {k: v[s] for k, v in h.items()}
        f.update(heg_spearman=float(summ[s, 0]), hvg_spearman=float(summ[s, 1]), heg_kendall=float(summ[s, 2]),
                 hvg_kendall=float(summ[s, 3]), n_valid=int(summ[s, 4]), heg_genes=heg_h[s])
        folds.append(f)
    out: Dict[str, object] = {"folds": folds}
    for k in SUMMARY_KEYS:
        out[k] = float(np.mean([f[k] for f in folds]))
    return out


def score(pred: ArrayLike, true: ArrayLike, n_heg: int = N_HEG, tau: bool = True) -> Dict[str, object]:
    """One fold, as an entry of ``score_folds(...)["folds"]``."""
    return score_folds([pred], [true], n_heg, tau)["folds"][0]


def _pair(pred, true, dev: torch.device) -> Tuple[Tensor, Tensor]:
    accept = tuple(FLOAT_CODE)
    return matrix(pred, "pred", dev, accept, torch.float64), matrix(true, "true", dev, accept, torch.float64)


def _shapes(pred, true) -> Tuple[int, int]:
    if len(pred.shape) != 2 or tuple(pred.shape) != tuple(true.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and true {tuple(true.shape)} must be 2-D and of one shape")
    return int(pred.shape[0]), int(pred.shape[1])


def spot_rank(pred: ArrayLike, true: ArrayLike, tau: bool = True) -> Dict[str, np.ndarray]:
    """The ``dim=0`` form for a whole stacked (spots, genes) matrix: every spot's prediction ranked against its ground
    truth over the genes.  (rows,) arrays ``spearman``, ``spearman_pval``, ``spearman_neglog10_pval`` and, with ``tau``,
    ``kendall``, ``kendall_pval``, ``kendall_neglog10_pval``."""
    tau = check_flag(tau, "tau")
    rows, G = _shapes(pred, true)
    check_limits([G], G, _float_dtype(pred), _float_dtype(true), "spots")
    if rows < 1:
        raise ValueError("need at least one spot")
    dev = device("rank")
    p, t = _pair(pred, true, dev)
    d = rank_device(p, t, None, "spots", tau)
    return _host({k: v for k, v in d.items() if k != "ints"})


def get_R(pred, true, dim: int = 1, func: str = "spearmanr") -> Tuple[np.ndarray, np.ndarray]:
    """The reference's ``get_R(data1, data2, dim, func)`` for ``func`` = ``"spearmanr"`` or ``"kendalltau"`` (the names of
    the scipy functions, or the functions themselves): ``(r, p)`` arrays over the genes (``dim=1``) or the spots
    (``dim=0``).  ``pred`` / ``true``: (spots, genes) arrays, or objects whose ``.X`` is one (AnnData)."""
    name = getattr(func, "__name__", func)
    if name not in ("spearmanr", "kendalltau"):
        raise ValueError(f"func must be 'spearmanr' or 'kendalltau', got {func!r} (pearsonr: evaluate.gene_pcc / genes)")
    if dim not in (0, 1) or isinstance(dim, bool):
        raise ValueError(f"dim must be 0 or 1, got {dim!r}")
    pred, true = getattr(pred, "X", pred), getattr(true, "X", true)
    want_tau = name == "kendalltau"
    key = "kendall" if want_tau else "spearman"
    if dim == 0:
        res = spot_rank(pred, true, tau=want_tau)
    else:
        rows, G = _shapes(pred, true)
        check_limits([rows], G, _float_dtype(pred), _float_dtype(true), "genes")
        dev = device("rank")
        p, t = _pair(pred, true, dev)
        res = {k: v[0] for k, v in _host({k: v for k, v in rank_device(p, t, None, "genes", want_tau).items()
                                          if k != "ints"}).items()}
    return res[key], res[key + "_pval"]


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.rank",
                                description="Score predictions by rank: Spearman's rho and Kendall's tau-b per gene "
                                            "(the reference's get_R with func=spearmanr / kendalltau)")
    p.add_argument("--pred", required=True, nargs="+", help=f"one {evaluate.PRED_FILE} per slide, (G, N), in slide order")
    p.add_argument("--true", required=True, nargs="+", help="one preprocessed_matrix.npy per slide, (G, N), same order")
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the gene index)")
    p.add_argument("--no_tau", action="store_true", help="skip Kendall's tau (the O(n^2) pair walk)")
    p.add_argument("--spots", action="store_true", help="also rank every spot over the genes (get_R's dim=0)")
    p.add_argument("--top", type=int, default=TOP_N, help="how many genes to report")
    p.add_argument("--json", default=None, help="also write per-fold and average scores to this file")
    p.add_argument("--out_dir", default=None, metavar="D",
                   help="also write every slide's per-gene (and with --spots per-spot) arrays to D/<slide index>/")
    a = p.parse_args(argv)
    if len(a.pred) != len(a.true):
        p.error(f"{len(a.pred)} --pred files for {len(a.true)} --true files")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def format_report(res: Dict[str, object], tau: bool = True) -> str:
    """Per fold and on average the lines the evaluation scripts print for PCC, with Spearman and Kendall in its place."""
    names = [("heg_spearman", "heg spearman"), ("hvg_spearman", "hvg spearman")]
    if tau:
        names += [("heg_kendall", "heg kendall"), ("hvg_kendall", "hvg kendall")]
    lines = [f"fold {i}: " + ", ".join(f"{label}: {f[k]:.4f}" for k, label in names) for i, f in enumerate(res["folds"])]
    return "\n".join(lines + [f"avg {label}: {res[k]:.4f}" for k, label in names])


def top_genes(res: Dict[str, object], gene_names: Optional[Sequence[str]], top_n: int) -> List[Dict[str, object]]:
    """The genes by descending mean rho over the folds that define it (equal means by gene index, undefined genes last)."""
    rho = np.stack([f["spearman"] for f in res["folds"]])
    mean = np.array([nanmean(rho[:, g]) for g in range(rho.shape[1])])
    order = np.lexsort((np.arange(mean.size), -np.where(np.isnan(mean), -np.inf, mean), np.isnan(mean)))
    return [{"gene": int(g), "gene_name": str(gene_names[g]) if gene_names is not None else str(int(g)),
             "mean_spearman": float(mean[g]), "best_slide": int(np.nanargmax(rho[:, g])) if not np.isnan(mean[g]) else -1}
            for g in order[:max(1, min(int(top_n), mean.size))]]


def format_top(top: Sequence[Dict[str, object]]) -> List[str]:
    return [f"Gene: {t['gene_name']}, mean Spearman rho: {t['mean_spearman']:.4f}, best in slide {t['best_slide']}" for t in top]


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds, trues = genes.load_slides(args.pred, args.true)
    names = genes.load_gene_names(args.genes, preds[0].shape[1])
    tau = not args.no_tau
    res = score_folds(preds, trues, tau=tau)
    print(format_report(res, tau))
    top = top_genes(res, names, args.top)
    print("\n".join(format_top(top)))
    spots = [spot_rank(p, t, tau) for p, t in zip(preds, trues)] if args.spots else None
    if spots is not None:
        print(f"avg spot spearman: {float(np.mean([nanmean(s['spearman']) for s in spots])):.4f}")
    if args.out_dir:
        for i, f in enumerate(res["folds"]):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            for k, v in f.items():
                if isinstance(v, np.ndarray):
                    np.save(os.path.join(d, f"gene_{k}.npy"), v)
            for k, v in (spots[i] if spots is not None else {}).items():
                np.save(os.path.join(d, f"spot_{k}.npy"), v)
    if args.json:
        doc = {k: json_value(res[k]) for k in SUMMARY_KEYS}
        doc.update(tau=tau, top=top, folds=[{k: json_value(v) for k, v in f.items()} for f in res["folds"]])
        write_json(args.json, doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
