"""BLEEP's evaluation protocol on the MI355X: the prediction methods, the scoring block and the gene-gene-correlation
matrices of the baseline mclSTExp extends, on the device -- what a model trained with ``loss_kind="bleep"`` is compared by.

Reference (paths relative to /root/reference/baselines/Bleep/):
  prediction methods   BLEEP_inference.ipynb cell 5: ``simple`` (top 1), ``average`` (top 50), ``weighted_average`` (top 50,
                       ``w = exp(-(d - d_0 + 1))``) -> ``retrieval.combine_device`` / ``predict_expression(method=...)``
  scoring block        cell 5: mean correlation across cells, number of non-NaN genes, max gene correlation, mean correlation
                       of the 50 highly expressed (``np.sum``) and the 50 highly variable (``np.var``) genes and of the
                       marker genes
  GGC matrices         cell 7: ``np.corrcoef`` of the 50 genes of largest mean, ground truth and prediction, both reordered by
                       the leaves of ``hierarchy.linkage(corr_gt, 'ward')``

All folds are scored by ONE ``mcl_expr_metrics`` + ``mcl_cell_pearson`` + ``mcl_bleep_summary`` sequence (fp64,
deterministic: a fold scored inside a batch is bit-identical to the same fold scored alone).  The notebook compacts the gene
correlations (``corr = corr[~np.isnan(corr)]``) BEFORE it indexes them with gene indices of the full gene axis: with a NaN
gene the indices shift and may run out of range.  The default here indexes the full vector (a NaN gene among the chosen ones
makes that mean NaN); ``notebook_indexing=True`` reproduces the notebook's arithmetic, ``IndexError`` included.  No CPU
fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.bleep --embedding_dir DIR --expressions F1.npy F2.npy ... --method average [--top_k K]
                                 [--markers NAMES ... --genes names.npy] [--json OUT] [--save_pred DIR] [--ggc OUT.npz]
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import evaluate, retrieval
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, device, empty, matrix, paired_offsets, stack_rows, upload,
                      validate_offsets, write_json)
from ._lib import call

N_TOP = 50
METHOD_TOP_K = {"simple": 1, "average": 50, "weighted_average": 50}          # the notebook's top_k per method
SUMMARY_KEYS = ("cell_mean", "max_r", "heg_mean", "hvg_mean", "marker_mean")
COUNT_KEYS = ("n_cells_valid", "n_genes_valid")


def _markers(markers: Optional[Sequence[int]], G: int) -> np.ndarray:
    if markers is None:
        return np.zeros((0,), dtype=np.int32)
    m = np.asarray(markers)
    if m.ndim != 1 or (m.size and not np.issubdtype(m.dtype, np.integer)):
        raise ValueError(f"markers must be a 1-D list of integer gene indices, got {markers!r}")
    if m.size and (int(m.min()) < 0 or int(m.max()) >= G):
        raise IndexError(f"marker gene index out of range for {G} genes")
    return m.astype(np.int32)


def summary_device(pred: Tensor, true: Tensor, offsets: Sequence[int], markers: Optional[Sequence[int]] = None,
                   n_top: int = N_TOP) -> Dict[str, Tensor]:
    """The scoring sequence on row-stacked device matrices.  Device tensors: ``r`` (S, G), ``r_cell`` (rows,), ``gene_sum``
    and ``gene_var`` (S, G), ``top_sum`` and ``top_var`` (S, min(n_top, G)) int64 best first, ``summary`` (S, 7) =
    cell_mean, n_cells_valid, n_genes_valid, max_r, heg_mean, hvg_mean, marker_mean."""
    rows, G = pred.shape
    n_top = min(int(n_top), G)
    if n_top < 1:
        raise ValueError("n_top must be >= 1")
    mk = _markers(markers, G)
    r = evaluate.metrics_device(pred, true, offsets, n_top)["r"]         # (checks shapes, dtypes, offsets)
    S = r.shape[0]
    dev = pred.device
    off_d = upload(np.asarray(offsets, dtype=np.int64), dev)
    mk_d = upload(mk, dev) if mk.size else None
    e = empty(dev)
    r_cell = e((rows,), torch.float64)
    gene_sum, gene_var, summary = e((S, G), torch.float64), e((S, G), torch.float64), e((S, 7), torch.float64)
    top_sum, top_var = e((S, n_top), torch.int64), e((S, n_top), torch.int64)
    call("mcl_cell_pearson", pred, pred.stride(0), FLOAT_CODE[pred.dtype],
         true, true.stride(0), FLOAT_CODE[true.dtype], rows, G, r_cell)
    call("mcl_bleep_summary", true, true.stride(0), FLOAT_CODE[true.dtype], off_d, S, G,
         n_top, r, r_cell, mk_d, int(mk.size), gene_sum, gene_var, top_sum, top_var, summary)
    return {"r": r, "r_cell": r_cell, "gene_sum": gene_sum, "gene_var": gene_var, "top_sum": top_sum, "top_var": top_var,
            "summary": summary}


def notebook_means(pcc: np.ndarray, heg: np.ndarray, hvg: np.ndarray, markers: np.ndarray) -> Tuple[float, float, float]:
    """(heg_mean, hvg_mean, marker_mean) by the notebook's own arithmetic: the NaN genes are dropped first, then the
    compacted vector is indexed with gene indices of the FULL axis (ascending order, as ``np.argsort(...)[-50:]`` lists
    them).  Raises numpy's ``IndexError`` when a shifted index runs out of range."""
    corr = pcc[~np.isnan(pcc)]
    with np.errstate(invalid="ignore"):
        mark = float(np.mean(corr[markers])) if markers.size else float("nan")
        return float(np.mean(corr[heg[::-1]])), float(np.mean(corr[hvg[::-1]])), mark


def score_folds(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], markers: Optional[Sequence[int]] = None,
                n_top: int = N_TOP, notebook_indexing: bool = False) -> Dict[str, object]:
    """Scores every fold's (spots, genes) prediction against its ground truth in one scoring sequence.  Returns ``folds``:
    per-fold dicts as ``score`` returns them, and the ``np.mean`` over the folds of ``cell_mean``, ``max_r``, ``heg_mean``,
    ``hvg_mean`` and ``marker_mean``."""
    offsets = paired_offsets(preds, trues, "fold")
    G = int(preds[0].shape[1])
    mk = _markers(markers, G)
    dev = device("bleep")
    d = summary_device(stack_rows(preds, "preds", dev, convert_on_device=True)[0],
                       stack_rows(trues, "trues", dev, convert_on_device=True)[0], offsets, mk, n_top)
    r, r_cell, summ = d["r"].cpu().numpy(), d["r_cell"].cpu().numpy(), d["summary"].cpu().numpy()
    top_sum, top_var = d["top_sum"].cpu().numpy(), d["top_var"].cpu().numpy()
    folds = []
    for s in range(len(preds)):
        f = {"cell_mean": float(summ[s, 0]), "n_cells_valid": int(summ[s, 1]), "n_genes_valid": int(summ[s, 2]),
             "max_r": float(summ[s, 3]), "heg_mean": float(summ[s, 4]), "hvg_mean": float(summ[s, 5]),
             "marker_mean": float(summ[s, 6]), "pcc": r[s], "cell_pcc": r_cell[offsets[s]:offsets[s + 1]],
             "heg_genes": top_sum[s], "hvg_genes": top_var[s]}
        if notebook_indexing:
            f["heg_mean"], f["hvg_mean"], f["marker_mean"] = notebook_means(r[s], top_sum[s], top_var[s], mk)
        folds.append(f)
    out: Dict[str, object] = {"folds": folds}
    for k in SUMMARY_KEYS:
        out[k] = float(np.mean([f[k] for f in folds]))
    return out


def score(pred: ArrayLike, true: ArrayLike, markers: Optional[Sequence[int]] = None, n_top: int = N_TOP,
          notebook_indexing: bool = False) -> Dict[str, object]:
    """One fold, cell 5's scoring block: ``cell_mean`` ("Mean correlation across cells"), ``n_cells_valid``,
    ``n_genes_valid`` ("number of non-zero genes"), ``max_r``, ``heg_mean``, ``hvg_mean``, ``marker_mean`` (NaN without
    ``markers``), ``pcc`` (G,), ``cell_pcc`` (spots,), ``heg_genes`` / ``hvg_genes`` (min(n_top, G),) int64: the genes of
    largest ``np.sum`` / ``np.var`` of the ground truth, best first, equal values by descending gene index (the tail of a
    stable argsort read backwards)."""
    return score_folds([pred], [true], markers, n_top, notebook_indexing)["folds"][0]


def _cat_rows(parts: Sequence[ArrayLike]) -> Tensor:
    return stack_rows(list(parts), "slides", device("bleep"), convert_on_device=True)[0]


def predict_device(spot_key: ArrayLike, expression_key: ArrayLike, image_query: ArrayLike, method: str,
                   top_k: Optional[int] = None) -> Tensor:
    """Retrieval -> BLEEP's combination for one fold; the (Q, G) fp32 prediction stays on the device."""
    if method not in METHOD_TOP_K:
        raise ValueError(f"method must be one of {sorted(METHOD_TOP_K)}, got {method!r}")
    key = retrieval.to_device(spot_key, "spot_key")
    qry = retrieval.to_device(image_query, "image_query")
    _, idx = retrieval.find_matches_device(key, qry, METHOD_TOP_K[method] if top_k is None else int(top_k))
    return retrieval.combine_device(key, expression_key, qry, idx, method)[1]


def leave_one_slide_out(image_embeddings: Optional[Sequence[ArrayLike]], spot_embeddings: Optional[Sequence[ArrayLike]],
                        expressions: Sequence[ArrayLike], method: str = "average", top_k: Optional[int] = None,
                        per_fold: Optional[Callable[[int], Tuple[Sequence[ArrayLike], Sequence[ArrayLike]]]] = None,
                        markers: Optional[Sequence[int]] = None, return_preds: bool = False) -> Dict[str, object]:
    """BLEEP's fold protocol (cell 4: the queries are slide f's image embeddings, the keys every other slide's spot
    embeddings and expressions) with the notebook's defaults: ``top_k`` 1 for ``simple``, 50 otherwise.  Lists hold one
    (spots, ·) array per slide; ``per_fold(f)`` -> (image_embeddings, spot_embeddings) supplies fold-specific embeddings.
    Predictions stay on the device between retrieval and scoring; all folds are scored at once.  Returns what
    ``score_folds`` returns; with ``return_preds`` also ``preds``: every slide's (spots, genes) prediction, numpy."""
    n = len(expressions)
    if n < 2:
        raise ValueError("leave-one-slide-out needs >= 2 slides")
    if method not in METHOD_TOP_K:
        raise ValueError(f"method must be one of {sorted(METHOD_TOP_K)}, got {method!r}")
    preds = []
    for f in range(n):
        img, spot = per_fold(f) if per_fold is not None else (image_embeddings, spot_embeddings)
        if len(img) != n or len(spot) != n:
            raise ValueError(f"fold {f}: {len(img)} image / {len(spot)} spot embedding arrays for {n} slides")
        rest = [i for i in range(n) if i != f]
        preds.append(predict_device(_cat_rows([spot[i] for i in rest]), _cat_rows([expressions[i] for i in rest]), img[f],
                                    method, top_k))
    res = score_folds(preds, list(expressions), markers)
    if return_preds:
        res["preds"] = [p.cpu().numpy() for p in preds]
    return res


# ------------------------------------------------------------------------------------------- gene-gene correlation (cell 7)
def gene_gene_correlation(x: ArrayLike, genes: Sequence[int]) -> np.ndarray:
    """``np.corrcoef(x[:, genes].T)`` of a (spots, genes) matrix, (m, m) float64: the centred Gram matrix of the m gathered
    columns by ``mcl_pca_gram`` (its primal form, hence spots >= m) normalised by ``mcl_corr_from_gram``; a constant column
    gives a NaN row and column."""
    g = np.asarray(genes)
    if g.ndim != 1 or g.size < 1 or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"genes must be a non-empty 1-D list of integer gene indices, got {genes!r}")
    if not isinstance(x, Tensor):
        x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"x: expected a (spots, genes) array, got shape {tuple(x.shape)}")
    n, G = int(x.shape[0]), int(x.shape[1])
    m = int(g.size)
    if int(g.min()) < 0 or int(g.max()) >= G:
        raise IndexError(f"gene index out of range for {G} genes")
    if m > n:
        raise ValueError(f"the correlation of {m} genes needs at least {m} spots, got {n}")
    off = validate_offsets([0, n], n, min_rows=2)
    dev = device("bleep")
    e = empty(dev)
    if isinstance(x, Tensor):
        src = matrix(x, "x", dev, FLOAT_CODE, torch.float64)
        xs = e((n, m), src.dtype)
        for j, c in enumerate(g.tolist()):                    # plain strided copies, one per gathered column
            xs[:, j].copy_(src[:, c])
    else:
        xs = matrix(x[:, g], "x", dev, FLOAT_CODE, torch.float64)
    off_d, goff_d = upload(off, dev), upload(np.array([0, m * m], dtype=np.int64), dev)
    mean, gram, corr = e((1, m), torch.float64), e((m * m,), torch.float64), e((m, m), torch.float64)
    call("mcl_pca_gram", xs, xs.stride(0), FLOAT_CODE[xs.dtype], off_d, 1, m, n, goff_d, mean, gram)
    call("mcl_corr_from_gram", gram, m, corr)
    return corr.cpu().numpy()


def ward_leaves(corr: np.ndarray) -> np.ndarray:
    """The heat map's row order: ``hierarchy.dendrogram(hierarchy.linkage(corr, method='ward'), no_plot=True)['leaves']``.
    scipy is needed for this one function only."""
    try:
        from scipy.cluster import hierarchy
    except ImportError as e:
        raise RuntimeError("order='ward' needs scipy (scipy.cluster.hierarchy); pass order=None to skip the "
                           "reordering") from e
    return np.asarray(hierarchy.dendrogram(hierarchy.linkage(corr, method="ward"), no_plot=True)["leaves"], dtype=np.int64)


def ggc_matrices(true: ArrayLike, pred: ArrayLike, top_k: int = N_TOP, order: Optional[str] = "ward") -> Dict[str, np.ndarray]:
    """Cell 7's heat-map matrices of (spots, genes) ``true`` and ``pred``: ``genes`` the ``top_k`` genes of largest
    ground-truth mean (best first, equal means by gene index; the notebook's ``argpartition`` leaves their order open),
    ``corr_true`` and ``corr_pred`` their gene-gene correlation in ground truth and prediction.  ``order="ward"`` reorders
    both by ``leaves`` = ``ward_leaves(corr_true)``; ``order=None`` keeps the order of ``genes``."""
    if order not in ("ward", None):
        raise ValueError(f"order must be 'ward' or None, got {order!r}")
    if tuple(true.shape) != tuple(pred.shape) or len(true.shape) != 2:
        raise ValueError(f"true {tuple(true.shape)} and pred {tuple(pred.shape)} must be (spots, genes) of one shape")
    n, G = int(true.shape[0]), int(true.shape[1])
    dev = device("bleep")
    t = matrix(true, "true", dev, FLOAT_CODE, torch.float64)
    genes = evaluate.metrics_device(t, t, [0, n], min(int(top_k), G))["heg"][0].cpu().numpy()
    out = {"genes": genes, "corr_true": gene_gene_correlation(t, genes), "corr_pred": gene_gene_correlation(pred, genes)}
    if order == "ward":
        leaves = ward_leaves(out["corr_true"])
        out["leaves"] = leaves
        for k in ("corr_true", "corr_pred"):
            out[k] = out[k][leaves][:, leaves]
    return out


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.bleep",
                                description="Leave-one-slide-out scoring of saved embeddings by BLEEP's protocol "
                                            "(BLEEP_inference.ipynb, cells 5 and 7)")
    p.add_argument("--embedding_dir", required=True,
                   help="holds embeddings_{fold}/ with spot_embeddings_{i+1}.npy and img_embeddings_{i+1}.npy, (P, N)")
    p.add_argument("--expressions", required=True, nargs="+",
                   help="one expression matrix .npy per slide, (G, N), in slide order")
    p.add_argument("--method", default="average", choices=sorted(METHOD_TOP_K))
    p.add_argument("--top_k", type=int, default=None, help="matches per query (default: 1 for simple, 50 otherwise)")
    p.add_argument("--markers", default=None, nargs="+", help="marker gene names (needs --genes)")
    p.add_argument("--genes", default=None, help=".npy of G gene names")
    p.add_argument("--json", default=None, help="also write per-fold and average scores to this file")
    p.add_argument("--save_pred", default=None, metavar="DIR",
                   help=f"also write every slide's prediction to DIR/<slide index>/{evaluate.PRED_FILE}, (G, N)")
    p.add_argument("--ggc", default=None, metavar="OUT.npz",
                   help="also write every slide's gene-gene-correlation matrices (genes_i, corr_true_i, corr_pred_i, leaves_i)")
    a = p.parse_args(argv)
    if a.markers is not None and a.genes is None:
        p.error("--markers names genes: pass --genes names.npy")
    if a.top_k is not None and a.top_k < 1:
        p.error("--top_k must be >= 1")
    return a


def marker_indices(names: Sequence[str], gene_names: Sequence[str]) -> List[int]:
    """The index of every marker in ``gene_names`` (the notebook's ``np.where(gene_names == name)[0]``)."""
    where = {str(g): i for i, g in reversed(list(enumerate(gene_names)))}
    missing = [m for m in names if m not in where]
    if missing:
        raise ValueError(f"marker genes not among the gene names: {missing}")
    return [where[m] for m in names]


def format_report(res: Dict[str, object]) -> str:
    """The lines the notebook prints (cell 5), for one fold's dict or the averages."""
    lines = [f"Mean correlation across cells:  {res['cell_mean']}"]
    if "n_genes_valid" in res:
        lines.append(f"number of non-zero genes:  {res['n_genes_valid']}")
    lines += [f"max correlation:  {res['max_r']}",
              f"mean correlation highly expressed genes:  {res['heg_mean']}",
              f"mean correlation highly variable genes:  {res['hvg_mean']}",
              f"mean correlation marker genes:  {res['marker_mean']}"]
    return "\n".join(lines)


def _json_value(v):
    if isinstance(v, float) and math.isnan(v):
        return None
    if isinstance(v, np.ndarray):
        return [_json_value(float(x)) if v.dtype.kind == "f" else int(x) for x in v]
    return v


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    expressions = evaluate.load_expressions(args.expressions)
    n = len(expressions)
    markers = None
    if args.markers is not None:
        names = [str(x) for x in np.load(args.genes, allow_pickle=True).reshape(-1)]
        if len(names) != expressions[0].shape[1]:
            raise ValueError(f"{args.genes}: {len(names)} gene names for {expressions[0].shape[1]} genes")
        markers = marker_indices(args.markers, names)

    def per_fold(f):
        images, spots = evaluate.load_fold_embeddings(args.embedding_dir, f, n)
        evaluate.check_layout(images, spots, expressions, f)
        return images, spots

    res = leave_one_slide_out(None, None, expressions, args.method, args.top_k, per_fold=per_fold, markers=markers,
                              return_preds=args.save_pred is not None or args.ggc is not None)
    for f, fold in enumerate(res["folds"]):
        print(f"fold {f}:")
        print(format_report(fold))
    print("average over folds:")
    print(format_report(res))
    if args.save_pred:
        evaluate.save_predictions(args.save_pred, res["preds"])
    if args.ggc:
        doc = {}
        for i, (t, p) in enumerate(zip(expressions, res["preds"])):
            doc.update({f"{k}_{i}": v for k, v in ggc_matrices(t, p).items()})
        np.savez_compressed(args.ggc, **doc)
    if args.json:
        doc = {k: _json_value(res[k]) for k in SUMMARY_KEYS}
        doc.update(method=args.method, top_k=METHOD_TOP_K[args.method] if args.top_k is None else args.top_k,
                   markers=markers, folds=[{k: _json_value(v) for k, v in f.items()} for f in res["folds"]])
        write_json(args.json, doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
