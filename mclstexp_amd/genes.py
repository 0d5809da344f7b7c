"""Gene-level significance of expression predictions on the MI355X: the per-gene Pearson p-value the reference's
``get_R`` returns next to r, and the gene table its tutorial ranks genes by.

Reference (paths relative to /root/reference/):
  get_R              utils.py:52-65 -> (r, p), p = scipy.stats.pearsonr's two-sided p-value
  gene table         tutorial.ipynb, third cell: a genes x slides frame of ``-np.log10(p)``, ``mean(axis=1)`` (skipna),
                     ``sort_values(ascending=False)``, ``head(7)``, per gene ``idxmax`` (the slide with the largest
                     -log10 p) and the PCC there

Two entry points of csrc/gene_significance.hip (fp64, deterministic): ``mcl_pearson_pvalue`` turns the (S, G) r matrix of
``mcl_expr_metrics`` into p and -log10 p, ``mcl_gene_rank`` reduces the table.  -log10 p is evaluated in log space and
stays finite where p underflows fp64 (n = 4784, r = 0.6: scipy gives p = 0 and -log10 p = inf, the value is 465.14).
No CPU fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.genes --pred P1.npy ... --true T1.npy ... [--genes names.npy] [--slides A2 A3 ...]
                                 [--top 7] [--reference_inf] [--csv OUT]
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import evaluate
from ._arrays import ArrayLike, Tensor, device, empty, load_gene_major, matrix, paired_offsets, upload
from ._lib import call

TOP_N = 7
PRED_FILE = evaluate.PRED_FILE     # what the tutorial reads per slide; ``evaluate --save_pred`` writes it


def _f64_matrix(a: ArrayLike, name: str, dev: torch.device) -> Tensor:
    """A dense (slides, genes) float64 device matrix: arrays are converted on the host, tensors must be float64."""
    if isinstance(a, Tensor) and a.dtype != torch.float64:
        raise ValueError(f"{name}: expected a float64 tensor, got {a.dtype}")
    return matrix(a, name, dev, (torch.float64,), torch.float64, dense=True)


def pvalues_device(r: Tensor, offsets: Sequence[int]) -> Tuple[Tensor, Tensor]:
    """One ``mcl_pearson_pvalue`` call: ``r`` (S, G) float64 on the device (``evaluate.metrics_device(...)["r"]``),
    ``offsets`` the S + 1 fold boundaries that produced it (host integers, or a device int64 tensor).  Returns the
    device tensors ``p`` and ``neglog10p``, both (S, G) float64."""
    device("genes")
    if not isinstance(r, Tensor) or not r.is_cuda or r.dtype != torch.float64 or r.dim() != 2 or not r.is_contiguous():
        raise RuntimeError("r: expected a contiguous (slides, genes) float64 device matrix")
    S, G = r.shape
    if isinstance(offsets, Tensor):
        if offsets.dtype != torch.int64 or offsets.numel() != S + 1:
            raise ValueError(f"offsets: expected {S + 1} int64 entries")
        off_d = offsets.to(r.device).contiguous()
    else:
        off = np.asarray(offsets)
        if off.ndim != 1 or off.size != S + 1:
            raise ValueError(f"offsets must be a 1-D integer array of S + 1 = {S + 1} entries, got {off!r}")
        off_d = upload(evaluate.validate_offsets(off, off[-1]), r.device)
    e = empty(r.device)
    p, nl = e((S, G), torch.float64), e((S, G), torch.float64)
    call("mcl_pearson_pvalue", r, off_d, S, G, p, nl)
    return p, nl


def significance_device(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike]) -> Dict[str, Tensor]:
    """``pcc``, ``p``, ``neglog10p`` as (S, G) float64 device tensors: one ``evaluate.metrics_device`` call for r, one
    ``mcl_pearson_pvalue`` call on it; nothing leaves the device in between."""
    offsets = paired_offsets(preds, trues, "slide")
    device("genes")                                   # without a GPU this module is the one that says so
    m = evaluate.stacked_metrics(preds, trues, offsets)
    p, nl = pvalues_device(m["r"], offsets)
    return {"pcc": m["r"], "p": p, "neglog10p": nl}


def gene_significance(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike]) -> Dict[str, np.ndarray]:
    """Both outputs of the reference's ``get_R(adata_pred, adata_true)`` for every slide at once, and -log10 p.  ``preds``
    / ``trues``: one (spots, genes) array or device tensor per slide, float32 or float64.  Returns (S, G) float64 numpy
    arrays: ``pcc`` (NaN for a constant column), ``p`` (NaN where pcc is; 1 on a two-spot slide; underflows to 0 as
    scipy's does) and ``neglog10p`` (evaluated in log space: finite where ``p`` is 0, +inf only where |pcc| = 1)."""
    return {k: v.cpu().numpy() for k, v in significance_device(preds, trues).items()}


def rank_genes(neglog10p: ArrayLike, r: ArrayLike, top_n: int = TOP_N, log_space: bool = True,
               p: Optional[ArrayLike] = None) -> Dict[str, object]:
    """The tutorial's gene table, reduced by one ``mcl_gene_rank`` call.  ``neglog10p`` and ``r``: (S, G) float64, arrays
    or device tensors.  Returns ``mean`` (G,): the skipna mean of every gene's -log10 p over the slides (NaN if no slide
    defines it); ``n_defined`` (G,); ``order`` (G,) int64: the genes by descending mean, equal means by gene index, NaN
    last; ``top``: for the first ``top_n`` of them ``{gene, mean, best_slide, best_value, pcc}`` -- the first slide with
    the gene's largest -log10 p (pandas ``idxmax``), that value, and the PCC there.

    ``log_space=True`` (default) ranks by the log-space -log10 p.  ``log_space=False`` is the tutorial's own arithmetic,
    quirk for quirk: the table is ``-np.log10(p)`` of the fp64 ``p`` (pass it as ``p``), which is ``inf`` wherever ``p``
    underflowed.  On slides of a few thousand spots that happens to every well-predicted gene (n = 4784: from r ~ 0.5
    on), all of them then share the mean ``inf`` and the ranking among them is arbitrary -- which is why it is not the
    default.  Where no ``p`` underflows (the HER2ST slides) the two modes agree to rounding."""
    dev = device("genes")
    if not log_space:
        if p is None:
            raise ValueError("log_space=False ranks by -log10 of the fp64 p: pass p")
        ph = p.cpu().numpy() if isinstance(p, Tensor) else np.asarray(p, dtype=np.float64)
        with np.errstate(divide="ignore"):
            neglog10p = -np.log10(ph)            # the tutorial's line, in numpy as there: bit for bit its table
    nl = _f64_matrix(neglog10p, "neglog10p", dev)
    rr = _f64_matrix(r, "r", dev)
    if nl.shape != rr.shape:
        raise ValueError(f"neglog10p {tuple(nl.shape)} and r {tuple(rr.shape)} differ in shape")
    S, G = nl.shape
    top_n = max(1, min(int(top_n), G))
    e = empty(dev)
    mean, best_value, best_r = e((G,), torch.float64), e((G,), torch.float64), e((G,), torch.float64)
    n_defined, best_slide, order = e((G,), torch.int32), e((G,), torch.int32), e((G,), torch.int64)
    call("mcl_gene_rank", nl, rr, S, G, top_n, mean, n_defined, order, best_slide, best_value, best_r)
    mean_h, order_h = mean.cpu().numpy(), order.cpu().numpy()
    slide_h, value_h, r_h = best_slide.cpu().numpy(), best_value.cpu().numpy(), best_r.cpu().numpy()
    top = [{"gene": int(g), "mean": float(mean_h[g]), "best_slide": int(slide_h[g]), "best_value": float(value_h[g]),
            "pcc": float(r_h[g])} for g in order_h[:top_n]]
    return {"mean": mean_h, "n_defined": n_defined.cpu().numpy(), "order": order_h, "top": top}


def significance_table(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike],
                       gene_names: Optional[Sequence[str]] = None, slide_names: Optional[Sequence[str]] = None,
                       top_n: int = TOP_N, log_space: bool = True) -> Dict[str, object]:
    """``gene_significance`` then ``rank_genes``.  Returns ``pcc``, ``p``, ``neglog10p`` (S, G) -- ``neglog10p`` is the
    table that was ranked, i.e. ``-np.log10(p)`` when ``log_space=False`` --, ``mean``, ``n_defined``, ``order``, ``top``
    (each entry also carries ``gene_name`` and ``slide_name``), ``gene_names`` and ``slide_names`` (default: the indices
    as strings)."""
    S, G = len(preds), int(preds[0].shape[1]) if len(preds) else 0
    genes = [str(g) for g in (gene_names if gene_names is not None else range(G))]
    slides = [str(s) for s in (slide_names if slide_names is not None else range(S))]
    if len(genes) != G or len(slides) != S:
        raise ValueError(f"{len(genes)} gene names / {len(slides)} slide names for {G} genes / {S} slides")
    d = significance_device(preds, trues)
    res = rank_genes(d["neglog10p"], d["pcc"], top_n, log_space, p=d["p"])
    out: Dict[str, object] = {k: v.cpu().numpy() for k, v in d.items()}
    if not log_space:
        with np.errstate(divide="ignore"):
            out["neglog10p"] = -np.log10(out["p"])
    for t in res["top"]:
        t["gene_name"] = genes[t["gene"]]
        t["slide_name"] = slides[t["best_slide"]] if t["best_slide"] >= 0 else None
    out.update(res, gene_names=genes, slide_names=slides)
    return out


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.genes",
                                description="Rank genes by the Pearson p-value of their prediction (the reference's "
                                            "tutorial.ipynb, third cell)")
    p.add_argument("--pred", required=True, nargs="+", help=f"one {PRED_FILE} per slide, (G, N), in slide order")
    p.add_argument("--true", required=True, nargs="+", help="one preprocessed_matrix.npy per slide, (G, N), same order")
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the gene index)")
    p.add_argument("--slides", default=None, nargs="+", help="slide names (default: the slide index)")
    p.add_argument("--top", type=int, default=TOP_N, help="how many genes to report")
    p.add_argument("--reference_inf", action="store_true",
                   help="rank by -log10 of the fp64 p as the tutorial does: inf where p underflows")
    p.add_argument("--csv", default=None, help="write the sorted genes x slides table plus avg_p_value to this file")
    a = p.parse_args(argv)
    if len(a.pred) != len(a.true):
        p.error(f"{len(a.pred)} --pred files for {len(a.true)} --true files")
    if a.slides is not None and len(a.slides) != len(a.pred):
        p.error(f"{len(a.slides)} --slides names for {len(a.pred)} slides")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def load_slides(pred_paths: Sequence[str], true_paths: Sequence[str]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(spots, genes) arrays from files stored (G, N_i), the layout the reference stores; shapes checked pairwise."""
    preds, trues = load_gene_major(pred_paths), load_gene_major(true_paths)
    for fp, ft, a, b in zip(pred_paths, true_paths, preds, trues):
        if b.shape != a.shape:
            raise ValueError(f"{ft}: expected {a.T.shape} as {fp}, got {b.T.shape}")
    return preds, trues


def load_gene_names(path: Optional[str], G: int) -> Optional[List[str]]:
    if path is None:
        return None
    names = [str(x) for x in np.load(path, allow_pickle=True).reshape(-1)]
    if len(names) != G:
        raise ValueError(f"{path}: {len(names)} gene names for {G} genes")
    return names


def format_top(res: Dict[str, object]) -> List[str]:
    """The line the tutorial prints per top gene."""
    return [f"Gene: {t['gene_name']}, Max -log(p-value) in {t['slide_name']}: {t['best_value']}, "
            f"PCC in {t['slide_name']}: {t['pcc']}" for t in res["top"]]


def write_csv(path: str, res: Dict[str, object]) -> None:
    """The tutorial's ``sorted_result_df.to_csv``: genes (sorted) x slides plus ``avg_p_value``; NaN as an empty field."""
    def cell(v: float) -> str:
        return "" if np.isnan(v) else repr(float(v))
    nl, mean = res["neglog10p"], res["mean"]
    with open(path, "w") as fh:
        fh.write(",".join([""] + list(res["slide_names"]) + ["avg_p_value"]) + "\n")
        for g in res["order"]:
            fh.write(",".join([res["gene_names"][g]] + [cell(v) for v in nl[:, g]] + [cell(mean[g])]) + "\n")


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds, trues = load_slides(args.pred, args.true)
    genes = load_gene_names(args.genes, preds[0].shape[1])
    res = significance_table(preds, trues, genes, args.slides, args.top, log_space=not args.reference_inf)
    print("\n".join(format_top(res)))
    if args.csv:
        write_csv(args.csv, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
