"""Scoring of expression predictions on the MI355X: the closing block of the reference's evaluation scripts
(per-gene Pearson r, HEG / HVG mean r, MSE, MAE) and its leave-one-slide-out protocol, on the device.

Reference (paths relative to /root/reference/):
  get_R              utils.py:52-65 (scipy.stats.pearsonr per gene, dim=1)
  scoring block      evel_her2st.py:196-226, evel_cscc.py:226-261, evel_visium.py:212-244
  leave one out      evel_her2st.py:140-154 (queries: slide f's image embeddings; keys: every other slide)
  presets            top 200 / L1 evel_her2st.py:174,176; top 600 / L2 evel_cscc.py:197,209; top 200 / L2
                     evel_visium.py:193,197

All folds are scored by ONE ``mcl_expr_metrics`` call (csrc/eval_metrics.hip, fp64, deterministic: a fold scored inside a
batch is bit-identical to the same fold scored alone).  Arrays move to the device once; no CPU fallback: without a GPU /
the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.evaluate --dataset her2st --embedding_dir DIR --expressions F1.npy F2.npy ... [--json OUT]
                                    [--save_pred DIR]
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _arrays
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, device, empty, load_gene_major, paired_offsets, stack_rows, upload,
                      write_json)
from ._lib import call

# dataset -> (top_k, ord of the distance norm in the weighting)
PRESETS = {"her2st": (200, 1), "cscc": (600, 2), "10x": (200, 2)}
N_HEG = 50
SUMMARY_KEYS = ("heg_pcc", "hvg_pcc", "mse", "mae")
PRED_FILE = "matched_spot_expression_pred_mclSTExp.npy"


def validate_offsets(offsets: Sequence[int], rows: int) -> np.ndarray:
    """The preconditions of mcl_expr_metrics' device-resident offsets, checked on the host: offsets[0] = 0, every fold
    >= 2 spots (scipy.stats.pearsonr raises below 2), offsets[-1] = rows.  Returns them as int64."""
    return _arrays.validate_offsets(offsets, rows, min_rows=2, noun="fold")


def metrics_device(pred: Tensor, true: Tensor, offsets: Sequence[int], n_heg: int = N_HEG) -> Dict[str, Tensor]:
    """One mcl_expr_metrics call on row-stacked device matrices.  Device tensors: ``r`` (S, G), ``true_mean`` (S, G),
    ``heg`` (S, min(n_heg, G)) int64, ``summary`` (S, 5) = heg_pcc, hvg_pcc, mse, mae, n_valid."""
    if pred.shape != true.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and true {tuple(true.shape)} differ in shape")
    rows, G = pred.shape
    off = validate_offsets(offsets, rows)
    S = off.size - 1
    n_heg = min(int(n_heg), G)
    if n_heg < 1:
        raise ValueError("n_heg must be >= 1")
    for t, name in ((pred, "pred"), (true, "true")):
        if not t.is_cuda or t.dtype not in FLOAT_CODE or (t.stride(1) != 1 and G != 1):
            raise RuntimeError(f"{name}: expected a row-major float32 / float64 device matrix")
    off_d = upload(off, pred.device)
    e = empty(pred.device)
    r, true_mean, summary = e((S, G), torch.float64), e((S, G), torch.float64), e((S, 5), torch.float64)
    heg = e((S, n_heg), torch.int64)
    work = e((2 * S * G,), torch.float64)
    call("mcl_expr_metrics", pred, pred.stride(0), FLOAT_CODE[pred.dtype], true, true.stride(0),
         FLOAT_CODE[true.dtype], off_d, S, G, n_heg, r, true_mean, heg, summary, work)
    return {"r": r, "true_mean": true_mean, "heg": heg, "summary": summary}


def stacked_metrics(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], offsets: np.ndarray,
                    n_heg: int = N_HEG) -> Dict[str, Tensor]:
    """``metrics_device`` of the per-fold arrays row-stacked on the device (``offsets``: their ``paired_offsets``).  Device
    folds of differing dtype are converted by the stacking copy."""
    dev = device("evaluate")
    return metrics_device(stack_rows(preds, "preds", dev, convert_on_device=True)[0],
                          stack_rows(trues, "trues", dev, convert_on_device=True)[0], offsets, n_heg)


def score_folds(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], n_heg: int = N_HEG) -> Dict[str, object]:
    """Scores every fold's (spots, genes) prediction against its ground truth in ONE metrics call.  Returns
    ``folds``: per-fold dicts as ``score`` returns them, and ``heg_pcc``, ``hvg_pcc``, ``mse``, ``mae``: ``np.mean`` over
    the folds, as the reference's scripts print them (a NaN fold heg_pcc makes the average NaN)."""
    offsets = paired_offsets(preds, trues, "fold")
    m = stacked_metrics(preds, trues, offsets, n_heg)
    r, heg, summ = m["r"].cpu().numpy(), m["heg"].cpu().numpy(), m["summary"].cpu().numpy()
    folds = [{"heg_pcc": float(summ[s, 0]), "hvg_pcc": float(summ[s, 1]), "mse": float(summ[s, 2]),
              "mae": float(summ[s, 3]), "n_valid": int(summ[s, 4]), "pcc": r[s], "heg_genes": heg[s]}
             for s in range(len(preds))]
    out: Dict[str, object] = {"folds": folds}
    for k in SUMMARY_KEYS:
        out[k] = float(np.mean([f[k] for f in folds]))
    return out


def score(pred: ArrayLike, true: ArrayLike, n_heg: int = N_HEG) -> Dict[str, object]:
    """One fold: ``heg_pcc``, ``hvg_pcc``, ``mse``, ``mae``, ``pcc`` (G,), ``heg_genes`` (min(n_heg, G),), ``n_valid``."""
    return score_folds([pred], [true], n_heg)["folds"][0]


def gene_pcc(pred: ArrayLike, true: ArrayLike) -> np.ndarray:
    """Per-gene Pearson r (G,): the first output of the reference's ``get_R(adata_pred, adata_true)`` (NaN for a
    constant column)."""
    return score(pred, true)["pcc"]


def _predict_device(spot_key: ArrayLike, expression_key: ArrayLike, image_query: ArrayLike, top_k: int,
                    ord: int) -> Tensor:
    from . import retrieval
    key = retrieval.to_device(spot_key, "spot_key")
    qry = retrieval.to_device(image_query, "image_query")
    _, idx = retrieval.find_matches_device(key, qry, top_k)
    _, expr = retrieval.weighted_average_device(key, expression_key, qry, idx, ord)
    return expr


def evaluate_fold(spot_key: ArrayLike, expression_key: ArrayLike, image_query: ArrayLike, expression_gt: ArrayLike,
                  top_k: int, ord: int, n_heg: int = N_HEG) -> Dict[str, object]:
    """Retrieval -> weighted average -> score for one fold (evel_her2st.py:174-226); the prediction never leaves the
    device."""
    return score(_predict_device(spot_key, expression_key, image_query, top_k, ord), expression_gt, n_heg)


def _cat_rows(parts: Sequence[ArrayLike]) -> ArrayLike:
    if any(isinstance(p, Tensor) for p in parts):
        dev = device("evaluate")
        return torch.cat([torch.as_tensor(p).to(device=dev, dtype=torch.float32) for p in parts])
    return np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])


def leave_one_slide_out(image_embeddings: Optional[Sequence[ArrayLike]], spot_embeddings: Optional[Sequence[ArrayLike]],
                        expressions: Sequence[ArrayLike], top_k: int, ord: int,
                        per_fold: Optional[Callable[[int], Tuple[Sequence[ArrayLike], Sequence[ArrayLike]]]] = None,
                        n_heg: int = N_HEG, return_preds: bool = False) -> Dict[str, object]:
    """The reference's protocol (evel_her2st.py:140-226): fold f queries slide f's image embeddings against the spot
    embeddings and expressions of all OTHER slides; every list holds one (spots, ·) array per slide.  ``per_fold(f)``
    -> (image_embeddings, spot_embeddings) supplies fold-specific embeddings (the reference loads ``embeddings_{f}/``
    from fold f's own checkpoint); without it one model's embeddings serve all folds.  Retrieval runs per fold, the
    scoring of all folds is one call.  Returns what ``score_folds`` returns; with ``return_preds`` also ``preds``: every
    slide's (spots, genes) prediction as a numpy array (what ``mclstexp_amd.genes`` ranks genes from)."""
    n = len(expressions)
    if n < 2:
        raise ValueError("leave-one-slide-out needs >= 2 slides")
    preds = []
    for f in range(n):
        img, spot = per_fold(f) if per_fold is not None else (image_embeddings, spot_embeddings)
        if len(img) != n or len(spot) != n:
            raise ValueError(f"fold {f}: {len(img)} image / {len(spot)} spot embedding arrays for {n} slides")
        rest = [i for i in range(n) if i != f]
        key = _cat_rows([spot[i] for i in rest])
        expr = _cat_rows([expressions[i] for i in rest])
        preds.append(_predict_device(key, expr, img[f], top_k, ord))
    res = score_folds(preds, list(expressions), n_heg)
    if return_preds:
        res["preds"] = [p.cpu().numpy() for p in preds]
    return res


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.evaluate",
                                description="Leave-one-slide-out scoring of saved embeddings (the reference's evel_*.py)")
    p.add_argument("--dataset", required=True, choices=sorted(PRESETS))
    p.add_argument("--embedding_dir", required=True,
                   help="holds embeddings_{fold}/ with spot_embeddings_{i+1}.npy and img_embeddings_{i+1}.npy, (P, N)")
    p.add_argument("--expressions", required=True, nargs="+",
                   help="one preprocessed_matrix.npy per slide, (G, N), in slide order")
    p.add_argument("--json", default=None, help="also write per-fold and average scores to this file")
    p.add_argument("--save_pred", default=None, metavar="DIR",
                   help=f"also write every slide's prediction to DIR/<slide index>/{PRED_FILE}, (G, N)")
    return p.parse_args(argv)


def load_fold_embeddings(embedding_dir: str, fold: int, n_slides: int) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(image_embeddings, spot_embeddings) of ``embeddings_{fold}/`` as (N_i, P) arrays, from the layout the reference's
    save_embeddings writes (evel_her2st.py:87-119: ``.T`` of (N_i, P), files numbered from 1).  Only slide ``fold``'s
    image embeddings are read (the fold's queries); the other image entries are None."""
    d = os.path.join(embedding_dir, f"embeddings_{fold}")
    spot = [np.load(os.path.join(d, f"spot_embeddings_{i + 1}.npy")) for i in range(n_slides)]
    img = np.load(os.path.join(d, f"img_embeddings_{fold + 1}.npy"))
    for a, what in [(x, f"spot_embeddings_{i + 1}") for i, x in enumerate(spot)] + [(img, f"img_embeddings_{fold + 1}")]:
        if a.ndim != 2 or a.shape[0] != spot[0].shape[0]:
            raise ValueError(f"{d}/{what}.npy: expected (P, N) with P = {spot[0].shape[0]}, got {a.shape}")
    images: List[Optional[np.ndarray]] = [None] * n_slides
    images[fold] = img.T
    return images, [s.T for s in spot]


def load_expressions(paths: Sequence[str]) -> List[np.ndarray]:
    """(N_i, G) arrays from preprocessed_matrix.npy files stored (G, N_i)."""
    return load_gene_major(paths)


def check_layout(images: Sequence[Optional[np.ndarray]], spots: Sequence[np.ndarray], expressions: Sequence[np.ndarray],
                 fold: int) -> None:
    """Spot counts of the embeddings agree with the expression matrices (no guessing by shape)."""
    for i, (s, e) in enumerate(zip(spots, expressions)):
        if s.shape[0] != e.shape[0]:
            raise ValueError(f"embeddings_{fold}: slide {i + 1} has {s.shape[0]} spot embeddings, {e.shape[0]} expression rows")
    if images[fold].shape[0] != expressions[fold].shape[0]:
        raise ValueError(f"embeddings_{fold}: {images[fold].shape[0]} image embeddings for slide {fold + 1}, "
                         f"{expressions[fold].shape[0]} expression rows")


def save_predictions(root: str, preds: Sequence[np.ndarray]) -> List[str]:
    """Writes slide i's (spots, genes) prediction to ``root/<i>/matched_spot_expression_pred_mclSTExp.npy`` stored (G, N)
    -- the file the reference's tutorial.ipynb reads per slide (``python -m mclstexp_amd.genes --pred``).  Returns the
    paths in slide order."""
    paths = []
    for i, p in enumerate(preds):
        a = np.asarray(p)
        if a.ndim != 2:
            raise ValueError(f"prediction of slide {i}: expected a (spots, genes) array, got {a.shape}")
        d = os.path.join(root, str(i))
        os.makedirs(d, exist_ok=True)
        paths.append(os.path.join(d, PRED_FILE))
        np.save(paths[-1], np.ascontiguousarray(a.T))
    return paths


def format_report(res: Dict[str, object]) -> str:
    """The four lines the reference's scripts print last (evel_her2st.py:223-226)."""
    return "\n".join([f"avg heg pcc: {res['heg_pcc']:.4f}", f"avg hvg pcc: {res['hvg_pcc']:.4f}",
                      f"Mean Squared Error (MSE): {res['mse']:.4f}", f"Mean Absolute Error (MAE): {res['mae']:.4f}"])


def _json_value(v):
    if isinstance(v, float) and math.isnan(v):
        return None
    if isinstance(v, np.ndarray):
        return [_json_value(float(x)) if v.dtype.kind == "f" else int(x) for x in v]
    return v


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    top_k, ord_ = PRESETS[args.dataset]
    expressions = load_expressions(args.expressions)
    n = len(expressions)

    def per_fold(f):
        images, spots = load_fold_embeddings(args.embedding_dir, f, n)
        check_layout(images, spots, expressions, f)
        return images, spots

    res = leave_one_slide_out(None, None, expressions, top_k, ord_, per_fold=per_fold,
                              return_preds=args.save_pred is not None)
    print(format_report(res))
    if args.save_pred:
        save_predictions(args.save_pred, res["preds"])
    if args.json:
        doc = {k: _json_value(res[k]) for k in SUMMARY_KEYS}
        doc.update(dataset=args.dataset, top_k=top_k, ord=ord_,
                   folds=[{k: _json_value(v) for k, v in f.items()} for f in res["folds"]])
        write_json(args.json, doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
