"""numpy restatement of BLEEP's prediction methods and scoring block (tests only), for the tests of mclstexp_amd.bleep and
retrieval.combine_device.

Line by line baselines/Bleep/BLEEP_inference.ipynb, cell 5 (the three ``if method == ...`` blocks, the correlation
statements) and cell 7 (``np.corrcoef`` of the chosen genes), in the notebook's own dtypes (fp32 inputs stay fp32).  Pinned
against the notebook's own outputs by tests/test_bleep_host.py (tests/golden/bleep_protocol.npz, written by
tests/golden/gen_bleep_protocol_goldens.py)."""
import os
import warnings

import numpy as np

from mclstexp_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleep_protocol.npz")

# name -> (N keys, Q queries, G genes, k, seed): inputs are synth.make_retrieval_case(N, Q, 256, G, seed=seed)
RETRIEVAL_CASES = {
    "tiny": (257, 5, 19, 7, 11),       # k not a multiple of 4, G < 50, G not a multiple of 4
    "mid": (600, 33, 97, 50, 12),
    "her2st": (3000, 48, 171, 50, 13),
}
# name -> does one true column stay constant; segments (37, 2, 64), G = 97, one constant pred row, markers (3, 50, 96)
SCORING_CASES = {"nan_gene": True, "plain": False}
SEGMENTS = (37, 2, 64)
SCORING_GENES = 97
MARKERS = (3, 50, 96)
CONST_COLUMN = 5
CONST_PRED_ROW = 11


def retrieval_case(name):
    n, q, g, k, seed = RETRIEVAL_CASES[name]
    d = synth.make_retrieval_case(n, q, 256, g, seed=seed)
    d["k"] = k
    return d


def scoring_case(name):
    """``pred``, ``true`` (rows, 97) float64 and ``offsets``: synth.make_eval_case plus one constant prediction ROW."""
    d = synth.make_eval_case(list(SEGMENTS), SCORING_GENES, seed=22, const_true=[CONST_COLUMN] if SCORING_CASES[name] else [])
    d["pred"][CONST_PRED_ROW, :] = 0.75
    return d


# ------------------------------------------------------------------------------------------------- prediction methods
def simple(spot_key, expression_key, indices):
    return spot_key[indices[:, 0], :], expression_key[indices[:, 0], :]


def average(spot_key, expression_key, indices):
    emb = np.zeros((indices.shape[0], spot_key.shape[1]))
    expr = np.zeros((indices.shape[0], expression_key.shape[1]))
    for i in range(indices.shape[0]):
        emb[i, :] = np.average(spot_key[indices[i, :], :], axis=0)
        expr[i, :] = np.average(expression_key[indices[i, :], :], axis=0)
    return emb, expr


def weighted_average(spot_key, expression_key, image_query, indices, dtype=None):
    """``dtype=None``: the notebook's arithmetic (fp32 arrays -> fp32 distances and weights); ``np.float64``: the same
    formula on the inputs widened first."""
    if dtype is not None:
        spot_key, expression_key, image_query = (a.astype(dtype) for a in (spot_key, expression_key, image_query))
    emb = np.zeros((indices.shape[0], spot_key.shape[1]))
    expr = np.zeros((indices.shape[0], expression_key.shape[1]))
    for i in range(indices.shape[0]):
        a = np.sum((spot_key[indices[i, 0], :] - image_query[i, :]) ** 2)
        weights = np.exp(-(np.sum((spot_key[indices[i, :], :] - image_query[i, :]) ** 2, axis=1) - a + 1))
        emb[i, :] = np.average(spot_key[indices[i, :], :], axis=0, weights=weights)
        expr[i, :] = np.average(expression_key[indices[i, :], :], axis=0, weights=weights)
    return emb, expr


def row_scaled_gap(a, b):
    """max over rows of max|a - b| / max|b| of the row."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)))


# --------------------------------------------------------------------------------------------------------- scoring block
def correlations(pred, true):
    """(per-cell r, per-gene r), both with their NaN entries kept."""
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        cell = np.zeros(pred.shape[0])
        for i in range(pred.shape[0]):
            cell[i] = np.corrcoef(pred[i, :], true[i, :],)[0, 1]
        gene = np.zeros(pred.shape[1])
        for i in range(pred.shape[1]):
            gene[i] = np.corrcoef(pred[:, i], true[:, i],)[0, 1]
    return cell, gene


def score(pred, true, markers=(), n_top=50, notebook_indexing=False):
    """The seven summaries and the index lists of one fold.  ``top_sum`` / ``top_var`` are best first with equal values by
    descending gene index (a stable argsort read backwards; the notebook's default argsort leaves ties open).
    ``notebook_indexing``: the three index means as the notebook computes them -- on the compacted vector (may raise
    IndexError); otherwise on the full vector."""
    cell, gene = correlations(pred, true)
    cell_ok, gene_ok = cell[~np.isnan(cell)], gene[~np.isnan(gene)]
    top_sum = np.argsort(np.sum(true, axis=0), kind="stable")[-n_top:][::-1]
    top_var = np.argsort(np.var(true, axis=0), kind="stable")[-n_top:][::-1]
    corr = gene_ok if notebook_indexing else gene
    mk = np.asarray(markers, dtype=np.int64)
    return {"cell_pcc": cell, "pcc": gene, "top_sum": top_sum, "top_var": top_var,
            "cell_mean": float(np.mean(cell_ok)) if cell_ok.size else float("nan"),
            "n_cells_valid": int(cell_ok.size), "n_genes_valid": int(gene_ok.size),
            "max_r": float(np.max(gene_ok)) if gene_ok.size else float("nan"),
            "heg_mean": float(np.mean(corr[top_sum[::-1]])), "hvg_mean": float(np.mean(corr[top_var[::-1]])),
            "marker_mean": float(np.mean(corr[mk])) if mk.size else float("nan")}


def rel_close(a, b, rel=1e-12):
    """Scalars equal within ``rel`` relative, NaN only where the other is NaN."""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) <= rel * max(abs(b), 1e-300)
