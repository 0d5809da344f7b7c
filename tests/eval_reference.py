"""fp64 numpy restatement of the reference's scoring block (tests only), for the tests of mclstexp_amd.evaluate.

Per fold: ``scipy.stats.pearsonr`` per gene as utils.py:52-65 get_R calls it (two-pass centred sums; NaN when a column
is exactly constant; clipped to [-1, 1]), the HEG genes of evel_her2st.py:200-202 with exact ties ordered by gene index,
the HEG / HVG means of evel_her2st.py:207-213 and sklearn's uniform-average MSE / MAE (evel_her2st.py:217-222).  Pinned
against the reference's own outputs by tests/test_eval_host.py (tests/golden/eval_metrics.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")
# name -> synth.make_eval_case arguments (as tests/golden/gen_eval_goldens.py generates them)
EVAL_CASES = {
    "her2st": dict(segments=[346], genes=785, seed=1, const_true=[3], const_pred=[10]),
    "folds": dict(segments=[120, 2, 77, 301], genes=171, seed=2, const_true=[5], const_pred=[7], heg_const=True),
    "g1": dict(segments=[50, 7], genes=1, seed=3),
    "g30": dict(segments=[64, 33], genes=30, seed=4, const_pred=[2]),
    "g3467": dict(segments=[250, 180], genes=3467, seed=5, const_true=[100], const_pred=[2000]),
}


def pearson_r(pred, true):
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(true, dtype=np.float64)
    dp = p - p.mean(axis=0)
    dt = t - t.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (dp * dt).sum(axis=0) / (np.sqrt((dp * dp).sum(axis=0)) * np.sqrt((dt * dt).sum(axis=0)))
    r = np.clip(r, -1.0, 1.0)
    const = (p.min(axis=0) == p.max(axis=0)) | (t.min(axis=0) == t.max(axis=0))
    r[const] = np.nan
    return r


def heg_genes(true, n_heg=50):
    m = np.asarray(true, dtype=np.float64).mean(axis=0)
    order = np.lexsort((np.arange(m.size), -m))
    return order[:min(n_heg, m.size)]


def score_fold(pred, true, n_heg=50):
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(true, dtype=np.float64)
    r = pearson_r(p, t)
    heg = heg_genes(t, n_heg)
    valid = r[~np.isnan(r)]
    return {"pcc": r, "heg_genes": heg, "heg_pcc": float(np.mean(r[heg])),
            "hvg_pcc": float(np.mean(valid)) if valid.size else float("nan"), "n_valid": int(valid.size),
            "mse": float(np.mean(np.mean((t - p) ** 2, axis=0))), "mae": float(np.mean(np.mean(np.abs(t - p), axis=0)))}


def score_segments(pred, true, offsets, n_heg=50):
    return [score_fold(pred[offsets[s]:offsets[s + 1]], true[offsets[s]:offsets[s + 1]], n_heg)
            for s in range(len(offsets) - 1)]


def rel_close(a, b, rel=1e-12):
    """Scalars equal within ``rel`` relative, NaN only where the other is NaN."""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) <= rel * max(abs(b), 1e-300)


def write_layout(root, images, spots, expressions):
    """The on-disk layout of the reference's save_embeddings (evel_her2st.py:87-119) and preprocessed matrices:
    embeddings_{f}/{img,spot}_embeddings_{i+1}.npy stored (P, N_i), expression files (G, N_i)."""
    n = len(expressions)
    for f in range(n):
        d = os.path.join(root, f"embeddings_{f}")
        os.makedirs(d, exist_ok=True)
        for i in range(n):
            np.save(os.path.join(d, f"spot_embeddings_{i + 1}.npy"), spots[f][i].T)
            np.save(os.path.join(d, f"img_embeddings_{i + 1}.npy"), images[f][i].T)
    paths = []
    for i, e in enumerate(expressions):
        p = os.path.join(root, f"slide{i}_preprocessed_matrix.npy")
        np.save(p, e.T)
        paths.append(p)
    return paths
