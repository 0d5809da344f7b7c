"""CPU restatement of what the reference's hvg_*.py scripts ask of scanpy per slide (hvg_her2st.py:35-37):

    sc.pp.normalize_total(adata); sc.pp.log1p(adata); sc.pp.highly_variable_genes(adata, n_top_genes=n)

TEST INFRASTRUCTURE ONLY.  Parity status: "parity unpinned" -- scanpy and anndata are un-vendored dependencies absent
here, so the functions below restate, line by line, scanpy 1.9's ``normalize_total`` / ``_normalize_data``
(preprocessing/_normalization.py), ``_get_mean_var`` (preprocessing/_utils.py) and
``_highly_variable_genes_single_batch`` (preprocessing/_highly_variable_genes.py, flavor="seurat", n_bins=20) from their
published source, with pandas' OWN ``cut`` and ``groupby(...).mean() / .std(ddof=1)`` doing the binning exactly as scanpy
has them do it.

Two modes:
  dtype=np.float32   what scanpy does to an integer matrix: cast to fp32, divide by the fp64 size factors into fp32,
                     ``log1p`` and (inside highly_variable_genes) ``expm1`` in fp32, fp32 squares, fp64 means;
  dtype=np.float64   the form csrc/preprocess.hip implements: the same steps in fp64 without the log1p / expm1 round trip
                     (the identity).  ``sums="fsum"`` replaces numpy's column and row sums by exactly rounded ones
                     (math.fsum): the gap between the two is the yardstick of the GPU tolerance.
"""
import math
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hvg.npz")
N_BINS = 20
CONTINUOUS = ("means", "dispersions", "dispersions_norm", "cutoff", "target_sum")

# name -> (n_top_genes or None = chosen by the generator, [make_counts_case kwargs per slide])
_RAGGED = (97, 350, 613, 211, 128, 402)
HVG_CASES = {
    "ragged": (200, [dict(spots=n, genes=1200, seed=10 + i, zero_genes=3 * (i % 3), zero_spot=(i == 2))
                     for i, n in enumerate(_RAGGED)]),
    "zero_genes": (150, [dict(spots=300, genes=800, seed=21, zero_genes=9)]),
    "zero_spot": (150, [dict(spots=257, genes=800, seed=22, zero_spot=True)]),
    "single_bin": (150, [dict(spots=300, genes=800, seed=23, top_gene=True)]),
    "n_top_large": (5000, [dict(spots=200, genes=600, seed=24, zero_genes=5)]),
    "neg_cutoff": (700, [dict(spots=300, genes=800, seed=25, zero_genes=6)]),
    "tie": (None, [dict(spots=300, genes=800, seed=26, duplicate=(660, 517))]),
}
TIE_RANK_WINDOW = (100, 300)    # the generator asserts that the duplicated pair ranks in here


def _col_sums(x, sums):
    if sums == "fsum":
        return np.array([math.fsum(x[:, g]) for g in range(x.shape[1])], dtype=np.float64)
    return np.sum(x, axis=0, dtype=np.float64)


def normalize_total(counts, dtype=np.float64, sums="numpy"):
    """normalize_total(adata, target_sum=None) -> (X normalised, target).  scanpy: ``counts_per_cell = X.sum(1)``;
    ``_normalize_data``: integer X -> float32; ``after = np.median(counts[counts > 0])``; ``counts += counts == 0``;
    ``counts = counts / after``; ``np.divide(X, counts[:, None], out=X)``."""
    c = np.asarray(counts)
    if dtype == np.float32:
        x = c.astype(np.float32) if np.issubdtype(c.dtype, np.integer) else c.copy()
        per_cell = np.ravel(c.sum(1))                       # int64 for an integer matrix, fp32 for an fp32 one
    else:
        x = c.astype(np.float64)
        per_cell = np.array([math.fsum(r) for r in x]) if sums == "fsum" else x.sum(1)
    per_cell = per_cell.astype(np.float64) if dtype == np.float64 else per_cell
    after = np.median(per_cell[per_cell > 0])
    per_cell = per_cell + (per_cell == 0)
    per_cell = per_cell / after
    np.divide(x, per_cell[:, None], out=x, casting="same_kind")
    return x, float(after)


def get_mean_var(x, sums="numpy"):
    """_get_mean_var: ``mean = np.mean(X, 0, dtype=float64)``; ``mean_sq = np.multiply(X, X).mean(0, dtype=float64)``;
    ``var = mean_sq - mean**2``; ``var *= n / (n - 1)``."""
    n = x.shape[0]
    mean = _col_sums(x, sums) / n
    mean_sq = _col_sums(np.multiply(x, x), sums) / n
    var = mean_sq - mean ** 2
    var *= n / (n - 1)
    return mean, var


def highly_variable_genes(counts, n_top_genes=1000, dtype=np.float64, sums="numpy"):
    """The three calls on one slide.  Returns means, dispersions, dispersions_norm (fp64), mean_bin (int32),
    highly_variable (bool), cutoff, target_sum, edges (the 21 bin edges pandas.cut used)."""
    x, target = normalize_total(counts, dtype, sums)
    if dtype == np.float32:
        x = np.log1p(x)                                     # sc.pp.log1p
        x = np.expm1(x)                                     # _highly_variable_genes_single_batch: X = np.expm1(X)
    mean, var = get_mean_var(x, sums)
    mean[mean == 0] = 1e-12                                 # set entries equal to zero to small value
    with np.errstate(divide="ignore", invalid="ignore"):
        dispersion = var / mean
        dispersion[dispersion == 0] = np.nan                # seurat: logarithmized mean and dispersion
        dispersion = np.log(dispersion)
    mean = np.log1p(mean)
    df = pd.DataFrame()
    df["means"] = mean
    df["dispersions"] = dispersion
    df["mean_bin"], edges = pd.cut(df["means"], bins=N_BINS, retbins=True)
    disp_grouped = df.groupby("mean_bin", observed=False)["dispersions"]
    disp_mean_bin = disp_grouped.mean()
    disp_std_bin = disp_grouped.std(ddof=1)
    one_gene_per_bin = disp_std_bin.isnull()                # a single gene in the bin: normalised dispersion 1
    disp_std_bin[one_gene_per_bin.values] = disp_mean_bin[one_gene_per_bin.values].values
    disp_mean_bin[one_gene_per_bin.values] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = (df["dispersions"].values - disp_mean_bin[df["mean_bin"].values].values) \
            / disp_std_bin[df["mean_bin"].values].values
    dn = norm[~np.isnan(norm)]
    dn[::-1].sort()
    n_top = min(int(n_top_genes), counts.shape[1], dn.size)
    cutoff = dn[n_top - 1]
    hv = np.nan_to_num(norm) >= cutoff
    return {"means": mean, "dispersions": dispersion, "dispersions_norm": np.asarray(norm, dtype=np.float64),
            "mean_bin": df["mean_bin"].cat.codes.values.astype(np.int32), "highly_variable": hv,
            "cutoff": np.float64(cutoff), "target_sum": np.float64(target), "edges": np.asarray(edges)}


def max_gap(a, b):
    """Largest |a - b| over the continuous outputs where both are finite; the NaN / inf patterns must coincide."""
    worst = 0.0
    for k in CONTINUOUS:
        x, y = np.atleast_1d(a[k]).astype(np.float64), np.atleast_1d(b[k]).astype(np.float64)
        fin = np.isfinite(x)
        assert np.array_equal(fin, np.isfinite(y)) and np.array_equal(x[~fin], y[~fin], equal_nan=True), k
        if fin.any():
            worst = max(worst, float(np.abs(x[fin] - y[fin]).max()))
    return worst


def edge_margin(means, edges):
    """Smallest distance of a ``means`` value to a bin edge (the lowered first edge included).  The largest mean IS the
    last edge by construction (linspace ends on it, intervals are closed on the right): that one pair is left out."""
    d = np.abs(means[:, None] - edges[None, :])
    d[means == edges[-1], -1] = np.inf
    return float(d.min())


def cutoff_margin(norm, cutoff):
    """Smallest distance to the cut-off of a non-NaN dispersions_norm that is not exactly at it (the gene that defines
    the cut-off and planted exact ties are at distance 0 by construction)."""
    v = norm[~np.isnan(norm)]
    v = v[v != cutoff]
    return float(np.abs(v - cutoff).min()) if v.size else float("inf")


def case_slides(name):
    from mclstexp_amd import synth
    return [synth.make_counts_case(**kw)["counts"] for kw in HVG_CASES[name][1]]


def shared_genes(name_lists):
    """The documented behaviour of preprocess.shared_genes, restated with sets: names made unique the way anndata's
    var_names_make_unique does (second and later occurrences get -1, -2, ...), the sorted intersection, and per slide
    the column of every shared name."""
    uniq = []
    for names in name_lists:
        seen, out = {}, []
        for n in names:
            k = seen.get(n, 0)
            out.append(n if k == 0 else f"{n}-{k}")
            seen[n] = k + 1
        uniq.append(out)
    shared = sorted(set.intersection(*[set(u) for u in uniq]))
    return shared, [np.array([u.index(n) for n in shared], dtype=np.int32) for u in uniq]
