"""fp64 numpy restatement of the gene-significance computation (tests only), for the tests of mclstexp_amd.genes.

``pearson_pvalue``: the two-sided p-value of ``scipy.stats.pearsonr`` (the second output of the reference's get_R,
utils.py:52-65), by the SAME log-space algorithm as csrc/gene_significance.hip: ``log p = log 2 + log I_x(a, a)`` with
``a = n / 2 - 1``, ``x = (1 - |r|) / 2``, the prefactor ``lgamma(2a) - 2 lgamma(a) + a log x + a log1p(-x) - log a`` and
the modified-Lentz continued fraction; ``-log10 p`` comes from ``log p`` and stays finite where ``p`` underflows.

``tutorial_table``: the pandas block of the reference's tutorial.ipynb (third cell), line for line: the genes x slides
frame of ``-log10 p``, ``mean(axis=1)``, ``sort_values(ascending=False)``, ``head``, ``idxmax``.

Pinned against scipy, mpmath and pandas' own results by tests/test_genes_host.py (tests/golden/gene_significance.npz)."""
import math
import os
import warnings

import numpy as np
import pandas as pd

from eval_reference import pearson_r

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gene_significance.npz")
# name -> synth.make_eval_case arguments (as tests/golden/gen_gene_goldens.py generates them)
GENE_CASES = {
    "folds": dict(segments=[120, 2, 77, 301], genes=171, seed=2, const_true=[5], const_pred=[7], heg_const=True),
    "her2st8": dict(segments=[346, 160, 295, 176, 350, 252, 311, 203], genes=785, seed=21, const_true=[3],
                    const_pred=[10]),
    "tenx": dict(segments=[4784, 2432, 1211], genes=40, seed=31),
}
UNDERFLOW_CASE = "tenx"
TOP_N = 7
CF_MAX_ITER = 1000
LN2 = 0.6931471805599453
LN10 = 2.302585092994046


def log_betacf_sym(a, x):
    """log of the continued fraction of I_x(a, a) for arrays ``x`` <= 1/2 (modified Lentz); NaN where not converged."""
    tiny, tol = 1e-300, 4.440892098500626e-16
    x = np.asarray(x, dtype=np.float64)
    qab, qap, qam = 2.0 * a, a + 1.0, a - 1.0

    def floor_(v):
        return np.where(np.abs(v) < tiny, tiny, v)

    c = np.ones_like(x)
    d = 1.0 / floor_(1.0 - qab * x / qap)
    h = d.copy()
    out = np.full_like(x, np.nan)
    live = np.ones(x.shape, dtype=bool)
    for m in range(1, CF_MAX_ITER + 1):
        dm, m2 = float(m), 2.0 * m
        aa = dm * (a - dm) * x / ((qam + m2) * (a + m2))
        d = 1.0 / floor_(1.0 + aa * d)
        c = floor_(1.0 + aa / c)
        h = h * (d * c)
        aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2))
        d = 1.0 / floor_(1.0 + aa * d)
        c = floor_(1.0 + aa / c)
        delta = d * c
        h = h * delta
        done = live & (np.abs(delta - 1.0) <= tol)
        out[done] = np.log(h[done])
        live &= ~done
        if not live.any():
            break
    return out


def pearson_pvalue(r, n):
    """(p, neglog10p) of the (G,) Pearson r of one slide of ``n`` spots."""
    r = np.asarray(r, dtype=np.float64)
    p = np.full(r.shape, np.nan)
    nl = np.full(r.shape, np.nan)
    ok = ~np.isnan(r)
    if n < 2:
        return p, nl
    if n == 2:
        p[ok], nl[ok] = 1.0, 0.0
        return p, nl
    one = ok & (np.abs(r) >= 1.0)
    p[one], nl[one] = 0.0, np.inf
    reg = ok & ~one
    a = 0.5 * n - 1.0
    x = 0.5 * (1.0 - np.abs(r[reg]))
    pre = math.lgamma(2.0 * a) - 2.0 * math.lgamma(a) + a * np.log(x) + a * np.log1p(-x) - math.log(a)
    lp = LN2 + pre + log_betacf_sym(a, x)
    lp = np.where(lp > 0.0, 0.0, lp)
    nl[reg] = 0.0 - lp / LN10
    p[reg] = np.exp(lp)
    return p, nl


def significance(pred, true, offsets):
    """(r, p, neglog10p), each (S, G), of row-stacked folds."""
    rs, ps, ns = [], [], []
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        r = pearson_r(pred[lo:hi], true[lo:hi])
        p, nl = pearson_pvalue(r, hi - lo)
        rs.append(r), ps.append(p), ns.append(nl)
    return np.stack(rs), np.stack(ps), np.stack(ns)


def reference_neglog10(p):
    """``-np.log10(p)`` as the tutorial writes it: +inf where p underflowed to 0."""
    with np.errstate(divide="ignore"):
        return -np.log10(np.asarray(p, dtype=np.float64))


def tutorial_table(neglog10p, r, genes, slides, top_n=TOP_N):
    """The tutorial's table block over ``neglog10p`` (S, G) (there: ``-np.log10(p_value_list)`` per slide) and ``r``
    (S, G).  Returns the sorted frame, ``mean`` (G,) in gene order, ``order`` = the gene indices in sorted order and
    ``top`` = [(gene index, slide index, value, pcc)] of the first ``top_n`` rows.  Needs unique gene names."""
    genes, slides = list(genes), list(slides)
    result_df = pd.DataFrame(index=genes, columns=slides)
    for fold, name in enumerate(slides):
        result_df[name] = neglog10p[fold]
    result_df["avg_p_value"] = result_df.mean(axis=1)
    sorted_result_df = result_df.sort_values(by="avg_p_value", ascending=False)
    top = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for gene, row in sorted_result_df.head(top_n).iterrows():
            max_p_value_slice = row.idxmax()
            max_p_value = row[max_p_value_slice]
            s = slides.index(max_p_value_slice)      # 'avg_p_value' is not a slide: raises if the mean is the maximum
            g = genes.index(gene)
            top.append((g, s, float(max_p_value), float(r[s][g])))
    mean = result_df["avg_p_value"].to_numpy(dtype=np.float64)
    order = np.array([genes.index(g) for g in sorted_result_df.index], dtype=np.int64)
    return sorted_result_df, mean, order, top


def stable_order(mean):
    """Descending by mean, equal means by ascending gene index, NaN last: the library's tie rule (pandas' default
    quicksort leaves the order of equal keys unspecified)."""
    m = np.asarray(mean, dtype=np.float64)
    key = np.where(np.isnan(m), -np.inf, m)
    return np.lexsort((np.arange(m.size), -key, np.isnan(m))).astype(np.int64)


def format_line(gene, slide, value, pcc):
    """The line the tutorial prints per top gene."""
    return f"Gene: {gene}, Max -log(p-value) in {slide}: {value}, PCC in {slide}: {pcc}"
