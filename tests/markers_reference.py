"""fp64 numpy restatement of the marker-gene computation (tests only), for the tests of mclstexp_amd.markers.

One slide at a time, line by line what DESIGN 6.15 states: rows labelled -1 are dropped first; per group g against the
rest (scanpy's ``reference="rest"``) the moments, the log fold change, the Wilcoxon rank-sum z with exact integer rank sums
``R2`` (twice the tie-averaged ranks) and tie terms ``T``, the Welch t with the Welch-Satterthwaite nu and its two-sided p
``I_{nu / (nu + t^2)}(nu / 2, 1 / 2)`` by the same log-space algorithm as csrc/markers.hip, ``-log10 p`` in log space,
Benjamini-Hochberg over the genes, and the order (descending score, equal scores by gene index -- scanpy's
``argpartition`` leaves that order open).  The sums are taken in extended precision and rounded once, so the restatement's
own summation error is below one ulp of the result.  ``c = 1 - T / (N^3 - N)`` is evaluated as ``((N^3 - N) - T) /
(N^3 - N)``: the same number with one rounding instead of a cancelling subtraction.

Pinned against scipy and mpmath by tests/test_markers_host.py (tests/golden/markers.npz).  scanpy is not installed:
parity with a scanpy release is unpinned."""
import os

import numpy as np
from scipy import special

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "markers.npz")
METHODS = ("wilcoxon", "t-test", "t-test_overestim_var")
CF_MAX_ITER = 1000
LN10 = 2.302585092994046
LGAMMA_HALF = 0.5723649429247001
EPS = 2.0 ** -52


def make_case(n, G, k, seed, kind="grid", dtype=np.float32, drop=0.0, shift=0.6):
    """A procedural slide: ``x`` (n, G) of log1p-like values, ``labels`` (n,) in [0, k) with a fraction ``drop`` set to -1.
    ``kind``: "grid" half zeros and the rest on a grid of thirds (many ties), "counts" small integers, "zeros" 90 % zeros,
    "cont" continuous.  Group g shifts gene j up when j % k == g, so every group has markers."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k, size=n).astype(np.int32)
    labels[:min(n, k)] = np.arange(min(n, k))                     # every group that fits is carried
    if kind == "grid":
        x = rng.integers(0, 10, size=(n, G)) / 3.0 * (rng.random((n, G)) < 0.5)
    elif kind == "counts":
        x = rng.poisson(1.5, size=(n, G)).astype(np.float64)
    elif kind == "zeros":
        x = rng.gamma(2.0, 1.0, size=(n, G)) * (rng.random((n, G)) < 0.1)
    else:
        x = rng.gamma(2.0, 0.5, size=(n, G))
    mark = (np.arange(G)[None, :] % k) == labels[:, None]
    if kind == "counts":
        x = x + mark * rng.integers(0, 3, size=(n, G))
    elif kind == "grid":
        x = x + mark * (rng.integers(0, 4, size=(n, G)) / 3.0)
    else:
        x = x + mark * shift * rng.random((n, G)) * (x != 0)
    if drop > 0:
        labels[rng.random(n) < drop] = -1
        labels[:2] = [0, min(1, k - 1)]                           # two kept rows at least
    return np.ascontiguousarray(x.astype(dtype)), labels


def _sum(a, axis=0):
    return np.sum(a.astype(np.longdouble), axis=axis).astype(np.float64)


def rankdata2(col):
    """Twice the tie-averaged 1-based ranks of one column (exact integers), and T = sum over tie runs of t^3 - t.
    -0.0 == +0.0 compare equal, as in scipy.stats.rankdata."""
    order = np.argsort(col, kind="stable")
    s = col[order]
    n = s.size
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    end = np.concatenate([start[1:], [n]]) - 1
    t = (end - start + 1).astype(np.int64)
    r2_sorted = np.repeat(start + end + 2, t).astype(np.int64)
    r2 = np.empty(n, dtype=np.int64)
    r2[order] = r2_sorted
    return r2, int((t ** 3 - t).sum())


def log_betacf(a, b, x):
    """log of the continued fraction of I_x(a, b) (modified Lentz), elementwise on arrays; NaN where not converged."""
    tiny, tol = 1e-300, 4.440892098500626e-16
    a, b, x = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(x, np.float64))
    qab, qap, qam = a + b, a + 1.0, a - 1.0

    def floor_(v):
        return np.where(np.abs(v) < tiny, tiny, v)

    with np.errstate(all="ignore"):
        c = np.ones_like(x)
        d = 1.0 / floor_(1.0 - qab * x / qap)
        h = d.copy()
        out = np.full_like(x, np.nan)
        live = np.ones(x.shape, dtype=bool)
        for m in range(1, CF_MAX_ITER + 1):
            dm, m2 = float(m), 2.0 * m
            aa = dm * (b - dm) * x / ((qam + m2) * (a + m2))
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


def student_p(t, nu):
    """(p, neglog10p) of Student's t, two-sided, elementwise: I_{nu / (nu + t^2)}(nu / 2, 1 / 2) in log space."""
    t, nu = np.asarray(t, np.float64), np.asarray(nu, np.float64)
    p, nl = np.ones_like(t), np.zeros_like(t)
    with np.errstate(all="ignore"):
        t2, a, b = t * t, 0.5 * nu, 0.5
        inf = np.isinf(t2)
        p[inf], nl[inf] = 0.0, np.inf
        live = (t2 != 0.0) & ~inf
        x = nu / (nu + t2)
        logx, logy = -np.log1p(t2 / nu), -np.log1p(nu / t2)
        logB = (special.gammaln(a) + LGAMMA_HALF) - special.gammaln(a + b)
        direct = live & (x < (a + 1.0) / (a + b + 2.0))
        if direct.any():
            lp = ((a * logx + b * logy) - np.log(a) - logB)[direct] + log_betacf(a[direct], b, x[direct])
            lp = np.where(lp > 0.0, 0.0, lp)
            p[direct], nl[direct] = np.exp(lp), 0.0 - lp / LN10
        other = live & ~direct
        if other.any():
            y = t2 / (nu + t2)
            lq = ((b * logy + a * logx) - np.log(b) - logB)[other] + log_betacf(b, a[other], y[other])
            lq = np.where(lq > 0.0, 0.0, lq)
            p[other], nl[other] = 0.0 - np.expm1(lq), 0.0 - np.log1p(0.0 - np.exp(lq)) / LN10
    bad = np.isnan(p)
    p[bad], nl[bad] = 1.0, 0.0
    return p, nl


def normal_p(z):
    """(p, neglog10p) of a standard normal z, two-sided: erfc(|z| / sqrt 2), -log10 of it through erfcx where it is small."""
    az = np.abs(z) / 1.4142135623730951
    p = special.erfc(az)
    with np.errstate(all="ignore"):
        nl = np.where(az < 1.0, 0.0 - np.log10(p), (az * az - np.log(special.erfcx(az))) / LN10)
    return p, nl


def benjamini_hochberg(p):
    """scipy.stats.false_discovery_control(method="bh") of one vector, NaN as 1, back in the input's order."""
    p = np.where(np.isnan(p), 1.0, p)
    G = p.size
    order = np.argsort(p, kind="stable")
    q = p[order] * (float(G) / np.arange(1, G + 1))
    q = np.minimum.accumulate(q[::-1])[::-1]
    out = np.empty(G)
    out[order] = np.minimum(q, 1.0)
    return out


def score_order(scores, rankby_abs=False):
    v = np.abs(scores) if rankby_abs else scores
    return np.argsort(-v, kind="stable")


def rank_genes_groups(x, labels, k, method="wilcoxon", tie_correct=False, n_genes=None, rankby_abs=False):
    """One slide.  Returns a dict of (k, G) arrays in gene order (``means``, ``vars``, ``means_rest``, ``vars_rest``,
    ``pts``, ``pts_rest``, ``nnz``, ``nnz_rest``, ``R2``, ``full_scores``, ``full_pvals``, ``full_pvals_adj``,
    ``full_neglog10_pvals``, ``full_logfoldchanges``), ``T`` (G,), ``group_sizes`` (k,), ``n_valid``, and the ordered
    (k, n_genes) ``names``, ``scores``, ``pvals``, ``pvals_adj``, ``neglog10_pvals``, ``logfoldchanges``."""
    assert method in METHODS
    keep = np.asarray(labels) >= 0
    x = np.asarray(x)[keep].astype(np.float64)
    lab = np.asarray(labels)[keep]
    N, G = x.shape
    n_genes = G if n_genes is None else n_genes
    r2 = np.empty((N, G), dtype=np.int64)
    T = np.empty(G, dtype=np.int64)
    for j in range(G):
        r2[:, j], T[j] = rankdata2(x[:, j])
    out = {name: np.full((k, G), np.nan) for name in
           ("means", "vars", "means_rest", "vars_rest", "pts", "pts_rest", "full_scores", "full_pvals",
            "full_pvals_adj", "full_neglog10_pvals", "full_logfoldchanges")}
    out.update(nnz=np.zeros((k, G), np.int32), nnz_rest=np.zeros((k, G), np.int32), R2=np.zeros((k, G), np.int64), T=T,
               group_sizes=np.zeros(k, np.int32), n_valid=N)
    with np.errstate(all="ignore"):
        for g in range(k):
            m = lab == g
            xg, xr = x[m], x[~m]
            ng, nr = int(m.sum()), int(N - m.sum())
            out["group_sizes"][g] = ng
            mg, mr = _sum(xg) / np.float64(ng), _sum(xr) / np.float64(nr)
            vg = _sum((xg - mg) * (xg - mg)) / np.float64(ng - 1) if ng >= 2 else np.full(G, np.nan)
            vr = _sum((xr - mr) * (xr - mr)) / np.float64(nr - 1) if nr >= 2 else np.full(G, np.nan)
            out["means"][g], out["vars"][g], out["means_rest"][g], out["vars_rest"][g] = mg, vg, mr, vr
            out["nnz"][g], out["nnz_rest"][g] = (xg != 0).sum(axis=0), (xr != 0).sum(axis=0)
            out["pts"][g] = out["nnz"][g] / np.float64(ng)
            out["pts_rest"][g] = out["nnz_rest"][g] / np.float64(nr)
            out["R2"][g] = r2[m].sum(axis=0)
            if method == "wilcoxon":
                num = out["R2"][g] / 2.0 - ng * (N + 1) / 2.0
                c = ((N ** 3 - N) - T) / np.float64(N ** 3 - N) if tie_correct else 1.0
                den = np.sqrt(c * np.float64(ng * nr * (N + 1)) / 12.0)
                z = num / den
                z = np.where(np.isnan(z) | ~(den > 0.0), 0.0, z)
                score = z
                p, nl = normal_p(z)
            else:
                nrr = float(ng if method == "t-test_overestim_var" else nr)
                a, b = vg / float(ng), vr / nrr
                t = (mg - mr) / np.sqrt(a + b)
                nu = ((a + b) * (a + b)) / ((a * a) / (float(ng) - 1.0) + (b * b) / (nrr - 1.0))
                bad = np.isnan(t) | np.isnan(nu)
                score = np.where(bad, 0.0, t)
                p, nl = student_p(np.where(bad, 0.0, t), np.where(bad, 1.0, nu))
            out["full_scores"][g], out["full_pvals"][g], out["full_neglog10_pvals"][g] = score, p, nl
            out["full_pvals_adj"][g] = benjamini_hochberg(p)
            out["full_logfoldchanges"][g] = np.log2((np.expm1(mg) + 1e-9) / (np.expm1(mr) + 1e-9))
    names = np.stack([score_order(out["full_scores"][g], rankby_abs)[:n_genes] for g in range(k)]).astype(np.int64)
    out["names"] = names
    for key in ("scores", "pvals", "pvals_adj", "neglog10_pvals", "logfoldchanges"):
        out[key] = np.take_along_axis(out["full_" + key], names, axis=1)
    return out


def marker_recovery(pred, true, labels, k, n_top=50, **kw):
    """Overlap count and Jaccard index (k,) of the top ``n_top`` markers of every group, predicted against measured."""
    a = rank_genes_groups(pred, labels, k, n_genes=n_top, **kw)["names"]
    b = rank_genes_groups(true, labels, k, n_genes=n_top, **kw)["names"]
    overlap = np.array([np.intersect1d(a[g], b[g]).size for g in range(k)], dtype=np.int64)
    return overlap, overlap / (2.0 * a.shape[1] - overlap)
