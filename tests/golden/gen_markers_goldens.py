"""Generates tests/golden/markers.npz: what scipy and mpmath give for the procedural cases of tests/markers_reference.py
(``make_case`` regenerates the inputs from the seed, so only results are stored), and the restatement's own largest error
against them per case.

    python tests/golden/gen_markers_goldens.py

Stored per scipy case ``<name>.``: ``rank2`` (twice ``scipy.stats.rankdata``), ``z`` / ``p`` (``ranksums``), ``U`` / ``p_tc``
(``mannwhitneyu(use_continuity=False, method="asymptotic")``), ``t`` / ``p_t`` / ``df`` (``ttest_ind(equal_var=False)``),
``adj`` (``false_discovery_control`` of ``p``), ``order`` (stable descending order of ``z``), and the errors.  Per mpmath
case: -log10 p at 50 digits at the restatement's own z and (t, nu), where fp64 p underflows.

Where a test compares an order against scipy-derived scores, adjacent scores of the fixture must be exactly equal or
further apart than the score tolerance, so that neither a tie-break nor a rounding can flip a position: checked here."""
import os
import sys

import mpmath
import numpy as np
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import markers_reference as mr  # noqa: E402

EPS = 2.0 ** -52
SCORE_ULPS = 8
# name -> make_case arguments.  "check": the column set the formulas were first checked on (257 values, 5 groups, half
# zeros, the rest on a grid of thirds)
SCIPY_CASES = {
    "check": dict(n=257, G=40, k=5, seed=7, kind="grid", dtype=np.float64),
    "counts": dict(n=301, G=24, k=3, seed=11, kind="counts", dtype=np.float32),
    "cont": dict(n=190, G=16, k=4, seed=13, kind="cont", dtype=np.float64, drop=0.1),
}
MP_CASES = {"big": dict(n=4000, G=6, k=2, seed=17, kind="cont", dtype=np.float64, shift=3.0)}


def rel(a, b):
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r)))


def gap_ok(scores):
    for row in scores:
        s = np.sort(row)[::-1]
        d = s[:-1] - s[1:]
        if ((d != 0) & (d <= 4 * SCORE_ULPS * EPS * np.abs(s).max())).any():
            return False
    return True


def main():
    mpmath.mp.dps = 50
    out = {}
    for name, kw in SCIPY_CASES.items():
        x, labels = mr.make_case(**kw)
        k = kw["k"]
        keep = labels >= 0
        xs, ls = x[keep].astype(np.float64), labels[keep]
        G = xs.shape[1]
        rank2 = np.stack([np.rint(2 * stats.rankdata(xs[:, j])).astype(np.int64) for j in range(G)], axis=1)
        z, p, U, p_tc, t, p_t, df = (np.zeros((k, G)) for _ in range(7))
        for g in range(k):
            a, b = xs[ls == g], xs[ls != g]
            for j in range(G):
                r = stats.ranksums(a[:, j], b[:, j])
                z[g, j], p[g, j] = r.statistic, r.pvalue
                m = stats.mannwhitneyu(a[:, j], b[:, j], use_continuity=False, method="asymptotic")
                U[g, j], p_tc[g, j] = m.statistic, m.pvalue
            tt = stats.ttest_ind(a, b, equal_var=False)
            t[g], p_t[g], df[g] = tt.statistic, tt.pvalue, tt.df
        adj = np.stack([stats.false_discovery_control(p[g], method="bh") for g in range(k)])
        assert gap_ok(z) and gap_ok(t), f"{name}: adjacent scores closer than the tolerance; pick another seed"
        w = mr.rank_genes_groups(x, labels, k, "wilcoxon")
        wt = mr.rank_genes_groups(x, labels, k, "wilcoxon", tie_correct=True)
        tr = mr.rank_genes_groups(x, labels, k, "t-test")
        assert np.array_equal(w["R2"], np.stack([rank2[ls == g].sum(axis=0) for g in range(k)]))
        ng = w["group_sizes"].astype(np.float64)[:, None]
        assert np.array_equal(w["R2"] / 2.0 - ng * (ng + 1) / 2.0, U)
        # the restatement's p against mpmath at its own statistic (no conditioning in the comparison)
        p_mp = np.array([[float(mpmath.erfc(abs(mpmath.mpf(v)) / mpmath.sqrt(2))) for v in row] for row in w["full_scores"]])
        nu = _welch_nu(tr)
        pt_mp = np.array([[float(mpmath.betainc(mpmath.mpf(n_) / 2, 0.5, 0, mpmath.mpf(n_) / (mpmath.mpf(n_) + mpmath.mpf(v) ** 2),
                                                regularized=True)) for v, n_ in zip(rv, rn)]
                          for rv, rn in zip(tr["full_scores"], nu)])
        out.update({f"{name}.rank2": rank2, f"{name}.z": z, f"{name}.p": p, f"{name}.U": U, f"{name}.p_tc": p_tc,
                    f"{name}.t": t, f"{name}.p_t": p_t, f"{name}.df": df, f"{name}.adj": adj,
                    f"{name}.order": np.stack([mr.score_order(z[g]) for g in range(k)]),
                    f"{name}.order_t": np.stack([mr.score_order(t[g]) for g in range(k)]),
                    f"{name}.err_z": rel(w["full_scores"], z), f"{name}.err_p": rel(w["full_pvals"], p),
                    f"{name}.err_p_tc": rel(wt["full_pvals"], p_tc), f"{name}.err_t": rel(tr["full_scores"], t),
                    f"{name}.err_p_t": rel(tr["full_pvals"], p_t), f"{name}.err_adj": rel(w["full_pvals_adj"], adj),
                    f"{name}.err_p_mp": rel(w["full_pvals"], p_mp), f"{name}.err_p_t_mp": rel(tr["full_pvals"], pt_mp)})
    for name, kw in MP_CASES.items():
        x, labels = mr.make_case(**kw)
        k = kw["k"]
        w = mr.rank_genes_groups(x, labels, k, "wilcoxon")
        tr = mr.rank_genes_groups(x, labels, k, "t-test")
        nu = _welch_nu(tr)
        nl_w = np.array([[float(-mpmath.log10(mpmath.erfc(abs(mpmath.mpf(v)) / mpmath.sqrt(2)))) for v in row]
                         for row in w["full_scores"]])
        nl_t = np.array([[float(-mpmath.log10(mpmath.betainc(mpmath.mpf(n_) / 2, 0.5, 0,
                                                             mpmath.mpf(n_) / (mpmath.mpf(n_) + mpmath.mpf(v) ** 2),
                                                             regularized=True))) for v, n_ in zip(rv, rn)]
                         for rv, rn in zip(tr["full_scores"], nu)])
        assert (w["full_pvals"] == 0).any(), f"{name}: no p underflows; make the markers stronger"
        out.update({f"{name}.z": w["full_scores"], f"{name}.t": tr["full_scores"], f"{name}.nu": nu, f"{name}.nl_w": nl_w,
                    f"{name}.nl_t": nl_t, f"{name}.err_nl_w": rel(w["full_neglog10_pvals"], nl_w),
                    f"{name}.err_nl_t": rel(tr["full_neglog10_pvals"], nl_t)})
    path = mr.GOLDEN
    np.savez_compressed(path, **out)
    for key in sorted(out):
        if ".err" in key:
            print(f"{key}: {float(out[key]):.3e} ({float(out[key]) / EPS:.1f} eps)")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


def _welch_nu(tr):
    """The Welch-Satterthwaite nu of the restatement's own moments, as it computes it."""
    ng = tr["group_sizes"].astype(np.float64)[:, None]
    nr = tr["n_valid"] - ng
    a, b = tr["vars"] / ng, tr["vars_rest"] / nr
    return ((a + b) * (a + b)) / ((a * a) / (ng - 1.0) + (b * b) / (nr - 1.0))


if __name__ == "__main__":
    main()
