"""Generates tests/golden/ligrec.npz: the inputs of a few small slides and what an INDEPENDENT statement of the
ligand-receptor permutation test gives for them, after checking the restatement tests/ligrec_reference.py against it.

    python tests/golden/gen_ligrec_goldens.py

The independent statement (``independent``) shares no arithmetic with the restatement: the kept spots are subset with a
boolean mask, permutation pi is applied to the LABEL VECTOR itself (spot order[pi[j]] takes the label of sorted position
j), the group means and the counts of positive values come from pandas ``groupby``, the pairs are walked by plain Python
loops, and Benjamini-Hochberg is ``scipy.stats.false_discovery_control``.  The permutations themselves are recorded
(``<case>.perms``, from ``spatial_reference.permutation``).

Stored per case: ``x``, ``labels``, ``perms`` and the independent ``means``, ``count``, ``pvalues``, ``defined``,
``pvalues_adj`` (both axes), ``group_means``, ``group_frac``.  On the quantised cases (values multiples of 2^-12 below 16:
every sum is exact in fp64 in any order) the restatement must equal them exactly; on the continuous case the largest
relative error of its means is stored as ``cont.err_means``.  squidpy, omnipath and CellPhoneDB are not installed: parity
with a release of any of them is unpinned."""
import os
import sys

import numpy as np
import pandas as pd
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ligrec_reference as lr  # noqa: E402
import spatial_reference as sr  # noqa: E402

PERM_SEED, PERM_P, THRESHOLD = 11, 24, 0.1
# name -> (n, K, seed, quantised, empty group, group of one spot)
CASES = {"q_two": (37, 2, 1, True, None, None), "q_seven": (143, 7, 2, True, 3, 6), "cont": (90, 4, 3, False, None, None)}


def independent(x, labels, interactions, K, perms, threshold):
    """One slide, complex_policy "min", by pandas and plain loops."""
    keep = labels >= 0
    xk, lk = pd.DataFrame(x[keep].astype(np.float64)), labels[keep]
    n = int(keep.sum())
    order = np.argsort(lk, kind="stable")                      # positions within the kept subset
    sorted_labels = lk[order]
    overall = xk.mean(axis=0).to_numpy()

    def stats_of(lab):
        g = xk.groupby(lab)
        mean = g.mean().reindex(range(K)).to_numpy()
        nnz = (xk > 0).groupby(lab).sum().reindex(range(K)).fillna(0).to_numpy()
        size = pd.Series(lab).value_counts().reindex(range(K)).fillna(0).to_numpy()
        return mean, nnz, size

    mean, nnz, size = stats_of(lk)
    pairs = []
    for a, b in interactions:
        pick = []
        for side in (a, b):
            members = sorted(set(side)) if isinstance(side, tuple) else [side]
            pick.append(min(members, key=lambda gcol: (overall[gcol], gcol)))
        pairs.append(tuple(pick))
    I = len(pairs)
    means, defined, obs = np.zeros((I, K, K)), np.zeros((I, K, K), bool), np.zeros((I, K, K))
    for i, (a, b) in enumerate(pairs):
        for c1 in range(K):
            for c2 in range(K):
                m1, m2 = mean[c1, a], mean[c2, b]
                obs[i, c1, c2] = (m1 + m2) / 2
                if np.isnan(m1) or np.isnan(m2):
                    means[i, c1, c2] = np.nan
                elif m1 > 0 and m2 > 0:
                    means[i, c1, c2] = (m1 + m2) / 2
                    defined[i, c1, c2] = nnz[c1, a] >= threshold * size[c1] and nnz[c2, b] >= threshold * size[c2]
    count = np.zeros((I, K, K), dtype=np.int32)
    for perm in perms:
        lab = np.empty(n, dtype=np.int64)
        lab[order[perm]] = sorted_labels
        pm, _, _ = stats_of(lab)
        for i, (a, b) in enumerate(pairs):
            for c1 in range(K):
                for c2 in range(K):
                    count[i, c1, c2] += bool((pm[c1, a] + pm[c2, b]) / 2 >= obs[i, c1, c2])
    pvalues = np.where(defined, count / len(perms), np.nan)
    adj_c, adj_i = np.full(pvalues.shape, np.nan), np.full(pvalues.shape, np.nan)
    for i in range(I):
        ok = np.isfinite(pvalues[i])
        if ok.any():
            adj_c[i][ok] = stats.false_discovery_control(pvalues[i][ok], method="bh")
    for c1 in range(K):
        for c2 in range(K):
            ok = np.isfinite(pvalues[:, c1, c2])
            if ok.any():
                adj_i[ok, c1, c2] = stats.false_discovery_control(pvalues[ok, c1, c2], method="bh")
    with np.errstate(all="ignore"):
        frac = nnz / size[:, None]
    return {"means": means, "count": count, "pvalues": pvalues, "defined": defined, "pvalues_adj": adj_c,
            "pvalues_adj_interactions": adj_i, "group_means": mean, "group_frac": frac,
            "picked": np.asarray(pairs, dtype=np.int64)}


def rel(a, b):
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, r)
    return float(np.nanmax(r)) if r.size else 0.0


def build():
    out = {}
    for name, (n, K, seed, quantised, empty, single) in CASES.items():
        x, labels = lr.make_slide(n, K, seed, quantised=quantised, empty=empty, single=single)
        kept = int((labels >= 0).sum())
        perms = sr.permutations(PERM_SEED, PERM_P, kept)
        ind = independent(x, labels, lr.INTERACTIONS, K, perms, THRESHOLD)
        ref = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=THRESHOLD, perms=list(perms))
        used = ref["used_genes"]
        assert np.array_equal(ref["interactions"], ind["picked"]), name
        assert np.array_equal(ref["defined"], ind["defined"]), name
        if quantised:
            for key in ("means", "count", "pvalues", "pvalues_adj"):
                assert np.array_equal(ref[key], ind[key], equal_nan=True), (name, key)
            assert np.array_equal(ref["group_means"], ind["group_means"][:, used], equal_nan=True), name
            assert np.array_equal(lr.adjust(ref["pvalues"], "interactions"), ind["pvalues_adj_interactions"], equal_nan=True)
        else:
            out[f"{name}.err_means"] = max(rel(ref["means"], ind["means"]), rel(ref["group_means"], ind["group_means"][:, used]))
        out.update({f"{name}.x": x, f"{name}.labels": labels.astype(np.int16), f"{name}.perms": perms.astype(np.int16)})
        out.update({f"{name}.{key}": v for key, v in ind.items()})
    return out


def main():
    out = build()
    np.savez_compressed(lr.GOLDEN, **out)
    for key in sorted(out):
        if ".err" in key:
            print(f"{key}: {float(out[key]):.3e} ({float(out[key]) / lr.EPS:.1f} eps)")
    print(f"wrote {lr.GOLDEN}: {os.path.getsize(lr.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
