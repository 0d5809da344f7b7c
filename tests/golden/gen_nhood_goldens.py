"""Generates tests/golden/nhood.npz: the inputs of a few small slides and what INDEPENDENT statements of the neighbourhood
counts and the co-occurrence give for them, after checking the restatement tests/nhood_reference.py against them.

    python tests/golden/gen_nhood_goldens.py

The independent statements share no arithmetic with the restatement:

* ``count_dense`` = L^T A L with A = ``spatial_reference.dense(nbr, w) != 0`` and L the one-hot label matrix (a dropped spot
  is a zero row);
* ``count_crosstab`` = a ``pandas.crosstab`` of (label of i, label of j) over the edge list of the kept slots;
* ``sims`` = the same crosstab under the PERMUTED LABEL VECTOR (spot order[pi[j]] takes the label of sorted position j),
  for the recorded permutations (``<case>.perms``, from ``spatial_reference.permutation``);
* ``pairs`` = a crosstab over ``scipy.spatial.distance.cdist(c, c, "sqeuclidean") <= r * r`` without the diagonal, on
  INTEGER coordinates with the radii 1, 2, 5, where every d^2 and r * r is an exact integer and d^2 hits r * r (25 = 3^2 +
  4^2 = 5^2 + 0, the 3-4-5 triangle), so the comparison is exact;
* ``occ`` = (pairs / row) / (col / tot) in plain Python floats.

squidpy is not installed: parity with a release is unpinned."""
import os
import sys

import numpy as np
import pandas as pd
from scipy.spatial import distance

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ligrec_reference as lr  # noqa: E402
import nhood_reference as nh  # noqa: E402
import spatial_reference as sr  # noqa: E402

PERM_SEED, PERM_P = 7, 16
RADII = np.array([1.0, 2.0, 5.0])
# name -> (grid rows, grid columns, K, seed, graph k, prune, empty group, group of one spot)
CASES = {"stripes": (20, 17, 4, 0, 8, "NA", None, None), "seven": (13, 11, 7, 2, 8, "STD", 3, 6),
         "two": (5, 8, 2, 1, 3, "NA", None, None)}


def make_case(name):
    gr, gc, K, seed, k, prune, empty, single = CASES[name]
    coords = sr.make_coords(gr, gc, seed, integer=True).astype(np.float64)
    if name == "stripes":
        labels = nh.make_stripes(gr, gc, K)[1]
    else:
        labels = lr.make_labels(coords.shape[0], K, np.random.default_rng(seed), empty=empty, single=single)
    if name == "seven":
        coords[5] = coords[4]                                    # coincident spots
    g = sr.lattice(coords, k, prune)
    return coords, labels, g["nbr"], g["w"]


def crosstab(a, b, K):
    t = pd.crosstab(pd.Series(a, name="a"), pd.Series(b, name="b"))
    return t.reindex(index=range(K), columns=range(K), fill_value=0).to_numpy().astype(np.int64)


def edge_counts(lab, nbr, w, K):
    i, c = np.nonzero(w != 0)
    j = nbr[i, c]
    keep = (lab[i] >= 0) & (lab[j] >= 0)
    return crosstab(lab[i][keep], lab[j][keep], K)


def dense_counts(lab, nbr, w, K):
    A = (sr.dense(nbr, w) != 0).astype(np.int64)
    L = np.zeros((lab.size, K), dtype=np.int64)
    L[np.flatnonzero(lab >= 0), lab[lab >= 0]] = 1
    return L.T @ A @ L


def permuted_labels(labels, perm):
    kept = np.flatnonzero(labels >= 0)
    order = kept[np.argsort(labels[kept], kind="stable")]
    out = labels.copy()
    out[order[perm]] = labels[order]
    return out


def pair_table(coords, labels, K, radii):
    kept = np.flatnonzero(labels >= 0)
    c, lab = coords[kept], labels[kept]
    d2 = distance.cdist(c, c, "sqeuclidean")
    out = []
    for r in radii:
        near = d2 <= r * r
        np.fill_diagonal(near, False)
        i, j = np.nonzero(near)
        out.append(crosstab(lab[i], lab[j], K))
    return np.stack(out)


def occ_python(pairs):
    T, K, _ = pairs.shape
    occ = np.full(pairs.shape, np.nan)
    for t in range(T):
        tot = int(pairs[t].sum())
        for a in range(K):
            row = int(pairs[t, a].sum())
            for b in range(K):
                col = int(pairs[t, :, b].sum())
                if row and col and tot:
                    occ[t, a, b] = (float(int(pairs[t, a, b])) / float(row)) / (float(col) / float(tot))
    return occ


def build():
    out = {"radii": RADII}
    for name, spec in CASES.items():
        K = spec[2]
        coords, labels, nbr, w = make_case(name)
        n = int((labels >= 0).sum())
        perms = sr.permutations(PERM_SEED, PERM_P, n)
        sims = np.stack([edge_counts(permuted_labels(labels, p), nbr, w, K) for p in perms])
        pairs = pair_table(coords, labels, K, RADII)
        rec = {"coords": coords, "labels": labels, "nbr": nbr, "w": w, "perms": perms,
               "count_dense": dense_counts(labels, nbr, w, K), "count_crosstab": edge_counts(labels, nbr, w, K),
               "sims": sims, "pairs": pairs, "occ": occ_python(pairs)}
        r = nh.nhood(labels, nbr, w, K, perms=list(perms))
        assert np.array_equal(r["count"], rec["count_dense"]) and np.array_equal(r["count"], rec["count_crosstab"]), name
        assert np.array_equal(r["sims"], sims), name
        c = nh.co_occurrence(coords, labels, K, RADII)
        assert np.array_equal(c["pairs"], pairs) and np.array_equal(c["occ"], rec["occ"], equal_nan=True), name
        out.update({f"{name}.{key}": v for key, v in rec.items()})
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nhood.npz")
    np.savez_compressed(path, **build())
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
