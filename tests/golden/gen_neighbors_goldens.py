"""Writes tests/golden/neighbors.npz: the inputs of the cases of tests/neighbors_reference.py and, per case and quantity,
how far the restatement itself can be trusted.  The tests recompute every expectation with the restatement.

    python tests/golden/gen_neighbors_goldens.py

err_<case>_<rho|sigma|data>: the larger of the float64 restatement's deviation from its np.longdouble run and from a float64
run on inputs perturbed in the last place, relative to max |value| and floored at 2^-53.  <case>_rho_agree: the rows whose
rho the float64 and longdouble runs give identically.  Refuses to write unless the reference alone is stable: identical
neighbour lists in the float64, longdouble and perturbed runs, and no bisection step within 1e-9 of its stopping bound.
For the random cases it also checks sklearn's brute-force kneighbors (sklearn 1.7.2) against the restatement's index sets
and records the share of rows skipped for a near-tie at the k-th place (sklearn_skipped_<case>, below 1 %)."""
import os
import sys

import numpy as np
from sklearn.neighbors import NearestNeighbors

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neighbors_reference as nr  # noqa: E402

LD = np.longdouble
FLOOR = 2.0 ** -53
GUARD = 1e-9


def perturb(a, seed):
    rng = np.random.RandomState(seed)
    return np.asarray(a, dtype=np.float64) * (1.0 + 2.0 ** -52 * rng.choice([-1.0, 1.0], size=np.shape(a)))


def err(base, *others):
    scale = np.max(np.abs(base))
    return max(FLOOR, *(float(np.max(np.abs(np.asarray(o, dtype=LD) - base)) / scale) for o in others))


def main():
    out = {}
    for name, (sizes, D, k) in nr.CASES.items():
        X = nr.make_case(name)
        off = nr.offsets_of(name)
        out[f"{name}_X"] = X
        base, ld, pt = nr.segments(name, X), nr.segments(name, X, LD), nr.segments(name, perturb(X, 31))
        e = {"rho": FLOOR, "sigma": FLOOR, "data": FLOOR}
        agree, skipped, margin = [], 0, np.inf
        for s, (g, g_ld, g_pt) in enumerate(zip(base, ld, pt)):
            assert np.array_equal(g["knn_indices"], g_ld["knn_indices"]), (name, s, "longdouble lists differ")
            if name in nr.RANDOM:
                assert np.array_equal(g["knn_indices"], g_pt["knn_indices"]), (name, s, "perturbed lists differ")
            for run in (g, g_ld, g_pt):
                assert run["info"]["margin"] >= GUARD, (name, s, run["info"]["margin"])
                margin = min(margin, run["info"]["margin"])
            others = (g_ld, g_pt) if name in nr.RANDOM else (g_ld,)     # a perturbed duplicate is no duplicate
            for q in ("rho", "sigma"):
                e[q] = max(e[q], err(g[q], *(o[q] for o in others)))
            e["data"] = max(e["data"], err(g["dense"], *(o["dense"] for o in others)))
            agree.append(g["rho"] == g_ld["rho"].astype(np.float64))
            if name in nr.RANDOM:
                Xs = X[off[s]:off[s + 1]]
                n = Xs.shape[0]
                _, sk = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(Xs).kneighbors(Xs)
                d2 = np.sort(nr.sq_distances(Xs), axis=1)               # column 0 is the row itself
                kth = np.sqrt(d2[:, k - 1])
                nxt = np.sqrt(d2[:, k]) if k < n else np.full(n, np.inf)
                clear = (nxt - kth) > 1e-9 * kth
                skipped += int((~clear).sum())
                for i in np.flatnonzero(clear):
                    assert set(sk[i].tolist()) == set(g["knn_indices"][i].tolist()), (name, s, i)
        for q, v in e.items():
            out[f"err_{name}_{q}"] = v
        out[f"{name}_rho_agree"] = np.concatenate(agree)
        out[f"margin_{name}"] = margin
        if name in nr.RANDOM:
            out[f"sklearn_skipped_{name}"] = skipped / X.shape[0]
            assert out[f"sklearn_skipped_{name}"] < 0.01, (name, skipped)
        print(name, {q: f"{v:.3e}" for q, v in e.items()}, "margin", f"{margin:.3e}", "rho agree",
              float(out[f"{name}_rho_agree"].mean()), "sklearn skipped", out.get(f"sklearn_skipped_{name}"))
    np.savez_compressed(nr.GOLDEN, **out)
    print("wrote", nr.GOLDEN, os.path.getsize(nr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
