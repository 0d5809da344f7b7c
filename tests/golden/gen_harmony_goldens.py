"""Writes tests/golden/harmony.npz from tests/harmony_reference.py:  python tests/golden/gen_harmony_goldens.py

Per case (harmony_reference.CASES): the initial centroids Y0 that the runs replay, the objective lists, kmeans_rounds,
converged, Z_corr (every row, or every 16th / 2nd row for the cases c / e, to stay small) and the per-quantity errors err_*.
For case a also the objective's three terms, E and O after every k-means iteration; for the cases a, b and c, of the first
k-means iteration of the first round and the last one of the last round (keys <case>_first_* / <case>_last_*): Y, E, O, the
three terms, and the rows hr.slice_rows(N) of D, S and of R after the blocks 0, 1, 2 and the last; of the first and the
last correction (<case>_corrfirst_* / <case>_corrlast_*): M and W of the clusters 0, 1, 2 and those rows of Z_corr.

Y0: what harmonypy calls -- sklearn's KMeans(n_clusters=K, init="k-means++", n_init=10, max_iter=25, random_state=0) on the
unit rows Zc (sklearn 1.7.2 when this fixture was generated), replayed through init_centroids.

Tolerances are measured: the restatement runs in float64, in np.longdouble, and in float64 on Z (1 + 1e-15 u), u uniform in
[-1, 1]; err_<case>_<quantity> = the larger deviation from the float64 run, relative to max |value|, the maximum over every
step of the run.  Two assertions guard the fixture: every convergence test's left-hand side stays >= 1000 x its own deviation
away from its epsilon (so iteration counts are pinned), and Z_corr moves <= 1e-9 max |Z| under the perturbation."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import harmony_reference as hr  # noqa: E402

Z_CORR_STRIDE = {"a": 1, "b": 1, "c": 16, "d": 1, "e": 2}


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    scale = np.max(np.abs(a)) if scale is None else scale
    return float(np.max(np.abs(a - b)) / (scale if scale > 0 else 1))


def deviations(base, other):
    """Per quantity, the largest relative deviation of `other` from `base` over every step of the traced runs."""
    assert len(base["steps"]) == len(other["steps"]) and len(base["corrections"]) == len(other["corrections"])
    assert np.array_equal(base["kmeans_rounds"], other["kmeans_rounds"])
    dev = {q: 0.0 for q in hr.QUANTITIES + ("S", "M")}
    def up(q, a, b):
        dev[q] = max(dev[q], rel(a, b))
    up("Zc", base["Zc0"], other["Zc0"])
    up("Y", base["Y_init"], other["Y_init"])
    up("D", base["D_init"], other["D_init"])
    up("R", base["R_init"], other["R_init"])
    up("E", base["E_init"], other["E_init"])
    up("O", base["O_init"], other["O_init"])
    up("terms", base["terms_init"], other["terms_init"])
    for s, t in zip(base["steps"], other["steps"]):
        for q in ("Zc", "Y", "D", "S", "R", "E", "O", "terms"):
            up(q, s[q], t[q])
        for blk in s["blocks"]:
            for q in ("R", "E", "O"):
                up(q, s["blocks"][blk][q], t["blocks"][blk][q])
    for s, t in zip(base["corrections"], other["corrections"]):
        up("M", s["M"], t["M"])
        # W = A^-1 M is measured on the scale of max |Z|: with one batch it is 0 analytically
        dev["W"] = max(dev["W"], rel(s["W"], t["W"], scale=float(np.max(np.abs(base["Z_corr"])))))
        up("Z_corr", s["Z_corr"], t["Z_corr"])
        up("Zc", s["Zc"], t["Zc"])
    up("objective", base["objective_kmeans"], other["objective_kmeans"])
    return dev


def main(argv):
    from sklearn.cluster import KMeans
    doc = {}
    for name, c in hr.CASES.items():
        Z, batch, K, params, _, orders = hr.case_inputs(name)
        src = "a" if name == "e" else name
        if f"{src}_Y0" not in doc:
            km = KMeans(n_clusters=K, init="k-means++", n_init=10, max_iter=25, random_state=0)
            doc[f"{src}_Y0"] = km.fit(hr.normalize_rows(Z, True)).cluster_centers_.astype(np.float64)
        Y0 = doc[f"{src}_Y0"]
        base = hr.harmony(Z, batch, K, Y0, orders, trace=True, **params)
        wide = hr.harmony(Z, batch, K, Y0, orders, trace=True, dtype=np.longdouble, **params)
        u = np.random.RandomState(2000 + c["seed"]).uniform(-1, 1, size=Z.shape)
        pert = hr.harmony(Z * (1 + 1e-15 * u), batch, K, Y0, orders, trace=True, **params)
        dw, dp = deviations(base, wide), deviations(base, pert)
        for q in dw:
            doc[f"err_{name}_{q}"] = np.float64(max(dw[q], dp[q]))
        # guard 1: the convergence tests are decided with room
        kinds = set()
        for t0, t1, t2 in zip(base["tests"], wide["tests"], pert["tests"]):
            kind, lhs, eps = t0
            d = max(abs(lhs - t1[1]), abs(lhs - t2[1]))
            assert abs(lhs - eps) >= 1000 * d, f"case {name}: {kind} test {lhs} vs {eps} decided within 1000 x {d}"
            if lhs < eps:
                kinds.add(kind)
        if name in ("a", "b", "c"):
            assert kinds == {"kmeans", "harmony"}, f"case {name}: early stops seen: {kinds}"
        if name == "e":
            cap = params["max_iter_kmeans"] - 1      # (a k-means test that passes in the capped iteration changes nothing)
            assert not base["converged"] and (base["kmeans_rounds"] == cap).all(), "case e must stop at its caps"
        # guard 2: the fixture does not amplify rounding noise
        moved = float(np.max(np.abs(base["Z_corr"] - pert["Z_corr"])) / np.max(np.abs(Z)))
        assert moved <= 1e-9, f"case {name}: Z_corr moves {moved} max|Z| under a 1e-15 perturbation"
        doc[f"{name}_objective_kmeans"] = base["objective_kmeans"]
        doc[f"{name}_objective_harmony"] = base["objective_harmony"]
        doc[f"{name}_kmeans_rounds"] = base["kmeans_rounds"]
        doc[f"{name}_converged"] = np.bool_(base["converged"])
        doc[f"{name}_orders_used"] = np.int64(base["orders_used"])
        doc[f"{name}_Z_corr"] = base["Z_corr"][::Z_CORR_STRIDE[name]]
        if name == "a":
            doc["a_terms"] = np.stack([s["terms"] for s in base["steps"]])
            doc["a_E"] = np.stack([s["E"] for s in base["steps"]])
            doc["a_O"] = np.stack([s["O"] for s in base["steps"]])
        if name in ("a", "b", "c"):
            doc.update(hr.stored_slices(name, base))
        print(name, "rounds", base["kmeans_rounds"].tolist(), "converged", base["converged"], "moved", f"{moved:.2e}",
              {q: f"{doc[f'err_{name}_{q}']:.1e}" for q in dw})
    np.savez_compressed(hr.GOLDEN, **doc)
    print("wrote", hr.GOLDEN, os.path.getsize(hr.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
