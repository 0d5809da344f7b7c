"""Writes tests/golden/umap.npz: the inputs of the cases of tests/umap_reference.py and how far the restatement itself can
be trusted.  The tests recompute every expectation with the restatement.

    python tests/golden/gen_umap_goldens.py

a, b: find_ab_params(1.0, 0.5) as scipy fitted them here.  <case>_X, <case>_Y0: the input and the start.  err_<case>_Y<k>
for k = 1, 10 and <case>_trajectory_len: the larger of the float64 restatement's deviation from its np.longdouble run and
from a float64 run with Y0, a and b perturbed by 1e-15 relative, relative to max |Y| and floored at 2^-53.  The schedule is
not perturbed and always float64: it is exact by definition, and a weight perturbed by 1e-15 flips next <= n where eps = 1.
The trajectory length is the longest multiple of 10 up to 60 (and up to the case's n_epochs) whose uncertainty stays <= 1e-6;
where not even 10 epochs stay below it (case d: the layout's own sensitivity, a repulsion of slope 2 b / 0.001 between
near-coincident points, multiplies a rounding error every epoch), the largest number of epochs below 10 that does.
Case e: sklearn's trustworthiness(X, Y, n_neighbors=15) (sklearn 1.7.2) and the nearest-neighbour label purity of
the full default-length run for four seeds, for the Jacobi restatement and for the sequential-order one.  Refuses to write
unless every Jacobi run is finite, has purity 1.0 and reaches a trustworthiness of at least the sequential form's minimum
minus the sequential form's own max - min."""
import os
import sys

import numpy as np
from sklearn.manifold import trustworthiness

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import umap_reference as ur  # noqa: E402

LD = np.longdouble
FLOOR = 2.0 ** -53


def perturb(a, seed):
    rng = np.random.RandomState(seed)
    return np.asarray(a, dtype=np.float64) * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=np.shape(a)))


def err(base, *others):
    scale = np.max(np.abs(base))
    return max(FLOOR, *(float(np.max(np.abs(np.asarray(o, dtype=LD) - base)) / scale) for o in others))


def main():
    a, b = ur.find_ab_params(1.0, 0.5)
    assert abs(a - 0.5830300) < 1e-6 and abs(b - 1.3341670) < 1e-6, (a, b)
    out = {"a": a, "b": b}
    for name in ur.TRAJECTORY:
        X, sizes, _ = ur.case_input(name)
        off = np.concatenate([[0], np.cumsum(sizes)])
        Y0, graphs, n_epochs = ur.case_start(name), ur.case_graphs(name), ur.CASES[name][3]
        out[f"{name}_X"], out[f"{name}_Y0"] = X, Y0
        top = min(ur.MAX_TRAJECTORY, n_epochs)
        keep = tuple(range(1, 10)) + tuple(range(10, top + 1, 10))
        dev = {k: FLOOR for k in keep}
        a_pt, b_pt = float(perturb(a, 41)), float(perturb(b, 42))
        for s, g in enumerate(graphs):
            y0 = Y0[off[s]:off[s + 1]]
            base = ur.run(g, y0, n_epochs, a, b, ur.SEED, stop_after=top, keep=keep)
            ld = ur.run(g, y0.astype(LD), n_epochs, LD(a), LD(b), ur.SEED, stop_after=top, keep=keep, dtype=LD)
            pt = ur.run(g, perturb(y0, 43 + s), n_epochs, a_pt, b_pt, ur.SEED, stop_after=top, keep=keep)
            assert np.isfinite(base["Y"]).all(), (name, s)
            assert base["attractive_samples"] == ld["attractive_samples"] == pt["attractive_samples"], (name, s)
            assert base["negative_samples"] == ld["negative_samples"] == pt["negative_samples"], (name, s)
            for k in keep:
                dev[k] = max(dev[k], err(base["trace"][k], ld["trace"][k], pt["trace"][k]))
        length = top
        while length > 1 and dev[length] > 1e-6:
            length -= 10 if length > 10 else 1
        assert dev[length] <= 1e-6, (name, dev)
        out[f"{name}_trajectory_len"] = length
        for k in (1, 10, length):
            out[f"err_{name}_Y{k}"] = dev[k]
        print(name, "trajectory length", length, {k: f"{v:.2e}" for k, v in dev.items()})

    # ---- case e: full runs, four seeds, both forms
    X, sizes, _ = ur.case_input("e")
    g, lab = ur.case_graphs("e")[0], ur.case_labels("e")
    n_epochs = ur.default_epochs(sizes[0])
    jac, seq, pur = [], [], []
    for seed in ur.FULL_SEEDS:
        y0 = ur.random_init(sizes[0], seed)
        yj = ur.run(g, y0, n_epochs, a, b, seed)["Y"]
        ys = ur.run_sequential(g, y0, n_epochs, a, b, seed)
        assert np.isfinite(yj).all() and np.isfinite(ys).all(), seed
        tj, ts = trustworthiness(X, yj, n_neighbors=ur.TRUST_K), trustworthiness(X, ys, n_neighbors=ur.TRUST_K)
        assert abs(ur.trustworthiness(X, yj) - tj) < 1e-12 and abs(ur.trustworthiness(X, ys) - ts) < 1e-12
        jac.append(tj)
        seq.append(ts)
        pur.append((ur.nn_purity(yj, lab), ur.nn_purity(ys, lab)))
        print("e seed", seed, "trustworthiness jacobi", tj, "sequential", ts, "purity", pur[-1], "extent", np.abs(yj).max())
    jac, seq, pur = np.array(jac), np.array(seq), np.array(pur)
    assert (pur[:, 0] == 1.0).all(), pur
    assert jac.min() >= seq.min() - (seq.max() - seq.min()), (jac, seq)
    out["e_X"] = X
    out["e_trust_jacobi"], out["e_trust_sequential"], out["e_purity"] = jac, seq, pur
    np.savez_compressed(ur.GOLDEN, **out)
    print("wrote", ur.GOLDEN, os.path.getsize(ur.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
