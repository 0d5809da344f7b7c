"""Generates tests/golden/nmf.npz on the CPU: scikit-learn's multiplicative-update NMF (the oracle of DESIGN 6.24) on the
cases of tests/nmf_reference.py, whose inputs are regenerated from their seeds, and the restatement's own re-ordering spread.

    python tests/golden/gen_nmf_goldens.py

Per case and loss (f = frobenius, kl = kullback-leibler): ``<case>.<loss>.W`` / ``.H`` / ``.err`` after 30 iterations with
``tol = 0`` from the custom start (of the large case every 16th row of W and every 2nd gene of H), ``.spread`` = (W, H) re-ordering spread of the
restatement (``nmf_reference.permuted_spread``).  The stacked case holds one such record per segment.  ``random.W`` /
``random.H``: ``_initialize_nmf(init="random")``.  ``transform.<loss>.*``: ``NMF.transform``.  ``stop.<loss>.*``: one run
with ``tol > 0`` whose deciding quantity stays 1e-6 relative away from ``tol`` at the stopping check and at every check
before it (asserted here, so that rounding cannot move the decision)."""
import os
import sys
import warnings

import numpy as np
from sklearn.decomposition import NMF, non_negative_factorization
from sklearn.decomposition._nmf import _beta_divergence, _initialize_nmf
from sklearn.exceptions import ConvergenceWarning

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nmf_reference as nr  # noqa: E402

TAG = {"frobenius": "f", "kullback-leibler": "kl"}
RANDOM_SEED = 7
MARGIN = 1e-6


def sk_fit(X, W0, H0, loss, max_iter, tol):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        W, H, n_iter = non_negative_factorization(X, W=W0.copy(), H=H0.copy(), n_components=H0.shape[0], init="custom",
                                                  solver="mu", beta_loss=loss, tol=tol, max_iter=max_iter)
    warned = any(issubclass(w.category, ConvergenceWarning) for w in caught)
    return W, H, n_iter, warned


def record(out, key, X, W0, H0, loss, stride=1, hstride=1):
    W, H, n_iter, _ = sk_fit(X, W0, H0, loss, nr.ITERS, 0)
    assert n_iter == nr.ITERS
    out[f"{key}.W"], out[f"{key}.H"] = W[::stride], H[:, ::hstride]
    out[f"{key}.err"] = np.float64(_beta_divergence(X, W, H, loss, square_root=True))
    out[f"{key}.spread"] = np.array(nr.permuted_spread(X, W0, H0, loss, nr.ITERS))


def stop_tolerance(X, W0, H0, loss):
    """A tol at which the run stops at a middle check, the deciding quantity MARGIN away from it at every check taken."""
    hist = nr.fit(X, W0, H0, loss, nr.STOP_MAX_ITER, 1e-300)[4]
    q = (hist[:-1] - hist[1:]) / hist[0]                          # the deciding quantity of check 1, 2, ...
    c = min(5, q.size - 1)
    while c > 1 and not (q[:c] > q[c]).all():
        c -= 1
    tol = float(np.sqrt(q[c] * q[:c].min()))
    assert q[c] < tol * (1 - MARGIN) and (q[:c] > tol * (1 + MARGIN)).all(), (q, tol)
    return tol, 10 * (c + 1)


def main():
    out = {}
    for name, rows, G, k, seed in nr.CASES:
        X, W0, H0 = nr.make_case(rows, G, k, seed)
        for loss in nr.LOSSES:
            record(out, f"{name}.{TAG[loss]}", X, W0, H0, loss, nr.W_STRIDE.get(name, 1), nr.H_STRIDE.get(name, 1))
    name, rows, G, k, seed = nr.STACKED
    X, W0, H0 = nr.make_case(rows, G, k, seed)
    off = nr.STACKED_OFFSETS
    for j in range(len(off) - 1):
        for loss in nr.LOSSES:
            record(out, f"{name}.{j}.{TAG[loss]}", X[off[j]:off[j + 1]], W0[off[j]:off[j + 1]], H0, loss)

    X, W0, H0 = nr.case(nr.CASES[0][0])
    W, H = _initialize_nmf(X, nr.CASES[0][3], init="random", random_state=RANDOM_SEED)
    out["random.W"], out["random.H"], out["random.seed"] = W, H, np.int64(RANDOM_SEED)

    X, W0, H0 = nr.case(nr.TRANSFORM_CASE)
    for loss in nr.LOSSES:
        est = NMF(n_components=H0.shape[0], init="custom", solver="mu", beta_loss=loss, max_iter=nr.TRANSFORM_ITERS, tol=0)
        est.fit(X, W=W0.copy(), H=H0.copy())
        Wt = est.transform(X)
        key = f"transform.{TAG[loss]}"
        out[f"{key}.H"], out[f"{key}.W"] = est.components_, Wt
        rng = np.random.RandomState(1)
        pr, pg = rng.permutation(X.shape[0]), rng.permutation(X.shape[1])
        Wr = nr.transform(X, est.components_, loss, nr.TRANSFORM_ITERS, 0.0)[0]
        Wp = nr.transform(X[pr][:, pg], est.components_[:, pg], loss, nr.TRANSFORM_ITERS, 0.0)[0]
        out[f"{key}.spread"] = np.float64(np.abs(Wp - Wr[pr]).max() / np.abs(Wr).max())

    X, W0, H0 = nr.case(nr.STOP_CASE)
    for loss in nr.LOSSES:
        tol, want = stop_tolerance(X, W0, H0, loss)
        W, H, n_iter, warned = sk_fit(X, W0, H0, loss, nr.STOP_MAX_ITER, tol)
        assert n_iter == want and not warned, (n_iter, want, warned)
        key = f"stop.{TAG[loss]}"
        out[f"{key}.tol"], out[f"{key}.n_iter"], out[f"{key}.converged"] = np.float64(tol), np.int64(n_iter), np.int64(not warned)
        out[f"{key}.err"] = np.float64(_beta_divergence(X, W, H, loss, square_root=True))
    path = os.path.join(HERE, "nmf.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    for key in sorted(out):
        if key.endswith(".spread"):
            print(key, np.asarray(out[key]) / nr.EPS)


if __name__ == "__main__":
    main()
