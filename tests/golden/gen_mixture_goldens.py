"""Writes tests/golden/mixture.npz: sklearn's own results on the fixtures of tests/mixture_reference.py (needs scikit-learn;
recorded with 1.7.2).  The inputs are not stored: ``mixture_reference.make_case`` regenerates them, and a checksum of each
is recorded so that a drifting generator is noticed.

    python tests/golden/gen_mixture_goldens.py

GaussianMixture's k-means step is replaced by given labels: ``_initialize_parameters`` calls sklearn's ``_initialize`` on
one-hot responsibilities; everything else is sklearn's code."""
import os
import sys
import warnings

import numpy as np
from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mixture_reference as mr  # noqa: E402


class LabelInitGMM(GaussianMixture):
    def __init__(self, labels=None, **kw):
        super().__init__(**kw)
        self.labels = labels

    def _initialize_parameters(self, X, random_state):
        resp = (np.asarray(self.labels)[:, None] == np.arange(self.n_components)[None, :]).astype(np.float64)
        self._initialize(X, resp)


def validity_labelings(case):
    """{name: labels} scored for a fixture: its noisy initial labels; and with a singleton cluster and dropped rows."""
    n, D, K, sep = case
    x, init, truth = mr.make_case(*case)
    out = {"init": init.copy()}
    if n >= 40:
        lab = init.copy()
        lab[5] = 900                     # a cluster of one row
        lab[10:20] = -1                  # dropped rows
        out["edge"] = lab
    return x, out


def main():
    out = {}
    for case in mr.CASES:
        n, D, K, sep = case
        name = mr.case_name(case)
        x, init, truth = mr.make_case(*case)
        out[f"{name}/checksum"] = np.array([x.sum(), np.abs(x).sum(), x[0, 0], x[-1, -1], float(init.sum())])
        for ctype in mr.TYPES:
            g = LabelInitGMM(labels=init, n_components=K, covariance_type=ctype, tol=1e-3, max_iter=100, reg_covar=1e-6)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                labels = g.fit_predict(x)
            key = f"{name}/{ctype}/"
            out[key + "lower_bounds"] = np.asarray(g.lower_bounds_)
            out[key + "n_iter"] = np.int32(g.n_iter_)
            out[key + "converged"] = np.int32(g.converged_)
            out[key + "weights"] = g.weights_
            out[key + "means"] = g.means_
            out[key + "covariances"] = g.covariances_
            out[key + "precisions_cholesky"] = g.precisions_cholesky_
            out[key + "labels"] = labels.astype(np.int8)
            out[key + "score"] = np.float64(g.score(x))
            out[key + "bic"] = np.float64(g.bic(x))
            out[key + "aic"] = np.float64(g.aic(x))
            lse = g.score_samples(x)
            resp = g.predict_proba(x)
            out[key + "score_samples_head"] = lse[:32]
            out[key + "resp_head"] = resp[:32]
        xs, labs = validity_labelings(case)
        for lname, lab in labs.items():
            keep = lab >= 0
            key = f"{name}/validity_{lname}/"
            out[key + "labels"] = lab.astype(np.int16)
            sil = np.full(n, np.nan)
            sil[keep] = silhouette_samples(xs[keep], lab[keep])
            out[key + "silhouette_samples"] = sil
            out[key + "calinski_harabasz"] = np.float64(calinski_harabasz_score(xs[keep], lab[keep]))
            out[key + "davies_bouldin"] = np.float64(davies_bouldin_score(xs[keep], lab[keep]))
    path = os.path.join(HERE, "mixture.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
