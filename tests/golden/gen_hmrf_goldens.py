"""Writes tests/golden/hmrf.npz: the recorded outputs of tests/hmrf_reference.py on the fixtures of the Potts-HMRF mixtures,
and the results of independent dense formulas for the same quantities (needs scipy; recorded with 1.15.3).  The inputs are
not stored: ``hmrf_reference.make_case`` regenerates them, and a checksum of each is recorded so that a drifting generator
is noticed.

    python tests/golden/gen_hmrf_goldens.py

Independent of the restatement's orders: the field as a dense matrix product W @ Q, the densities by
``scipy.stats.multivariate_normal.logpdf`` from the covariances (not from their Cholesky factors), every log-sum-exp by
``scipy.special.logsumexp``, the refine rule by ``numpy.bincount`` per row, the agreement sums as sums over a dense matrix."""
import os
import sys

import numpy as np
from scipy.special import logsumexp
from scipy.stats import multivariate_normal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hmrf_reference as hr  # noqa: E402
import mixture_reference as mr  # noqa: E402


def dense_weights(nbr, w):
    n = nbr.shape[0]
    W = np.zeros((n, n))
    np.add.at(W, (np.repeat(np.arange(n), nbr.shape[1]), nbr.ravel()), w.ravel())
    return W


def covariance(cov, ctype, k, D):
    if ctype in ("full", "tied"):
        return cov[k] if ctype == "full" else cov
    return np.diag(cov[k]) if ctype == "diag" else np.eye(D) * cov[k]


def dense_estep(x, w, mu, cov, ctype, nbr, gw, q, beta):
    n, D = x.shape
    f = dense_weights(nbr, gw) @ q
    g = np.stack([multivariate_normal.logpdf(x, mu[k], covariance(cov, ctype, k, D), allow_singular=False)
                  for k in range(w.size)], axis=1).reshape(n, w.size) + np.log(w)
    v = g + beta * f
    lse = logsumexp(v, axis=1)
    za = logsumexp(np.log(w) + beta * f, axis=1)
    return {"field": f, "wlp": g, "lse": lse, "za": za, "log_resp": v - lse[:, None], "score": float(np.mean(lse - za))}


def bincount_refine(labels, nbr, w):
    out = labels.copy()
    for i in range(labels.size):
        if labels[i] < 0:
            continue
        near = labels[nbr[i][w[i] != 0.0]]
        near = near[near >= 0]
        cnt = np.bincount(np.append(near, labels[i]))
        top = int(np.argmax(cnt))                              # the first largest: ties to the smallest label
        if 2 * cnt[labels[i]] < near.size and 2 * cnt[top] > near.size:
            out[i] = top
    return out


def dense_agreement(labels, nbr, w):
    W = dense_weights(nbr, w)
    both = (labels[:, None] >= 0) & (labels[None, :] >= 0)
    return float((W * (both & (labels[:, None] == labels[None, :]))).sum()), float((W * both).sum())


def main():
    out = {}
    for name in hr.FIT_CASES:
        c = hr.make_case(name)
        out[f"{name}/checksum"] = hr.checksum(c)
        for ctype in c["types"]:
            f = hr.ref_fit(name, ctype)
            key = f"{name}/{ctype}/"
            for field in ("lower_bounds", "weights", "means", "score", "bic"):
                out[key + field] = np.asarray(f[field])
            out[key + "n_iter"], out[key + "converged"] = np.int32(f["n_iter"]), np.int32(f["converged"])
            out[key + "labels"] = f["labels"].astype(np.int8)
            out[key + "field_head"] = f["field"][:16]
    c = hr.make_case("B")
    f1, f0 = hr.ref_fit("B", "full"), hr.ref_fit("B", "full", beta=0.0)
    e1, e0 = hr.edge_sums(f1["labels"], c["nbr"], c["w"]), hr.edge_sums(f0["labels"], c["nbr"], c["w"])
    out["B/recovery"] = np.array([hr.ari(f1["labels"], c["truth"]), hr.ari(f0["labels"], c["truth"]), e1[0] / e1[1],
                                  e0[0] / e0[1], float(f1["n_iter"]), float(f0["n_iter"])])
    for name in ("A", "C", "G"):
        t = hr.teacher_case(name)
        for ctype in t["types"]:
            w, mu, _, cov = t["params"][ctype]
            d = dense_estep(t["x"], w, mu, cov, ctype, t["nbr"], t["w"], t["q"], t["beta"])
            for field, v in d.items():
                out[f"{name}/{ctype}/dense_{field}"] = np.asarray(v)
    for name in ("A", "C"):
        c = hr.make_case(name)
        lab = hr.label_case(name)
        out[f"{name}/refine_in"] = lab.astype(np.int16)
        out[f"{name}/refine_bincount"] = bincount_refine(lab, c["nbr"], c["w"]).astype(np.int16)
        out[f"{name}/agreement_dense"] = np.array(dense_agreement(lab, c["nbr"], c["w"]))
    path = os.path.join(HERE, "hmrf.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
