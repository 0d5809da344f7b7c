"""fp64 numpy restatement of the reference's cluster() arithmetic (tests only), for the tests of mclstexp_amd.cluster:
PCA through the eigen-decomposition of the smaller centred Gram matrix (sklearn's ``PCA(svd_solver="arpack")`` scores,
sign rule of sklearn >= 1.5), Lloyd's k-means with sklearn's stopping rule, ARI / NMI from the contingency table.  Pinned
against sklearn's own outputs (tests/golden/cluster.npz) by tests/test_cluster_host.py; used by the GPU tests for the cases
that have no fixture (fp32 input, odd shapes, views)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster.npz")
# name -> synth.make_cluster_case arguments (as tests/golden/gen_cluster_goldens.py generates them)
CLUSTER_CASES = {
    "c346": dict(n=346, genes=785, k=6, seed=1, sep=0.12, undetermined_frac=0.1),
    "c613": dict(n=613, genes=171, k=4, seed=2, sep=0.15, undetermined_frac=0.1),
    "c3200": dict(n=3200, genes=685, k=7, seed=3, sep=0.08, undetermined_frac=0.1),
    "c250": dict(n=250, genes=3467, k=5, seed=4, sep=0.06, undetermined_frac=0.1),
    "c1500": dict(n=1500, genes=300, k=10, seed=7, sep=0.10, undetermined_frac=0.1),
    "sep": dict(n=300, genes=200, k=4, seed=5, sep=1.0, undetermined_frac=0.1),
    # three slides of one evaluation (same genes; the last one is in the dual form): the segmented end-to-end case
    "s300": dict(n=300, genes=171, k=4, seed=11, sep=0.2, undetermined_frac=0.1),
    "s420": dict(n=420, genes=171, k=5, seed=12, sep=0.2, undetermined_frac=0.1),
    "s150": dict(n=150, genes=171, k=3, seed=13, sep=0.2, undetermined_frac=0.1),
}
NOISY = ("c346", "c613", "c3200", "c250", "c1500")
SEGMENTED = ("c613", "c250", "c346")      # the segmented k-means case stacks the scores of these three
SLIDES = ("s300", "s420", "s150")         # slides of one evaluation: same genes
N_COMPS = 9


def kept(d):
    """(pred rows, label strings, integer truth) of the spots cluster() keeps."""
    idx = d["label"] != "undetermined"
    return d["pred"][idx], d["label"][idx], d["truth"][idx]


def pca_scores(x, n_comps=N_COMPS):
    """(scores (n, n_comps), explained variance (n_comps,), leading eigenvalues)."""
    x = np.asarray(x, dtype=np.float64)
    n, g = x.shape
    xc = x - x.mean(axis=0)
    if n >= g:
        w, v = np.linalg.eigh(xc.T @ xc)
        w, v = w[::-1][:n_comps], v[:, ::-1][:, :n_comps]
        z, load = xc @ v, v
    else:
        w, u = np.linalg.eigh(xc @ xc.T)
        w, u = w[::-1][:n_comps], u[:, ::-1][:, :n_comps]
        z, load = u * np.sqrt(w), xc.T @ u
    top = np.abs(load).argmax(axis=0)
    sign = np.where(load[top, np.arange(n_comps)] < 0, -1.0, 1.0)
    return z * sign, w / (n - 1), w


def sign_rule_holds(x, z):
    """Every component's loading of largest magnitude is positive (loadings ~ Xc^T z)."""
    x = np.asarray(x, dtype=np.float64)
    load = (x - x.mean(axis=0)).T @ z
    return bool((load[np.abs(load).argmax(axis=0), np.arange(z.shape[1])] > 0).all())


def align_signs(z, ref):
    return z * np.where((z * ref).sum(axis=0) < 0, -1.0, 1.0)


def _sqdist(z, c):
    return ((z[:, None, :] - c[None, :, :]) ** 2).sum(axis=-1)


def lloyd(z, centers, tol=1e-4, max_iter=300):
    """sklearn's ``KMeans(algorithm="lloyd")`` from given initial centres: dict of labels, centers, inertia, n_iter,
    min_margin (the smallest relative gap between a point's nearest and second-nearest squared distance over all
    assignments) and ever_empty.  Ties go to the lowest centre; an emptied cluster takes the point farthest from its own
    centre (ties: lowest row)."""
    z = np.asarray(z, dtype=np.float64)
    c = np.array(centers, dtype=np.float64)
    k = c.shape[0]
    tol_abs = tol * z.var(axis=0).mean()
    old = np.full(z.shape[0], -1)
    margin, ever_empty, strict = np.inf, False, False
    for it in range(max_iter):
        d = _sqdist(z, c)
        lab = d.argmin(axis=1)
        if k > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            margin = min(margin, float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min()))
        eff = lab.copy()
        own = d[np.arange(z.shape[0]), lab].copy()
        cnt = np.bincount(eff, minlength=k)
        for j in range(k):
            if cnt[j] == 0:
                ever_empty = True
                f = int(np.argmax(own))
                cnt[eff[f]] -= 1
                eff[f] = j
                cnt[j] = 1
                own[f] = -1.0
        new = np.stack([z[eff == j].sum(axis=0) * (1.0 / cnt[j]) if cnt[j] else c[j] for j in range(k)])
        shift = ((new - c) ** 2).sum()
        c = new
        if np.array_equal(lab, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = lab
    if not strict:
        lab = _sqdist(z, c).argmin(axis=1)
    inertia = float(((z - c[lab]) ** 2).sum())
    return {"labels": lab.astype(np.int32), "centers": c, "inertia": inertia, "n_iter": it + 1, "min_margin": margin,
            "ever_empty": ever_empty}


def contingency(a, b):
    _, ia = np.unique(np.asarray(a), return_inverse=True)
    _, ib = np.unique(np.asarray(b), return_inverse=True)
    t = np.zeros((ia.max() + 1, ib.max() + 1), dtype=np.int64)
    np.add.at(t, (ia.reshape(-1), ib.reshape(-1)), 1)
    return t


def ari_nmi(a, b):
    """sklearn's adjusted_rand_score (pair-confusion form) and normalized_mutual_info_score (arithmetic, natural log)."""
    t = contingency(a, b)
    n = int(t.sum())
    ra, cb = t.sum(axis=1), t.sum(axis=0)
    ssq = int((t.astype(object) ** 2).sum())
    tp = ssq - n
    fp = int((cb.astype(object) ** 2).sum()) - ssq
    fn = int((ra.astype(object) ** 2).sum()) - ssq
    tn = n * n - fp - fn - ssq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    if t.shape == (1, 1):
        return ari, 1.0
    if 1 in t.shape:
        return ari, 0.0
    i, j = np.nonzero(t)
    v = t[i, j].astype(np.float64)
    mi = (v / n) * (np.log(v) - np.log(n)) + (v / n) * (-np.log((ra[i] * cb[j]).astype(np.float64)) + 2 * np.log(n))
    mi = max(float(np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi).sum()), 0.0)
    if mi == 0.0:
        return ari, 0.0
    h = [-float(((p / n) * (np.log(p) - np.log(n))).sum()) for p in (ra.astype(np.float64), cb.astype(np.float64))]
    return ari, mi / (0.5 * (h[0] + h[1]))


def label_pairs():
    """Hand-made label pairs for cluster_scores (the fixture stores sklearn's ARI / NMI for them, in this order)."""
    r = np.random.default_rng(11)
    a = r.integers(0, 5, 400)
    perm = np.array([3, 0, 4, 1, 2])
    return [
        ("identical", a, a.copy()),
        ("permuted", a, perm[a]),
        ("one_vs_many", np.zeros(60, dtype=np.int64), np.arange(60) % 7),
        ("many_vs_one", np.arange(60) % 7, np.zeros(60, dtype=np.int64)),
        ("single_both", np.full(30, 2), np.full(30, 5)),
        ("n2_same", np.array([0, 0]), np.array([1, 1])),
        ("n2_split", np.array([0, 1]), np.array([0, 0])),
        ("n2_both_split", np.array([0, 1]), np.array([1, 0])),
        ("independent", r.integers(0, 6, 1000), r.integers(0, 9, 1000)),
        ("all_distinct", np.arange(100), np.arange(100)[::-1].copy()),
        ("sparse_values", r.integers(0, 4, 300) * 250 + 3, r.integers(0, 3, 300) * 500 + 23),
    ]
