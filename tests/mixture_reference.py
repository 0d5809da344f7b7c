"""NumPy restatement of the Gaussian-mixture and cluster-validity arithmetic DESIGN 6.17 states (csrc/mixture.hip), in the
kernels' summation orders: the yardstick of tests/test_mixture_host.py (against sklearn's own results, recorded in
tests/golden/mixture.npz) and of tests/test_mixture_gpu.py (against the device).

Orders restated (everything fp64, products and sums rounded separately):
  sums over rows (n_k, means, x^2 moments, scatter matrices, X^T X)   row ascending, one running sum
  y = (x - mu_k) P_k                                                  d ascending per column j
  ||y||^2                                                             four partial sums, j = 16 jt + 4 q + lane over (jt, q)
                                                                      ascending, combined (s0 + s1) + (s2 + s3)
  log-sum-exp, weights sum, tied sum_k n_k mu mu^T                    k ascending, the maximum subtracted
  lower bound / score, mean silhouette, intra dispersion              per-thread sums over rows t, t + 256, ... then a
                                                                      binary tree over the 256 threads
  Cholesky                                                            right-looking; the inverse by forward substitution
  silhouette distance sums, centroids                                 over a cluster's rows ascending
The device's MFMA accumulates the same terms in the same order; whether it rounds each product is not stated by the ISA
guide, which is why the device test bounds these sums instead of asking for equality."""
import numpy as np

EPS = 2.0 ** -52
LOG_2PI = 1.8378770664093453
TYPES = ("full", "tied", "diag", "spherical")
T = 256

# (n, D, K, sep): the fixtures of the issue
CASES = [(257, 9, 4, 3.0), (143, 9, 6, 2.0), (64, 1, 2, 3.0), (1000, 50, 8, 1.5), (4097, 9, 7, 2.0), (40, 3, 3, 4.0)]


def case_name(case):
    return "n%d_d%d_k%d" % case[:3]


def make_case(n, D, K, sep, seed=0):
    """K centres randn(K, D) * sep, per-cluster mixing matrix I + 0.3 randn(D, D); initial labels = the truth with 15 % of
    the rows reassigned at random and rows 0 .. K - 1 forced to labels 0 .. K - 1."""
    r = np.random.default_rng([seed, n, D, K])
    centres = r.standard_normal((K, D)) * sep
    mix = np.eye(D)[None] + 0.3 * r.standard_normal((K, D, D))
    truth = r.integers(0, K, n)
    x = centres[truth] + np.einsum("nd,nde->ne", r.standard_normal((n, D)), mix[truth])
    init = truth.copy()
    flip = r.random(n) < 0.15
    init[flip] = r.integers(0, K, int(flip.sum()))
    init[:K] = np.arange(K)
    return np.ascontiguousarray(x), init.astype(np.int32), truth.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- helpers
def seq_sum(a, axis=0):
    """One running sum along ``axis`` (np.add.accumulate is sequential)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def block_sum(v):
    """Thread t sums v[t], v[t + 256], ... in turn; then red[t] += red[t + h] for h = 128, 64, ..., 1."""
    v = np.asarray(v, dtype=np.float64)
    m = -(-v.size // T)
    a = np.zeros(m * T)
    a[:v.size] = v
    part = np.zeros(T)
    for row in a.reshape(m, T):
        part = part + row
    h = T // 2
    while h:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return float(part[0])


def cov_shape(ctype, K, D):
    return {"full": (K, D, D), "tied": (D, D), "diag": (K, D), "spherical": (K,)}[ctype]


def n_parameters(ctype, K, D):
    cov = {"full": K * D * (D + 1) / 2.0, "tied": D * (D + 1) / 2.0, "diag": K * D, "spherical": K}[ctype]
    return int(cov + D * K + K - 1)


# ----------------------------------------------------------------------------------------------------------- E-step
def quad_form(x, mu, P):
    """||(x - mu) P||^2 per row, P (D, D) upper triangular, in the kernel's order."""
    n, D = x.shape
    diff = x - mu
    njt = -(-D // 16)
    y = np.zeros((n, njt * 16))
    for d in range(D):
        y[:, d:D] = y[:, d:D] + diff[:, d:d + 1] * P[d, d:D]
    sq = (y * y).reshape(n, njt, 4, 4)            # [jt][q][lane]: j = 16 jt + 4 q + lane
    part = seq_sum(sq.reshape(n, njt * 4, 4), axis=1)
    return (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])


def log_det(pc, ctype, K, D):
    if ctype == "full":
        return np.array([seq_sum(np.log(np.diag(pc[k]))) for k in range(K)])
    if ctype == "tied":
        return np.full(K, seq_sum(np.log(np.diag(pc))))
    if ctype == "diag":
        return seq_sum(np.log(pc), axis=1)
    return D * np.log(pc)


def estep(x, w, mu, pc, ctype):
    """-> dict: wlp (weighted log prob), lse (log_prob_norm), log_resp, resp, labels, score (the mean of lse)."""
    n, D = x.shape
    K = w.size
    ld, lw = log_det(pc, ctype, K, D), np.log(w)
    c0 = D * LOG_2PI
    wlp = np.empty((n, K))
    for k in range(K):
        if ctype in ("full", "tied"):
            ss = quad_form(x, mu[k], pc[k] if ctype == "full" else pc)
        else:
            t = (x - mu[k]) * (pc[k] if ctype == "diag" else pc[k])
            ss = seq_sum(t * t, axis=1)
        wlp[:, k] = ((-0.5 * (c0 + ss)) + ld[k]) + lw[k]
    mx = wlp.max(axis=1)
    s = seq_sum(np.exp(wlp - mx[:, None]), axis=1)
    lse = mx + np.log(s)
    log_resp = wlp - lse[:, None]
    return {"wlp": wlp, "lse": lse, "log_resp": log_resp, "resp": np.exp(log_resp),
            "labels": np.argmax(log_resp, axis=1).astype(np.int32), "score": block_sum(lse) / n}


# ----------------------------------------------------------------------------------------------------------- M-step
def precision_cholesky(C):
    """(P upper triangular with P^T P = C^-1, failed): right-looking Cholesky, forward substitution per column."""
    D = C.shape[0]
    a = np.array(C, dtype=np.float64)
    for j in range(D):
        piv = a[j, j]
        if not piv > 0.0:
            return None, True
        ljj = np.sqrt(piv)
        a[j, j] = ljj
        a[j + 1:, j] = a[j + 1:, j] / ljj
        col = a[j + 1:, j]
        a[j + 1:, j + 1:] = a[j + 1:, j + 1:] - col[:, None] * col[None, :]
    L = np.tril(a)
    P = np.zeros((D, D))
    for c in range(D):
        P[c, c] = 1.0 / L[c, c]
    for i in range(1, D):
        s = seq_sum(L[i, :i][None, :] * P[:, :i], axis=1)       # P[c, t] = 0 for t < c: the sum starts at t = c
        P[:i, i] = (0.0 - s[:i]) / L[i, i]
    return P, False


def mstep(x, resp, reg, ctype, init=False):
    """sklearn's _estimate_gaussian_parameters + _compute_precision_cholesky -> (w, mu, cov, pc, failed)."""
    n, D = x.shape
    K = resp.shape[1]
    nk = seq_sum(resp, axis=0) + 10.0 * EPS
    mu = seq_sum(resp[:, :, None] * x[:, None, :], axis=0) / nk[:, None]
    nk_sum = seq_sum(nk)
    w = nk / (float(n) if init else nk_sum)
    if ctype == "full":
        cov, pc = np.empty((K, D, D)), np.empty((K, D, D))
        for k in range(K):
            diff = x - mu[k]
            acc = seq_sum((resp[:, k:k + 1] * diff)[:, :, None] * diff[:, None, :], axis=0) / nk[k]
            c = np.tril(acc) + np.tril(acc, -1).T
            c[np.diag_indices(D)] += reg
            cov[k] = c
        for k in range(K):
            pc[k], failed = precision_cholesky(cov[k])
            if failed:
                return w, mu, cov, None, True
        return w, mu, cov, pc, False
    if ctype == "tied":
        xtx = seq_sum(x[:, :, None] * x[:, None, :], axis=0)
        s = seq_sum((nk[:, None] * mu)[:, :, None] * mu[:, None, :], axis=0)
        acc = (xtx - s) / nk_sum
        cov = np.tril(acc) + np.tril(acc, -1).T
        cov[np.diag_indices(D)] += reg
        pc, failed = precision_cholesky(cov)
        return w, mu, cov, pc, failed
    x2 = seq_sum(resp[:, :, None] * (x * x)[:, None, :], axis=0)
    diag = ((x2 / nk[:, None]) - mu * mu) + reg
    cov = diag if ctype == "diag" else seq_sum(diag, axis=1) / float(D)
    failed = not bool((cov > 0.0).all())
    with np.errstate(all="ignore"):
        pc = 1.0 / np.sqrt(cov)
    return w, mu, cov, pc, failed


# -------------------------------------------------------------------------------------------------------------- fit
def fit(x, K, init_labels, ctype="full", tol=1e-3, max_iter=100, reg=1e-6):
    """sklearn's fit_predict from one-hot responsibilities.  -> dict (status 1: ill-defined covariance)."""
    n, D = x.shape
    resp = (np.asarray(init_labels)[:, None] == np.arange(K)[None, :]).astype(np.float64)
    w, mu, cov, pc, failed = mstep(x, resp, reg, ctype, init=True)
    lb, it, conv, bounds = -np.inf, 0, 0, []
    while not failed and it < max_iter:
        prev = lb
        e = estep(x, w, mu, pc, ctype)
        lb = e["score"]
        bounds.append(lb)
        w, mu, cov, pc, failed = mstep(x, e["resp"], reg, ctype)
        it += 1
        if failed:
            break
        if abs(lb - prev) < tol:
            conv = 1
            break
    if failed:
        return {"status": 1, "n_iter": it, "lower_bound": np.nan, "converged": 0}
    e = estep(x, w, mu, pc, ctype)
    p = n_parameters(ctype, K, D)
    return {"status": 0, "n_iter": it, "converged": conv, "lower_bound": lb, "lower_bounds": np.array(bounds),
            "score": e["score"], "weights": w, "means": mu, "covariances": cov, "precisions_cholesky": pc,
            "labels": e["labels"], "resp": e["resp"], "log_resp": e["log_resp"], "lse": e["lse"],
            "bic": ((-2.0 * e["score"]) * n) + p * np.log(float(n)), "aic": ((-2.0 * e["score"]) * n) + 2.0 * p}


def top_two_gap(log_resp):
    """Per row the gap between the two largest log responsibilities (inf for one component)."""
    if log_resp.shape[1] < 2:
        return np.full(log_resp.shape[0], np.inf)
    s = np.sort(log_resp, axis=1)
    return s[:, -1] - s[:, -2]


# --------------------------------------------------------------------------------------------------------- validity
def validity(x, labels):
    """-> dict: silhouette_samples (NaN for rows labelled -1), silhouette, calinski_harabasz, davies_bouldin (NaN all
    when there are fewer than 2 or more than kept - 1 non-empty clusters)."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    n, D = x.shape
    kept = np.flatnonzero(labels >= 0)
    values = np.unique(labels[kept])
    ncl, nkept = values.size, kept.size
    nan = {"silhouette_samples": np.full(n, np.nan), "silhouette": np.nan, "calinski_harabasz": np.nan,
           "davies_bouldin": np.nan}
    if ncl < 2 or ncl > nkept - 1 or labels.min() < -1 or labels.max() >= 1024:
        return nan
    members = [np.flatnonzero(labels == v) for v in values]            # rows ascending
    dense = np.full(n, -1)
    for c, m in enumerate(members):
        dense[m] = c

    def dist_to(j):
        sq = np.zeros(n)
        for d in range(D):
            df = x[:, d] - x[j, d]
            sq = sq + df * df
        return np.sqrt(sq)
    a, b = np.zeros(n), np.full(n, np.inf)
    for c, m in enumerate(members):
        acc = np.zeros(n)
        for j in m:
            acc = acc + dist_to(j)
        own = dense == c
        a[own] = acc[own] / (m.size - 1) if m.size > 1 else 0.0
        with np.errstate(all="ignore"):
            b[~own] = np.minimum(b[~own], acc[~own] / m.size)
    with np.errstate(all="ignore"):
        sil = (b - a) / np.maximum(a, b)
    sil[np.isnan(sil)] = 0.0
    sizes = np.array([m.size for m in members])
    sil[sizes[np.maximum(dense, 0)] == 1] = 0.0
    sil[dense < 0] = np.nan
    order = np.concatenate(members)
    cen = np.array([seq_sum(x[m], axis=0) / m.size for m in members])
    mean = np.array([block_sum(x[order, d]) / nkept for d in range(D)])
    sq = np.zeros(nkept)
    for d in range(D):
        df = x[order, d] - cen[dense[order], d]
        sq = sq + df * df
    dcen = np.sqrt(sq)
    intra = block_sum(sq)
    sqc = np.zeros(ncl)
    for d in range(D):
        df = cen[:, d] - mean[d]
        sqc = sqc + df * df
    extra = block_sum(sizes * sqc)
    ch = 1.0 if intra == 0.0 else (extra * float(nkept - ncl)) / (intra * (float(ncl) - 1.0))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    sc = np.array([seq_sum(dcen[starts[c]:starts[c + 1]]) / sizes[c] for c in range(ncl)])
    sqcc = np.zeros((ncl, ncl))
    for d in range(D):
        df = cen[:, None, d] - cen[None, :, d]
        sqcc = sqcc + df * df
    dcc = np.sqrt(sqcc)
    with np.errstate(all="ignore"):
        ratio = np.where(dcc != 0.0, (sc[:, None] + sc[None, :]) / dcc, 0.0)
    best = np.zeros(ncl)
    for j in range(ncl):
        best = np.maximum(best, ratio[:, j])
    db = 0.0 if (not (sc > 1e-8).any() or not (dcc > 1e-8).any()) else block_sum(best) / ncl
    return {"silhouette_samples": sil, "silhouette": block_sum(np.where(dense >= 0, sil, 0.0)) / nkept,
            "calinski_harabasz": ch, "davies_bouldin": db}
