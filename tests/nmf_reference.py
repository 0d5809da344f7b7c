"""numpy restatement (fp64) of the multiplicative-update NMF of DESIGN 6.24, i.e. of scikit-learn's
``non_negative_factorization(solver="mu")`` for the Frobenius and the Kullback-Leibler loss without regularisation, and
the cases the NMF tests share.  tests/golden/gen_nmf_goldens.py pins it to scikit-learn and records the re-ordering
spread of every case; the GPU tests hold the device to this restatement."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPSILON = float(np.finfo(np.float32).eps)          # sklearn.decomposition._nmf.EPSILON
LOSSES = ("frobenius", "kullback-leibler")
ITERS = 30                                         # iterations of the recorded tol = 0 runs

# (name, rows, G, k, seed)
CASES = (("a70x37k5", 70, 37, 5, 11), ("b300x171k12", 300, 171, 12, 12), ("c533x171k64", 533, 171, 64, 13),
         ("d70x37k1", 70, 37, 1, 14))
STACKED = ("s370x37k5", 370, 37, 5, 15)
STACKED_OFFSETS = (0, 7, 70, 370)
W_STRIDE = {"c533x171k64": 16}                     # the golden keeps every 16th row of the large case's W
H_STRIDE = {"c533x171k64": 2}                      # and every 2nd gene of its H
STOP_CASE, STOP_MAX_ITER = "b300x171k12", 200
TRANSFORM_CASE, TRANSFORM_ITERS = "a70x37k5", 30


def make_case(rows, G, k, seed):
    """(X, W0, H0): X = log1p(poisson(W_t H_t)) with a sparse H_t, row 3 all zero, gene columns 2 and G - 1 all zero; a
    custom start (W0, H0) with exact zeros in it."""
    rng = np.random.RandomState(seed)
    kt = max(k, 2)
    Wt = rng.gamma(1.0, 1.0, size=(rows, kt))
    Ht = rng.gamma(1.0, 2.0, size=(kt, G)) * (rng.uniform(size=(kt, G)) < 0.3)
    X = np.log1p(rng.poisson(Wt @ Ht).astype(np.float64))
    X[min(3, rows - 1)] = 0.0
    X[:, 2] = 0.0
    X[:, G - 1] = 0.0
    avg = np.sqrt(X.mean() / k)
    H0 = avg * np.abs(rng.standard_normal((k, G)))
    W0 = avg * np.abs(rng.standard_normal((rows, k)))
    W0[1, 0] = 0.0
    H0[0, 5] = 0.0
    return X, W0, H0


def case(name):
    for c in CASES + (STACKED,):
        if c[0] == name:
            return make_case(*c[1:])
    raise KeyError(name)


def random_init(X, k, seed):
    """sklearn's ``_initialize_nmf(init="random")``: H is drawn first, then W."""
    X = np.asarray(X, dtype=np.float64)
    avg = np.sqrt(X.mean() / k)
    rng = np.random.RandomState(seed)
    H = avg * rng.standard_normal(size=(k, X.shape[1]))
    W = avg * rng.standard_normal(size=(X.shape[0], k))
    np.abs(H, out=H)
    np.abs(W, out=W)
    return W, H


def update_w(X, W, H, loss):
    if loss == "frobenius":
        num = X @ H.T
        den = W @ (H @ H.T)
    else:
        WH = W @ H
        WH[WH < EPSILON] = EPSILON
        num = (X / WH) @ H.T
        den = np.sum(H, axis=1)[None, :].copy()
    den[den == 0] = EPSILON
    return W * (num / den)


def update_h(X, W, H, loss):
    if loss == "frobenius":
        num = W.T @ X
        den = np.linalg.multi_dot([W.T, W, H])
    else:
        WH = W @ H
        WH[WH < EPSILON] = EPSILON
        num = W.T @ (X / WH)
        ws = np.sum(W, axis=0)
        ws[ws == 0] = 1.0
        den = ws[:, None].copy()
    den[den == 0] = EPSILON
    H = H * (num / den)
    if loss != "frobenius":
        H[H < EPS] = 0.0
    return H


def error(X, W, H, loss):
    """sklearn's ``_beta_divergence(X, W, H, beta, square_root=True)``."""
    WH = W @ H
    if loss == "frobenius":
        d = (X - WH).ravel()
        return float(np.sqrt(np.dot(d, d)))
    x, wh = X.ravel(), WH.ravel()
    keep = x > EPSILON
    x, wh = x[keep], wh[keep]
    wh[wh < EPSILON] = EPSILON
    res = np.dot(x, np.log(x / wh)) + (np.dot(np.sum(W, axis=0), np.sum(H, axis=1)) - x.sum())
    return float(np.sqrt(2 * max(res, 0)))


def fit(X, W0, H0, loss, max_iter, tol, update_H=True):
    """(W, H, n_iter, converged, history): ``history`` holds the error at init and at every check."""
    X = np.asarray(X, dtype=np.float64)
    W, H = np.array(W0, dtype=np.float64), np.array(H0, dtype=np.float64)
    init = prev = error(X, W, H, loss)
    history, n_iter, converged = [init], max_iter, False
    for it in range(1, max_iter + 1):
        W = update_w(X, W, H, loss)
        if update_H:
            H = update_h(X, W, H, loss)
        if tol > 0 and it % 10 == 0:
            err = error(X, W, H, loss)
            history.append(err)
            if (prev - err) / init < tol:
                n_iter, converged = it, it < max_iter
                break
            prev = err
    return W, H, n_iter, converged, np.array(history)


def transform(X, H, loss, max_iter, tol):
    """sklearn's ``NMF(solver="mu").transform``: H fixed, W from ``full(sqrt(X.mean() / k))``."""
    X = np.asarray(X, dtype=np.float64)
    k = H.shape[0]
    W0 = np.full((X.shape[0], k), np.sqrt(X.mean() / k))
    W, _, n_iter, converged, hist = fit(X, W0, H, loss, max_iter, tol, update_H=False)
    return W, n_iter, converged, hist


def permuted_spread(X, W0, H0, loss, iters, seed=0):
    """max |difference| / max |value| of W and of H between the restatement and itself under a row and gene permutation
    (another summation order): the reference's own spread."""
    rng = np.random.RandomState(seed)
    pr, pg = rng.permutation(X.shape[0]), rng.permutation(X.shape[1])
    W, H = fit(X, W0, H0, loss, iters, 0.0)[:2]
    Wp, Hp = fit(X[pr][:, pg], W0[pr], H0[:, pg], loss, iters, 0.0)[:2]
    return float(np.abs(Wp - W[pr]).max() / np.abs(W).max()), float(np.abs(Hp - H[:, pg]).max() / np.abs(H).max())


# ------------------------------------------------------------------------------------------------- one-step bounds
def step_bounds(rows, G, k, loss):
    """Relative bounds (new W, new H) of one iteration, element by element: every sum is over non-negative
    terms, so a sum of m terms carries a relative error of at most m eps whatever its order."""
    a = (G + 2 * k + 3) * EPS if loss == "frobenius" else (2 * G + k + 3) * EPS
    return a, 3 * a + (2 * rows + k + 3) * EPS


def error_bound(X, W, H, loss):
    """How far two fp64 evaluations of ``error`` of the same (X, W, H) may lie apart.  The error is not a sum of
    non-negative inputs: x - WH and the three terms of the KL divergence cancel.  With m = rows + G + k + 4 covering any
    summation order and the k-term WH: Frobenius |d err| <= 2 (k + 2) eps ||WH||_F + 2 m eps err; KL |d res| <= 2 eps
    ((k + 4) sum x + m (sum |x log(x / WH)| + sum x + sum WH)) and d err = d res / err."""
    rows, G = X.shape
    k = W.shape[1]
    WH = W @ H
    err = error(X, W, H, loss)
    m = rows + G + k + 4
    if loss == "frobenius":
        return 2 * (k + 2) * EPS * float(np.sqrt((WH * WH).sum())) + 2 * m * EPS * err
    keep = X > EPSILON
    x, wh = X[keep], np.maximum(WH[keep], EPSILON)
    dres = 2 * EPS * ((k + 4) * x.sum() + m * (np.abs(x * np.log(x / wh)).sum() + x.sum() + WH.sum()))
    return float(dres / err) if err > 0 else float(np.sqrt(2 * dres))


# --------------------------------------------------------------------------------------------------- recovery, host
def normalise(W, H):
    """(programs, usage, dominant) of one segment: H rows scaled to sum 1, the scale moved into W."""
    hs = H.sum(axis=1)
    programs = np.where(hs[:, None] > 0, H / np.where(hs > 0, hs, 1.0)[:, None], 0.0)
    usage = W * hs[None, :]
    dominant = np.where(usage.max(axis=1) > 0, usage.argmax(axis=1), -1).astype(np.int32)
    return programs, usage, dominant
