"""NumPy restatement of the exact t-SNE arithmetic DESIGN 6.10 states (sklearn's exact path, two components), the
yardstick of tests/test_tsne_host.py (against sklearn's own functions, recorded in tests/golden/tsne.npz) and of
tests/test_tsne_gpu.py (against the kernels).  Every function takes ``dtype`` so that the fixture generator can measure
the restatement's own rounding against a longdouble run."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne.npz")

# name -> (segment sizes, D, perplexity)
CASES = {"a": ((33,), 9, 5.0), "b": ((130,), 9, 30.0), "c": ((257,), 50, 30.0), "d": ((64,), 3, 10.0),
         "e": ((65,), 9, 10.0), "f": ((37, 130, 64), 9, 10.0)}
SINGLE = "abcde"
EPS = 2.220446049250313e-16          # sklearn's MACHINE_EPSILON
SEARCH_STEPS, SEARCH_TOL, ZERO_SUM = 100, 1e-5, 1e-8
EXPLORATION_ITERS, CHECK_EVERY = 250, 50
TRAJECTORY = 60                      # iterations of the recorded short trajectories
SAMPLE = 512                         # entries of P stored for the larger cases


def make_case(name):
    """(X, blob label per row): three Gaussian blobs per segment, seeded by the case name.  Case e repeats 4 rows; case f
    is float32."""
    sizes, D, _ = CASES[name]
    rng = np.random.RandomState(1000 + ord(name))
    xs, labs = [], []
    for n in sizes:
        centres = 6.0 * rng.standard_normal((3, D))
        lab = np.arange(n) % 3
        xs.append(centres[lab] + rng.standard_normal((n, D)))
        labs.append(lab)
    X, lab = np.concatenate(xs), np.concatenate(labs)
    if name == "e":
        X[[7, 20, 41, 64]] = X[[3, 3, 40, 0]]
    if name == "f":
        X = X.astype(np.float32)
    return X, lab


def offsets_of(name):
    return np.concatenate([[0], np.cumsum(CASES[name][0])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------- affinities
def sq_distances(X, float32=False, dtype=np.float64):
    """d_ij = sum_k (x_ik - x_jk)^2, summed over k in index order; ``float32``: rounded to float32 and back."""
    X = np.asarray(X).astype(dtype)
    n, D = X.shape
    d = np.zeros((n, n), dtype=dtype)
    for k in range(D):
        t = X[:, k][:, None] - X[:, k][None, :]
        d = d + t * t
    return d.astype(np.float32).astype(dtype) if float32 else d


def binary_search(d, perplexity, dtype=np.float64):
    """sklearn.manifold._utils._binary_search_perplexity on the (n, n) squared distances: (C, beta), all rows at once."""
    d = np.asarray(d).astype(dtype)
    n = d.shape[0]
    off_diag = ~np.eye(n, dtype=bool)
    target = np.log(dtype(perplexity))
    beta = np.ones(n, dtype=dtype)
    lo, hi = np.full(n, -np.inf, dtype=dtype), np.full(n, np.inf, dtype=dtype)
    C = np.zeros((n, n), dtype=dtype)
    todo = np.ones(n, dtype=bool)
    for step in range(SEARCH_STEPS):
        r = np.flatnonzero(todo)
        if r.size == 0:
            break
        e = np.where(off_diag[r], np.exp(-d[r] * beta[r, None]), dtype(0))
        s = e.sum(axis=1)
        s = np.where(s == 0, dtype(ZERO_SUM), s)
        H = np.log(s) + beta[r] * (d[r] * e).sum(axis=1) / s
        C[r] = e / s[:, None]
        diff = H - target
        stop = np.abs(diff) <= SEARCH_TOL
        todo[r[stop]] = False
        if step == SEARCH_STEPS - 1:
            break
        up, dn = r[~stop & (diff > 0)], r[~stop & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2, (beta[up] + hi[up]) / 2)
        hi[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2, (beta[dn] + lo[dn]) / 2)
    return C, beta


def joint_from_conditional(C):
    P = C + C.T
    total = max(P.sum(), EPS)
    P = np.maximum(P / total, EPS)
    np.fill_diagonal(P, 0)
    return P


def joint_probabilities(X, perplexity, float32_distances=False, dtype=np.float64, distances=None):
    """(P, beta) of one segment."""
    d = sq_distances(X, float32_distances, dtype) if distances is None else np.asarray(distances).astype(dtype)
    C, beta = binary_search(d, perplexity, dtype)
    return joint_from_conditional(C), beta


# --------------------------------------------------------------------------------------------------------- gradient
def gradient(P, Y, exaggeration=1.0, dtype=np.float64):
    """(grad, KL, min Q) of one segment at Y (n, 2) over p' = exaggeration P."""
    Pe = np.asarray(P).astype(dtype) * dtype(exaggeration)
    Y = np.asarray(Y).astype(dtype)
    n = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1 / (1 + (diff * diff).sum(axis=2))
    off_diag = ~np.eye(n, dtype=bool)
    sum_q = w[off_diag].sum()
    A = ((Pe * w)[:, :, None] * diff).sum(axis=1)
    R = ((w * w)[:, :, None] * diff).sum(axis=1)
    grad = 4 * (A - R / sum_q)
    K = (Pe * np.log(np.maximum(Pe, EPS) / w)).sum()
    return grad, K + np.log(sum_q) * Pe.sum(), (w[off_diag] / sum_q).min()


def step(Y, grad, update, gains, momentum, lr):
    """One sklearn ``_gradient_descent`` step: (Y, update, gains, squared norm of the gain-scaled gradient)."""
    inc = update * grad < 0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    g = grad * gains
    update = momentum * update - lr * g
    return Y + update, update, gains, (g * g).sum()


def learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def run(P, Y0, n_iter, early_exaggeration=12.0, lr=None, keep=(), dtype=np.float64):
    """The schedule of one segment for ``n_iter`` iterations (no early stop is taken: the fixture's trajectories meet
    none).  Returns Y, the KL of the last iteration, and ``trace``: Y after the iterations listed in ``keep``."""
    P = np.asarray(P).astype(dtype)
    Y = np.asarray(Y0).astype(dtype).copy()
    n = Y.shape[0]
    lr = dtype(learning_rate(n, early_exaggeration) if lr is None else lr)
    switch = min(EXPLORATION_ITERS, n_iter)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    trace, kl, min_q = {}, np.nan, np.inf
    for it in range(n_iter):
        if it == switch:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        first = it < switch
        grad, kl, q = gradient(P, Y, early_exaggeration if first else 1.0, dtype)
        min_q = min(min_q, q)
        Y, update, gains, _ = step(Y, grad, update, gains, dtype(0.5 if first else 0.8), lr)
        if it + 1 in keep:
            trace[it + 1] = Y.copy()
    return {"Y": Y, "kl": kl, "trace": trace, "min_q": min_q}


def nn_purity(Y, labels):
    """The share of points whose nearest embedded neighbour carries their own label."""
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(labels[np.argmin(d, axis=1)] == labels))


def sample_index(n):
    """The fixed sample of entries of an (n, n) matrix the fixture stores for the larger cases."""
    rng = np.random.RandomState(n)
    return rng.randint(0, n, SAMPLE), rng.randint(0, n, SAMPLE)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
