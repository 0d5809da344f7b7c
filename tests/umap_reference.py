"""NumPy restatement of the UMAP layout DESIGN 6.12 states (one Jacobi step per epoch over the connectivities CSR of
tests/neighbors_reference.py, counter-based negative sampling), the yardstick of tests/test_umap_host.py and
tests/test_umap_gpu.py.  ``run`` takes ``dtype`` so that the fixture generator can measure the restatement's own rounding
against a longdouble run; the schedule is always float64, it is exact by definition.  ``run_sequential`` is the same
schedule and the same samples with umap-learn's in-place updates; only the fixture generator uses it, to show that the
Jacobi form gives up nothing.  Where this statement and a umap-learn release differ, the statement holds."""
import os

import numpy as np

import neighbors_reference as nr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umap.npz")

# name -> (case of neighbors_reference, its segments, start, n_epochs of the compared run)
CASES = {"a": ("a", (0,), "random", 100), "b": ("b", (0, 1, 2), "pca", 40), "d": ("d", (0,), "pca", 100),
         "e": ("b", (1,), "random", None)}
TRAJECTORY = ("a", "b", "d")
SEED = 20261
FULL_SEEDS = (0, 1, 2, 3)                  # case e: the four full runs
TRUST_K = 15
R, GAMMA, ALPHA = 5, 1.0, 1.0
MAX_TRAJECTORY = 60
MASK = (1 << 64) - 1

# mix(x) and k = (((h >> 32) * n) >> 32), worked out with Python integers
MIX_VECTORS = ((0x0000000000000000, 0xE220A8397B1DCDAF), (0x0000000000000001, 0x910A2DEC89025CC1),
               (0xFFFFFFFFFFFFFFFF, 0xE4D971771B652C20), (0x0123456789ABCDEF, 0x157A3807A48FAA9D))
K_VECTORS = ((0xE220A8397B1DCDAF, 151, 133), (0x910A2DEC89025CC1, 16384, 9282), (0xFFFFFFFFFFFFFFFF, 70, 69),
             (0x00000000FFFFFFFF, 16384, 0))


# ---------------------------------------------------------------------------------------------------- the generator
def mix_int(x):
    """The splitmix64 step on a Python integer."""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def mix(x):
    """The same on a uint64 array."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def sample_index(h, n):
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def _u64(a):
    return np.asarray(a).astype(np.uint64)


def negative_samples(seed, epoch, i, r, p, n):
    """k of sample number p of the entry of rank r in row i at ``epoch`` (arrays of equal length)."""
    h = mix(np.uint64(mix_int(seed & MASK)) ^ np.uint64(epoch))
    h = mix(mix(mix(h ^ _u64(i)) ^ _u64(r)) ^ _u64(p))
    return sample_index(h, n).astype(np.int64)


def random_init(n, seed):
    """y = 20 ((h >> 11) 2^-53) - 10, h = mix(mix(mix(seed ^ 0xFFFFFFFFFFFFFFFF) ^ i) ^ c)."""
    h0 = np.uint64(mix_int((seed & MASK) ^ MASK))
    hi = mix(h0 ^ np.arange(n, dtype=np.uint64))
    out = np.empty((n, 2), dtype=np.float64)
    for c in range(2):
        h = mix(hi ^ np.uint64(c))
        out[:, c] = np.float64(20.0) * ((h >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)) - np.float64(10.0)
    return out


def pca_init(X):
    """The first two columns times 10 / (their largest absolute value); all zeros stay zeros."""
    Y = np.array(np.asarray(X)[:, :2], dtype=np.float64)
    m = np.max(np.abs(Y))
    return Y * (np.float64(10.0) / m) if m > 0 else Y


def find_ab_params(spread=1.0, min_dist=0.5):
    """umap-learn's fit of 1 / (1 + a x^(2b)) to the offset exponential."""
    from scipy.optimize import curve_fit
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(n):
    return 500 if n <= 10000 else 200


# ------------------------------------------------------------------------------------------------------- the schedule
def schedule(w, n_epochs, rate=R):
    """(live, eps, epn): every operation one float64 operation."""
    w = np.asarray(w, dtype=np.float64)
    wmax = w.max()
    live = w >= wmax / np.float64(n_epochs)
    eps = wmax / w
    with np.errstate(divide="ignore"):
        epn = eps / np.float64(rate)
    return live, eps, epn


def _csr_parts(m):
    m = m.tocsr()
    assert m.has_sorted_indices
    indptr = m.indptr.astype(np.int64)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(indptr))
    rank = np.arange(indptr[-1]) - indptr[rows]
    return indptr, rows, m.indices.astype(np.int64), rank, np.asarray(m.data, dtype=np.float64)


def _ordered_row_sum(n, crow, C):
    """acc[i] = the contributions of row i added one by one in their order (crow ascends)."""
    acc = np.zeros((n, 2), dtype=C.dtype)
    if crow.size == 0:
        return acc
    pos = np.arange(crow.size) - np.searchsorted(crow, crow, side="left")
    order = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[order], np.arange(pos.max() + 2), side="left")
    for t in range(cuts.size - 1):
        sel = order[cuts[t]:cuts[t + 1]]
        acc[crow[sel]] = acc[crow[sel]] + C[sel]
    return acc


def run(m, Y0, n_epochs, a, b, seed=0, gamma=GAMMA, rate=R, alpha=ALPHA, stop_after=None, keep=(), dtype=np.float64):
    """The Jacobi form on one segment's symmetric CSR ``m``: a dict of Y, attractive_samples, negative_samples, trace
    ({epochs done: Y} for ``keep``), live."""
    indptr, rows, cols, rank, w = _csr_parts(m)
    n = m.shape[0]
    live, eps, epn = schedule(w, n_epochs, rate)
    nxt, nneg = eps.copy(), epn.copy()
    Y = np.array(Y0, dtype=dtype)
    a, b, gamma = dtype(a), dtype(b), dtype(gamma)
    one, two, four = dtype(1), dtype(2), dtype(4)
    n_att = n_neg = 0
    trace = {}
    stop = n_epochs if stop_after is None else min(int(stop_after), n_epochs)
    for ep in range(stop):
        nf = np.float64(ep)
        alpha_n = dtype(np.float64(alpha) * (np.float64(1.0) - nf / np.float64(n_epochs)))
        act = np.flatnonzero(live & (nxt <= nf))
        i, j = rows[act], cols[act]
        if rate > 0:
            q = np.maximum(0, np.trunc((nf - nneg[act]) / epn[act])).astype(np.int64)
        else:
            q = np.zeros(act.size, dtype=np.int64)
        # attraction
        d = Y[i] - Y[j]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        pos = d2 > 0
        safe = np.where(pos, d2, one)
        c = np.where(pos, -two * a * b * np.power(safe, b - one) / (a * np.power(safe, b) + one), dtype(0))
        att = two * np.clip(c[:, None] * d, -four, four)
        # repulsion
        owner = np.repeat(np.arange(act.size), q)
        first = np.cumsum(q) - q
        p = np.arange(owner.size) - first[owner]
        k = negative_samples(seed, ep, i[owner], rank[act][owner], p, n)
        dn = Y[i[owner]] - Y[k]
        dn2 = dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]
        posn = dn2 > 0
        safen = np.where(posn, dn2, one)
        cn = np.where(posn, two * gamma * b / ((dtype(0.001) + safen) * (a * np.power(safen, b) + one)), dtype(0))
        rep = np.where(posn[:, None], np.clip(cn[:, None] * dn, -four, four), dtype(0))
        # every row's contributions in order: an entry's attraction, then its samples
        start = np.cumsum(1 + q) - (1 + q)
        C = np.zeros((act.size + owner.size, 2), dtype=dtype)
        crow = np.empty(act.size + owner.size, dtype=np.int64)
        C[start], crow[start] = att, i
        C[start[owner] + 1 + p], crow[start[owner] + 1 + p] = rep, i[owner]
        Y = Y + alpha_n * _ordered_row_sum(n, crow, C)
        nxt[act] = nxt[act] + eps[act]
        if rate > 0:
            nneg[act] = nneg[act] + q.astype(np.float64) * epn[act]
        n_att += int(act.size)
        n_neg += int(q.sum())
        if ep + 1 in keep:
            trace[ep + 1] = Y.copy()
    return {"Y": Y, "attractive_samples": n_att, "negative_samples": n_neg, "trace": trace, "live": live}


def run_sequential(m, Y0, n_epochs, a, b, seed=0, gamma=GAMMA, rate=R, alpha=ALPHA):
    """The same schedule and samples with umap-learn's in-place updates in storage order: the head of (i, j) moves, its
    tail moves the other way, then the head moves away from each sample."""
    indptr, rows, cols, rank, w = _csr_parts(m)
    n = m.shape[0]
    live, eps, epn = schedule(w, n_epochs, rate)
    nxt, nneg = eps.copy(), epn.copy()
    y = [[float(v[0]), float(v[1])] for v in np.asarray(Y0, dtype=np.float64)]
    a, b, gamma = float(a), float(b), float(gamma)

    def clip(v):
        return 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)

    for ep in range(n_epochs):
        alpha_n = float(alpha) * (1.0 - ep / n_epochs)
        act = np.flatnonzero(live & (nxt <= ep))
        q = np.maximum(0, np.trunc((ep - nneg[act]) / epn[act])).astype(np.int64) if rate > 0 else np.zeros(act.size, int)
        owner = np.repeat(np.arange(act.size), q)
        first = np.cumsum(q) - q
        ks = negative_samples(seed, ep, rows[act][owner], rank[act][owner], np.arange(owner.size) - first[owner], n).tolist()
        at = 0
        for e, qe in zip(act.tolist(), q.tolist()):
            yi, yj = y[rows[e]], y[cols[e]]
            d0, d1 = yi[0] - yj[0], yi[1] - yj[1]
            d2 = d0 * d0 + d1 * d1
            if d2 > 0:
                c = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
                g0, g1 = clip(c * d0), clip(c * d1)
                yi[0] += alpha_n * g0
                yi[1] += alpha_n * g1
                yj[0] -= alpha_n * g0
                yj[1] -= alpha_n * g1
            for k in ks[at:at + qe]:
                yk = y[k]
                d0, d1 = yi[0] - yk[0], yi[1] - yk[1]
                d2 = d0 * d0 + d1 * d1
                if d2 > 0:
                    c = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                    yi[0] += alpha_n * clip(c * d0)
                    yi[1] += alpha_n * clip(c * d1)
            at += qe
        nxt[act] = nxt[act] + eps[act]
        if rate > 0:
            nneg[act] = nneg[act] + q.astype(np.float64) * epn[act]
    return np.array(y)


# ---------------------------------------------------------------------------------------------------------- the cases
def case_input(name):
    """(X of the case's segments row-stacked, their sizes, k)."""
    src, segs, _, _ = CASES[name]
    X, off = nr.make_case(src), nr.offsets_of(src)
    return np.concatenate([X[off[s]:off[s + 1]] for s in segs]), [int(off[s + 1] - off[s]) for s in segs], nr.CASES[src][2]


def case_labels(name):
    """neighbors_reference.make_case draws row i of a segment around centre i % 3."""
    _, sizes, _ = case_input(name)
    return np.concatenate([np.arange(n) % 3 for n in sizes])


def case_graphs(name):
    """One symmetric scipy CSR per segment: the restatement's connectivities of the case's input."""
    X, sizes, k = case_input(name)
    off = np.concatenate([[0], np.cumsum(sizes)])
    out = []
    for s in range(len(sizes)):
        g = nr.graph(X[off[s]:off[s + 1]], k)
        out.append(nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"]))
    return out


def case_start(name, seed=SEED):
    X, sizes, _ = case_input(name)
    off = np.concatenate([[0], np.cumsum(sizes)])
    if CASES[name][2] == "random":
        return np.concatenate([random_init(n, seed) for n in sizes])
    return np.concatenate([pca_init(X[off[s]:off[s + 1]]) for s in range(len(sizes))])


# ------------------------------------------------------------------------------------------------------------ scores
def nn_purity(Y, labels):
    """The share of points whose nearest embedded neighbour carries their own label."""
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(labels[np.argmin(d, axis=1)] == labels))


def trustworthiness(X, Y, k=TRUST_K):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k) for the Euclidean metric (the generator checks it is)."""
    n = X.shape[0]
    dx = nr.sq_distances(X)
    np.fill_diagonal(dx, np.inf)
    rank_x = np.empty((n, n), dtype=np.int64)
    rank_x[np.arange(n)[:, None], np.argsort(dx, axis=1, kind="stable")] = np.arange(1, n + 1)[None, :]
    dy = nr.sq_distances(Y)
    np.fill_diagonal(dy, np.inf)
    near = np.argsort(dy, axis=1, kind="stable")[:, :k]
    t = np.take_along_axis(rank_x, near, axis=1) - k
    return float(1.0 - np.sum(t[t > 0]) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))

