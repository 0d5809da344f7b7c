"""NumPy + scipy.sparse restatement of the neighbourhood-graph arithmetic DESIGN 6.11 states (exact kNN, umap-learn's
smooth_knn_dist and compute_membership_strengths with the fuzzy union), the yardstick of tests/test_neighbors_host.py and
tests/test_neighbors_gpu.py.  Every function takes ``dtype`` so that the fixture generator can measure the restatement's
own rounding against a longdouble run.  Where this statement and a umap-learn release differ, the statement holds."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neighbors.npz")

# name -> (segment sizes, D, k)
CASES = {"a": ((70,), 5, 15), "b": ((257, 151, 300), 50, 150), "c": ((1100,), 9, 256), "d": ((130,), 3, 10)}
SEEDS = {"a": 2001, "b": 2002, "c": 2005, "d": 2004}      # chosen so that the generator's guards hold
RANDOM = "abc"                       # the cases with recorded sklearn agreement; d holds exact ties
SMOOTH_STEPS, SMOOTH_TOL, MIN_SCALE = 64, 1e-5, 1e-3


def make_case(name):
    """The (rows, D) float64 input.  a-c: three Gaussian blobs per segment.  d: integer coordinates in 0..3 (64 distinct
    points for 130 rows: exact duplicates, exact ties in d^2), its first eleven rows one point, so that rows 0..10 have no
    positive distance among their ten neighbours (rho = 0 and the segment-mean floor)."""
    sizes, D, _ = CASES[name]
    rng = np.random.RandomState(SEEDS[name])
    if name == "d":
        X = rng.randint(0, 4, size=(sizes[0], D)).astype(np.float64)
        X[:11] = X[0]
        return X
    xs = []
    for n in sizes:
        centres = 4.0 * rng.standard_normal((3, D))
        xs.append(centres[np.arange(n) % 3] + rng.standard_normal((n, D)))
    return np.concatenate(xs)


def offsets_of(name):
    return np.concatenate([[0], np.cumsum(CASES[name][0])]).astype(np.int64)


# -------------------------------------------------------------------------------------------------------------- kNN
def sq_distances(X, dtype=np.float64):
    """d2_ij = sum_c (x_ic - x_jc)^2, summed over c in index order."""
    X = np.asarray(X).astype(dtype)
    n, D = X.shape
    d = np.zeros((n, n), dtype=dtype)
    for c in range(D):
        t = X[:, c][:, None] - X[:, c][None, :]
        d = d + t * t
    return d


def knn(X, k, dtype=np.float64):
    """(indices (n, k) int32, distances (n, k), d2 (n, k)) of one segment: position 0 the row itself at 0, then the other
    rows in ascending (d2, j)."""
    d2 = sq_distances(X, dtype)
    n = d2.shape[0]
    key = d2.copy()
    key[np.arange(n), np.arange(n)] = -1                 # the row itself first; a stable sort breaks ties by index
    idx = np.argsort(key, axis=1, kind="stable")[:, :k]
    sel = np.take_along_axis(d2, idx, axis=1)
    sel[:, 0] = 0
    return idx.astype(np.int32), np.sqrt(sel), sel


# -------------------------------------------------------------------------------------------------------- smoothing
def ordered_sum(a, first=0):
    """Row sums of a[:, first:] in index order."""
    s = np.zeros(a.shape[0], dtype=a.dtype)
    for j in range(first, a.shape[1]):
        s = s + a[:, j]
    return s


def smooth(dist, dtype=np.float64):
    """umap-learn's smooth_knn_dist(n_iter=64, local_connectivity=1, bandwidth=1) on the (n, k) distances of one segment:
    (rho, sigma, info).  info: ``margin`` the smallest | |psum - target| - 1e-5 | met at any step of any row, ``floored``
    the rows whose sigma a floor raised, ``psum`` the last sum of every row."""
    d = np.asarray(dist).astype(dtype)
    n, k = d.shape
    target = dtype(np.log2(k))
    pos = np.where(d > 0, d, dtype(np.inf))
    rho = pos.min(axis=1)
    rho = np.where(np.isinf(rho), dtype(0), rho)
    t = d - rho[:, None]
    lo, hi, mid = np.zeros(n, dtype=dtype), np.full(n, np.inf, dtype=dtype), np.ones(n, dtype=dtype)
    todo = np.ones(n, dtype=bool)
    last = np.zeros(n, dtype=dtype)
    margin = np.inf
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(SMOOTH_STEPS):
            r = np.flatnonzero(todo)
            if r.size == 0:
                break
            e = np.where(t[r] > 0, np.exp(-(t[r] / mid[r, None])), dtype(1))
            psum = ordered_sum(e, 1)
            last[r] = psum
            gap = np.abs(psum - target)
            margin = min(margin, float(np.min(np.abs(gap - dtype(SMOOTH_TOL)))))
            stop = gap < SMOOTH_TOL
            todo[r[stop]] = False
            up, dn = r[~stop & (psum > target)], r[~stop & ~(psum > target)]
            hi[up] = mid[up]
            mid[up] = (lo[up] + hi[up]) / 2
            lo[dn] = mid[dn]
            mid[dn] = np.where(np.isinf(hi[dn]), mid[dn] * 2, (lo[dn] + hi[dn]) / 2)
    row_sum = ordered_sum(d)
    row_floor = dtype(MIN_SCALE) * (row_sum / dtype(k))
    seg_floor = dtype(MIN_SCALE) * (row_sum.sum() / (dtype(n) * dtype(k)))
    floor = np.where(rho > 0, row_floor, seg_floor)
    sigma = np.maximum(mid, floor)
    return rho, sigma, {"margin": margin, "floored": sigma > mid, "psum": last, "stopped": ~todo}


# --------------------------------------------------------------------------------------------------- connectivities
def directed_weights(idx, dist, rho, sigma, dtype=np.float64):
    """(n, k): 0 for the row itself, 1 where d - rho <= 0 or sigma == 0, else exp(-(d - rho) / sigma)."""
    d = np.asarray(dist).astype(dtype)
    rho, sigma = np.asarray(rho).astype(dtype), np.asarray(sigma).astype(dtype)
    n = d.shape[0]
    t = d - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.where((t <= 0) | (sigma[:, None] == 0), dtype(1), np.exp(-(t / sigma[:, None])))
    return np.where(np.asarray(idx) == np.arange(n)[:, None], dtype(0), w)


def connectivities_dense(idx, dist, rho, sigma, mix=1.0, dtype=np.float64):
    """The (n, n) symmetric weights of one segment, 0 where nothing is stored."""
    w = directed_weights(idx, dist, rho, sigma, dtype)
    n = w.shape[0]
    a = np.zeros((n, n), dtype=dtype)
    a[np.repeat(np.arange(n), w.shape[1]), np.asarray(idx).ravel()] = w.ravel()
    b = a.T
    prod = a * b
    out = dtype(mix) * ((a + b) - prod) + (dtype(1) - dtype(mix)) * prod
    out[np.arange(n), np.arange(n)] = 0
    return out


def connectivities(idx, dist, rho, sigma, mix=1.0):
    """scipy.sparse.csr_matrix of the float64 weights: no diagonal, no zeros, sorted columns."""
    from scipy import sparse
    m = sparse.csr_matrix(connectivities_dense(idx, dist, rho, sigma, mix))
    m.eliminate_zeros()
    m.sort_indices()
    return m


def distances_matrix(idx, dist):
    """scanpy's obsp["distances"]: the neighbours other than the row itself at a distance above 0."""
    from scipy import sparse
    n, k = idx.shape
    rows = np.repeat(np.arange(n), k)
    keep = (idx.ravel() != rows) & (dist.ravel() > 0)
    m = sparse.csr_matrix((np.asarray(dist, dtype=np.float64).ravel()[keep], (rows[keep], idx.ravel()[keep])), shape=(n, n))
    m.sort_indices()
    return m


def graph(X, k, mix=1.0, dtype=np.float64):
    """Everything of one segment: a dict of knn_indices, knn_distances, d2, rho, sigma, info, dense."""
    idx, dist, d2 = knn(X, k, dtype)
    rho, sigma, info = smooth(dist, dtype)
    return {"knn_indices": idx, "knn_distances": dist, "d2": d2, "rho": rho, "sigma": sigma, "info": info,
            "dense": connectivities_dense(idx, dist, rho, sigma, mix, dtype)}


def segments(name, X=None, dtype=np.float64):
    """``graph`` of every segment of a case."""
    X = make_case(name) if X is None else X
    off = offsets_of(name)
    return [graph(np.asarray(X[off[s]:off[s + 1]]).astype(dtype), CASES[name][2], 1.0, dtype) for s in range(off.size - 1)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
