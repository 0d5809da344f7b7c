"""The four calls of csrc/deconv.hip restated in numpy, step for step: ``gram``, ``products``, ``solve`` and
``residual``, the fixtures of the deconvolution tests (``make_case``) and the bounds they assert (``coef_bound``,
``kkt_tolerance``, ``rnorm_bound``).  The restatement states the rule; it does not reproduce the device's summation order
inside a dot product (numpy's pairwise sums stand for the MFMA and the butterflies), so device results are compared by the
bounds, not bit for bit.  ``scipy_nnls`` is the yardstick: ``scipy.optimize.nnls`` once per spot."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_T, MAX_G = 64, 16384
LDS_BYTES = 155648
# (G, T, n, collinear): the cases of tests/golden/deconv.npz
CASES = [(5, 1, 40, 0.0), (7, 2, 40, 0.0), (64, 12, 257, 0.0), (171, 20, 200, 0.9), (785, 33, 300, 0.0),
         (785, 64, 300, 0.99), (130, 64, 200, 0.0)]
SLIDES_CASE = (171, 20, 1025, 0.0)           # split over slides of 2, 37 and 986 rows
SLIDES = (2, 37, 986)


def case_name(G, T, n, collinear):
    return f"g{G}_t{T}_n{n}_c{int(round(100 * collinear))}"


def case_seed(G, T, n):
    return 1000 * G + 10 * T + n % 7


def make_case(G, T, n, seed, collinear=0.0):
    """(S (T, G), x (n, G)), both exactly representable in fp32.  Positive signatures (row 1 optionally ``collinear`` row 0
    + (1 - ``collinear``) itself); spots = sparse Dirichlet mixtures of them plus Gaussian noise; row 0 all zero, row 1 all
    negative (the solution is exactly 0), row 2 exactly signature 0 (a vertex)."""
    assert n >= 3 and 1 <= T <= G
    rng = np.random.default_rng(seed)
    S = rng.gamma(2.0, 1.0, size=(T, G)) + 0.05
    if collinear and T > 1:
        S[1] = collinear * S[0] + (1.0 - collinear) * S[1]
    S = S.astype(np.float32).astype(np.float64)
    b = np.zeros((n, T))
    for i in range(n):
        k = int(rng.integers(1, min(T, 4) + 1))
        pick = rng.choice(T, size=k, replace=False)
        b[i, pick] = rng.dirichlet(np.ones(k)) * rng.uniform(0.5, 2.0)
    x = b @ S + 0.05 * rng.standard_normal((n, G))
    x[0] = 0.0
    x[1] = -np.abs(x[1]) - 0.1
    x = x.astype(np.float32).astype(np.float64)
    x[2] = S[0]
    return S, x


def solve_waves(T):
    """The spots a workgroup of the solve kernel takes at a time: LDS left beside A over a wave's triangle and list."""
    return min(16, (LDS_BYTES - 8 * T * T) // (8 * (T * (T + 1) // 2 + (T + 1) // 2)))


# ------------------------------------------------------------------------------------------------------------- gram
def gram(S):
    """(A, L, status): A = S S^T (upper triangle, mirrored), the Cholesky factor of A column by column, status[0] = 1 + the
    first type whose pivot is not above T eps A_jj, status[1] = 1 + the first type with a non-finite entry."""
    S = np.asarray(S, dtype=np.float64)
    T = S.shape[0]
    status = np.zeros(2, dtype=np.int64)
    with np.errstate(all="ignore"):
        A = np.triu(S @ S.T)
    A = A + np.triu(A, 1).T
    L = np.zeros((T, T))
    bad = np.flatnonzero(~np.isfinite(S).all(axis=1))
    if bad.size:
        status[1] = int(bad[0]) + 1
        return A, L, status
    W = A.copy()
    for k in range(T):
        d = W[k, k]
        if not d > T * EPS * A[k, k]:
            status[0] = k + 1
            break
        root = np.sqrt(d)
        W[k, k] = root
        W[k + 1:, k] = W[k + 1:, k] / root
        W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], W[k + 1:, k])
    return A, np.tril(W), status


# --------------------------------------------------------------------------------------------------------- products
def products(x, S):
    """(c (rows, T), q (rows,), status): c_i = S x_i, q_i = x_i . x_i in fp64 (x converted on load); status = the first row
    with a non-finite entry, -1 for none."""
    x = np.asarray(x).astype(np.float64)
    bad = np.flatnonzero(~np.isfinite(x).all(axis=1))
    with np.errstate(all="ignore"):
        return x @ np.asarray(S, dtype=np.float64).T, np.einsum("ij,ij->i", x, x), int(bad[0]) if bad.size else -1


# ------------------------------------------------------------------------------------------------------------ solve
class _Factor:
    """The Cholesky factor of A_PP in list order: ``L[p, :p + 1]`` is row p; ``rdiag[p]`` = 1 / L[p, p]."""

    def __init__(self, A):
        self.A, self.T = A, A.shape[0]
        self.order, self.L, self.rdiag = [], np.zeros(A.shape), np.zeros(A.shape[0])

    def _sweep(self, r):
        """forward substitution L y = r by columns: y_k = r_k rdiag_k, then every later entry loses its multiple"""
        m = len(r)
        y = np.array(r, dtype=np.float64)
        for k in range(m):
            y[k] = y[k] * self.rdiag[k]
            y[k + 1:] = y[k + 1:] - self.L[k + 1:m, k] * y[k]
        return y

    def append(self, j):
        m = len(self.order)
        ell = self._sweep(self.A[j, self.order])
        d = self.A[j, j]
        for k in range(m):
            d = d - ell[k] * ell[k]
        if not d > self.T * EPS * self.A[j, j]:
            return False
        root = np.sqrt(d)
        self.L[m, :m], self.L[m, m], self.rdiag[m] = ell, root, 1.0 / root
        self.order.append(j)
        return True

    def pop(self):
        self.order.pop()

    def solve(self, c):
        m = len(self.order)
        y = self._sweep(c[self.order])
        for k in range(m - 1, -1, -1):
            y[k] = y[k] * self.rdiag[k]
            y[:k] = y[:k] - self.L[k, :k] * y[k]
        return y

    def remove(self, leaving):
        """the indices in ``leaving`` go; the factor is recomputed from the first removed position onward"""
        first = min(self.order.index(j) for j in leaving)
        tail = [j for j in self.order[first:] if j not in leaving]
        del self.order[first:]
        return all(self.append(j) for j in tail)


def solve_one(A, c, cap=None):
    """Lawson-Hanson on the normal equations of one spot.  Returns (b, inner solves, converged).  ``cap``: the inner
    solves allowed (the device's 3 T)."""
    T = A.shape[0]
    b, w = np.zeros(T), np.array(c, dtype=np.float64)
    tol = 10.0 * T * EPS * np.abs(c).max()
    f = _Factor(A)
    it, cap = 0, 3 * T if cap is None else cap
    while len(f.order) < T:
        outside = np.ones(T, dtype=bool)
        outside[f.order] = False
        cand = np.where(outside, w, -np.inf)
        j = int(np.argmax(cand))                                 # ties: the smaller index
        if not cand[j] > tol:
            break
        if not f.append(j):
            return b, it, 0
        first, rejected = True, False
        while True:
            if it >= cap:
                return b, it, 0
            it += 1
            z = np.zeros(T)
            z[f.order] = f.solve(c)
            if first and not z[j] > 0.0:                         # the entering index steps back out
                f.pop()
                w[j] = 0.0
                rejected = True
                break
            first = False
            P = np.array(f.order)
            if z[P].min() > 0.0:
                b = z
                break
            neg = P[z[P] <= 0.0]
            ratio = b[neg] / (b[neg] - z[neg])
            alpha = ratio.min()
            step = np.zeros(T)
            step[P] = b[P] + alpha * (z[P] - b[P])
            b = step
            leaving = set(P[b[P] <= 0.0].tolist()) | set(neg[ratio == alpha].tolist())
            b[list(leaving)] = 0.0
            if not f.remove(leaving):
                return b, it, 0
            if not f.order:
                break
        if rejected:
            continue
        w = c - A @ b
    return b, it, 1


def solve(A, c):
    """(coef (rows, T), n_iter int32, converged uint8) of every row of c."""
    out = [solve_one(A, ci) for ci in np.asarray(c, dtype=np.float64)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.uint8))


# --------------------------------------------------------------------------------------------------------- residual
def residual(x, S, coef, q):
    """(rnorm, r2, proportions, dominant): the residual norm from x itself, r2 = 1 - rnorm^2 / q (NaN where q = 0),
    proportions = coef / sum(coef) summed over the types ascending (a zero row where the sum is 0), dominant = its argmax
    (ties: the smaller index; -1 for a zero row)."""
    x, S, coef = np.asarray(x).astype(np.float64), np.asarray(S, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    r = x - coef @ S
    ss = np.einsum("ij,ij->i", r, r)
    with np.errstate(all="ignore"):
        r2 = np.where(q == 0.0, np.nan, 1.0 - ss / q)
    tot = np.zeros(coef.shape[0])
    for t in range(coef.shape[1]):
        tot = tot + coef[:, t]
    with np.errstate(all="ignore"):
        prop = np.where(tot[:, None] > 0.0, coef / tot[:, None], 0.0)
    dom = np.where(tot > 0.0, np.argmax(prop, axis=1), -1).astype(np.int32)
    return np.sqrt(ss), r2, prop, dom


def nnls(x, S):
    """The chain of the four calls: what ``mclstexp_amd.deconv.nnls`` returns."""
    A, _, status = gram(S)
    assert not status.any(), status
    c, q, bad = products(x, S)
    assert bad < 0, bad
    coef, n_iter, conv = solve(A, c)
    rnorm, r2, prop, dom = residual(x, S, coef, q)
    return {"coef": coef, "rnorm": rnorm, "r2": r2, "n_iter": n_iter, "converged": conv, "proportions": prop,
            "dominant": dom}


# ----------------------------------------------------------------------------------------------------------- bounds
def scipy_nnls(x, S):
    """(coef, rnorm) of ``scipy.optimize.nnls(S^T, x_i)`` spot by spot."""
    from scipy.optimize import nnls as sp_nnls
    out = [sp_nnls(np.asarray(S, dtype=np.float64).T, xi) for xi in np.asarray(x, dtype=np.float64)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def coef_bound(x, S):
    """4 (G + T) eps || |S| |x_i| ||_2 / lambda_min(A) per spot: the perturbation bound of the normal equations under the
    rounding of c (lambda_min(A_PP) >= lambda_min(A) by interlacing)."""
    S, x = np.asarray(S, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, G = S.shape
    lam = float(np.linalg.eigvalsh(S @ S.T)[0])
    return 4.0 * (G + T) * EPS * np.linalg.norm(np.abs(x) @ np.abs(S).T, axis=1) / lam


def kkt_tolerance(x, S, coef):
    """t = 4 (G + T) eps (|| |S| |x_i| ||_inf + || |A| |b_i| ||_inf) per spot."""
    S, x = np.asarray(S, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, G = S.shape
    A = S @ S.T
    return 4.0 * (G + T) * EPS * ((np.abs(x) @ np.abs(S).T).max(axis=1) + (np.abs(coef) @ np.abs(A)).max(axis=1))


def check_kkt(x, S, coef):
    """The certificate from ``coef`` alone: coef >= 0 exactly, w = S x - A b <= t where b = 0, |w| <= t where b > 0."""
    S, x = np.asarray(S, dtype=np.float64), np.asarray(x, dtype=np.float64)
    assert (coef >= 0.0).all()
    w = x @ S.T - coef @ (S @ S.T)
    t = kkt_tolerance(x, S, coef)[:, None]
    zero = coef == 0.0
    assert (w[zero] <= np.broadcast_to(t, w.shape)[zero]).all(), float((w - t)[zero].max())
    assert (np.abs(w)[~zero] <= np.broadcast_to(t, w.shape)[~zero]).all(), float((np.abs(w) - t)[~zero].max())


def rnorm_bound(x, S):
    """sqrt(T) ||S||_2 (the coef bound) + 4 (G + T) eps ||x_i||_2."""
    S, x = np.asarray(S, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, G = S.shape
    return np.sqrt(T) * np.linalg.norm(S, 2) * coef_bound(x, S) + 4.0 * (G + T) * EPS * np.linalg.norm(x, axis=1)


def r2_bound(x, S, coef, q):
    """The rounding of sum_g (x_g - sum_t S_tg b_t)^2 summed in two orders, over q: 4 (G + T) eps || |x_i| + |S|^T |b_i|
    ||_2^2 / q_i, and 4 eps for the division and the subtraction from 1."""
    S, x = np.asarray(S, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, G = S.shape
    mag = np.abs(x) + np.abs(coef) @ np.abs(S)
    with np.errstate(all="ignore"):
        return 4.0 * (G + T) * EPS * np.einsum("ij,ij->i", mag, mag) / q + 4.0 * EPS
