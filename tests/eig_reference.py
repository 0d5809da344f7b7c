"""fp64 numpy restatement of csrc/eig.hip (tests only), DESIGN 6.14 step by step: (a) Householder tridiagonalisation on the
full symmetric storage, (b) bisection on the Sturm count for the k largest eigenvalues, (c) block inverse iteration with
``dgttrf`` / ``dgtts2`` solves and group-wise modified Gram-Schmidt, (d) the certificate, (e) the back-transformation,
(f) the sign rule.  Pinned against ``numpy.linalg.eigh`` by tests/test_eig_host.py; its results on the case matrices are the
fixture tests/golden/eig.npz (tests/golden/gen_eig_goldens.py).  The kernels sum in another order than numpy does, so the
device is compared with ``eigh`` inside the method's backward-error bounds, not with this file bit for bit."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eig.npz")
EPS = 2.0 ** -52
SAFEMIN = float(np.finfo(np.float64).tiny)
MAX_M, MAX_K = 4096, 64
N_BISECT = 128       # halvings at most; an interval that no longer splits in fp64 stops earlier
N_ITER = 3           # inverse iterations
PERT = 10.0          # eigenvalues closer than PERT eps |T| to their predecessor are pushed apart (dstein)
ORTOL = 1e-3         # consecutive eigenvalues within ORTOL |T| share a Gram-Schmidt group (dstein)


# ------------------------------------------------------------------------------------------------ (a) tridiagonalisation
def tridiagonalize(a):
    """(d, e, tau, a): T = tridiag(e, d, e) = Q^T A Q; the reflector of column j has v[0] = 1 and v[1:] in a[j+2:, j]."""
    a = np.array(a, dtype=np.float64)
    m = a.shape[0]
    d, e, tau = np.zeros(m), np.zeros(max(m - 1, 0)), np.zeros(max(m - 1, 0))
    for j in range(m - 1):
        x = a[j + 1:, j].copy()
        alpha = x[0]
        xnorm = np.sqrt(np.sum(x[1:] * x[1:]))
        d[j] = a[j, j]
        if xnorm == 0.0:
            e[j] = alpha
            continue
        beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
        t = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1.0
        e[j], tau[j] = beta, t
        a[j + 1:, j] = v
        a[j, j + 1:] = v
        s = a[j + 1:, j + 1:]
        p = t * (s * v[None, :]).sum(axis=1)          # (plain sums, no BLAS: the fixture is reproduced bit for bit)
        w = p - (0.5 * t * (p * v).sum()) * v
        s -= np.outer(v, w) + np.outer(w, v)          # the two products are rounded, then added: exactly symmetric
    d[m - 1] = a[m - 1, m - 1]
    return d, e, tau, a


# --------------------------------------------------------------------------------------------------- (b) eigenvalues of T
def t_norm(d, e):
    """(|T| = the larger absolute Gershgorin bound, lower bound, upper bound)."""
    ea = np.abs(e)
    r = np.concatenate([[0.0], ea]) + np.concatenate([ea, [0.0]])
    gl, gu = float((d - r).min()), float((d + r).max())
    return max(abs(gl), abs(gu)), gl, gu


def sturm_count(d, e2, pivmin, x):
    """Number of eigenvalues of T below each x (dstebz: q <- d_i - x - e_{i-1}^2 / q, |q| < pivmin -> -pivmin)."""
    x = np.asarray(x, dtype=np.float64)
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    count = (q < 0.0).astype(np.int64)
    for i in range(1, d.size):
        q = d[i] - x - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        count += q < 0.0
    return count


def top_eigenvalues(d, e, k):
    """The k largest eigenvalues of T, descending."""
    m = d.size
    tn, gl, gu = t_norm(d, e)
    if tn == 0.0:
        return np.zeros(k)
    e2 = e * e
    pivmin = SAFEMIN * max(1.0, float(e2.max()) if e2.size else 1.0)
    widen = 2.0 * m * EPS * tn + 2.0 * pivmin
    lo, hi = np.full(k, gl - widen), np.full(k, gu + widen)
    want = m - 1 - np.arange(k)                       # ascending index of the i-th largest
    for _ in range(N_BISECT):
        mid = 0.5 * (lo + hi)
        live = (mid > lo) & (mid < hi)                # (an interval that stopped splitting stays as it is)
        if not live.any():
            break
        above = sturm_count(d, e2, pivmin, mid) > want
        hi = np.where(live & above, mid, hi)
        lo = np.where(live & ~above, mid, lo)
    return 0.5 * (lo + hi)


# -------------------------------------------------------------------------------------------------- (c) eigenvectors of T
def _mix(x):
    """The splitmix64 step of csrc/umap.hip on a uint64 array."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def start_vectors(m, k):
    """x[r, c] in [-1, 1) from the hash of (r << 32 | c), every column normalised."""
    r = np.arange(m, dtype=np.uint64)[:, None]
    c = np.arange(k, dtype=np.uint64)[None, :]
    h = _mix((r << np.uint64(32)) | c)
    x = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0
    return x / np.sqrt((x * x).sum(axis=0))


def perturbed(lam, tn):
    lp = lam.copy()
    for i in range(1, lp.size):
        if lp[i - 1] - lp[i] < PERT * EPS * tn:
            lp[i] = lp[i - 1] - PERT * EPS * tn
    return lp


def group_starts(lam, tn):
    g = np.zeros(lam.size, dtype=np.int64)
    for i in range(1, lam.size):
        g[i] = g[i - 1] if lam[i - 1] - lam[i] <= ORTOL * tn else i
    return g


def _floor_pivot(p, floor):
    return np.where(np.abs(p) < floor, np.where(np.signbit(p), -floor, floor), p)


def factor(d, e, shifts, floor):
    """dgttrf of T - shift I for every shift at once (one column each): (dl, dd, du, du2, swapped)."""
    m, k = d.size, shifts.size
    dd = d[:, None] - shifts[None, :]
    dl = np.repeat(e[:, None], k, axis=1)
    du = dl.copy()
    du2 = np.zeros((max(m - 2, 0), k))
    swapped = np.zeros((max(m - 1, 0), k), dtype=bool)
    for r in range(m - 1):
        sw = np.abs(dd[r]) < np.abs(dl[r])
        piv = _floor_pivot(np.where(sw, dl[r], dd[r]), floor)
        other = np.where(sw, dd[r], dl[r])
        fact = other / piv
        nxt, up = dd[r + 1].copy(), du[r].copy()
        dd[r] = piv
        dl[r] = fact
        du[r] = np.where(sw, nxt, up)
        dd[r + 1] = np.where(sw, up - fact * nxt, nxt - fact * up)
        if r < m - 2:
            du2[r] = np.where(sw, du[r + 1], 0.0)
            du[r + 1] = np.where(sw, -fact * du[r + 1], du[r + 1])
        swapped[r] = sw
    dd[m - 1] = _floor_pivot(dd[m - 1], floor)
    return dl, dd, du, du2, swapped


def solve(f, b):
    """dgtts2 (no transpose): every column of b against its own factorisation."""
    dl, dd, du, du2, swapped = f
    b = b.copy()
    m = b.shape[0]
    for r in range(m - 1):
        top, bot = b[r].copy(), b[r + 1].copy()
        b[r] = np.where(swapped[r], bot, top)
        b[r + 1] = np.where(swapped[r], top - dl[r] * bot, bot - dl[r] * top)
    b[m - 1] = b[m - 1] / dd[m - 1]
    if m > 1:
        b[m - 2] = (b[m - 2] - du[m - 2] * b[m - 1]) / dd[m - 2]
    for r in range(m - 3, -1, -1):
        b[r] = (b[r] - du[r] * b[r + 1] - du2[r] * b[r + 2]) / dd[r]
    return b


def orthonormalize(y, groups):
    """In column order: twice modified Gram-Schmidt against the finished columns of the group, then normalise."""
    z = y.copy()
    for i in range(z.shape[1]):
        for _ in range(2):
            for c in range(int(groups[i]), i):
                z[:, i] -= (z[:, c] * z[:, i]).sum() * z[:, c]
        z[:, i] /= np.sqrt((z[:, i] * z[:, i]).sum())
    return z


def t_eigenvectors(d, e, lam):
    m, k = d.size, lam.size
    tn = t_norm(d, e)[0]
    if tn == 0.0:
        return np.eye(m)[:, :k].copy()
    f = factor(d, e, perturbed(lam, tn), EPS * tn)
    groups = group_starts(lam, tn)
    z = start_vectors(m, k)
    for _ in range(N_ITER):
        z = orthonormalize(solve(f, z), groups)
    return z


# ------------------------------------------------------------------------------------------------------ (d) certificate
def t_matvec(d, e, z):
    y = d[:, None] * z
    if d.size > 1:
        y[:-1] += e[:, None] * z[1:]
        y[1:] += e[:, None] * z[:-1]
    return y


def certificate(d, e, lam, z):
    """(max_i |T z_i - lam_i z_i|_2 / |T|, max |Z^T Z - I|); (0, 0) for the zero matrix."""
    tn = t_norm(d, e)[0]
    if tn == 0.0:
        return np.zeros(2)
    r = t_matvec(d, e, z) - lam[None, :] * z
    return np.array([np.sqrt((r * r).sum(axis=0)).max() / tn, np.abs((z[:, :, None] * z[:, None, :]).sum(axis=0) - np.eye(lam.size)).max()])


# ---------------------------------------------------------------------------------- (e) back-transformation, (f) sign
def back_transform(a, tau, z):
    z = z.copy()
    for j in range(a.shape[0] - 3, -1, -1):
        if tau[j] == 0.0:
            continue
        v = a[j + 1:, j].copy()
        v[0] = 1.0
        z[j + 1:] -= tau[j] * np.outer(v, (v[:, None] * z[j + 1:]).sum(axis=0))
    return z


def fix_signs(z):
    top = np.abs(z).argmax(axis=0)                    # ties: the lowest index
    return z * np.where(z[top, np.arange(z.shape[1])] < 0.0, -1.0, 1.0)


def sign_rule_holds(z):
    z = np.asarray(z)
    return bool((z[np.abs(z).argmax(axis=0), np.arange(z.shape[1])] > 0.0).all())


def eigh_top(a, k):
    """(values (k,) descending, vectors (m, k), certificate (2,)) of one symmetric matrix."""
    a = np.asarray(a, dtype=np.float64)
    m = a.shape[0]
    if a.shape != (m, m) or not 1 <= m <= MAX_M or not 1 <= k <= min(m, MAX_K):
        raise ValueError(f"eigh_top: shape {a.shape}, k = {k}")
    d, e, tau, r = tridiagonalize(a)
    lam = top_eigenvalues(d, e, k)
    z = t_eigenvectors(d, e, lam)
    return lam, fix_signs(back_transform(r, tau, z)), certificate(d, e, lam, z)


# ---------------------------------------------------------------------------------------------------------------- cases
SIZES = (1, 2, 3, 17, 64, 65, 130)
BATCH = (130, 3, 65, 17, 2)                         # one call: the trailing launches are no-ops for the short slides
SPECTRA = ("spike", "flat", "rank30", "pairs", "close", "diag10")
GRAM_CASES = ("c346", "c613", "c250", "sep", "s150")
# cases whose k + 1 leading eigenvalues have relative gaps >= 1e-3: vectors are compared one by one
SEPARATED = ("spike", "flat") + tuple(f"m{m}" for m in SIZES)


def _from_spectrum(w, seed):
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((w.size, w.size)))[0]
    a = (q * w) @ q.T
    return 0.5 * (a + a.T)


def counts(m):
    return sorted({k for k in (1, 9, m - 1, min(m, MAX_K)) if 1 <= k <= min(m, MAX_K)})


def case_matrices():
    """name -> symmetric fp64 matrix.  m<size>: a well-separated spectrum at every size of SIZES; the hard spectra at
    m = 130 (diag10: a diagonal matrix with a 10-fold eigenvalue, so T is fully split); zero: rule (c)'s last line."""
    out = {}
    for m in SIZES:
        out[f"m{m}"] = _from_spectrum(np.arange(1.0, m + 1.0) + 0.25 * np.sin(np.arange(m)), 100 + m)   # gaps >= 0.5
    m = 130
    r = np.random.default_rng(7)
    out["spike"] = _from_spectrum(np.concatenate([[1e6], np.linspace(1.0, 2.0, m - 1)]), 1)
    out["flat"] = _from_spectrum(np.linspace(1.0, 1.5, m), 2)
    out["rank30"] = _from_spectrum(np.concatenate([r.uniform(1.0, 50.0, 30), np.zeros(m - 30)]), 3)
    out["pairs"] = _from_spectrum(np.concatenate([np.repeat(np.linspace(10.0, 40.0, 30), 2), r.uniform(0.0, 5.0, m - 60)]), 4)
    out["close"] = _from_spectrum(np.concatenate([5.0 + 1e-10 * np.arange(20), r.uniform(0.0, 4.0, m - 20)]), 5)
    out["diag10"] = np.diag(np.concatenate([np.full(10, 7.0), r.uniform(0.0, 6.0, m - 10)])[r.permutation(m)])
    out["zero"] = np.zeros((17, 17))
    return out


def pack(a):
    """The upper triangle of a symmetric matrix, row by row (how the fixture stores the case matrices)."""
    return a[np.triu_indices(a.shape[0])]


def unpack(t):
    m = int(round((np.sqrt(8.0 * t.size + 1.0) - 1.0) / 2.0))
    a = np.zeros((m, m))
    a[np.triu_indices(m)] = t
    return a + np.triu(a, 1).T


def stored_vectors(name, m):
    """The k whose vectors the fixture keeps for a case (values and certificates are kept for every k of ``counts``)."""
    return 9 if name in SPECTRA else min(m, MAX_K)


def gram_matrix(x):
    """The centred Gram matrix in its smaller form, as mcl_pca_gram writes it (up to rounding)."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(axis=0)
    return xc.T @ xc if x.shape[0] >= x.shape[1] else xc @ xc.T


def bounds(m, norm2):
    """(|d lambda|, residual, orthogonality) bounds of the method: 4 m eps |A|_2, 4 m eps |A|_2, 4 m eps."""
    return 4.0 * m * EPS * norm2, 4.0 * m * EPS * norm2, 4.0 * m * EPS


def errors(a, lam, z):
    """(max |d lambda|, max residual 2-norm, max |Z^T Z - I|, |A|_2, eigh's values descending, eigh's vectors)."""
    w, v = np.linalg.eigh(a)
    w, v = w[::-1], v[:, ::-1]
    k = lam.size
    res = np.sqrt(((a @ z - z * lam) ** 2).sum(axis=0)).max()
    return (np.abs(lam - w[:k]).max(), res, np.abs(z.T @ z - np.eye(k)).max(), max(abs(w[0]), abs(w[-1])), w, v)
