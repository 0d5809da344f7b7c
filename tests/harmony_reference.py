"""Plain-numpy restatement of the Harmony arithmetic of DESIGN 6.9 (what mclstexp_amd.harmony runs on the device), with
loops where harmonypy loops (blocks, clusters), in any floating dtype (float64, or np.longdouble for the error measurement).
Also the procedural cases of tests/golden/harmony.npz and the helpers the tests share.  No GPU, no mclstexp_amd import."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "harmony.npz")
LLOYD_ITERS = 25

# name -> N, d, batch probabilities, K, seed, run parameters
CASES = {
    "a": dict(N=611, d=37, probs=(0.5, 0.3, 0.2), K=20, seed=11, params={}),
    "b": dict(N=203, d=131, probs=(0.6, 0.4), K=7, seed=12, params={}),
    "c": dict(N=3000, d=70, probs=(0.4, 0.3, 0.2, 0.1), K=100, seed=13, params={}),
    "d": dict(N=305, d=16, probs=(1.0,), K=10, seed=14, params={}),
    "e": dict(N=611, d=37, probs=(0.5, 0.3, 0.2), K=20, seed=11, params=dict(max_iter_kmeans=5, max_iter_harmony=2)),
}
DEFAULTS = dict(theta=2.0, lamb=1.0, sigma=0.1, tau=0.0, block_size=0.05, max_iter_harmony=10, max_iter_kmeans=20,
                epsilon_cluster=1e-5, epsilon_harmony=1e-4)
QUANTITIES = ("Zc", "Y", "D", "R", "E", "O", "terms", "W", "Z_corr", "objective")


def make_case(name):
    """(Z (N, d) float64 non-negative, batch (N,) int32 interleaved and unsorted): log1p-like mixtures of a few cell types
    with an additive shift per batch."""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    N, d, B = c["N"], c["d"], len(c["probs"])
    types = 5
    profile = rng.gamma(2.0, 1.0, size=(types, d))
    cell_type = rng.randint(0, types, size=N)
    batch = rng.choice(B, size=N, p=np.asarray(c["probs"])).astype(np.int32)
    for b in range(B):                                   # every batch present
        batch[b] = b
    depth = rng.uniform(0.5, 2.0, size=(N, 1))
    counts = rng.poisson(profile[cell_type] * depth * 3.0)
    shift = np.abs(rng.normal(0.0, 0.4, size=(B, d)))
    Z = np.log1p(counts.astype(np.float64)) + shift[batch] + 0.05
    return Z, batch


def default_nclust(N):
    return int(min(np.round(N / 30.0), 100))


def block_bounds(N, nb):
    return np.concatenate([[0], np.cumsum([len(x) for x in np.array_split(np.arange(N), nb)])])


def draw_orders(random_state, N, count):
    """`count` successive np.random.shuffle(np.arange(N)) of the legacy stream."""
    rng = np.random.RandomState(random_state)
    out = []
    for _ in range(count):
        o = np.arange(N)
        rng.shuffle(o)
        out.append(o)
    return out


def normalize_rows(Z, by_max):
    if by_max:
        Z = Z / Z.max(axis=1, keepdims=True)
    return Z / np.sqrt((Z * Z).sum(axis=1, keepdims=True))


def lloyd(Zc, seed_rows, iters=LLOYD_ITERS):
    """Hard k-means on unit rows: argmax of Zc Y^T (ties: lowest centre), means, an emptied cluster keeps its centroid;
    the rows of the result are L2-normalised."""
    Y = Zc[np.asarray(seed_rows)].copy()
    K = Y.shape[0]
    for _ in range(iters):
        lab = np.argmax(Zc @ Y.T, axis=1)
        for k in range(K):
            m = lab == k
            if m.any():
                Y[k] = Zc[m].sum(axis=0) / m.sum()
    return normalize_rows(Y, False)


def gauss_jordan_inverse(A):
    """Inverse by Gauss-Jordan with partial pivoting (ties: the lowest row), in A's dtype."""
    n = A.shape[0]
    aug = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(aug[c:, c])))
        if p != c:
            aug[[c, p]] = aug[[p, c]]
        aug[c] = aug[c] / aug[c, c]
        for r in range(n):
            if r != c:
                aug[r] = aug[r] - aug[r, c] * aug[c]
    return aug[:, n:]


def softmax_scale(D, sigma):
    v = -D / sigma
    return np.exp(v - v.max(axis=1, keepdims=True))


def objective_terms(R, D, batch, E, O, theta, sigma):
    with np.errstate(divide="ignore", invalid="ignore"):
        x = R * np.log(R)
    x = np.where(np.isfinite(x), x, 0)
    t1 = (R * D).sum()
    t2 = sigma * x.sum()
    t3 = sigma * (R * (theta[batch][:, None] * np.log((O + 1) / (E + 1)).T[batch])).sum()
    return np.array([t1, t2, t3], dtype=R.dtype)


def update_block(R, S, batch, cells, E, O, theta, Pr, B):
    """Step 2d for one block, in place."""
    def sums():
        tot = R[cells].sum(axis=0)
        per = np.stack([R[cells][batch[cells] == b].sum(axis=0) for b in range(B)], axis=1)   # (K, B)
        return np.outer(tot, Pr), per
    e, o = sums()
    E -= e
    O -= o
    ratio = np.power((E + 1) / (O + 1), theta[None, :])          # (K, B)
    new = S[cells] * ratio.T[batch[cells]]
    R[cells] = new / np.abs(new).sum(axis=1, keepdims=True)
    e, o = sums()
    E += e
    O += o


def ridge_weights(R, O, Z_orig, batch, lamb, B, clusters=None):
    """W (K, B + 1, d) and M (K, B + 1, d)."""
    N, K = R.shape
    d = Z_orig.shape[1]
    W = np.zeros((K, B + 1, d), dtype=R.dtype)
    M = np.zeros((K, B + 1, d), dtype=R.dtype)
    for k in (range(K) if clusters is None else clusters):
        A = np.zeros((B + 1, B + 1), dtype=R.dtype)
        A[0, 0] = O[k].sum()
        for b in range(B):
            A[0, b + 1] = A[b + 1, 0] = O[k, b]
            A[b + 1, b + 1] = O[k, b] + lamb[b]
        M[k, 0] = R[:, k] @ Z_orig
        for b in range(B):
            m = batch == b
            M[k, b + 1] = R[m, k] @ Z_orig[m]
        W[k] = gauss_jordan_inverse(A) @ M[k]
        W[k, 0] = 0
    return W, M


def apply_correction(Z_orig, R, W, batch):
    Zc = Z_orig.copy()
    for k in range(R.shape[1]):
        Zc -= R[:, k:k + 1] * W[k][batch + 1]
    return Zc


def harmony(Z, batch, K, Y0, orders, *, theta=2.0, lamb=1.0, sigma=0.1, tau=0.0, block_size=0.05, max_iter_harmony=10,
            max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, dtype=np.float64, trace=False):
    """The whole run.  Y0 (K, d): initial centroids (L2-normalised here); orders: the permutations, consumed in order.
    Returns a dict: Z_corr, R, Y, objective_kmeans, objective_harmony, kmeans_rounds, converged, orders_used,
    tests (every convergence test: kind, left-hand side, epsilon), and with ``trace`` a list ``steps`` of dicts holding
    the state before and after every kernel-sized step of every k-means iteration, plus ``corrections``."""
    Z = np.asarray(Z, dtype=dtype)
    batch = np.asarray(batch)
    N, d = Z.shape
    B = int(batch.max()) + 1
    counts = np.bincount(batch, minlength=B)
    Pr = (counts / dtype(N)).astype(dtype)
    theta = np.full(B, theta, dtype=dtype) if np.ndim(theta) == 0 else np.asarray(theta, dtype=dtype)
    lamb = np.full(B, lamb, dtype=dtype) if np.ndim(lamb) == 0 else np.asarray(lamb, dtype=dtype)
    if tau > 0:
        theta = theta * (1 - np.exp(-(counts / (K * dtype(tau))) ** 2))
    sigma = dtype(sigma)
    nb = int(math.ceil(1.0 / block_size))
    bounds = block_bounds(N, nb)
    Zc = normalize_rows(Z, True)
    Zc0 = Zc.copy()
    Y = normalize_rows(np.asarray(Y0, dtype=dtype), False)
    D = 2 * (1 - Zc @ Y.T)
    R = softmax_scale(D, sigma)
    R = R / R.sum(axis=1, keepdims=True)
    E = np.outer(R.sum(axis=0), Pr)
    O = np.stack([R[batch == b].sum(axis=0) for b in range(B)], axis=1)
    terms0 = objective_terms(R, D, batch, E, O, theta, sigma)
    obj_k = [terms0.sum()]
    obj_h = [obj_k[0]]
    out = dict(Zc0=Zc0, Y_init=Y.copy(), D_init=D.copy(), R_init=R.copy(), E_init=E.copy(), O_init=O.copy(),
               terms_init=terms0, theta=theta, lamb=lamb, Pr=Pr)
    rounds, tests, steps, corrections = [], [], [], []
    used = 0
    converged = False
    Z_corr = Z.copy()
    for rnd in range(max_iter_harmony):
        i = 0
        for i in range(max_iter_kmeans):
            st = dict(round=rnd, iter=i, Zc=Zc.copy(), R_in=R.copy(), E_in=E.copy(), O_in=O.copy()) if trace else None
            Y = normalize_rows(R.T @ Zc, False)
            D = 2 * (1 - Zc @ Y.T)
            S = softmax_scale(D, sigma)
            order = np.asarray(orders[used])
            used += 1
            if trace:
                st.update(Y=Y.copy(), D=D.copy(), S=S.copy(), order=order.copy(), blocks={})
            for blk in range(nb):
                update_block(R, S, batch, order[bounds[blk]:bounds[blk + 1]], E, O, theta, Pr, B)
                if trace and blk in (0, 1, 2, nb - 2, nb - 1):
                    st["blocks"][blk] = dict(R=R.copy(), E=E.copy(), O=O.copy())
            terms = objective_terms(R, D, batch, E, O, theta, sigma)
            obj_k.append(terms.sum())
            if trace:
                st.update(R=R.copy(), E=E.copy(), O=O.copy(), terms=terms)
                steps.append(st)
            if i > 3:
                old = new = dtype(0)
                for j in range(3):
                    old += obj_k[-2 - j]
                    new += obj_k[-1 - j]
                lhs = abs(old - new) / abs(old)
                tests.append(("kmeans", float(lhs), epsilon_cluster))
                if lhs < epsilon_cluster:
                    break
        rounds.append(i)
        obj_h.append(obj_k[-1])
        W, M = ridge_weights(R, O, Z, batch, lamb, B)
        Z_corr = apply_correction(Z, R, W, batch)
        Zc = normalize_rows(Z_corr, False)
        if trace:
            corrections.append(dict(round=rnd, R=R.copy(), O=O.copy(), M=M, W=W, Z_corr=Z_corr.copy(), Zc=Zc.copy()))
        lhs = (obj_h[-2] - obj_h[-1]) / abs(obj_h[-2])
        tests.append(("harmony", float(lhs), epsilon_harmony))
        if lhs < epsilon_harmony:
            converged = True
            break
    out.update(Z_corr=Z_corr, R=R, Y=Y, objective_kmeans=np.array(obj_k, dtype=dtype),
               objective_harmony=np.array(obj_h, dtype=dtype), kmeans_rounds=np.array(rounds), converged=converged,
               orders_used=used, tests=tests, steps=steps, corrections=corrections)
    return out


def case_inputs(name, z=None):
    """Everything a replay of case `name` needs: Z, batch, K, params, and from the fixture `z` (np.load(GOLDEN)) Y0."""
    c = CASES[name]
    Z, batch = make_case(name)
    params = dict(DEFAULTS)
    params.update(c["params"])
    max_orders = params["max_iter_harmony"] * params["max_iter_kmeans"]
    src = "a" if name == "e" else name                  # e replays a's data and centroids under other caps
    Y0 = None if z is None else z[f"{src}_Y0"]
    return Z, batch, c["K"], params, Y0, draw_orders(0, c["N"], max_orders)


def run_case(name, z, dtype=np.float64, trace=False, Z=None):
    Z0, batch, K, params, Y0, orders = case_inputs(name, z)
    return harmony(Z0 if Z is None else Z, batch, K, Y0, orders, dtype=dtype, trace=trace, **params)


def slice_rows(N):
    """The ~24 evenly spaced rows of the N x K and N x d matrices that the fixture stores."""
    return np.arange(0, N, max(1, N // 24))


def stored_slices(name, r):
    """{key: array} of a traced run `r` of case `name`: what tests/golden/harmony.npz keeps of the first and last k-means
    iteration and of the first and last correction (see gen_harmony_goldens.py)."""
    rows = slice_rows(r["Z_corr"].shape[0])
    out = {}
    for tag, st in (("first", r["steps"][0]), ("last", r["steps"][-1])):
        for q in ("Y", "E", "O", "terms"):
            out[f"{name}_{tag}_{q}"] = st[q]
        out[f"{name}_{tag}_D"], out[f"{name}_{tag}_S"] = st["D"][rows], st["S"][rows]
        for blk in sorted(st["blocks"]):
            if blk in (0, 1, 2, max(st["blocks"])):
                out[f"{name}_{tag}_R_block{blk}"] = st["blocks"][blk]["R"][rows]
    for tag, c in (("corrfirst", r["corrections"][0]), ("corrlast", r["corrections"][-1])):
        out[f"{name}_{tag}_M"], out[f"{name}_{tag}_W"] = c["M"][:3], c["W"][:3]
        out[f"{name}_{tag}_Z_corr"] = c["Z_corr"][rows]
    return out
