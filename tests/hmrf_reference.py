"""NumPy restatement of the Potts-HMRF arithmetic DESIGN 6.18 states (csrc/hmrf.hip), in the kernel's summation orders: the
yardstick of tests/test_hmrf_host.py (against dense formulas, scipy and tests/mixture_reference.py, recorded in
tests/golden/hmrf.npz) and of tests/test_hmrf_gpu.py (against the device).

Orders restated on top of mixture_reference's (everything fp64, products and sums rounded separately):
  field f_ik = sum_c w_ic q[nbr_ic, k]        slots c ascending, one running sum from 0.0, pruned slots (w = 0) skipped
  v = g + (beta f)                            g the mixture's weighted log prob, beta f rounded first
  a = log w_k + (beta f), za its log-sum-exp  k ascending, the maximum subtracted, as lse
  lower bound / score                         block_sum(lse - za) / n
  q of the iteration before                   exp(log_resp), rounded once (what the M-step turns log_resp into)
  edge agreement                              per row the slots ascending, then block_sum over the rows
The fixtures of the issue (cases A .. I) are built here, seeded, so that the golden generator and both test files share them."""
import numpy as np

import mixture_reference as mr
import spatial_reference as sr

EPS = mr.EPS
BAD_INDEX = 4


# ----------------------------------------------------------------------------------------------------------- pieces
def field(nbr, w, q):
    """f (n, K): the running sum over the slots ascending; a slot with w = 0 or an index outside 0 .. n - 1 adds nothing.
    -> (f, bad): bad when a kept slot held such an index."""
    nbr, w, q = np.asarray(nbr), np.asarray(w, dtype=np.float64), np.asarray(q, dtype=np.float64)
    n = q.shape[0]
    f = np.zeros_like(q)
    bad = False
    for c in range(nbr.shape[1]):
        j = nbr[:, c]
        inside = (j >= 0) & (j < n)
        kept = w[:, c] != 0.0
        bad = bad or bool((kept & ~inside).any())
        term = w[:, c:c + 1] * q[np.where(inside, j, 0)]
        f = np.where((kept & inside)[:, None], f + term, f)
    return f, bad


def log_sum_exp(v):
    mx = v.max(axis=1)
    return mx + np.log(mr.seq_sum(np.exp(v - mx[:, None]), axis=1))


def estep(x, w, mu, pc, ctype, nbr, gw, q_prev, beta):
    """One E-step under given parameters and previous responsibilities -> dict: field, wlp (g), v, lse, za, log_resp, resp,
    labels, score, bad."""
    n = x.shape[0]
    f, bad = field(nbr, gw, q_prev)
    g = mr.estep(x, w, mu, pc, ctype)["wlp"]
    bf = beta * f
    v = g + bf
    lse = log_sum_exp(v)
    log_resp = v - lse[:, None]
    za = log_sum_exp(np.log(w)[None, :] + bf)
    return {"field": f, "wlp": g, "v": v, "lse": lse, "za": za, "log_resp": log_resp, "resp": np.exp(log_resp),
            "labels": np.argmax(log_resp, axis=1).astype(np.int32), "score": mr.block_sum(lse - za) / n, "bad": bad}


def fit(x, K, init_labels, nbr, gw, beta, ctype="full", tol=1e-3, max_iter=100, reg=1e-6):
    """The whole fit from one start -> dict (status 1: ill-defined covariance; bit 4: a bad neighbour index)."""
    n, D = x.shape
    q = (np.asarray(init_labels)[:, None] == np.arange(K)[None, :]).astype(np.float64)
    w, mu, cov, pc, failed = mr.mstep(x, q, reg, ctype, init=True)
    lb, it, conv, bounds, bad = -np.inf, 0, 0, [], False
    while not failed and it < max_iter:
        prev = lb
        e = estep(x, w, mu, pc, ctype, nbr, gw, q, beta)
        bad = bad or e["bad"]
        lb = e["score"]
        bounds.append(lb)
        q = e["resp"]
        w, mu, cov, pc, failed = mr.mstep(x, q, reg, ctype)
        it += 1
        if failed:
            break
        if abs(lb - prev) < tol:
            conv = 1
            break
    flag = BAD_INDEX if bad else 0
    if failed:
        return {"status": 1 | flag, "n_iter": it, "lower_bound": np.nan, "converged": 0}
    e = estep(x, w, mu, pc, ctype, nbr, gw, q, beta)
    p = mr.n_parameters(ctype, K, D)
    return {"status": flag, "n_iter": it, "converged": conv, "lower_bound": lb, "lower_bounds": np.array(bounds),
            "score": e["score"], "weights": w, "means": mu, "covariances": cov, "precisions_cholesky": pc,
            "labels": e["labels"], "resp": e["resp"], "log_resp": e["log_resp"], "lse": e["lse"], "za": e["za"],
            "field": e["field"],
            "bic": ((-2.0 * e["score"]) * n) + p * np.log(float(n)), "aic": ((-2.0 * e["score"]) * n) + 2.0 * p}


def refine(labels, nbr, w):
    """One synchronous round of majority relabelling -> (labels, changed)."""
    labels, nbr, w = np.asarray(labels), np.asarray(nbr), np.asarray(w)
    n = labels.size
    out = labels.copy()
    for i in range(n):
        l = labels[i]
        if l < 0:
            continue
        near = [labels[j] for j, wv in zip(nbr[i], w[i]) if wv != 0.0 and 0 <= j < n and labels[j] >= 0]
        m = len(near)
        pool = near + [l]
        own = pool.count(l)
        top = min(set(pool), key=lambda v: (-pool.count(v), v))
        if 2 * own < m and 2 * pool.count(top) > m:
            out[i] = top
    return out.astype(np.int32), int((out != labels).sum())


def edge_sums(labels, nbr, w):
    """(sum_i sum_c w_ic [l_i = l_nbr], sum_i sum_c w_ic) over the kept slots whose two labels are >= 0."""
    labels, nbr, w = np.asarray(labels), np.asarray(nbr), np.asarray(w, dtype=np.float64)
    n = labels.size
    a, t = np.zeros(n), np.zeros(n)
    for c in range(nbr.shape[1]):
        j = nbr[:, c]
        inside = (j >= 0) & (j < n)
        lj = labels[np.where(inside, j, 0)]
        kept = (w[:, c] != 0.0) & inside & (labels >= 0) & (lj >= 0)
        t = np.where(kept, t + w[:, c], t)
        a = np.where(kept & (lj == labels), a + w[:, c], a)
    return mr.block_sum(a), mr.block_sum(t)


def ari(a, b):
    """The adjusted Rand index of two labellings (Hubert and Arabie)."""
    a, b = np.asarray(a), np.asarray(b)
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    t = np.zeros((ua.size, ub.size))
    np.add.at(t, (ia, ib), 1)
    c2 = lambda v: v * (v - 1) / 2.0       # noqa: E731
    s, sa, sb, tot = c2(t).sum(), c2(t.sum(axis=1)).sum(), c2(t.sum(axis=0)).sum(), c2(float(a.size))
    exp = sa * sb / tot
    return float((s - exp) / (0.5 * (sa + sb) - exp))


# ---------------------------------------------------------------------------------------------------------- fixtures
def grid_coords(gr, gc, jitter=0.0, drop=0.0, seed=0):
    rng = np.random.default_rng([seed, gr, gc])
    yy, xx = np.meshgrid(np.arange(gr), np.arange(gc), indexing="ij")
    c = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float64)
    keep = rng.random(c.shape[0]) >= drop
    c = c[keep]
    return c + rng.uniform(-jitter, jitter, size=c.shape), keep


def blobs(truth, D, K, sep, noise, seed):
    rng = np.random.default_rng([seed, truth.size, D, K])
    centres = rng.standard_normal((K, D)) * sep
    return np.ascontiguousarray(centres[truth] + noise * rng.standard_normal((truth.size, D)))


def noisy_start(truth, K, frac, seed):
    rng = np.random.default_rng([seed, truth.size, K, 7])
    init = truth.copy()
    flip = rng.random(truth.size) < frac
    init[flip] = rng.integers(0, K, int(flip.sum()))
    init[:K] = np.arange(K)
    return init.astype(np.int32)


def kmeans_labels(x, K, seed, iters=20):
    """A plain Lloyd start for case B (host only; the device's k-means stream is not reproduced)."""
    rng = np.random.default_rng([seed, x.shape[0], K, 11])
    cen = x[rng.choice(x.shape[0], K, replace=False)]
    for _ in range(iters):
        lab = np.argmin(((x[:, None, :] - cen[None]) ** 2).sum(axis=2), axis=1)
        cen = np.array([x[lab == k].mean(axis=0) if (lab == k).any() else cen[k] for k in range(K)])
    return lab.astype(np.int32)


# name -> seed; chosen so that every full fit decides clearly (tests/test_hmrf_host.py checks the margins)
B_SEP = 1.3      # spread of the four stripe centres of case B (noise 2.2 per coordinate)
SEEDS = {"A": 3, "B": 5, "C": 0, "D": 0, "E": 0}
_CACHE = {}


def make_case(name, seed=None):
    """-> dict: x (n, D), K, init (n,), nbr, w, beta, types, truth (where planted).  ``seed``: another draw of the case."""
    seed = SEEDS.get(name, 0) if seed is None else seed
    if (name, seed) in _CACHE:
        return _CACHE[(name, seed)]
    if name == "A":                                   # 12 x 11 jittered grid: 132 = 8 x 16 + 4 spots
        coords, _ = grid_coords(12, 11, jitter=0.12, seed=seed)
        truth = np.minimum((coords[:, 0] / 3.7).astype(np.int64), 2).astype(np.int32)
        g = sr.lattice(coords, 8, "NA", row_standardise=False)
        c = {"x": blobs(truth, 2, 3, 2.5, 1.0, seed), "K": 3, "truth": truth, "init": noisy_start(truth, 3, 0.2, seed),
             "beta": 0.5, "types": mr.TYPES}
    elif name == "B":                                 # 20 x 17 grid, four planted stripes, noise 2.2 per coordinate
        coords, _ = grid_coords(20, 17, seed=seed)
        truth = np.minimum((coords[:, 0] / 4.25).astype(np.int64), 3).astype(np.int32)
        g = sr.lattice(coords, 8, "NA", row_standardise=False)
        x = blobs(truth, 9, 4, B_SEP, 2.2, seed)
        c = {"x": x, "K": 4, "truth": truth, "init": kmeans_labels(x, 4, seed), "beta": 1.0, "types": ("full",)}
    elif name == "C":                                 # 9 x 10 grid with dropped spots, STD pruning, row-standardised
        coords, _ = grid_coords(9, 10, jitter=0.1, drop=0.12, seed=seed)
        truth = ((coords[:, 0] > 4.5).astype(np.int64) + 2 * (coords[:, 1] > 4.0).astype(np.int64)).astype(np.int32)
        truth = np.where((coords[:, 0] < 2.0) & (coords[:, 1] < 2.5), 4, truth).astype(np.int32)
        g = sr.lattice(coords, 8, "STD", row_standardise=True)
        c = {"x": blobs(truth, 17, 5, 1.2, 1.0, seed), "K": 5, "truth": truth, "init": noisy_start(truth, 5, 0.15, seed),
             "beta": 6.0, "types": mr.TYPES}
    elif name == "D":                                 # the smallest slide
        coords = np.array([[0.0, 0.0], [1.0, 0.1], [2.0, 0.0], [5.0, 0.1], [6.0, 0.0], [7.0, 0.1]])
        truth = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
        g = sr.lattice(coords, 2, "NA", row_standardise=False)
        x = np.array([[0.1], [0.4], [-0.3], [3.2], [2.7], [3.5]])
        c = {"x": x, "K": 2, "truth": truth, "init": truth.copy(), "beta": 1.0, "types": ("full",)}
    elif name == "E":                                 # a given graph with rows of degree 0
        coords, _ = grid_coords(8, 9, jitter=0.1, seed=seed)
        truth = (coords[:, 1] > 3.5).astype(np.int32)
        g = sr.lattice(coords, 6, "NA", row_standardise=False)
        g = {"nbr": g["nbr"].copy(), "w": g["w"].copy()}
        g["w"][[0, 5, 17, 40, 71]] = 0.0
        g["w"][10:30, 3:] = 0.0
        c = {"x": blobs(truth, 3, 2, 2.0, 1.0, seed), "K": 2, "truth": truth, "init": noisy_start(truth, 2, 0.2, seed),
             "beta": 1.5, "types": ("full",)}
    else:
        raise KeyError(name)
    c.update(nbr=np.ascontiguousarray(g["nbr"], dtype=np.int32), w=np.ascontiguousarray(g["w"], dtype=np.float64),
             coords=coords, name=name)
    _CACHE[(name, seed)] = c
    return c


FIT_CASES = ("A", "B", "C", "D", "E")


def ref_fit(name, ctype, seed=None, **kw):
    c = make_case(name, seed)
    return fit(c["x"], c["K"], c["init"], c["nbr"], c["w"], kw.pop("beta", c["beta"]), ctype, **kw)


def teacher_case(name):
    """Parameters and previous responsibilities for one teacher-forced E-step -> dict: the case with ``params`` {type: (w, mu,
    pc, cov)} (A, C, G: the mixture's own fit from the case's start) and ``q`` (the full fit's responsibilities)."""
    if name in ("A", "C", "G"):
        c = dict(make_case("A" if name == "G" else name))
        if name == "G":
            c["beta"], c["types"] = 50.0, ("full",)
        c["params"] = {}
        for ctype in c["types"]:
            f = mr.fit(c["x"], c["K"], c["init"], ctype)
            c["params"][ctype] = (f["weights"], f["means"], f["precisions_cholesky"], f["covariances"])
            c["q"] = f["resp"] if ctype == "full" else c.get("q")
        return c
    if name == "F":                                   # the largest D and K: n = 1024, D = K = 64, no fit
        rng = np.random.default_rng(64)
        n, D, K = 1024, 64, 64
        coords, _ = grid_coords(32, 32, jitter=0.1, seed=5)
        g = sr.lattice(coords, 8, "NA", row_standardise=False)
        truth = rng.integers(0, K, n)
        mu = rng.standard_normal((K, D)) * 1.5
        x = np.ascontiguousarray(mu[truth] + rng.standard_normal((n, D)))
        pc = np.empty((K, D, D))
        for k in range(K):
            a = np.eye(D) + 0.05 * rng.standard_normal((D, D))
            pc[k] = mr.precision_cholesky(a @ a.T)[0]
        w = rng.random(K) + 0.5
        w = w / w.sum()
        q = rng.random((n, K)) ** 4
        q = q / q.sum(axis=1, keepdims=True)
        return {"x": x, "K": K, "nbr": g["nbr"].astype(np.int32), "w": g["w"], "beta": 1.0, "types": ("full",),
                "params": {"full": (w, mu, pc, None)}, "q": q, "name": "F"}
    raise KeyError(name)


def label_case(name):
    """Labels for the refine / agreement tests on the graph of case ``name``: the planted domains with a quarter of the
    spots relabelled at random (one of them to a label no other spot has) and every eleventh spot without a label."""
    c = make_case(name)
    rng = np.random.default_rng([SEEDS[name], 13])
    lab = c["truth"].astype(np.int32).copy()
    flip = rng.random(lab.size) < 0.25
    lab[flip] = rng.integers(0, c["K"], int(flip.sum()))
    lab[4] = 1000
    lab[::11] = -1
    return lab


def checksum(c):
    x = c["x"]
    return np.array([x.sum(), np.abs(x).sum(), x[0, 0], x[-1, -1], float(c["init"].sum()), float(c["nbr"].sum()),
                     float(c["w"].sum())])


def make_h():
    """Case H: case A from a start in which component 2 owns one spot; with reg_covar = 0 its covariance is singular."""
    c = dict(make_case("A"))
    init = np.where(c["init"] == 2, 0, c["init"]).astype(np.int32)
    init[7] = 2
    c.update(init=init, name="H", types=("full",))
    return c
