"""fp64 numpy restatement of the ligand-receptor permutation test (tests only), for the tests of mclstexp_amd.ligrec.

One slide at a time, line by line what DESIGN 6.19 states, INCLUDING the kernel's summation order: the sum of a group over
a segment of m spots is ``segment_sum`` (lane l of 64 adds the values at segment positions l, l + 64, ... ascending, starting
from 0; the lanes are combined by the halving tree p[l] += p[l + o], o = 32, 16, ... 1), a function of m alone.  With
correctly rounded + and / on both sides every group sum and mean is therefore the device's own number; the GPU tests still
only assume the first-order bound they derive where the data are not quantised.

Pinned by tests/test_ligrec_host.py (tests/golden/ligrec.npz) to an independent statement: the permutation applied to the
label vector itself, pandas ``groupby`` means and counts, a plain Python loop over the pairs, and
``scipy.stats.false_discovery_control``.  squidpy, omnipath and CellPhoneDB are not installed: parity with a release of
any of them is unpinned."""
import itertools
import os

import numpy as np

import spatial_reference as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ligrec.npz")
LANES = 64
EPS = 2.0 ** -52
X_BYTES, CMAX = 155648, 8          # csrc/ligrec.hip: LDS for the gathered columns, columns per workgroup
G = 12
# 9 interactions over the 12 genes of ``make_slide``: a_i = b_i, a duplicated pair, the gene that is zero everywhere (11),
# the gene expressed in exactly threshold * size spots of group 0 (10), and two complexes
INTERACTIONS = [(0, 1), (2, 3), (4, 4), (0, 1), (5, 11), (10, 6), ((7, 8), 9), (3, (1, 2)), (6, 0)]


# ------------------------------------------------------------------------------------------------------------ cases
def make_labels(n, K, rng, drop=0.1, empty=None, single=None):
    """n labels in -1 .. K - 1: about ``drop`` of them -1, group ``empty`` without a spot, group ``single`` with one, and
    (K >= 2, n >= 30) group 0 with exactly 20 spots, so that 0.1 * size is the integer 2 in fp64."""
    nd = int(round(drop * n)) if n > 2 * K + 2 else 0
    fixed = {}
    if K >= 2 and n >= 30:
        fixed[0] = 20
    if single is not None:
        fixed[single] = 1
    if empty is not None:
        fixed[empty] = 0
    free = [c for c in range(K) if c not in fixed]
    left = n - nd - sum(fixed.values())
    sizes = np.zeros(K, dtype=np.int64)
    for c, v in fixed.items():
        sizes[c] = v
    assert free and left >= len(free), (n, K)
    sizes[free] = 1 + rng.multinomial(left - len(free), np.ones(len(free)) / len(free))
    lab = np.concatenate([np.repeat(np.arange(K), sizes), np.full(nd, -1)]).astype(np.int64)
    rng.shuffle(lab)
    return lab


def make_expression(labels, rng, quantised=True, dtype=np.float64, genes=G):
    """(n, genes) values >= 0: sparse gamma counts with a group pattern; the last gene is zero everywhere, the one before
    it is positive in exactly a tenth of the spots of group 0 (when that is an integer).  ``quantised``: multiples of 2^-12
    below 16: every sum of at most 16384 of them is exact in fp64 in any order, and every value is exact in fp32."""
    n = labels.size
    x = rng.gamma(2.0, 1.0, (n, genes)) * (rng.random((n, genes)) < 0.6)
    x = x * (1.0 + 0.5 * ((labels[:, None] % 3) == (np.arange(genes)[None, :] % 3)))
    x = np.minimum(x, 15.9)
    x[:, genes - 1] = 0.0
    g0 = np.flatnonzero(labels == 0)
    if g0.size and g0.size % 10 == 0:
        x[g0, genes - 2] = 0.0
        x[g0[:g0.size // 10], genes - 2] = 1.5
    if quantised:
        x = np.floor(x * 4096.0) / 4096.0
    return np.ascontiguousarray(x.astype(dtype))


def make_slide(n, K, seed, quantised=True, dtype=np.float64, drop=0.1, empty=None, single=None):
    rng = np.random.default_rng(seed)
    labels = make_labels(n, K, rng, drop, empty, single)
    return make_expression(labels, rng, quantised, dtype), labels


PLANTED = [(0, 1), (1, 0), (2, 3), (4, 5), (6, 7), (0, 0), (1, 1)]


def make_planted(seed, n=200, genes=8):
    """Two groups of n / 2 spots: gene 0 ("A") is high in group 0, gene 1 ("B") in group 1, the other genes are noise."""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(2), n // 2).astype(np.int64)
    rng.shuffle(labels)
    x = rng.gamma(2.0, 0.5, (n, genes))
    x[labels == 0, 0] += 3.0
    x[labels == 1, 1] += 3.0
    return np.ascontiguousarray(np.floor(x * 4096.0) / 4096.0), labels


# ------------------------------------------------------------------------------------------------------------ order
def segment_sum(v):
    """The sum over axis 0 of a segment in the kernel's fixed order."""
    v = np.asarray(v, dtype=np.float64)
    m = v.shape[0]
    blocks = -(-m // LANES)
    pad = np.zeros((max(blocks, 1) * LANES,) + v.shape[1:])
    pad[:m] = v
    acc = np.zeros((LANES,) + v.shape[1:])
    for b in range(blocks):
        acc = acc + pad[b * LANES:(b + 1) * LANES]
    h = LANES // 2
    while h:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def chain(m):
    """The longest addition chain a value of a segment of m spots travels through: its lane's chain and six tree levels."""
    return -(-m // LANES) + 6


def columns(n):
    """Used gene columns a workgroup takes for a slide of n kept spots."""
    c = X_BYTES // (8 * max(n, 1))
    return 8 if c >= 8 else 4 if c >= 4 else 2 if c >= 2 else 1


# ------------------------------------------------------------------------------------------------------- statistics
def prepare(labels, k):
    """order: the kept spots in the stable order by (label, spot); start (k + 1,): group c owns order[start[c]:start[c+1]]."""
    labels = np.asarray(labels)
    kept = np.flatnonzero(labels >= 0)
    order = kept[np.argsort(labels[kept], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(labels[kept], minlength=k))]).astype(np.int64)
    return order, start


def used_columns(sides):
    return np.unique(np.array([g for s in sides for t in s for g in t], dtype=np.int64))


def expand(interactions, policy="min"):
    """The sides after the policy: tuples of gene columns; ``"all"`` expands the product of two complexes."""
    sides = []
    for a, b in interactions:
        sa = tuple(sorted(set(a))) if isinstance(a, (tuple, list)) else (int(a),)
        sb = tuple(sorted(set(b))) if isinstance(b, (tuple, list)) else (int(b),)
        if policy == "all":
            sides.extend(((u,), (v,)) for u, v in itertools.product(sa, sb))
        else:
            sides.append((sa, sb))
    return sides


def group_stats(xs, start, perm=None):
    """sum, nnz (K, U) of the (label, spot)-sorted columns ``xs`` (n, U): group c receives the rows perm[start[c]:start[c+1]]."""
    xp = xs if perm is None else xs[np.asarray(perm)]
    K = start.size - 1
    sums = np.stack([segment_sum(xp[start[c]:start[c + 1]]) for c in range(K)])
    nnz = np.stack([(xp[start[c]:start[c + 1]] > 0).sum(axis=0) for c in range(K)]).astype(np.int64)
    return sums, nnz


def group_means(sums, start):
    size = np.diff(start).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        return sums / size


def choose(sides, used, sums, n):
    """(I, 2) positions in ``used``: of a complex the member of lowest mean over the kept spots (the group sums added in
    ascending group order, / n), ties to the smaller column."""
    tot = np.zeros(sums.shape[1])
    for c in range(sums.shape[0]):
        tot = tot + sums[c]
    with np.errstate(all="ignore"):
        mall = tot / float(n)
    out = np.zeros((len(sides), 2), dtype=np.int64)
    for i, side in enumerate(sides):
        for t, members in enumerate(side):
            pos = np.searchsorted(used, np.asarray(members))
            best = pos[0]
            for u in pos[1:]:
                if mall[u] < mall[best]:
                    best = u
            out[i, t] = best
    return out


def bh(p):
    """Benjamini-Hochberg over the finite entries; NaN stays NaN."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    ok = np.flatnonzero(np.isfinite(p))
    if ok.size:
        q = p[ok]
        o = np.argsort(q, kind="stable")
        scaled = q[o] * (float(ok.size) / np.arange(1, ok.size + 1).astype(np.float64))
        adj = np.empty(ok.size)
        adj[o] = np.minimum(1.0, np.minimum.accumulate(scaled[::-1])[::-1])
        out[ok] = adj
    return out


def adjust(pvalues, corr_axis):
    I, K = pvalues.shape[0], pvalues.shape[1]
    if corr_axis is None:
        return np.full(pvalues.shape, np.nan)
    flat = pvalues.reshape(I, K * K)
    if corr_axis == "clusters":
        return np.stack([bh(r) for r in flat]).reshape(pvalues.shape)
    return np.stack([bh(c) for c in flat.T], axis=1).reshape(pvalues.shape)


def ligrec(x, labels, interactions, k=None, n_perms=0, seed=0, threshold=0.1, perms=None, corr_axis="clusters",
           complex_policy="min"):
    """Everything ``mclstexp_amd.ligrec.ligrec`` returns for one slide."""
    labels = np.asarray(labels)
    K = int(labels.max(initial=-1)) + 1 if k is None else int(k)
    K = max(K, 1)
    sides = expand(interactions, complex_policy)
    used = used_columns(sides)
    order, start = prepare(labels, K)
    n = order.size
    xs = np.asarray(x).astype(np.float64)[order][:, used]
    sums, nnz = group_stats(xs, start)
    mean = group_means(sums, start)
    size = np.diff(start)
    with np.errstate(all="ignore"):
        frac = nnz / size.astype(np.float64)[:, None]
    expressed = nnz >= threshold * size.astype(np.float64)[:, None]
    pairs = choose(sides, used, sums, n)
    ia, ib = pairs[:, 0], pairs[:, 1]
    m1, m2 = mean[:, ia].T[:, :, None], mean[:, ib].T[:, None, :]           # (I, K, 1), (I, 1, K)
    with np.errstate(invalid="ignore"):
        pos = (m1 > 0) & (m2 > 0)
        obs = (m1 + m2) / 2.0
    means = np.where(np.isnan(obs), np.nan, np.where(pos, obs, 0.0))
    defined = pos & expressed[:, ia].T[:, :, None] & expressed[:, ib].T[:, None, :]
    if perms is None:
        perms = [sr.permutation(seed, p, n) for p in range(n_perms)] if n >= 2 else [np.arange(n)] * n_perms
    P = len(perms)
    count = np.zeros(means.shape, dtype=np.int32)
    for perm in perms:
        ps, _ = group_stats(xs, start, perm)
        pm = group_means(ps, start)
        with np.errstate(invalid="ignore"):
            count += (pm[:, ia].T[:, :, None] + pm[:, ib].T[:, None, :]) / 2.0 >= obs
    with np.errstate(all="ignore"):
        pvalues = np.where(defined, count / float(P), np.nan) if P else np.full(means.shape, np.nan)
    return {"means": means, "pvalues": pvalues, "pvalues_adj": adjust(pvalues, corr_axis), "defined": defined, "count": count,
            "group_means": mean, "group_frac": frac, "sum": sums, "nnz": nnz, "expressed": expressed, "sizes": size,
            "order": order, "start": start, "used_genes": used, "interactions": used[pairs], "n": n, "k": K, "n_perms": P,
            "permutations": np.stack(perms) if P else np.zeros((0, n), dtype=np.int64)}


# --------------------------------------------------------------------------------------------------------- recovery
def significant(r, alpha, adjusted):
    p = r["pvalues_adj"] if adjusted else r["pvalues"]
    with np.errstate(invalid="ignore"):
        return np.isfinite(p) & (p < alpha)


def recovery(rp, rt, alpha=0.05, adjusted=True):
    """(Pearson r of the means over the entries defined in both, overlap, Jaccard, precision, recall) of two results."""
    both = rp["defined"] & rt["defined"]
    r = float(np.corrcoef(rp["means"][both], rt["means"][both])[0, 1]) if both.sum() >= 2 else float("nan")
    a, b = significant(rp, alpha, adjusted), significant(rt, alpha, adjusted)
    o, u = int((a & b).sum()), int((a | b).sum())
    return (r, o, o / u if u else float("nan"), o / int(a.sum()) if a.any() else float("nan"),
            o / int(b.sum()) if b.any() else float("nan"))


def top_interactions(r, n):
    rows = [(r["pvalues"][idx], -r["means"][idx], idx) for idx in np.ndindex(r["pvalues"].shape) if np.isfinite(r["pvalues"][idx])]
    rows.sort()
    return np.array([idx for _, _, idx in rows[:n]], dtype=np.int64).reshape(-1, 3)
