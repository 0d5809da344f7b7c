"""numpy restatement of the neighbourhood enrichment and co-occurrence of spot groups (tests only), for the tests of
mclstexp_amd.nhood.

One slide at a time, line by line what DESIGN 6.20 states.  Every count is an integer, so the device must give these very
numbers whatever its schedule; the three stated roundings of z (one conversion each of the exact numerator and radicand, one
sqrt, one division) and of occ (three divisions) are taken here with Python integers and numpy's correctly rounded fp64, so
every comparison of the GPU tests is ``array_equal`` (NaN equal to NaN).

Pinned by tests/test_nhood_host.py (tests/golden/nhood.npz) to independent statements: the dense product L^T A L, a
``pandas.crosstab`` over the edge list, the same under the permuted label vector, a crosstab over
``scipy.spatial.distance.cdist`` and the occ formula in plain Python floats.  squidpy is not installed: parity with a release
is unpinned."""
import math
import os

import numpy as np

import ligrec_reference as lr
import spatial_reference as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nhood.npz")
EPS = 2.0 ** -52
LDS_BYTES, CELL_BYTES = 155648, 32      # csrc/nhood.hip: the dynamic LDS of the counting kernel, bytes per (c1, c2) cell
MAX_N, MAX_K, MAX_KW = 16384, 255, 64


# ------------------------------------------------------------------------------------------------------------ rules
def budget(n):
    """LDS left beside the two byte arrays (group of a spot, group of a sorted position) of a slide of n rows."""
    return LDS_BYTES - 2 * ((n + 15) // 16 * 16)


def tile_rows(n, K):
    """Source groups a workgroup takes for a slide of n rows and K groups."""
    return max(1, min(K, budget(n) // (CELL_BYTES * K)))


def staged(n, K, kw):
    """Does the slide's uint16 neighbour list sit in LDS beside labels and cells?"""
    return n * kw * 2 <= budget(n) - tile_rows(n, K) * K * CELL_BYTES


# ------------------------------------------------------------------------------------------------------------ cases
def make_stripes(gr=20, gc=17, stripes=4):
    """The gr x gc integer grid (x = column, y = row) with ``stripes`` vertical bands of equal labels."""
    yy, xx = np.meshgrid(np.arange(gr), np.arange(gc), indexing="ij")
    coords = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float64)
    labels = (xx.ravel() * stripes // gc).astype(np.int64)
    return coords, labels


def ring_list(n, kw):
    """The given list i + 1 .. i + kw (mod n), every weight 1."""
    nbr = ((np.arange(n)[:, None] + np.arange(1, kw + 1)[None, :]) % n).astype(np.int32)
    return nbr, np.ones((n, kw))


# -------------------------------------------------------------------------------------------------- neighbourhoods
def relabel(labels, order, start, perm=None):
    """The label vector under a permutation: the spot order[perm[j]] receives the group that owns position j; a dropped
    spot stays -1."""
    K = start.size - 1
    out = np.full(np.asarray(labels).size, -1, dtype=np.int64)
    owner = np.repeat(np.arange(K), np.diff(start))
    out[order if perm is None else order[np.asarray(perm)]] = owner
    return out


def counts(lab, nbr, w, K):
    """count[c1][c2] = #(spot i, slot c) with w != 0, the index inside the slide, both ends kept, lab[i] = c1 and
    lab[nbr] = c2; and the number of kept slots whose index lies outside the slide."""
    nbr, w = np.asarray(nbr), np.asarray(w, dtype=np.float64)
    n = nbr.shape[0]
    inside = (nbr >= 0) & (nbr < n)
    kept = w != 0
    j = np.where(inside, nbr, 0)
    li, lj = np.broadcast_to(np.asarray(lab)[:, None], nbr.shape), np.asarray(lab)[j]
    ok = kept & inside & (li >= 0) & (lj >= 0)
    c = np.zeros((K, K), dtype=np.int64)
    np.add.at(c, (li[ok], lj[ok]), 1)
    return c, int((kept & ~inside).sum())


def zscore(count, S1, S2, P):
    """z = (P count - S1) / sqrt(P S2 - S1^2): numerator and radicand exact (Python integers), one conversion each, one
    sqrt, one division; NaN where the radicand is 0."""
    z = np.full(count.shape, np.nan)
    for idx in np.ndindex(count.shape):
        num = P * int(count[idx]) - int(S1[idx])
        rad = P * int(S2[idx]) - int(S1[idx]) ** 2
        if rad != 0:
            z[idx] = float(num) / math.sqrt(float(rad))
    return z


def nhood(labels, nbr, w, k=None, n_perms=0, seed=0, perms=None):
    """Everything ``mclstexp_amd.nhood.nhood_enrichment`` returns for one slide (and ``sims`` (P, K, K), ``bad_index``)."""
    labels = np.asarray(labels)
    K = max(1, int(labels.max(initial=-1)) + 1 if k is None else int(k))
    order, start = lr.prepare(labels, K)
    n = order.size
    count, bad = counts(relabel(labels, order, start), nbr, w, K)
    if perms is None:
        perms = [sr.permutation(seed, p, n) for p in range(n_perms)] if n >= 2 else [np.arange(n)] * n_perms
    P = len(perms)
    out = {"count": count, "sizes": np.diff(start), "n": n, "k": K, "n_perms": P, "order": order, "start": start,
           "bad_index": bad}
    if not P:
        return out
    sims = np.stack([counts(relabel(labels, order, start, perm), nbr, w, K)[0] for perm in perms])
    if P * int(np.asarray(nbr).size) ** 2 < 2 ** 62:               # (int64 cannot overflow: a count is at most the slots)
        S1, S2 = sims.sum(axis=0).astype(object), (sims * sims).sum(axis=0).astype(object)
    else:
        S1, S2 = np.zeros((K, K), dtype=object), np.zeros((K, K), dtype=object)
        for sim in sims:
            S1 = S1 + sim.astype(object)
            S2 = S2 + sim.astype(object) ** 2
    n_ge, n_le = (sims >= count).sum(axis=0), (sims <= count).sum(axis=0)
    rad = np.array([[float(P * int(S2[a, b]) - int(S1[a, b]) ** 2) for b in range(K)] for a in range(K)]).reshape(K, K)
    out.update({"zscore": zscore(count, S1, S2, P), "perm_sum": S1.astype(np.int64), "perm_sumsq": S2.astype(np.int64),
                "perm_mean": S1.astype(np.float64) / float(P), "perm_std": np.sqrt(rad) / float(P), "n_ge": n_ge,
                "n_le": n_le, "pval_enriched": n_ge / float(P), "pval_depleted": n_le / float(P), "sims": sims,
                "permutations": np.stack(perms)})
    return out


def interaction_matrix(labels, nbr, w, k=None, normalized=False):
    c = nhood(labels, nbr, w, k)["count"]
    if not normalized:
        return c
    tot = c.sum(axis=1, keepdims=True).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(tot == 0.0, np.nan, c / tot)


def z_bound(count, sims):
    """The bound on |exact-integer z - numpy's two-pass (count - mean) / std|: (P + 8) eps ((|count| + |mean|) / std + |z|),
    from a P-term sum in mean and std and the cancellation in the numerator."""
    P = sims.shape[0]
    mean, std = sims.mean(axis=0), sims.std(axis=0)
    with np.errstate(all="ignore"):
        z = (count - mean) / std
        return z, (P + 8) * EPS * ((np.abs(count) + np.abs(mean)) / std + np.abs(z))


# ---------------------------------------------------------------------------------------------------- co-occurrence
def default_radii(coords_kept, T):
    """linspace(R / T, R, T), R half the diagonal of the bounding box of the kept spots; R = 1 when they have no extent."""
    c = np.asarray(coords_kept, dtype=np.float64).reshape(-1, 2)
    R = 0.0
    if c.shape[0]:
        d = c.max(axis=0) - c.min(axis=0)
        R = 0.5 * float(np.sqrt(d[0] * d[0] + d[1] * d[1]))
    if not R > 0.0:
        R = 1.0
    return np.linspace(R / float(T), R, T)


def pair_counts(coords, labels, K, radii, block=512):
    """pairs[t][c1][c2] = #ordered (i, j), i != j, both kept, with d2 <= r_t r_t; d2 = dx dx + dy dy, every product and the
    sum rounded separately.  A pair is binned into the first t that holds; the running sum over t is integer arithmetic."""
    labels = np.asarray(labels)
    order, start = lr.prepare(labels, K)
    c = np.asarray(coords).astype(np.float64)[order]
    g = labels[order].astype(np.int64)
    r = np.asarray(radii, dtype=np.float64)
    r2 = r * r
    T, n = r.size, order.size
    hist = np.zeros(T * K * K, dtype=np.int64)
    for a in range(0, n, block):
        dx = c[a:a + block, 0][:, None] - c[:, 0][None, :]
        dy = c[a:a + block, 1][:, None] - c[:, 1][None, :]
        d2 = dx * dx + dy * dy
        t = np.searchsorted(r2, d2.ravel(), side="left").reshape(d2.shape)       # the first t with d2 <= r2[t]
        ok = t < T
        ok[np.arange(d2.shape[0]), np.arange(a, a + d2.shape[0])] = False
        key = (t * K + g[a:a + block][:, None]) * K + g[None, :]
        hist += np.bincount(key[ok], minlength=T * K * K)
    return np.cumsum(hist.reshape(T, K, K), axis=0)


def occ_scores(pairs):
    """occ = (pairs / row) / (col / tot): three divisions, NaN where a denominator is 0."""
    p = pairs.astype(np.float64)
    row, col = p.sum(axis=2, keepdims=True), p.sum(axis=1, keepdims=True)
    tot = p.sum(axis=(1, 2), keepdims=True)
    with np.errstate(all="ignore"):
        occ = (p / row) / (col / tot)
    return np.where((row == 0) | (col == 0) | (tot == 0), np.nan, occ)


def co_occurrence(coords, labels, k=None, radii=50):
    """Everything ``mclstexp_amd.nhood.co_occurrence`` returns for one slide."""
    labels = np.asarray(labels)
    K = max(1, int(labels.max(initial=-1)) + 1 if k is None else int(k))
    c = np.asarray(coords).astype(np.float64)
    r = default_radii(c[labels >= 0], int(radii)) if isinstance(radii, (int, np.integer)) else np.asarray(radii, np.float64)
    pairs = pair_counts(c, labels, K, r)
    order, start = lr.prepare(labels, K)
    return {"pairs": pairs, "occ": occ_scores(pairs), "radii": r, "sizes": np.diff(start), "n": order.size, "k": K}


def grid_pairs(side, radius):
    """Ordered pairs within ``radius`` on the full side x side integer grid, in closed form: the sum over (dx, dy) != 0
    with dx^2 + dy^2 <= r^2 of (side - |dx|)(side - |dy|)."""
    m = int(math.floor(radius))
    tot = 0
    for dx in range(-m, m + 1):
        for dy in range(-m, m + 1):
            if (dx or dy) and dx * dx + dy * dy <= radius * radius:
                tot += (side - abs(dx)) * (side - abs(dy))
    return tot


# --------------------------------------------------------------------------------------------------------- recovery
def greedy_match(table):
    """Largest cell first, ties to the smaller (row, column), its row and column leave; cells of 0 are never matched."""
    t = np.array(table, dtype=np.int64)
    rows, cols, out = set(range(t.shape[0])), set(range(t.shape[1])), []
    while rows and cols:
        best = max(((t[r, c], -r, -c) for r in rows for c in cols))
        if best[0] <= 0:
            break
        r, c = -best[1], -best[2]
        out.append((r, c))
        rows.discard(r)
        cols.discard(c)
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def _pearson(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.corrcoef(a[ok], b[ok])[0, 1]) if ok.sum() >= 2 else float("nan")


def recovery(pred, true, rp, rt):
    """(matching, pearson_z, sign_agreement, pearson_occ, cells left out by the finite mask) of two label vectors and
    their results (dicts with ``zscore``, ``occ``, ``k``)."""
    pred, true = np.asarray(pred), np.asarray(true)
    table = np.zeros((rp["k"], rt["k"]), dtype=np.int64)
    for a, b in zip(pred, true):
        if a >= 0 and b >= 0:
            table[a, b] += 1
    match = greedy_match(table)
    p, t = match[:, 0], match[:, 1]
    zp, zt = rp["zscore"][np.ix_(p, p)], rt["zscore"][np.ix_(t, t)]
    ok = np.isfinite(zp) & np.isfinite(zt)
    sign = float((np.sign(zp[ok]) == np.sign(zt[ok])).mean()) if ok.any() else float("nan")
    with np.errstate(all="ignore"):
        op, ot = np.log2(rp["occ"][:, p][:, :, p]), np.log2(rt["occ"][:, t][:, :, t])
    return match, _pearson(zp, zt), sign, _pearson(op, ot), int((~ok).sum())
