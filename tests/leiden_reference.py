"""NumPy + scipy.sparse restatement of the deterministic Leiden DESIGN 6.13 states (csrc/leiden.hip), the yardstick of
tests/test_leiden_host.py and tests/test_leiden_gpu.py, and the case table.  Written from the statement; one slide at a time.

Weights are fixed point: q = rint(w 2^e), e = 61 - ex - ceil(log2(nnz)) with wmax < 2^ex (frexp), so every sum of weights is an
exact int64 (at most 2^61) and no order of summation matters.  Every floating-point value is one IEEE fp64 operation on
converted integers, in the order written here.  Where this statement and a leidenalg release differ, the statement holds."""
import os

import numpy as np
from scipy import sparse

import neighbors_reference as nr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leiden.npz")
MAX_LEVELS, MAX_SWEEPS, MAX_ITERATIONS = 32, 512, 64
NX_SEEDS = tuple(range(8))
# name -> resolutions run; the graphs come from case_graphs()
CASES = {"a": (1.0, 0.5, 2.0), "b": (1.0,), "d": (1.0,), "ring": (1.0,), "blobs": (1.0,), "star": (1.0,), "isolated": (1.0,),
         "twocomp": (1.0,), "empty": (1.0,)}
RESOLUTION_CASE = "a"
BOUNDED = ("a", "b", "d", "ring", "blobs", "star", "twocomp")        # cases with a recorded networkx Louvain bound
STAR_LEAVES = 600


def _knn_graph(X, k):
    idx, dist, _ = nr.knn(X, k)
    rho, sigma, _ = nr.smooth(dist)
    return nr.connectivities(idx, dist, rho, sigma)


def _cliques(sizes, first=0):
    """(rows, cols) of unit edges of disjoint cliques laid out from vertex ``first``."""
    r, c, o = [], [], first
    for n in sizes:
        i, j = np.nonzero(~np.eye(n, dtype=bool))
        r.append(i + o)
        c.append(j + o)
        o += n
    return np.concatenate(r), np.concatenate(c), o


def _sym(r, c, w, n):
    m = sparse.csr_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    m.sum_duplicates()
    m.sort_indices()
    return m


def case_graphs(name):
    """The scipy CSR matrices (float64, symmetric, no diagonal) of a case, one per slide."""
    if name in ("a", "b", "d"):
        X, off = nr.make_case(name), nr.offsets_of(name)
        return [_knn_graph(X[off[s]:off[s + 1]], nr.CASES[name][2]) for s in range(off.size - 1)]
    if name == "ring":                                   # 30 five-cliques, clique q joined to q + 1 by one unit edge
        r, c, n = _cliques([5] * 30)
        q = np.arange(30)
        r2, c2 = np.concatenate([r, 5 * q + 4, 5 * ((q + 1) % 30)]), np.concatenate([c, 5 * ((q + 1) % 30), 5 * q + 4])
        m = sparse.csr_matrix((np.ones(r2.size), (r2, c2)), shape=(n, n))
        m.sort_indices()
        return [m]
    if name == "blobs":                                  # 11 Gaussian blobs of unequal size in 6-D, k = 12
        rng = np.random.RandomState(3101)
        sizes = [5, 9, 14, 20, 27, 33, 41, 50, 58, 66, 77]
        X = np.concatenate([6.0 * rng.standard_normal(6) + rng.standard_normal((n, 6)) for n in sizes])
        return [_knn_graph(X, 12)]
    if name == "star":                                   # a hub with STAR_LEAVES leaves, four cliques hanging off leaves
        L = STAR_LEAVES
        r, c, n = _cliques([6, 7, 8, 9], first=L + 1)
        hub = np.zeros(L, dtype=np.int64)
        leaves = np.arange(1, L + 1)
        firsts = np.array([L + 1, L + 7, L + 14, L + 22])
        rr = np.concatenate([hub, np.array([1, 2, 3, 4])])
        cc = np.concatenate([leaves, firsts])
        w = np.concatenate([0.25 + 0.5 * ((leaves * 7) % 11) / 11.0, np.ones(4)])
        keep = r < c
        return [_sym(np.concatenate([rr, r[keep]]), np.concatenate([cc, c[keep]]), np.concatenate([w, np.ones(keep.sum())]), n)]
    if name == "isolated":                               # case a with five more vertices that have no edge
        m = case_graphs("a")[0].tocoo()
        return [sparse.csr_matrix((m.data, (m.row + 2, m.col + 2)), shape=(m.shape[0] + 5, m.shape[0] + 5))]
    if name == "twocomp":                                # two k = 8 graphs side by side, no edge between them
        rng = np.random.RandomState(3102)
        a, b = _knn_graph(rng.standard_normal((60, 4)), 8), _knn_graph(rng.standard_normal((45, 3)), 8)
        return [sparse.block_diag([a, b], format="csr")]
    if name == "empty":                                  # 2m = 0, next to a slide that has edges
        return [sparse.csr_matrix((7, 7), dtype=np.float64), case_graphs("ring")[0]]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------ arithmetic
def quantise(m):
    """(int64 CSR of q = rint(w 2^e) without zeros, e) of one slide's float64 CSR."""
    m = sparse.csr_matrix(m, dtype=np.float64)
    m.sort_indices()
    if m.nnz == 0:
        return sparse.csr_matrix(m.shape, dtype=np.int64), 0
    _, ex = np.frexp(m.data.max())
    e = 61 - int(ex) - int(m.nnz - 1).bit_length()
    q = sparse.csr_matrix((np.rint(np.ldexp(m.data, e)).astype(np.int64), m.indices.copy(), m.indptr.copy()), shape=m.shape)
    q.eliminate_zeros()
    return q, e


def _f(x):
    return np.asarray(x).astype(np.float64)


def _penalty(gamma, a, b, m2):
    """((gamma a) b) / 2m, each operation rounded once."""
    return ((np.float64(gamma) * _f(a)) * _f(b)) / np.float64(m2)


def fixed_sum(v):
    """The device's sum: partial t adds v[t], v[t + 256], .. in order; then p[t] += p[t + o] for o = 128, 64, .. 1."""
    v = _f(v)
    pad = np.zeros(-(-max(v.size, 1) // 256) * 256)
    pad[:v.size] = v
    p = np.zeros(256)
    for row in pad.reshape(-1, 256):
        p = p + row
    o = 128
    while o:
        p = p[:o] + p[o:2 * o]
        o //= 2
    return float(p[0])


def quality(A, k, labels, gamma, m2):
    """Q = in / 2m - gamma sum_c (tot_c / 2m)^2 over community ids 0 .. n - 1 in the fixed order; A holds self-loops."""
    if m2 == 0:
        return 0.0
    n = A.shape[0]
    coo = A.tocoo()
    inside = int(coo.data[labels[coo.row] == labels[coo.col]].sum())
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, labels, k)
    t = _f(tot) / np.float64(m2)
    return float(np.float64(inside) / np.float64(m2) - np.float64(gamma) * np.float64(fixed_sum(t * t)))


def modularity(m, labels, gamma=1.0):
    """Q of arbitrary labels on one slide's float64 graph, quantised as the device does, the communities taken in the order
    of their smallest member."""
    A, _ = quantise(m)
    k = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    return quality(A, k, canonical(labels), gamma, int(k.sum()))


class _Margins:
    def __init__(self):
        self.smallest = np.inf

    def note(self, diff, scale):
        diff, scale = np.abs(_f(diff)).ravel(), np.abs(_f(scale)).ravel()
        ok = diff > 0
        if ok.any():
            self.smallest = min(self.smallest, float((diff[ok] / np.maximum(scale[ok], 1e-300)).min()))


def _links(A, groups, mask=None):
    """coo (i, c, k_ic) of sum_j A_ij [groups_j = c] over j != i (and mask_ij where given)."""
    coo = A.tocoo()
    keep = coo.row != coo.col
    if mask is not None:
        keep &= mask(coo.row, coo.col)
    n = A.shape[0]
    K = sparse.csr_matrix((coo.data[keep], (coo.row[keep], groups[coo.col[keep]])), shape=(n, n))
    K.sum_duplicates()
    K = K.tocoo()
    return K.row, K.col, K.data.astype(np.int64)


def _best(n, i, c, gain, marg):
    """Per vertex the candidate of largest gain, ties to the smaller id: (target or -1, its gain)."""
    target, best = np.full(n, -1, dtype=np.int64), np.zeros(n)
    if i.size == 0:
        return target, best
    order = np.lexsort((c, -gain, i))
    i, c, gain = i[order], c[order], gain[order]
    first = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])
    second = first + 1
    has2 = (second < i.size)
    has2[has2] = i[second[has2]] == i[first[has2]]
    marg.note(gain[first[has2]] - gain[second[has2]], gain[first[has2]])
    target[i[first]], best[i[first]] = c[first], gain[first]
    return target, best


def sweep(A, k, P, tot, gamma, m2, parity, marg):
    """One Jacobi sweep of local moving: the new labels."""
    n = A.shape[0]
    i, c, kic = _links(A, P)
    own = c == P[i]
    kown = np.zeros(n, dtype=np.int64)
    kown[i[own]] = kic[own]
    stay = _f(kown) - _penalty(gamma, k, tot[P] - k, m2)
    i, c, kic = i[~own], c[~own], kic[~own]
    gain = _f(kic) - _penalty(gamma, k[i], tot[c], m2)
    target, best = _best(n, i, c, gain, marg)
    diff = best - stay
    has = target >= 0
    marg.note(diff[has], np.maximum(np.abs(best[has]), np.abs(stay[has])))
    move = has & (diff > 0) & ((target < P) if parity == 0 else (target > P))
    return np.where(move, target, P)


def _tally(k, labels):
    tot = np.zeros(k.size, dtype=np.int64)
    np.add.at(tot, labels, k)
    return tot


def move_phase(A, k, P, gamma, m2, st, marg, max_sweeps):
    tot, Q = _tally(k, P), quality(A, k, P, gamma, m2)
    parity = fails = done = accepted = 0
    while fails < 2:
        if done == max_sweeps:
            raise RuntimeError(f"local moving did not end within {max_sweeps} sweeps")
        new = sweep(A, k, P, tot, gamma, m2, parity, marg)
        Qn = quality(A, k, new, gamma, m2)
        marg.note(Qn - Q, Q)
        if Qn > Q:
            P, tot, Q, fails = new, _tally(k, new), Qn, 0
            accepted += 1
            st["trace"].append(Qn)
        else:
            fails += 1
        parity ^= 1
        done += 1
    st["sweeps"] += done
    st["accepted_sweeps"] += accepted
    return P, accepted


def refine_phase(A, k, P, gamma, m2, st, marg, max_sweeps):
    """The refined partition R of P: ids are founding vertices."""
    n = A.shape[0]
    R = np.arange(n, dtype=np.int64)
    totS = _tally(k, P)
    same = lambda r, c: P[r] == P[c]
    Q = quality(A, k, R, gamma, m2)
    rounds = 0
    st["refine_trace"].append([Q])
    while True:
        if rounds == max_sweeps:
            raise RuntimeError(f"refinement did not end within {max_sweeps} rounds")
        rounds += 1
        totR = _tally(k, R)
        size = np.bincount(R, minlength=n)
        i, c, kic = _links(A, R, same)
        ext = np.zeros(n, dtype=np.int64)
        np.add.at(ext, R[i], np.where(c != R[i], kic, 0))
        kS = np.zeros(n, dtype=np.int64)
        np.add.at(kS, i, kic)
        vertex_ok = (size[R] == 1) & (_f(kS) >= _penalty(gamma, k, totS[P] - k, m2))
        comm_ok = _f(ext) >= _penalty(gamma, totR, totS[P] - totR, m2)          # indexed by founder (P of founder = S)
        cand = vertex_ok[i] & (c != R[i]) & comm_ok[c] & ((size[c] > 1) | (c < R[i]))
        i, c, kic = i[cand], c[cand], kic[cand]
        gain = _f(kic) - _penalty(gamma, k[i], totR[c], m2)
        marg.note(gain, kic)
        pos = gain > 0
        target, _ = _best(n, i[pos], c[pos], gain[pos], marg)
        flagged = np.zeros(n, dtype=bool)
        flagged[target[target >= 0]] = True
        move = (target >= 0) & ~flagged
        new = np.where(move, target, R)
        Qn = quality(A, k, new, gamma, m2)
        marg.note(Qn - Q, Q)
        if not Qn > Q:
            break
        R, Q = new, Qn
        st["refine_trace"][-1].append(Qn)
    st["rounds"] += rounds
    return R


def aggregate(A, k, P, R):
    """Nodes = refined communities in order of id; (A', k', P', node_of)."""
    n = A.shape[0]
    ids = np.unique(R)
    node_of = np.searchsorted(ids, R)
    H = sparse.csr_matrix((np.ones(n, dtype=np.int64), (np.arange(n), node_of)), shape=(n, ids.size))
    A2 = sparse.csr_matrix(H.T @ A @ H).astype(np.int64)
    A2.eliminate_zeros()
    A2.sort_indices()
    k2 = np.zeros(ids.size, dtype=np.int64)
    np.add.at(k2, node_of, k)
    first = np.full(n, ids.size, dtype=np.int64)                 # per community of P the smallest node in it
    np.minimum.at(first, P, node_of)
    return A2, k2, first[P[ids]], node_of


def canonical(labels):
    """Every label replaced by the smallest index that carries it."""
    _, idx, inv = np.unique(np.asarray(labels), return_index=True, return_inverse=True)
    return idx[inv].astype(np.int64)


def by_size(labels):
    """Renumbered by descending size, ties to the smaller smallest member."""
    ids, idx, inv, cnt = np.unique(labels, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((idx, -cnt))
    rank = np.empty(ids.size, dtype=np.int64)
    rank[order] = np.arange(ids.size)
    return rank[inv].astype(np.int32)


def iteration(A0, k0, P0, gamma, m2, st, marg, max_levels, max_sweeps):
    """One pass over the levels from partition P0 (canonical ids): (labels per vertex, accepted sweeps)."""
    n0 = A0.shape[0]
    A, k, P, node = A0, k0, P0.copy(), np.arange(n0)
    total = 0
    for _ in range(max_levels):
        st["levels"] += 1
        P, acc = move_phase(A, k, P, gamma, m2, st, marg, max_sweeps)
        R = refine_phase(A, k, P, gamma, m2, st, marg, max_sweeps)
        total += acc
        A2, k2, P2, node_of = aggregate(A, k, P, R)
        merged = A2.shape[0] < A.shape[0]
        node = node_of[node]
        A, k, P = A2, k2, P2
        if acc == 0 and not merged:
            return canonical(P[node]), total
    raise RuntimeError(f"the levels did not end within {max_levels}")


def run(m, gamma=1.0, partition=None, n_iterations=-1, max_levels=MAX_LEVELS, max_sweeps=MAX_SWEEPS):
    """The whole run on one slide.  Returns labels, n_clusters, modularity, the counters, trace (Q after every accepted sweep,
    over all levels and iterations), refine_trace (per refinement: Q of the singletons, then Q after every accepted round)
    and margin (the smallest non-zero relative margin that decided anything)."""
    A, _ = quantise(m)
    n = A.shape[0]
    k = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    m2 = int(k.sum())
    st = {"levels": 0, "sweeps": 0, "accepted_sweeps": 0, "rounds": 0, "iterations": 0, "trace": [], "refine_trace": []}
    marg = _Margins()
    P = np.arange(n, dtype=np.int64) if partition is None else canonical(partition)
    if m2 > 0:
        while True:
            if st["iterations"] == MAX_ITERATIONS:
                raise RuntimeError("the iterations did not end")
            P, acc = iteration(A, k, P, gamma, m2, st, marg, max_levels, max_sweeps)
            st["iterations"] += 1
            if acc == 0 or st["iterations"] == n_iterations:
                break
    else:
        P = np.arange(n, dtype=np.int64)
    labels = by_size(P)
    st.update(labels=labels, n_clusters=int(labels.max()) + 1, modularity=quality(A, k, canonical(labels), gamma, m2),
              margin=marg.smallest)
    return st


def refine(m, partition, gamma=1.0):
    """The refinement of a given partition at level 0: canonical ids of the refined communities."""
    A, _ = quantise(m)
    k = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    m2 = int(k.sum())
    if m2 == 0:
        return np.arange(A.shape[0], dtype=np.int64)
    st = {"rounds": 0, "refine_trace": []}
    return canonical(refine_phase(A, k, canonical(partition), gamma, m2, st, _Margins(), MAX_SWEEPS))


def connected(m, labels):
    """Every community's subgraph is one component."""
    from scipy.sparse.csgraph import connected_components
    m = sparse.csr_matrix(m)
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)
        if connected_components(m[idx][:, idx], directed=False)[0] != 1:
            return False
    return True


def nx_modularity(m, labels, gamma=1.0):
    import networkx as nx
    g = nx.from_scipy_sparse_array(sparse.csr_matrix(m))
    comms = [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]
    return nx.community.modularity(g, comms, weight="weight", resolution=gamma)


def nx_louvain(m, gamma=1.0):
    """Q (networkx's) of networkx Louvain over NX_SEEDS."""
    import networkx as nx
    g = nx.from_scipy_sparse_array(sparse.csr_matrix(m))
    return np.array([nx.community.modularity(g, nx.community.louvain_communities(g, weight="weight", resolution=gamma, seed=s),
                                             weight="weight", resolution=gamma) for s in NX_SEEDS])
