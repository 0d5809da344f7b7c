"""CPU: the numpy restatement of DESIGN 6.11 (tests/neighbors_reference.py) on the cases of tests/golden/neighbors.npz, the
fixture's own invariants, and the host side of mclstexp_amd.neighbors (argument rules, to_scipy, CLI, the C entry points'
argument errors).  Fails where mclstexp_amd.neighbors does not exist."""
import numpy as np
import pytest
import torch

import neighbors_reference as nr
from mclstexp_amd import neighbors


@pytest.fixture(scope="module")
def z():
    return np.load(nr.GOLDEN)


@pytest.fixture(scope="module")
def ref(z):
    return {name: nr.segments(name, z[f"{name}_X"]) for name in nr.CASES}


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_lists_start_with_self_and_ascend(z, ref, name):
    off, k = nr.offsets_of(name), nr.CASES[name][2]
    for s, g in enumerate(ref[name]):
        n = off[s + 1] - off[s]
        idx, dist = g["knn_indices"], g["knn_distances"]
        assert idx.shape == (n, k) and idx.dtype == np.int32
        assert np.array_equal(idx[:, 0], np.arange(n)) and not dist[:, 0].any()
        assert (np.diff(dist[:, 1:], axis=1) >= 0).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        d2 = nr.sq_distances(z[f"{name}_X"][off[s]:off[s + 1]])
        assert np.array_equal(np.take_along_axis(d2, idx.astype(np.int64), axis=1)[:, 1:], g["d2"][:, 1:])
        # nothing left out is nearer than the last one kept
        left = d2.copy()
        np.put_along_axis(left, idx.astype(np.int64), np.inf, axis=1)
        assert (left.min(axis=1) >= g["d2"][:, -1]).all() or k == n


def test_ties_go_to_the_smaller_index(ref):
    g = ref["d"][0]
    idx, d2 = g["knn_indices"], g["d2"]
    tied = d2[:, 1:-1] == d2[:, 2:]
    assert tied.sum() > 100                                             # the case is made of ties
    assert (idx[:, 1:-1][tied] < idx[:, 2:][tied]).all()
    full = nr.sq_distances(nr.make_case("d"))
    cut = 0
    for i in range(idx.shape[0]):                                        # a tie across the k-th place keeps the smaller
        out = np.setdiff1d(np.flatnonzero(full[i] == d2[i, -1]), idx[i])
        if out.size:
            cut += 1
            assert out.min() > idx[i, 1:][d2[i, 1:] == d2[i, -1]].max()
    assert cut > 50
    assert not g["rho"][:11].any() and (g["rho"][11:] > 0).any()         # the rows of the repeated point


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_connectivities_are_a_symmetric_fuzzy_union(ref, name):
    k = nr.CASES[name][2]
    for g in ref[name]:
        m = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"])
        assert (m != m.T).nnz == 0 and not m.diagonal().any() and m.has_sorted_indices
        assert m.data.min() > 0 and m.data.max() <= 1
        assert np.array_equal(m.toarray(), g["dense"])
        w = nr.directed_weights(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"])
        plain = g["info"]["stopped"] & ~g["info"]["floored"]
        assert plain.sum() >= 0.9 * plain.size or name == "d"      # d: rows full of ties at rho never meet the target
        assert np.max(np.abs(w[plain].sum(axis=1) - np.log2(k))) < 1e-5 + 1e-12
        # the intersection (mix 0) keeps the mutual edges only
        inter = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"], 0.0)
        assert inter.nnz <= m.nnz and (inter != inter.T).nnz == 0


def test_fixture_invariants(z, ref):
    for name, (sizes, D, k) in nr.CASES.items():
        assert z[f"{name}_X"].shape == (sum(sizes), D) and z[f"{name}_X"].dtype == np.float64
        assert np.array_equal(z[f"{name}_X"], nr.make_case(name))
        for q in ("rho", "sigma", "data"):
            assert 2.0 ** -53 <= float(z[f"err_{name}_{q}"]) <= 1e-12, (name, q)
        assert float(z[f"margin_{name}"]) >= 1e-9
        assert z[f"{name}_rho_agree"].shape == (sum(sizes),) and z[f"{name}_rho_agree"].mean() > 0.25
        assert min(g["info"]["margin"] for g in ref[name]) >= 1e-9
        if name in nr.RANDOM:
            assert 0.0 <= float(z[f"sklearn_skipped_{name}"]) < 0.01
    assert nr.CASES["b"][0][1] == nr.CASES["b"][2] + 1
    X = z["d_X"]
    assert np.array_equal(X, np.round(X)) and (X[:11] == X[0]).all()


# ------------------------------------------------------------------------------------------------------ host rules
def test_argument_errors():
    X = np.random.RandomState(0).rand(40, 6)
    with pytest.raises(ValueError, match=r"n_neighbors must lie in 2 \.\. 256"):
        neighbors.neighbors(X, n_neighbors=1)
    with pytest.raises(ValueError, match=r"n_neighbors must lie in 2 \.\. 256"):
        neighbors.knn(np.zeros((300, 3)), n_neighbors=257)
    with pytest.raises(ValueError, match="n_neighbors must be an integer"):
        neighbors.knn(X, n_neighbors=15.0)
    with pytest.raises(ValueError, match="n_neighbors = 41 counts the row itself and needs at least 41 rows"):
        neighbors.neighbors(X, n_neighbors=41)
    with pytest.raises(ValueError, match="needs at least 15 rows in every segment"):
        neighbors.neighbors(X, offsets=[0, 30, 40], n_neighbors=15)
    with pytest.raises(ValueError, match="x has 65 columns"):
        neighbors.knn(np.zeros((40, 65)))
    with pytest.raises(ValueError, match="2-D"):
        neighbors.knn(np.zeros(40))
    with pytest.raises(ValueError, match=r"2 \.\. 16384 rows"):
        neighbors.knn(np.zeros((16385, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="offsets must run from 0"):
        neighbors.neighbors(X, offsets=[0, 20, 39])
    with pytest.raises(ValueError, match=r"set_op_mix_ratio must lie in 0 \.\. 1"):
        neighbors.neighbors(X, set_op_mix_ratio=1.5)
    with pytest.raises(ValueError, match=r"knn_distances: expected a 2-D"):
        neighbors.smooth(np.zeros(40))
    with pytest.raises(ValueError, match=r"knn_distances: expected shape \(40, 15\)"):
        neighbors.connectivities(np.zeros((40, 15), dtype=np.int32), np.zeros((40, 14)), np.zeros(40), np.zeros(40))
    with pytest.raises(ValueError, match=r"rho: expected shape \(40,\)"):
        neighbors.connectivities(np.zeros((40, 15), dtype=np.int32), np.zeros((40, 15)), np.zeros(39), np.zeros(40))
    with pytest.raises(ValueError, match="gene_stats normalises"):
        neighbors.expression_graph(np.ones((40, 30), dtype=np.float32), preprocess=True, normalize_and_log=False)
    with pytest.raises(ValueError, match="expr: expected a 2-D"):
        neighbors.expression_graph(np.ones(40, dtype=np.float32))
    with pytest.raises(ValueError, match="needs at least 150 rows"):
        neighbors.expression_graph(np.ones((40, 30), dtype=np.float32))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised without a GPU")
def test_no_gpu_error_names_the_module():
    X = np.random.RandomState(0).rand(40, 6)
    for call in (lambda: neighbors.neighbors(X), lambda: neighbors.knn(X), lambda: neighbors.smooth(np.zeros((40, 15))),
                 lambda: neighbors.expression_graph(X.astype(np.float32), preprocess=False, n_pcs=3, n_neighbors=10),
                 lambda: neighbors.expression_graph(np.ones((40, 30), dtype=np.float32), n_top_genes=8, n_pcs=3,
                                                    n_neighbors=10)):
        with pytest.raises(RuntimeError, match=r"mclstexp_amd\.(neighbors|cluster|preprocess): no GPU available"):
            call()


def test_to_scipy_round_trip(ref):
    """Two segments of case b as a result dict on the host: to_scipy gives back the restatement's matrices."""
    gs = ref["b"][:2]
    ms = [nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"]) for g in gs]
    off = np.array([0, 257, 408])
    res = {"knn_indices": np.concatenate([g["knn_indices"] for g in gs]),
           "knn_distances": torch.from_numpy(np.concatenate([g["knn_distances"] for g in gs])),
           "indptr": np.concatenate([m.indptr.astype(np.int64) for m in ms]),
           "indices": np.concatenate([m.indices for m in ms]), "data": np.concatenate([m.data for m in ms]),
           "offsets": off, "nnz_offsets": np.array([0, ms[0].nnz, ms[0].nnz + ms[1].nnz])}
    for s in range(2):
        d, c = neighbors.to_scipy(res, s)
        assert (c != ms[s]).nnz == 0 and c.shape == ms[s].shape and c.has_sorted_indices
        want = nr.distances_matrix(gs[s]["knn_indices"], gs[s]["knn_distances"])
        assert (d != want).nnz == 0 and d.nnz == (off[s + 1] - off[s]) * 149
    with pytest.raises(ValueError, match="segment must lie in 0 .. 1"):
        neighbors.to_scipy(res, 2)
    # zero distances are not stored (scanpy's eliminate_zeros)
    g = ref["d"][0]
    m = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"])
    one = {"knn_indices": g["knn_indices"], "knn_distances": g["knn_distances"], "indptr": m.indptr.astype(np.int64),
           "indices": m.indices, "data": m.data, "offsets": np.array([0, 130]), "nnz_offsets": np.array([0, m.nnz])}
    d, c = neighbors.to_scipy(one, 0)
    assert d.nnz == int((g["knn_distances"] > 0).sum()) < 130 * 9 and d[0].nnz == 0 and c[0].nnz >= 10


def test_cli_parsing():
    a = neighbors.parse_args(["--pred", "1.npy", "2.npy", "--raw", "--n_neighbors", "20", "--out_dir", "o"])
    assert a.pred == ["1.npy", "2.npy"] and a.raw and a.n_neighbors == 20 and a.n_pcs == 50 and a.out_dir == "o"
    assert a.n_top_genes == 1024
    b = neighbors.parse_args(["--pred", "1.npy"])
    assert not b.raw and b.n_neighbors == 150 and b.out_dir == "."
    for bad in (["--pred", "1.npy", "--n_neighbors", "1"], ["--pred", "1.npy", "--n_neighbors", "257"],
                ["--pred", "1.npy", "--n_pcs", "65"], ["--n_neighbors", "5"]):
        with pytest.raises(SystemExit):
            neighbors.parse_args(bad)


def test_capi_symbols_and_argument_errors_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_abi_version() == 13 == _lib.ABI_VERSION
    for s in ("mcl_knn_workspace_bytes", "mcl_knn_exact", "mcl_knn_smooth", "mcl_knn_connectivities"):
        assert s in _lib.PROTOTYPES and hasattr(lib, s)
    assert _lib._RESTYPES["mcl_knn_workspace_bytes"] is _lib.C.c_int64
    assert lib.mcl_knn_workspace_bytes(9269, 150) >= 9269 * 150 * 12 + 9269 * 12
    assert lib.mcl_knn_workspace_bytes(0, 15) == 0 and lib.mcl_knn_workspace_bytes(10, 257) == 0
    one = _lib.C.c_void_p(8)
    # null pointers
    assert lib.mcl_knn_exact(None, 5, 1, 5, None, 1, 70, 70, 70, 15, None, None, None) == -1
    assert lib.mcl_knn_smooth(None, None, 1, 70, 70, 70, 15, None, None, None, None) == -1
    assert lib.mcl_knn_connectivities(None, None, None, None, None, 1, 70, 70, 70, 15, 1.0, 0, None, None, None, None, 0,
                                      None, None, None) == -1
    # out-of-range arguments are refused before any launch, whatever the pointers
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 1, 70, 70, 70, 1, one, one, None) == -1          # k < 2
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 1, 70, 70, 70, 71, one, one, None) == -1         # k > n_s
    assert lib.mcl_knn_exact(one, 4, 1, 5, one, 1, 70, 70, 70, 15, one, one, None) == -1         # ld < D
    assert lib.mcl_knn_exact(one, 5, 2, 5, one, 1, 70, 70, 70, 15, one, one, None) == -1         # dtype
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 1, 70, 71, 70, 15, one, one, None) == -1         # min_n > max_n
    assert lib.mcl_knn_exact(one, 65, 1, 65, one, 1, 70, 70, 70, 15, one, one, None) == -2       # D > 64
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 1, 300, 300, 300, 257, one, one, None) == -2     # k > 256
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 1, 16385, 16385, 16385, 15, one, one, None) == -2
    assert lib.mcl_knn_exact(one, 5, 1, 5, one, 65536, 65536 * 20, 20, 20, 15, one, one, None) == -2
    assert lib.mcl_knn_smooth(one, one, 1, 70, 70, 70, 1, one, one, one, None) == -1
    assert lib.mcl_knn_smooth(one, one, 1, 70, 70, 70, 257, one, one, one, None) == -2
    assert lib.mcl_knn_smooth(one, one, 2, 70, 40, 40, 15, one, one, one, None) == -1            # rows < S min_n
    assert lib.mcl_knn_connectivities(one, one, one, one, one, 1, 70, 70, 70, 15, 1.5, 0, one, one, one, None, 0, None,
                                      None, None) == -1                                         # mix ratio
    assert lib.mcl_knn_connectivities(one, one, one, one, one, 1, 70, 70, 70, 15, 1.0, 2, one, one, one, None, 0, None,
                                      None, None) == -1                                         # phase
    assert lib.mcl_knn_connectivities(one, one, one, one, one, 1, 70, 70, 70, 15, 1.0, 1, one, one, None, None, 0, None,
                                      None, None) == -1                                         # phase 1 without outputs
    assert lib.mcl_knn_connectivities(one, one, one, one, one, 1, 70, 70, 70, 15, 1.0, 0, one, one, None, None, 0, None,
                                      None, None) == -1                                         # phase 0 without nnz
    assert lib.mcl_knn_connectivities(one, one, one, one, one, 1, 16385, 16385, 16385, 15, 1.0, 0, one, one, one, None, 0,
                                      None, None, None) == -2
