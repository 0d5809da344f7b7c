"""CPU: the restatement of the deterministic Leiden (tests/leiden_reference.py) against networkx and against its recorded
runs (tests/golden/leiden.npz), the invariants of those runs, and the host side of mclstexp_amd.leiden: argument errors
before the device, the CLI's parsing, the C entry points' argument checks and their prototypes."""
import os

import numpy as np
import pytest
from scipy import sparse

import leiden_reference as lr
from mclstexp_amd import _lib, leiden, umap

RUNS = [(name, s, g) for name, gs in lr.CASES.items() for s in range(2 if name == "empty" else 3 if name == "b" else 1) for g in gs]


@pytest.fixture(scope="module")
def z():
    return np.load(lr.GOLDEN)


@pytest.fixture(scope="module")
def graphs():
    return {name: lr.case_graphs(name) for name in lr.CASES}


def key(name, s, g):
    return f"{name}_{s}_{g}_"


def test_case_table_is_what_the_fixture_holds(z, graphs):
    assert sorted(key(*r) + "labels" for r in RUNS) == sorted(k for k in z.files if k.endswith("_labels"))
    assert graphs["b"][0].shape[0] == 257 and len(graphs["b"]) == 3 and graphs["star"][0].shape[0] == lr.STAR_LEAVES + 31
    assert int(np.diff(graphs["star"][0].indptr).max()) == lr.STAR_LEAVES > leiden.CUT          # the dense path's row
    assert graphs["empty"][0].nnz == 0 and (np.diff(graphs["isolated"][0].indptr) == 0).sum() == 5
    from scipy.sparse.csgraph import connected_components
    assert connected_components(graphs["twocomp"][0], directed=False)[0] == 2


@pytest.mark.parametrize("name,s,g", RUNS)
def test_restatement_gives_the_recorded_run(z, graphs, name, s, g):
    r, k = lr.run(graphs[name][s], g), key(name, s, g)
    assert np.array_equal(r["labels"], z[k + "labels"]) and r["labels"].dtype == np.int32
    for field in ("n_clusters", "levels", "sweeps", "accepted_sweeps", "rounds", "iterations"):
        assert int(r[field]) == int(z[k + field]), field
    assert r["modularity"] == float(z[k + "modularity"]) == lr.modularity(graphs[name][s], r["labels"], g)
    assert np.array_equal(np.asarray(r["trace"]), z[k + "trace"])


@pytest.mark.parametrize("name,s,g", RUNS)
def test_modularity_agrees_with_networkx(z, graphs, name, s, g):
    pytest.importorskip("networkx")
    m, k = graphs[name][s], key(name, s, g)
    if m.nnz == 0:
        assert float(z[k + "modularity"]) == 0.0
        return
    labels = z[k + "labels"]
    nxq = lr.nx_modularity(m, labels, g)
    assert abs(lr.modularity(m, labels, g) - nxq) <= 1e-12 and abs(float(z[k + "nx_modularity"]) - nxq) <= 1e-12
    rng = np.random.RandomState(5)                            # and on labels that are no optimum
    other = rng.randint(0, 4, size=m.shape[0])
    assert abs(lr.modularity(m, other, g) - lr.nx_modularity(m, other, g)) <= 1e-12


@pytest.mark.parametrize("name,s,g", RUNS)
def test_fixture_invariants(z, graphs, name, s, g):
    m, k = graphs[name][s], key(name, s, g)
    labels = z[k + "labels"]
    trace = z[k + "trace"]
    assert (np.diff(trace) > 0).all()                         # every accepted sweep raised Q
    rt = z[k + "refine_trace"]
    starts = np.flatnonzero(np.isnan(rt))
    for a, b in zip(starts, np.r_[starts[1:], rt.size]):
        assert (np.diff(rt[a + 1:b]) > 0).all()               # every accepted round raised Q
    assert int(z[k + "accepted_sweeps"]) == trace.size and int(z[k + "sweeps"]) >= trace.size
    assert lr.connected(m, labels)
    sizes = np.bincount(labels)
    assert sizes.size == int(z[k + "n_clusters"]) and (np.diff(sizes) <= 0).all() and sizes.min() >= 1
    first = np.array([np.flatnonzero(labels == c)[0] for c in range(sizes.size)])
    assert all(first[c] < first[c + 1] for c in range(sizes.size - 1) if sizes[c] == sizes[c + 1])
    assert float(z[k + "margin"]) >= 1e-10
    if name in lr.BOUNDED:
        lou = z[k + "louvain"]
        assert lou.size == len(lr.NX_SEEDS) >= 8
        assert float(z[k + "modularity"]) >= lou.min() - (lou.max() - lou.min())


def test_clusters_do_not_fall_with_the_resolution(z):
    counts = z["clusters_by_resolution"]
    assert counts.tolist() == [int(z[key(lr.RESOLUTION_CASE, 0, g) + "n_clusters"]) for g in sorted(lr.CASES[lr.RESOLUTION_CASE])]
    assert (np.diff(counts) >= 0).all() and counts[-1] > counts[0]


def test_refinement_parts_what_has_no_edge_between_it():
    """Two cliques with no edge between them in one community: the restatement's refinement returns them apart."""
    r, c, n = lr._cliques([5, 6])
    m = sparse.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    ref = lr.refine(m, np.zeros(n, dtype=np.int64))
    assert ref.tolist() == [0] * 5 + [5] * 6


def test_quantisation_cannot_overflow():
    """The largest sum of q the scaling admits: nnz entries of the largest weight stay at or below 2^61."""
    for wmax in (1.0, 0.999, 1e-300, 1.7e308, 3.0):
        for nnz in (1, 2, 3, 1000, 16384 * 16383):
            _, ex = np.frexp(wmax)
            e = 61 - int(ex) - int(nnz - 1).bit_length()
            assert int(np.rint(np.ldexp(wmax, e))) * nnz <= 2 ** 61


# ------------------------------------------------------------------------------------------------- mclstexp_amd.leiden
def test_argument_errors_come_before_the_device(graphs, monkeypatch):
    g = umap.from_scipy(graphs["a"])
    monkeypatch.setattr(leiden, "device", lambda who: pytest.fail("the device was touched"))
    n = graphs["a"][0].shape[0]
    for kw in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=float("nan")), dict(resolution=float("inf")),
               dict(resolution=True), dict(resolution="1"), dict(n_iterations=0), dict(n_iterations=-2), dict(n_iterations=True),
               dict(n_iterations=2.0), dict(partition=np.zeros(n - 1, dtype=np.int64)), dict(partition=np.zeros(n)),
               dict(partition=np.zeros((n, 1), dtype=np.int64)), dict(partition=np.zeros(n, dtype=bool)),
               dict(partition=-np.ones(n, dtype=np.int64)), dict(max_levels=0), dict(max_sweeps=True)):
        with pytest.raises(ValueError):
            leiden.leiden(g, **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        leiden.leiden(g, theta=0.1)
    with pytest.raises(TypeError, match=r"unexpected keyword arguments \['theta'\]"):
        leiden.cluster(np.zeros((10, 3)), None, 5, theta=0.1)
    with pytest.raises(TypeError, match="unexpected keyword"):
        leiden.expression_clusters(np.zeros((10, 30)), theta=0.1)
    with pytest.raises(ValueError):
        leiden.cluster(np.zeros((10, 3)), None, 5, resolution=0.0)
    with pytest.raises(ValueError):
        leiden.modularity(g, np.zeros(n - 1, dtype=np.int64))
    with pytest.raises(ValueError):
        leiden.refine(g, np.zeros(n, dtype=np.int64), resolution=-1.0)
    with pytest.raises(ValueError, match="no 'indptr'"):
        leiden.leiden({"indices": 0})


def test_no_gpu_error_names_the_module(graphs, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.leiden: no GPU available"):
        leiden.leiden(umap.from_scipy(graphs["a"]))


def test_canonical_ids():
    off = np.array([0, 4, 9])
    got = leiden.canonical(np.array([7, 3, 7, 3, 5, 5, 0, 0, 5]), off)
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 0, 1, 0, 0, 2, 2, 0]
    assert np.array_equal(lr.canonical(np.array([7, 3, 7, 3])), got[:4])


def test_cli_parsing():
    a = leiden.parse_args(["--pred", "a.npy", "b.npy", "--out_dir", "out"])
    assert (a.pred, a.raw, a.n_neighbors, a.n_pcs, a.resolution, a.n_iterations, a.umap) == (["a.npy", "b.npy"], False, 150, 50,
                                                                                             1.0, -1, False)
    a = leiden.parse_args(["--pred", "a.npy", "--raw", "--n_neighbors", "20", "--n_pcs", "10", "--resolution", "0.5", "--umap",
                           "--out_dir", "o"])
    assert a.raw and a.umap and (a.n_neighbors, a.n_pcs, a.resolution) == (20, 10, 0.5)
    for bad in (["--resolution", "0"], ["--resolution", "nan"], ["--n_neighbors", "1"], ["--n_pcs", "1"], ["--n_iterations", "0"]):
        with pytest.raises(SystemExit):
            leiden.parse_args(["--pred", "a.npy", "--out_dir", "o", *bad])
    with pytest.raises(SystemExit):
        leiden.parse_args(["--pred", "a.npy"])


NAMES = ("mcl_leiden_workspace_bytes", "mcl_leiden_init", "mcl_leiden_move_sweeps", "mcl_leiden_refine_rounds",
         "mcl_leiden_aggregate", "mcl_leiden_finish")


def test_header_and_prototypes_agree_for_the_new_names():
    from test_capi_symbols import header_prototypes, table_prototypes
    want, have = header_prototypes(), table_prototypes(_lib.PROTOTYPES, _lib._RESTYPES)
    for name in NAMES:
        assert want[name] == have[name], name
        assert "stream" not in want[name][1][:-1]
        assert want[name][1][-1] == "stream" or name == NAMES[0]      # the five launching names take the stream last
    assert want[NAMES[0]] == ("i64", ["i64", "i64", "i32", "i32"])
    assert _lib._SIGNATURES["mcl_leiden_init"][2] is True     # call() appends torch's current stream


def test_abi_and_argument_errors_without_gpu():
    from mclstexp_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert lib.mcl_abi_version() == _lib.ABI_VERSION == 13
    assert lib.mcl_leiden_workspace_bytes(1000, 50000, 2, 600) > 50000 * 8 and lib.mcl_leiden_workspace_bytes(0, 0, 1, 5) < 0
    assert lib.mcl_leiden_workspace_bytes(10, 0, 1, 16385) < 0 and lib.mcl_leiden_workspace_bytes(10, 0, 65536, 5) < 0
    p = 0x1000                                                # never dereferenced: the checks fail first
    g = (p, p, p, p, 1, 10, 10, 0)
    assert lib.mcl_leiden_init(None, None, None, None, None, 1, 10, 10, 0, 1.0, None, None, None, None) == -1
    assert lib.mcl_leiden_init(p, p, None, p, p, 1, 10, 10, 0, 1.0, None, None, p, None) == -1            # no data
    assert lib.mcl_leiden_init(p, p, p, p, p, 1, 10, 10, 0, 0.0, None, None, p, None) == -1               # resolution
    assert lib.mcl_leiden_init(p, p, p, p, p, 1, 10, 10, 0, 1.0, None, None, p + 4, None) == -1           # alignment
    assert lib.mcl_leiden_init(p, p, p, p, p, 1, 20000, 20000, 0, 1.0, None, None, p, None) == -2         # n_s > 16384
    assert lib.mcl_leiden_move_sweeps(1, 0, 10, 0, 5, *g, float("nan"), p, None) == -1
    assert lib.mcl_leiden_move_sweeps(-1, 0, 10, 0, 5, *g, 1.0, p, None) == -1
    assert lib.mcl_leiden_move_sweeps(1, 0, 11, 0, 5, *g, 1.0, p, None) == -1                             # n_cur > max_n
    assert lib.mcl_leiden_refine_rounds(1, 1, 0, 10, 0, 0, *g, 1.0, p, None) == -1                        # max_rounds
    assert lib.mcl_leiden_aggregate(-1, 10, 4, *g, 1.0, p, None) == -1
    assert lib.mcl_leiden_finish(2, 0, None, *g, p, p, None, None, None) == -1                            # source
    assert lib.mcl_leiden_finish(0, 1, None, *g, p, p, None, None, None) == -1                            # no labels
    with pytest.raises(RuntimeError, match="mcl_leiden_workspace_bytes rejected"):
        _lib.call("mcl_leiden_workspace_bytes", 0, 0, 1, 5)
