"""CPU: the numpy restatement of DESIGN 6.12 (tests/umap_reference.py) -- its generator against known answers, its
schedule, the fixture's own invariants -- and the host side of mclstexp_amd.umap (argument rules raised before a device is
touched, find_ab_params, from_scipy, CLI, the declarations and argument errors of the C entry points).  Fails where
mclstexp_amd.umap does not exist."""
import os
import re

import numpy as np
import pytest
import torch

import umap_reference as ur
from conftest import ROOT
from mclstexp_amd import umap

SYMBOLS = ("mcl_umap_workspace_bytes", "mcl_umap_prepare", "mcl_umap_init", "mcl_umap_epochs")


@pytest.fixture(scope="module")
def z():
    return np.load(ur.GOLDEN)


def _ring(n=40):
    """A symmetric ring graph as a scipy CSR."""
    from scipy import sparse
    i = np.arange(n)
    m = sparse.csr_matrix((np.ones(n), (i, (i + 1) % n)), shape=(n, n))
    return (m + m.T).tocsr()


# ------------------------------------------------------------------------------------------------- the restatement
def test_mix_known_answers():
    for x, want in ur.MIX_VECTORS:
        assert ur.mix_int(x) == want and int(ur.mix(x)[0]) == want
    for h, n, want in ur.K_VECTORS:
        assert ((h >> 32) * n) >> 32 == want == int(ur.sample_index(np.uint64(h), n))
    # the sample of (seed, epoch, i, r, p) is the five nested steps
    h = ur.mix_int(ur.mix_int(ur.mix_int(ur.mix_int(ur.mix_int(77) ^ 3) ^ 12) ^ 5) ^ 2)
    assert int(ur.negative_samples(77, 3, [12], [5], [2], 151)[0]) == ((h >> 32) * 151) >> 32
    y = ur.random_init(5, 9)
    h = ur.mix_int(ur.mix_int(ur.mix_int(9 ^ ur.MASK) ^ 4) ^ 1)
    assert y[4, 1] == 20.0 * ((h >> 11) * 2.0 ** -53) - 10.0 and (np.abs(y) <= 10).all()


def test_schedule_and_pruning():
    w = np.array([1.0, 0.5, 0.026, 0.024, 0.3])
    live, eps, epn = ur.schedule(w, 40, 5)
    assert live.tolist() == [True, True, True, False, True]             # 1 / 40 = 0.025
    assert np.array_equal(eps, 1.0 / w) and np.array_equal(epn, eps / 5.0)
    g = ur.case_graphs("a")[0]
    r = ur.run(g, ur.case_start("a"), 30, 0.583, 1.334, 1, keep=(1, 30))
    again = ur.run(g, ur.case_start("a"), 30, 0.583, 1.334, 1)
    assert np.array_equal(r["Y"], again["Y"]) and np.array_equal(r["Y"], r["trace"][30])
    assert r["attractive_samples"] > 0 and r["negative_samples"] > 3 * r["attractive_samples"]
    none = ur.run(g, ur.case_start("a"), 30, 0.583, 1.334, 1, rate=0)
    assert none["negative_samples"] == 0 and none["attractive_samples"] == r["attractive_samples"]
    assert np.array_equal(ur.pca_init(np.array([[1.0, -4.0, 9.0], [2.0, 0.5, 9.0]])), [[2.5, -10.0], [5.0, 1.25]])


def test_fixture_invariants(z):
    assert abs(float(z["a"]) - 0.5830300) < 1e-6 and abs(float(z["b"]) - 1.3341670) < 1e-6
    for name in ur.TRAJECTORY:
        X, sizes, _ = ur.case_input(name)
        assert np.array_equal(z[f"{name}_X"], X) and np.array_equal(z[f"{name}_Y0"], ur.case_start(name))
        L = int(z[f"{name}_trajectory_len"])
        assert 1 <= L <= min(ur.MAX_TRAJECTORY, ur.CASES[name][3])
        assert 2.0 ** -53 <= float(z[f"err_{name}_Y1"]) <= 1e-12
        assert 2.0 ** -53 <= float(z[f"err_{name}_Y{L}"]) <= 1e-6
    X = z["d_X"]
    assert (X[:11] == X[0]).all() and (z["d_Y0"][:11] == z["d_Y0"][0]).all()     # coincident start points
    assert np.array_equal(z["e_X"], ur.case_input("e")[0]) and z["e_X"].shape == (151, 50)
    jac, seq = z["e_trust_jacobi"], z["e_trust_sequential"]
    assert jac.shape == seq.shape == (len(ur.FULL_SEEDS),) and (z["e_purity"][:, 0] == 1.0).all()
    assert jac.min() >= seq.min() - (seq.max() - seq.min())
    assert os.path.getsize(ur.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(ur.GOLDEN), "neighbors.npz"))


# ------------------------------------------------------------------------------------------------------ host rules
def test_find_ab_params():
    a, b = umap.find_ab_params(1.0, 0.5)
    assert abs(a - 0.5830300) < 1e-6 and abs(b - 1.3341670) < 1e-6
    assert umap.find_ab_params() == (a, b) == ur.find_ab_params()


def test_argument_errors_come_before_the_device():
    g = umap.from_scipy([_ring(40)])
    x = np.random.RandomState(0).rand(40, 6)
    ab = dict(a=0.58, b=1.33)
    with pytest.raises(ValueError, match="init must be one of 'pca', 'random' or a .rows, 2. array.*spectral start is not"):
        umap.layout(g, init="spectral", x=x, **ab)
    with pytest.raises(ValueError, match="init must be one of"):
        umap.umap(x, n_neighbors=10, init="spectral")
    with pytest.raises(ValueError, match=r"n_epochs must lie in 1 \.\. 5000"):
        umap.layout(g, x=x, n_epochs=0, **ab)
    with pytest.raises(ValueError, match=r"n_epochs must lie in 1 \.\. 5000"):
        umap.layout(g, x=x, n_epochs=5001, **ab)
    with pytest.raises(ValueError, match="n_epochs must be an integer"):
        umap.umap(x, n_neighbors=10, n_epochs=10.0)
    with pytest.raises(ValueError, match=r"negative_sample_rate must be an integer in 0 \.\. 64"):
        umap.layout(g, x=x, negative_sample_rate=65, **ab)
    with pytest.raises(ValueError, match="negative_sample_rate"):
        umap.layout(g, x=x, negative_sample_rate=-1, **ab)
    for bad in (dict(a=float("nan"), b=1.3), dict(a=0.5, b=float("inf")), dict(a=0.5, b=1.3, gamma=float("inf")),
                dict(a=0.5, b=1.3, alpha=float("nan"))):
        with pytest.raises(ValueError, match="must be finite"):
            umap.layout(g, x=x, **bad)
    with pytest.raises(ValueError, match="a must be positive"):
        umap.layout(g, x=x, a=0.0, b=1.3)
    with pytest.raises(ValueError, match="b must be positive"):
        umap.expression_umap(np.ones((200, 30), dtype=np.float32), a=0.5, b=-1.0)
    with pytest.raises(ValueError, match="give both a and b"):
        umap.layout(g, x=x, a=0.5)
    with pytest.raises(ValueError, match="seed must be an integer"):
        umap.layout(g, x=x, seed=1.5, **ab)
    with pytest.raises(ValueError, match="init='pca' reads x"):
        umap.layout(g, **ab)
    with pytest.raises(ValueError, match=r"x: expected a \(40, D >= 2\) array"):
        umap.layout(g, x=x[:, :1], **ab)
    with pytest.raises(ValueError, match=r"init: expected shape \(40, 2\)"):
        umap.layout(g, init=np.zeros((39, 2)), **ab)
    with pytest.raises(ValueError, match="it has no 'indptr'"):
        umap.layout({"offsets": [0, 40]}, x=x, **ab)
    with pytest.raises(ValueError, match="indices must hold 80 entries"):
        umap.layout(dict(g, indices=g["indices"][:-1]), x=x, **ab)
    # the limits on the segments: 2 .. 16384 rows, at most 65535 of them
    big = {"indptr": np.zeros(16386, dtype=np.int64), "indices": np.zeros(0, dtype=np.int32), "data": np.zeros(0),
           "offsets": np.array([0, 16385]), "nnz_offsets": np.array([0, 0])}
    with pytest.raises(ValueError, match=r"2 \.\. 16384 rows"):
        umap.layout(big, init="random", **ab)
    S = 65536
    many = {"indptr": np.zeros(3 * S, dtype=np.int64), "indices": np.zeros(0, dtype=np.int32), "data": np.zeros(0),
            "offsets": 2 * np.arange(S + 1), "nnz_offsets": np.zeros(S + 1, dtype=np.int64)}
    with pytest.raises(ValueError, match="at most 65535"):
        umap.layout(many, init="random", **ab)
    with pytest.raises(ValueError, match="n_pcs must be at least 2"):
        umap.expression_umap(np.ones((200, 30), dtype=np.float32), n_pcs=1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised without a GPU")
def test_no_gpu_error_names_the_module():
    g = umap.from_scipy([_ring(40)])
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.umap: no GPU available"):
        umap.layout(g, init="random", a=0.58, b=1.33)
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.neighbors: no GPU available"):
        umap.umap(np.random.RandomState(0).rand(40, 6), n_neighbors=10)


def test_from_scipy():
    from scipy import sparse
    a, b = _ring(40), _ring(7)
    g = umap.from_scipy([a, b.tocoo()])
    assert g["offsets"].tolist() == [0, 40, 47] and g["nnz_offsets"].tolist() == [0, 80, 94]
    assert g["indptr"].shape == (49,) and g["indptr"].dtype == np.int64 and g["indices"].dtype == np.int32
    assert np.array_equal(g["indptr"][41:], b.indptr) and np.array_equal(g["indices"][80:], b.indices)
    asym = a.tolil()
    asym[0, 1] = 0.5
    with pytest.raises(ValueError, match="matrix 1: not symmetric"):
        umap.from_scipy([a, asym.tocsr()])
    missing = a.tolil()
    missing[0, 5] = 1.0
    with pytest.raises(ValueError, match="not symmetric"):
        umap.from_scipy([missing.tocsr()])
    with pytest.raises(ValueError, match="the diagonal must be empty"):
        umap.from_scipy([(a + sparse.identity(40)).tocsr()])
    with pytest.raises(ValueError, match="positive and finite"):
        umap.from_scipy([(-a).tocsr()])
    with pytest.raises(ValueError, match="square scipy.sparse matrix"):
        umap.from_scipy([np.eye(4)])
    with pytest.raises(ValueError, match=r"2 \.\. 16384 rows"):
        umap.from_scipy([sparse.csr_matrix((1, 1))])


def test_cli_parsing():
    a = umap.parse_args(["--pred", "1.npy", "2.npy", "--raw", "--n_neighbors", "20", "--n_epochs", "50", "--seed", "7",
                         "--out_dir", "o"])
    assert a.pred == ["1.npy", "2.npy"] and a.raw and a.n_neighbors == 20 and a.n_pcs == 50 and a.out_dir == "o"
    assert a.n_epochs == 50 and a.seed == 7 and a.n_top_genes == 1024
    b = umap.parse_args(["--pred", "1.npy", "--out_dir", "o"])
    assert not b.raw and b.n_neighbors == 150 and b.n_epochs is None and b.seed == 0
    for bad in (["--pred", "1.npy"], ["--out_dir", "o"], ["--pred", "1.npy", "--out_dir", "o", "--n_neighbors", "1"],
                ["--pred", "1.npy", "--out_dir", "o", "--n_pcs", "1"], ["--pred", "1.npy", "--out_dir", "o", "--n_pcs", "65"],
                ["--pred", "1.npy", "--out_dir", "o", "--n_epochs", "0"],
                ["--pred", "1.npy", "--out_dir", "o", "--n_epochs", "5001"]):
        with pytest.raises(SystemExit):
            umap.parse_args(bad)


# -------------------------------------------------------------------------------------------------------- the C ABI
def _count_args(text, name, call):
    """The number of top-level arguments of the first ``name(...)`` in ``text`` (``call``: a call, else a declaration)."""
    m = re.search(r"\b" + name + r"\s*\(", text)
    assert m, f"{name} not found"
    depth, args, i = 1, 1, m.end()
    while depth:
        ch = text[i]
        depth += ch in "(["
        depth -= ch in ")]"
        args += ch == "," and depth == 1
        i += 1
    return args


def test_declarations_agree():
    """include/mclstexp_hip.h, the ctypes prototypes and INTEGRATION.md's calls name the same entry points with the same
    number of arguments; the ABI number stays."""
    from mclstexp_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    assert lib.mcl_abi_version() == 13 == _lib.ABI_VERSION
    for s in SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(lib, s)
        assert _count_args(header, s, False) == len(_lib.PROTOTYPES[s]), s
        assert _count_args(doc, "lib." + s, True) == len(_lib.PROTOTYPES[s]), s
    assert _lib._RESTYPES["mcl_umap_workspace_bytes"] is _lib.C.c_int64
    assert _lib.PROTOTYPES["mcl_umap_epochs"][18] is _lib.C.c_uint64 and _lib.PROTOTYPES["mcl_umap_init"][10] is _lib.C.c_uint64


def test_capi_argument_errors_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_umap_workspace_bytes(1000, 3) >= 1000 * 33 + 3 * 8
    assert lib.mcl_umap_workspace_bytes(-1, 1) == 0 and lib.mcl_umap_workspace_bytes(10, 0) == 0
    one, two = _lib.C.c_void_p(16), _lib.C.c_void_p(32)

    def epochs(first=0, count=1, S=1, rows=70, min_n=70, max_n=70, max_epochs=100, a=0.58, b=1.33, gamma=1.0, alpha=1.0,
               rate=5, y1=two):
        return lib.mcl_umap_epochs(first, count, one, one, one, one, one, S, rows, min_n, max_n, 1000, max_epochs, a, b, gamma,
                                   alpha, rate, 0, one, one, y1, one, None)
    nan, inf = float("nan"), float("inf")
    # null pointers and inconsistent arguments
    assert lib.mcl_umap_prepare(None, None, None, 1, 10, 10, 100, 5, None, None, None) == -1
    assert lib.mcl_umap_init(1, None, 0, 1, 0, None, 1, 70, 70, 70, 0, None, None) == -1
    assert lib.mcl_umap_epochs(0, 1, None, None, None, None, None, 1, 70, 70, 70, 10, 100, 0.5, 1.3, 1.0, 1.0, 5, 0, None,
                               None, None, None, None) == -1
    assert lib.mcl_umap_init(2, one, 5, 1, 5, one, 1, 70, 70, 70, 0, one, None) == -1            # mode
    assert lib.mcl_umap_init(0, one, 5, 1, 1, one, 1, 70, 70, 70, 0, one, None) == -1            # D < 2
    assert lib.mcl_umap_init(0, None, 5, 1, 5, one, 1, 70, 70, 70, 0, one, None) == -1           # pca without x
    assert lib.mcl_umap_prepare(one, one, one, 1, 10, 11, 100, 5, one, one, None) == -1          # max_nnz > nnz_total
    assert epochs(y1=one) == -1                                                                  # one buffer twice
    assert epochs(first=99, count=2) == -1                                                       # beyond max_epochs
    assert epochs(first=-1) == -1 and epochs(min_n=71) == -1
    # the limits, refused before any launch whatever the pointers
    assert epochs(rows=1, min_n=1, max_n=1) == -2                                                # n_s < 2
    assert epochs(rows=16385, min_n=16385, max_n=16385) == -2
    assert epochs(S=65536, rows=65536 * 2, min_n=2, max_n=2) == -2
    assert epochs(max_epochs=0) == -2 and epochs(max_epochs=5001) == -2
    assert epochs(rate=-1) == -2 and epochs(rate=65) == -2
    for kw in (dict(a=nan), dict(b=inf), dict(gamma=nan), dict(alpha=-inf), dict(a=0.0), dict(b=-1.0)):
        assert epochs(**kw) == -2, kw
    assert lib.mcl_umap_prepare(one, one, one, 1, 10, 10, 5001, 5, one, one, None) == -2
    assert lib.mcl_umap_prepare(one, one, one, 1, 10, 10, 100, 65, one, one, None) == -2
    assert lib.mcl_umap_prepare(one, one, one, 65536, 10, 10, 100, 5, one, one, None) == -2
    assert lib.mcl_umap_init(1, None, 0, 1, 0, one, 1, 16385, 16385, 16385, 0, one, None) == -2
    assert lib.mcl_umap_init(1, None, 0, 1, 0, one, 1, 1, 1, 1, 0, one, None) == -2
