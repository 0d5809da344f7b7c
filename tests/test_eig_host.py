"""CPU: the restatement of the device eigensolver (tests/eig_reference.py) against numpy.linalg.eigh inside the method's
backward-error bounds and against its own fixture (tests/golden/eig.npz) bit for bit; the host side of mclstexp_amd.eig and
of ``cluster.pca_device(solver=...)``: every argument error before the library is touched; the C entry points' checks."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cluster_reference as cr
import eig_reference as er
from mclstexp_amd import synth


@pytest.fixture(scope="module")
def golden():
    return np.load(er.GOLDEN)


@pytest.fixture(scope="module")
def matrices(golden):
    return {n: er.unpack(golden[f"{n}.a"]) for n in er.case_matrices()}


CASES = tuple(f"m{m}" for m in er.SIZES) + er.SPECTRA + ("zero",)


def _same_constants():
    """The restatement and the module under test state the same limits, guard and arithmetic constants."""
    from mclstexp_amd import eig
    assert (er.MAX_M, er.MAX_K, er.EPS) == (eig.MAX_M, eig.MAX_K, eig.EPS) and eig.GUARD == 64.0


def _within_bounds(a, k):
    lam, z, cert = er.eigh_top(a, k)
    m = a.shape[0]
    dl, res, orth, norm2, _, _ = er.errors(a, lam, z)
    bl, br, bo = er.bounds(m, norm2)
    print(f"m {m} k {k}: |dlam| {dl:.2e} / {bl:.2e}, residual {res:.2e} / {br:.2e}, orthogonality {orth:.2e} / {bo:.2e}")
    assert dl <= bl and res <= br and orth <= bo
    assert er.sign_rule_holds(z)
    assert (cert <= 64.0 * m * er.EPS).all()
    return lam, z, cert


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_eigh_and_fixture(golden, matrices, name):
    a = matrices[name]
    m = a.shape[0]
    assert np.array_equal(a, a.T)
    assert er.counts(m) == sorted({k for k in (1, 9, m - 1, min(m, 64)) if 1 <= k <= min(m, 64)})
    for k in er.counts(m):
        lam, z, cert = _within_bounds(a, k)
        assert lam.tobytes() == golden[f"{name}.k{k}.values"].tobytes(), (name, k)
        assert cert.tobytes() == golden[f"{name}.k{k}.certificate"].tobytes(), (name, k)
        if k == er.stored_vectors(name, m):
            assert z.tobytes() == golden[f"{name}.k{k}.vectors"].tobytes(), (name, k)


@pytest.mark.parametrize("name", er.GRAM_CASES)
def test_restatement_on_the_gram_matrices_of_the_cluster_cases(name):
    _same_constants()
    a = er.gram_matrix(cr.kept(synth.make_cluster_case(**cr.CLUSTER_CASES[name]))[0])
    assert np.array_equal(a, a.T)
    for k in (9, 64):
        _within_bounds(a, k)


def test_case_table(matrices):
    assert sorted(a.shape[0] for n, a in matrices.items() if n.startswith("m")) == sorted(er.SIZES) == [1, 2, 3, 17, 64, 65, 130]
    assert all(matrices[n].shape == (130, 130) for n in er.SPECTRA)
    assert er.BATCH == (130, 3, 65, 17, 2)
    assert not matrices["zero"].any()
    w = np.linalg.eigvalsh(matrices["diag10"])
    assert (np.abs(w - 7.0) < 1e-12).sum() == 10 and np.count_nonzero(matrices["diag10"] - np.diag(np.diag(matrices["diag10"]))) == 0
    w = np.linalg.eigvalsh(matrices["pairs"])[::-1]
    assert (np.abs(w[0:60:2] - w[1:60:2]) < 1e-12).all()
    assert np.linalg.matrix_rank(matrices["rank30"]) == 30
    # the cases named SEPARATED have relative gaps >= 1e-3 between their k + 1 leading eigenvalues, for every k tested
    for n in er.SEPARATED:
        w = np.linalg.eigvalsh(matrices[n])[::-1]
        top = w[:min(w.size, 65)]
        if top.size > 1:
            assert ((top[:-1] - top[1:]) / np.abs(top[:-1])).min() >= 1e-3, n


def test_zero_matrix_gives_unit_vectors(matrices):
    lam, z, cert = er.eigh_top(matrices["zero"], 9)
    assert not lam.any() and np.array_equal(z, np.eye(17)[:, :9]) and not cert.any()


def test_start_vectors_depend_on_row_and_column_only():
    _same_constants()
    big, small = er.start_vectors(130, 64), er.start_vectors(17, 9)
    part = big[:17, :9] / np.sqrt((big[:17, :9] ** 2).sum(axis=0))       # the same hash values, normalised over 17 rows
    # a sum of m rounded squares, a square root and a division: (m + 4) eps / 2 per normalisation, two of them compared
    assert np.abs(small - part).max() <= (17 + 4) * er.EPS
    assert np.abs((big * big).sum(axis=0) - 1.0).max() <= (130 + 4) * er.EPS
    assert abs(big.mean()) < 0.05 / np.sqrt(130) and np.linalg.matrix_rank(big) == 64


# ------------------------------------------------------------------------------------------------ host-side validation
@pytest.fixture
def untouched(monkeypatch):
    """No GPU, and the library must not be reached: loading it or calling into it fails the test."""
    import torch
    from mclstexp_amd import _lib, cluster, eig

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(eig, "call", boom)
    monkeypatch.setattr(cluster, "call", boom)


def test_eigh_top_argument_errors_come_before_the_library(untouched):
    from mclstexp_amd import eig
    a = np.diag(np.arange(1.0, 6.0))
    for k in (0, -1, 6, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="k must"):
            eig.eigh_top(a, k)
    with pytest.raises(ValueError, match="k must"):
        eig.eigh_top(np.eye(100), 65)
    with pytest.raises(ValueError, match="4096"):
        eig.eigh_top(np.zeros((4097, 4097), dtype=np.float32), 3)
    for bad in (np.zeros((4, 5)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match="square"):
            eig.eigh_top(bad, 1)
    ns = np.eye(4)
    ns[0, 3] = 1e-300
    with pytest.raises(ValueError, match="not symmetric"):
        eig.eigh_top(ns, 2)
    import torch
    flat = torch.zeros(13, dtype=torch.float64)
    with pytest.raises(ValueError, match="need 13 elements|device tensor"):
        eig.eigh_top(flat, 1, sizes=[3, 2])
    with pytest.raises(ValueError, match="elements"):
        eig.eigh_top(flat, 1, sizes=[3, 3])
    for sizes in ([0, 3], [4097], [], [[3]], [3.0]):
        with pytest.raises(ValueError):
            eig.eigh_top(flat, 1, sizes=sizes)
    with pytest.raises(ValueError, match="k must"):
        eig.eigh_top(flat, 3, sizes=[3, 2])
    with pytest.raises(ValueError, match="at most"):
        eig.check_sizes(np.full(65536, 3), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # valid arguments: the next thing is the missing GPU
        eig.eigh_top(a, 3)
    with pytest.raises(RuntimeError, match="slide 1"):
        eig.check_certificate(np.array([[1e-15, 1e-15], [1e-15, float("nan")]]), np.array([10, 20], dtype=np.int32))
    with pytest.raises(RuntimeError, match="slide 0"):
        eig.check_certificate(np.array([[64.0 * 10 * er.EPS * 1.01, 0.0]]), np.array([10], dtype=np.int32))
    eig.check_certificate(np.array([[64.0 * 10 * er.EPS, 0.0]]), np.array([10], dtype=np.int32))


def test_pca_solver_argument_errors_come_before_the_library(untouched):
    from mclstexp_amd import cluster, leiden, neighbors, tsne, umap
    x = np.zeros((30, 12))
    lab = np.array(["a", "b"] * 15)
    with pytest.raises(ValueError, match="solver must be one of"):
        cluster.pca_device(x, solver="gpu")
    with pytest.raises(ValueError, match="solver must be one of"):
        cluster.pca_scores_slides([x], solver="lapack")
    with pytest.raises(ValueError, match="solver must be one of"):
        cluster.cluster_slides([x], [lab], solver="")
    with pytest.raises(ValueError, match="solver must be one of"):
        cluster.cluster(x, lab, solver=None)
    big = np.zeros((4100, 4097), dtype=np.float32)
    with pytest.raises(ValueError, match='use solver="host"'):
        cluster.pca_device(big, solver="device")
    with pytest.raises(ValueError, match='use solver="host"'):
        cluster.pca_device(np.zeros((4130, 4097), dtype=np.float32), offsets=[0, 30, 4130], solver="device")
    with pytest.raises(ValueError):
        cluster.pca_device(x, n_comps=65, solver="device")
    for solver in cluster.SOLVERS:                                   # valid: the next thing is the missing GPU
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.pca_device(x, solver=solver)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.pca_device(big, solver="host")                       # the host solver has no such limit
    with pytest.raises(ValueError, match="pca_solver must be one of"):
        tsne.tsne(np.zeros((40, 9)), pca_solver="gpu")
    with pytest.raises(ValueError, match="solver must be one of"):
        tsne.embed_slides([np.zeros((40, 12))], pca_solver="gpu")
    with pytest.raises(ValueError, match="pca_solver must be one of"):
        neighbors.expression_graph(np.zeros((40, 12)), preprocess=False, pca_solver="gpu")
    with pytest.raises(ValueError, match="pca_solver must be one of"):
        umap.expression_umap(np.zeros((40, 12)), preprocess=False, pca_solver="gpu")
    with pytest.raises(ValueError, match="pca_solver must be one of"):
        leiden.expression_clusters(np.zeros((40, 12)), preprocess=False, pca_solver="gpu")


def test_the_keyword_is_threaded_through_and_host_stays_the_default():
    from mclstexp_amd import cluster, leiden, neighbors, tsne, umap
    for fn in (cluster.pca_device, cluster.pca_scores, cluster.pca_scores_slides, cluster.cluster_slides, cluster.cluster):
        assert inspect.signature(fn).parameters["solver"].default == "host", fn.__name__
    for fn in (tsne.tsne, tsne.embed_slides, neighbors.expression_graph, umap.expression_umap, leiden.expression_clusters):
        assert inspect.signature(fn).parameters["pca_solver"].default == "host", fn.__name__
    args = ["--pred", "p.npy", "--labels", "l.npy"]
    assert cluster.parse_args(args).pca_solver == "host"
    assert cluster.parse_args(args + ["--pca_solver", "device"]).pca_solver == "device"
    with pytest.raises(SystemExit):
        cluster.parse_args(args + ["--pca_solver", "gpu"])


# ---------------------------------------------------------------------------------------------------------- the C ABI
def test_abi_is_13_and_the_entry_points_reject_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_abi_version() == 13 == _lib.ABI_VERSION
    for s in ("mcl_sym_eig_workspace_bytes", "mcl_sym_eig_top"):
        assert s in _lib.PROTOTYPES and hasattr(lib, s)
    assert _lib._RESTYPES["mcl_sym_eig_workspace_bytes"] is C.c_int64
    ws = lib.mcl_sym_eig_workspace_bytes
    assert ws(1, 1, 1, 1) > 0
    assert ws(5, 130, 217, 9) >= 8 * (217 * 5 + 217 * 9 * 5)
    assert ws(1, 4096, 4096, 64) > ws(1, 4096, 4096, 9) > 0
    for bad in ((0, 5, 5, 1), (1, 0, 0, 1), (1, 5, 5, 0), (1, 5, 5, 6), (2, 5, 1, 1), (2, 5, 11, 1)):
        assert ws(*bad) == -1, bad
    for bad in ((1, 4097, 4097, 1), (1, 100, 100, 65), (65536, 2, 65536 * 2, 1)):
        assert ws(*bad) == -2, bad
    P = C.c_void_p(64)       # never dereferenced: every call below must be rejected on the host

    def top(a=P, aoff=P, m=P, S=2, max_m=8, sum_m=12, k=3, stages=7, ev=P, vec=P, eoff=P, cert=P, work=P):
        return lib.mcl_sym_eig_top(a, aoff, m, S, max_m, sum_m, k, stages, ev, vec, eoff, cert, work, None)

    for kw in ({"a": None}, {"aoff": None}, {"m": None}, {"ev": None}, {"vec": None}, {"eoff": None}, {"cert": None},
               {"work": None}, {"S": 0}, {"max_m": 0}, {"k": 0}, {"k": 9}, {"sum_m": 1}, {"sum_m": 17}, {"stages": 0},
               {"stages": 8}):
        assert top(**kw) == -1, kw
    assert top(max_m=4097, sum_m=4100) == -2 and top(k=65, max_m=100, sum_m=150) == -2
    assert top(S=65536, max_m=3, sum_m=65536 * 3) == -2
