"""CPU: the numpy restatement tests/nmf_reference.py against scikit-learn's recorded multiplicative-update NMF
(tests/golden/nmf.npz, written by tests/golden/gen_nmf_goldens.py; the inputs are regenerated from their seeds), and the host
side of mclstexp_amd.nmf: the random start, the limits, the matching and the scores of ``program_recovery``.

The restatement runs scikit-learn's arithmetic through the same BLAS calls; what may differ is the summation order inside
them, so the bound is 64 eps max|.|, a few times the 25 eps seen over 200 Kullback-Leibler iterations."""
import os

import numpy as np
import pytest

import nmf_reference as nr
from conftest import GOLDEN_DIR
from mclstexp_amd import nmf

TAG = {"frobenius": "f", "kullback-leibler": "kl"}
PAIRS = [(c, loss) for c in nr.CASES for loss in nr.LOSSES]
TOL = 64 * nr.EPS


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "nmf.npz"))


def close(got, want, what):
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{what}: {err / nr.EPS:.2f} eps")
    assert got.shape == want.shape and err <= TOL, (what, err / nr.EPS)


# ------------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("case,loss", PAIRS, ids=[f"{c[0]}-{TAG[loss]}" for c, loss in PAIRS])
def test_restatement_matches_sklearn(case, loss, golden):
    name = case[0]
    X, W0, H0 = nr.make_case(*case[1:])
    W, H, n_iter, converged, _ = nr.fit(X, W0, H0, loss, nr.ITERS, 0.0)
    key = f"{name}.{TAG[loss]}"
    assert n_iter == nr.ITERS and not converged
    close(W[::nr.W_STRIDE.get(name, 1)], golden[f"{key}.W"], key + ".W")
    close(H[:, ::nr.H_STRIDE.get(name, 1)], golden[f"{key}.H"], key + ".H")
    want = float(golden[f"{key}.err"])
    assert abs(nr.error(X, W, H, loss) - want) <= TOL * want
    # zero rows and columns stay exactly zero, nothing is NaN
    assert (W[3] == 0).all() and (H[:, 2] == 0).all() and (H[:, -1] == 0).all() and np.isfinite(W).all() and np.isfinite(H).all()


@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_restatement_on_segments_transform_and_stop(loss, golden):
    name, off = nr.STACKED[0], nr.STACKED_OFFSETS
    X, W0, H0 = nr.case(name)
    for j in range(len(off) - 1):
        W, H = nr.fit(X[off[j]:off[j + 1]], W0[off[j]:off[j + 1]], H0, loss, nr.ITERS, 0.0)[:2]
        close(W, golden[f"{name}.{j}.{TAG[loss]}.W"], f"{name}.{j}.W")
        close(H, golden[f"{name}.{j}.{TAG[loss]}.H"], f"{name}.{j}.H")
    X, _, _ = nr.case(nr.TRANSFORM_CASE)
    Wt = nr.transform(X, golden[f"transform.{TAG[loss]}.H"], loss, nr.TRANSFORM_ITERS, 0.0)[0]
    close(Wt, golden[f"transform.{TAG[loss]}.W"], "transform.W")
    X, W0, H0 = nr.case(nr.STOP_CASE)
    W, H, n_iter, converged, hist = nr.fit(X, W0, H0, loss, nr.STOP_MAX_ITER, float(golden[f"stop.{TAG[loss]}.tol"]))
    assert n_iter == int(golden[f"stop.{TAG[loss]}.n_iter"]) and int(converged) == int(golden[f"stop.{TAG[loss]}.converged"])
    assert n_iter % 10 == 0 and 10 < n_iter < nr.STOP_MAX_ITER and hist.size == n_iter // 10 + 1
    want = float(golden[f"stop.{TAG[loss]}.err"])
    assert abs(nr.error(X, W, H, loss) - want) <= TOL * want


def test_random_init_is_sklearns_bit_for_bit(golden):
    X, _, _ = nr.case(nr.CASES[0][0])
    k, seed = nr.CASES[0][3], int(golden["random.seed"])
    for fn in (nmf.random_init, nr.random_init):
        W, H = fn(X, k, seed)
        assert np.array_equal(W, golden["random.W"]) and np.array_equal(H, golden["random.H"])
    W32, _ = nmf.random_init(X.astype(np.float32), k, seed)           # (fp32 input: the mean of its fp64 up-conversion)
    assert np.array_equal(W32, nmf.random_init(X.astype(np.float32).astype(np.float64), k, seed)[0])


def test_stored_spreads_are_the_restatements(golden):
    name, rows, G, k, seed = nr.CASES[0]
    X, W0, H0 = nr.make_case(rows, G, k, seed)
    for loss in nr.LOSSES:
        got = np.array(nr.permuted_spread(X, W0, H0, loss, nr.ITERS))
        assert np.array_equal(got, golden[f"{name}.{TAG[loss]}.spread"]) and (got > 0).all() and (got < 64 * nr.EPS).all()


# ----------------------------------------------------------------------------------------------------------- limits
def test_limits_and_bad_arguments_raise_before_the_library(monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library or the device was touched")
    monkeypatch.setattr(nmf, "call", touched)
    monkeypatch.setattr(nmf, "device", touched)
    x = np.ones((20, 6))
    bad = [dict(k=0), dict(k=65), dict(k=2.0), dict(k=True), dict(k=2, beta_loss="itakura-saito"), dict(k=2, n_init=0),
           dict(k=2, max_iter=0), dict(k=2, tol=-1.0), dict(k=2, tol=float("nan")), dict(k=2, tol=float("inf")),
           dict(k=2, init="nndsvd"), dict(k=2, init="nndsvda"), dict(k=2, offsets=[0, 10]), dict(k=2, offsets=[0, 10, 10, 20]),
           dict(k=2, offsets=[1, 20]), dict(k=2, ld=8), dict(k=2, ld=4, n_genes=6), dict(k=2, n_genes=5),
           dict(k=2, seed=-1), dict(k=2, init=(np.ones((20, 3)), np.ones((2, 6)))), dict(k=2, init=(np.ones((20, 2)), np.ones((2, 5)))),
           dict(k=2, init=(-np.ones((20, 2)), np.ones((2, 6)))), dict(k=2, init=(np.ones((3, 20, 2)), np.ones((3, 2, 6))), n_init=2),
           dict(k=2, init=(np.ones((20, 2)),)), dict(k=2, offsets=[0, 5, 20], n_init=40000)]
    for kw in bad:
        with pytest.raises(ValueError):
            nmf.nmf(x, **kw)
    for shape in ((20,), (2, 3, 4), (0, 6)):
        with pytest.raises(ValueError):
            nmf.nmf(np.ones(shape), 2)
    with pytest.raises(ValueError, match="genes"):
        nmf.check_problem((4, nmf.MAX_GENES + 1), 2)
    with pytest.raises(ValueError, match="usages"):
        nmf.check_problem((1 << 26, 8), 64)
    with pytest.raises(ValueError, match="problems"):
        nmf.check_problem((70000, 8), 2, offsets=np.arange(70001), n_init=1)
    with pytest.raises(ValueError):
        nmf.transform(x, np.ones((2, 5)))
    with pytest.raises(ValueError):
        nmf.transform(x, np.ones((2, 2, 6)))
    with pytest.raises(ValueError):
        nmf.transform(x, np.ones(6))
    for v in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="H must be"):
            nmf.transform(x, np.full((2, 6), v))
    with pytest.raises(ValueError):
        nmf.program_recovery([x], [x, x], 2)
    with pytest.raises(ValueError):
        nmf.program_recovery([x], [x], 2, n_top=0)
    assert nmf.check_problem((20, 8), 3, ld=8, n_genes=6)[:2] == (20, 6)
    rows, G, off = nmf.check_problem((20, 6), 64, offsets=[0, 7, 20], n_init=3)
    assert (rows, G, off.tolist()) == (20, 6, [0, 7, 20])


def test_custom_init_layouts():
    W0, H0 = np.ones((20, 2)), np.ones((2, 6))
    W, H, n = nmf.custom_init((W0, H0), 20, 6, 2, 1, 1)
    assert W.shape == (1, 20, 2) and H.shape == (1, 1, 2, 6) and n == 1
    W, H, n = nmf.custom_init((np.ones((3, 20, 2)), np.arange(36.0).reshape(3, 2, 6)), 20, 6, 2, 1, 3)
    assert H.shape == (1, 3, 2, 6) and n == 3 and H[0, 2, 1, 5] == 35
    W, H, n = nmf.custom_init((W0, np.arange(24.0).reshape(2, 2, 6)), 20, 6, 2, 2, 1)
    assert H.shape == (2, 1, 2, 6) and H[1, 0, 0, 0] == 12
    H4 = np.arange(72.0).reshape(3, 2, 2, 6)                              # (n_init, segments, k, G)
    W, H, n = nmf.custom_init((np.ones((3, 20, 2)), H4), 20, 6, 2, 2, 1)
    assert H.shape == (2, 3, 2, 6) and n == 3 and H[1, 2, 0, 0] == H4[2, 1, 0, 0]


# ------------------------------------------------------------------------------------------------- recovery helpers
def test_match_programs_overlaps_and_scores():
    a = np.array([[1.0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 1, 1]])
    b = np.array([[0, 2.0, 2, 0], [0, 0, 0, 0], [3, 0, 0, 0.0], [0, 0, 1, 3]])
    pairs, cos = nmf.match_programs(a, b)
    assert pairs[:3].tolist() == [[0, 2], [1, 0], [3, 3]]                  # two cosines of 1: the smaller (row, column) first
    assert np.allclose(cos[:2], 1.0, atol=4 * nr.EPS) and abs(cos[2] - 4 / np.sqrt(20)) <= 4 * nr.EPS
    assert pairs[3].tolist() == [2, 1] and cos[3] == 0.0                   # the zero programs: matched last, cosine 0
    assert nmf.match_programs(a[:2], b)[0].shape == (2, 2)
    assert nmf.top_indices(np.array([0.5, 2.0, 2.0, 0.1]), 3).tolist() == [1, 2, 0]
    pa = np.array([[5.0, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5]])
    pb = np.array([[0.0, 0, 1, 5, 4, 3], [5, 4, 0, 3, 2, 1]])
    over, jac = nmf.top_gene_overlap(pa, pb, np.array([[0, 1], [1, 0]]), 3)
    assert over.tolist() == [2, 3] and np.allclose(jac, [2 / 4, 1.0])
    up = np.array([[1.0, 0], [2, 1], [3, 0], [4, 5], [0, 1.0], [1, 2]])
    ut = np.array([[2.0, 0], [4, 0], [6, 0], [8, 5], [1, 1.0], [0, 2]])
    dp, dt = np.array([0, 0, 0, 1, 1, 1]), np.array([0, 0, 0, 0, 0, 1])
    sc = nmf.usage_scores(up, ut, dp, dt, np.array([0, 4, 6]))
    assert sc["pearson"].shape == (2, 2) and abs(sc["pearson"][0, 0] - 1.0) <= 4 * nr.EPS and abs(sc["pearson"][1, 0] + 1.0) <= 4 * nr.EPS
    assert sc["dominant_agreement"].tolist() == [0.75, 0.5] and abs(sc["dominant_agreement_pooled"] - 4 / 6) < 1e-15
    assert np.isnan(nmf.column_pearson(np.ones((3, 1)), np.arange(3.0)[:, None])[0])
    prog, usage, dom = nr.normalise(np.array([[1.0, 2], [0, 0], [3, 0]]), np.array([[1.0, 3], [0, 0]]))
    assert prog.tolist() == [[0.25, 0.75], [0, 0]] and usage.tolist() == [[4, 0], [0, 0], [12, 0]] and dom.tolist() == [0, -1, 0]


# ---------------------------------------------------------------------------------------------------------- symbols
def test_entry_points_are_declared_bound_and_check_their_arguments():
    from mclstexp_amd import _lib, build
    names = ("mcl_nmf_workspace_bytes", "mcl_nmf_check", "mcl_nmf_steps", "mcl_nmf_error", "mcl_nmf_programs")
    text = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, "include", "mclstexp_hip.h")).read()
    for n in names:
        assert n in _lib.PROTOTYPES and f"{n}(" in text
        assert (_lib.PROTOTYPES[n][-1:] == [_lib.c_s]) == (n != "mcl_nmf_workspace_bytes")
    assert _lib.ABI_VERSION == 13
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    # hht + hsum + wsum + wtw + wtx + err (a partial per wave of a tile), in doubles: 2 problems, 1 run, 5 tiles
    want = 2 * 25 + 2 * 5 + 2 * 5 + 2 * 25 + 2 * 5 * 37 + 2 * 5 * 8
    assert lib.mcl_nmf_workspace_bytes(70, 37, 5, 1, 2, 70, 0) == 8 * want
    assert lib.mcl_nmf_workspace_bytes(70, 37, 5, 1, 2, 70, 1) == 8 * (want - 2 * 25)       # KL: no W^T W, and no ratio matrix
    for args in ((70, 37, 65, 1, 1, 70, 0), (70, 16385, 5, 1, 1, 70, 0), (70, 37, 5, 65535, 2, 70, 0), (70, 37, 5, 1, 1, 71, 0),
                 (70, 37, 5, 1, 1, 70, 2), (0, 37, 5, 1, 1, 1, 0)):
        assert lib.mcl_nmf_workspace_bytes(*args) == -1
    assert lib.mcl_nmf_check(None, 37, 1, 70, 37, None, None) == -1
    assert lib.mcl_nmf_steps(None, 37, 1, None, 1, 1, 70, 37, 5, 70, 0, 1, None, None, None, None, 1, None) == -1
    assert lib.mcl_nmf_error(None, 37, 1, None, 1, 1, 70, 37, 5, 70, 0, None, None, None, None, 0, 0, 0.0, 10, None, None, 0, None) == -1
    assert lib.mcl_nmf_programs(None, None, None, 1, 70, 37, 5, 70, None, None, None, None, None) == -1
