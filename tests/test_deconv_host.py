"""CPU: the host rules of mclstexp_amd.deconv and the numpy restatement tests/deconv_reference.py against
``scipy.optimize.nnls``, ``numpy.linalg``, ``pandas.groupby`` and ``numpy.corrcoef``.  No device code runs here."""
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

import deconv_reference as dr
from conftest import GOLDEN_DIR
from mclstexp_amd import deconv as dc


def _generator():
    spec = importlib.util.spec_from_file_location("gen_deconv_goldens", os.path.join(GOLDEN_DIR, "gen_deconv_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scipy_results():
    """scipy's coef and rnorm of every case, computed once."""
    return _generator().build(check=False)


@pytest.fixture(scope="module")
def cases():
    return {c: dr.make_case(c[0], c[1], c[2], dr.case_seed(*c[:3]), c[3]) for c in dr.CASES}


# ------------------------------------------------------------------------------------------------- the restatement
def test_golden_regenerates(scipy_results):
    stored = np.load(os.path.join(GOLDEN_DIR, "deconv.npz"))
    assert sorted(stored.files) == sorted(scipy_results)
    for key, v in scipy_results.items():
        assert np.array_equal(stored[key], v), key
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "deconv.npz")) < 1 << 20


@pytest.mark.parametrize("case", dr.CASES, ids=lambda c: dr.case_name(*c))
def test_restatement_against_scipy(case, cases, scipy_results):
    """Every spot within a quarter of the perturbation bound, which leaves the device honest room; the KKT certificate;
    at most T / 2 + 7 inner solves on these fixtures."""
    S, x = cases[case]
    G, T, n, _ = case
    name = dr.case_name(*case)
    got = dr.nnls(x, S)
    err = np.abs(got["coef"] - scipy_results[f"{name}.coef"]).max(axis=1)
    bound = dr.coef_bound(x, S)
    assert (err <= 0.25 * bound).all(), float((err / np.where(bound > 0, bound, 1)).max())
    dr.check_kkt(x, S, got["coef"])
    assert got["converged"].all() and got["n_iter"].max() <= T // 2 + 7
    assert (np.abs(got["rnorm"] - scipy_results[f"{name}.rnorm"]) <= dr.rnorm_bound(x, S)).all()
    # the special rows
    assert (got["coef"][:2] == 0.0).all() and (got["dominant"][:2] == -1).all()
    assert np.isnan(got["r2"][0]) and not np.isnan(got["r2"][1:]).any()
    assert abs(got["coef"][2, 0] - 1.0) <= bound[2] and got["dominant"][2] == 0
    assert np.allclose(got["proportions"][2:].sum(axis=1), np.where(got["coef"][2:].sum(axis=1) > 0, 1.0, 0.0), atol=1e-14)


def test_fixture_is_what_the_issue_states():
    S, x = dr.make_case(171, 20, 50, 3, 0.9)
    assert (S > 0).all() and (x[0] == 0).all() and (x[1] < 0).all() and np.array_equal(x[2], S[0])
    assert np.array_equal(S, S.astype(np.float32).astype(np.float64)) and np.array_equal(x, x.astype(np.float32))
    S0, _ = dr.make_case(171, 20, 50, 3, 0.0)
    assert np.array_equal(S0[0], S[0]) and np.allclose(S[1], 0.9 * S0[0] + 0.1 * S0[1], rtol=1e-6)
    S99, _ = dr.make_case(785, 64, 300, dr.case_seed(785, 64, 300), 0.99)
    assert 1e5 < np.linalg.cond(S99 @ S99.T) < 1e7


def test_gram_restatement_against_numpy():
    S, _ = dr.make_case(130, 64, 3, 1, 0.0)
    A, L, status = dr.gram(S)
    assert not status.any() and np.array_equal(A, A.T)
    assert np.allclose(A, S @ S.T, rtol=1e-14) and np.allclose(L, np.linalg.cholesky(A), rtol=1e-9, atol=1e-9)
    dup = S.copy()
    dup[5] = dup[2]
    assert dr.gram(dup)[2].tolist() == [6, 0]
    zero = S.copy()
    zero[3] = 0.0
    assert dr.gram(zero)[2].tolist() == [4, 0]
    nan = S.copy()
    nan[7, 11] = np.nan
    assert dr.gram(nan)[2].tolist() == [0, 8]
    xs = np.ones((4, 130))
    xs[2, 5] = np.inf
    assert dr.products(xs, S)[2] == 2 and dr.products(np.ones((4, 130)), S)[2] == -1


def test_cap_keeps_the_last_feasible_iterate():
    """A spot that reaches the cap does not loop: converged = 0, n_iter = the cap, coef >= 0 and no worse a fit than b = 0."""
    S, x = dr.make_case(130, 64, 8, 2, 0.0)
    A, c = dr.gram(S)[0], dr.products(x, S)[0]
    b, it, conv = dr.solve_one(A, c[5])
    assert conv == 1 and it > 2
    b2, it2, conv2 = dr.solve_one(A, c[5], cap=2)
    assert conv2 == 0 and it2 == 2 and (b2 >= 0).all() and (b2 > 0).any()
    assert np.linalg.norm(x[5] - b2 @ S) < np.linalg.norm(x[5])


def test_solve_waves_follow_the_lds_budget():
    assert dr.solve_waves(64) == 7 and dr.solve_waves(33) == 16 and dr.solve_waves(8) == 16 and dr.solve_waves(1) == 16
    assert 64 * 64 * 8 + 7 * (64 * 65 // 2 + 32) * 8 <= dr.LDS_BYTES <= 160 * 1024
    assert dc.MAX_TYPES == dr.MAX_T and dc.MAX_GENES == dr.MAX_G


# ------------------------------------------------------------------------------------------------------ host rules
@pytest.mark.parametrize("xs,ss,ld,what", [
    ((10, 8), (65, 8), None, "types"), ((10, 8), (0, 8), None, "types"), ((10, 4), (5, 4), None, "genes"),
    ((10, 16385), (4, 16385), None, "genes"), ((10, 9), (4, 8), None, "expected"), ((10, 8), (4, 8), 7, "ld"),
    ((10, 8), (4, 8), 11, "expected"), ((0, 8), (4, 8), None, "no spot"), ((1 << 26, 64), (64, 64), None, "coefficients"),
    ((10,), (4, 8), None, "2-D"), ((10, 8), (4,), None, "2-D")])
def test_every_limit_is_a_value_error(xs, ss, ld, what):
    with pytest.raises(ValueError, match=what):
        dc.check_problem(xs, ss, ld)


def test_limits_that_pass():
    assert dc.check_problem((10, 11), (4, 8), 11) == (10, 8, 4)
    assert dc.check_problem((1, 64), (64, 64)) == (1, 64, 64)
    assert dc.check_problem(((1 << 25) - 1, 64), (64, 64)) == ((1 << 25) - 1, 64, 64)


def test_entry_checks_come_before_the_device():
    with pytest.raises(ValueError, match="types"):
        dc.nnls(np.zeros((3, 70)), np.ones((65, 70)))
    with pytest.raises(ValueError, match="genes"):
        dc.nnls(np.zeros((3, 4)), np.ones((5, 4)))
    with pytest.raises(ValueError, match="one label vector"):
        dc.signatures_from_groups([np.zeros((3, 4))], [])
    with pytest.raises(ValueError, match="do not match"):
        dc.signatures_from_groups([np.zeros((3, 4))], [np.zeros(2, dtype=np.int64)])
    with pytest.raises(ValueError, match="occurs on no slide"):
        dc.signatures_from_groups([np.zeros((3, 4))], [np.array([0, 2, 2])])
    with pytest.raises(ValueError, match="at least one slide"):
        dc.deconvolve_slides([], np.ones((2, 4)))
    with pytest.raises(ValueError, match="one ground truth"):
        dc.deconvolution_recovery([np.zeros((3, 4))], [], np.ones((2, 4)))


def test_encode_pooled():
    codes, names = dc.encode_pooled([np.array(["b", "undetermined", "a"]), np.array(["c", "a"])])
    assert names.tolist() == ["a", "b", "c"] and [c.tolist() for c in codes] == [[1, -1, 0], [2, 0]]
    codes, names = dc.encode_pooled([np.array([1, -1, 0]), np.array([2, 2])])
    assert names.tolist() == [0, 1, 2] and [c.tolist() for c in codes] == [[1, -1, 0], [2, 2]]
    with pytest.raises(ValueError, match="occurs on no slide"):
        dc.encode_pooled([np.array([0, 3]), np.array([1])])
    with pytest.raises(ValueError, match="no spot is left"):
        dc.encode_pooled([np.array(["undetermined"])])
    with pytest.raises(ValueError, match=">= -1"):
        dc.encode_pooled([np.array([0, -2])])


def test_pooling_against_pandas_groupby():
    rng = np.random.default_rng(0)
    K, G = 4, 6
    mats = [rng.standard_normal((n, G)) for n in (30, 7, 55)]
    labs = [rng.integers(-1, K, m.shape[0]) for m in mats]
    labs[1][labs[1] == 2] = 0                                     # a group absent from a slide
    means, sizes = [], []
    for m, lab in zip(mats, labs):
        sizes.append(np.array([(lab == g).sum() for g in range(K)]))
        with np.errstate(all="ignore"):
            means.append(np.stack([m[lab == g].mean(axis=0) if (lab == g).any() else np.full(G, np.nan) for g in range(K)]))
    got = dc.pool_means(means, sizes)
    frame = pd.DataFrame(np.concatenate(mats))
    frame["label"] = np.concatenate(labs)
    want = frame[frame["label"] >= 0].groupby("label").mean().to_numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_recovery_formulas_against_numpy():
    rng = np.random.default_rng(1)
    n, T = 50, 5
    pp, pt = rng.dirichlet(np.ones(T), n), rng.dirichlet(np.ones(T), n)
    pp[:, 3] = 0.25                                               # a constant column: r undefined
    rp = {"proportions": pp, "dominant": pp.argmax(axis=1)}
    rt = {"proportions": pt, "dominant": pt.argmax(axis=1)}
    sc = dc.recovery_scores(rp, rt)
    for t in range(T):
        if t == 3:
            assert np.isnan(sc["pearson"][t])
        else:
            assert abs(sc["pearson"][t] - np.corrcoef(pp[:, t], pt[:, t])[0, 1]) <= 1e-12
    assert sc["dominant_agreement"] == np.mean(pp.argmax(axis=1) == pt.argmax(axis=1))
    assert abs(sc["rmse"] - np.sqrt(np.mean((pp - pt) ** 2))) <= 1e-15
    assert np.isnan(dc.column_pearson(pp[:1], pt[:1])).all()
    res = [{"proportions": np.array([[0.5, 0.5, 0.0], [0.1, 0.1, 0.8]])}]
    assert dc.top_types(res, 0, 2).tolist() == [2, 0] and dc.top_types(res, 0, 5).tolist() == [2, 0, 1]


# ------------------------------------------------------------------------------------------------------------- CLI
def test_cli_argument_parsing():
    a = dc.parse_args(["--pred", "p0.npy", "p1.npy", "--signatures", "s.npy"])
    assert a.pred == ["p0.npy", "p1.npy"] and a.signatures == "s.npy" and a.true is None and a.top == dc.TOP_N
    a = dc.parse_args(["--pred", "p.npy", "--labels", "l.npy", "--true", "t.npy", "--top", "3", "--out_dir", "d",
                       "--types", "n.npy"])
    assert a.labels == ["l.npy"] and a.true == ["t.npy"] and a.top == 3 and a.out_dir == "d" and a.types == "n.npy"
    for bad in (["--pred", "p.npy"], ["--pred", "p.npy", "--signatures", "s.npy", "--labels", "l.npy", "--true", "t.npy"],
                ["--pred", "p.npy", "--labels", "l.npy"], ["--pred", "p.npy", "q.npy", "--labels", "l.npy", "--true", "t.npy"],
                ["--pred", "p.npy", "q.npy", "--signatures", "s.npy", "--true", "t.npy"],
                ["--pred", "p.npy", "--signatures", "s.npy", "--top", "0"], ["--signatures", "s.npy"]):
        with pytest.raises(SystemExit):
            dc.parse_args(bad)


def test_format_lines():
    res = [{"coef": np.ones((2, 3)), "proportions": np.array([[0.5, 0.5, 0.0], [0.1, 0.1, 0.8]]), "r2": np.array([0.5, np.nan]),
            "dominant": np.array([0, -1])}]
    assert dc.format_slides(res, ["a", "b", "c"], 2) == ["slide 0 n = 2 mean r2 0.5000 unassigned 1: c 0.4000, a 0.3000"]
    rec = {"pearson": np.array([[0.5, np.nan]]), "dominant_agreement": np.array([0.25]), "rmse": np.array([0.125]),
           "mean_pearson": 0.5, "mean_dominant_agreement": 0.25, "mean_rmse": 0.125}
    assert dc.format_recovery(rec)[-1] == "recovery: mean Pearson 0.5000, mean dominant agreement 0.2500, mean RMSE 0.1250"
