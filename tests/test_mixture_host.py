"""CPU: the numpy restatement tests/mixture_reference.py (the yardstick of tests/test_mixture_gpu.py) against sklearn's own
results, recorded in tests/golden/mixture.npz by tests/golden/gen_mixture_goldens.py (scikit-learn 1.7.2): GaussianMixture
with its k-means step replaced by given labels, ``.bic()`` / ``.aic()`` / ``score_samples`` / ``predict_proba``,
``silhouette_samples``, ``calinski_harabasz_score`` and ``davies_bouldin_score``.

Fixtures (mixture_reference.make_case: K centres randn * sep, per-cluster mixing I + 0.3 randn, initial labels = the truth
with 15 % of the rows reassigned and rows 0 .. K - 1 forced to 0 .. K - 1), (n, D, K, sep) = (257, 9, 4, 3), (143, 9, 6, 2),
(64, 1, 2, 3), (1000, 50, 8, 1.5), (4097, 9, 7, 2), (40, 3, 3, 4), all four covariance types.  On them sklearn converges in
3 - 10 iterations, ||change of lower_bound| - tol| >= 4.9e-5 at every iteration (asserted >= 1e-6: n_iter cannot flip), and
no row has a top-two log_resp gap below 1.0e-2 (asserted: the share of rows below 1e-6 is 0).

Tolerances: both sides are fp64 and differ in summation order and libm only.  MEASURED holds the largest deviation of each
output over all fixtures and types as measured on the CPU this was written on; 16 x that is allowed.  n_iter, converged
and the labels are equal.  precisions_cholesky and score_samples carry the conditioning of the covariances they invert
(the 50-dimensional full ones most of all); the mean silhouette came out within one rounding of a value below 1, so its
allowance is 16 roundings."""
import os

import numpy as np
import pytest

import mixture_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture.npz")
EPS = 2.0 ** -52
MARGIN = 16.0
MEASURED = {  # absolute unless the name ends in _rel (then relative to the largest magnitude of the recorded array)
    "lower_bounds": 5.0e-14, "weights": 3.1e-16, "means": 5.0e-15, "covariances": 2.2e-14,
    "precisions_cholesky_rel": 9.5e-12, "score": 2.9e-14, "bic_rel": 7.2e-16, "aic_rel": 7.4e-16,
    "score_samples": 9.2e-12, "resp": 2.5e-14, "silhouette_samples": 5.0e-15, "silhouette": EPS,
    "calinski_harabasz_rel": 4.7e-16, "davies_bouldin_rel": 1.3e-15,
}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def fits():
    """The restatement's fit of every fixture and type, computed once."""
    out = {}
    for case in mr.CASES:
        x, init, _ = mr.make_case(*case)
        for ctype in mr.TYPES:
            out[(mr.case_name(case), ctype)] = mr.fit(x, case[2], init, ctype)
    return out


def close(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.max(np.abs(got - want)))
    if name.endswith("_rel"):
        err /= float(np.max(np.abs(want)))
    assert err <= MARGIN * MEASURED[name], (name, err, MEASURED[name])
    return err


@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_name)
def test_fixture_is_the_recorded_one(case, golden):
    x, init, _ = mr.make_case(*case)
    want = golden[mr.case_name(case) + "/checksum"]
    got = np.array([x.sum(), np.abs(x).sum(), x[0, 0], x[-1, -1], float(init.sum())])
    assert np.allclose(got, want, rtol=1e-12, atol=0), "numpy's generator no longer reproduces the recorded fixture"
    assert np.array_equal(init[:case[2]], np.arange(case[2]))


@pytest.mark.parametrize("ctype", mr.TYPES)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_name)
def test_fixture_conditions(case, ctype, golden, fits):
    """No iteration sits within 1e-6 of the stopping threshold and no row within 1e-6 of a label tie."""
    key = f"{mr.case_name(case)}/{ctype}/"
    lbs = golden[key + "lower_bounds"]
    change = np.abs(np.diff(np.concatenate([[-np.inf], lbs])))
    assert np.min(np.abs(change - 1e-3)) >= 1e-6
    assert 3 <= lbs.size <= 10 and int(golden[key + "converged"]) == 1
    gap = mr.top_two_gap(fits[(mr.case_name(case), ctype)]["log_resp"])
    assert np.mean(gap < 1e-6) == 0.0


@pytest.mark.parametrize("ctype", mr.TYPES)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_name)
def test_restated_fit_is_sklearns(case, ctype, golden, fits):
    key = f"{mr.case_name(case)}/{ctype}/"
    f = fits[(mr.case_name(case), ctype)]
    assert f["status"] == 0
    assert f["n_iter"] == int(golden[key + "n_iter"]) and f["converged"] == int(golden[key + "converged"])
    close(f["lower_bounds"], golden[key + "lower_bounds"], "lower_bounds")
    assert f["lower_bound"] == f["lower_bounds"][-1]
    for name in ("weights", "means", "covariances"):
        assert f[name].shape == golden[key + name].shape
        close(f[name], golden[key + name], name)
    assert f["precisions_cholesky"].shape == mr.cov_shape(ctype, case[2], case[1])
    close(f["precisions_cholesky"], golden[key + "precisions_cholesky"], "precisions_cholesky_rel")
    close(f["score"], golden[key + "score"], "score")
    close(f["bic"], golden[key + "bic"], "bic_rel")
    close(f["aic"], golden[key + "aic"], "aic_rel")
    close(f["lse"][:32], golden[key + "score_samples_head"], "score_samples")
    close(f["resp"][:32], golden[key + "resp_head"], "resp")
    assert np.array_equal(f["labels"], golden[key + "labels"].astype(np.int32))


@pytest.mark.parametrize("labelling", ["init", "edge"])
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_name)
def test_restated_validity_is_sklearns(case, labelling, golden):
    """init: the fixture's noisy labels; edge: one row alone in cluster 900 (silhouette 0) and ten rows labelled -1."""
    key = f"{mr.case_name(case)}/validity_{labelling}/"
    if key + "labels" not in golden.files:
        assert labelling == "edge" and case[0] < 40
        return
    x, _, _ = mr.make_case(*case)
    lab = golden[key + "labels"].astype(np.int64)
    v = mr.validity(x, lab)
    want = golden[key + "silhouette_samples"]
    assert np.array_equal(np.isnan(v["silhouette_samples"]), lab < 0)
    keep = lab >= 0
    close(v["silhouette_samples"][keep], want[keep], "silhouette_samples")
    close(v["silhouette"], np.mean(want[keep]), "silhouette")
    close(v["calinski_harabasz"], golden[key + "calinski_harabasz"], "calinski_harabasz_rel")
    close(v["davies_bouldin"], golden[key + "davies_bouldin"], "davies_bouldin_rel")
    if labelling == "edge":
        assert v["silhouette_samples"][5] == 0.0


def test_restated_edges():
    """What sklearn refuses or leaves open, as the kernels state it."""
    x, init, _ = mr.make_case(40, 3, 3, 4.0)
    one = mr.validity(x, np.zeros(40, dtype=np.int64))                    # one cluster
    each = mr.validity(x, np.arange(40))                                  # n clusters
    for v in (one, each):
        assert np.isnan(v["silhouette"]) and np.isnan(v["calinski_harabasz"]) and np.isnan(v["davies_bouldin"])
        assert np.isnan(v["silhouette_samples"]).all()
    lab = init.copy()
    lab[lab == 2] = 0
    lab[7] = 2                                                            # a one-point component
    assert mr.fit(x, 3, lab, "full", reg=0.0)["status"] == 1              # sklearn: ill-defined empirical covariance
    assert mr.fit(x, 3, lab, "full", reg=1e-6)["status"] == 0
    f = mr.fit(x[:3], 3, np.arange(3), "full")                            # n = K: every covariance is reg_covar alone
    assert f["status"] == 0 and np.allclose(f["covariances"], 1e-6 * np.eye(3)[None], rtol=0, atol=1e-18)
    assert mr.n_parameters("full", 8, 50) == 8 * 50 * 51 // 2 + 400 + 7
    assert mr.n_parameters("tied", 8, 50) == 50 * 51 // 2 + 400 + 7
    assert mr.n_parameters("diag", 8, 50) == 400 + 400 + 7 and mr.n_parameters("spherical", 8, 50) == 8 + 400 + 7
