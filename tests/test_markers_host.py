"""CPU: the numpy restatement of the marker-gene computation against scipy (live and the stored fixture) and mpmath's stored
values; argument validation of mclstexp_amd.markers and of the C entry points (MCL_EINVAL without a GPU); CLI parsing."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import markers_reference as mr
from golden.gen_markers_goldens import MP_CASES, SCIPY_CASES, gap_ok

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return np.load(mr.GOLDEN)


def rel(a, b):
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))))


@pytest.mark.parametrize("name", sorted(SCIPY_CASES))
def test_restatement_matches_the_scipy_fixture(golden, name):
    kw = SCIPY_CASES[name]
    x, labels = mr.make_case(**kw)
    k = kw["k"]
    w = mr.rank_genes_groups(x, labels, k, "wilcoxon")
    wt = mr.rank_genes_groups(x, labels, k, "wilcoxon", tie_correct=True)
    t = mr.rank_genes_groups(x, labels, k, "t-test")
    ls = labels[labels >= 0]
    assert np.array_equal(w["R2"], np.stack([golden[f"{name}.rank2"][ls == g].sum(axis=0) for g in range(k)]))
    ng = w["group_sizes"].astype(np.float64)[:, None]
    assert np.array_equal(w["R2"] / 2.0 - ng * (ng + 1) / 2.0, golden[f"{name}.U"])       # scipy's U statistic, exactly
    assert np.array_equal(w["full_scores"], golden[f"{name}.z"])                          # ranksums' z to the last bit
    assert rel(w["full_pvals"], golden[f"{name}.p"]) <= 64 * EPS                           # (8 z^2 eps of |z| / sqrt 2)
    assert rel(wt["full_pvals"], golden[f"{name}.p_tc"]) <= 64 * EPS
    assert rel(w["full_pvals_adj"], golden[f"{name}.adj"]) <= 64 * EPS
    assert rel(t["full_pvals"], golden[f"{name}.p_t"]) <= 1e-11                            # eps * lgamma(nu / 2)
    assert np.abs(t["full_scores"] - golden[f"{name}.t"]).max() <= 1e-13 * np.abs(golden[f"{name}.t"]).max()
    assert np.array_equal(w["names"], golden[f"{name}.order"]) and np.array_equal(t["names"], golden[f"{name}.order_t"])
    assert gap_ok(golden[f"{name}.z"]) and gap_ok(golden[f"{name}.t"])
    for key in ("err_z", "err_p", "err_p_tc", "err_p_t", "err_adj"):                       # the recorded errors are these
        got = {"err_z": rel(w["full_scores"], golden[f"{name}.z"]), "err_p": rel(w["full_pvals"], golden[f"{name}.p"]),
               "err_p_tc": rel(wt["full_pvals"], golden[f"{name}.p_tc"]),
               "err_p_t": rel(t["full_pvals"], golden[f"{name}.p_t"]),
               "err_adj": rel(w["full_pvals_adj"], golden[f"{name}.adj"])}[key]
        assert got == float(golden[f"{name}.{key}"]), key


def test_restatement_against_live_scipy():
    x, labels = mr.make_case(n=83, G=9, k=3, seed=3, kind="grid", dtype=np.float64, drop=0.15)
    keep = labels >= 0
    xs, ls = x[keep], labels[keep]
    w = mr.rank_genes_groups(x, labels, 3, "wilcoxon", tie_correct=True)
    t = mr.rank_genes_groups(x, labels, 3, "t-test")
    for j in range(9):
        r2, T = mr.rankdata2(xs[:, j])
        assert np.array_equal(r2, np.rint(2 * stats.rankdata(xs[:, j])).astype(np.int64))
        _, cnt = np.unique(xs[:, j], return_counts=True)
        assert T == int((cnt.astype(np.int64) ** 3 - cnt).sum()) == w["T"][j]
    for g in range(3):
        a, b = xs[ls == g], xs[ls != g]
        p = np.array([stats.mannwhitneyu(a[:, j], b[:, j], use_continuity=False, method="asymptotic").pvalue
                      for j in range(9)])
        assert rel(w["full_pvals"][g], p) <= 64 * EPS
        tt = stats.ttest_ind(a, b, equal_var=False)
        assert rel(t["full_pvals"][g], tt.pvalue) <= 1e-11
        assert np.allclose(t["full_scores"][g], tt.statistic, rtol=1e-12, atol=1e-14)
        assert rel(w["full_pvals_adj"][g], stats.false_discovery_control(w["full_pvals"][g], method="bh")) <= 4 * EPS
        assert np.array_equal(w["names"][g], np.argsort(-w["full_scores"][g], kind="stable"))
    assert np.array_equal(mr.rank_genes_groups(x, labels, 3)["R2"], mr.rank_genes_groups(xs, ls, 3)["R2"])


def test_restatement_log_space_against_mpmath(golden):
    name, kw = next(iter(MP_CASES.items()))
    x, labels = mr.make_case(**kw)
    w = mr.rank_genes_groups(x, labels, kw["k"], "wilcoxon")
    t = mr.rank_genes_groups(x, labels, kw["k"], "t-test")
    assert np.array_equal(w["full_scores"], golden[f"{name}.z"]) and np.array_equal(t["full_scores"], golden[f"{name}.t"])
    assert (w["full_pvals"] == 0).any() and np.isfinite(w["full_neglog10_pvals"]).all()
    assert np.isfinite(t["full_neglog10_pvals"]).all() and w["full_neglog10_pvals"].max() > 308
    assert rel(w["full_neglog10_pvals"], golden[f"{name}.nl_w"]) <= 16 * EPS
    assert rel(t["full_neglog10_pvals"], golden[f"{name}.nl_t"]) <= 64 * EPS


def test_restatement_edge_cases():
    x = np.ones((6, 2))
    x[:, 1] = [0.0, -0.0, 0.0, -0.0, 1.0, 1.0]
    labels = np.array([0, 0, 0, 1, 1, 2], dtype=np.int32)
    for tc in (False, True):
        w = mr.rank_genes_groups(x, labels, 4, "wilcoxon", tie_correct=tc)
        assert (w["full_scores"][:, 0] == 0).all() and (w["full_pvals"][:, 0] == 1).all()      # all equal: c = 0 / num 0
        assert w["T"].tolist() == [6 ** 3 - 6, (4 ** 3 - 4) + (2 ** 3 - 2)]                     # -0.0 ties with +0.0
        assert (w["full_scores"][3] == 0).all() and w["group_sizes"].tolist() == [3, 2, 1, 0]   # a label nobody carries
    t = mr.rank_genes_groups(x, labels, 4, "t-test")
    assert (t["full_scores"][2:] == 0).all() and (t["full_pvals"][2:] == 1).all()                # one spot, no spot
    one = mr.rank_genes_groups(x, np.zeros(6, np.int32), 1)
    assert (one["full_scores"] == 0).all() and (one["full_pvals"] == 1).all()                    # empty rest
    p = np.array([0.01, np.nan, 0.04, 0.03])
    assert np.allclose(mr.benjamini_hochberg(p), [0.04, 1.0, 0.04 * 4 / 3, 0.04 * 4 / 3])


# ------------------------------------------------------------------------------------------------ argument validation
def test_python_layer_validates_before_the_gpu():
    from mclstexp_amd import markers
    x = np.zeros((10, 4), np.float32)
    lab = np.zeros(10, np.int32)
    bad = [
        dict(x=np.zeros((10,), np.float32)), dict(x=np.zeros((10, 16385), np.float32)), dict(offsets=[0, 1, 10]),
        dict(offsets=[0, 11]), dict(k=256), dict(k=0), dict(k=[1, 2]), dict(method="logreg"), dict(tie_correct=1),
        dict(n_genes=0), dict(rankby_abs="yes"), dict(labels=np.zeros(9, np.int32)), dict(labels=np.zeros(10)),
        dict(x=np.zeros((16385, 1), np.float32), labels=np.zeros(16385, np.int32)),
    ]
    for kw in bad:
        args = dict(x=x, labels=lab, offsets=None, k=None)
        args.update(kw)
        with pytest.raises(ValueError):
            markers.rank_genes_groups(**args)
    with pytest.raises(ValueError):
        markers.marker_slides([x], [lab, lab])
    with pytest.raises(ValueError):
        markers.marker_slides([x], [np.zeros(9, np.int32)])
    with pytest.raises(ValueError):
        markers.marker_recovery([x], [np.zeros((10, 5), np.float32)], [lab])
    with pytest.raises(ValueError):
        markers.marker_recovery([x], [x], [lab], n_top=0)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU"):
            markers.rank_genes_groups(x, lab)


def test_label_encoding_and_host_helpers():
    from mclstexp_amd import markers
    codes, ks, cats = markers.encode_slides([np.array(["b", "undetermined", "a", "b"]), np.array([2, -1, 0])])
    assert codes.tolist() == [1, -1, 0, 1, 2, -1, 0] and ks.tolist() == [2, 3] and cats[0].tolist() == ["a", "b"]
    assert markers.infer_k(np.array([0, 1, -1, -1]), np.array([0, 2, 4])).tolist() == [2, 1]
    o, j = markers.recovery_table(np.array([[0, 1, 2], [3, 4, 5]]), np.array([[2, 1, 9], [6, 7, 8]]))
    assert o.tolist() == [2, 0] and np.allclose(j, [2 / 4, 0.0])
    assert markers.top_markers([{"names": np.array([[5, 1, 2], [1, 7, 3]])}], 0, 2).tolist() == [1, 5, 7]


def test_capi_argument_errors_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_marker_workspace_bytes(1000, 12, 2, 50) >= 2 * 32 + 1000 * 4 + 12 * 50 * 12
    for args in ((1, 1, 1, 1), (10, 0, 1, 1), (10, 1, 0, 1), (10, 1, 1, 16385), (16385, 1, 1, 1), (10, 256, 1, 1)):
        assert lib.mcl_marker_workspace_bytes(*args) == -1
    one = C.c_void_p(16)

    def stats_(x=one, ld=8, dtype=0, S=1, rows=100, G=8, max_n=100, kmax=3, KT=3, status=one):
        return lib.mcl_marker_stats(x, ld, dtype, one, one, one, S, rows, G, max_n, kmax, KT, one, one, one, one, one, one,
                                    one, one, one, one, one, status, None)
    for kw in (dict(x=None), dict(status=None), dict(S=0), dict(ld=7), dict(dtype=2), dict(max_n=16385), dict(max_n=1),
               dict(rows=101), dict(kmax=256), dict(kmax=0), dict(KT=4), dict(KT=0), dict(G=0), dict(G=16385, ld=16385)):
        assert stats_(**kw) == -1, kw
    assert lib.mcl_marker_rank_sums(None, 8, 0, one, 1, 100, 8, 100, 3, 3, one, one, one, None) == -1
    assert lib.mcl_marker_rank_sums(one, 8, 0, one, 1, 100, 8, 16385, 3, 3, one, one, one, None) == -1
    assert lib.mcl_marker_test(3, 0, 1, 100, 8, 3, 3, one, one, one, one, one, one, one, one, one, one, one, one, None) == -1
    assert lib.mcl_marker_test(0, 0, 1, 100, 8, 3, 3, one, one, one, one, one, one, None, one, one, one, one, one, None) == -1
    assert lib.mcl_marker_rank_adjust(1, 100, 8, 3, 3, 9, 0, *([one] * 12), None) == -1          # n_genes > G
    assert lib.mcl_marker_rank_adjust(1, 100, 8, 3, 3, 8, 0, None, *([one] * 11), None) == -1
    with pytest.raises(RuntimeError, match=r"mcl_marker_workspace_bytes rejected"):
        _lib.call("mcl_marker_workspace_bytes", 1, 1, 1, 1)


def test_cli_parsing():
    from mclstexp_amd import markers
    a = markers.parse_args(["--pred", "a.npy", "b.npy", "--labels", "la.npy", "lb.npy", "--out_dir", "d"])
    assert (a.method, a.tie_correct, a.top, a.true) == ("wilcoxon", False, 50, None)
    a = markers.parse_args(["--pred", "a.npy", "--labels", "l.npy", "--true", "t.npy", "--method", "t-test", "--tie_correct",
                            "--top", "7", "--out_dir", "d"])
    assert (a.method, a.tie_correct, a.top, a.true) == ("t-test", True, 7, ["t.npy"])
    for argv in (["--pred", "a.npy", "--labels", "l.npy", "m.npy", "--out_dir", "d"],
                 ["--pred", "a.npy", "--labels", "l.npy", "--true", "t.npy", "u.npy", "--out_dir", "d"],
                 ["--pred", "a.npy", "--labels", "l.npy", "--top", "0", "--out_dir", "d"],
                 ["--pred", "a.npy", "--labels", "l.npy", "--method", "logreg", "--out_dir", "d"],
                 ["--pred", "a.npy", "--labels", "l.npy"]):
        with pytest.raises(SystemExit):
            markers.parse_args(argv)
