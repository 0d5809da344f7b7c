"""CPU: the host side of mclstexp_amd.rank -- the library's null and limit checks, the Python layer's ValueErrors, the CLI's
arguments and report -- and the Python-int restatement (tests/rank_reference.py) against scipy (tests/golden/rank.npz)."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import rank_reference as rr
from genes_reference import pearson_pvalue
from rank_reference import EPS, GOLDEN, INT_NAMES, P_FLOOR, T_P_REL, case_inputs, normal_p_bound

CASES = ("batch", "spots", "zi1500")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def vectors(z, name):
    pred, true = case_inputs(z, name)
    if name == "batch":
        off = z["batch.offsets"]
        return [(pred[off[s]:off[s + 1], g], true[off[s]:off[s + 1], g]) for s in range(len(off) - 1)
                for g in range(pred.shape[1])]
    if name == "spots":
        return list(zip(pred, true))
    return [(pred[:, g], true[:, g]) for g in range(pred.shape[1])]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", CASES)
def test_integers_equal_brute_force_and_rankdata(z, name):
    for x, y in vectors(z, name)[::3]:
        ints = dict(zip(INT_NAMES, rr.integers(x, y)))
        n = x.size
        rx, ry = stats.rankdata(x), stats.rankdata(y)            # average ranks
        ax, ay = (2 * rx).astype(np.int64), (2 * ry).astype(np.int64)
        assert np.array_equal(ax, rr.ranks2(x)[0]) and np.array_equal(ay, rr.ranks2(y)[0])
        assert ints["n"] == n and ints["Sxy"] == int((ax * ay).sum())
        iu = np.triu_indices(n, 1)
        sx, sy = np.sign(x[:, None] - x[None, :])[iu], np.sign(y[:, None] - y[None, :])[iu]
        assert ints["s"] == int((sx * sy).sum()) and ints["joint"] == int(((sx == 0) & (sy == 0)).sum())
        for side, v in (("x", x), ("y", y)):
            t = np.unique(v, return_counts=True)[1].astype(object)
            assert ints["T" + side] == int((t ** 3 - t).sum()) and ints[side + "tie"] == int((t * (t - 1) // 2).sum())
            assert ints[side + "0"] == int((t * (t - 1) * (t - 2)).sum())
            assert ints[side + "1"] == int((t * (t - 1) * (2 * t + 5)).sum())
            assert ints[side + "tie"] == int((sx == 0).sum() if side == "x" else (sy == 0).sum())


@pytest.mark.parametrize("name", CASES + ("limit",))
def test_restatement_matches_scipy_fixture(z, name):
    """rho and tau within scipy's recorded deviation from the exact value plus 4 eps (three conversions, two square roots, a
    product and a division, |value| <= 1); the p-values within the bounds the t-based and the normal-tail p already have."""
    if name == "limit":
        res = [rr.finish(z["limit.ints"])]
        n_of = [16384]
    else:
        vs = vectors(z, name)
        res = [rr.finish(rr.integers(x, y)) for x, y in vs]
        n_of = [x.size for x, _ in vs]
    rho, tau, zs = (np.array(c) for c in zip(*res))
    want = {k: z[f"{name}.{k}"].reshape(-1) for k in ("rho", "rho_p", "tau", "tau_p")}
    for got, key in ((rho, "rho"), (tau, "tau")):
        assert np.array_equal(np.isnan(got), np.isnan(want[key]))
        ok = ~np.isnan(got)
        assert ok.sum() > 0 and np.abs(got[ok] - want[key][ok]).max() <= float(z[f"{name}.dev_{key}"]) + 4 * EPS
    assert float(z[f"{name}.dev_rho"]) <= 4 * EPS and float(z[f"{name}.dev_tau"]) <= 4 * EPS   # scipy is at rounding level
    # Spearman's p: Student's t on rho = the arithmetic of mcl_pearson_pvalue
    for n in sorted(set(n_of)):
        m = np.array(n_of) == n
        p, nl = pearson_pvalue(rho[m], n)
        ref = want["rho_p"][m]
        if n == 2:          # zero degrees of freedom: scipy's spearmanr gives NaN, the library pearsonr's rule, p = 1
            assert np.isnan(ref).all() and np.array_equal(p[~np.isnan(rho[m])], np.ones((~np.isnan(rho[m])).sum()))
            continue
        assert np.array_equal(np.isnan(p), np.isnan(ref))
        big = ~np.isnan(ref) & (ref >= P_FLOOR)
        if big.any():
            assert (np.abs(p[big] - ref[big]) / ref[big]).max() <= T_P_REL
            assert np.abs(nl[big] - (0.0 - np.log10(ref[big]))).max() <= 1e-9
        assert (p[~big & ~np.isnan(ref)] < 2 * P_FLOOR).all()
    # Kendall's p: the two-sided normal tail of z; NaN at n < 3, where scipy divides by zero
    tp, tnl = rr.normal_tail(zs, True)
    small = np.array(n_of) < 3
    assert np.isnan(tp[small]).all() and np.array_equal(np.isnan(tp[~small]), np.isnan(want["tau_p"][~small]))
    ok = ~np.isnan(tp) & (want["tau_p"] >= P_FLOOR)
    assert np.all(np.abs(tp[ok] - want["tau_p"][ok]) <= normal_p_bound(zs[ok], want["tau_p"][ok]))
    assert np.all(np.isfinite(tnl[~np.isnan(tp)]))


def test_edge_values():
    v = rr.vector_stats([1.0, 2.0], [3.0, 1.0])                         # n = 2: tau defined, Kendall p NaN, Spearman p = 1
    assert (v["rho"], v["tau"], v["rho_p"]) == (-1.0, -1.0, 1.0) and np.isnan(v["tau_p"])
    v = rr.vector_stats([1.0, 1.0, 1.0], [3.0, 1.0, 2.0])               # a constant side
    assert all(np.isnan(v[k]) for k in ("rho", "rho_p", "tau", "tau_p", "tau_nl"))
    a = np.array([0.0, -0.0, 1.0, 0.0]), np.array([3.0, 1.0, 2.0, 5.0])
    assert rr.integers(*a) == rr.integers(np.abs(a[0]), a[1])           # -0.0 ties +0.0
    x = np.array([0.5, 2.0, 2.0, 7.0, -1.0])
    v = rr.vector_stats(x, x)
    assert (v["rho"], v["tau"], v["rho_p"]) == (1.0, 1.0, 0.0) and np.isposinf(v["rho_nl"])
    v = rr.vector_stats(x, -x)
    assert (v["rho"], v["tau"]) == (-1.0, -1.0)
    assert rr.summary(np.array([0.5, np.nan, 0.25, 1.0]), np.array([0.5, np.nan, 0.0, 1.0]), [3, 0]) == \
        (0.75, (0.5 + 0.25 + 1.0) / 3.0, 0.75, 0.5, 3)


def test_reference_get_R_values_are_scipys(z):
    """The reference's own get_R(..., func=spearmanr), stored where the fixture was generated beside the reference, is
    scipy column by column (dim=1) and row by row (dim=0)."""
    assert "ref.r1" in z.files, "the committed fixture is generated beside the reference"
    s = int(z["ref.slide"])
    assert np.array_equal(z["ref.r1"], z["batch.rho"][s], equal_nan=True)
    assert np.array_equal(z["ref.p1"], z["batch.rho_p"][s], equal_nan=True)
    assert np.array_equal(z["ref.r0"], z["spots.rho"], equal_nan=True)
    assert np.array_equal(z["ref.p0"], z["spots.rho_p"], equal_nan=True)


# ------------------------------------------------------------------------------------------------ the library's checks
def test_rank_entry_points_reject_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib, rank
    lib = _lib.load()
    assert _lib.ABI_VERSION == 13 and lib.mcl_abi_version() == 13       # entry points were only added
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def stats_(pred=P, ldp=8, dp=0, true=P, ldt=8, dt=0, off=P, S=2, rows=20, G=8, max_n=12, axis=0, tau=1, ints=P, st=P):
        return lib.mcl_rank_stats(pred, ldp, dp, true, ldt, dt, off, S, rows, G, max_n, axis, tau, ints, st, None)

    for kw in ({"pred": None}, {"true": None}, {"off": None}, {"ints": None}, {"st": None}, {"dp": 2}, {"dt": -1},
               {"axis": 2}, {"G": 0}, {"G": 16385}, {"ldp": 7}, {"ldt": 7}, {"S": 0}, {"S": 65536}, {"max_n": 1},
               {"max_n": 16385}, {"max_n": 8193, "dt": 1}, {"max_n": 8193, "dp": 1}, {"rows": 1}, {"rows": 25},
               {"axis": 1, "S": 1, "max_n": 8, "G": 1, "ldp": 8}, {"axis": 1, "S": 2, "max_n": 8},
               {"axis": 1, "S": 1, "max_n": 9}):
        assert stats_(**kw) == -1, kw
    assert lib.mcl_rank_finish(None, 4, 1, P, P, P, P, None) == -1 and lib.mcl_rank_finish(P, 4, 1, None, P, P, P, None) == -1
    assert lib.mcl_rank_finish(P, 4, 1, P, None, P, P, None) == -1 and lib.mcl_rank_finish(P, 0, 0, P, None, None, None, None) == -1
    for args in ((None, P, P, 2, 8, 4, P), (P, P, None, 2, 8, 4, P), (P, P, P, 2, 8, 4, None), (P, P, P, 0, 8, 4, P),
                 (P, P, P, 2, 8, 9, P), (P, P, P, 2, 8, 0, P), (P, P, P, 2, 16385, 4, P), (P, P, P, 65536, 8, 4, P)):
        assert lib.mcl_rank_summary(*args, None) == -1, args
    # the limits the Python layer states are the library's
    import torch
    f32, f64 = torch.float32, torch.float64
    assert lib.mcl_rank_max_elements(0, 0) == rank.max_elements(f32, f32) == rank.MAX_ELEMENTS_F32 == 16384
    for a, b in ((0, 1), (1, 0), (1, 1)):
        assert lib.mcl_rank_max_elements(a, b) == rank.MAX_ELEMENTS_F64 == 8192
    assert rank.max_elements(f32, f64) == rank.max_elements(f64, f32) == rank.max_elements(f64, f64) == 8192
    assert lib.mcl_rank_max_elements(2, 0) == -1
    assert lib.mcl_rank_columns(16384, 0, 0) == 1 and lib.mcl_rank_columns(8192, 1, 0) == 1
    assert lib.mcl_rank_columns(16385, 0, 0) == -1 and lib.mcl_rank_columns(8193, 0, 1) == -1 and lib.mcl_rank_columns(1, 0, 0) == -1
    assert lib.mcl_rank_columns(2, 0, 0) == 32 and lib.mcl_rank_columns(1025, 0, 0) == 4 and lib.mcl_rank_columns(1025, 0, 1) == 2
    assert rank.N_INTS == len(rank.INT_NAMES) == len(INT_NAMES) and rank.INT_NAMES == INT_NAMES


def test_value_errors_come_before_the_device(monkeypatch):
    import torch
    from mclstexp_amd import rank
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # anything that gets past the checks says so
    a = np.zeros((5, 3), np.float32)
    for preds, trues in (([a], [np.zeros((5, 4), np.float32)]), ([a, np.zeros((1, 3))], [a, np.zeros((1, 3))]), ([], []),
                         ([a], [a, a]), ([np.zeros((16385, 1), np.float32)], [np.zeros((16385, 1), np.float32)]),
                         ([np.zeros((8193, 1))], [np.zeros((8193, 1), np.float32)]),
                         ([np.zeros((4, 16385), np.float32)], [np.zeros((4, 16385), np.float32)])):
        with pytest.raises(ValueError):
            rank.score_folds(preds, trues)
    with pytest.raises(ValueError, match="16384"):
        rank.score(np.zeros((16385, 2), np.float32), np.zeros((16385, 2), np.float32))
    with pytest.raises(ValueError, match="8192"):
        rank.get_R(np.zeros((8193, 2)), np.zeros((8193, 2)))
    with pytest.raises(ValueError, match="bool"):
        rank.score_folds([a], [a], tau=1)
    for kw in ({"func": "pearsonr"}, {"dim": 2}, {"dim": True}):
        with pytest.raises(ValueError):
            rank.get_R(a, a, **kw)
    with pytest.raises(ValueError, match="genes"):
        rank.spot_rank(np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32))
    with pytest.raises(ValueError):
        rank.spot_rank(a, np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match="axis"):
        rank.check_limits([5], 3, torch.float32, torch.float32, "rows")
    for call in (lambda: rank.score_folds([a], [a]), lambda: rank.score(a, a, tau=False), lambda: rank.spot_rank(a, a),
                 lambda: rank.get_R(a, a, dim=0, func=stats.spearmanr), lambda: rank.get_R(a, a, func="kendalltau"),
                 lambda: rank.score(np.zeros((16384, 1), np.float32), np.zeros((16384, 1), np.float32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_arguments():
    from mclstexp_amd import rank
    a = rank.parse_args(["--pred", "p1.npy", "p2.npy", "--true", "t1.npy", "t2.npy"])
    assert (a.pred, a.true, a.genes, a.no_tau, a.spots, a.top, a.json, a.out_dir) == \
        (["p1.npy", "p2.npy"], ["t1.npy", "t2.npy"], None, False, False, 7, None, None)
    a = rank.parse_args(["--pred", "p.npy", "--true", "t.npy", "--genes", "g.npy", "--no_tau", "--spots", "--top", "3",
                         "--json", "o.json", "--out_dir", "d"])
    assert (a.genes, a.no_tau, a.spots, a.top, a.json, a.out_dir) == ("g.npy", True, True, 3, "o.json", "d")
    for bad in (["--pred", "p.npy"], ["--true", "t.npy"], ["--pred", "p1.npy", "p2.npy", "--true", "t.npy"],
                ["--pred", "p.npy", "--true", "t.npy", "--top", "0"]):
        with pytest.raises(SystemExit):
            rank.parse_args(bad)


def test_report_and_top_genes_on_canned_results():
    from mclstexp_amd import rank
    folds = [{"heg_spearman": 0.5, "hvg_spearman": 0.25, "heg_kendall": 0.375, "hvg_kendall": 0.125,
              "spearman": np.array([0.5, np.nan, 0.9, 0.5])},
             {"heg_spearman": 0.75, "hvg_spearman": 0.5, "heg_kendall": 0.5, "hvg_kendall": 0.25,
              "spearman": np.array([0.7, np.nan, 0.1, 0.7])}]
    res = {"folds": folds, "heg_spearman": 0.625, "hvg_spearman": 0.375, "heg_kendall": 0.4375, "hvg_kendall": 0.1875}
    assert rank.format_report(res).splitlines() == [
        "fold 0: heg spearman: 0.5000, hvg spearman: 0.2500, heg kendall: 0.3750, hvg kendall: 0.1250",
        "fold 1: heg spearman: 0.7500, hvg spearman: 0.5000, heg kendall: 0.5000, hvg kendall: 0.2500",
        "avg heg spearman: 0.6250", "avg hvg spearman: 0.3750", "avg heg kendall: 0.4375", "avg hvg kendall: 0.1875"]
    assert rank.format_report(res, tau=False).splitlines() == [
        "fold 0: heg spearman: 0.5000, hvg spearman: 0.2500", "fold 1: heg spearman: 0.7500, hvg spearman: 0.5000",
        "avg heg spearman: 0.6250", "avg hvg spearman: 0.3750"]
    top = rank.top_genes(res, ["A", "B", "C", "D"], 3)
    assert [(t["gene"], t["gene_name"], t["best_slide"]) for t in top] == [(0, "A", 1), (3, "D", 1), (2, "C", 0)]
    assert abs(top[0]["mean_spearman"] - 0.6) < 1e-15 and top[2]["mean_spearman"] == 0.5
    assert [t["gene"] for t in rank.top_genes(res, None, 9)] == [0, 3, 2, 1]            # the undefined gene last
    assert rank.format_top(top[:1]) == ["Gene: A, mean Spearman rho: 0.6000, best in slide 1"]
