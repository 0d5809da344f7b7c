"""CPU: the numpy restatement tests/ligrec_reference.py against the fixture tests/golden/ligrec.npz (an independent
statement by pandas ``groupby``, plain loops and ``scipy.stats.false_discovery_control``), the host-side rules of
mclstexp_amd.ligrec, ``resolve_pairs``, the complex policies and the CLI parser.

On the quantised cases (values multiples of 2^-12 below 16) every sum is exact in fp64 in any order, so the restatement
must equal the independent statement exactly.  On the continuous case a group mean of m spots carries (m + 1) eps of either
side's own rounding; the comparison allows 2 (m + 1) eps with m the slide's n."""
import numpy as np
import pytest
import torch

import ligrec_reference as lr
from golden import gen_ligrec_goldens as gen
from mclstexp_amd import ligrec as lg

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(lr.GOLDEN))


def case(golden, name):
    n, K = gen.CASES[name][:2]
    return golden[f"{name}.x"], golden[f"{name}.labels"].astype(np.int64), golden[f"{name}.perms"].astype(np.int64), K


# ------------------------------------------------------------------------------------------------ the restatement
def test_fixture_regenerates_identically(golden):
    again = gen.build()
    assert sorted(again) == sorted(golden)
    for key, v in again.items():
        assert np.array_equal(np.asarray(v), golden[key], equal_nan=np.asarray(v).dtype.kind == "f"), key
    for name, (n, K, seed, quantised, empty, single) in gen.CASES.items():
        x, labels = lr.make_slide(n, K, seed, quantised=quantised, empty=empty, single=single)
        assert np.array_equal(x, golden[f"{name}.x"]) and np.array_equal(labels, golden[f"{name}.labels"])


@pytest.mark.parametrize("name", ["q_two", "q_seven"])
def test_restatement_is_the_pandas_statement_exactly(golden, name):
    x, labels, perms, K = case(golden, name)
    r = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=gen.THRESHOLD, perms=list(perms))
    for key in ("means", "count", "pvalues", "defined", "pvalues_adj"):
        assert np.array_equal(r[key], golden[f"{name}.{key}"], equal_nan=key != "defined" and key != "count"), key
    assert np.array_equal(lr.adjust(r["pvalues"], "interactions"), golden[f"{name}.pvalues_adj_interactions"], equal_nan=True)
    used = r["used_genes"]
    assert np.array_equal(r["group_means"], golden[f"{name}.group_means"][:, used], equal_nan=True)
    assert np.array_equal(r["group_frac"], golden[f"{name}.group_frac"][:, used], equal_nan=True)
    assert np.array_equal(r["interactions"], golden[f"{name}.picked"])
    # the recorded tables are the pure function of (seed, p, n)
    assert np.array_equal(perms, lr.sr.permutations(gen.PERM_SEED, gen.PERM_P, r["n"]))
    assert np.isfinite(r["pvalues"]).any() and np.isnan(r["pvalues"]).any()


def test_edge_cases_of_the_quantised_fixture(golden):
    x, labels, perms, K = case(golden, "q_seven")
    r = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=0.1, perms=list(perms))
    assert (labels == -1).any() and r["n"] == (labels >= 0).sum()
    assert r["sizes"][3] == 0 and r["sizes"][6] == 1 and r["sizes"][0] == 20
    assert np.isnan(r["means"][:, 3, :]).all() and np.isnan(r["means"][:, :, 3]).all() and not r["defined"][:, 3].any()
    assert np.array_equal(r["means"][0], r["means"][3], equal_nan=True) and np.array_equal(r["count"][0], r["count"][3])
    u11, u10 = np.searchsorted(r["used_genes"], 11), np.searchsorted(r["used_genes"], 10)
    assert (r["sum"][:, u11] == 0).all() and not r["defined"][4].any()          # the gene that is zero everywhere
    live = np.arange(K) != 3
    assert (r["means"][4][np.ix_(live, live)] == 0).all()
    assert r["nnz"][0, u10] == 2 and r["expressed"][0, u10]                     # exactly threshold * size
    strict = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=0.1000001, perms=list(perms[:2]))
    assert not strict["expressed"][0, u10]
    none = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=0.0, perms=list(perms[:2]))
    assert none["expressed"].all()
    # the identity permutation reproduces the observed values: every comparison holds
    ident = lr.ligrec(x, labels, lr.INTERACTIONS, K, perms=[np.arange(r["n"])] * 3)
    assert (ident["count"][np.isfinite(ident["means"])] == 3).all()
    assert np.isnan(lr.ligrec(x, labels, lr.INTERACTIONS, K, n_perms=0)["pvalues"]).all()


def test_continuous_case_within_its_bound(golden):
    x, labels, perms, K = case(golden, "cont")
    r = lr.ligrec(x, labels, lr.INTERACTIONS, K, threshold=gen.THRESHOLD, perms=list(perms))
    tol = 2 * (r["n"] + 1) * EPS
    assert float(golden["cont.err_means"]) <= tol
    want = golden["cont.means"]
    assert np.array_equal(np.isnan(r["means"]), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(r["means"][ok] - want[ok]) <= tol * np.abs(want[ok]))
    assert np.array_equal(r["defined"], golden["cont.defined"])


def test_segment_sum_order():
    rng = np.random.default_rng(0)
    for m in (0, 1, 63, 64, 65, 200, 1025):
        v = rng.random((m, 3))
        acc = np.zeros((64, 3))
        for t in range(m):                                   # lane t % 64 adds position t, positions ascending
            acc[t % 64] = acc[t % 64] + v[t]
        for o in (32, 16, 8, 4, 2, 1):
            acc[:o] = acc[:o] + acc[o:2 * o]
        assert np.array_equal(lr.segment_sum(v), acc[0])
    assert lr.chain(1) == 7 and lr.chain(64) == 7 and lr.chain(65) == 8
    assert [lr.columns(n) for n in (0, 1, 2432, 2433, 4864, 4865, 9728, 9729, 16384)] == [8, 8, 8, 4, 4, 2, 2, 1, 1]


# ------------------------------------------------------------------------------------------------------ host rules
def test_argument_and_limit_errors_come_before_any_device_call():
    x, labels = lr.make_slide(37, 2, 1)
    ok = dict(x=x, labels=labels, interactions=lr.INTERACTIONS)

    def bad(match, **kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            lg.ligrec(**args)

    bad("2-D", x=x[0])
    bad("integer group ids", labels=labels.astype(np.float64))
    bad("labels", labels=labels[:-1])
    bad("n_perms", n_perms=-1)
    bad("n_perms", n_perms=lg.MAX_PERMS + 1)
    bad("n_perms", n_perms=2.5)
    bad("seed", seed=-1)
    bad("threshold", threshold=1.5)
    bad("threshold", threshold="a")
    bad("corr_axis", corr_axis="genes")
    bad("complex_policy", complex_policy="max")
    bad("return_permutations", return_permutations=1)
    bad("gene columns", interactions=[(0, 12)])
    bad("gene columns", interactions=[(0, -1)])
    bad("gene columns", interactions=[(0, 1.5)])
    bad("source, target", interactions=[(0, 1, 2)])
    bad("at least one", interactions=[])
    bad("empty complex", interactions=[((), 1)])
    bad("groups", k=256)
    bad("groups", k=0)
    bad("offsets", offsets=[0, 10])
    bad("every slide needs", offsets=[0, 1, 37])
    bad("permutations", permutations=[np.zeros((2, 5), dtype=np.int64)])
    bad("not a permutation", permutations=[np.zeros((2, int((labels >= 0).sum())), dtype=np.int64)])
    big = np.zeros((lg.MAX_ROWS + 1, 2))
    with pytest.raises(ValueError, match="every slide needs"):
        lg.ligrec(big, np.zeros(big.shape[0], dtype=np.int64), [(0, 1)])
    with pytest.raises(ValueError, match="genes per call"):
        lg.check_problem((10, lg.MAX_GENES + 1), None, 2, None, 1)
    with pytest.raises(ValueError, match="interactions x k"):
        lg.check_problem((600, 4), None, 255, None, 259)              # 259 * 255^2 > 2^24
    with pytest.raises(ValueError, match="interactions x k"):
        lg.check_problem((400, 4), np.arange(0, 401, 2), 100, None, 1100)   # 200 slides x 1.1e7 > 2^31
    with pytest.raises(ValueError, match="at most 65535 interactions"):
        lg.prepare_interactions([(0, 1)] * 65536, 4)
    with pytest.raises(ValueError, match="one label vector per slide"):
        lg.ligrec_slides([x], [labels, labels], lr.INTERACTIONS)
    with pytest.raises(ValueError, match="do not match"):
        lg.ligrec_slides([x], [labels[:-1]], lr.INTERACTIONS)
    with pytest.raises(ValueError, match="alpha"):
        lg.interaction_recovery([x], [x], [labels], lr.INTERACTIONS, alpha=0)
    with pytest.raises(ValueError, match="differ in shape"):
        lg.interaction_recovery([x], [x[:-1]], [labels], lr.INTERACTIONS)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present")
def test_no_cpu_fallback():
    x, labels = lr.make_slide(37, 2, 1)
    with pytest.raises(RuntimeError, match="no GPU available"):
        lg.ligrec(x, labels, lr.INTERACTIONS, n_perms=4)


def test_resolve_pairs():
    genes = ["TGFB1", "TGFBR1", "TGFBR2", "HLA_A", "CD8A", "CD8B", "EGFR"]
    pairs = [("TGFB1", "TGFBR1_TGFBR2"),      # a complex on the target side
             ("HLA_A", "CD8A_CD8B"),          # a panel name that holds the separator stays one gene
             ("TGFB1", "ERBB2"),              # outside the panel
             ("EGF_TGFB1", "EGFR"),           # a complex with a member outside the panel
             ("TGFB1", "TGFBR2_TGFBR1"),      # the first pair again, members in another order
             (" EGFR ", "EGFR"),
             ("CD8A_CD8A", "EGFR")]           # a complex of one distinct gene is that gene
    r = lg.resolve_pairs(pairs, genes)
    assert r["interactions"] == [(0, (1, 2)), (3, (4, 5)), (6, 6), (4, 6)]
    assert r["kept"].tolist() == [0, 1, 5, 6] and r["n_missing"] == 2 and r["n_duplicates"] == 1
    assert r["names"][2] == ("EGFR", "EGFR")
    with pytest.raises(ValueError, match="source, target"):
        lg.resolve_pairs([("a", "b", "c")], genes)
    assert lg.resolve_pairs([], genes)["interactions"] == []


def test_read_pairs(tmp_path):
    f = tmp_path / "pairs.tsv"
    f.write_text("source\ttarget\n# comment\nTGFB1\tTGFBR1_TGFBR2\n\nEGFR\tEGFR\textra\n")
    assert lg.read_pairs(str(f)) == [("TGFB1", "TGFBR1_TGFBR2"), ("EGFR", "EGFR")]
    f.write_text("A,B\n")
    assert lg.read_pairs(str(f)) == [("A", "B")]
    f.write_text("lonely\n")
    with pytest.raises(ValueError, match="two columns"):
        lg.read_pairs(str(f))


def test_complex_policies(golden):
    sides, used, moff, members = lg.prepare_interactions(lr.INTERACTIONS, lr.G, "min")
    assert len(sides) == 9 and sides == lr.expand(lr.INTERACTIONS, "min")
    assert np.array_equal(used, lr.used_columns(sides)) and used.tolist() == list(range(12))
    assert moff.size == 19 and moff[-1] == members.size == 20
    assert members[moff[12]:moff[13]].tolist() == [7, 8] and members[moff[15]:moff[16]].tolist() == [1, 2]
    sides_all, used_all, moff_all, members_all = lg.prepare_interactions(lr.INTERACTIONS, lr.G, "all")
    assert len(sides_all) == 11 and sides_all == lr.expand(lr.INTERACTIONS, "all")
    assert sides_all[6:10] == [((7,), (9,)), ((8,), (9,)), ((3,), (1,)), ((3,), (2,))]
    assert np.array_equal(np.diff(moff_all), np.ones(22, dtype=np.int32))
    # a sparse set of genes: positions in ``used``, not gene columns
    _, used2, moff2, members2 = lg.prepare_interactions([((9, 4), 7)], 12, "min")
    assert used2.tolist() == [4, 7, 9] and members2.tolist() == [0, 2, 1]
    # "min" takes the member of lowest overall mean; "all" holds both of its members' rows
    x, labels, perms, K = case(golden, "q_two")
    rmin = lr.ligrec(x, labels, lr.INTERACTIONS, K, perms=list(perms[:4]), complex_policy="min")
    rall = lr.ligrec(x, labels, lr.INTERACTIONS, K, perms=list(perms[:4]), complex_policy="all")
    overall = x[labels >= 0].mean(axis=0)
    assert rmin["interactions"][6].tolist() == [7 if overall[7] <= overall[8] else 8, 9]
    assert rmin["interactions"][7].tolist() == [3, 1 if overall[1] <= overall[2] else 2]
    pick = 6 + (0 if overall[7] <= overall[8] else 1)
    assert np.array_equal(rall["means"][pick], rmin["means"][6]) and np.array_equal(rall["count"][pick], rmin["count"][6])
    assert rall["means"].shape == (11, K, K)


def test_bh_and_top_interactions():
    from scipy import stats
    rng = np.random.default_rng(5)
    p = rng.random((6, 3, 3))
    p[rng.random(p.shape) < 0.3] = np.nan
    p[2] = np.nan
    for axis in ("clusters", "interactions"):
        got = lg.adjust(p, axis)
        assert np.array_equal(got, lr.adjust(p, axis), equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(p))
    row = p[0][np.isfinite(p[0])]
    assert np.allclose(lg.adjust(p, "clusters")[0][np.isfinite(p[0])], stats.false_discovery_control(row), rtol=0, atol=0)
    assert np.isnan(lg.adjust(p, None)).all()
    res = [{"pvalues": np.array([[[0.5, 0.0], [0.0, np.nan]], [[0.0, 0.2], [np.nan, 0.0]]]),
            "means": np.array([[[1.0, 2.0], [3.0, 9.0]], [[3.0, 1.0], [1.0, 0.5]]])}]
    top = lg.top_interactions(res, 0, 5)
    assert top.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 1, 1], [1, 0, 1]]      # p, then larger mean, then index
    assert np.array_equal(top, lr.top_interactions(res[0], 5))
    assert lg.top_interactions(res, 0, 100).shape == (6, 3) and lg.top_interactions(res, 0, 0).shape == (0, 3)


def test_cli_argument_errors(capsys):
    base = ["--pred", "a.npy", "--labels", "l.npy", "--pairs", "p.tsv", "--genes", "g.npy"]
    a = lg.parse_args(base)
    assert (a.n_perms, a.threshold, a.seed, a.alpha, a.top, a.corr_axis, a.out_dir) == (1000, 0.1, 0, 0.05, 10, "clusters", None)
    assert lg.parse_args(base + ["--corr_axis", "none"]).corr_axis is None
    for extra in (["--labels", "l.npy", "m.npy"], ["--true", "t.npy", "u.npy"], ["--n_perms", "-1"], ["--n_perms", "70000"],
                  ["--threshold", "2"], ["--seed", "-3"], ["--alpha", "0"], ["--top", "0"], ["--complex_policy", "max"]):
        with pytest.raises(SystemExit):
            lg.parse_args(base + extra)
    for missing in ("--pred", "--labels", "--pairs", "--genes"):
        i = base.index(missing)
        with pytest.raises(SystemExit):
            lg.parse_args(base[:i] + base[i + 2:])
    capsys.readouterr()
