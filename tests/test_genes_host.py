"""CPU: the host side of mclstexp_amd.genes -- C-side argument validation of its two entry points, the CLI's arguments and
file layout, the ``evaluate --save_pred`` plumbing -- and the in-test fp64 restatement (tests/genes_reference.py) against
the reference's own p-values, mpmath and pandas (tests/golden/gene_significance.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from genes_reference import (GENE_CASES, GOLDEN, TOP_N, UNDERFLOW_CASE, format_line, pearson_pvalue, reference_neglog10,
                             significance, stable_order, tutorial_table)
from mclstexp_amd import synth

P_FLOOR = 1e-290
TABLE_CASES = sorted(set(GENE_CASES) - {UNDERFLOW_CASE})


def test_pearson_pvalue_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_pearson_pvalue
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def call(r=P, off=P, S=2, G=8, p=P, nl=P):
        return fn(r, off, S, G, p, nl, None)

    for kw in ({"r": None}, {"off": None}, {"p": None}, {"nl": None}, {"S": 0}, {"S": -1}, {"G": 0}, {"G": -5}):
        assert call(**kw) == -1, kw
    assert call(S=65536) == -2
    assert call(G=1048577) == -2


def test_gene_rank_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_gene_rank
    P = C.c_void_p(64)

    def call(nl=P, r=P, S=2, G=8, top_n=7, mean=P, nd=P, order=P, slide=P, value=P, br=P):
        return fn(nl, r, S, G, top_n, mean, nd, order, slide, value, br, None)

    for kw in ({"nl": None}, {"r": None}, {"mean": None}, {"nd": None}, {"order": None}, {"slide": None}, {"value": None},
               {"br": None}, {"S": 0}, {"G": 0}, {"G": -1}, {"top_n": 0}, {"top_n": 9}):
        assert call(**kw) == -1, kw
    assert call(S=65536) == -2
    assert call(G=1048577) == -2


def test_abi_version_is_unchanged():
    from mclstexp_amd import _lib
    assert _lib.ABI_VERSION == 13 and _lib.load().mcl_abi_version() == 13   # entry points were only added


def test_no_gpu_raises(monkeypatch):
    import torch
    from mclstexp_amd import genes
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.arange(12.0).reshape(4, 3) ** 2
    for call in (lambda: genes.gene_significance([x], [x + 1]), lambda: genes.significance_table([x], [x + 1]),
                 lambda: genes.rank_genes(np.ones((2, 3)), np.ones((2, 3))),
                 lambda: genes.pvalues_device(torch.ones((1, 3), dtype=torch.float64), [0, 4])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_slide_lists_are_checked_before_the_device():
    from mclstexp_amd import genes
    a = np.zeros((5, 3))
    for preds, trues in (([a], [np.zeros((5, 4))]), ([a, np.zeros((4, 2))], [a, np.zeros((4, 2))]),
                         ([a, np.zeros((1, 3))], [a, np.zeros((1, 3))]), ([], []), ([a], [a, a])):
        with pytest.raises(ValueError):
            genes.gene_significance(preds, trues)
    with pytest.raises(ValueError, match="slide names"):
        genes.significance_table([a, a], [a, a], slide_names=["A1"])
    with pytest.raises(ValueError, match="gene names"):
        genes.significance_table([a], [a], gene_names=["x", "y"])


def test_cli_arguments():
    from mclstexp_amd import genes
    a = genes.parse_args(["--pred", "p1.npy", "p2.npy", "--true", "t1.npy", "t2.npy"])
    assert (a.pred, a.true, a.genes, a.slides, a.top, a.reference_inf, a.csv) == \
        (["p1.npy", "p2.npy"], ["t1.npy", "t2.npy"], None, None, 7, False, None)
    a = genes.parse_args(["--pred", "p.npy", "--true", "t.npy", "--genes", "g.npy", "--slides", "A2", "--top", "3",
                          "--reference_inf", "--csv", "o.csv"])
    assert (a.genes, a.slides, a.top, a.reference_inf, a.csv) == ("g.npy", ["A2"], 3, True, "o.csv")
    for bad in (["--pred", "p.npy"], ["--true", "t.npy"], ["--pred", "p1.npy", "p2.npy", "--true", "t.npy"],
                ["--pred", "p.npy", "--true", "t.npy", "--slides", "A", "B"],
                ["--pred", "p.npy", "--true", "t.npy", "--top", "0"]):
        with pytest.raises(SystemExit):
            genes.parse_args(bad)


def test_cli_file_layout_checks(tmp_path):
    from mclstexp_amd import genes
    rng = np.random.default_rng(0)
    G, sizes = 9, [5, 7]
    pp, tp = [], []
    for i, n in enumerate(sizes):
        pp.append(str(tmp_path / f"p{i}.npy")), tp.append(str(tmp_path / f"t{i}.npy"))
        np.save(pp[-1], rng.random((G, n)).astype(np.float32))     # stored (G, N), as the reference stores them
        np.save(tp[-1], rng.random((G, n)).astype(np.float32))
    preds, trues = genes.load_slides(pp, tp)
    assert [p.shape for p in preds] == [(n, G) for n in sizes] and [t.shape for t in trues] == [(n, G) for n in sizes]
    assert np.array_equal(preds[1], np.load(pp[1]).T)
    np.save(str(tmp_path / "names.npy"), np.array([f"GENE{g}" for g in range(G)], dtype=object))
    assert genes.load_gene_names(str(tmp_path / "names.npy"), G)[:2] == ["GENE0", "GENE1"]
    assert genes.load_gene_names(None, G) is None
    with pytest.raises(ValueError, match="gene names"):
        genes.load_gene_names(str(tmp_path / "names.npy"), G + 1)
    np.save(tp[1], np.zeros((G, 6), np.float32))                   # spot counts disagree
    with pytest.raises(ValueError, match="expected \\(9, 7\\)"):
        genes.load_slides(pp, tp)
    np.save(pp[1], np.zeros((G + 1, 7), np.float32))               # gene counts disagree
    with pytest.raises(ValueError, match="expected \\(G, N\\)"):
        genes.load_slides(pp, tp)
    with pytest.raises(FileNotFoundError):
        genes.load_slides([str(tmp_path / "nope.npy")], tp[:1])


def test_top_lines_and_csv(tmp_path):
    from mclstexp_amd import genes
    res = {"top": [{"gene": 2, "gene_name": "ERBB2", "slide_name": "B1", "best_value": 173.25, "pcc": 0.5, "mean": 9.0}],
           "neglog10p": np.array([[1.0, np.nan, 3.0], [0.5, np.nan, np.inf]]), "mean": np.array([0.75, np.nan, np.inf]),
           "order": np.array([2, 0, 1]), "gene_names": ["A", "B", "ERBB2"], "slide_names": ["A1", "B1"]}
    assert genes.format_top(res) == [format_line("ERBB2", "B1", 173.25, 0.5)]
    assert genes.format_top(res) == ["Gene: ERBB2, Max -log(p-value) in B1: 173.25, PCC in B1: 0.5"]
    genes.write_csv(str(tmp_path / "t.csv"), res)
    assert open(tmp_path / "t.csv").read().splitlines() == [",A1,B1,avg_p_value", "ERBB2,3.0,inf,inf", "A,1.0,0.5,0.75",
                                                            "B,,,"]


def test_save_pred_plumbing(tmp_path):
    """``evaluate --save_pred``: the option, and the files it writes are what ``genes --pred`` reads back."""
    from mclstexp_amd import evaluate, genes
    base = ["--dataset", "her2st", "--embedding_dir", "d", "--expressions", "a.npy"]
    assert evaluate.parse_args(base).save_pred is None
    assert evaluate.parse_args(base + ["--save_pred", "out"]).save_pred == "out"
    rng = np.random.default_rng(1)
    preds = [rng.random((n, 6)).astype(np.float32) for n in (4, 9, 5)]
    paths = evaluate.save_predictions(str(tmp_path / "pred"), preds)
    assert paths == [os.path.join(str(tmp_path / "pred"), str(i), "matched_spot_expression_pred_mclSTExp.npy")
                     for i in range(3)]
    assert [np.load(f).shape for f in paths] == [(6, 4), (6, 9), (6, 5)]
    back, _ = genes.load_slides(paths, paths)
    assert all(np.array_equal(b, p) for b, p in zip(back, preds))
    with pytest.raises(ValueError):
        evaluate.save_predictions(str(tmp_path / "bad"), [np.zeros(3)])
    import inspect
    assert inspect.signature(evaluate.leave_one_slide_out).parameters["return_preds"].default is False


# --------------------------------------------------------------------------- the restatement against the fixture
@pytest.mark.parametrize("name", sorted(GENE_CASES))
def test_restatement_matches_reference_fixture(name):
    """tests/genes_reference.py against scipy's p (through the reference's get_R) and mpmath's -log10 p, within the errors
    the generator recorded for it: pins the restatement and the tolerances the GPU tests derive from it."""
    z = np.load(GOLDEN)
    d = synth.make_eval_case(**GENE_CASES[name])
    off = d["offsets"]
    p_ref, nl_mp = z[f"{name}.p"], z[f"{name}.nl_mp"]
    r, p, nl = significance(d["pred"], d["true"], off)
    alone = [pearson_pvalue(z[f"{name}.r"][s], int(off[s + 1] - off[s])) for s in range(len(off) - 1)]
    for key, pp, nn in (("restatement", p, nl), ("kernel", np.stack([a[0] for a in alone]), np.stack([a[1] for a in alone]))):
        assert np.array_equal(np.isnan(pp), np.isnan(p_ref)) and np.array_equal(np.isnan(nn), np.isnan(nl_mp))
        assert np.array_equal(np.isposinf(nn), np.isposinf(nl_mp))
        big = ~np.isnan(p_ref) & (p_ref >= P_FLOOR)
        fin = np.isfinite(nl_mp)
        # (libm may differ by an ulp between machines: 2 x what the generating machine measured)
        assert (np.abs(pp[big] - p_ref[big]) / p_ref[big]).max() <= 2 * float(z[f"{name}.{key}_p_rel"])
        assert np.abs(nn[fin] - nl_mp[fin]).max() <= 2 * float(z[f"{name}.{key}_nl_abs"])
        assert (pp[~big & ~np.isnan(p_ref)] < 2 * P_FLOOR).all()      # the underflowing rest: 0 or next to it


def test_recorded_errors_are_the_algorithms_rounding():
    """The p-value algorithm alone is at the prototype's level (eps * lgamma(2a): ~5e-12 relative at n = 4784, below 1e-12
    at HER2ST sizes); the end-to-end figures are larger only by the last-digit difference between two ways of computing
    r, amplified by d log p / d r."""
    z = np.load(GOLDEN)
    assert float(z["tenx.kernel_p_rel"]) < 1e-11 and float(z["tenx.kernel_nl_abs"]) < 1e-11
    for name in TABLE_CASES:
        assert float(z[f"{name}.kernel_p_rel"]) < 1e-12 and float(z[f"{name}.kernel_nl_abs"]) < 2e-13
    for name in GENE_CASES:
        assert float(z[f"{name}.restatement_p_rel"]) < 1e-10


def test_known_values():
    """The underflow finding: n = 4784, r = 0.6 -> scipy's p is 0 (-log10 p = inf); mpmath at 60 digits gives
    465.1398821221 (and 474.9653314083 at r = 0.605)."""
    p, nl = pearson_pvalue(np.array([0.6, -0.6, 0.0, 1.0, -1.0, np.nan, 0.605]), 4784)
    assert p[0] == 0.0 and abs(nl[0] - 465.1398821221) < 1e-9 and nl[1] == nl[0] and abs(nl[6] - 474.9653314083) < 1e-9
    assert abs(p[2] - 1.0) < 2e-11 and 0.0 <= nl[2] < 1e-11      # r = 0: 1 up to eps * lgamma(2a), never above
    assert (p[3:5] == 0.0).all() and np.isposinf(nl[3:5]).all() and np.isnan(p[5]) and np.isnan(nl[5])
    p2, nl2 = pearson_pvalue(np.array([1.0, -1.0, np.nan]), 2)
    assert p2[:2].tolist() == [1.0, 1.0] and nl2[:2].tolist() == [0.0, 0.0] and np.isnan(p2[2])
    p3, _ = pearson_pvalue(np.array([0.5]), 3)            # a = 1/2, the arcsine law: p = (4 / pi) asin(sqrt(1/4)) = 2/3
    assert abs(p3[0] - 2.0 / 3.0) < 1e-15


@pytest.mark.parametrize("name", TABLE_CASES)
def test_table_restatement_matches_pandas_fixture(name):
    z = np.load(GOLDEN)
    S, G = z[f"{name}.p"].shape
    genes, slides = [f"g{g}" for g in range(G)], [f"s{s}" for s in range(S)]
    _, mean, order, top = tutorial_table(reference_neglog10(z[f"{name}.p"]), z[f"{name}.r"], genes, slides, TOP_N)
    assert np.array_equal(np.isnan(mean), np.isnan(z[f"{name}.mean"]))
    assert np.allclose(mean, z[f"{name}.mean"], rtol=1e-14, atol=0, equal_nan=True)
    n_ok = int((~np.isnan(mean)).sum())
    assert np.array_equal(order[:n_ok], z[f"{name}.order"][:n_ok])
    assert np.array_equal(order[:n_ok], stable_order(mean)[:n_ok])
    assert [t[0] for t in top] == z[f"{name}.top_gene"].tolist() and [t[1] for t in top] == z[f"{name}.top_slide"].tolist()


def test_fixture_covers_the_edge_cases():
    z = np.load(GOLDEN)
    assert min(GENE_CASES["folds"]["segments"]) == 2 and (z["folds.p"][1][~np.isnan(z["folds.p"][1])] == 1.0).all()
    assert np.isnan(z["folds.r"]).any() and np.isnan(z["folds.mean"]).sum() >= 2          # constant columns
    assert z["her2st8.p"].shape == (8, 785)
    for name in TABLE_CASES:
        p = z[f"{name}.p"]
        assert np.nanmin(p) >= P_FLOOR
        m = np.sort(z[f"{name}.mean"][~np.isnan(z[f"{name}.mean"])])[::-1]
        assert -np.diff(m[:TOP_N + 1]).max() > 1e-6       # the top order rests on neither rounding nor the sort's tie rule
        assert -np.diff(m).max() > 1e-9                   # ... and nor does the rest
        for g, v in zip(z[f"{name}.top_gene"], z[f"{name}.top_value"]):
            assert z[f"{name}.mean"][g] < v               # idxmax over a row that also holds avg_p_value names a slide
    p = z["tenx.p"]
    assert (p == 0.0).sum() >= 20 and np.isfinite(z["tenx.nl_mp"]).all() and z["tenx.nl_mp"].max() > 2000
    assert 0 < z["tenx.inf_genes"].size < p.shape[1]
    assert os.path.getsize(GOLDEN) < 1 << 20
