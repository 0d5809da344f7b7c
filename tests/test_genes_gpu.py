"""Gene significance on the MI355X (mclstexp_amd.genes, csrc/gene_significance.hip) against the reference's own p-values
(scipy through its get_R), mpmath's -log10 p and pandas' table (tests/golden/gene_significance.npz), and the fp64
restatement (tests/genes_reference.py).  pytest -m gpu.

Tolerances are derived, not chosen: the fixture records the restatement's own largest error per case, and the device may
take 4 x that (its lgamma / log / log1p are specified to a few ulp where libm's are below one, and the error is a
cancelling sum of three such terms), plus 1e-290 absolute on p so that the subnormal elements compare.  As generated:

  case      restatement_p_rel  restatement_nl_abs   kernel_p_rel  kernel_nl_abs
  folds         1.023e-11          4.405e-12          4.726e-13     8.527e-14
  her2st8       1.578e-11          6.821e-12          7.606e-13     1.137e-13
  tenx          2.881e-11          8.527e-10          5.484e-12     2.728e-12

``restatement_*``: end to end from the expression matrices (r computed in two passes, which differs from scipy's r in the
last digits; d log p / d r ~ 1e4 .. 1e5 at these r ~ 0.95 amplifies that) -- the bound of the end-to-end tests.
``kernel_*``: the p-value algorithm alone, fed the reference's own r -- the bound of the tests that hand
``mcl_pearson_pvalue`` the fixture's r (eps * lgamma(2a): ~5e-12 relative at n = 4784)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eval_reference import write_layout
from genes_reference import (GENE_CASES, GOLDEN, TOP_N, UNDERFLOW_CASE, format_line, reference_neglog10, significance,
                             stable_order, tutorial_table)
from mclstexp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_ABS = 1e-290
TABLE_CASES = sorted(set(GENE_CASES) - {UNDERFLOW_CASE})


@pytest.fixture(scope="module")
def gn():
    from mclstexp_amd import _lib, genes
    _lib.lib()  # must load: no fallback
    return genes


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _slides(name, dtype=np.float64):
    d = synth.make_eval_case(**GENE_CASES[name])
    off = d["offsets"]
    p, t = d["pred"].astype(dtype), d["true"].astype(dtype)
    return ([p[off[s]:off[s + 1]] for s in range(len(off) - 1)], [t[off[s]:off[s + 1]] for s in range(len(off) - 1)], off)


def _check_p(got_p, got_nl, p_ref, nl_ref, p_rel, nl_abs, what):
    """NaN and +inf positions equal; p within p_rel relative + 1e-290; -log10 p within nl_abs wherever nl_ref is finite."""
    assert np.array_equal(np.isnan(got_p), np.isnan(p_ref)), f"{what}: NaN positions of p"
    assert np.array_equal(np.isnan(got_nl), np.isnan(nl_ref)), f"{what}: NaN positions of -log10 p"
    assert np.array_equal(np.isposinf(got_nl), np.isposinf(nl_ref)), f"{what}: +inf positions"
    ok = ~np.isnan(p_ref)
    err_p = np.abs(got_p[ok] - p_ref[ok]) - P_ABS
    worst_p = float((err_p / np.maximum(p_ref[ok], 1e-300)).max())
    fin = np.isfinite(nl_ref)
    worst_nl = float(np.abs(got_nl[fin] - nl_ref[fin]).max())
    print(f"{what}: p rel err {worst_p:.3e} (bound {p_rel:.3e}), -log10 p abs err {worst_nl:.3e} (bound {nl_abs:.3e})")
    assert (np.abs(got_p[ok] - p_ref[ok]) <= p_rel * p_ref[ok] + P_ABS).all(), what
    assert worst_nl <= nl_abs, what


@pytest.mark.parametrize("name", sorted(GENE_CASES))
def test_p_and_neglog10p_against_reference_fixture(gn, z, name):
    """End to end: p against scipy's, -log10 p against mpmath's -- finite wherever mpmath's is, so through the underflow."""
    preds, trues, _ = _slides(name)
    res = gn.gene_significance(preds, trues)
    r_ref = z[f"{name}.r"]
    assert np.array_equal(np.isnan(res["pcc"]), np.isnan(r_ref))
    _check_p(res["p"], res["neglog10p"], z[f"{name}.p"], z[f"{name}.nl_mp"], 4 * float(z[f"{name}.restatement_p_rel"]),
             4 * float(z[f"{name}.restatement_nl_abs"]), name)
    one = np.abs(np.nan_to_num(r_ref)) == 1.0
    assert np.array_equal(np.isposinf(res["neglog10p"]), one & (np.diff(_slides(name)[2])[:, None] != 2))
    if name == UNDERFLOW_CASE:
        under = z[f"{name}.p"] == 0.0
        assert under.sum() >= 20 and np.isfinite(res["neglog10p"][under]).all() and (res["neglog10p"][under] > 323).all()


@pytest.mark.parametrize("name", sorted(GENE_CASES))
def test_pvalue_kernel_on_the_reference_r(gn, z, name):
    """mcl_pearson_pvalue alone, handed the fixture's r: the algorithm's own rounding, an order of magnitude tighter."""
    r = torch.from_numpy(z[f"{name}.r"]).to(DEV)
    off = np.concatenate([[0], np.cumsum(GENE_CASES[name]["segments"])]).astype(np.int64)
    p, nl = gn.pvalues_device(r, off)
    p2, nl2 = gn.pvalues_device(r, torch.from_numpy(off).to(DEV))     # device-resident offsets
    assert torch.equal(p.view(torch.int64), p2.view(torch.int64)) and torch.equal(nl.view(torch.int64), nl2.view(torch.int64))
    _check_p(p.cpu().numpy(), nl.cpu().numpy(), z[f"{name}.p"], z[f"{name}.nl_mp"], 4 * float(z[f"{name}.kernel_p_rel"]),
             4 * float(z[f"{name}.kernel_nl_abs"]), f"{name} (reference r)")


def test_special_values(gn):
    """r NaN -> NaN; n == 2 -> p = 1, -log10 p = 0; |r| >= 1 -> p = 0, +inf; r = 0 -> p = 1 to rounding, never above."""
    r = torch.tensor([[np.nan, 1.0, -1.0, 0.0, 0.6, -0.6], [np.nan, 1.0, -1.0, 1.0, -1.0, 1.0],
                      [np.nan, 1.0, -1.0, 0.0, 0.5, -0.5]], dtype=torch.float64, device=DEV)
    p, nl = gn.pvalues_device(r, [0, 4784, 4786, 4789])
    p, nl = p.cpu().numpy(), nl.cpu().numpy()
    assert np.isnan(p[:, 0]).all() and np.isnan(nl[:, 0]).all()
    assert (p[1, 1:] == 1.0).all() and (nl[1, 1:] == 0.0).all() and not np.signbit(nl[1, 1:]).any()
    for s in (0, 2):
        assert (p[s, 1:3] == 0.0).all() and np.isposinf(nl[s, 1:3]).all()
        assert abs(p[s, 3] - 1.0) < 1e-10 and p[s, 3] <= 1.0 and 0.0 <= nl[s, 3] < 1e-10
        assert nl[s, 4] == nl[s, 5] and p[s, 4] == p[s, 5]                     # two-sided: a function of |r|
    assert p[0, 4] == 0.0 and abs(nl[0, 4] - 465.1398821221) < 1e-8            # mpmath, 60 digits
    assert abs(p[2, 4] - 2.0 / 3.0) < 1e-14                                    # n = 3, the arcsine law


@pytest.mark.parametrize("log_space", [True, False])
@pytest.mark.parametrize("name", TABLE_CASES)
def test_order_and_top_equal_pandas(gn, z, name, log_space):
    preds, trues, _ = _slides(name)
    S, G = z[f"{name}.p"].shape
    genes, slides = [f"g{g}" for g in range(G)], [f"s{s}" for s in range(S)]
    res = gn.significance_table(preds, trues, genes, slides, TOP_N, log_space=log_space)
    mean_ref = z[f"{name}.mean"]
    assert np.array_equal(np.isnan(res["mean"]), np.isnan(mean_ref))
    ok = ~np.isnan(mean_ref)
    # a mean of S terms, each within the -log10 p bound (-np.log10 of a p within the p bound adds p_rel / ln 10)
    bound = 4 * float(z[f"{name}.restatement_nl_abs"]) + 4 * float(z[f"{name}.restatement_p_rel"]) / np.log(10)
    print(f"{name} log_space={log_space}: mean abs err {np.abs(res['mean'][ok] - mean_ref[ok]).max():.3e} (bound {bound:.3e})")
    assert np.abs(res["mean"][ok] - mean_ref[ok]).max() <= bound
    n_ok = int(ok.sum())
    assert np.array_equal(res["order"][:n_ok], z[f"{name}.order"][:n_ok]), "order of the defined genes"
    assert np.array_equal(res["order"], stable_order(res["mean"])), "ties by gene index, NaN last"
    assert np.array_equal(res["n_defined"], (~np.isnan(z[f"{name}.p"])).sum(axis=0))
    assert len(res["top"]) == TOP_N
    for t, g, s, v, pcc in zip(res["top"], z[f"{name}.top_gene"], z[f"{name}.top_slide"], z[f"{name}.top_value"],
                               z[f"{name}.top_pcc"]):
        assert (t["gene"], t["best_slide"]) == (int(g), int(s)) and (t["gene_name"], t["slide_name"]) == (f"g{g}", f"s{s}")
        assert abs(t["best_value"] - v) <= bound and abs(t["pcc"] - pcc) <= 1e-12
        assert t["mean"] == res["mean"][g]


def test_reference_inf_mode_on_the_underflow_case(gn, z):
    """log_space=False is the tutorial's arithmetic: the genes with an underflowed p share the mean inf, exactly the
    reference's set, ahead of every finite one; the default keeps all of them finite and ordered."""
    name = UNDERFLOW_CASE
    preds, trues, _ = _slides(name)
    ref = gn.significance_table(preds, trues, log_space=False)
    inf_genes = np.flatnonzero(np.isposinf(ref["mean"]))
    assert np.array_equal(inf_genes, z[f"{name}.inf_genes"])
    k = inf_genes.size
    assert sorted(ref["order"][:k].tolist()) == inf_genes.tolist() and np.isfinite(ref["mean"][ref["order"][k:]]).all()
    assert np.array_equal(ref["order"], stable_order(ref["mean"]))
    assert np.array_equal(np.isposinf(ref["neglog10p"]), ref["p"] == 0.0)
    for t in ref["top"][:min(k, TOP_N)]:
        s = t["best_slide"]
        assert np.isposinf(t["best_value"]) and s == int(np.flatnonzero(ref["p"][:, t["gene"]] == 0.0)[0])   # first inf
    log = gn.significance_table(preds, trues)
    assert np.isfinite(log["mean"]).all() and np.array_equal(log["order"], stable_order(log["mean"]))
    want = z[f"{name}.nl_mp"].mean(axis=0)
    assert np.abs(log["mean"] - want).max() <= 4 * float(z[f"{name}.restatement_nl_abs"])
    assert np.array_equal(log["order"], stable_order(want))


@pytest.mark.parametrize("name", sorted(GENE_CASES))
def test_fp32_against_restatement(gn, z, name):
    preds, trues, off = _slides(name, np.float32)
    res = gn.gene_significance(preds, trues)
    r, p, nl = significance(np.concatenate(preds).astype(np.float64), np.concatenate(trues).astype(np.float64), off)
    assert np.array_equal(np.isnan(res["pcc"]), np.isnan(r))
    _check_p(res["p"], res["neglog10p"], p, nl, 4 * float(z[f"{name}.restatement_p_rel"]),
             4 * float(z[f"{name}.restatement_nl_abs"]), f"{name} fp32")


def _bits(res):
    return tuple(np.ascontiguousarray(res[k]).view(np.int64).tobytes() for k in ("pcc", "p", "neglog10p"))


def test_batch_equals_alone_and_run_to_run(gn):
    for name in ("folds", UNDERFLOW_CASE):
        preds, trues, _ = _slides(name)
        batch = gn.gene_significance(preds, trues)
        assert _bits(batch) == _bits(gn.gene_significance(preds, trues)), f"{name}: run to run"
        for s in range(len(preds)):
            alone = gn.gene_significance([preds[s]], [trues[s]])
            assert _bits(alone) == _bits({k: batch[k][s:s + 1] for k in batch}), f"{name}: slide {s} alone vs in the batch"
    preds, trues, _ = _slides("her2st8")
    a, b = gn.significance_table(preds, trues), gn.significance_table(preds, trues)
    assert a["mean"].tobytes() == b["mean"].tobytes() and a["order"].tobytes() == b["order"].tobytes() and a["top"] == b["top"]


def test_rank_rules(gn):
    """skipna mean, +inf propagation, NaN genes last, exact ties by gene index, the FIRST slide of the row maximum; more
    genes than one workgroup ranks."""
    rng = np.random.default_rng(5)
    S, G = 6, 1500
    nl = rng.random((S, G)) * 50
    r = rng.random((S, G))
    nl[:, 10] = np.nan                                   # undefined everywhere
    nl[:, 700] = np.nan
    nl[2:, 20] = np.nan                                  # defined on two slides
    nl[3, 30] = np.inf
    nl[:, 41] = nl[:, 40]                                # bit-equal means
    nl[:, 1400] = nl[:, 40]
    nl[:, 50] = 7.0
    nl[1, 50] = nl[4, 50] = 99.0                         # the maximum twice: slide 1 wins
    res = gn.rank_genes(nl, r, top_n=5)
    want = np.array([np.nan if np.isnan(c).all() else np.nansum(c) / (~np.isnan(c)).sum() for c in nl.T])
    assert np.array_equal(np.isnan(res["mean"]), np.isnan(want)) and np.isposinf(res["mean"][30])
    fin = np.isfinite(want)
    assert np.abs(res["mean"][fin] - want[fin]).max() <= 1e-13
    assert np.array_equal(res["order"], stable_order(res["mean"]))
    assert res["order"][0] == 30 and res["order"][-2:].tolist() == [10, 700]
    pos = {int(g): i for i, g in enumerate(res["order"])}
    assert pos[40] + 1 == pos[41] and pos[41] + 1 == pos[1400]
    assert np.array_equal(res["n_defined"], (~np.isnan(nl)).sum(axis=0))
    full = gn.rank_genes(nl, r, top_n=G)
    top = {t["gene"]: t for t in full["top"]}
    assert len(top) == G and top[50]["best_slide"] == 1 and top[50]["best_value"] == 99.0 and top[50]["pcc"] == r[1, 50]
    assert top[10]["best_slide"] == -1 and np.isnan(top[10]["best_value"]) and np.isnan(top[10]["pcc"])
    assert top[20]["best_slide"] == int(np.argmax(nl[:2, 20]))
    for g in (0, 40, 999, 1499):
        assert top[g]["best_slide"] == int(np.argmax(nl[:, g])) and top[g]["pcc"] == r[top[g]["best_slide"], g]
    with pytest.raises(ValueError):
        gn.rank_genes(nl, r, log_space=False)            # needs p


def _run_cli(args, cwd=ROOT):
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, "-m", *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    return proc.stdout.strip().splitlines()


def test_cli_in_a_fresh_process(gn, z, tmp_path):
    """The CLI on files in the reference's layout prints the tutorial's lines for the reference's top genes."""
    name = "her2st8"
    preds, trues, _ = _slides(name)
    S, G = len(preds), preds[0].shape[1]
    slides = ["A2", "A3", "B1", "B2", "C1", "C2", "D1", "D2"]
    gene_names = np.array([f"GENE{g}" for g in range(G)], dtype=object)
    pp, tp = [], []
    for s in range(S):
        os.makedirs(tmp_path / slides[s])
        pp.append(str(tmp_path / slides[s] / "matched_spot_expression_pred_mclSTExp.npy"))
        tp.append(str(tmp_path / slides[s] / "preprocessed_matrix.npy"))
        np.save(pp[-1], preds[s].T), np.save(tp[-1], trues[s].T)
    np.save(str(tmp_path / "genes.npy"), gene_names)
    csv = str(tmp_path / "sorted.csv")
    out = _run_cli(["mclstexp_amd.genes", "--pred", *pp, "--true", *tp, "--genes", str(tmp_path / "genes.npy"), "--slides",
                    *slides, "--csv", csv])
    want = gn.significance_table(preds, trues, list(gene_names), slides)
    assert out[-TOP_N:] == gn.format_top(want)
    assert [ln.split(",")[0] for ln in out[-TOP_N:]] == [f"Gene: GENE{g}" for g in z[f"{name}.top_gene"]]
    assert [ln.split(" in ")[1].split(":")[0] for ln in out[-TOP_N:]] == [slides[s] for s in z[f"{name}.top_slide"]]
    first = want["top"][0]
    assert out[-TOP_N] == format_line(first["gene_name"], first["slide_name"], first["best_value"], first["pcc"])
    rows = open(csv).read().splitlines()
    assert rows[0] == "," + ",".join(slides) + ",avg_p_value" and len(rows) == G + 1
    assert [r.split(",")[0] for r in rows[1:TOP_N + 1]] == [f"GENE{g}" for g in z[f"{name}.top_gene"]]
    assert float(rows[1].split(",")[-1]) == want["mean"][want["order"][0]]
    ref = _run_cli(["mclstexp_amd.genes", "--pred", *pp, "--true", *tp, "--top", "3", "--reference_inf"])
    assert ref[-3:] == gn.format_top(gn.significance_table(preds, trues, top_n=3, log_space=False))


def test_save_pred_round_trip(gn, tmp_path):
    """``evaluate --save_pred`` -> ``genes --pred`` equals ``leave_one_slide_out(return_preds=True)`` ->
    ``significance_table`` in memory; ``return_preds`` changes nothing else."""
    from mclstexp_amd import evaluate
    sizes, G, P = [230, 210, 250], 50, 256
    per_fold = []
    for f in range(3):
        d = synth.make_retrieval_case(sum(sizes), sum(sizes), P, G, seed=60 + f)
        cut = np.cumsum([0] + sizes)
        sl = lambda a: [a[cut[i]:cut[i + 1]] for i in range(3)]  # noqa: E731
        per_fold.append((sl(d["image_query"]), sl(d["spot_key"]), sl(d["expression_key"])))
    exprs = [e.astype(np.float32) for e in per_fold[0][2]]
    paths = write_layout(str(tmp_path), [p[0] for p in per_fold], [p[1] for p in per_fold], exprs)
    plain = evaluate.leave_one_slide_out(None, None, exprs, 200, 1, per_fold=lambda f: per_fold[f][:2])
    mem = evaluate.leave_one_slide_out(None, None, exprs, 200, 1, per_fold=lambda f: per_fold[f][:2], return_preds=True)
    assert "preds" not in plain and [p.shape for p in mem["preds"]] == [(n, G) for n in sizes]
    assert all(mem[k] == plain[k] for k in evaluate.SUMMARY_KEYS)
    pred_dir = str(tmp_path / "pred")
    out = _run_cli(["mclstexp_amd.evaluate", "--dataset", "her2st", "--embedding_dir", str(tmp_path), "--expressions",
                    *paths, "--save_pred", pred_dir])
    assert out[-4:] == evaluate.format_report(plain).splitlines()
    pp = [os.path.join(pred_dir, str(i), "matched_spot_expression_pred_mclSTExp.npy") for i in range(3)]
    for f, m in zip(pp, mem["preds"]):
        assert np.array_equal(np.load(f), m.T)
    lines = _run_cli(["mclstexp_amd.genes", "--pred", *pp, "--true", *paths])
    assert lines[-TOP_N:] == gn.format_top(gn.significance_table(mem["preds"], exprs))


def test_table_launches_own_kernels_only(gn):
    from mclstexp_amd import kernel_audit
    preds, trues, _ = _slides("her2st8")
    preds = [torch.from_numpy(p).float().to(DEV) for p in preds]
    trues = [torch.from_numpy(t).to(DEV) for t in trues]
    for log_space in (True, False):
        gn.significance_table(preds, trues, log_space=log_space)   # warm-up
        ks = kernel_audit.step_kernels(lambda: gn.significance_table(preds, trues, log_space=log_space))
        assert not kernel_audit.foreign(ks), kernel_audit.foreign(ks)
        for k in ("expr_gene_stats_kernel", "pearson_pvalue_kernel", "gene_row_kernel", "gene_order_kernel"):
            assert any(k in n for n in ks), (k, ks)
