"""GPU: BLEEP's prediction methods (mcl_knn_combine), scoring block (mcl_cell_pearson, mcl_bleep_summary over
mcl_expr_metrics) and gene-gene correlation (mcl_corr_from_gram over mcl_pca_gram) against the notebook's own outputs
(tests/golden/bleep_protocol.npz) and the numpy restatement tests/bleep_reference.py.

Bars: ``average`` 5e-6 of the row's largest value (the project's bar for fp32-pairwise against fp64 accumulation,
test_retrieval_gpu.py; the notebook itself sits 2.7e-7 from the fp64 value); ``weighted_average`` 4 x the case's recorded
distance of the notebook's fp32 arithmetic from the same formula in fp64 (the margin test_genes_gpu.py uses over a fixture's
own measured error) -- the device computes in fp64, so that distance is all it can be asked to match; correlations and
their means 1e-12 (test_eval_metrics_gpu.py); counts, index lists and NaN positions exact."""
import numpy as np
import pytest
import torch

import bleep_reference as ref
from mclstexp_amd import synth

pytestmark = pytest.mark.gpu

METHODS = ("simple", "average", "weighted_average")
AVERAGE_BAR = 5e-6


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(ref.GOLDEN))


@pytest.fixture(scope="module")
def cases():
    return {name: ref.retrieval_case(name) for name in ref.RETRIEVAL_CASES}


@pytest.fixture(scope="module")
def rt():
    from mclstexp_amd import retrieval
    return retrieval


@pytest.fixture(scope="module")
def bleep():
    from mclstexp_amd import bleep as b
    return b


def rows_close(a, b, rel, what):
    """Every row of ``a`` within ``rel`` of that row of ``b``'s largest magnitude."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    err = np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)
    print(f"{what}: max row-scaled error {err.max():.3e} (bar {rel:.3e})")
    assert np.all(err <= rel), f"{what}: {err.max():.3e} > {rel:.3e}"


def expected(golden, case, name, method):
    """(emb, expr, emb bar, expr bar) of the notebook for the fixture's own indices; bar None = bit for bit."""
    if method == "simple":
        e, x = ref.simple(case["spot_key"], case["expression_key"], golden[f"{name}.indices_simple"])
        return e, x, None, None
    if method == "average":
        return golden[f"{name}.average_emb"], golden[f"{name}.average_expr"], AVERAGE_BAR, AVERAGE_BAR
    return (golden[f"{name}.weighted_emb"], golden[f"{name}.weighted_expr"], 4 * float(golden[f"{name}.gap_weighted_emb"]),
            4 * float(golden[f"{name}.gap_weighted"]))


def check_prediction(emb, expr, want, what):
    e, x, bar_e, bar_x = want
    if bar_e is None:
        assert np.array_equal(emb.view(np.uint32), e.view(np.uint32)), what
        assert np.array_equal(expr.view(np.uint32), x.view(np.uint32)), what
    else:
        rows_close(emb, e, bar_e, what + " embeddings")
        rows_close(expr, x, bar_x, what + " expression")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(ref.RETRIEVAL_CASES))
def test_combine_matches_the_notebook(rt, golden, cases, name, method):
    c = cases[name]
    idx = golden[f"{name}.indices_simple"] if method == "simple" else golden[f"{name}.indices"]
    emb, expr = rt.combine_device(c["spot_key"], c["expression_key"], c["image_query"], idx, method)
    assert emb.dtype == expr.dtype == torch.float32
    check_prediction(emb.cpu().numpy(), expr.cpu().numpy(), expected(golden, c, name, method), f"{name} {method}")
    if method == "simple":   # the first column of a wider index list is what "simple" uses
        emb2, expr2 = rt.combine_device(c["spot_key"], c["expression_key"], c["image_query"], golden[f"{name}.indices"], method)
        assert torch.equal(emb2, emb) and torch.equal(expr2, expr)


@pytest.mark.parametrize("method", METHODS)
def test_combine_strided_inputs_and_no_expression(rt, golden, cases, method):
    """ld > cols on every input (an aligned padding of 4 and an odd one: the 16-byte and the element-wise row loads),
    expression_key=None, and the result does not depend on the layout."""
    c, name = cases["mid"], "mid"
    idx = golden[f"{name}.indices"]
    dev = torch.device("cuda")
    base = rt.combine_device(c["spot_key"], c["expression_key"], c["image_query"], idx, method)
    for pad in (3, 4):
        def padded(a):
            buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=dev, dtype=torch.float32)
            buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
            return buf[:, :a.shape[1]]
        key, expr_key, qry = padded(c["spot_key"]), padded(c["expression_key"]), padded(c["image_query"])
        assert key.stride(0) == 256 + pad and expr_key.stride(0) == 97 + pad
        emb, expr = rt.combine_device(key, expr_key, qry, idx, method)
        check_prediction(emb.cpu().numpy(), expr.cpu().numpy(), expected(golden, c, name, method), f"pad {pad} {method}")
        # both layouts round the same fp64 value (up to its last bits) to fp32: at most one fp32 ulp, 2^-23, apart
        rows_close(emb.cpu().numpy(), base[0].cpu().numpy(), 1.2e-7, f"pad {pad} {method} against the dense layout (emb)")
        rows_close(expr.cpu().numpy(), base[1].cpu().numpy(), 1.2e-7, f"pad {pad} {method} against the dense layout (expr)")
        emb2, none = rt.combine_device(key, None, qry, idx, method)
        assert none is None and torch.equal(emb2, emb)


@pytest.mark.parametrize("method", METHODS)
def test_combine_k1_and_narrow_embeddings(rt, method):
    """k = 1 (every method returns the one neighbour's rows) and dim = 30, no multiple of 64, against the restatement."""
    c = synth.make_retrieval_case(90, 9, 30, 13, seed=5)
    rng = np.random.default_rng(3)
    idx1 = rng.integers(0, 90, (9, 1))
    emb, expr = rt.combine_device(c["spot_key"], c["expression_key"], c["image_query"], idx1, method)
    assert np.array_equal(emb.cpu().numpy(), c["spot_key"][idx1[:, 0]])
    assert np.array_equal(expr.cpu().numpy(), c["expression_key"][idx1[:, 0]])
    idx = np.stack([rng.permutation(90)[:6] for _ in range(9)])
    emb, expr = rt.combine_device(c["spot_key"], c["expression_key"], c["image_query"], idx, method)
    if method == "simple":
        want = ref.simple(c["spot_key"], c["expression_key"], idx) + (None, None)
    elif method == "average":
        want = ref.average(c["spot_key"], c["expression_key"], idx) + (AVERAGE_BAR, AVERAGE_BAR)
    else:       # against the formula in fp64: the device's own arithmetic, so one fp32 rounding of the result
        want = ref.weighted_average(c["spot_key"], c["expression_key"], c["image_query"], idx, np.float64) + (1e-7, 1e-7)
    check_prediction(emb.cpu().numpy(), expr.cpu().numpy(), want, f"dim 30 {method}")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["mid", "her2st"])
def test_predict_expression_end_to_end(rt, golden, cases, name, method):
    c = cases[name]
    k = 1 if method == "simple" else c["k"]
    out = rt.predict_expression(c["spot_key"], c["expression_key"], c["image_query"], top_k=k, ord=7, method=method)
    assert out["matched_spot_expression_pred"].dtype == np.float64 and out["indices"].shape == (c["image_query"].shape[0], k)
    z = golden[f"{name}.indices_simple"] if method == "simple" else golden[f"{name}.indices"]
    # the methods read the order too: d_0 is the FIRST match's distance
    same = np.array([set(a.tolist()) == set(b.tolist()) and a[0] == b[0] for a, b in zip(out["indices"], z)])
    assert same.mean() >= 0.9
    e, x, bar_e, bar_x = expected(golden, c, name, method)
    check_prediction(out["matched_spot_embeddings_pred"][same].astype(np.float32),
                     out["matched_spot_expression_pred"][same].astype(np.float32), (e[same], x[same], bar_e, bar_x),
                     f"{name} {method} end to end")


def fold_golden(golden, name, s):
    return {k[len(f"{name}.{s}."):]: v for k, v in golden.items() if k.startswith(f"{name}.{s}.")}


def check_fold(f, g):
    for key, want in (("pcc", g["pcc"]), ("cell_pcc", g["cell_pcc"])):
        assert np.array_equal(np.isnan(f[key]), np.isnan(want)), key
        ok = ~np.isnan(want)
        assert np.all(np.abs(f[key][ok] - want[ok]) <= 1e-12), (key, np.abs(f[key][ok] - want[ok]).max())
    assert np.array_equal(f["heg_genes"][::-1], g["ind_sum"]) and np.array_equal(f["hvg_genes"][::-1], g["ind_var"])
    assert f["n_genes_valid"] == int(g["n_genes_valid"]) and f["n_cells_valid"] == int((~np.isnan(g["cell_pcc"])).sum())
    for key, want in (("cell_mean", g["cell_mean"]), ("max_r", g["max_r"]), ("heg_mean", g["heg_mean_full"]),
                      ("hvg_mean", g["hvg_mean_full"]), ("marker_mean", g["marker_mean_full"])):
        assert ref.rel_close(f[key], float(want), 1e-12), (key, f[key], float(want))


@pytest.mark.parametrize("name", sorted(ref.SCORING_CASES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scoring_matches_the_notebook(bleep, golden, name, dtype):
    d = ref.scoring_case(name)
    off = d["offsets"]
    if dtype is np.float32:      # fp32 inputs hold other numbers: the expectation is the restatement on them
        pred, true = d["pred"].astype(np.float32), d["true"].astype(np.float32)
        want = [ref.score(pred[off[s]:off[s + 1]].astype(np.float64), true[off[s]:off[s + 1]].astype(np.float64), ref.MARKERS)
                for s in range(3)]
        want = [{**w, "ind_sum": w["top_sum"][::-1], "ind_var": w["top_var"][::-1], "heg_mean_full": w["heg_mean"],
                 "hvg_mean_full": w["hvg_mean"], "marker_mean_full": w["marker_mean"]} for w in want]
    else:
        pred, true = d["pred"], d["true"]
        want = [fold_golden(golden, name, s) for s in range(3)]
    res = bleep.score_folds([pred[off[s]:off[s + 1]] for s in range(3)], [true[off[s]:off[s + 1]] for s in range(3)],
                            markers=ref.MARKERS)
    for s in range(3):
        check_fold(res["folds"][s], want[s])
    assert res["folds"][0]["n_cells_valid"] == ref.SEGMENTS[0] - 1           # the constant prediction row
    for k in bleep.SUMMARY_KEYS:
        assert ref.rel_close(res[k], float(np.mean([f[k] for f in res["folds"]])), 1e-15)


def test_notebook_indexing_on_the_device_results(bleep, golden):
    d = ref.scoring_case("nan_gene")
    off = d["offsets"]
    g = fold_golden(golden, "nan_gene", 0)
    f = bleep.score(d["pred"][:off[1]], d["true"][:off[1]], notebook_indexing=True)
    assert ref.rel_close(f["heg_mean"], float(g["heg_mean"]), 1e-12) and ref.rel_close(f["hvg_mean"], float(g["hvg_mean"]), 1e-12)
    assert np.isnan(bleep.score(d["pred"][:off[1]], d["true"][:off[1]])["heg_mean"])      # full vector: the NaN gene is a HEG
    with pytest.raises(IndexError):
        bleep.score(d["pred"][:off[1]], d["true"][:off[1]], markers=ref.MARKERS, notebook_indexing=True)


def test_equal_sums_at_the_boundary_go_to_the_higher_gene_index(bleep):
    """Columns 2 and 7 are equal (same sum, same variance) and share rank n_top: the higher index is taken, as by the tail
    of a stable argsort; with one more place both are listed, the higher index first."""
    rng = np.random.default_rng(1)
    true = rng.random((40, 12)) + np.arange(12)[None, :] * 3.0            # sums and variances ascending with the index
    true[:, 6:] *= np.linspace(1.0, 2.0, 6)[None, :]
    true[:, 7] = true[:, 2]
    pred = true + rng.random((40, 12))
    s, v = true.sum(axis=0), true.var(axis=0)
    for n_top in (9, 10):
        f = bleep.score(pred, true, n_top=n_top)
        assert np.array_equal(f["heg_genes"], np.argsort(s, kind="stable")[-n_top:][::-1])
        assert np.array_equal(f["hvg_genes"], np.argsort(v, kind="stable")[-n_top:][::-1])
    f = bleep.score(pred, true, n_top=9)
    assert f["heg_genes"][-1] == 7 and 2 not in f["heg_genes"]
    f = bleep.score(pred, true, n_top=10)
    assert f["heg_genes"][-2:].tolist() == [7, 2]


@pytest.mark.parametrize("G,n_top", [(3000, 2500), (5000, 50), (257, 256)])
def test_top_gene_rank_paths(bleep, G, n_top):
    """The three paths of the top-n selection under the higher-index tie rule: n_top above the sample of 256 (no threshold,
    all 3000 genes are candidates, more than the 2048 the LDS ranks: the global rank), many genes behind a threshold, and
    a sample one short of G.  Two pairs of identical columns, one of them straddling rank n_top."""
    rng = np.random.default_rng(G)
    true = rng.random((20, G)) * np.linspace(1.0, 3.0, G)[None, :]
    by_sum = np.argsort(true.sum(axis=0), kind="stable")
    lo, hi = sorted((int(by_sum[-n_top]), int(by_sum[-n_top - 1])))     # ranks n_top and n_top + 1 by sum ...
    true[:, hi] = true[:, lo]                                             # ... now equal: only the higher index is listed
    a, b = sorted(int(g) for g in by_sum[-3:-1])                          # and a pair well inside the list
    true[:, b] = true[:, a]
    pred = true + rng.random((20, G))
    s, v = true.sum(axis=0), true.var(axis=0)
    want = np.argsort(s, kind="stable")[-n_top:][::-1]
    assert want[-1] == hi and lo not in want and abs(int(np.where(want == a)[0][0]) - int(np.where(want == b)[0][0])) == 1
    f = bleep.score(pred, true, n_top=n_top)
    assert np.array_equal(f["heg_genes"], want)
    assert np.array_equal(f["hvg_genes"], np.argsort(v, kind="stable")[-n_top:][::-1])


def test_a_segment_in_a_batch_is_bit_identical_to_the_segment_alone(bleep):
    d = ref.scoring_case("nan_gene")
    off = d["offsets"]
    parts = lambda a: [a[off[s]:off[s + 1]] for s in range(3)]
    batch = bleep.score_folds(parts(d["pred"]), parts(d["true"]), markers=ref.MARKERS)["folds"][1]
    alone = bleep.score(d["pred"][off[1]:off[2]], d["true"][off[1]:off[2]], markers=ref.MARKERS)
    for k, v in alone.items():
        a, b = np.asarray(v), np.asarray(batch[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def test_gene_gene_correlation(bleep, golden):
    d = ref.scoring_case("plain")
    off = d["offsets"]
    true, pred = d["true"][off[2]:off[3]], d["pred"][off[2]:off[3]]
    ind = golden["ggc.ind"]
    for x, want in ((true, golden["ggc.corr_true"]), (pred, golden["ggc.corr_pred_raw"]),
                    (torch.from_numpy(true).cuda(), golden["ggc.corr_true"])):
        c = bleep.gene_gene_correlation(x, ind)
        assert c.dtype == np.float64 and np.abs(c - want).max() <= 1e-12
    const = true.copy()
    const[:, 4] = 2.5
    c = bleep.gene_gene_correlation(const, [1, 4, 9])
    assert np.isnan(c[1]).all() and np.isnan(c[:, 1]).all() and not np.isnan(c[[0, 2]][:, [0, 2]]).any()
    with pytest.raises(ValueError):
        bleep.gene_gene_correlation(true[:30], ind)                       # m = 50 > n = 30
    m = bleep.ggc_matrices(true, pred, top_k=50, order=None)
    assert set(m["genes"].tolist()) == set(ind.tolist())
    assert np.array_equal(m["genes"], np.lexsort((np.arange(97), -true.mean(axis=0)))[:50])
    assert np.abs(m["corr_true"] - np.corrcoef(true[:, m["genes"]].T)).max() <= 1e-12
    assert np.abs(m["corr_pred"] - np.corrcoef(pred[:, m["genes"]].T)).max() <= 1e-12


def test_leave_one_slide_out_equals_per_fold_prediction_and_score(bleep, rt):
    sizes, G = [70, 55, 64], 23
    c = synth.make_retrieval_case(sum(sizes), sum(sizes), 30, G, seed=9)
    off = np.concatenate([[0], np.cumsum(sizes)])
    cut = lambda a: [a[off[i]:off[i + 1]] for i in range(3)]
    spots, images, exprs = cut(c["spot_key"]), cut(c["image_query"]), cut(c["expression_key"])
    markers = [0, 22]
    for method in ("weighted_average", "simple"):
        res = bleep.leave_one_slide_out(images, spots, exprs, method=method, markers=markers, return_preds=True)
        for f in range(3):
            rest = [i for i in range(3) if i != f]
            out = rt.predict_expression(np.concatenate([spots[i] for i in rest]), np.concatenate([exprs[i] for i in rest]),
                                        images[f], top_k=bleep.METHOD_TOP_K[method], method=method)
            assert np.array_equal(res["preds"][f], out["matched_spot_expression_pred"].astype(np.float32))
            one = bleep.score(out["matched_spot_expression_pred"], exprs[f], markers=markers)
            for k, v in one.items():
                assert np.array_equal(np.asarray(v), np.asarray(res["folds"][f][k]), equal_nan=True), (method, f, k)
