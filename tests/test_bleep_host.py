"""CPU: the host side of BLEEP's evaluation protocol -- the new C entry points' argument validation, the in-test numpy
restatement (tests/bleep_reference.py) against the notebook's own outputs (tests/golden/bleep_protocol.npz), the notebook's
compact-then-index quirk, method selection and the CLI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bleep_reference as ref
from conftest import ROOT

NEW_SYMBOLS = ("mcl_knn_combine", "mcl_cell_pearson", "mcl_bleep_summary", "mcl_corr_from_gram")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(ref.GOLDEN))


def test_new_symbols_are_declared_exported_and_prototyped():
    from mclstexp_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text), f"{s} is not declared in include/mclstexp_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.PROTOTYPES
    assert lib.mcl_abi_version() == 13            # new entry points only
    assert len(_lib.PROTOTYPES["mcl_knn_combine"]) == len(_lib.PROTOTYPES["mcl_knn_weighted_average"])


def test_knn_combine_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_knn_combine
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def call(key=P, ldk=8, expr=P, lde=6, qry=P, ldq=8, idx=P, nq=3, k=4, dim=8, genes=6, mode=1, emb=P, out=P):
        return fn(key, ldk, expr, lde, qry, ldq, idx, nq, k, dim, genes, mode, emb, out, None)

    for kw in ({"key": None}, {"qry": None}, {"idx": None}, {"expr": None}, {"nq": -1}, {"k": 0}, {"k": -2}, {"dim": 0},
               {"ldk": 7}, {"ldq": 7}, {"lde": 5}, {"genes": 0}):
        assert call(**kw) == -1, kw
    for kw in ({"mode": 3}, {"mode": -1}, {"k": 7501}):
        assert call(**kw) == -2, kw
    assert call(nq=0, key=None) == 0
    assert call(expr=None, out=None, mode=7) == -2        # expression_key may be NULL when expr_pred is


def test_cell_pearson_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_cell_pearson
    P = C.c_void_p(64)

    def call(pred=P, ldp=8, dtp=0, true=P, ldt=8, dtt=1, rows=5, G=8, r=P):
        return fn(pred, ldp, dtp, true, ldt, dtt, rows, G, r, None)

    for kw in ({"pred": None}, {"true": None}, {"r": None}, {"rows": -1}, {"G": 0}, {"ldp": 7}, {"ldt": 3}, {"dtp": 2},
               {"dtt": -1}):
        assert call(**kw) == -1, kw
    assert call(rows=0, pred=None) == 0


def test_bleep_summary_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_bleep_summary
    P = C.c_void_p(64)

    def call(true=P, ldt=8, dtt=0, off=P, S=2, G=8, n_top=4, rg=P, rc=P, mk=P, nm=2, gs=P, gv=P, ts=P, tv=P, summ=P):
        return fn(true, ldt, dtt, off, S, G, n_top, rg, rc, mk, nm, gs, gv, ts, tv, summ, None)

    for kw in ({"true": None}, {"off": None}, {"rg": None}, {"rc": None}, {"gs": None}, {"gv": None}, {"ts": None},
               {"tv": None}, {"summ": None}, {"S": -1}, {"G": 0}, {"n_top": 0}, {"n_top": 9}, {"ldt": 7}, {"dtt": 2},
               {"nm": -1}, {"mk": None}):
        assert call(**kw) == -1, kw
    assert call(S=70000) == -2
    assert call(G=1048577, ldt=1048577) == -2
    assert call(S=0, true=None) == 0
    assert call(mk=None, nm=0, S=70000) == -2             # no markers is valid


def test_corr_from_gram_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    fn = _lib.load().mcl_corr_from_gram
    P = C.c_void_p(64)
    assert fn(None, 4, P, None) == -1
    assert fn(P, 4, None, None) == -1
    assert fn(P, -1, P, None) == -1
    assert fn(P, 40000, P, None) == -2
    assert fn(None, 0, None, None) == 0


@pytest.mark.parametrize("name", sorted(ref.RETRIEVAL_CASES))
def test_restated_methods_equal_the_notebook(golden, name):
    d = ref.retrieval_case(name)
    idx, idx1 = golden[f"{name}.indices"], golden[f"{name}.indices_simple"]
    assert idx.shape == (d["image_query"].shape[0], d["k"]) and np.array_equal(idx[:, :1], idx1)
    emb, expr = ref.average(d["spot_key"], d["expression_key"], idx)
    assert np.array_equal(emb, golden[f"{name}.average_emb"]) and np.array_equal(expr, golden[f"{name}.average_expr"])
    emb, expr = ref.weighted_average(d["spot_key"], d["expression_key"], d["image_query"], idx)
    assert np.array_equal(emb, golden[f"{name}.weighted_emb"]) and np.array_equal(expr, golden[f"{name}.weighted_expr"])
    _, x64 = ref.weighted_average(d["spot_key"], d["expression_key"], d["image_query"], idx, np.float64)
    assert ref.row_scaled_gap(expr, x64) == float(golden[f"{name}.gap_weighted"])
    assert 1e-8 < float(golden[f"{name}.gap_weighted"]) < 1e-5 and float(golden[f"{name}.gap_average"]) < 1e-6


def test_fixture_weights_exercise_both_tails(golden):
    """In the stored cases the fp32 weights span many orders of magnitude and some exceed 1 (d_0 is not the smallest
    distance)."""
    d = ref.retrieval_case("her2st")
    idx = golden["her2st.indices"]
    dist = np.sum((d["spot_key"][idx] - d["image_query"][:, None, :]) ** 2, axis=2)
    w = np.exp(-(dist - dist[:, :1] + 1))
    assert w.min() < 1e-8 and (w > 1).any() and np.all(w[:, 0] == np.exp(np.float32(-1)))


@pytest.mark.parametrize("name", sorted(ref.SCORING_CASES))
def test_restated_scoring_equals_the_notebook(golden, name):
    d = ref.scoring_case(name)
    off = d["offsets"]
    for s in range(len(off) - 1):
        g = {k[len(f"{name}.{s}."):]: v for k, v in golden.items() if k.startswith(f"{name}.{s}.")}
        pred, true = d["pred"][off[s]:off[s + 1]], d["true"][off[s]:off[s + 1]]
        r = ref.score(pred, true, ref.MARKERS)
        assert np.array_equal(r["pcc"], g["pcc"], equal_nan=True) and np.array_equal(r["cell_pcc"], g["cell_pcc"], equal_nan=True)
        assert np.array_equal(r["top_sum"][::-1], g["ind_sum"]) and np.array_equal(r["top_var"][::-1], g["ind_var"])
        assert r["n_genes_valid"] == int(g["n_genes_valid"])
        for k in ("cell_mean", "max_r"):
            assert ref.rel_close(r[k], float(g[k]), 1e-15), (s, k)
        for k in ("heg_mean", "hvg_mean", "marker_mean"):
            assert ref.rel_close(r[k], float(g[k + "_full"]), 1e-15), (s, k)
            if int(g[k + "_raises"]):
                with pytest.raises(IndexError):
                    ref.score(pred, true, ref.MARKERS if k == "marker_mean" else (), notebook_indexing=True)
        if not any(int(g[k + "_raises"]) for k in ("heg_mean", "hvg_mean", "marker_mean")):
            nb = ref.score(pred, true, ref.MARKERS, notebook_indexing=True)
            for k in ("heg_mean", "hvg_mean", "marker_mean"):
                assert ref.rel_close(nb[k], float(g[k]), 1e-15), (s, k)


def test_notebook_indexing_shifts_as_the_fixture_records_and_raises_out_of_range(golden):
    """With a NaN gene the notebook's compacted vector is indexed by full-axis gene indices: segment 0 of the NaN-gene case
    records the shifted means (they differ from the full-vector ones), its marker 96 runs out of the 96 entries."""
    from mclstexp_amd import bleep
    g = {k[len("nan_gene.0."):]: v for k, v in golden.items() if k.startswith("nan_gene.0.")}
    pcc = g["pcc"]
    assert int(np.isnan(pcc).sum()) == 1 and np.isnan(pcc[ref.CONST_COLUMN])
    heg, hvg = g["ind_sum"][::-1].copy(), g["ind_var"][::-1].copy()          # best first, as the device lists them
    none = np.zeros((0,), dtype=np.int32)
    h, v, m = bleep.notebook_means(pcc, heg, hvg, none)
    assert h == float(g["heg_mean"]) and v == float(g["hvg_mean"]) and np.isnan(m)
    assert h != float(g["hvg_mean_full"]) and v != float(g["hvg_mean_full"]) and np.isnan(float(g["heg_mean_full"]))
    assert int(g["marker_mean_raises"]) == 1
    with pytest.raises(IndexError):
        bleep.notebook_means(pcc, heg, hvg, np.asarray(ref.MARKERS, dtype=np.int32))
    # without a NaN gene the two ways agree
    p = {k[len("plain.0."):]: v for k, v in golden.items() if k.startswith("plain.0.")}
    h, v, m = bleep.notebook_means(p["pcc"], p["ind_sum"][::-1].copy(), p["ind_var"][::-1].copy(),
                                   np.asarray(ref.MARKERS, dtype=np.int32))
    assert (h, v, m) == (float(p["heg_mean_full"]), float(p["hvg_mean_full"]), float(p["marker_mean_full"]))


def test_unknown_method_still_raises_value_error():
    from mclstexp_amd import bleep, retrieval
    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        retrieval.predict_expression(x, x, x, top_k=2, method="nonsense")
    with pytest.raises(ValueError):
        retrieval.combine_device(x, x, x, np.zeros((4, 1), dtype=np.int64), "weighted")
    with pytest.raises(ValueError):
        bleep.leave_one_slide_out([x, x], [x, x], [x, x], method="weighted")
    assert retrieval.COMBINE_MODES == {"simple": 0, "average": 1, "weighted_average": 2}
    assert bleep.METHOD_TOP_K == {"simple": 1, "average": 50, "weighted_average": 50}


def test_no_gpu_raises(monkeypatch):
    import torch
    from mclstexp_amd import bleep
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.ones((4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bleep.score(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bleep.gene_gene_correlation(x, [0, 1])


def test_host_checks_of_scoring_and_ggc():
    from mclstexp_amd import bleep
    x = np.ones((6, 4))
    with pytest.raises(IndexError):
        bleep.score(x, x, markers=[4])
    with pytest.raises(ValueError):
        bleep.score(x, x, markers=[[1]])
    with pytest.raises(ValueError):
        bleep.score_folds([x], [np.ones((6, 5))])
    with pytest.raises(ValueError, match="at least"):
        bleep.gene_gene_correlation(np.ones((3, 9)), [0, 1, 2, 3])       # m > n
    with pytest.raises(IndexError):
        bleep.gene_gene_correlation(x, [0, 4])
    with pytest.raises(ValueError):
        bleep.ggc_matrices(x, x, order="average")


def test_cli_arguments_and_marker_lookup():
    from mclstexp_amd import bleep
    a = bleep.parse_args(["--embedding_dir", "d", "--expressions", "a.npy", "b.npy"])
    assert (a.method, a.top_k, a.markers, a.json, a.save_pred, a.ggc) == ("average", None, None, None, None, None)
    a = bleep.parse_args(["--embedding_dir", "d", "--expressions", "a.npy", "--method", "weighted_average", "--top_k", "20",
                          "--markers", "VWF", "SOX9", "--genes", "n.npy", "--ggc", "o.npz"])
    assert (a.method, a.top_k, a.markers, a.genes, a.ggc) == ("weighted_average", 20, ["VWF", "SOX9"], "n.npy", "o.npz")
    for bad in (["--expressions", "a.npy"], ["--embedding_dir", "d"],
                ["--embedding_dir", "d", "--expressions", "a.npy", "--method", "weighted"],
                ["--embedding_dir", "d", "--expressions", "a.npy", "--markers", "VWF"],
                ["--embedding_dir", "d", "--expressions", "a.npy", "--top_k", "0"]):
        with pytest.raises(SystemExit):
            bleep.parse_args(bad)
    assert bleep.marker_indices(["c", "a"], ["a", "b", "c", "a"]) == [2, 0]
    with pytest.raises(ValueError, match="zz"):
        bleep.marker_indices(["a", "zz"], ["a", "b"])


def test_cli_prints_the_notebooks_lines(tmp_path, monkeypatch, capsys):
    """main() with the device call stubbed: files are read in the evaluate layout, the marker names become indices, the
    notebook's six lines are printed per fold, and --json / --save_pred are written."""
    import json
    from eval_reference import write_layout
    from mclstexp_amd import bleep, evaluate
    sizes, P, G = [5, 7], 16, 9
    rng = np.random.default_rng(0)
    spots = [[rng.standard_normal((n, P)).astype(np.float32) for n in sizes] for _ in sizes]
    images = [[rng.standard_normal((n, P)).astype(np.float32) for n in sizes] for _ in sizes]
    exprs = [rng.random((n, G)).astype(np.float32) for n in sizes]
    paths = write_layout(str(tmp_path), images, spots, exprs)
    np.save(tmp_path / "names.npy", np.array([f"g{i}" for i in range(G)]))
    seen = {}

    def fake(image_embeddings, spot_embeddings, expressions, method, top_k, per_fold=None, markers=None, return_preds=False):
        img, spot = per_fold(1)
        seen.update(method=method, top_k=top_k, markers=markers, n=len(expressions), q=img[1].shape, key=spot[0].shape)
        fold = {"cell_mean": 0.5, "n_cells_valid": 5, "n_genes_valid": 8, "max_r": 0.75, "heg_mean": 0.25,
                "hvg_mean": float("nan"), "marker_mean": 0.125, "pcc": np.array([0.5, np.nan]), "cell_pcc": np.zeros(2),
                "heg_genes": np.array([1, 0]), "hvg_genes": np.array([0, 1])}
        return {"folds": [fold, dict(fold)], "cell_mean": 0.5, "max_r": 0.75, "heg_mean": 0.25, "hvg_mean": float("nan"),
                "marker_mean": 0.125, "preds": [np.asarray(e) for e in expressions]}

    monkeypatch.setattr(bleep, "leave_one_slide_out", fake)
    rc = bleep.main(["--embedding_dir", str(tmp_path), "--expressions", *paths, "--method", "simple", "--markers", "g3",
                     "g8", "--genes", str(tmp_path / "names.npy"), "--json", str(tmp_path / "o.json"), "--save_pred",
                     str(tmp_path / "pred")])
    assert rc == 0
    assert seen == {"method": "simple", "top_k": None, "markers": [3, 8], "n": 2, "q": (7, P), "key": (5, P)}
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "fold 0:" and out[7] == "fold 1:" and out[14] == "average over folds:"
    assert out[1:7] == ["Mean correlation across cells:  0.5", "number of non-zero genes:  8", "max correlation:  0.75",
                        "mean correlation highly expressed genes:  0.25", "mean correlation highly variable genes:  nan",
                        "mean correlation marker genes:  0.125"]
    assert [l.split(":")[0] for l in out[15:]] == ["Mean correlation across cells", "max correlation",
                                                   "mean correlation highly expressed genes",
                                                   "mean correlation highly variable genes", "mean correlation marker genes"]
    doc = json.load(open(tmp_path / "o.json"))
    assert doc["method"] == "simple" and doc["top_k"] == 1 and doc["markers"] == [3, 8] and doc["hvg_mean"] is None
    assert doc["folds"][0]["pcc"] == [0.5, None] and doc["folds"][1]["heg_genes"] == [1, 0]
    assert np.load(tmp_path / "pred" / "1" / evaluate.PRED_FILE).shape == (G, 7)


def test_ward_ordering_equals_the_fixture(golden):
    pytest.importorskip("scipy")
    from mclstexp_amd import bleep
    leaves = bleep.ward_leaves(golden["ggc.corr_true"])
    assert np.array_equal(leaves, golden["ggc.leaves"])
    assert np.array_equal(golden["ggc.corr_pred_raw"][leaves][:, leaves], golden["ggc.corr_pred_ordered"])
    d = ref.scoring_case("plain")
    t = d["true"][d["offsets"][2]:d["offsets"][3]]
    assert np.array_equal(np.corrcoef(t[:, golden["ggc.ind"]].T), golden["ggc.corr_true"])


def test_ward_ordering_without_scipy_is_a_clear_error(monkeypatch):
    import sys
    from mclstexp_amd import bleep
    for m in [k for k in sys.modules if k == "scipy" or k.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "scipy.cluster", None)
    with pytest.raises(RuntimeError, match="scipy"):
        bleep.ward_leaves(np.eye(3))
