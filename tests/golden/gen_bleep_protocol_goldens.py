#!/usr/bin/env python3
"""Generate ``bleep_protocol.npz`` by running the REFERENCE's own notebook statements (BLEEP's evaluation protocol).

Runs only where the reference tree is present.  ``baselines/Bleep/BLEEP_inference.ipynb`` is a notebook whose cells read
datasets from absolute paths, so it cannot be run.  This generator takes the code cells out of the notebook's JSON, parses
them with ``ast`` and executes, unmodified and in memory:

  * cell 2's ``find_matches`` function definition,
  * cell 5's three ``if method == ...`` blocks,
  * cell 5's correlation statements, from ``true = expression_gt`` to the highly-variable line (the value every ``print``
    shows is evaluated from the print's own argument),
  * cell 7's ``np.corrcoef`` / ``hierarchy.linkage`` statements (the body of ``plot_heatmap`` up to the plotting calls),

on the procedural inputs of tests/bleep_reference.py (``synth.make_retrieval_case`` / ``synth.make_eval_case``, regenerated
by the tests, never stored).  The marker line reads files; it is restated as ``np.mean(corr[marker_ind])``.  The notebook
asks ``find_matches`` for 50 matches; the small case asks for its own k through the ``top_k`` argument the statement passes.
Only the notebook's OUTPUTS are stored (predictions as float32: ``np.average`` of float32 rows is float32, checked below).

    python tests/golden/gen_bleep_protocol_goldens.py        # writes tests/golden/bleep_protocol.npz
"""
import ast
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import bleep_reference as ref  # noqa: E402

NOTEBOOK = "/root/reference/baselines/Bleep/BLEEP_inference.ipynb"


def cell_trees():
    nb = json.load(open(NOTEBOOK, encoding="utf-8"))
    return [ast.parse("".join(c["source"])) for c in nb["cells"] if c["cell_type"] == "code"]


def code(nodes, name):
    return compile(ast.Module(body=list(nodes), type_ignores=[]), name, "exec")


def lift():
    trees = cell_trees()
    fm = next(n for t in trees for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "find_matches")
    cell5 = next(t for t in trees if any(isinstance(n, ast.If) and "method ==" in ast.unparse(n.test) for n in t.body))
    methods = {}
    for n in cell5.body:
        if isinstance(n, ast.If) and "method ==" in ast.unparse(n.test):
            methods[n.test.comparators[0].value] = code([n], "cell5")
    assert sorted(methods) == ["average", "simple", "weighted_average"], sorted(methods)
    first = next(i for i, n in enumerate(cell5.body) if ast.unparse(n).startswith("true = expression_gt"))
    last = next(i for i, n in enumerate(cell5.body) if "highly variable" in ast.unparse(n))
    scoring = cell5.body[first:last + 1]
    heat = next(n for t in trees for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "plot_heatmap")
    ggc = [n for n in heat.body if not ast.unparse(n).startswith(("plt.", "sns."))]
    ns = {"torch": torch, "F": F, "np": np}
    exec(code([fm], "cell2"), ns)
    return ns["find_matches"], methods, scoring, ggc


def run_method(block, find_matches, name, d, k):
    ns = {"np": np, "method": name, "spot_key": d["spot_key"], "image_query": d["image_query"],
          "expression_key": d["expression_key"],
          "find_matches": lambda key, qry, top_k: find_matches(key, qry, top_k=1 if top_k == 1 else k)}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(block, ns)
    return ns["indices"].astype(np.int64), ns["matched_spot_embeddings_pred"], ns["matched_spot_expression_pred"]


def as_f32(a):
    b = np.asarray(a).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), np.asarray(a, dtype=np.float64))
    return b


def run_scoring(stmts, pred, true, markers):
    """Executes the scoring statements one by one.  Records the correlation vector after each loop (NaN kept), every
    ``ind``, and the value of every print's last argument (NaN + a flag where evaluating it raises IndexError)."""
    ns = {"np": np, "expression_gt": true, "matched_spot_expression_pred": pred}
    out, loops, inds = {}, [], []
    labels = {"across cells": "cell_mean", "non-zero genes": "n_genes_valid", "max correlation": "max_r",
              "highly expressed": "heg_mean", "highly variable": "hvg_mean"}
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"), \
            contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        for n in stmts:
            if isinstance(n, ast.Expr) and isinstance(n.value, ast.Call) and ast.unparse(n.value.func) == "print":
                text = ast.unparse(n.value.args[0])
                key = next((v for k, v in labels.items() if k in text), None)
                if key is not None:
                    try:
                        out[key] = float(eval(compile(ast.Expression(n.value.args[-1]), "cell5", "eval"), ns))
                        out[key + "_raises"] = 0
                    except IndexError:
                        out[key], out[key + "_raises"] = float("nan"), 1
                continue
            exec(code([n], "cell5"), ns)
            if isinstance(n, ast.For):
                loops.append(ns["corr"].copy())
            if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "ind":
                inds.append(ns["ind"].copy())
        ns["marker_ind"] = np.asarray(markers)
        try:
            out["marker_mean"], out["marker_mean_raises"] = float(np.mean(ns["corr"][ns["marker_ind"]])), 0
        except IndexError:
            out["marker_mean"], out["marker_mean_raises"] = float("nan"), 1
    assert len(loops) == 2 and len(inds) == 2
    out.update(cell_pcc=loops[0], pcc=loops[1], ind_sum=inds[0].astype(np.int64), ind_var=inds[1].astype(np.int64))
    # the same three means on the FULL gene vector, with the notebook's own index lists
    out["heg_mean_full"] = float(np.mean(loops[1][inds[0]]))
    out["hvg_mean_full"] = float(np.mean(loops[1][inds[1]]))
    out["marker_mean_full"] = float(np.mean(loops[1][np.asarray(markers)]))
    return out


def run_ggc(stmts, true, pred, top_k):
    """Cell 7 on (genes, spots) matrices: the chosen genes, both correlation matrices (the ground truth's before and the
    prediction's after reordering) and the leaves."""
    from scipy.cluster import hierarchy
    ns = {"np": np, "hierarchy": hierarchy, "expression_gt": true.T, "matched_spot_expression_pred": pred.T, "top_k": top_k}
    out = {}
    for n in stmts:
        exec(code([n], "cell7"), ns)
        if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "corr_matrix" and "corr_true" not in out:
            out["corr_true"] = ns["corr_matrix"].copy()
        elif isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "corr_matrix" and "corr_pred_raw" not in out:
            out["corr_pred_raw"] = ns["corr_matrix"].copy()
    out.update(ind=ns["ind"].astype(np.int64), leaves=np.asarray(ns["cluster_idx"], dtype=np.int64),
               corr_pred_ordered=ns["corr_matrix"].copy())
    return out


def main():
    find_matches, methods, scoring, ggc = lift()
    doc = {}
    for name in ref.RETRIEVAL_CASES:
        d = ref.retrieval_case(name)
        k = d["k"]
        idx1, _, _ = run_method(methods["simple"], find_matches, "simple", d, k)
        idx, a_emb, a_expr = run_method(methods["average"], find_matches, "average", d, k)
        idx_w, w_emb, w_expr = run_method(methods["weighted_average"], find_matches, "weighted_average", d, k)
        assert idx.shape == (d["image_query"].shape[0], k) and np.array_equal(idx, idx_w) and idx1.shape[1] == 1
        e64, x64 = ref.weighted_average(d["spot_key"], d["expression_key"], d["image_query"], idx, np.float64)
        m64 = [np.mean(a.astype(np.float64)[idx], axis=1) for a in (d["spot_key"], d["expression_key"])]
        doc.update({f"{name}.indices": idx, f"{name}.indices_simple": idx1,
                    f"{name}.average_emb": as_f32(a_emb), f"{name}.average_expr": as_f32(a_expr),
                    f"{name}.weighted_emb": as_f32(w_emb), f"{name}.weighted_expr": as_f32(w_expr),
                    f"{name}.gap_weighted": np.float64(ref.row_scaled_gap(w_expr, x64)),
                    f"{name}.gap_weighted_emb": np.float64(ref.row_scaled_gap(w_emb, e64)),
                    f"{name}.gap_average": np.float64(ref.row_scaled_gap(a_expr, m64[1]))})
        print(name, idx.shape, "gap_weighted %.2e (emb %.2e) gap_average %.2e" % (
            doc[f"{name}.gap_weighted"], doc[f"{name}.gap_weighted_emb"], doc[f"{name}.gap_average"]))
    for name in ref.SCORING_CASES:
        d = ref.scoring_case(name)
        off = d["offsets"]
        for s in range(len(off) - 1):
            res = run_scoring(scoring, d["pred"][off[s]:off[s + 1]], d["true"][off[s]:off[s + 1]], ref.MARKERS)
            doc.update({f"{name}.{s}.{k}": np.asarray(v) for k, v in res.items()})
            print(name, s, {k: v for k, v in res.items() if np.ndim(v) == 0})
    d = ref.scoring_case("plain")
    off = d["offsets"]
    res = run_ggc(ggc, d["true"][off[2]:off[3]], d["pred"][off[2]:off[3]], 50)
    doc.update({f"ggc.{k}": v for k, v in res.items()})
    path = os.path.join(HERE, "bleep_protocol.npz")
    np.savez_compressed(path, **doc)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
