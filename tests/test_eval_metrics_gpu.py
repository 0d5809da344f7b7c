"""Scoring of expression predictions on the MI355X (mclstexp_amd.evaluate, csrc/eval_metrics.hip) against the
reference's own scores (tests/golden/eval_metrics.npz) and the fp64 restatement (tests/eval_reference.py).  pytest -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eval_reference import EVAL_CASES, GOLDEN, rel_close, score_fold, score_segments, write_layout
from helpers import RETRIEVAL_CASES, load_retrieval_golden
from mclstexp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("heg_pcc", "hvg_pcc", "mse", "mae")


@pytest.fixture(scope="module")
def ev():
    from mclstexp_amd import _lib, evaluate
    _lib.lib()  # must load: no fallback
    return evaluate


def _folds(d, dtype=np.float64):
    off = d["offsets"]
    p, t = d["pred"].astype(dtype), d["true"].astype(dtype)
    return [p[off[s]:off[s + 1]] for s in range(len(off) - 1)], [t[off[s]:off[s + 1]] for s in range(len(off) - 1)]


def _check(got, want, what):
    assert np.array_equal(np.isnan(got["pcc"]), np.isnan(want["pcc"])), f"{what}: NaN positions"
    ok = ~np.isnan(want["pcc"])
    if ok.any():
        assert np.abs(got["pcc"][ok] - want["pcc"][ok]).max() <= 1e-12, what
    assert np.array_equal(got["heg_genes"], want["heg_genes"]), f"{what}: HEG set"
    for k in KEYS:
        assert rel_close(got[k], want[k]), (what, k, got[k], want[k])


def _bits(res):
    return [(f["pcc"].view(np.int64).tobytes(), f["heg_genes"].tobytes(),
             np.array([f[k] for k in KEYS]).view(np.int64).tobytes(), f["n_valid"]) for f in res["folds"]]


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_fp64_against_reference_fixture(ev, name):
    z = np.load(GOLDEN)
    preds, trues = _folds(synth.make_eval_case(**EVAL_CASES[name]))
    res = ev.score_folds(preds, trues)
    for s, f in enumerate(res["folds"]):
        want = {"pcc": z[f"{name}.r"][s], "heg_genes": z[f"{name}.heg"][s]}
        want.update({k: float(z[f"{name}.{k}"][s]) for k in KEYS})
        _check(f, want, f"{name} fold {s}")
        assert f["n_valid"] == int((~np.isnan(want["pcc"])).sum())
    for k in KEYS:   # the scripts' last four lines: np.mean over folds (NaN propagates)
        assert rel_close(res[k], float(np.mean(z[f"{name}.{k}"]))), k


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_fp32_against_restatement(ev, name):
    d = synth.make_eval_case(**EVAL_CASES[name])
    preds, trues = _folds(d, np.float32)
    res = ev.score_folds(preds, trues)
    for s, (f, p, t) in enumerate(zip(res["folds"], preds, trues)):
        _check(f, score_fold(p, t), f"{name} fold {s} fp32")


def test_mixed_dtypes_and_device_views(ev):
    d = synth.make_eval_case([90, 40], 300, seed=11)
    preds, trues = _folds(d)
    want = score_segments(d["pred"], d["true"], d["offsets"])
    wide = torch.zeros((130, 313), dtype=torch.float64, device=DEV)
    wide[:, :300] = torch.from_numpy(d["pred"])
    single = ev.score(wide[:90, :300], trues[0])             # a row-major view with leading dimension 313
    _check(single, want[0], "strided view")
    res = ev.score_folds([p.astype(np.float32) for p in preds], [torch.from_numpy(t).to(DEV) for t in trues])
    for s, f in enumerate(res["folds"]):
        _check(f, score_fold(preds[s].astype(np.float32), trues[s]), f"mixed fold {s}")


def test_segmented_equals_per_fold_and_run_to_run(ev):
    for name in ("folds", "g3467"):
        preds, trues = _folds(synth.make_eval_case(**EVAL_CASES[name]))
        batch = ev.score_folds(preds, trues)
        assert _bits(batch) == _bits(ev.score_folds(preds, trues)), f"{name}: run to run"
        for s in range(len(preds)):
            alone = ev.score_folds([preds[s]], [trues[s]])
            assert _bits(alone)[0] == _bits(batch)[s], f"{name}: fold {s} alone vs in the batch"


def test_heg_tie_rule(ev):
    """Exact ties in the true mean go to the lower gene index: planted duplicate columns, across the rank-50 cut too."""
    rng = np.random.default_rng(3)
    rows, G = 40, 400
    true = rng.random((rows, G))
    pred = rng.random((rows, G))
    for group in ([10, 3, 250], [399, 0, 77, 78], [120, 5]):   # identical columns -> bit-equal means
        for g in group[1:]:
            true[:, g] = true[:, group[0]]
    m = true.mean(axis=0)
    cut = np.lexsort((np.arange(G), -m))
    for g in (cut[49], cut[50], cut[51]):                      # a 3-way tie straddling rank 50
        true[:, g] = true[:, cut[49]]
    got = ev.score(pred, true)
    want = score_fold(pred, true)
    assert np.array_equal(got["heg_genes"], want["heg_genes"])
    assert len(set(np.round(true.mean(axis=0)[want["heg_genes"]], 14))) < 50   # the ties are really there


@pytest.mark.parametrize("G,n_heg", [(3000, 1000), (5000, 50), (257, 256)])
def test_heg_rank_paths(ev, G, n_heg):
    """Large n_heg (every gene a candidate: the global-memory rank), many genes, a sample of exactly n_heg."""
    d = synth.make_eval_case([33, 20], G, seed=G)
    pred = torch.from_numpy(d["pred"]).to(DEV)
    true = torch.from_numpy(d["true"]).to(DEV)
    m = ev.metrics_device(pred, true, d["offsets"], n_heg)
    heg = m["heg"].cpu().numpy()
    for s, want in enumerate(score_segments(d["pred"], d["true"], d["offsets"], n_heg)):
        assert np.array_equal(heg[s], want["heg_genes"])
        assert rel_close(float(m["summary"][s, 0]), want["heg_pcc"])


@pytest.mark.parametrize("name", sorted(RETRIEVAL_CASES))
def test_evaluate_fold_equals_predict_expression_then_score(ev, name):
    from mclstexp_amd import retrieval
    _, case, meta = load_retrieval_golden(name)
    Q, G = meta["Q"], meta["G"]
    gt = synth.uniform_tensor("eval.gt", (Q, G), 0.0, 3.0, seed=meta["N"]).numpy().astype(np.float64)
    got = ev.evaluate_fold(case["spot_key"], case["expression_key"], case["image_query"], gt, meta["top_k"], meta["ord"])
    pred = retrieval.predict_expression(case["spot_key"], case["expression_key"], case["image_query"], meta["top_k"],
                                        meta["ord"])["matched_spot_expression_pred"]
    _check(got, score_fold(pred, gt), name)


def _slides(sizes, G, seed, P=256):
    d = synth.make_retrieval_case(sum(sizes), sum(sizes), P, G, seed=seed)
    cut = np.cumsum([0] + sizes)
    sl = lambda a: [a[cut[i]:cut[i + 1]] for i in range(len(sizes))]  # noqa: E731
    return sl(d["image_query"]), sl(d["spot_key"]), [e.astype(np.float64) for e in sl(d["expression_key"])]


def test_leave_one_slide_out_equals_fold_by_fold(ev):
    imgs, spots, exprs = _slides([60, 45, 50, 38], 40, seed=21)
    top_k, ord_ = 20, 1
    res = ev.leave_one_slide_out(imgs, spots, exprs, top_k, ord_)
    for f in range(4):
        rest = [i for i in range(4) if i != f]
        one = ev.evaluate_fold(np.concatenate([spots[i] for i in rest]), np.concatenate([exprs[i] for i in rest]),
                               imgs[f], exprs[f], top_k, ord_)
        assert _bits({"folds": [one]}) == [_bits(res)[f]], f"fold {f}"
    for k in KEYS:
        assert res[k] == float(np.mean([f[k] for f in res["folds"]]))
    # fold-specific embeddings (each fold's own checkpoint)
    alt = [_slides([60, 45, 50, 38], 40, seed=30 + f)[:2] for f in range(4)]
    res2 = ev.leave_one_slide_out(None, None, exprs, top_k, ord_, per_fold=lambda f: alt[f])
    for f in range(4):
        img, spot = alt[f]
        rest = [i for i in range(4) if i != f]
        one = ev.evaluate_fold(np.concatenate([spot[i] for i in rest]), np.concatenate([exprs[i] for i in rest]),
                               img[f], exprs[f], top_k, ord_)
        assert _bits({"folds": [one]}) == [_bits(res2)[f]], f"per-fold embeddings, fold {f}"


def test_cli_in_a_fresh_process(ev, tmp_path):
    sizes = [230, 210, 250]
    per_fold = [_slides(sizes, 50, seed=40 + f) for f in range(3)]
    exprs = [e.astype(np.float32) for e in per_fold[0][2]]
    paths = write_layout(str(tmp_path), [p[0] for p in per_fold], [p[1] for p in per_fold], exprs)
    out_json = str(tmp_path / "scores.json")
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, "-m", "mclstexp_amd.evaluate", "--dataset", "her2st", "--embedding_dir",
                           str(tmp_path), "--expressions", *paths, "--json", out_json],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    want = ev.leave_one_slide_out(None, None, exprs, 200, 1, per_fold=lambda f: per_fold[f][:2])
    assert proc.stdout.strip().splitlines()[-4:] == ev.format_report(want).splitlines()
    doc = json.load(open(out_json))
    assert doc["dataset"] == "her2st" and (doc["top_k"], doc["ord"]) == (200, 1) and len(doc["folds"]) == 3
    for k in KEYS:
        assert doc[k] == want[k]


def test_scoring_launches_own_kernels_only(ev):
    from mclstexp_amd import kernel_audit
    d = synth.make_eval_case([300, 280, 310], 785, seed=7)
    off = d["offsets"]
    preds = [torch.from_numpy(d["pred"][off[s]:off[s + 1]]).float().to(DEV) for s in range(3)]
    trues = [torch.from_numpy(d["true"][off[s]:off[s + 1]]).to(DEV) for s in range(3)]
    ev.score_folds(preds, trues)   # warm-up
    ks = kernel_audit.step_kernels(lambda: ev.score_folds(preds, trues))
    assert not kernel_audit.foreign(ks), kernel_audit.foreign(ks)
    assert any("expr_gene_stats_kernel" in k for k in ks) and any("expr_summary_kernel" in k for k in ks), ks
