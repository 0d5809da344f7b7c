"""CPU: the host side of mclstexp_amd.evaluate -- C-side argument validation, offsets, presets, the CLI's file layout --
and the in-test fp64 restatement (tests/eval_reference.py) against the reference's own scores (eval_metrics.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from eval_reference import EVAL_CASES, GOLDEN, rel_close, score_segments, write_layout
from mclstexp_amd import synth


def test_expr_metrics_rejects_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    lib = _lib.load()
    fn = lib.mcl_expr_metrics
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def call(pred=P, ldp=8, dtp=0, true=P, ldt=8, dtt=0, off=P, S=2, G=8, n_heg=4, r=P, tm=P, heg=P, summ=P, work=P):
        return fn(pred, ldp, dtp, true, ldt, dtt, off, S, G, n_heg, r, tm, heg, summ, work, None)

    for kw in ({"pred": None}, {"true": None}, {"off": None}, {"r": None}, {"tm": None}, {"heg": None}, {"summ": None},
               {"work": None}, {"S": 0}, {"S": -3}, {"G": 0}, {"n_heg": 0}, {"n_heg": 9}, {"dtp": 2}, {"dtt": -1},
               {"ldp": 7}, {"ldt": 3}):
        assert call(**kw) == -1, kw
    assert call(S=70000) == -2


def test_offsets_validation():
    from mclstexp_amd import evaluate
    assert evaluate.validate_offsets([0, 2, 5], 5).tolist() == [0, 2, 5]
    assert evaluate.validate_offsets(np.array([0, 346], dtype=np.int32), 346).dtype == np.int64
    for off, rows in (([0, 1, 5], 5), ([0, 3, 3, 6], 6), ([0, 4, 2, 6], 6), ([1, 5], 5), ([0, 5], 6), ([0], 0),
                      ([[0, 5]], 5), ([0.0, 5.0], 5)):
        with pytest.raises(ValueError):
            evaluate.validate_offsets(off, rows)


def test_presets_are_the_reference_scripts():
    from mclstexp_amd import evaluate
    # evel_her2st.py:174,176 (top 200, L1); evel_cscc.py:197,209 (top 600, L2); evel_visium.py:193,197 (top 200, L2)
    assert evaluate.PRESETS == {"her2st": (200, 1), "cscc": (600, 2), "10x": (200, 2)}


def test_no_gpu_raises(monkeypatch):
    import torch
    from mclstexp_amd import evaluate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.ones((4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.score(x, x)


def test_score_folds_rejects_mismatched_folds():
    from mclstexp_amd import evaluate
    a = np.zeros((5, 3))
    with pytest.raises(ValueError):
        evaluate.score_folds([a], [np.zeros((5, 4))])
    with pytest.raises(ValueError):
        evaluate.score_folds([a, np.zeros((4, 2))], [a, np.zeros((4, 2))])
    with pytest.raises(ValueError):
        evaluate.score_folds([a, np.zeros((1, 3))], [a, np.zeros((1, 3))])
    with pytest.raises(ValueError):
        evaluate.score_folds([], [])


def test_cli_arguments():
    from mclstexp_amd import evaluate
    a = evaluate.parse_args(["--dataset", "cscc", "--embedding_dir", "d", "--expressions", "a.npy", "b.npy"])
    assert (a.dataset, a.embedding_dir, a.expressions, a.json) == ("cscc", "d", ["a.npy", "b.npy"], None)
    for bad in (["--dataset", "visium", "--embedding_dir", "d", "--expressions", "a.npy"],
                ["--dataset", "10x", "--expressions", "a.npy"],
                ["--dataset", "10x", "--embedding_dir", "d"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)


def test_cli_file_discovery_and_layout_checks(tmp_path):
    from mclstexp_amd import evaluate
    sizes, P, G = [5, 7, 6], 16, 9
    rng = np.random.default_rng(0)
    images = [[rng.standard_normal((s, P)).astype(np.float32) for s in sizes] for _ in sizes]
    spots = [[rng.standard_normal((s, P)).astype(np.float32) for s in sizes] for _ in sizes]
    expr = [rng.random((s, G)).astype(np.float32) for s in sizes]
    paths = write_layout(str(tmp_path), images, spots, expr)
    ex = evaluate.load_expressions(paths)
    assert [e.shape for e in ex] == [(s, G) for s in sizes]
    for f in range(3):
        img, spot = evaluate.load_fold_embeddings(str(tmp_path), f, 3)
        assert np.array_equal(img[f], images[f][f])
        assert all(img[i] is None for i in range(3) if i != f)
        assert all(np.array_equal(spot[i], spots[f][i]) for i in range(3))
        evaluate.check_layout(img, spot, ex, f)
    # a spot count that disagrees with the expression matrix
    with pytest.raises(ValueError, match="expression rows"):
        evaluate.check_layout(img, spot, [ex[0], ex[1], ex[2][:-1]], 2)
    # an embedding file of the wrong width
    np.save(os.path.join(str(tmp_path), "embeddings_1", "spot_embeddings_2.npy"), np.zeros((P + 1, 7), np.float32))
    with pytest.raises(ValueError, match="expected \\(P, N\\)"):
        evaluate.load_fold_embeddings(str(tmp_path), 1, 3)
    # expression files with different gene counts
    np.save(paths[1], np.zeros((G + 1, 7), np.float32))
    with pytest.raises(ValueError, match="expected \\(G, N\\)"):
        evaluate.load_expressions(paths)
    with pytest.raises(FileNotFoundError):
        evaluate.load_fold_embeddings(str(tmp_path), 3, 3)


def test_report_format():
    from mclstexp_amd import evaluate
    txt = evaluate.format_report({"heg_pcc": 0.123456, "hvg_pcc": float("nan"), "mse": 1.0, "mae": 2.5})
    assert txt.splitlines() == ["avg heg pcc: 0.1235", "avg hvg pcc: nan", "Mean Squared Error (MSE): 1.0000",
                                "Mean Absolute Error (MAE): 2.5000"]


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_restatement_matches_reference_fixture(name):
    """tests/eval_reference.py against the reference's get_R / HEG / MSE / MAE outputs: pins the restatement that the
    GPU tests use for fp32 inputs and for cases without a fixture."""
    z = np.load(GOLDEN)
    d = synth.make_eval_case(**EVAL_CASES[name])
    got = score_segments(d["pred"], d["true"], d["offsets"])
    r_ref = z[f"{name}.r"]
    for s, f in enumerate(got):
        assert np.array_equal(np.isnan(f["pcc"]), np.isnan(r_ref[s]))
        ok = ~np.isnan(r_ref[s])
        assert np.abs(f["pcc"][ok] - r_ref[s][ok]).max() <= 1e-12
        assert np.array_equal(f["heg_genes"], z[f"{name}.heg"][s])
        for k in ("heg_pcc", "hvg_pcc", "mse", "mae"):
            assert rel_close(f[k], float(z[f"{name}.{k}"][s])), (name, s, k, f[k], z[f"{name}.{k}"][s])


def test_fixture_covers_the_edge_cases():
    z = np.load(GOLDEN)
    assert np.isnan(z["folds.heg_pcc"]).all()                  # a constant column among the top-50 means
    assert np.isnan(z["her2st.r"]).sum() == 2                  # one constant in true, one in pred
    assert z["g30.heg"].shape == (2, 30) and z["g1.heg"].shape == (2, 1)
    assert z["g3467.r"].shape == (2, 3467)
    assert min(np.diff([0] + list(np.cumsum(EVAL_CASES["folds"]["segments"])))) == 2
