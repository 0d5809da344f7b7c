"""CPU: the host array layer shared by retrieval / evaluate / cluster / preprocess / genes (mclstexp_amd/_arrays.py).  The
helpers take the device as an argument, so their host-side decisions -- limits, dtypes, layouts -- run here on CPU tensors."""
import json

import numpy as np
import pytest
import torch

from mclstexp_amd import _arrays as A

CPU = torch.device("cpu")


def test_offsets_validator_under_both_callers_limits():
    from mclstexp_amd import cluster, evaluate
    assert A.cumulative_offsets([3, 2, 4]).tolist() == [0, 3, 5, 9] and A.cumulative_offsets([3]).dtype == np.int64
    assert A.cumulative_offsets(np.array([40000, 40000], dtype=np.int32) ** 2).tolist() == [0, 1600000000, 3200000000]
    # evaluate: folds of >= 2 rows, no upper limit, None is not an offsets array
    assert evaluate.validate_offsets([0, 2, 60002], 60002).tolist() == [0, 2, 60002]
    assert evaluate.validate_offsets(np.array([0, 5], dtype=np.int32), 5).dtype == np.int64
    with pytest.raises(ValueError, match="every fold needs >= 2 rows"):
        evaluate.validate_offsets([0, 1, 5], 5)
    with pytest.raises(ValueError):
        evaluate.validate_offsets(None, 5)
    # cluster: segments of min_rows .. 50 000 rows, at most 65 535 of them, None = one segment
    assert cluster.validate_offsets(None, 7).tolist() == [0, 7]
    assert cluster.validate_offsets([0, 1, 7], 7).tolist() == [0, 1, 7]
    with pytest.raises(ValueError, match="every segment needs 2 .. 50000 rows"):
        cluster.validate_offsets([0, 1, 7], 7, min_rows=2)
    with pytest.raises(ValueError, match="50000"):
        cluster.validate_offsets([0, 50001], 50001)
    with pytest.raises(ValueError, match="at most 65535 segments"):
        cluster.validate_offsets(np.arange(65537), 65536)
    assert cluster.validate_offsets(np.arange(65536), 65535).size == 65536
    for check in (lambda off, rows: evaluate.validate_offsets(off, rows), lambda off, rows: cluster.validate_offsets(off, rows)):
        for off, rows in (([0, 5, 19], 20), ([1, 20], 20), ([0, 10, 10, 20], 20), ([0.0, 20.0], 20), ([[0, 20]], 20), ([0], 0)):
            with pytest.raises(ValueError):
                check(off, rows)


def test_paired_slides_check():
    a = np.zeros((5, 3))
    assert A.paired_offsets([a, np.zeros((2, 3))], [a, np.zeros((2, 3))], "fold").tolist() == [0, 5, 7]
    assert A.paired_offsets([torch.zeros(4, 3)], [a[:4]], "slide").tolist() == [0, 4]       # tensors and arrays mix
    for preds, trues, what in (([a], [np.zeros((5, 4))], "differ in shape"), ([], [], ">= 1 slide"), ([a], [a, a], "one ground truth"),
                               ([a, np.zeros((4, 2))], [a, np.zeros((4, 2))], r"slide 1: expected \(spots, 3\)"),
                               ([a, np.zeros((1, 3))], [a, np.zeros((1, 3))], "every slide needs >= 2 rows")):
        with pytest.raises(ValueError, match=what):
            A.paired_offsets(preds, trues, "slide")


def test_stack_rows_dtype_choice_on_host_inputs():
    f32, f64 = np.ones((2, 3), np.float32), np.full((3, 3), 2.0)
    x, off = A.stack_rows([f32, f32 * 3], "xs", CPU)
    assert x.dtype == torch.float32 and off.tolist() == [0, 2, 4] and x[2:].eq(3).all()      # one shared float dtype is kept
    x, off = A.stack_rows([f32, f64], "xs", CPU)
    assert x.dtype == torch.float64 and off.tolist() == [0, 2, 5] and x[:2].eq(1).all() and x[2:].eq(2).all()
    assert A.stack_rows([f32.astype(np.float16), f32.astype(np.float16)], "xs", CPU)[0].dtype == torch.float64
    assert A.stack_rows([np.arange(6).reshape(2, 3)], "xs", CPU)[0].dtype == torch.float64   # a single part follows the rule too
    assert A.stack_rows([f64], "xs", CPU)[0].dtype == torch.float64
    t = torch.arange(12.0).reshape(3, 4).t()                                                 # a transposed view is laid out row-major
    x, _ = A.stack_rows([t, t], "xs", CPU, convert_on_device=True)
    assert x.is_contiguous() and torch.equal(x[4:], t)
    for parts in ([], [f32, np.ones((2, 4), np.float32)], [f32, np.ones(3, np.float32)]):
        with pytest.raises(ValueError, match="xs"):
            A.stack_rows(parts, "xs", CPU)


def test_matrix_host_conversions():
    m = A.matrix(np.arange(6, dtype=np.int64).reshape(2, 3), "x", CPU, A.FLOAT_CODE, torch.float64)
    assert m.dtype == torch.float64 and m.is_contiguous() and m.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert A.matrix(np.ones((2, 3), np.float32), "x", CPU, A.FLOAT_CODE, torch.float64).dtype == torch.float32   # accepted: kept
    assert A.matrix(np.ones((2, 3)), "x", CPU, (torch.float32,), torch.float32).dtype == torch.float32
    t = A.matrix(np.arange(6.0).reshape(2, 3).T, "x", CPU, A.FLOAT_CODE, torch.float64, dense=True)
    assert t.is_contiguous() and t.tolist() == [[0, 3], [1, 4], [2, 5]]
    by_kind = lambda h: torch.float32 if h.dtype.is_floating_point else torch.int32  # noqa: E731
    assert A.matrix(np.ones((2, 3), np.int64), "x", CPU, (torch.float32, torch.int32), by_kind).dtype == torch.int32
    assert A.matrix(np.ones((2, 3), np.float16), "x", CPU, (torch.float32, torch.int32), by_kind).dtype == torch.float32
    with pytest.raises(ValueError, match="x: expected a 2-D array"):
        A.matrix(np.ones(3), "x", CPU, A.FLOAT_CODE, torch.float64)
    with pytest.raises(RuntimeError, match="x: expected a 2-D array"):                      # each caller keeps its class
        A.matrix(np.ones(3), "x", CPU, A.FLOAT_CODE, torch.float64, RuntimeError)


def test_dense_checks_shape_then_kind_and_converts_host_arrays():
    d = A.dense(np.arange(6).reshape(2, 3), "nbr", (2, 3), torch.int32, CPU, integer=True)
    assert d.dtype == torch.int32 and d.is_contiguous() and d.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert A.dense([[1, 2]], "w", (1, 2), torch.float64, CPU).dtype == torch.float64         # integer=None: any host kind
    src = torch.ones((2, 2), dtype=torch.float64)
    assert A.dense(src, "Y", (2, 2), torch.float64, CPU, copy=True).data_ptr() != src.data_ptr()
    with pytest.raises(ValueError, match=r"nbr: expected shape \(2, 3\), got \(3, 2\)"):    # the shape comes first
        A.dense(np.ones((3, 2)), "nbr", (2, 3), torch.int32, CPU, integer=True)
    with pytest.raises(ValueError, match=r"nbr: expected integers, got torch.float64"):
        A.dense(np.ones((2, 3)), "nbr", (2, 3), torch.int32, CPU, integer=True)
    with pytest.raises(ValueError, match=r"nbr: expected integers, got torch.bool"):
        A.dense(np.ones((2, 3), bool), "nbr", (2, 3), torch.int32, CPU, integer=True)
    with pytest.raises(ValueError, match=r"w: expected floating-point values, got torch.int64"):
        A.dense(np.ones((2, 3), np.int64), "w", (2, 3), torch.float64, CPU, integer=False)


def test_check_columns_and_nanmean():
    assert A.check_columns(np.ones((5, 64)), 64) == (5, 64) and A.check_columns(torch.ones(3, 1), 64) == (3, 1)
    for bad in (np.ones(4), np.ones((2, 2, 2)), torch.ones(4)):
        with pytest.raises(ValueError, match=r"x: expected a 2-D \(rows, D\) array, got shape"):
            A.check_columns(bad, 64)
    for cols in (0, 65):
        with pytest.raises(ValueError, match=rf"x has {cols} columns; the kernel handles 1 \.\. 64"):
            A.check_columns(np.ones((3, cols)), 64)
    assert A.nanmean([1.0, np.nan, 3.0, np.inf]) == 2.0 and np.isnan(A.nanmean([np.nan])) and np.isnan(A.nanmean([]))


def test_count_slides_follow_the_same_helper():
    from mclstexp_amd import preprocess
    assert preprocess._slide(np.ones((2, 3), np.int64), "s", CPU).dtype == torch.int32
    assert preprocess._slide(np.ones((2, 3), bool), "s", CPU).dtype == torch.float32
    assert preprocess._slide(np.ones((2, 3), np.int32), "s", CPU, torch.float32).dtype == torch.float32
    with pytest.raises(ValueError, match="do not fit int32"):
        preprocess._slide(np.full((2, 3), 2 ** 31), "s", CPU)
    with pytest.raises(ValueError, match="2-D"):
        preprocess._slide(np.ones(3), "s", CPU)


def test_every_module_names_itself_without_a_gpu(monkeypatch):
    from mclstexp_amd import cluster, evaluate, genes, preprocess, retrieval
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.arange(12.0).reshape(4, 3) ** 2
    counts = np.arange(12).reshape(4, 3)
    for who, call in (("genes", lambda: genes.gene_significance([x], [x + 1])),
                      ("genes", lambda: genes.rank_genes(np.ones((2, 3)), np.ones((2, 3)))),
                      ("genes", lambda: genes.pvalues_device(torch.ones((1, 3), dtype=torch.float64), [0, 4])),
                      ("evaluate", lambda: evaluate.score(x, x + 1)), ("cluster", lambda: cluster.kmeans(x, 2)),
                      ("preprocess", lambda: preprocess.gene_stats([counts])),
                      ("retrieval", lambda: retrieval.find_matches(x, x))):
        with pytest.raises(RuntimeError, match=rf"mclstexp_amd\.{who}: no GPU available \(HIP kernels, no CPU fallback\)"):
            call()


def test_file_helpers(tmp_path):
    paths = [str(tmp_path / f"{i}.npy") for i in range(2)]
    np.save(paths[0], np.arange(6.0).reshape(2, 3)), np.save(paths[1], np.ones((2, 5)))
    a, b = A.load_gene_major(paths)
    assert a.shape == (3, 2) and b.shape == (5, 2) and a[2].tolist() == [2.0, 5.0]
    np.save(paths[1], np.ones((3, 5)))
    with pytest.raises(ValueError, match=r"1.npy: expected \(G, N\) with G = 2, got \(3, 5\)"):
        A.load_gene_major(paths)
    A.write_json(str(tmp_path / "d.json"), {"a": [1, 2], "b": None})
    text = open(tmp_path / "d.json").read()
    assert json.loads(text) == {"a": [1, 2], "b": None} and text.startswith('{\n "a": [\n  1,')   # indent=1, as the CLIs wrote it
