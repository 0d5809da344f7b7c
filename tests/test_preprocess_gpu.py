"""HVG selection and the preprocessed expression matrices on the MI355X (mclstexp_amd.preprocess, csrc/preprocess.hip)
against the restatement of scanpy's steps over pandas' own cut / groupby (tests/hvg_reference.py ->
tests/golden/hvg.npz) and the numpy oracle of the normalisation (oracle/ref_input.py).  pytest -m gpu.

Tolerances.  Continuous outputs: at most 64 x the case's ``order_gap`` (the fixture's own sensitivity to the summation
order: numpy sums vs exactly rounded ones) from the fp64 golden.  Bins and flags: EQUAL to the fp64 golden and to the
fp32-mode golden (tests/test_preprocess_host.py asserts the room that makes this a fair demand).  The matrices: the
2e-6 / 2e-6 of tests/test_input_gpu.py for the same arithmetic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hvg_reference as hr
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("means", "dispersions", "dispersions_norm", "mean_bin", "highly_variable", "cutoff", "target_sum")


@pytest.fixture(scope="module")
def pp():
    from mclstexp_amd import _lib, preprocess
    _lib.lib()  # must load: no fallback
    return preprocess


@pytest.fixture(scope="module")
def golden():
    return np.load(hr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {n: hr.case_slides(n) for n in hr.HVG_CASES}


def _h(t):
    return t.cpu().numpy()


def _bits(res):
    return [_h(res[k]).tobytes() for k in OUTPUTS]


# ---------------------------------------------------------------------------------------------- 1. the golden cases
@pytest.mark.parametrize("name", sorted(hr.HVG_CASES))
def test_gene_stats_against_fixture(pp, golden, cases, name):
    slides = cases[name]
    res = {k: _h(v) for k, v in pp.gene_stats(slides, n_top_genes=int(golden[f"{name}.n_top"])).items()}
    gap = float(golden[f"{name}.order_gap"])
    worst = 0.0
    for i in range(len(slides)):
        for k in hr.CONTINUOUS:
            want = np.atleast_1d(golden[f"{name}.{i}.{k}"])
            got = np.atleast_1d(res[k][i])
            fin = np.isfinite(want)
            assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (name, i, k, "NaN / inf pattern")
            assert np.isfinite(got[fin]).all(), (name, i, k)
            if fin.any():
                worst = max(worst, float(np.abs(got[fin] - want[fin]).max()))
    print(f"{name}: max |gpu - fp64 golden| = {worst:.2e} = {worst / gap:.2f} x order_gap ({gap:.2e}); bound 64 x")
    assert worst <= 64 * gap
    for i in range(len(slides)):
        assert res["mean_bin"][i].min() >= 0
        assert np.array_equal(res["mean_bin"][i], golden[f"{name}.{i}.mean_bin"]), (name, i)
        assert np.array_equal(res["highly_variable"][i], golden[f"{name}.{i}.highly_variable"]), (name, i)
        # the fp32-mode golden (what scanpy does to an integer matrix) has the same bins and flags
        hv32 = np.nan_to_num(golden[f"{name}.{i}.dispersions_norm32"]) >= golden[f"{name}.{i}.cutoff32"]
        assert np.array_equal(res["highly_variable"][i], hv32), (name, i, "fp32 mode")


def test_what_the_special_cases_are_there_for(pp, golden, cases):
    r = pp.gene_stats(cases["tie"], n_top_genes=int(golden["tie.n_top"]))
    a, b = hr.HVG_CASES["tie"][1][0]["duplicate"]
    z, hv = _h(r["dispersions_norm"])[0], _h(r["highly_variable"])[0]
    assert z[a] == z[b] == float(r["cutoff"][0]) and hv[a] and hv[b], "both genes of an exact tie at the cut-off pass"
    assert int(hv.sum()) == int(golden["tie.n_top"]) + 1
    r = pp.gene_stats(cases["neg_cutoff"], n_top_genes=int(golden["neg_cutoff.n_top"]))
    z, hv = _h(r["dispersions_norm"])[0], _h(r["highly_variable"])[0]
    assert float(r["cutoff"][0]) <= 0 and np.isnan(z).any() and hv[np.isnan(z)].all(), "NaN genes pass a cut-off <= 0"
    r = pp.gene_stats(cases["single_bin"], n_top_genes=150)
    assert float(r["dispersions_norm"][0, -1]) == 1.0 and int(r["mean_bin"][0, -1]) == 19
    r = pp.gene_stats(cases["n_top_large"], n_top_genes=5000)
    assert bool(r["highly_variable"].cpu().numpy().all())


def test_flat_means_are_reported(pp):
    flat = np.full((40, 30), 3, dtype=np.int32)
    with pytest.raises(ValueError, match="all equal"):
        pp.gene_stats([flat])
    with pytest.raises(ValueError, match="slide 1"):
        pp.gene_stats([hr.case_slides("zero_spot")[0][:, :30], flat])
    with pytest.raises(ValueError, match="no spot holds a count"):
        pp.gene_stats([np.zeros((40, 30), dtype=np.int32)])


# -------------------------------------------------------------------------------------------------- 2. determinism
def test_batch_equals_slide_alone_and_runs_repeat(pp, golden, cases):
    slides = cases["ragged"]
    batch = pp.gene_stats(slides, n_top_genes=200)
    assert _bits(batch) == _bits(pp.gene_stats(slides, n_top_genes=200)), "run to run"
    for i, c in enumerate(slides):
        alone = pp.gene_stats([c], n_top_genes=200)
        for k in OUTPUTS:
            assert _h(alone[k])[0].tobytes() == _h(batch[k])[i].tobytes(), (i, k)
    # another order and other neighbours: the same bits per slide
    perm = [4, 0, 5, 2]
    sub = pp.gene_stats([slides[j] for j in perm], n_top_genes=200)
    for pos, j in enumerate(perm):
        for k in OUTPUTS:
            assert _h(sub[k])[pos].tobytes() == _h(batch[k])[j].tobytes(), (j, k)


def test_column_maps_equal_a_host_subset_and_dtypes_agree(pp, cases):
    rng = np.random.default_rng(5)
    slides = cases["ragged"][:3]
    maps = [np.sort(rng.choice(1200, 900, replace=False))[rng.permutation(900)].astype(np.int32) for _ in slides]
    via_map = pp.gene_stats(slides, maps, n_top_genes=120)
    copies = [np.ascontiguousarray(c[:, m]) for c, m in zip(slides, maps)]
    via_copy = pp.gene_stats(copies, n_top_genes=120)
    assert _bits(via_map) == _bits(via_copy)
    as_f32 = pp.gene_stats([c.astype(np.float32) for c in copies], n_top_genes=120)
    assert _bits(as_f32) == _bits(via_copy), "int32 and float32 counts"
    as_i64 = pp.gene_stats([c.astype(np.int64) for c in copies], n_top_genes=120)      # converted on the host
    assert _bits(as_i64) == _bits(via_copy)
    # device tensors, one of them a strided view
    wide = torch.full((slides[1].shape[0], 1300), 9, dtype=torch.int32, device=DEV)
    wide[:, :1200] = torch.from_numpy(slides[1])
    dev = [torch.from_numpy(slides[0]).to(DEV), wide[:, :1200], torch.from_numpy(slides[2]).to(DEV)]
    assert _bits(pp.gene_stats(dev, maps, n_top_genes=120)) == _bits(via_map)


# ------------------------------------------------------------------------------------------------------ 3. pooling
def test_pool_against_numpy(pp):
    rng = np.random.default_rng(2)
    hv = rng.random((7, 1500)) < 0.4
    extra = np.array([3, 77, 1499, 3])
    uni, inter = pp.pool(hv, extra)
    want = hv.any(0)
    want[extra] = True
    assert uni.dtype == torch.bool and np.array_equal(_h(uni), want) and np.array_equal(_h(inter), hv.all(0))
    uni, inter = pp.pool(torch.from_numpy(hv[:1]).to(DEV))
    assert np.array_equal(_h(uni), hv[0]) and np.array_equal(_h(inter), hv[0])


# ----------------------------------------------------------------------------------------------------- 4. matrices
def test_expression_matrices_match_the_oracle(pp, cases):
    from oracle import ref_input
    rng = np.random.default_rng(3)
    slides = cases["ragged"]
    genes = rng.choice(1200, 785, replace=False)
    mats = pp.expression_matrices(slides, None, genes)
    for c, m in zip(slides, mats):
        assert m.dtype == torch.float32 and tuple(m.shape) == (785, c.shape[0]) and m.is_contiguous()
        assert_close(_h(m), ref_input.log_library_size_normalize(c[:, genes]).T, 2e-6, 2e-6, what="preprocessed matrix")
    assert (mats[2][:, 1] == 0).all(), "a spot without counts stays zero"
    # through column maps, fp32 input, an odd number of genes
    maps = [rng.permutation(1200)[:1000].astype(np.int32) for _ in slides]
    g2 = rng.choice(1000, 171, replace=False)
    mats2 = pp.expression_matrices([c.astype(np.float32) for c in slides], maps, g2)
    for c, mp, m in zip(slides, maps, mats2):
        assert_close(_h(m), ref_input.log_library_size_normalize(c[:, mp[g2]]).T, 2e-6, 2e-6, what="mapped matrix")
    one = pp.expression_matrices([slides[3]], None, genes)[0]
    assert np.array_equal(_h(one), _h(mats[3])), "a slide alone is bit-identical"


# ------------------------------------------------------------------------------------------- 5. run() and the CLI
def _named(cases):
    """Three ragged slides with their own shuffled, partly missing, partly duplicated gene names."""
    rng = np.random.default_rng(11)
    base = [f"G{j:04d}" for j in range(1200)]
    slides, names = [], []
    for c in cases["ragged"][:3]:
        keep = np.sort(rng.choice(1200, 1100, replace=False))
        order = keep[rng.permutation(keep.size)]
        n = [base[j] for j in order]
        n[5] = n[9]                                          # a duplicate: the second becomes NAME-1
        slides.append(np.ascontiguousarray(c[:, order]))
        names.append(n)
    return slides, names


def test_run_composes_the_pieces(pp, cases):
    slides, names = _named(cases)
    shared, maps = hr.shared_genes(names)
    gene_list = [shared[j] for j in (700, 3, 250, 41)]
    res = pp.run(slides, names, n_top_genes=150, gene_list=gene_list, select="union")
    assert res["shared"] == shared
    hv = np.stack([hr.highly_variable_genes(np.ascontiguousarray(c[:, m]), 150)["highly_variable"]
                   for c, m in zip(slides, maps)])
    assert np.array_equal(_h(res["stats"]["highly_variable"]), hv)
    assert (res["n_union"], res["n_intersection"]) == (int(hv.any(0).sum()), int(hv.all(0).sum()))
    uni = hv.any(0)
    uni[[700, 3, 250, 41]] = True
    assert np.array_equal(_h(res["union"]), uni) and np.array_equal(res["genes"], np.flatnonzero(uni))
    from oracle import ref_input
    for c, mp, m in zip(slides, maps, res["matrices"]):
        assert_close(_h(m), ref_input.log_library_size_normalize(c[:, mp[res["genes"]]]).T, 2e-6, 2e-6, what="union")
    lst = pp.run(slides, names, n_top_genes=150, gene_list=gene_list)                  # select="list": the list's order
    assert lst["gene_names"] == gene_list and tuple(lst["matrices"][0].shape) == (4, slides[0].shape[0])
    with pytest.raises(ValueError, match="not shared"):
        pp.run(slides, names, gene_list=["no-such-gene"])


def test_cli_round_trip(pp, cases, tmp_path):
    from mclstexp_amd import evaluate
    slides, names = _named(cases)
    shared, maps = hr.shared_genes(names)
    counts, genes = [], []
    for i, (c, n) in enumerate(zip(slides, names)):
        counts.append(str(tmp_path / f"S{i}.npy"))
        genes.append(str(tmp_path / f"S{i}.txt"))
        np.save(counts[-1], c)
        open(genes[-1], "w").write("\n".join(n) + "\n")
    gl = str(tmp_path / "list.txt")
    open(gl, "w").write("\n".join(shared[::7]) + "\n")
    out_dir, js = str(tmp_path / "out"), str(tmp_path / "sel.json")
    proc = subprocess.run([sys.executable, "-m", "mclstexp_amd.preprocess", "--counts", *counts, "--genes", *genes,
                           "--gene_list", gl, "--out_dir", out_dir, "--n_top_genes", "150", "--json", js], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr
    doc = json.load(open(js))
    lines = proc.stdout.splitlines()
    assert lines[0] == f"Number of HVGs:  {doc['n_union']}" and lines[1].startswith("Number of HVGs (intersection):  ")
    paths = [os.path.join(out_dir, f"S{i}", "preprocessed_matrix.npy") for i in range(3)]
    K = len(shared[::7])
    for p, c in zip(paths, slides):
        m = np.load(p)
        assert m.shape == (K, c.shape[0]) and m.dtype == np.float32
    ex = evaluate.load_expressions(paths)                     # what --expressions of the evaluation reads
    assert [e.shape for e in ex] == [(c.shape[0], K) for c in slides]
    direct = pp.run(slides, names, n_top_genes=150, gene_list=shared[::7])
    assert np.array_equal(np.load(paths[1]), _h(direct["matrices"][1]))


# --------------------------------------------------------------------------------------------------- 6. own kernels
def test_preprocessing_launches_own_kernels_only(pp, cases):
    from mclstexp_amd import kernel_audit
    slides, names = _named(cases)
    shared, _ = hr.shared_genes(names)
    fn = lambda: pp.run(slides, names, n_top_genes=150, gene_list=shared[:50], select="union")  # noqa: E731
    fn()   # warm-up
    ks = kernel_audit.step_kernels(fn)
    assert not kernel_audit.foreign(ks), kernel_audit.foreign(ks)
    for want in ("hvg_libsize_kernel", "hvg_target_kernel", "hvg_moments_kernel", "hvg_select_kernel", "hvg_pool_kernel",
                 "hvg_force_kernel", "expr_matrices_kernel"):
        assert any(want in k for k in ks), (want, sorted(ks))
