"""CPU: the host side of mclstexp_amd.preprocess -- gene-name bookkeeping, argument validation before any launch, the C
entry points' checks, the CLI -- and the fixture tests/golden/hvg.npz: it regenerates bit for bit from
tests/hvg_reference.py, and it has the room that makes exact equality of bins and flags a fair demand of the GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import hvg_reference as hr
from mclstexp_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(hr.GOLDEN)


def _slides_of(golden, name):
    return range(len(hr.HVG_CASES[name][1]))


# ---------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", sorted(hr.HVG_CASES))
def test_fixture_leaves_room_for_exact_bins_and_flags(golden, name):
    gap, gap32 = float(golden[f"{name}.order_gap"]), float(golden[f"{name}.gap32"])
    assert 1e-15 <= gap <= 1e-12 and gap32 <= 5e-6, (gap, gap32)
    for i in _slides_of(golden, name):
        g = lambda k: golden[f"{name}.{i}.{k}"]  # noqa: E731
        em = hr.edge_margin(g("means"), g("edges"))
        assert em > 1000 * gap, (name, i, "a mean sits on a bin edge", em)
        for norm, cut in ((g("dispersions_norm"), g("cutoff")), (g("dispersions_norm32"), g("cutoff32"))):
            cm = hr.cutoff_margin(norm, cut)
            assert cm > 10 * gap32, (name, i, "a normalised dispersion sits on the cut-off", cm)
        # the two reference modes agree on every flag, and the stored flags are the rule applied to the stored values
        hv64 = np.nan_to_num(g("dispersions_norm")) >= g("cutoff")
        hv32 = np.nan_to_num(g("dispersions_norm32")) >= g("cutoff32")
        assert np.array_equal(hv64, g("highly_variable")) and np.array_equal(hv32, g("highly_variable"))
        assert np.array_equal(np.isnan(g("dispersions_norm")), np.isnan(g("dispersions_norm32")))
        # the stored bins are (edges strictly below the mean) - 1; the generator, re-run by the regeneration test below,
        # asserts that the fp32 mode (with its own edges) lands every gene in the same bin
        b = (g("edges")[None, :] < g("means")[:, None]).sum(1) - 1
        assert np.array_equal(b, g("mean_bin")) and b.min() >= 0
        assert g("target_sum") == g("target_sum32")


def test_fixture_covers_the_cases_the_rules_need(golden):
    assert len(hr.HVG_CASES["ragged"][1]) >= 5 and len({kw["spots"] for kw in hr.HVG_CASES["ragged"][1]}) >= 5
    assert int(np.isnan(golden["zero_genes.0.dispersions_norm"]).sum()) >= 9
    assert np.bincount(golden["single_bin.0.mean_bin"], minlength=hr.N_BINS)[-1] == 1
    assert golden["single_bin.0.dispersions_norm"][-1] == 1.0
    assert int(golden["n_top_large.n_top"]) > int((~np.isnan(golden["n_top_large.0.dispersions_norm"])).sum())
    assert float(golden["neg_cutoff.0.cutoff"]) <= 0
    assert golden["neg_cutoff.0.highly_variable"][np.isnan(golden["neg_cutoff.0.dispersions_norm"])].all()
    a, b = hr.HVG_CASES["tie"][1][0]["duplicate"]
    z = golden["tie.0.dispersions_norm"]
    assert z[a] == z[b] == float(golden["tie.0.cutoff"])
    assert int(golden["tie.0.highly_variable"].sum()) == int(golden["tie.n_top"]) + 1
    assert os.path.getsize(hr.GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(hr.GOLDEN), f))
                                             for f in os.listdir(os.path.dirname(hr.GOLDEN)) if f != "hvg.npz")


def test_fixture_regenerates_bit_for_bit(golden):
    spec = importlib.util.spec_from_file_location("gen_hvg_goldens", os.path.join(ROOT, "tests", "golden",
                                                                                  "gen_hvg_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = gen.build()
    assert sorted(out) == sorted(golden.files)
    for k in golden.files:
        a, b = np.asarray(out[k]), golden[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_make_counts_case():
    d = synth.make_counts_case(120, 300, seed=4, zero_genes=5, zero_spot=True, top_gene=True, duplicate=(7, 91))
    c = d["counts"]
    assert c.shape == (120, 300) and c.dtype == np.int32 and c.min() >= 0
    assert (c[:, np.arange(5) * 60 + 30] == 0).all(), "five evenly spread all-zero genes"
    assert c[1].sum() == 0 and np.array_equal(c[:, 7], c[:, 91])
    assert c[:, -1].mean() > 10 * np.delete(c, -1, axis=1).mean(0).max() / 2
    again = synth.make_counts_case(120, 300, seed=4, zero_genes=5, zero_spot=True, top_gene=True, duplicate=(7, 91))
    assert np.array_equal(c, again["counts"])
    assert not np.array_equal(c, synth.make_counts_case(120, 300, seed=5)["counts"])
    plain = synth.make_counts_case(400, 200, seed=1)["counts"].astype(np.float64)
    live = plain / synth.make_counts_case(400, 200, seed=1)["depth"][:, None]
    ratio = live.mean(0) / synth.make_counts_case(400, 200, seed=1)["mean"]
    assert 0.5 < np.median(ratio) < 1.5, "the counts follow the per-gene means"
    assert synth.make_counts_case(10, 20, dtype=np.float32)["counts"].dtype == np.float32


def test_restatement_modes_agree_to_fp32_rounding():
    c = synth.make_counts_case(150, 400, seed=8, zero_genes=3)["counts"]
    r64, r32 = hr.highly_variable_genes(c, 80), hr.highly_variable_genes(c, 80, np.float32)
    assert hr.max_gap(r64, r32) < 5e-6 and hr.max_gap(r64, hr.highly_variable_genes(c, 80, sums="fsum")) < 1e-12
    assert np.array_equal(hr.highly_variable_genes(c.astype(np.float32), 80)["dispersions_norm"],
                          r64["dispersions_norm"], equal_nan=True), "fp32 counts hold the same integers"


# ------------------------------------------------------------------------------------------------- gene bookkeeping
def test_shared_genes_on_shuffled_and_duplicated_names():
    from mclstexp_amd import preprocess as pp
    rng = np.random.default_rng(0)
    base = [f"g{j}" for j in range(60)]
    lists = []
    for s in range(4):
        keep = [base[j] for j in rng.permutation(60)[:50]]
        keep[3] = keep[11]                                   # a duplicated name: the later one becomes NAME-1
        keep[20] = keep[11]                                  # and NAME-2
        lists.append(keep)
    shared, maps = pp.shared_genes(lists)
    want, want_maps = hr.shared_genes(lists)
    assert shared == want == sorted(shared) and len(shared) > 10
    for m, w, names in zip(maps, want_maps, lists):
        assert m.dtype == np.int32 and np.array_equal(m, w)
        uniq = pp.make_unique(names)
        assert [uniq[j] for j in m] == shared
    assert pp.make_unique(["a", "b", "a", "a", "b"]) == ["a", "b", "a-1", "a-2", "b-1"]
    assert pp.make_unique(["a", "a-1", "a"]) == ["a", "a-1", "a-2"], "a suffix never collides with a present name"
    assert pp.shared_genes([["x", "y"]])[0] == ["x", "y"]
    with pytest.raises(ValueError):
        pp.shared_genes([["a"], ["b"]])
    with pytest.raises(ValueError):
        pp.shared_genes([])


# ------------------------------------------------------------------------------------------------------ validation
def test_entry_points_reject_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_abi_version() == 13
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def stats(sl=P, ld=P, rows=P, nc=P, off=P, dt=1, cm=None, S=2, G=100, mr=50, top=10, work=P, m=P, d=P, z=P, b=P,
              hv=P, cut=P, tgt=P, st=P):
        return lib.mcl_hvg_stats(sl, ld, rows, nc, off, dt, cm, S, G, mr, top, work, m, d, z, b, hv, cut, tgt, st, None)

    for kw in ({"sl": None}, {"ld": None}, {"rows": None}, {"nc": None}, {"off": None}, {"work": None}, {"m": None},
               {"d": None}, {"z": None}, {"b": None}, {"hv": None}, {"cut": None}, {"tgt": None}, {"st": None},
               {"S": 0}, {"G": 1}, {"mr": 1}, {"top": 0}, {"dt": 2}, {"dt": -1}):
        assert stats(**kw) == -1, kw
    assert stats(S=70000) == -2 and stats(G=(1 << 20) + 1) == -2 and stats(mr=50001) == -2

    def pool(hv=P, S=3, G=10, ex=None, ne=0, u=P, i=P):
        return lib.mcl_hvg_pool(hv, S, G, ex, ne, u, i, None)

    for kw in ({"hv": None}, {"u": None}, {"i": None}, {"S": 0}, {"G": 0}, {"ne": -1}, {"ne": 3}):
        assert pool(**kw) == -1, kw

    def mats(sl=P, ld=P, rows=P, nc=P, off=P, dt=0, sel=P, S=1, K=5, mr=9, rs=1e4, out=P):
        return lib.mcl_expression_matrices(sl, ld, rows, nc, off, dt, sel, S, K, mr, rs, out, None)

    for kw in ({"sl": None}, {"ld": None}, {"rows": None}, {"nc": None}, {"off": None}, {"sel": None}, {"out": None},
               {"S": 0}, {"K": 0}, {"mr": 0}, {"dt": 3}, {"rs": 0.0}, {"rs": float("nan")}):
        assert mats(**kw) == -1, kw
    assert mats(S=65536) == -2 and mats(mr=50001) == -2 and mats(K=(1 << 20) + 1) == -2


@pytest.fixture
def fake_gpu(monkeypatch):
    """Argument checks run before the device is asked for: with validation passing, the next thing is the missing GPU."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_python_validation_raises_before_any_launch(fake_gpu):
    from mclstexp_amd import preprocess as pp
    c = np.ones((20, 30), dtype=np.int32)
    for call in (lambda: pp.gene_stats([c]), lambda: pp.pool(np.zeros((2, 5), dtype=bool)),
                 lambda: pp.expression_matrices([c], None, [0, 1]), lambda: pp.run([c], gene_list=[1, 2]),
                 lambda: pp.run([c], select="union")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    bad_stats = (
        lambda: pp.gene_stats([]), lambda: pp.gene_stats([np.ones(20)]), lambda: pp.gene_stats([np.ones((1, 30))]),
        lambda: pp.gene_stats([np.ones((50001, 2))]), lambda: pp.gene_stats([np.ones((20, 1))]),
        lambda: pp.gene_stats([c], n_top_genes=0),
        lambda: pp.gene_stats([c, np.ones((20, 31))]),                       # different widths need column maps
        lambda: pp.gene_stats([c, c], [np.arange(5)]),                       # one map per slide
        lambda: pp.gene_stats([c], [np.array([0, 30])]),                     # a column outside the slide
        lambda: pp.gene_stats([c], [np.array([0.0, 1.0])]),
        lambda: pp.gene_stats([c, c], [np.arange(5), np.arange(6)]),         # maps of different lengths
    )
    for call in bad_stats:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: pp.pool(np.zeros(5, dtype=bool)), lambda: pp.pool(np.zeros((2, 5))),
                 lambda: pp.pool(np.zeros((2, 5), dtype=bool), [5]), lambda: pp.pool(np.zeros((2, 5), dtype=bool), [0.5]),
                 lambda: pp.expression_matrices([c], None, []), lambda: pp.expression_matrices([c], None, [30]),
                 lambda: pp.expression_matrices([c], None, [[0, 1]]),
                 lambda: pp.run([c]), lambda: pp.run([c], select="all"), lambda: pp.run([c], gene_list=["A"]),
                 lambda: pp.run([c], names=[["a"] * 29], gene_list=[0]), lambda: pp.run([c, c], names=[["a"] * 30]),
                 lambda: pp.run([c], gene_list=[40]), lambda: pp.run([c], n_top_genes=0, gene_list=[0])):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------------------- CLI
def test_cli_arguments_and_help(tmp_path):
    from mclstexp_amd import preprocess as pp
    a = pp.parse_args(["--counts", "d/A1.npy", "d/B1.npy", "--out_dir", "o"])
    assert (a.counts, a.genes, a.gene_list, a.select, a.n_top_genes, a.json) == (["d/A1.npy", "d/B1.npy"], None, None,
                                                                                 "union", 1000, None)
    a = pp.parse_args(["--counts", "A.npy", "--genes", "A.txt", "--gene_list", "l.npy", "--out_dir", "o", "--json", "j"])
    assert a.select == "list" and a.genes == ["A.txt"] and a.json == "j"
    for bad in (["--counts", "a.npy"], ["--out_dir", "o"], ["--counts", "a.npy", "b.npy", "--genes", "a.txt", "--out_dir", "o"],
                ["--counts", "a.npy", "--out_dir", "o", "--select", "list"], ["--counts", "x/a.npy", "y/a.npy", "--out_dir", "o"]):
        with pytest.raises(SystemExit):
            pp.parse_args(bad)
    proc = subprocess.run([sys.executable, "-m", "mclstexp_amd.preprocess", "--help"], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "--gene_list" in proc.stdout and "--out_dir" in proc.stdout
    assert pp.format_report({"n_union": 1712, "n_intersection": 3}).splitlines() == [
        "Number of HVGs:  1712", "Number of HVGs (intersection):  3"]
    (tmp_path / "n.txt").write_text("GATA3\n\nERBB2 \n")
    (tmp_path / "i.txt").write_text("4\n17\n")
    np.save(tmp_path / "l.npy", np.array(["FASN", "MYL12B"]))
    assert pp.read_names(str(tmp_path / "n.txt")) == ["GATA3", "ERBB2"]
    assert pp.read_gene_list(str(tmp_path / "i.txt")).tolist() == [4, 17]
    assert pp.read_gene_list(str(tmp_path / "l.npy")).tolist() == ["FASN", "MYL12B"]
    assert pp.slide_name("data/ST-cnts/A1.npy") == "A1"
