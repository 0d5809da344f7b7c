"""GPU: csrc/umap.hip through mclstexp_amd.umap against the numpy restatement (tests/umap_reference.py) on the cases of
tests/golden/umap.npz: the two sample counters exactly, the positions after 1, 10 and the recorded trajectory length within
4 x the uncertainty the fixture recorded, the starts exactly, pruning, determinism, a full default-length run, and the
notebook function and the CLI end to end.  The graphs are the restatement's own (neighbors_reference), handed over through
umap.from_scipy, so that both sides start from the same bits."""
import os

import numpy as np
import pytest
import torch

import umap_reference as ur
from mclstexp_amd import neighbors, umap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(ur.GOLDEN)


@pytest.fixture(scope="module")
def graphs():
    """name -> (scipy CSR per segment, the dict layout() takes), computed once."""
    out = {}
    for name in ur.CASES:
        ms = ur.case_graphs(name)
        out[name] = (ms, umap.from_scipy(ms))
    return out


def _marks(z, name):
    return sorted({1, min(10, ur.CASES[name][3]), int(z[f"{name}_trajectory_len"])})


@pytest.fixture(scope="module")
def ref(z, graphs):
    """name -> [run per segment] of the restatement over the whole n_epochs, keeping the compared epochs."""
    out = {}
    for name in ur.TRAJECTORY:
        off = graphs[name][1]["offsets"]
        out[name] = [ur.run(m, z[f"{name}_Y0"][off[s]:off[s + 1]], ur.CASES[name][3], float(z["a"]), float(z["b"]), ur.SEED,
                            keep=_marks(z, name)) for s, m in enumerate(graphs[name][0])]
    return out


def _layout(z, graphs, name, **kw):
    args = dict(init=ur.CASES[name][2], x=z[f"{name}_X"], n_epochs=ur.CASES[name][3], a=float(z["a"]), b=float(z["b"]),
                seed=ur.SEED)
    args.update(kw)
    return umap.layout(graphs[name][1], **args)


@pytest.mark.parametrize("name", ur.TRAJECTORY)
def test_counters_and_trajectory(z, graphs, ref, name):
    off = graphs[name][1]["offsets"]
    full = _layout(z, graphs, name)
    assert full["embedding"].shape == (off[-1], 2) and full["embedding"].dtype == torch.float64
    assert full["attractive_samples"].dtype == np.int64 and full["n_epochs"].tolist() == [ur.CASES[name][3]] * (off.size - 1)
    assert full["attractive_samples"].tolist() == [r["attractive_samples"] for r in ref[name]]
    assert full["negative_samples"].tolist() == [r["negative_samples"] for r in ref[name]]
    assert torch.isfinite(full["embedding"]).all()
    for k in _marks(z, name):
        got = _layout(z, graphs, name, stop_after=k)
        Y = got["embedding"].cpu().numpy()
        part = [ur.run(m, z[f"{name}_Y0"][off[s]:off[s + 1]], ur.CASES[name][3], float(z["a"]), float(z["b"]), ur.SEED,
                       stop_after=k) for s, m in enumerate(graphs[name][0])] if k == int(z[f"{name}_trajectory_len"]) else None
        if part is not None:                                   # the counters after L epochs
            assert got["attractive_samples"].tolist() == [r["attractive_samples"] for r in part]
            assert got["negative_samples"].tolist() == [r["negative_samples"] for r in part]
        allow = 4 * float(z[f"err_{name}_Y{k}"])
        for s, r in enumerate(ref[name]):
            e = ur.rel(Y[off[s]:off[s + 1]], r["trace"][k])
            print(name, "segment", s, "epochs", k, "deviation", e, "of", allow)
            assert e <= allow, (name, s, k)


def test_starts(z, graphs):
    for name in ur.TRAJECTORY:                                  # a: "random"; b, d: "pca"
        got = _layout(z, graphs, name, stop_after=0)
        assert np.array_equal(got["embedding"].cpu().numpy(), z[f"{name}_Y0"]), name
        assert not got["attractive_samples"].any() and not got["negative_samples"].any()
    off = graphs["b"][1]["offsets"]
    rnd = _layout(z, graphs, "b", init="random", stop_after=0)["embedding"].cpu().numpy()
    assert np.array_equal(rnd, np.concatenate([ur.random_init(int(n), ur.SEED) for n in np.diff(off)]))
    x32 = z["b_X"].astype(np.float32)                           # float32 input, on the device with a row stride
    wide = torch.zeros((x32.shape[0], 64), dtype=torch.float32)
    wide[:, :50] = torch.from_numpy(x32)
    pca = _layout(z, graphs, "b", x=wide.cuda()[:, :50], stop_after=0)["embedding"].cpu().numpy()
    want = np.concatenate([ur.pca_init(x32[off[s]:off[s + 1]].astype(np.float64)) for s in range(3)])
    assert np.array_equal(pca, want)
    # a start passed as an array is used as given, host or device, and is left alone
    Y0 = np.random.RandomState(3).uniform(-10, 10, size=(70, 2))
    assert np.array_equal(_layout(z, graphs, "a", init=Y0, stop_after=0)["embedding"].cpu().numpy(), Y0)
    dev = torch.from_numpy(Y0).cuda()
    on_device = _layout(z, graphs, "a", init=dev, stop_after=3)["embedding"]
    assert np.array_equal(dev.cpu().numpy(), Y0)
    assert torch.equal(on_device, _layout(z, graphs, "a", init=Y0, stop_after=3)["embedding"])
    assert not np.array_equal(on_device.cpu().numpy(), Y0)


def test_pruning(z, graphs, ref):
    """Case b with n_epochs = 40: a large share of the entries lies below wmax / 40.  Any contribution of one of them
    would show in the counters, which count every attraction taken and every sample drawn."""
    assert ur.CASES["b"][3] == 40
    got = _layout(z, graphs, "b")
    for s, r in enumerate(ref["b"]):
        pruned = 1.0 - float(r["live"].mean())
        print("b segment", s, "pruned share", pruned)
        assert pruned > 0.25
        assert int(got["attractive_samples"][s]) == r["attractive_samples"]
        assert int(got["negative_samples"][s]) == r["negative_samples"]


def test_determinism(z, graphs):
    off = graphs["b"][1]["offsets"]
    a = _layout(z, graphs, "b")
    b = _layout(z, graphs, "b")
    assert torch.equal(a["embedding"], b["embedding"])
    assert np.array_equal(a["attractive_samples"], b["attractive_samples"])
    for s, m in enumerate(graphs["b"][0]):
        lo, hi = off[s], off[s + 1]
        alone = umap.layout(umap.from_scipy([m]), init="pca", x=z["b_X"][lo:hi], n_epochs=40, a=float(z["a"]),
                            b=float(z["b"]), seed=ur.SEED)
        assert torch.equal(alone["embedding"], a["embedding"][lo:hi]), s
        assert alone["attractive_samples"][0] == a["attractive_samples"][s]
        assert alone["negative_samples"][0] == a["negative_samples"][s]
    other = _layout(z, graphs, "b", seed=ur.SEED + 1)
    assert not torch.equal(other["embedding"], a["embedding"])
    assert np.array_equal(other["attractive_samples"], a["attractive_samples"])      # the schedule knows no seed


def test_segments_of_different_length_finish_alone(z, graphs):
    """n_epochs=None is per segment: a ring of 10001 vertices runs 200 epochs, case a's 70 rows run 500 beside it; each
    ends with the bits it has alone, and a batch stopped early is where its segments are alone after as many epochs."""
    from scipy import sparse
    n = 10001
    i = np.arange(n)
    ring = sparse.csr_matrix((1.0 / (1.0 + i % 3), (i, (i + 1) % n)), shape=(n, n))
    ring = (ring + ring.T).tocsr()
    ma = graphs["a"][0][0]
    kw = dict(init="random", a=float(z["a"]), b=float(z["b"]), seed=ur.SEED)
    both = umap.layout(umap.from_scipy([ring, ma]), **kw)
    assert both["n_epochs"].tolist() == [200, 500]
    r_alone, a_alone = umap.layout(umap.from_scipy([ring]), **kw), umap.layout(umap.from_scipy([ma]), **kw)
    assert torch.equal(both["embedding"][:n], r_alone["embedding"]) and torch.equal(both["embedding"][n:], a_alone["embedding"])
    assert both["attractive_samples"].tolist() == [int(r_alone["attractive_samples"][0]), int(a_alone["attractive_samples"][0])]
    assert both["negative_samples"].tolist() == [int(r_alone["negative_samples"][0]), int(a_alone["negative_samples"][0])]
    assert torch.isfinite(both["embedding"]).all()
    early = umap.layout(umap.from_scipy([ring, ma]), stop_after=201, **kw)
    assert torch.equal(early["embedding"][:n], r_alone["embedding"])
    assert torch.equal(early["embedding"][n:], umap.layout(umap.from_scipy([ma]), stop_after=201, **kw)["embedding"])


def test_full_run(z, graphs):
    """Case e: 151 spots, k = 150, the default 500 epochs from a random start."""
    X, lab = z["e_X"], ur.case_labels("e")
    got = umap.layout(graphs["e"][1], init="random", a=float(z["a"]), b=float(z["b"]), seed=ur.FULL_SEEDS[0])
    assert got["n_epochs"].tolist() == [500]
    Y = got["embedding"].cpu().numpy()
    assert np.isfinite(Y).all()
    jac = z["e_trust_jacobi"]
    bound = float(jac.min() - (jac.max() - jac.min()))
    t, p = ur.trustworthiness(X, Y), ur.nn_purity(Y, lab)
    print("e trustworthiness", t, "bound", bound, "purity", p, "extent", float(np.abs(Y).max()))
    assert p == 1.0
    assert t >= bound


@pytest.fixture(scope="module")
def counts():
    """300 spots x 400 genes of synthetic counts: three spot groups, gene means spread over two decades."""
    rng = np.random.RandomState(11)
    base = np.exp(rng.uniform(np.log(0.2), np.log(20.0), size=400))
    group = np.exp(0.8 * rng.standard_normal((3, 400)))
    return rng.poisson(base * group[np.arange(300) % 3]).astype(np.float32)


def test_umap_is_neighbors_then_layout(z):
    X, off = z["b_X"], ur.nr.offsets_of("b")
    kw = dict(n_epochs=25, a=float(z["a"]), b=float(z["b"]), seed=5)
    res = umap.umap(X, off, n_neighbors=20, **kw)
    g = neighbors.neighbors(X, off, 20)
    by_hand = umap.layout(g, "pca", x=X, **kw)
    assert torch.equal(res["embedding"], by_hand["embedding"]) and torch.equal(res["graph"]["data"], g["data"])
    assert np.array_equal(res["negative_samples"], by_hand["negative_samples"]) and res["negative_samples"].min() > 0
    fit = umap.umap(X[:257], None, n_neighbors=20, n_epochs=5)           # a, b from find_ab_params
    assert abs(fit["a"] - 0.5830300) < 1e-6 and abs(fit["b"] - 1.3341670) < 1e-6


def test_expression_umap_and_cli(counts, tmp_path, capsys):
    res = umap.expression_umap(counts, n_top_genes=64, n_pcs=10, n_neighbors=20, n_epochs=30, seed=2)
    capsys.readouterr()
    g = res["graph"]
    by_hand = umap.layout(g, "pca", x=g["scores"], n_epochs=30, seed=2)
    assert res["embedding"].shape == (300, 2) and torch.equal(res["embedding"], by_hand["embedding"])
    assert torch.isfinite(res["embedding"]).all() and res["attractive_samples"][0] > 0
    files = []
    for i, part in enumerate((counts[:160], counts[160:])):
        files.append(str(tmp_path / f"s{i}.npy"))
        np.save(files[-1], np.ascontiguousarray(part.T))                 # gene-major
    out = str(tmp_path / "out")
    assert umap.main(["--pred", *files, "--raw", "--n_top_genes", "64", "--n_pcs", "10", "--n_neighbors", "20",
                      "--n_epochs", "30", "--seed", "2", "--out_dir", out]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("slide ")]
    assert len(lines) == 2 and "160 spots, epochs 30, attractions " in lines[0] and "140 spots" in lines[1]
    assert "negative samples " in lines[0] and "extent " in lines[0]
    for i, n in enumerate((160, 140)):
        Y = np.load(os.path.join(out, str(i + 1), umap.OUT_FILE))
        assert Y.shape == (n, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
