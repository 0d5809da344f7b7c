"""GPU: csrc/leiden.hip through mclstexp_amd.leiden against the numpy restatement (tests/leiden_reference.py) on its case
table: labels, counters and Q, the recorded networkx bound, connectedness, determinism, a slide alone against the same slide
in a batch, the restart from a partition, the building blocks, and the notebook function and the CLI end to end.  The graphs
are the restatement's own, handed over through umap.from_scipy, so that both sides start from the same bits."""
import os

import numpy as np
import pytest
import torch
from scipy import sparse

import leiden_reference as lr
from mclstexp_amd import leiden, neighbors, umap

pytestmark = pytest.mark.gpu
COUNTERS = ("n_clusters", "levels", "sweeps", "accepted_sweeps", "rounds", "iterations")


@pytest.fixture(scope="module")
def z():
    return np.load(lr.GOLDEN)


@pytest.fixture(scope="module")
def graphs():
    """name -> (scipy CSR per slide, the dict leiden() takes), computed once."""
    return {name: (ms, umap.from_scipy(ms)) for name, ms in ((n, lr.case_graphs(n)) for n in lr.CASES)}


@pytest.fixture(scope="module")
def ref(graphs):
    """(name, slide, resolution) -> the restatement's run, computed once."""
    return {(name, s, g): lr.run(m, g) for name, gs in lr.CASES.items() for s, m in enumerate(graphs[name][0]) for g in gs}


@pytest.fixture(scope="module")
def got(graphs):
    """(name, resolution) -> the device's run of the whole batch, computed once."""
    return {(name, g): leiden.leiden(graphs[name][1], resolution=g) for name, gs in lr.CASES.items() for g in gs}


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("name", list(lr.CASES))
def test_equals_the_restatement(z, graphs, ref, got, name):
    ms, g = graphs[name]
    for gamma in lr.CASES[name]:
        res = got[(name, gamma)]
        assert res["labels"].dtype == torch.int32 and res["labels"].shape == (g["offsets"][-1],)
        assert res["modularity"].dtype == np.float64 and np.array_equal(res["offsets"], g["offsets"])
        labels = res["labels"].cpu().numpy()
        again = leiden.modularity(g, res["labels"], gamma)
        for s, m in enumerate(ms):
            r, lab = ref[(name, s, gamma)], labels[g["offsets"][s]:g["offsets"][s + 1]]
            q = float(res["modularity"][s])
            print(name, s, gamma, {c: int(res[c][s]) for c in COUNTERS}, "Q", q, "restatement", r["modularity"])
            assert np.array_equal(lab, r["labels"]), (name, s, gamma)
            for c in COUNTERS:
                assert int(res[c][s]) == int(r[c]), (name, s, gamma, c)
            assert rel(q, r["modularity"]) <= 1e-12 if r["modularity"] else q == 0.0
            assert q == float(again[s])
            assert lab.min() == 0 and lab.max() == int(res["n_clusters"][s]) - 1
            assert lr.connected(m, lab)
            if name in lr.BOUNDED:
                lou = z[f"{name}_{s}_{gamma}_louvain"]
                bound = float(lou.min() - (lou.max() - lou.min()))
                print(name, s, gamma, "networkx Louvain", float(lou.min()), "..", float(lou.max()), "bound", bound)
                assert q >= bound


def test_resolutions(got):
    name = lr.RESOLUTION_CASE
    assert set(lr.CASES[name]) >= {0.5, 1.0, 2.0}              # (each equals the restatement: test_equals_the_restatement)
    counts = [int(got[(name, g)]["n_clusters"][0]) for g in sorted(lr.CASES[name])]
    assert counts == sorted(counts) and counts[-1] > counts[0]


def test_determinism_and_a_slide_alone(graphs, got):
    ms, g = graphs["b"]
    a, b = got[("b", 1.0)], leiden.leiden(g)
    assert torch.equal(a["labels"], b["labels"]) and np.array_equal(a["modularity"], b["modularity"])
    for c in COUNTERS:
        assert np.array_equal(a[c], b[c]), c
    off = g["offsets"]
    for s, m in enumerate(ms):
        alone = leiden.leiden(umap.from_scipy([m]))
        assert torch.equal(alone["labels"], a["labels"][off[s]:off[s + 1]]), s
        assert alone["modularity"][0] == a["modularity"][s]
        for c in COUNTERS:
            assert alone[c][0] == a[c][s], (s, c)
    # the slide with 2m = 0 beside one with edges, and that one alone
    ring = leiden.leiden(umap.from_scipy(graphs["ring"][0]))
    both = got[("empty", 1.0)]
    assert torch.equal(both["labels"][7:], ring["labels"]) and both["labels"][:7].tolist() == list(range(7))
    assert both["modularity"].tolist() == [0.0, float(ring["modularity"][0])] and both["iterations"].tolist() == [0, 2]


def test_restart_from_the_partition_found(graphs, got):
    for name in ("b", "blobs", "star"):
        g, first = graphs[name][1], got[(name, 1.0)]
        for start in (first["labels"], first["labels"].cpu().numpy().astype(np.int64) * 3 + 5):          # device, host
            res = leiden.leiden(g, partition=start)
            assert torch.equal(res["labels"], first["labels"]), name
            assert res["iterations"].tolist() == [1] * len(graphs[name][0]) and not res["accepted_sweeps"].any()
            assert np.array_equal(res["modularity"], first["modularity"])
    one = leiden.leiden(graphs["d"][1], n_iterations=1)
    assert one["iterations"].tolist() == [1]
    r = lr.run(graphs["d"][0][0], 1.0, n_iterations=1)
    assert np.array_equal(one["labels"].cpu().numpy(), r["labels"]) and int(one["sweeps"][0]) == r["sweeps"]


def test_refine_parts_what_has_no_edge_between_it(graphs):
    """Two cliques with no edge between them in one community come back apart (plain Louvain cannot do this), next to a
    second slide; and the refinement of the partition found on case blobs equals the restatement's."""
    r, c, n = lr._cliques([5, 6])
    m = sparse.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    blobs = graphs["blobs"][0][0]
    g = umap.from_scipy([m, blobs])
    start = np.concatenate([np.zeros(n, dtype=np.int64), lr.run(blobs, 1.0)["labels"]])
    got = leiden.refine(g, start).cpu().numpy()
    assert got.dtype == np.int32 and got[:n].tolist() == [0] * 5 + [5] * 6
    assert np.array_equal(got[:n], lr.refine(m, start[:n])) and np.array_equal(got[n:], lr.refine(blobs, start[n:]))
    assert lr.connected(blobs, got[n:])
    star = graphs["star"][0][0]                               # the dense path, from one community
    zero = np.zeros(star.shape[0], dtype=np.int64)
    assert np.array_equal(leiden.refine(graphs["star"][1], zero).cpu().numpy(), lr.refine(star, zero))


def test_modularity_of_given_labels(graphs):
    ms, g = graphs["b"]
    rng = np.random.RandomState(9)
    labels = rng.randint(0, 5, size=int(g["offsets"][-1])) * 11
    q = leiden.modularity(g, labels, 1.5)
    assert q.shape == (3,) and np.array_equal(q, leiden.modularity(g, torch.from_numpy(labels).cuda(), 1.5))
    for s, m in enumerate(ms):
        want = lr.modularity(m, labels[g["offsets"][s]:g["offsets"][s + 1]], 1.5)
        assert rel(float(q[s]), want) <= 1e-12, s


def test_caps_raise(graphs):
    with pytest.raises(RuntimeError, match="reached a cap"):
        leiden.leiden(graphs["blobs"][1], max_sweeps=2)
    with pytest.raises(RuntimeError, match="reached a cap"):
        leiden.leiden(graphs["blobs"][1], max_levels=1)


def test_cluster_is_neighbors_then_leiden():
    X, off = lr.nr.make_case("b"), lr.nr.offsets_of("b")
    res = leiden.cluster(X, off, n_neighbors=20, resolution=0.8)
    g = neighbors.neighbors(X, off, 20)
    by_hand = leiden.leiden(g, resolution=0.8)
    assert torch.equal(res["labels"], by_hand["labels"]) and torch.equal(res["graph"]["data"], g["data"])
    assert np.array_equal(res["modularity"], by_hand["modularity"]) and res["n_clusters"].min() >= 2
    for s in range(3):                                         # the device's graph, through the restatement
        conn = neighbors.to_scipy(g, s)[1]
        r = lr.run(conn, 0.8)
        assert np.array_equal(res["labels"][off[s]:off[s + 1]].cpu().numpy(), r["labels"]), s


@pytest.fixture(scope="module")
def counts():
    """300 spots x 400 genes of synthetic counts: three spot groups, gene means spread over two decades."""
    rng = np.random.RandomState(11)
    base = np.exp(rng.uniform(np.log(0.2), np.log(20.0), size=400))
    group = np.exp(0.8 * rng.standard_normal((3, 400)))
    return rng.poisson(base * group[np.arange(300) % 3]).astype(np.float32)


def test_expression_clusters_and_cli(counts, tmp_path, capsys):
    kw = dict(n_top_genes=64, n_pcs=10, n_neighbors=20)
    res = leiden.expression_clusters(counts, umap_kw=dict(n_epochs=30, seed=2), **kw)
    lay = umap.expression_umap(counts, n_epochs=30, seed=2, **kw)
    assert res["embedding"].shape == (300, 2) and torch.equal(res["embedding"], lay["embedding"])
    lab = res["labels"].cpu().numpy()
    assert lab.shape == (300,) and lab.min() == 0 and lab.max() == int(res["n_clusters"][0]) - 1 >= 1
    assert torch.equal(res["labels"], leiden.leiden(res["graph"])["labels"])
    assert leiden.expression_clusters(counts, layout=False, **kw)["embedding"] is None
    capsys.readouterr()
    files = []
    for i, part in enumerate((counts[:160], counts[160:])):
        files.append(str(tmp_path / f"s{i}.npy"))
        np.save(files[-1], np.ascontiguousarray(part.T))                 # gene-major
    out = str(tmp_path / "out")
    args = ["--pred", *files, "--raw", "--n_top_genes", "64", "--n_pcs", "10", "--n_neighbors", "20", "--out_dir", out]
    assert leiden.main(args + ["--umap", "--n_epochs", "30", "--seed", "2"]) == 0
    lines = capsys.readouterr().out.splitlines()
    found = [ln for ln in lines if ln.startswith("n_clusters:  ")]
    assert len(found) == 2 and sum(ln.startswith("modularity ") for ln in lines) == 2
    for i, (n, part) in enumerate(((160, counts[:160]), (140, counts[160:]))):
        lab = np.load(os.path.join(out, str(i + 1), leiden.OUT_FILE))
        assert lab.shape == (n,) and lab.dtype == np.int32
        assert lab.min() == 0 and lab.max() == int(found[i].split()[-1]) - 1
        Y = np.load(os.path.join(out, str(i + 1), umap.OUT_FILE))
        want = umap.expression_umap(part, n_epochs=30, seed=2, **kw)["embedding"].cpu().numpy()
        assert np.array_equal(Y, want)
    out2 = str(tmp_path / "out2")
    assert leiden.main(args[:-1] + [out2]) == 0                          # without --umap: labels only
    assert sorted(os.listdir(os.path.join(out2, "1"))) == [leiden.OUT_FILE]
