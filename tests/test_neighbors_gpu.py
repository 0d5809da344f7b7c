"""GPU: csrc/neighbors.hip through mclstexp_amd.neighbors against the numpy restatement (tests/neighbors_reference.py) on
the cases of tests/golden/neighbors.npz: the lists exactly, rho where the restatement's own two runs agree, sigma and the
weights within 4 x the uncertainty the fixture recorded, the CSR structure exactly, each later stage also on the
restatement's own lists, determinism, and the notebook function and the CLI end to end."""
import os

import numpy as np
import pytest
import torch

import neighbors_reference as nr
from mclstexp_amd import cluster, neighbors, preprocess

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(nr.GOLDEN)


@pytest.fixture(scope="module")
def ref(z):
    """name -> [graph per segment] of the restatement, computed once."""
    return {name: nr.segments(name, z[f"{name}_X"]) for name in nr.CASES}


@pytest.fixture(scope="module")
def got(z):
    """name -> neighbors() of the whole case, computed once."""
    return {name: neighbors.neighbors(z[f"{name}_X"], nr.offsets_of(name), nr.CASES[name][2]) for name in nr.CASES}


def _csr(res, s):
    from scipy import sparse
    off, nnz_off = res["offsets"], res["nnz_offsets"]
    n = int(off[s + 1] - off[s])
    indptr = res["indptr"].cpu().numpy()[off[s] + s:off[s + 1] + s + 1]
    return sparse.csr_matrix((res["data"].cpu().numpy()[nnz_off[s]:nnz_off[s + 1]],
                              res["indices"].cpu().numpy()[nnz_off[s]:nnz_off[s + 1]], indptr), shape=(n, n))


def _check_csr(m, g, name, z, what):
    want = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"])
    mine = m.copy()
    mine.sort_indices()
    assert np.array_equal(m.indices, mine.indices), what               # the columns of every row already ascend
    assert np.array_equal(m.indptr, want.indptr) and np.array_equal(m.indices, want.indices), what
    assert (m != m.T).nnz == 0 and not m.diagonal().any() and m.data.min() > 0, what
    e = float(np.max(np.abs(m.data - want.data)) / np.max(np.abs(want.data)))
    print(name, what, "data", e, "of", 4 * float(z[f"err_{name}_data"]))
    assert e <= 4 * float(z[f"err_{name}_data"]), what


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_knn(z, ref, got, name):
    off = nr.offsets_of(name)
    idx, dist = got[name]["knn_indices"].cpu().numpy(), got[name]["knn_distances"].cpu().numpy()
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    for s, g in enumerate(ref[name]):
        assert np.array_equal(idx[off[s]:off[s + 1]], g["knn_indices"]), s
        d, d_ref = dist[off[s]:off[s + 1]], g["knn_distances"]
        assert np.all(np.abs(d - d_ref) <= 2.0 ** -51 * d_ref), s          # d^2 identical, sqrt within one ulp
    i2, d2 = neighbors.knn(z[f"{name}_X"], off, nr.CASES[name][2])
    assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(d2.cpu().numpy(), dist)


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_rho_sigma_and_connectivities(z, ref, got, name):
    off = nr.offsets_of(name)
    rho, sigma = got[name]["rho"].cpu().numpy(), got[name]["sigma"].cpu().numpy()
    agree = z[f"{name}_rho_agree"]
    for s, g in enumerate(ref[name]):
        r, sg, ok = rho[off[s]:off[s + 1]], sigma[off[s]:off[s + 1]], agree[off[s]:off[s + 1]]
        assert np.array_equal(r[ok], g["rho"][ok]), s
        print(name, s, "rho", nr.rel(r, g["rho"]), "of", 4 * float(z[f"err_{name}_rho"]), "sigma", nr.rel(sg, g["sigma"]),
              "of", 4 * float(z[f"err_{name}_sigma"]))
        assert nr.rel(r, g["rho"]) <= 4 * float(z[f"err_{name}_rho"]), s
        assert nr.rel(sg, g["sigma"]) <= 4 * float(z[f"err_{name}_sigma"]), s
        _check_csr(_csr(got[name], s), g, name, z, f"segment {s}")
    assert got[name]["nnz_offsets"][-1] == got[name]["data"].numel() == got[name]["indices"].numel()


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_teacher_forced_stages(z, ref, name):
    """mcl_knn_smooth and mcl_knn_connectivities on the restatement's own lists, rho and sigma."""
    off = nr.offsets_of(name)
    gs = ref[name]
    idx = np.concatenate([g["knn_indices"] for g in gs])
    dist = np.concatenate([g["knn_distances"] for g in gs])
    rho_ref, sigma_ref = np.concatenate([g["rho"] for g in gs]), np.concatenate([g["sigma"] for g in gs])
    rho, sigma = neighbors.smooth(dist, off)
    assert np.array_equal(rho.cpu().numpy(), rho_ref)                     # the same distances: the same minimum
    e = max(nr.rel(sigma.cpu().numpy()[off[s]:off[s + 1]], g["sigma"]) for s, g in enumerate(gs))
    print(name, "sigma", e, "of", 4 * float(z[f"err_{name}_sigma"]))
    assert e <= 4 * float(z[f"err_{name}_sigma"])
    res = neighbors.connectivities(idx, dist, rho_ref, sigma_ref, off)
    for s, g in enumerate(gs):
        _check_csr(_csr(res, s), g, name, z, f"forced segment {s}")
    # the intersection (mix 0) against the restatement's
    inter = neighbors.connectivities(idx, dist, rho_ref, sigma_ref, off, set_op_mix_ratio=0.0)
    for s, g in enumerate(gs):
        want = nr.connectivities(g["knn_indices"], g["knn_distances"], g["rho"], g["sigma"], 0.0)
        m = _csr(inter, s)
        assert np.array_equal(m.indptr, want.indptr) and np.array_equal(m.indices, want.indices)
        assert np.max(np.abs(m.data - want.data)) <= 4 * float(z[f"err_{name}_data"]) * np.max(want.data)


def test_batch_is_bit_identical_to_its_slides_and_to_its_repeat(z, got):
    X, off, k = z["b_X"], nr.offsets_of("b"), nr.CASES["b"][2]
    a = got["b"]
    wide = torch.zeros((X.shape[0], 64), dtype=torch.float64)
    wide[:, :50] = torch.from_numpy(X)
    b = neighbors.neighbors(wide.cuda()[:, :50], off, k)                  # on the device with a row stride of 64
    keys = ("knn_indices", "knn_distances", "rho", "sigma", "indptr", "indices", "data")
    for key in keys:
        assert torch.equal(a[key], b[key]), key
    for s in range(3):
        lo, hi = off[s], off[s + 1]
        alone = neighbors.neighbors(X[lo:hi], None, k)
        for key in ("knn_indices", "knn_distances", "rho", "sigma"):
            assert torch.equal(alone[key], a[key][lo:hi]), (s, key)
        assert torch.equal(alone["indptr"], a["indptr"][lo + s:hi + s + 1]), s
        na, nb = a["nnz_offsets"][s], a["nnz_offsets"][s + 1]
        assert torch.equal(alone["indices"], a["indices"][na:nb]) and torch.equal(alone["data"], a["data"][na:nb]), s
    # float32 input: the same lists as the float64 restatement of the rounded values
    X32 = z["a_X"].astype(np.float32)
    i32, d32 = neighbors.knn(X32, None, nr.CASES["a"][2])
    want_i, want_d, _ = nr.knn(X32.astype(np.float64), nr.CASES["a"][2])
    assert np.array_equal(i32.cpu().numpy(), want_i) and np.all(np.abs(d32.cpu().numpy() - want_d) <= 2.0 ** -51 * want_d)


@pytest.fixture(scope="module")
def counts():
    """300 spots x 400 genes of synthetic counts: three spot groups, gene means spread over two decades."""
    rng = np.random.RandomState(11)
    base = np.exp(rng.uniform(np.log(0.2), np.log(20.0), size=400))
    group = np.exp(0.8 * rng.standard_normal((3, 400)))
    return rng.poisson(base * group[np.arange(300) % 3]).astype(np.float32)


def test_expression_graph(counts, capsys):
    res = neighbors.expression_graph(counts, batch_idx="kept", n_top_genes=64, n_pcs=10, n_neighbors=20)
    assert "n_top_genes:  " in capsys.readouterr().out and res["batch_idx"] == "kept"
    hv = preprocess.gene_stats([counts], None, 64)["highly_variable"][0]
    genes = np.flatnonzero(hv.cpu().numpy())
    assert 0 < genes.size <= 64 and torch.equal(res["highly_variable"], hv)
    x = preprocess.expression_matrices([counts], None, genes)[0].T
    scores = cluster.pca_device(x, None, 10)["scores"]
    by_hand = neighbors.neighbors(scores, None, 20)
    assert torch.equal(res["scores"], scores) and res["knn_indices"].shape == (300, 20)
    for key in ("knn_indices", "knn_distances", "rho", "sigma", "indptr", "indices", "data"):
        assert torch.equal(res[key], by_hand[key]), key
    # the graph is the restatement's on the same scores
    g = nr.graph(scores.cpu().numpy(), 20)
    assert np.array_equal(res["knn_indices"].cpu().numpy(), g["knn_indices"])
    # preprocess=False: the PCA of the matrix as given
    plain = neighbors.expression_graph(x, preprocess=False, n_pcs=10, n_neighbors=20)
    assert plain["highly_variable"] is None and torch.equal(plain["knn_indices"], res["knn_indices"])
    with pytest.raises(ValueError, match="gene_stats normalises"):
        neighbors.expression_graph(counts, preprocess=True, normalize_and_log=False, n_top_genes=64, n_pcs=10,
                                   n_neighbors=20)


def test_cli_writes_one_graph_per_slide(counts, tmp_path, capsys):
    files = []
    for i, part in enumerate((counts[:160], counts[160:])):
        files.append(str(tmp_path / f"s{i}.npy"))
        np.save(files[-1], np.ascontiguousarray(part.T))                 # gene-major
    out = str(tmp_path / "out")
    assert neighbors.main(["--pred", *files, "--raw", "--n_top_genes", "64", "--n_pcs", "10", "--n_neighbors", "20",
                           "--out_dir", out]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("slide ")]
    assert len(lines) == 2 and "160 spots, k 20, nnz " in lines[0] and "140 spots" in lines[1] and "sigma " in lines[0]
    from scipy import sparse
    for i, n in enumerate((160, 140)):
        f = np.load(os.path.join(out, str(i + 1), neighbors.OUT_FILE))
        assert f["knn_indices"].shape == (n, 20) and np.array_equal(f["knn_indices"][:, 0], np.arange(n))
        c = sparse.csr_matrix((f["connectivities_data"], f["connectivities_indices"], f["connectivities_indptr"]), shape=(n, n))
        d = sparse.csr_matrix((f["distances_data"], f["distances_indices"], f["distances_indptr"]), shape=(n, n))
        assert (c != c.T).nnz == 0 and c.nnz >= d.nnz == n * 19 and f"nnz {c.nnz}" in lines[i]
