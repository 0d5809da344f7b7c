"""CPU: the numpy restatement tests/spatial_reference.py against the fixture tests/golden/spatial.npz (the reference's own
``calcADJ``, dense-matrix formulas, scipy, mpmath), the host-side rules of mclstexp_amd.spatial, and its CLI parser.

Bounds (eps = 2^-52): a dense-formula I or C of n spots and k neighbours carries about (n + k) eps of its own, as the
restatement does: the comparison allows 8 (n + k) eps (relative for C and S0 / S1 / S2, absolute x max|I| scale 1 for I,
which passes through zero).  sf(|z|) is conditioned like z^2: (2 z^2 + 16) eps relative; -log10 p in log space 16 eps."""
import math

import numpy as np
import pytest
import torch

import spatial_reference as sr
from golden.gen_spatial_goldens import KS, PERM_P, PERM_SEED, TAIL_MP

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


def fake_graph(sizes, k=4):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {"nbr": None, "w": None, "consts": None, "offsets": off, "k": k}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_adjacency_is_calcadj(golden, name):
    coords, _ = sr.make_case(name)
    n = coords.shape[0]
    for k in KS:
        for prune in sr.PRUNES:
            want = np.unpackbits(golden[f"{name}.adj.{prune}.{k}"])[:n * n].reshape(n, n).astype(bool)
            for std in (False, True):
                g = sr.lattice(coords, k, prune, std)
                W = sr.dense(g["nbr"], g["w"])
                assert np.array_equal(W != 0, want), (name, k, prune)
                assert np.array_equal(g["deg"], want.sum(axis=1))
                if std:
                    rs = W.sum(axis=1)
                    assert np.all(np.abs(rs[g["deg"] > 0] - 1.0) <= k * EPS) and np.all(rs[g["deg"] == 0] == 0)
                else:
                    assert set(np.unique(W)) <= {0.0, 1.0}
    assert want.sum() < n * 8                      # (Grid pruning removed edges: the border spots)


def test_tie_rule_on_an_exact_lattice(golden):
    from golden.gen_spatial_goldens import LATTICE
    lat = sr.make_coords(LATTICE["gr"], LATTICE["gc"], LATTICE["seed"], integer=True)
    g = sr.lattice(lat, 8, "Grid", True)
    assert np.array_equal(g["nbr"], golden["lattice.nbr"]) and np.array_equal(g["deg"], golden["lattice.deg"])
    # ascending (distance, index): equal distances are listed by ascending index
    d = g["dist"]
    tied = d[:, 1:] == d[:, :-1]
    assert tied.any() and np.all(g["nbr"][:, 1:][tied] > g["nbr"][:, :-1][tied])
    # a corner spot keeps its 3 lattice neighbours within 2 and the 2 at distance 2 exactly
    assert g["deg"].min() == 5 and g["deg"].max() == 8


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_statistics_match_the_dense_formulas(golden, name):
    coords, x = sr.make_case(name)
    n, k = coords.shape[0], 8
    tol = 8 * (n + k) * EPS
    for std, tag in ((False, "b"), (True, "r")):
        g = sr.lattice(coords, k, "STD", std)
        I, C = sr.statistics(x, g["nbr"], g["w"], g["S0"])
        S = np.array([g["S0"], g["S1"], g["S2"]])
        assert np.all(np.abs(S - golden[f"{name}.S.{tag}"]) <= tol * golden[f"{name}.S.{tag}"])
        assert np.all(np.abs(I - golden[f"{name}.I.{tag}"]) <= tol)
        assert np.all(np.abs(C - golden[f"{name}.C.{tag}"]) <= tol * golden[f"{name}.C.{tag}"])
    for key in ("err_I", "err_C", "err_S", "err_simI", "err_simC"):
        assert float(golden[f"{name}.{key}"]) <= tol
    perms = golden[f"{name}.perms"].astype(np.int64)
    assert np.array_equal(perms, sr.permutations(PERM_SEED, PERM_P, n))
    sI, sC = sr.simulate(x, g["nbr"], g["w"], g["S0"], perms)
    assert np.all(np.abs(sI - golden[f"{name}.simI"]) <= tol)
    assert np.all(np.abs(sC - golden[f"{name}.simC"]) <= tol * golden[f"{name}.simC"])
    # the identity permutation is the observed statistic, bit for bit
    iI, iC = sr.simulate(x, g["nbr"], g["w"], g["S0"], [np.arange(n)])
    assert np.array_equal(iI[0], I) and np.array_equal(iC[0], C)


def test_moments_and_a_symmetric_graph():
    """On a symmetric binary graph S1 = 2 S0 and S2 = 4 sum deg^2; E[I] = -1 / (n - 1); a checkerboard has I < 0 < a
    gradient's I and C > 1 > the gradient's C."""
    lat = sr.make_coords(6, 7, 0, integer=True)
    g = sr.lattice(lat, 4, "Grid", False)              # k = 4: rook neighbours, border rows hold distance-2 / sqrt(2) fill-ins
    W = sr.dense(g["nbr"], g["w"])
    sym = np.array_equal(W, W.T)
    S = (W.sum(), 0.5 * ((W + W.T) ** 2).sum(), ((W.sum(axis=1) + W.sum(axis=0)) ** 2).sum())
    assert (g["S0"], g["S1"], g["S2"]) == S
    if sym:
        assert S[1] == 2 * S[0]
    x = np.stack([(lat.sum(axis=1) % 2).astype(float), lat[:, 0].astype(float), np.full(lat.shape[0], 3.0)], axis=1)
    I, C = sr.statistics(x, g["nbr"], g["w"], g["S0"])
    assert I[0] < 0 < I[1] and C[0] > 1 > C[1]
    assert np.isnan(I[2]) and np.isnan(C[2])           # a constant gene
    EI, VI, EC, VC = sr.moments(42, *S)
    assert EI == -1 / 41 and EC == 1.0 and VI > 0 and VC > 0
    r = sr.autocorr(x, lat, 4, "Grid", False, n_perms=5)
    for m in ("moran", "geary"):
        for key in ("stat", "z_norm", "pval_norm", "neglog10_pval_norm", "pval_norm_adj", "pval_sim", "pval_z_sim"):
            assert np.isnan(r[m][key][2]) and not np.isnan(r[m][key][:2]).any(), (m, key)


def test_tails_and_bh(golden):
    z = golden["tail.z"]
    for two in (False, True):
        p, nl = sr.normal_tail(z, two)
        want = golden["tail.sf"] * (2 if two else 1)
        assert np.all(np.abs(p - want) <= (2 * z * z + 16) * EPS * want)
        assert np.all(np.abs(nl - (0.0 - np.log10(want))) <= (2 * z * z + 16) * EPS / sr.LN10 + 16 * EPS * nl)
        big, nlb = sr.normal_tail(np.array(TAIL_MP), two)
        mp = golden["tail.nl_mp2" if two else "tail.nl_mp1"]
        assert big[1] == 0.0 and np.all(np.isfinite(nlb)) and np.all(np.abs(nlb - mp) <= 16 * EPS * mp)
    assert float(golden["tail.err_nl"]) <= 16 * EPS
    p = golden["bh.p"]
    assert np.all(np.abs(sr.bh(p) - golden["bh.adj"]) <= 4 * EPS * golden["bh.adj"])
    withnan = np.concatenate([p[:5], [np.nan]])
    adj = sr.bh(withnan)
    assert np.isnan(adj[5]) and np.array_equal(adj[:5], sr.bh(np.concatenate([p[:5], [1.0]]))[:5])


def test_fixed_sum_and_perm_summary():
    rng = np.random.default_rng(0)
    for n in (1, 2, 255, 256, 257, 1000, 4097):
        v = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4, size=(n, 3))
        got = sr.fixed_sum(v)
        for j in range(3):
            assert abs(got[j] - math.fsum(v[:, j])) <= (-(-n // 256) + 8) * EPS * np.abs(v[:, j]).sum()
    stat = np.array([0.5, 0.5, np.nan, -1.0])
    sims = np.array([[0.1, 0.9, 0.0, 0.0], [0.5, 0.8, 0.0, 0.0], [0.7, 0.7, 0.0, 0.0], [0.2, 0.6, 0.0, 0.0]])
    r = sr.perm_summary(stat, sims)
    assert r["count_sim"].tolist() == [2, 0, -1, 0]                 # 2 of 4; 4 folded to 0; NaN; 4 folded to 0
    assert np.allclose(r["pval_sim"][[0, 1, 3]], [3 / 5, 1 / 5, 1 / 5]) and np.isnan(r["pval_sim"][2])
    assert np.allclose(r["var_sim"], sims.var(axis=0)) and np.allclose(r["mean_sim"], sims.mean(axis=0))


@pytest.mark.parametrize("n", [2, 16384])
def test_keys_are_unique_and_every_pi_a_permutation(n):
    for seed, p in ((0, 0), (0, 1), (2 ** 64 - 1, 7), (12345, 999)):
        keys = sr.perm_keys(seed, p, n)
        assert keys.dtype == np.uint64 and np.unique(keys).size == n
        assert np.array_equal(keys & np.uint64(0x3FFF), np.arange(n, dtype=np.uint64))
        pi = sr.permutation(seed, p, n)
        assert np.array_equal(np.sort(pi), np.arange(n))
    assert not np.array_equal(sr.permutation(0, 0, n), sr.permutation(0, 1, n)) or n == 2
    assert not np.array_equal(sr.permutation(0, 0, 16384), sr.permutation(1, 0, 16384))


def test_splitmix64_is_the_published_stream():
    """The first outputs of splitmix64 seeded with 0 (Vigna's reference implementation)."""
    state = np.uint64(0)
    got = []
    for _ in range(3):
        got.append(int(sr.mix(np.array([state]))[0]))
        with np.errstate(over="ignore"):
            state = state + np.uint64(0x9E3779B97F4A7C15)
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


# ----------------------------------------------------------------------------------------------------- host rules
def test_lattice_validation():
    from mclstexp_amd import spatial
    c = np.zeros((10, 2))
    bad = [
        (dict(coords=np.zeros((10, 3))), "rows, 2"),
        (dict(coords=np.zeros(10)), "rows, 2"),
        (dict(coords=c, k=0), "k must be"),
        (dict(coords=c, k=65), "k must be"),
        (dict(coords=c, k=2.0), "k must be"),
        (dict(coords=c, k=True), "k must be"),
        (dict(coords=c, k=10), "at least 11 spots"),
        (dict(coords=c, offsets=[0, 5, 10], k=5), "at least 6 spots"),
        (dict(coords=c, offsets=[0, 5, 9]), "offsets"),
        (dict(coords=c, prune="std"), "prune must be"),
        (dict(coords=c, row_standardise=1), "row_standardise"),
        (dict(), "needs coords"),
        (dict(coords=c, nbr=np.zeros((10, 2), np.int32), w=np.ones((10, 2))), "no coords"),
        (dict(nbr=np.zeros((10, 2), np.int32)), "both nbr= and w="),
        (dict(nbr=np.zeros(10, np.int32), w=np.ones(10)), "2-D"),
        (dict(nbr=np.zeros((10, 70), np.int32), w=np.ones((10, 70))), "k must be"),
        (dict(nbr=np.zeros((10, 2), np.int32), w=np.full((10, 2), np.nan)), "finite"),
        (dict(nbr=np.zeros((10, 2), np.int32), w=np.full((10, 2), np.inf)), "finite"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            spatial.lattice(**kw)
    with pytest.raises(ValueError, match="16384"):
        spatial.check_lattice((16385, 2), None, 8, "NA", True)
    off, k, code = spatial.check_lattice((9, 2), None, 8, "Grid", False)
    assert off.tolist() == [0, 9] and (k, code) == (8, 2)


def test_autocorr_validation():
    from mclstexp_amd import spatial
    g = fake_graph([6, 4])
    x = np.zeros((10, 3))
    bad = [
        (dict(x=np.zeros(10), graph=g), "2-D"),
        (dict(x=np.zeros((10, 0)), graph=g), "genes per call"),
        (dict(x=np.zeros((10, 16385)), graph=g), "genes per call"),
        (dict(x=np.zeros((9, 3)), graph=g), "9 rows"),
        (dict(x=x, graph={"nbr": None}), "lattice"),
        (dict(x=x, graph=g, mode="morans"), "mode must be"),
        (dict(x=x, graph=g, n_perms=-1), "n_perms"),
        (dict(x=x, graph=g, n_perms=1.5), "n_perms"),
        (dict(x=x, graph=g, n_perms=65536), "n_perms"),
        (dict(x=x, graph=g, seed=-1), "seed"),
        (dict(x=x, graph=g, two_tailed=1), "two_tailed"),
        (dict(x=x, graph=g, return_sims="yes"), "return_sims"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None]]), "list of 2"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None], np.arange(5)[None]]), r"permutations\[1\]"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None], np.arange(4.0)[None]]), r"permutations\[1\]"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None], np.array([[0, 1, 2, 2]])]), "row 0 is not a permutation"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None], np.array([[0, 1, 2, 4]])]), "not a permutation"),
        (dict(x=x, graph=g, permutations=[np.arange(6)[None], np.stack([np.arange(4)] * 2)]), "same"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            spatial.autocorr(**kw)
    table = spatial.check_permutations([np.array([[1, 0, 2]]), np.array([[0, 1], ])], np.array([3, 2]))
    assert table.dtype == np.int16 and table.tolist() == [1, 0, 2, 0, 1]
    with pytest.raises(ValueError, match="one coordinate array per slide"):
        spatial.autocorr_slides([x], [])
    with pytest.raises(ValueError, match="do not match"):
        spatial.autocorr_slides([x], [np.zeros((9, 2))])
    with pytest.raises(ValueError, match="n_top"):
        spatial.svg_recovery([x], [x], [np.zeros((10, 2))], n_top=0)
    with pytest.raises(ValueError, match="differ in shape"):
        spatial.svg_recovery([x], [x[:5]], [np.zeros((10, 2))])
    with pytest.raises(ValueError, match="'moran' or 'geary'"):
        spatial.svg_recovery([x], [x], [np.zeros((10, 2))], mode="both")


def test_host_helpers_match_the_restatement():
    from mclstexp_amd import _lib, build, spatial
    import os
    v = np.array([0.3, np.nan, 0.9, 0.3, -0.2])
    assert spatial.rank_genes(v, "moran").tolist() == sr.rank_genes(v, "moran").tolist() == [2, 0, 3, 4, 1]
    assert spatial.rank_genes(v, "geary").tolist() == [4, 0, 3, 2, 1]
    res = [{"moran": {"stat": v}}]
    assert spatial.top_genes(res, 0, 2).tolist() == [2, 0] and spatial.top_genes(res, 0, 99).size == 5
    a, b = np.array([1.0, 2.0, np.nan, 4.0, 0.0]), np.array([2.0, 1.0, 5.0, 9.0, 1.0])
    assert abs(spatial.pearson(a, b) - sr.recovery(a, b, 2)[0]) < 1e-15
    mom = spatial.expected_moments(100, 800.0, 150.0, 6500.0)
    EI, VI, EC, VC = sr.moments(100, 800.0, 150.0, 6500.0)
    assert (mom["EI"], mom["EC"]) == (EI, EC) and abs(mom["VI"] - VI) < 1e-15 and abs(mom["VC"] - VC) < 1e-15
    # the column rule of the kernel, read from the library itself (no GPU needed)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    for n in (2, 9, 3242, 3243, 3891, 3892, 4000, 4864, 4865, 6485, 9728, 9729, 16384):
        assert lib.mcl_spatial_columns(n) == sr.columns(n), n
    assert lib.mcl_spatial_columns(1) == -1 and lib.mcl_spatial_columns(16385) == -1
    assert lib.mcl_spatial_workspace_bytes(100, 9, 0) >= 100 * 9 * 4
    assert lib.mcl_spatial_workspace_bytes(100, 0, 7) >= 100 * 7 * 2
    assert lib.mcl_spatial_workspace_bytes(1, 0, 0) == -1 and lib.mcl_spatial_workspace_bytes(100, 66, 0) == -1
    assert lib.mcl_spatial_lattice(None, None, None, 1, 10, 10, 8, 0, 1, 0, None, None, None, None, None, None, None) == -1
    assert lib.mcl_spatial_stats(None, 0, 0, None, 1, 10, 3, 10, 8, 2, None, None, None, None, 1, None, None, None, None,
                                 None) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU error")
def test_no_cpu_fallback():
    from mclstexp_amd import spatial
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spatial.lattice(np.random.default_rng(0).random((12, 2)), k=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spatial.autocorr(np.zeros((10, 3)), fake_graph([6, 4]))


def test_cli_parser():
    from mclstexp_amd import spatial
    a = spatial.parse_args(["--pred", "p0.npy", "p1.npy", "--coords", "c0.npy", "c1.npy"])
    assert (a.k, a.prune, a.mode, a.n_perms, a.seed, a.true, a.genes, a.out_dir) == (8, "NA", "moran", 100, 0, None, None, None)
    a = spatial.parse_args(["--pred", "p.npy", "--coords", "c.npy", "--true", "t.npy", "--k", "6", "--prune", "Grid", "--mode",
                            "both", "--n_perms", "0", "--seed", "3", "--genes", "g.npy", "--out_dir", "D"])
    assert (a.k, a.prune, a.mode, a.n_perms, a.seed, a.true, a.genes, a.out_dir) == (6, "Grid", "both", 0, 3, ["t.npy"],
                                                                                    "g.npy", "D")
    for argv in (["--pred", "p.npy"], ["--pred", "p.npy", "--coords", "a.npy", "b.npy"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--true", "a.npy", "b.npy"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--k", "0"], ["--pred", "p.npy", "--coords", "c.npy", "--k", "65"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--prune", "grid"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--mode", "lisa"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--n_perms", "-1"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--seed", "-1"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--top", "0"]):
        with pytest.raises(SystemExit):
            spatial.parse_args(argv)
    r = {"n": 5, "moran": {"stat": np.arange(3.0), "sims": np.zeros((2, 3))}, "mean": np.zeros(3)}
    flat = spatial.flatten(r)
    assert set(flat) == {"n", "moran_stat", "moran_sims", "mean"} and flat["moran_sims"].shape == (2, 3)
