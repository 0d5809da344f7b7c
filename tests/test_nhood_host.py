"""CPU: the numpy restatement tests/nhood_reference.py against the fixture tests/golden/nhood.npz (independent statements by
a dense matrix product, ``pandas.crosstab`` and ``scipy.spatial.distance.cdist``), the exact-integer z against numpy's
two-pass form, the edge cases, and the host-side rules of mclstexp_amd.nhood: limits, argument errors, the greedy matching,
the CLI parser and ``mcl_nhood_tile_rows`` (host-callable).

Counts are integers, so every comparison with the independent statements is exact.  The z comparison allows
(P + 8) eps ((|count| + |mean|) / std + |z|): numpy's mean and std are P-term sums (P eps each, relative), and the numerator
count - mean cancels, which turns the relative error of the mean into (|count| + |mean|) / std in units of z."""
import os

import numpy as np
import pytest
import torch

import nhood_reference as nh
import spatial_reference as sr
from golden import gen_nhood_goldens as gen
from mclstexp_amd import nhood as nhd


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(nh.GOLDEN))


def case(golden, name):
    return tuple(golden[f"{name}.{key}"] for key in ("coords", "labels", "nbr", "w", "perms")) + (gen.CASES[name][2],)


# ----------------------------------------------------------------------------------------------------- the fixture
def test_fixture_regenerates_identically(golden):
    again = gen.build()
    assert sorted(again) == sorted(golden)
    for key, v in again.items():
        assert np.array_equal(np.asarray(v), golden[key], equal_nan=np.asarray(v).dtype.kind == "f"), key
    assert os.path.getsize(nh.GOLDEN) < 100 * 1024


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_restatement_is_the_independent_statements_exactly(golden, name):
    coords, labels, nbr, w, perms, K = case(golden, name)
    r = nh.nhood(labels, nbr, w, K, perms=list(perms))
    assert np.array_equal(r["count"], golden[f"{name}.count_dense"])
    assert np.array_equal(r["count"], golden[f"{name}.count_crosstab"])
    assert np.array_equal(r["sims"], golden[f"{name}.sims"])
    assert np.array_equal(perms, sr.permutations(gen.PERM_SEED, gen.PERM_P, r["n"]))
    assert np.array_equal(r["perm_sum"], golden[f"{name}.sims"].sum(axis=0))
    assert np.array_equal(r["n_ge"], (golden[f"{name}.sims"] >= r["count"]).sum(axis=0))
    assert np.array_equal(r["n_le"], (golden[f"{name}.sims"] <= r["count"]).sum(axis=0))
    assert np.array_equal(r["pval_enriched"], r["n_ge"] / float(gen.PERM_P))
    c = nh.co_occurrence(coords, labels, K, golden["radii"])
    assert np.array_equal(c["pairs"], golden[f"{name}.pairs"])
    assert np.array_equal(c["occ"], golden[f"{name}.occ"], equal_nan=True)
    assert (np.diff(c["pairs"], axis=0) >= 0).all() and c["pairs"][0].sum() > 0


@pytest.mark.parametrize("shape,K,P", [((20, 17), 4, 200), ((30, 30), 12, 300)])
def test_exact_integer_z_against_numpy_two_pass(shape, K, P):
    coords, labels = nh.make_stripes(shape[0], shape[1], K)
    rng = np.random.default_rng(5)
    flip = rng.random(labels.size) < 0.15                        # noisy stripes: no count is constant under permutation
    labels = np.where(flip, rng.integers(0, K, labels.size), labels)
    g = sr.lattice(coords, 8, "NA")
    r = nh.nhood(labels, g["nbr"], g["w"], K, n_perms=P, seed=3)
    z, bound = nh.z_bound(r["count"], r["sims"])
    assert np.isfinite(z).all() and np.isfinite(r["zscore"]).all()
    err = np.abs(r["zscore"] - z)
    print(f"{shape} K = {K} P = {P}: largest |z - two-pass| / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    assert np.allclose(r["perm_mean"], r["sims"].mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(r["perm_std"], r["sims"].std(axis=0), rtol=1e-10, atol=0)


def test_module_z_is_the_restated_z_bit_for_bit():
    rng = np.random.default_rng(0)
    P = 65535
    count = rng.integers(0, 1 << 20, (6, 6))
    sims = rng.integers(0, 1 << 20, (8, 6, 6)).astype(object)
    S1 = (sims.sum(axis=0) * (P // 8)).astype(np.int64)           # as if every drawn count came P / 8 times
    S2 = ((sims ** 2).sum(axis=0) * (P // 8)).astype(np.int64)
    assert int(S2.max()) * P > 1 << 63                            # the radicand's P S2 passes int64
    z, mean, std = nhd.zscore(count, S1, S2, (P // 8) * 8)
    assert np.array_equal(z, nh.zscore(count, S1, S2, (P // 8) * 8)) and np.isfinite(z).all()
    # the int64 accumulators' largest case: every count 2^20, P = 4: the radicand is exactly 0
    full = np.full((1, 1), 1 << 20, dtype=np.int64)
    z, mean, std = nhd.zscore(full, 4 * full, 4 * full * full, 4)
    assert np.isnan(z).all() and mean[0, 0] == float(1 << 20) and std[0, 0] == 0.0


# ------------------------------------------------------------------------------------------------------ edge cases
def test_edge_cases(golden):
    coords, labels, nbr, w, perms, K = case(golden, "seven")
    r = nh.nhood(labels, nbr, w, K, perms=list(perms))
    assert (labels == -1).any() and r["n"] == (labels >= 0).sum() and (w == 0).any()       # dropped spots, pruned slots
    assert r["sizes"][3] == 0 and r["sizes"][6] == 1
    assert (r["count"][3] == 0).all() and (r["count"][:, 3] == 0).all()
    assert np.isnan(r["zscore"][3]).all() and np.isnan(r["zscore"][:, 3]).all()             # the empty group: radicand 0
    assert (r["n_ge"][3] == gen.PERM_P).all() and (r["n_le"][3] == gen.PERM_P).all()
    assert np.isfinite(r["zscore"][0, 0]) and r["count"].sum() == ((w != 0) & (labels[:, None] >= 0) & (labels[nbr] >= 0)).sum()
    # a pruned slot does not count, whatever its index; a kept slot pointing outside the slide counts as pruned and is reported
    nbr2, w2 = nbr.copy(), w.copy()
    i, c = np.argwhere(w2 != 0)[0]
    w2[i, c] = 0.0
    nbr2[i, c] = 10 ** 6
    assert nh.nhood(labels, nbr2, w2, K)["bad_index"] == 0
    assert nh.nhood(labels, nbr2, w2, K)["count"].sum() == r["count"].sum() - (labels[i] >= 0 and labels[nbr[i, c]] >= 0)
    w2[i, c] = 1.0
    bad = nh.nhood(labels, nbr2, w2, K)
    assert bad["bad_index"] == 1 and np.array_equal(bad["count"], nh.nhood(labels, nbr, np.where(w2 == w, w, 0.0), K)["count"])
    nbr2[i, c] = -1
    assert nh.nhood(labels, nbr2, w2, K)["bad_index"] == 1
    # one group: every permuted count is the observed one
    one = nh.nhood(np.zeros(labels.size, dtype=np.int64), nbr, w, 1, n_perms=5)
    assert np.isnan(one["zscore"]).all() and one["n_ge"][0, 0] == 5 and one["n_le"][0, 0] == 5
    # zero and one kept spot: counts 0, the identity as the only permutation
    for kept in (0, 1):
        lab = np.full(labels.size, -1)
        lab[:kept] = 0
        e = nh.nhood(lab, nbr, w, 2, n_perms=3)
        assert e["n"] == kept and (e["count"] == 0).all() and np.isnan(e["zscore"]).all()
        o = nh.co_occurrence(coords, lab, 2, 4)
        assert (o["pairs"] == 0).all() and np.isnan(o["occ"]).all() and np.array_equal(o["radii"], np.linspace(0.25, 1, 4))
    # coincident spots count at every radius; a radius below every other distance leaves only them
    assert np.array_equal(coords[4], coords[5]) and labels[4] >= 0 and labels[5] >= 0
    o = nh.co_occurrence(coords, labels, K, np.array([0.5, 1.0]))
    assert o["pairs"][0].sum() == 2 and o["pairs"][0][labels[4], labels[5]] >= 1
    c2, l2 = case(golden, "two")[:2]
    o = nh.co_occurrence(c2, l2, 2, np.array([0.5, 1.0]))
    assert (o["pairs"][0] == 0).all() and np.isnan(o["occ"][0]).all() and np.isfinite(o["occ"][1]).any()
    # interaction_matrix
    m = nh.interaction_matrix(labels, nbr, w, K, normalized=True)
    assert np.isnan(m[3]).all() and np.allclose(np.nansum(m, axis=1)[[0, 1, 2, 4, 5]], 1.0)


def test_default_radii():
    c = np.array([[0.0, 0.0], [6.0, 8.0], [3.0, 1.0]])
    assert np.array_equal(nhd.default_radii(c, 5), np.linspace(1.0, 5.0, 5))
    assert np.array_equal(nhd.default_radii(c, 5), nh.default_radii(c, 5))
    assert np.array_equal(nhd.default_radii(c[:1], 2), [0.5, 1.0]) and np.array_equal(nhd.default_radii(c[:0], 1), [1.0])


# ------------------------------------------------------------------------------------------------------ host rules
def test_greedy_matching():
    table = np.array([[5, 5, 0], [5, 1, 0], [0, 0, 0], [2, 9, 0]])
    want = [(3, 1), (0, 0)]                                      # 9 first; then the 5s: (0, 0) before (1, 0); (0, 1) left with its column
    assert nhd.greedy_match(table).tolist() == [list(v) for v in want]
    assert nh.greedy_match(table).tolist() == [list(v) for v in want]
    ties = np.array([[3, 3], [3, 3]])
    assert nhd.greedy_match(ties).tolist() == [[0, 0], [1, 1]] == nh.greedy_match(ties).tolist()
    assert nhd.greedy_match(np.zeros((2, 3), dtype=np.int64)).shape == (0, 2)
    rng = np.random.default_rng(1)
    for _ in range(20):
        t = rng.integers(0, 4, (rng.integers(1, 6), rng.integers(1, 6)))
        assert np.array_equal(nhd.greedy_match(t), nh.greedy_match(t))
    pred, true = np.array([0, 0, 1, 1, 2, -1, 2]), np.array([1, 1, 0, 0, -1, 2, 2])
    assert nhd.contingency(pred, true, 3, 3).tolist() == [[0, 2, 0], [2, 0, 0], [0, 0, 1]]


def test_top_pairs():
    z = np.array([[1.0, -5.0, np.nan], [5.0, 0.5, 2.0], [np.inf, 0.0, -2.0]])
    assert nhd.top_pairs([{"zscore": z}], 0, 4).tolist() == [[0, 1], [1, 0], [1, 2], [2, 2]]
    assert nhd.top_pairs([{"zscore": np.full((2, 2), np.nan)}], 0, 3).shape == (0, 2)


def test_argument_and_limit_errors_come_before_any_device_call(golden):
    coords, labels, nbr, w, perms, K = case(golden, "two")
    n = labels.size
    graph = {"nbr": nbr, "w": w, "offsets": np.array([0, n])}

    def bad(match, fn=nhd.nhood_enrichment, **kw):
        args = dict(labels=labels, graph=graph)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            fn(**args)

    bad("spatial.lattice returns", graph={"nbr": nbr})
    bad("both be", graph={"nbr": nbr, "w": w[:, :2], "offsets": [0, n]})
    bad("neighbour slots", graph={"nbr": np.zeros((n, 65), np.int32), "w": np.ones((n, 65)), "offsets": [0, n]})
    bad("integers", graph={"nbr": nbr.astype(np.float64), "w": w, "offsets": [0, n]})
    bad("offsets", graph={"nbr": nbr, "w": w, "offsets": [0, n - 1]})
    bad("every slide needs", graph={"nbr": nbr, "w": w, "offsets": [0, 1, n]})
    bad("integer group ids", labels=labels.astype(np.float64))
    bad("integer group ids", labels=labels[:-1])
    bad("slide 0 holds 1 group ids outside", labels=np.where(np.arange(n) == 3, 2, labels), k=2)
    bad("slide 0 holds 1 group ids outside", labels=np.where(np.arange(n) == 3, -2, labels))
    two = {"nbr": np.concatenate([nbr, nbr]), "w": np.concatenate([w, w]), "offsets": [0, n, 2 * n]}
    bad("slide 1 holds 2 group ids outside", graph=two, labels=np.concatenate([labels, np.where(np.arange(n) < 2, 7, labels)]),
        k=[2, 2])
    bad("groups", k=256)
    bad("groups", k=0)
    bad("n_perms", n_perms=-1)
    bad("n_perms", n_perms=nhd.MAX_PERMS + 1)
    bad("n_perms", n_perms=2.5)
    bad("seed", seed=-1)
    bad("permutations", permutations=[np.zeros((2, 5), dtype=np.int64)])
    bad("not a permutation", permutations=[np.zeros((2, int((labels >= 0).sum())), dtype=np.int64)])
    bad("normalized", fn=nhd.interaction_matrix, normalized=1)
    big = 16385
    with pytest.raises(ValueError, match="every slide needs"):
        nhd.nhood_enrichment(np.zeros(big, np.int64), {"nbr": np.zeros((big, 1), np.int32), "w": np.ones((big, 1)),
                                                       "offsets": [0, big]})
    with pytest.raises(ValueError, match="at most"):
        nhd.check_cells(40000, 255, 1, "nhood")                  # 40000 x 255^2 > 2^31
    with pytest.raises(ValueError, match="at most"):
        nhd.check_cells(600, 255, 64, "co_occurrence")
    nhd.check_cells(33025, 255, 1, "nhood")                      # 33025 x 65025 = 2^31 - 1 - 22: inside

    def bad_c(match, **kw):
        args = dict(coords=coords, labels=labels, radii=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            nhd.co_occurrence(**args)

    bad_c(r"\(rows, 2\)", coords=coords[:, :1])
    bad_c("integer group ids", labels=labels[:-1])
    bad_c("slide 0 holds non-finite", coords=np.where(np.arange(n)[:, None] == 2, np.nan, coords))
    bad_c("slide 1 holds non-finite", coords=np.concatenate([coords, np.where(np.arange(n)[:, None] == 2, np.inf, coords)]),
          labels=np.concatenate([labels, labels]), offsets=[0, n, 2 * n])
    bad_c("radii", radii=0)
    bad_c("radii", radii=65)
    bad_c("radii", radii=np.linspace(1, 2, 65))
    bad_c("finite, positive and increasing", radii=[1.0, 1.0])
    bad_c("finite, positive and increasing", radii=[0.0, 1.0])
    bad_c("finite, positive and increasing", radii=[1.0, np.nan])
    bad_c("radii", radii="a")
    bad_c("radii", radii=[[1.0, 2.0]])
    bad_c("offsets", offsets=[0, 3])
    with pytest.raises(ValueError, match="one label vector per slide"):
        nhd.arrangement_slides([labels, labels], [coords])
    with pytest.raises(ValueError, match="do not match"):
        nhd.arrangement_slides([labels[:-1]], [coords])
    with pytest.raises(ValueError, match="predicted and"):
        nhd.arrangement_recovery([labels], [labels[:-1]], [coords])
    with pytest.raises(ValueError, match="n_perms must be"):
        nhd.arrangement_recovery([labels], [labels], [coords], n_perms=0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present")
def test_no_cpu_fallback(golden):
    coords, labels, nbr, w, perms, K = case(golden, "two")
    with pytest.raises(RuntimeError, match="no GPU available"):
        nhd.nhood_enrichment(labels, {"nbr": nbr, "w": w, "offsets": [0, labels.size]}, n_perms=4)
    with pytest.raises(RuntimeError, match="no GPU available"):
        nhd.co_occurrence(coords, labels, radii=4)
    with pytest.raises(RuntimeError, match="no GPU available"):
        nhd.arrangement_slides([labels], [coords])


def test_cli_parser(capsys):
    a = nhd.parse_args(["--labels", "a.npy", "b.npy", "--coords", "c.npy", "d.npy"])
    assert (a.k, a.prune, a.n_perms, a.radii, a.seed, a.top, a.out_dir, a.true_labels) == (8, "NA", 1000, 50, 0, 10, None, None)
    a = nhd.parse_args(["--labels", "a.npy", "--coords", "c.npy", "--true_labels", "t.npy", "--k", "6", "--prune", "STD",
                        "--n_perms", "64", "--radii", "12", "--seed", "3", "--top", "2", "--out_dir", "o"])
    assert (a.k, a.prune, a.n_perms, a.radii, a.seed, a.top, a.out_dir, a.true_labels) == (6, "STD", 64, 12, 3, 2, "o", ["t.npy"])
    for argv in (["--labels", "a.npy", "--coords", "c.npy", "d.npy"], ["--labels", "a.npy", "--coords", "c.npy", "--k", "0"],
                 ["--labels", "a.npy", "--coords", "c.npy", "--true_labels", "t.npy", "u.npy"],
                 ["--labels", "a.npy", "--coords", "c.npy", "--n_perms", "0"], ["--labels", "a.npy", "--coords", "c.npy", "--radii", "65"],
                 ["--labels", "a.npy", "--coords", "c.npy", "--prune", "x"], ["--labels", "a.npy", "--coords", "c.npy", "--top", "0"],
                 ["--labels", "a.npy", "--coords", "c.npy", "--seed", "-1"], ["--coords", "c.npy"]):
        with pytest.raises(SystemExit):
            nhd.parse_args(argv)
    capsys.readouterr()


def test_tile_rows_and_staging_rules_on_both_sides_of_every_boundary():
    """The library's host-callable rules against the restated ones: a full sweep over K at the slide sizes the GPU tests
    use, and every n at which the rule changes for K = 61 .. 70 and 255 (the LDS left shrinks by 32 bytes per 16 rows)."""
    from mclstexp_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert nh.budget(2) == 155648 - 32 and nh.budget(16384) == 155648 - 32768
    assert [nh.tile_rows(n, 255) for n in (2, 600, 16384)] == [19, 18, 15]
    assert (nh.tile_rows(600, 69), nh.tile_rows(600, 70)) == (69, 68) and (nh.tile_rows(16384, 61), nh.tile_rows(16384, 62)) == (61, 61)
    for n in (2, 37, 600, 4097, 16383, 16384):
        for K in range(1, 256):
            assert lib.mcl_nhood_tile_rows(n, K) == nh.tile_rows(n, K), (n, K)
    for K in list(range(61, 71)) + [255]:
        rows = np.array([nh.tile_rows(n, K) for n in range(2, 16385)])
        for i in np.flatnonzero(np.diff(rows)):
            n = 2 + int(i)
            assert lib.mcl_nhood_tile_rows(n, K) == rows[i] != rows[i + 1] == lib.mcl_nhood_tile_rows(n + 1, K), (n, K)
    for K, kw in ((3, 8), (8, 8), (8, 64), (69, 8), (70, 3), (255, 8), (1, 1)):
        st = np.array([nh.staged(n, K, kw) for n in range(2, 16385)])
        for n in [2, 16384] + [2 + int(i) + d for i in np.flatnonzero(np.diff(st)) for d in (0, 1)]:
            assert lib.mcl_nhood_staged(n, K, kw) == int(st[n - 2]), (n, K, kw)
    assert nh.staged(8532, 8, 8) and not nh.staged(8533, 8, 8) and nh.staged(1181, 8, 64) and not nh.staged(1182, 8, 64) and not nh.staged(16384, 3, 8) and not nh.staged(600, 255, 8)
    for args in ((1, 4), (16385, 4), (10, 0), (10, 256)):
        assert lib.mcl_nhood_tile_rows(*args) == -1
    for args in ((10, 4, 0), (10, 4, 65), (1, 4, 8)):
        assert lib.mcl_nhood_staged(*args) == -1
    assert lib.mcl_nhood_workspace_bytes(100, 8) == 1608 and lib.mcl_nhood_workspace_bytes(100, 65) == -1
    assert lib.mcl_cooccur_workspace_bytes(100) == 1608 and lib.mcl_cooccur_workspace_bytes(1) == -1
    # argument checks come before any launch
    assert lib.mcl_nhood_counts(*([None] * 5), 1, 10, 10, 2, None, None, 8, None, 0, None, None, None, None, None) == -1
    assert lib.mcl_cooccur_counts(*([None] * 5), 1, 10, 10, 2, None, 4, None, None, None, None) == -1
    assert lib.mcl_cooccur_scores(None, 1, 2, 4, None, None, None) == -1
