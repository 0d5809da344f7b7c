"""GPU: mclstexp_amd.nhood against the numpy restatement tests/nhood_reference.py.

Every quantity the device computes is an integer count, and z and occ are stated roundings of exact integers, so every
comparison of a device result is ``array_equal`` (NaN equal to NaN) and no case is left out of any comparison.  Only the
recovery scores, Pearson correlations formed on the host by two different formulas, are compared to 1e-12.  The lattices
come from ``spatial.lattice`` (pinned by its own tests); the restatement is given the same neighbour list.  P = 64 unless
said otherwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ligrec_reference as lr
import nhood_reference as nh
import spatial_reference as sr
from conftest import ROOT
from mclstexp_amd import nhood as nhd
from mclstexp_amd import spatial as sp

pytestmark = pytest.mark.gpu
P, SEED = 64, 5
NH_KEYS = ("count", "perm_sum", "perm_sumsq", "n_ge", "n_le", "zscore", "perm_mean", "perm_std", "pval_enriched",
           "pval_depleted", "sizes")
# n -> (K, empty group, group of one spot): the slides of the batch
BATCH = {2: (2, None, None), 37: (3, None, None), 143: (7, 3, 6), 257: (5, None, None), 1025: (6, None, None)}


def same(got, want, keys, what):
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, key)
    assert got["n"] == want["n"] and got["k"] == want["k"], what


def batch_labels(n, seed=0):
    K, empty, single = BATCH[n]
    if n == 2:
        return np.array([0, 1], dtype=np.int64)
    return lr.make_labels(n, K, np.random.default_rng(seed + n), empty=empty, single=single)


def jittered(n, seed):
    side = int(np.ceil(np.sqrt(n)))
    return sr.make_coords(side, side, seed)[:n]


def given_list(n, kw, seed):
    """A directed list with pruned slots: neighbours i + 1, i + 3, ... (mod n), a tenth of the slots pruned."""
    rng = np.random.default_rng(seed)
    nbr = ((np.arange(n)[:, None] + 1 + 2 * np.arange(kw)[None, :]) % n).astype(np.int32)
    return nbr, np.where(rng.random((n, kw)) < 0.1, 0.0, 1.0)


def stack(parts):
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts), off


def host_graph(graph):
    return graph["nbr"].cpu().numpy(), graph["w"].cpu().numpy()


# -------------------------------------------------------------------------------------------------- neighbourhoods
@pytest.fixture(scope="module")
def lattice_batch():
    sizes = [37, 143, 257, 1025]
    coords, off = stack([jittered(n, n) for n in sizes])
    labels = np.concatenate([batch_labels(n) for n in sizes])
    ks = [BATCH[n][0] for n in sizes]
    return sizes, coords, off, labels, ks


@pytest.mark.parametrize("prune,on_device", [("NA", False), ("STD", True)])
def test_lattice_batch_in_one_call(lattice_batch, prune, on_device):
    sizes, coords, off, labels, ks = lattice_batch
    graph = sp.lattice(coords, off, k=8, prune=prune)
    nbr, w = host_graph(graph)
    assert (w == 0).any() == (prune == "STD")
    lab = torch.from_numpy(labels.astype(np.int32)).cuda() if on_device else labels
    res = nhd.nhood_enrichment(lab, graph, ks, n_perms=P, seed=SEED)
    for s, n in enumerate(sizes):
        sl = slice(off[s], off[s + 1])
        want = nh.nhood(labels[sl], nbr[sl], w[sl], ks[s], n_perms=P, seed=SEED)
        same(res[s], want, NH_KEYS, (prune, n))
        assert res[s]["n_perms"] == P
    r = res[1]                                                    # n = 143: an empty group, a group of one spot, 10 % dropped
    assert r["sizes"][3] == 0 and r["sizes"][6] == 1 and r["n"] < 143 and np.isnan(r["zscore"][3]).all()
    # determinism: run to run, and a slide alone against the same slide in the batch
    again = nhd.nhood_enrichment(lab, graph, ks, n_perms=P, seed=SEED)
    for a, b in zip(res, again):
        same(a, b, NH_KEYS, "run to run")
    sl = slice(off[3], off[4])
    alone = nhd.nhood_enrichment(labels[sl], {"nbr": nbr[sl], "w": w[sl], "offsets": [0, sizes[3]]}, ks[3], n_perms=P, seed=SEED)
    same(alone[0], res[3], NH_KEYS, "alone")
    # the interaction matrix is the count; k inferred from host labels
    if not on_device:
        got = nhd.interaction_matrix(labels, graph)
        norm = nhd.interaction_matrix(labels, graph, normalized=True)
        for s in range(len(sizes)):
            sl = slice(off[s], off[s + 1])
            K = int(labels[sl].max()) + 1
            assert np.array_equal(got[s], nh.interaction_matrix(labels[sl], nbr[sl], w[sl], K))
            assert np.array_equal(norm[s], nh.interaction_matrix(labels[sl], nbr[sl], w[sl], K, True), equal_nan=True)


def test_given_list_batch_with_three_slots():
    sizes = [2, 37, 143, 257, 1025]
    lists = [given_list(n, 3, n) for n in sizes]
    nbr, off = stack([g[0] for g in lists])
    w = np.concatenate([g[1] for g in lists])
    w[:2] = [[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]
    labels = np.concatenate([batch_labels(n, 1) for n in sizes])
    ks = [BATCH[n][0] for n in sizes]
    res = nhd.nhood_enrichment(labels, {"nbr": nbr, "w": w, "offsets": off}, ks, n_perms=P, seed=SEED)
    for s, n in enumerate(sizes):
        sl = slice(off[s], off[s + 1])
        same(res[s], nh.nhood(labels[sl], nbr[sl], w[sl], ks[s], n_perms=P, seed=SEED), NH_KEYS, n)
    assert not np.array_equal(res[2]["count"], res[2]["count"].T)            # slots are directed
    none = nhd.nhood_enrichment(labels, {"nbr": nbr, "w": w, "offsets": off}, ks, n_perms=0)
    assert sorted(none[0]) == ["count", "k", "n", "n_perms", "sizes"]
    for a, b in zip(none, res):
        assert np.array_equal(a["count"], b["count"])


def test_255_groups_take_more_than_one_source_tile():
    n, K = 601, 255
    assert nh.tile_rows(n, K) < K
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, K, n)
    labels[labels == 17] = 18                                     # an empty group among them
    graph = sp.lattice(jittered(n, 4), k=8, prune="STD")
    nbr, w = host_graph(graph)
    res = nhd.nhood_enrichment(labels, graph, K, n_perms=P, seed=SEED)
    same(res[0], nh.nhood(labels, nbr, w, K, n_perms=P, seed=SEED), NH_KEYS, "K = 255")
    assert res[0]["sizes"][17] == 0 and res[0]["count"].sum() > 3000


def test_both_sides_of_every_tile_and_staging_boundary_in_one_call():
    """(n, K) with the ring list of 64 slots: one tile / two tiles (K = 69 / 70), the list staged in LDS / read through L2
    (n = 1181 / 1182 at K = 8), and two tiles with a staged list (n = 8, K = 70)."""
    cases = [(300, 69), (300, 70), (1181, 8), (1182, 8), (8, 70)]
    assert [nh.tile_rows(n, K) == K for n, K in cases] == [True, False, True, True, False]
    assert [nh.staged(n, K, 64) for n, K in cases] == [False, False, True, False, True]
    rng = np.random.default_rng(9)
    labels = [rng.integers(-1, K, n) for n, K in cases]
    lists = [nh.ring_list(n, 64) for n, _ in cases]
    nbr, off = stack([g[0] for g in lists])
    w = np.concatenate([g[1] for g in lists])
    w[rng.random(w.shape) < 0.05] = 0.0
    ks = [K for _, K in cases]
    res = nhd.nhood_enrichment(np.concatenate(labels), {"nbr": nbr, "w": w, "offsets": off}, ks, n_perms=P, seed=SEED)
    for s, (n, K) in enumerate(cases):
        sl = slice(off[s], off[s + 1])
        same(res[s], nh.nhood(labels[s], nbr[sl], w[sl], K, n_perms=P, seed=SEED), NH_KEYS, (n, K))


def test_largest_slide_fills_the_int64_accumulators():
    n = 16384
    nbr, w = nh.ring_list(n, 64)
    res = nhd.nhood_enrichment(np.zeros(n, dtype=np.int64), {"nbr": nbr, "w": w, "offsets": [0, n]}, 1, n_perms=4, seed=SEED)[0]
    assert res["count"][0, 0] == 1 << 20 and res["perm_sum"][0, 0] == 4 << 20 and res["perm_sumsq"][0, 0] == 4 << 40
    assert res["n_ge"][0, 0] == 4 and res["n_le"][0, 0] == 4 and np.isnan(res["zscore"][0, 0])
    assert res["perm_mean"][0, 0] == float(1 << 20) and res["perm_std"][0, 0] == 0.0


def test_largest_slide_three_groups_on_the_lattice():
    n = 16384
    yy, xx = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    coords = np.stack([xx.ravel(), yy.ravel()], axis=1) + np.random.default_rng(2).uniform(-0.1, 0.1, (n, 2))
    labels = (xx.ravel() * 3 // 128).astype(np.int64)
    labels[np.random.default_rng(3).random(n) < 0.05] = -1
    graph = sp.lattice(coords, k=8)
    nbr, w = host_graph(graph)
    res = nhd.nhood_enrichment(labels, graph, 3, n_perms=4, seed=SEED)
    same(res[0], nh.nhood(labels, nbr, w, 3, n_perms=4, seed=SEED), NH_KEYS, "n = 16384")


def test_identity_replay():
    sizes = [37, 143]
    lists = [given_list(n, 3, n) for n in sizes]
    nbr, off = stack([g[0] for g in lists])
    w = np.concatenate([g[1] for g in lists])
    labels = np.concatenate([batch_labels(n) for n in sizes])
    ks = [BATCH[n][0] for n in sizes]
    kept = [int((labels[off[s]:off[s + 1]] >= 0).sum()) for s in range(2)]
    graph = {"nbr": nbr, "w": w, "offsets": off}
    ident = [np.tile(np.arange(m), (5, 1)) for m in kept]
    res = nhd.nhood_enrichment(labels, graph, ks, permutations=ident)
    for r in res:
        assert r["n_perms"] == 5 and (r["n_ge"] == 5).all() and (r["n_le"] == 5).all()
        assert np.array_equal(r["perm_sum"], 5 * r["count"]) and np.array_equal(r["perm_sumsq"], 5 * r["count"] ** 2)
        assert np.isnan(r["zscore"]).all()
    tables = [sr.permutations(SEED, 7, m) for m in kept]                       # the generated tables, replayed
    a = nhd.nhood_enrichment(labels, graph, ks, permutations=tables)
    b = nhd.nhood_enrichment(labels, graph, ks, n_perms=7, seed=SEED)
    for x, y in zip(a, b):
        same(x, y, NH_KEYS, "replay")


# ---------------------------------------------------------------------------------------------------- co-occurrence
CC_KEYS = ("pairs", "occ", "radii", "sizes")


def cc_labels(n, K, seed, drop=0.1):
    rng = np.random.default_rng(seed)
    lab = np.sort(rng.integers(0, K, n))                          # spatially coherent along the raster, then some noise
    swap = rng.random(n) < 0.2
    lab[swap] = rng.integers(0, K, int(swap.sum()))
    if n > 10:
        lab[rng.random(n) < drop] = -1
    return lab.astype(np.int64)


@pytest.fixture(scope="module")
def cc_jittered():
    spec = [(2, 2), (37, 3), (257, 255), (1025, 7), (4097, 5)]
    coords = [jittered(n, 10 + n) for n, _ in spec]
    coords[3][7] = coords[3][6]                                   # coincident spots
    coords[3][300] = coords[3][6]
    labels = [cc_labels(n, K, n) for n, K in spec]
    labels[3][[6, 7, 300]] = [0, 0, 4]
    want = [nh.co_occurrence(c, lab, K, 50) for c, lab, (_, K) in zip(coords, labels, spec)]
    return spec, coords, labels, want


def test_cooccurrence_jittered_batch_with_default_radii(cc_jittered):
    spec, coords, labels, want = cc_jittered
    c, off = stack(coords)
    lab, ks = np.concatenate(labels), [K for _, K in spec]
    res = nhd.co_occurrence(c, lab, off, ks, radii=50)
    for s, (n, K) in enumerate(spec):
        same(res[s], want[s], CC_KEYS, (n, K))
        assert res[s]["pairs"].shape == (50, K, K)
    assert res[3]["pairs"][0][0, 0] >= 2 and res[3]["pairs"][0][0, 4] >= 2 and res[3]["pairs"][0][4, 0] >= 2   # d = 0 counts
    assert res[4]["n"] > 256 * 14 and np.isfinite(res[4]["occ"][-1]).all()
    # labels and fp32 coordinates given from the device; run to run; a slide alone against the batch
    lab_d = torch.from_numpy(lab.astype(np.int32)).cuda()
    again = nhd.co_occurrence(torch.from_numpy(c).cuda(), lab_d, off, ks, radii=50)
    for a, b in zip(res, again):
        same(a, b, CC_KEYS, "device inputs")
    alone = nhd.co_occurrence(coords[3], labels[3], None, 7, radii=50)
    same(alone[0], res[3], CC_KEYS, "alone")
    c32 = c.astype(np.float32)
    r32 = nhd.co_occurrence(torch.from_numpy(c32).cuda(), lab_d, off, ks, radii=50)
    same(r32[1], nh.co_occurrence(c32[off[1]:off[2]], labels[1], 3, 50), CC_KEYS, "fp32")


@pytest.mark.parametrize("T", [1, 64])
def test_cooccurrence_integer_grid_with_given_radii(T):
    """Integer coordinates and radii whose squares are hit exactly by many pairs (1, 2, 5: the 3-4-5 triangle)."""
    spec = [(2, 2), (37, 3), (257, 255), (1025, 7)]
    coords = [sr.make_coords(int(np.ceil(np.sqrt(n))), int(np.ceil(np.sqrt(n))), n, integer=True)[:n] for n, _ in spec]
    labels = [cc_labels(n, K, n + 1) for n, K in spec]
    radii = np.array([5.0]) if T == 1 else np.concatenate([[1.0, np.sqrt(2.0), 2.0, np.sqrt(5.0), 5.0], 5.5 + 0.5 * np.arange(59)])
    c, off = stack(coords)
    assert c.dtype == np.int64
    res = nhd.co_occurrence(c, np.concatenate(labels), off, [K for _, K in spec], radii=radii)
    for s, (n, K) in enumerate(spec):
        same(res[s], nh.co_occurrence(coords[s], labels[s], K, radii), CC_KEYS, (T, n, K))
    assert res[3]["pairs"].shape == (T, 7, 7) and np.array_equal(res[3]["radii"], radii)
    low = nhd.co_occurrence(c, np.concatenate(labels), off, [K for _, K in spec], radii=[0.5, 1.0])
    for r in low:                                                 # a radius below every distance: nothing defined there
        assert (r["pairs"][0] == 0).all() and np.isnan(r["occ"][0]).all()


def test_cooccurrence_full_grid_against_the_closed_form():
    """128 x 128 integer grid, one group: pairs[t] = sum over (dx, dy) != 0 with dx^2 + dy^2 <= r^2 of (128 - |dx|)(128 - |dy|)."""
    yy, xx = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    coords = np.stack([xx.ravel(), yy.ravel()], axis=1)
    radii = [1.0, 2.0, 5.0, 13.0]
    res = nhd.co_occurrence(coords, np.zeros(16384, dtype=np.int64), None, 1, radii=radii)[0]
    assert res["pairs"][:, 0, 0].tolist() == [nh.grid_pairs(128, r) for r in radii]
    assert np.array_equal(res["occ"], np.ones((4, 1, 1)))


# ----------------------------------------------------------------------------------------------------------- errors
def test_errors_name_the_slide():
    sizes = [37, 143]
    lists = [given_list(n, 3, n) for n in sizes]
    nbr, off = stack([g[0] for g in lists])
    w = np.concatenate([g[1] for g in lists])
    labels = np.concatenate([batch_labels(n) for n in sizes])
    ks = [BATCH[n][0] for n in sizes]
    graph = {"nbr": nbr, "w": w, "offsets": off}
    bad = labels.copy()
    bad[40] = 7
    with pytest.raises(ValueError, match="slide 1 holds 1 group ids outside"):
        nhd.nhood_enrichment(bad, graph, ks, n_perms=4)
    with pytest.raises(ValueError, match="labels: slide 1 holds 1 group ids outside"):
        nhd.nhood_enrichment(torch.from_numpy(bad.astype(np.int32)).cuda(), graph, ks, n_perms=4)
    far = nbr.copy()
    i, c = np.argwhere(w[37:] != 0)[0]
    far[37 + i, c] = 143
    with pytest.raises(ValueError, match="graph: slide 1 holds 1 kept neighbour indices outside the slide"):
        nhd.nhood_enrichment(labels, {"nbr": far, "w": w, "offsets": off}, ks, n_perms=4)
    coords, _ = stack([jittered(n, n) for n in sizes])
    nan = coords.copy()
    keep = np.flatnonzero(labels[37:] >= 0)[0]
    nan[37 + keep, 1] = np.nan
    with pytest.raises(ValueError, match="slide 1 holds non-finite"):
        nhd.co_occurrence(nan, labels, off, ks, radii=4)
    with pytest.raises(ValueError, match="coords: slide 1 holds 1 non-finite"):
        nhd.co_occurrence(torch.from_numpy(nan).cuda(), labels, off, ks, radii=[0.5, 1.0])
    with pytest.raises(ValueError, match="labels: slide 1 holds 1 group ids outside"):
        nhd.co_occurrence(coords, torch.from_numpy(bad.astype(np.int32)).cuda(), off, ks, radii=[0.5, 1.0])
    for radii in ([1.0, 0.5], [-1.0, 1.0], [1.0, np.inf], 0, 65):
        with pytest.raises(ValueError, match="radii"):
            nhd.co_occurrence(coords, labels, off, ks, radii=radii)


# -------------------------------------------------------------------------------------------------------- recovery
def test_planted_arrangement():
    """The 20 x 17 integer grid in four vertical stripes, k = 8, P = 64, seed 0, 50 radii.  The restatement gives

        z = [[ 36.997 -13.545 -16.095 -18.874]
             [-11.879  29.349 -10.314 -17.200]
             [-15.673  -9.815  29.766  -9.642]
             [-18.139 -16.429  -9.359  30.182]]

    (no NaN cell, so the finite-cell mask leaves nothing out), recovery against itself Pearson z 1.0, sign agreement 1.0,
    Pearson log2 occ 1.0, and against the same labels shuffled over the spots (``default_rng(0).permutation``) Pearson z
    -0.4688, sign agreement 0.25, Pearson log2 occ -0.3141 over 16 cells: whatever the restatement gives, not a target."""
    coords, labels = nh.make_stripes()
    shuffled = labels[np.random.default_rng(0).permutation(labels.size)]
    res = nhd.arrangement_slides([labels], [coords], k_graph=8, prune="NA", n_perms=P, seed=0, radii=50)[0]
    g = sr.lattice(coords, 8, "NA")

    def restated(lab):
        r = nh.nhood(lab, g["nbr"], g["w"], 4, n_perms=P, seed=0)
        r.update(nh.co_occurrence(coords, lab, 4, 50))
        return r

    rt, rs = restated(labels), restated(shuffled)
    same(res, rt, NH_KEYS + CC_KEYS, "stripes")
    z = res["zscore"]
    assert np.isfinite(z).all() and np.isfinite(rs["zscore"]).all()
    assert (np.diag(z) > 0).all() and all(z[a, b] < 0 for a in range(4) for b in range(4) if abs(a - b) >= 2)
    assert res["categories"].tolist() == [0, 1, 2, 3]
    own = nhd.arrangement_recovery([labels], [labels], [coords], n_perms=P, seed=0)
    assert own["matching"][0].tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]] and own["n_cells"][0] == 16
    assert abs(own["pearson_z"][0] - 1.0) < 1e-12 and own["sign_agreement"][0] == 1.0 and abs(own["pearson_occ"][0] - 1.0) < 1e-12
    rec = nhd.arrangement_recovery([shuffled], [labels], [coords], n_perms=P, seed=0)
    same(rec["pred"][0], rs, NH_KEYS + CC_KEYS, "shuffled")
    match, pz, sign, pocc, left_out = nh.recovery(shuffled, labels, rs, rt)
    assert left_out == 0 and rec["n_cells"][0] == 16 and np.array_equal(rec["matching"][0], match)
    print(f"shuffled: Pearson z {rec['pearson_z'][0]:.4f}, sign agreement {rec['sign_agreement'][0]:.4f}, Pearson log2 occ "
          f"{rec['pearson_occ'][0]:.4f}")
    assert abs(rec["pearson_z"][0] - pz) < 1e-12 and rec["sign_agreement"][0] == sign and abs(rec["pearson_occ"][0] - pocc) < 1e-12
    assert np.abs(rs["zscore"]).max() < 5 < np.abs(z).min()
    assert nhd.top_pairs([res], 0, 1).tolist() == [[0, 0]]
    # string annotations: "undetermined" is dropped
    names = np.array(["a", "b", "c", "d"])[labels].astype(object)
    names[:5] = "undetermined"
    dropped = labels.copy()
    dropped[:5] = -1
    named = nhd.arrangement_slides([names], [coords], n_perms=8, seed=0, radii=4)[0]
    want = nh.nhood(dropped, g["nbr"], g["w"], 4, n_perms=8, seed=0)
    want.update(nh.co_occurrence(coords, dropped, 4, 4))
    same(named, want, NH_KEYS + CC_KEYS, "annotations")
    assert named["categories"].tolist() == ["a", "b", "c", "d"] and named["n"] == labels.size - 5


def test_cli(tmp_path):
    coords, labels = nh.make_stripes()
    shuffled = labels[np.random.default_rng(0).permutation(labels.size)]
    np.save(tmp_path / "c.npy", coords)
    np.save(tmp_path / "l.npy", shuffled)
    np.save(tmp_path / "t.npy", labels)
    cmd = [sys.executable, "-m", "mclstexp_amd.nhood", "--labels", str(tmp_path / "l.npy"), "--coords", str(tmp_path / "c.npy"),
           "--true_labels", str(tmp_path / "t.npy"), "--n_perms", "16", "--radii", "8", "--top", "2", "--out_dir", str(tmp_path / "o")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "most enriched" in out.stdout and "most depleted" in out.stdout and "recovery: mean Pearson z" in out.stdout
    saved = np.load(tmp_path / "o" / "0" / nhd.OUT_FILE)
    g = sr.lattice(coords, 8, "NA")
    want = nh.nhood(shuffled, g["nbr"], g["w"], 4, n_perms=16, seed=0)
    assert np.array_equal(saved["count"], want["count"]) and np.array_equal(saved["zscore"], want["zscore"], equal_nan=True)
    assert saved["pairs"].shape == (8, 4, 4)
