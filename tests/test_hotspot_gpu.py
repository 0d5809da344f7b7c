"""GPU: mclstexp_amd.hotspot (csrc/hotspot.hip) against the numpy restatement tests/hotspot_reference.py, which
tests/test_hotspot_host.py pins to dense W-matrix formulas and to scipy.

Integer outputs are EQUAL to the restatement: draw tables, deg, count_ge, count_le, quadrant, cluster.  mean and den are
bit-equal to spatial.autocorr's.  Floating outputs lie within bounds derived to first order from the stated summation
orders (``hotspot_reference.bounds`` states every one; eps = 2^-52; not tuned): a value travels through at most
Lr = ceil(n / 256) + 8 additions of the fixed row order, d of the slot order or of a draw, P of the sums over the draws, and
device and restatement both carry that rounding.

Measured on MI355X, the largest error / bound over the cases of each test (every test prints its rows with -s).  mean, den,
lag, local_i, gi_z, sum_sim, sumsq_sim, pval_sim, mean_sim, var_sim and z_sim came out bit-equal to the restatement in every
case (ratio 0): the restatement follows the kernel's orders, and +, -, *, /, sqrt are correctly rounded on both sides.  What
differs is erfc, erfcx and log of the two libraries:

  test                              gi_pval_norm  gi_neglog10_pval_norm
  statistics, n = 2 ... 4097        0.0092        0.0083
  one column per workgroup, 16384   0.0016        0.0018

The behavioural cases (recorded in tests/golden/hotspot.npz by the restatement alone, alpha = 0.05, 199 draws, seed 0): the
planted 6 x 6 block has 16 interior spots, all labelled HH, and 6 of the 304 spots outside the block labelled HH; the
spot-shuffled "mid" slide (shuffle seed 1) has mean Pearson r of gi_z 0.097409 and mean HH Jaccard 0.027590."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hotspot_reference as hr
import spatial_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("quadrant", "cluster", "count_ge", "count_le")
PAIRED = {"sum_sim": "sum1", "sumsq_sim": "sum2"}
SHUFFLE_SEED = 1


def within(got, want, bound, what):
    """NaN exactly where the restatement has NaN, |got - want| <= bound elsewhere; returns the largest error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    ok = ~np.isnan(want)
    with np.errstate(all="ignore"):
        err = np.where(ok & ~(np.isinf(want) & (got == want)), np.abs(got - want), 0.0)
        ratio = np.where(err == 0, 0.0, err / bound)
    assert not (ratio[ok] > 1.0).any(), (what, float(np.nanmax(ratio[ok])))
    return float(ratio[ok].max()) if ok.any() else 0.0


def coords_of(n, kind, seed=0):
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil(np.sqrt(n * 1.3)))
    if kind == "integer":
        c = sr.make_coords(side, side, seed, integer=True).astype(np.float64)
    else:
        c = sr.make_coords(side, side, seed)
    c = c[rng.permutation(c.shape[0])[:n]]
    if kind == "holes":                           # spread some spots out: Grid pruning leaves isolated spots
        c = c * np.where(rng.random((n, 1)) < 0.3, 3.0, 1.0)
    return c


def graph_of(c, off, k, prune, std):
    from mclstexp_amd import spatial
    g = spatial.lattice(c, off, k, prune, std)
    return g, g["nbr"].cpu().numpy(), g["w"].cpu().numpy()


def compare(got, ref, x, nbr, w, what):
    """One slide of local_stats against the restatement; returns {output: largest error / bound}."""
    b = hr.bounds(x, nbr, w, ref)
    assert np.array_equal(got["deg"], ref["deg"]), (what, "deg")
    keys = ["quadrant"] + (list(INTS[1:]) if ref["n_perms"] else [])
    for key in keys:
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (what, key)
    worst = {}
    floats = ["lag", "local_i", "gi_z", "gi_pval_norm", "gi_neglog10_pval_norm"]
    if ref["n_perms"]:
        floats += ["sum_sim", "sumsq_sim", "pval_sim", "mean_sim", "var_sim", "z_sim"]
    for key in floats:
        rk = PAIRED.get(key, key)
        worst[key] = within(got[key], ref[rk], b[rk], (what, key))
    for key in ("mean", "den"):
        worst[key] = within(got[key], ref[key], b[key] + 1e-300, (what, key))
    return worst


# (n, k, prune, row_standardise, G, P, coordinates, values)
CASES = [
    (2, 1, "NA", True, 2, 1, "jitter", "cont"),            # the smallest slide, one draw
    (9, 8, "NA", False, 3, 7, "jitter", "cont"),           # n = k + 1: the complete graph, Gi* NaN
    (257, 8, "STD", True, 7, 7, "jitter", "special"),      # a second trip of the 256-lane row loop, unequal d_i, G = 6 + 1
    (293, 8, "Grid", False, 5, 19, "holes", "counts"),     # isolated spots (d_i = 0), binary weights, ties
    (293, 8, "NA", True, 6, 3, "integer", "scales"),       # six columns exactly
    (300, 12, "STD", True, 4, 5, "jitter", "cont"),        # k > 8: the wide draw kernel
    (1500, 4, "NA", False, 3, 2, "jitter", "cont"),        # more spots than threads
    (4097, 8, "NA", True, 5, 3, "jitter", "counts"),       # sp_columns = 4 < 6, G = 4 + 1
]


def values_of(c, G, kind, seed):
    if kind == "special":
        x = sr.make_expression(c, G, seed)
        x[:, 0] = 1.75                                       # a constant gene
        x[:, 1] = 0.0
        x[3, 1] = 3.0                                        # constant but for one spot
        return x
    return sr.make_expression(c, G, seed, kind=kind)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-k{c[1]}-{c[2]}-{'r' if c[3] else 'b'}-G{c[4]}-P{c[5]}")
def test_statistics_match_the_restatement(case):
    from mclstexp_amd import hotspot, spatial
    n, k, prune, std, G, P, ckind, vkind = case
    c = coords_of(n, ckind)
    x = values_of(c, G, vkind, n + 1)
    g, nbr, w = graph_of(c, None, k, prune, std)
    got = hotspot.local_stats(x, g, n_perms=P, seed=n, alpha=0.2, return_draws=True)[0]
    ref = hr.local_stats(x, nbr, w, n_perms=P, seed=n, alpha=0.2)
    assert np.array_equal(got["draws"], ref["draws"]), "draw table"
    assert hr.check_table(ref["draws"], np.minimum(ref["deg"], n - 1))
    worst = compare(got, ref, x, nbr, w, case)
    print(case, {key: f"{v:.2g}" for key, v in worst.items()})
    auto = spatial.autocorr(x, g)[0]
    assert np.array_equal(got["mean"], auto["mean"]) and np.array_equal(got["den"], auto["den"])
    assert hotspot.local_stats_device(x, g)["n_perms"] == 0           # no draws: the observed statistics alone
    if vkind == "special":
        for key in hr.FLOATS:
            assert np.isnan(got[key][:, 0]).all(), key
        assert (got["cluster"][:, 0] == 0).all() and (got["quadrant"][:, 0] == 0).all()
    if ckind == "holes":
        lone = got["deg"] == 0
        assert lone.any() and (got["lag"][lone] == 0).all() and (got["local_i"][lone] == 0).all()
        assert (got["pval_sim"][lone] == 1.0).all()
        assert (got["count_ge"] + got["count_le"] > P).any()          # ties are counted on both sides
    if n == k + 1:
        assert np.isnan(got["gi_z"]).all() and np.isfinite(got["local_i"]).all()
    if prune == "STD":
        assert np.unique(got["deg"]).size > 1


def test_one_column_per_workgroup_16384_spots():
    from mclstexp_amd import hotspot
    n, G, P = 16384, 4, 8
    c = sr.make_coords(128, 128, 4)
    x = sr.make_expression(c, G, 6)
    g, nbr, w = graph_of(c, None, 8, "NA", True)
    got = hotspot.local_stats(x, g, n_perms=P, seed=1, return_draws=True)[0]
    ref = hr.local_stats(x, nbr, w, n_perms=P, seed=1)
    assert np.array_equal(got["draws"], ref["draws"])
    print({key: f"{v:.2g}" for key, v in compare(got, ref, x, nbr, w, "16384").items()})


@pytest.fixture(scope="module")
def batch():
    """Three slides of unequal size in one call."""
    from mclstexp_amd import hotspot
    sizes, G, k = (143, 61, 300), 7, 6
    cs = [coords_of(n, "jitter", seed=s) for s, n in enumerate(sizes)]
    xs = [sr.make_expression(c, G, 20 + s) for s, c in enumerate(cs)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    g, nbr, w = graph_of(np.concatenate(cs), off, k, "STD", True)
    x = np.concatenate(xs)
    res = hotspot.local_stats(x, g, n_perms=7, seed=5, return_draws=True)
    return dict(cs=cs, xs=xs, off=off, g=g, nbr=nbr, w=w, x=x, res=res, k=k)


def same(a, b, what):
    for key, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[key], equal_nan=v.dtype.kind == "f"), (what, key)


def test_a_slide_in_a_batch_is_the_slide_alone_and_runs_repeat(batch):
    from mclstexp_amd import hotspot
    again = hotspot.local_stats(batch["x"], batch["g"], n_perms=7, seed=5, return_draws=True)
    for s, (c, x) in enumerate(zip(batch["cs"], batch["xs"])):
        same(batch["res"][s], again[s], ("twice", s))
        g, nbr, w = graph_of(c, None, batch["k"], "STD", True)
        alone = hotspot.local_stats(x, g, n_perms=7, seed=5, return_draws=True)[0]
        same(alone, batch["res"][s], ("alone", s))
        ref = hr.local_stats(x, nbr, w, n_perms=7, seed=5)
        assert np.array_equal(alone["draws"], ref["draws"])
        compare(alone, ref, x, nbr, w, ("batch", s))


def test_replay_gene_selection_fp32_and_strided_input(batch):
    from mclstexp_amd import hotspot
    g, x, res = batch["g"], batch["x"], batch["res"]
    replay = hotspot.local_stats(x, g, draws=[r["draws"] for r in res], seed=99)
    sel = hotspot.local_stats(torch.from_numpy(x).cuda(), g, genes=[5, 2], n_perms=7, seed=5)
    wide = torch.full((x.shape[0], x.shape[1] + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    strided = hotspot.local_stats(wide[:, :x.shape[1]], g, n_perms=7, seed=5)
    for s in range(3):
        for key in hr.FLOATS + INTS + ("lag", "sum_sim", "sumsq_sim"):
            assert np.array_equal(replay[s][key], res[s][key], equal_nan=True), ("replay", s, key)
            assert np.array_equal(strided[s][key], res[s][key], equal_nan=True), ("strided", s, key)
            assert np.array_equal(sel[s][key], res[s][key][:, [5, 2]], equal_nan=True), ("genes", s, key)
    x32 = x.astype(np.float32)
    got = hotspot.local_stats(torch.from_numpy(x32).cuda(), g, n_perms=7, seed=5)
    for s in range(3):
        a, b = int(batch["off"][s]), int(batch["off"][s + 1])
        xs = x32[a:b].astype(np.float64)
        ref = hr.local_stats(xs, batch["nbr"][a:b], batch["w"][a:b], n_perms=7, seed=5)
        compare(got[s], ref, xs, batch["nbr"][a:b], batch["w"][a:b], ("fp32", s))


def test_bivariate_pairs_and_colocalisation(batch):
    from mclstexp_amd import hotspot, ligrec
    g, x = batch["g"], batch["x"]
    pairs = np.array([[0, 3], [3, 0], [2, 2], [6, 1], [1, 6], [4, 5], [5, 5]])
    got = hotspot.local_stats(x, g, pairs=pairs, n_perms=9, seed=2)
    for s in range(3):
        a, b = int(batch["off"][s]), int(batch["off"][s + 1])
        ref = hr.local_stats(x[a:b], batch["nbr"][a:b], batch["w"][a:b], pairs, n_perms=9, seed=2)
        compare(got[s], ref, x[a:b], batch["nbr"][a:b], batch["w"][a:b], ("bivariate", s))
        assert np.isnan(got[s]["gi_z"][:, [0, 1, 3, 4, 5]]).all() and np.isfinite(got[s]["gi_z"][:, [2, 6]]).all()
    names = [f"g{j}" for j in range(x.shape[1])]
    rp = ligrec.resolve_pairs([("g0", "g3"), ("g6", "g1"), ("g9", "g1")], names)
    co = hotspot.colocalisation(x, g, rp["interactions"], n_perms=9, seed=2)
    for s in range(3):
        assert np.array_equal(co[s]["local_i"], got[s]["local_i"][:, [0, 3]])
        assert np.array_equal(co[s]["pval_sim"], got[s]["pval_sim"][:, [0, 3]])
        assert np.array_equal(co[s]["share_hh"], (got[s]["cluster"][:, [0, 3]] == 1).mean(axis=0))
    with pytest.raises(ValueError, match="complex"):
        hotspot.colocalisation(x, g, ligrec.resolve_pairs([("g0_g2", "g3")], names)["interactions"])


def test_bad_input_is_a_value_error_naming_the_slide(batch):
    from mclstexp_amd import hotspot
    g, x = batch["g"], batch["x"]
    bad = x.copy()
    bad[int(batch["off"][1]) + 2, 3] = np.inf
    with pytest.raises(ValueError, match="slide 1 holds non-finite"):
        hotspot.local_stats(bad, g, n_perms=3)
    with pytest.raises(ValueError, match="slide 0 holds pair columns"):
        hotspot.local_stats_device(x, g, pairs=torch.tensor([[0, 0], [1, 7]], dtype=torch.int32, device="cuda"), n_perms=3)
    broken = dict(g)
    off = batch["off"].copy()
    off[2] = off[3] + 5                                               # slide 1 now ends past the rows
    broken["offsets_device"] = torch.from_numpy(off).cuda()
    with pytest.raises(ValueError, match="slide 1 holds offsets"):
        hotspot.local_stats(x, broken, n_perms=3)
    draws = [r["draws"].copy() for r in batch["res"]]
    row = np.flatnonzero(batch["res"][2]["deg"] < batch["k"])[0]
    draws[2][0, row, :] = (np.arange(batch["k"]) + row + 1) % 300       # more spots than the row has kept neighbours
    with pytest.raises(ValueError, match="slide 2 holds draws"):
        hotspot.local_stats(x, g, draws=draws)


def test_planted_block_is_found():
    from mclstexp_amd import hotspot
    golden = np.load(hr.GOLDEN)
    c, x, interior, outside = hr.planted_case()
    res = hotspot.local_stats_slides([x], [c], k=8, n_perms=199, seed=0, alpha=0.05)
    hot = hotspot.hotspots(res, 0, 0)
    assert np.array_equal(np.flatnonzero(interior), golden["planted.interior"]) and np.isin(np.flatnonzero(interior), hot).all()
    assert np.isin(hot, np.flatnonzero(outside)).sum() <= int(golden["planted.outside_hh"]) + 2
    assert hotspot.hotspots(res, 0, 0, kind="cold").size == int((res[0]["cluster"][:, 0] == 3).sum())


def test_recovery_of_a_shuffled_prediction_and_cli(tmp_path):
    from mclstexp_amd import hotspot
    golden = np.load(hr.GOLDEN)
    c, x = sr.make_case("mid")
    xs = x[np.random.default_rng(SHUFFLE_SEED).permutation(x.shape[0])]
    rec = hotspot.hotspot_recovery([xs], [x], [c], n_perms=199, seed=0)
    own = hotspot.hotspot_recovery([x], [x], [c], n_perms=199, seed=0)
    assert own["mean_jaccard_hot"] == 1.0 and own["mean_agreement"] == 1.0
    assert rec["mean_jaccard_hot"] < own["mean_jaccard_hot"]
    assert rec["mean_jaccard_hot"] == pytest.approx(float(golden["shuffle.mean_jaccard_hot"]), abs=1e-12)
    # Pearson r of two 143-vectors of gi_z, each within its bound (relative 1e-13 at the most): 1e-9 is generous
    assert rec["mean_pearson"] == pytest.approx(float(golden["shuffle.mean_pearson"]), abs=1e-9)
    assert rec["n_nan"] == 0 and len(rec["pearson"]) == 1 and rec["pearson"][0].shape == (x.shape[1],)
    # the CLI in a fresh process, files gene-major
    np.save(tmp_path / "p.npy", xs.T)
    np.save(tmp_path / "t.npy", x.T)
    np.save(tmp_path / "c.npy", c)
    np.save(tmp_path / "names.npy", np.array([f"g{j}" for j in range(x.shape[1])]))
    (tmp_path / "lr.tsv").write_text("source\ttarget\ng0\tg3\ng2\tg1\n")
    out = subprocess.run([sys.executable, "-m", "mclstexp_amd.hotspot", "--pred", str(tmp_path / "p.npy"), "--coords",
                          str(tmp_path / "c.npy"), "--true", str(tmp_path / "t.npy"), "--genes", str(tmp_path / "names.npy"),
                          "--select", "g1", "g4", "--pairs", str(tmp_path / "lr.tsv"), "--n_perms", "49", "--seed", "3",
                          "--out_dir", str(tmp_path / "out")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "genes by HH spots" in out.stdout and "recovery (gi)" in out.stdout and "colocalisation" in out.stdout
    saved = np.load(tmp_path / "out" / "0" / hotspot.OUT_FILE)
    api = hotspot.local_stats_slides([xs], [c], genes=[1, 4], n_perms=49, seed=3)[0]
    for key in hr.FLOATS + INTS:
        assert np.array_equal(saved[key], api[key], equal_nan=True), key
    assert saved["coloc_local_i"].shape == (x.shape[0], 2)
