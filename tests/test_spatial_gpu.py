"""GPU: mclstexp_amd.spatial (csrc/spatial.hip) against the numpy restatement tests/spatial_reference.py, which
tests/test_spatial_host.py pins to the reference's calcADJ, to dense-matrix formulas, to scipy and to mpmath.

Bounds (derived to first order from the stated summation orders, not tuned; eps = 2^-52).  A value travels through at most
L = ceil(n / 256) + 8 additions of the fixed row order (its lane's chain, six butterfly levels, two wave levels) and k of
the slot order.  Device and restatement both carry that error, hence the leading 2:
  nbr, deg, the zero pattern of w, permutation tables, counts     exact (array_equal)
  w                                                               eps w (1 / deg is one correctly rounded division)
  S0, S1, S2                                                      2 (L + k + 4) eps S
  mean                                                            2 (L + 1) eps sum|x| / n                        =: bm
  z (not an output)                                               bm + eps max|z|                                  =: bz
  den                                                             2 ((L + 2) eps den + 2 bz sum|z|)
  num_I                                                           2 ((L + k + 3) eps sum_i |z_i| sum_t w |z_j| + bz sum w (|z_i| + |z_j|))
  num_C                                                           2 ((L + k + 4) eps num_C + 4 bz sum w |z_i - z_j|)
  I, C                                                            |I| (4 eps + bden / den) + (n / S0) b_I / den; C likewise
  sims                                                            the same bound evaluated at the permuted data
  z_norm                                                          b_I / sd + |z| (relVar / 2 + 8 eps), relVar = (bS + 8 eps) x the
                                                                  cancellation factor of the variance formula
  pval_norm                                                       p ((|z| + 1) bz_norm + (2 z^2 + 64) eps) + 1e-290  (Mills: phi / sf <= |z| + 1)
  -log10 p                                                        the relative p bound / ln 10 + 16 eps x the value
  pval_norm_adj                                                   the largest p bound of the slide (BH is monotone, 1-homogeneous)
  mean_sim                                                        max_p b_sims + 2 (P + 2) eps mean|sims|
  var_sim                                                         4 sd max_p b_sims + 2 (P + 6) eps var
  pval_z_sim                                                      as pval_norm from (b_stat + b_mean) / sd + |z| b_var / (2 var)
  pval_sim                                                        exact given the device's own sims and statistic

Measured on MI355X, largest error / bound over the cases of each test (every test prints its rows with -s).  w, S0, S1, S2,
mean, den, I, C, sims, z_norm, mean_sim and var_sim came out bit-equal to the restatement in every case (ratio 0): the
restatement follows the kernel's orders, and +, -, *, /, sqrt are correctly rounded on both sides.  What differs is erfc, erfcx
and log of the two libraries:

  test                              pval_norm  -log10 p  pval_norm_adj  pval_z_sim
  statistics, n = 2 ... 4097        0.0035     0.0029    0.00048        0.00024
  one column per workgroup, 16384   0          0         0              1.6e-07

The spot-shuffled prediction of test_recovery_and_cli: slide "mid" (143 spots), shuffle seed 1: the restatement's largest
|z_norm| of I(pred) over the 8 genes is recorded in SHUFFLE_MAX_Z below; it must stay below 5."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spatial_reference as sr

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
LN10 = np.log(10.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHUFFLE_SEED = 1


def ratio(err, bound):
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = r[~np.isnan(r)]
    return float(r.max()) if r.size else 0.0


def within(got, want, bound, what):
    """NaN exactly where the restatement has NaN, and |got - want| <= bound elsewhere.  Where the derived bound itself is
    not finite (a complete graph: Var(I) = 0, so z is 0 / 0 or x / 0) nothing can be asserted of a finite or infinite
    value.  Returns the largest ratio."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(bound, np.shape(want))
    open_ = ~np.isnan(want) & ~np.isfinite(bound)
    assert np.array_equal(np.isnan(got) & ~open_, np.isnan(want)), (what, "NaN pattern")
    ok = ~np.isnan(want) & ~open_
    same = np.isinf(want) & (got == want)
    err = np.where(same | ~ok, 0.0, np.abs(got - want))
    assert not (err[ok] > bound[ok]).any(), (what, float(np.nanmax(err[ok] / bound[ok])))
    return ratio(err[ok], bound[ok])


def padded(x, extra=5):
    """x as a device view with a row stride larger than its width."""
    wide = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.from_numpy(x[:1]).dtype, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def special_genes(x, rng):
    """Overwrites the first genes with the edge cases: a constant gene, one constant but for one spot."""
    x = x.copy()
    if x.shape[1] >= 1:
        x[:, 0] = 1.75
    if x.shape[1] >= 2:
        x[:, 1] = 0.0
        x[rng.integers(0, x.shape[0]), 1] = 3.0
    return x


# ------------------------------------------------------------------------------------------------------- the graph
LATTICE_CASES = [  # (n, k, prune, row_standardise, coordinates)
    (2, 1, "NA", True, "jitter"), (9, 8, "NA", False, "jitter"), (9, 8, "STD", True, "jitter"),
    (65, 4, "Grid", True, "holes"), (65, 64, "STD", False, "jitter"), (293, 6, "STD", True, "jitter"),
    (293, 8, "Grid", False, "integer"), (293, 8, "NA", True, "duplicates"), (4097, 8, "STD", True, "jitter"),
]


def coords_of(n, kind, seed=0):
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil(np.sqrt(n * 1.3)))
    if kind == "integer":
        c = sr.make_coords(side, side, seed, integer=True)
        return c[rng.permutation(c.shape[0])[:n]]
    c = sr.make_coords(side, side, seed)
    c = c[rng.permutation(c.shape[0])[:n]]
    if kind == "holes":                          # spread the spots out: Grid pruning leaves islands
        c = c * np.where(rng.random((n, 1)) < 0.3, 3.0, 1.0)
    if kind == "duplicates":
        c[n // 2:n // 2 + 20] = c[:20]
    return c


def graph_bound(n, k, S):
    return 2 * (-(-n // 256) + 8 + k + 4) * EPS * np.abs(S)


def check_graph(g, s, ref, n, k, what):
    a, b = int(g["offsets"][s]), int(g["offsets"][s + 1])
    nbr, w, deg = (g[key][a:b].cpu().numpy() for key in ("nbr", "w", "deg"))
    assert np.array_equal(nbr, ref["nbr"]), (what, "nbr")
    assert np.array_equal(deg, ref["deg"]), (what, "deg")
    assert np.array_equal(w == 0, ref["w"] == 0), (what, "zero pattern")
    worst = {"w": within(w, ref["w"], EPS * ref["w"] + 1e-300, (what, "w"))}
    for key in ("S0", "S1", "S2"):
        worst[key] = within(g[key][s], ref[key], graph_bound(n, k, ref[key]) + 1e-300, (what, key))
    return worst


@pytest.fixture(scope="module")
def lattice_refs():
    """The restatement's graph of every lattice case, computed once."""
    out = {}
    for case in LATTICE_CASES:
        n, k, prune, std, kind = case
        c = coords_of(n, kind)
        out[case] = (c, sr.lattice(c, k, prune, std))
    return out


@pytest.mark.parametrize("case", LATTICE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_lattice(case, lattice_refs):
    from mclstexp_amd import spatial
    n, k, prune, std, kind = case
    c, ref = lattice_refs[case]
    if kind == "holes":
        assert (ref["deg"] == 0).any() and (ref["deg"] > 0).any()            # islands
    if kind == "integer":
        assert (ref["dist"][:, 1:] == ref["dist"][:, :-1]).any()             # ties
    for coords in (c, torch.from_numpy(c.astype(np.float64)).cuda()) if kind != "integer" else (c,):
        g = spatial.lattice(coords, None, k, prune, std)
        print(case, check_graph(g, 0, ref, n, k, case))
    if kind == "jitter" and n == 293:                                        # fp32 coordinates: the fp32 values are the input
        c32 = c.astype(np.float32)
        g = spatial.lattice(c32, None, k, prune, std)
        check_graph(g, 0, sr.lattice(c32.astype(np.float64), k, prune, std), n, k, (case, "fp32"))


def test_given_graph_and_its_refusals():
    from mclstexp_amd import spatial
    c = coords_of(65, "jitter")
    ref = sr.lattice(c, 6, "STD", True)
    g = spatial.lattice(nbr=ref["nbr"], w=ref["w"])
    assert g["row_standardise"] is True
    check_graph(g, 0, ref, 65, 6, "given, standardised")
    refb = sr.lattice(c, 6, "STD", False)
    g = spatial.lattice(nbr=torch.from_numpy(refb["nbr"]).cuda(), w=torch.from_numpy(refb["w"]).cuda())
    assert g["row_standardise"] is False
    check_graph(g, 0, refb, 65, 6, "given, binary")
    # an expression-space kNN list scores too: self loops and all
    loops = np.stack([np.arange(65), (np.arange(65) + 1) % 65], axis=1).astype(np.int32)
    wl = np.ones((65, 2))
    g = spatial.lattice(nbr=loops, w=wl)
    W = sr.dense(loops, wl)
    want = {"S0": W.sum(), "S1": 0.5 * ((W + W.T) ** 2).sum(), "S2": ((W.sum(axis=1) + W.sum(axis=0)) ** 2).sum()}
    for key in want:
        assert g[key][0] == want[key] == sr.graph_consts(loops, wl)[key]
    bad = ref["nbr"].copy()
    bad[3, 2] = 65
    with pytest.raises(ValueError, match="indices outside"):
        spatial.lattice(nbr=bad, w=ref["w"])
    bad[3, 2] = -1
    with pytest.raises(ValueError, match="indices outside"):
        spatial.lattice(nbr=bad, w=ref["w"])
    wneg = refb["w"].copy()
    wneg[5, 0] = -1.0
    with pytest.raises(ValueError, match="negative"):
        spatial.lattice(nbr=refb["nbr"], w=wneg)
    with pytest.raises(ValueError, match="negative or not finite"):
        spatial.lattice(nbr=torch.from_numpy(refb["nbr"]).cuda(), w=torch.from_numpy(np.where(refb["w"] > 0, np.nan, 0.0)).cuda())
    dup = refb["nbr"].copy()
    dup[7, 1] = dup[7, 0]
    with pytest.raises(ValueError, match="twice"):
        spatial.lattice(nbr=dup, w=np.ones_like(refb["w"]))
    wany = np.where(refb["w"] > 0, 0.37, 0.0)
    with pytest.raises(ValueError, match="neither binary"):
        spatial.lattice(nbr=refb["nbr"], w=wany)


# ------------------------------------------------------------------------------------------------------ statistics
def tail_bounds(z, bz, p, nl):
    with np.errstate(all="ignore"):
        relp = (np.abs(z) + 1.0) * bz + (2 * z * z + 64) * EPS
        return relp * p + 1e-290, relp / LN10 + 16 * EPS * np.abs(nl) + 1e-300


def var_amplification(n, S0, S1, S2, bS):
    """Relative bounds of Var(I) and Var(C) under relative errors bS of S0, S1, S2 (and 8 eps of arithmetic)."""
    n, S0, S1, S2 = np.float64(n), np.float64(S0), np.float64(S1), np.float64(S2)
    with np.errstate(all="ignore"):
        return _var_amplification(n, S0, S1, S2, bS)


def _var_amplification(n, S0, S1, S2, bS):
    EI, VI, _, VC = sr.moments(n, S0, S1, S2)
    s02 = S0 * S0
    ampI = ((n * n * S1 + n * S2 + 3 * s02) / ((n * n - 1) * s02) + EI * EI) / VI
    ampC = (((2 * S1 + S2) * (n - 1) + 4 * s02) / (2 * (n + 1) * s02)) / VC
    return (3 * bS + 8 * EPS) * ampI, (3 * bS + 8 * EPS) * ampC, VI, VC


def check_stats(dev, x, ref_graph, k, what, two_tailed=False, perms=None):
    """One slide of the device result against the restatement, every bound of the module docstring."""
    n = x.shape[0]
    g = ref_graph
    b = sr.stat_bounds(x, g["nbr"], g["w"], g["S0"])
    I, C, parts = sr.statistics(x, g["nbr"], g["w"], g["S0"], parts=True)
    worst = {"mean": within(dev["mean"], parts["mean"], b["mean"] + 1e-300, (what, "mean")),
             "den": within(dev["den"], parts["den"], b["den"] + 1e-300, (what, "den"))}
    bS = 2 * (-(-n // 256) + 8 + k + 4) * EPS
    relI, relC, VI, VC = var_amplification(n, g["S0"], g["S1"], g["S2"], bS)
    zI, zC = sr.z_scores(I, C, n, g["S0"], g["S1"], g["S2"])
    for name, stat, bstat, z, relv, V in (("moran", I, b["I"], zI, relI, VI), ("geary", C, b["C"], zC, relC, VC)):
        if name not in dev:
            continue
        d = dev[name]
        with np.errstate(all="ignore"):
            bst = bstat + np.abs(stat) * bS                      # S0 enters as a factor
            bz = bst / np.sqrt(V) + np.abs(z) * (0.5 * relv + 8 * EPS)
        p, nl = sr.normal_tail(z, two_tailed)
        p, nl = np.where(np.isnan(z), np.nan, p), np.where(np.isnan(z), np.nan, nl)
        bp, bnl = tail_bounds(z, bz, p, nl)
        worst[name + " stat"] = within(d["stat"], stat, bst + 1e-300, (what, name, "stat"))
        worst[name + " z"] = within(d["z_norm"], z, bz + 1e-300, (what, name, "z_norm"))
        worst[name + " p"] = within(d["pval_norm"], p, bp, (what, name, "pval_norm"))
        worst[name + " nl"] = within(d["neglog10_pval_norm"], nl, bnl, (what, name, "neglog10"))
        worst[name + " adj"] = within(d["pval_norm_adj"], sr.bh(p), np.nanmax(bp) if np.isfinite(bp).any() else 1e-290,
                                      (what, name, "adj"))
        assert abs(d["expected"] - (sr.moments(n, g["S0"], g["S1"], g["S2"])[0 if name == "moran" else 2])) <= 4 * EPS
        with np.errstate(all="ignore"):
            within([d["var_norm"]], [V], np.array([(relv + 8 * EPS) * np.abs(V)]), (what, name, "var_norm"))
        if perms is None:
            continue
        # the sims against the statistic evaluated at the permuted data, and everything derived from them
        P = perms.shape[0]
        sims = d["sims"]
        want = sr.simulate(x, g["nbr"], g["w"], g["S0"], perms)[0 if name == "moran" else 1]
        bs = np.stack([sr.stat_bounds(x, g["nbr"], g["w"], g["S0"], pm)["I" if name == "moran" else "C"] for pm in perms])
        with np.errstate(all="ignore"):
            bs = bs + np.abs(want) * bS
        worst[name + " sims"] = within(sims, want, bs + 1e-300, (what, name, "sims"))
        own = sr.perm_summary(d["stat"], sims, two_tailed)       # the exact count over the device's own values
        assert np.array_equal(d["count_sim"], own["count_sim"]), (what, name, "count")
        assert np.array_equal(d["pval_sim"], own["pval_sim"], equal_nan=True), (what, name, "pval_sim")
        rs = sr.perm_summary(stat, want, two_tailed)
        with np.errstate(all="ignore"):
            bmax = bs.max(axis=0)
            bmean = bmax + 2 * (P + 2) * EPS * np.abs(want).mean(axis=0)
            sd = np.sqrt(rs["var_sim"])
            bvar = 4 * sd * bmax + 2 * (P + 6) * EPS * rs["var_sim"]
            bzs = (bst + bmean) / sd + np.abs(rs["z_sim"]) * (0.5 * bvar / rs["var_sim"] + 8 * EPS)
        pz = np.where(np.isnan(stat), np.nan, sr.normal_tail(rs["z_sim"], two_tailed)[0])
        worst[name + " mean_sim"] = within(d["mean_sim"], rs["mean_sim"], bmean + 1e-300, (what, name, "mean_sim"))
        worst[name + " var_sim"] = within(d["var_sim"], rs["var_sim"], bvar + 1e-300, (what, name, "var_sim"))
        finite = np.isfinite(bzs)                               # (var_sim = 0, as for P = 1: z_sim is +-inf or NaN on both sides)
        worst[name + " pz_sim"] = within(np.where(finite, d["pval_z_sim"], np.nan), np.where(finite, pz, np.nan),
                                         tail_bounds(rs["z_sim"], bzs, pz, pz)[0], (what, name, "pval_z_sim"))
    return worst


STAT_CASES = [  # (n, k, prune, row_standardise, G, dtype, expression kind, padded row stride)
    (2, 1, "NA", True, 7, np.float64, "cont", False),
    (9, 8, "NA", False, 1, np.float32, "cont", False),
    (65, 4, "Grid", True, 785, np.float32, "counts", False),
    (293, 6, "STD", True, 7, np.float64, "scales", True),
    (293, 8, "NA", True, 785, np.float64, "cont", False),
    (4097, 8, "STD", True, 7, np.float32, "counts", True),
]


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda c: "-".join(getattr(v, "__name__", str(v)) for v in c))
def test_statistics(case):
    from mclstexp_amd import spatial
    n, k, prune, std, G, dtype, kind, pad = case
    rng = np.random.default_rng(n + G)
    c = coords_of(n, "holes" if prune == "Grid" else "jitter")
    x = special_genes(sr.make_expression(c, G, n + G, kind, dtype), rng) if G > 1 else sr.make_expression(c, G, n, kind, dtype)
    ref = sr.lattice(c, k, prune, std)
    g = spatial.lattice(c, None, k, prune, std)
    xd = padded(x) if pad else x
    P = 7 if G <= 7 else 2
    for two in (False, True):
        res = spatial.autocorr(xd, g, mode="both", n_perms=P, seed=3, return_sims=True, two_tailed=two,
                               return_permutations=True)[0]
        perms = sr.permutations(3, P, n)
        assert np.array_equal(res["permutations"], perms)
        print(case, two, check_stats(res, x, ref, k, case, two, perms))
    if G > 1:
        for m in ("moran", "geary"):
            assert np.isnan(res[m]["stat"][0]) and np.isnan(res[m]["pval_sim"][0]) and res[m]["count_sim"][0] == -1
            assert np.isfinite(res[m]["stat"][1])
    only = spatial.autocorr(xd, g, mode="geary")[0]
    assert "moran" not in only and np.array_equal(only["geary"]["stat"], res["geary"]["stat"], equal_nan=True)
    bad = x.copy()
    bad[n // 2, G - 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        spatial.autocorr(bad, g)


def torus(side, std):
    """The rook graph of a side x side torus as a given list: n = side^2 without a kNN search."""
    i = np.arange(side * side)
    r, c = i // side, i % side
    nbr = np.stack([((r + 1) % side) * side + c, ((r - 1) % side) * side + c, r * side + (c + 1) % side,
                    r * side + (c - 1) % side], axis=1).astype(np.int32)
    return nbr, np.full(nbr.shape, 0.25 if std else 1.0)


def test_one_column_per_workgroup_at_16384_spots():
    from mclstexp_amd import spatial
    nbr, w = torus(128, True)
    n = nbr.shape[0]
    assert n == 16384 and sr.columns(n) == 1
    ref = {"nbr": nbr, "w": w}
    ref.update(sr.graph_consts(nbr, w))
    g = spatial.lattice(nbr=nbr, w=w)
    for key in ("S0", "S1", "S2"):
        within(g[key][0], ref[key], graph_bound(n, 4, ref[key]), key)
    yy, xx = np.divmod(np.arange(n), 128)
    x = np.stack([np.sin(xx / 9.0) + np.cos(yy / 13.0), np.random.default_rng(0).normal(size=n)], axis=1)
    res = spatial.autocorr(x, g, mode="both", n_perms=2, seed=11, return_sims=True, return_permutations=True)[0]
    perms = sr.permutations(11, 2, n)
    assert np.array_equal(res["permutations"], perms)
    print("16384", check_stats(res, x, ref, 4, "16384", False, perms))
    assert res["moran"]["stat"][0] > 0.9 and abs(res["moran"]["stat"][1]) < 0.05
    assert res["moran"]["pval_norm"][0] == 0.0 and np.isfinite(res["moran"]["neglog10_pval_norm"][0])   # |z| > 38


# ---------------------------------------------------------------------------------------------------- permutations
def ring(n):
    return ((np.arange(n) + 1) % n).astype(np.int32)[:, None], np.ones((n, 1))


@pytest.mark.parametrize("P", [1, 7, 100])
def test_permutation_table(P):
    """The device's table equals the restatement's for n in {2, 65, 4097, 16384}: one batch, and the slide's place in it
    is no input."""
    from mclstexp_amd import spatial
    sizes = [2, 65, 4097, 16384]
    parts = [ring(n) for n in sizes]
    g = spatial.lattice(nbr=np.concatenate([p[0] for p in parts]), w=np.concatenate([p[1] for p in parts]),
                        offsets=np.concatenate([[0], np.cumsum(sizes)]))
    x = np.random.default_rng(P).normal(size=(sum(sizes), 1))
    res = spatial.autocorr(x, g, n_perms=P, seed=5, return_permutations=True)
    for r, n in zip(res, sizes):
        assert np.array_equal(r["permutations"], sr.permutations(5, P, n)), n
    other = spatial.autocorr(x, g, n_perms=1, seed=6, return_permutations=True)
    assert not np.array_equal(other[3]["permutations"][0], res[3]["permutations"][0])


def test_identity_and_replayed_permutations():
    from mclstexp_amd import spatial
    n, k, G = 293, 6, 7
    c = coords_of(n, "jitter")
    x = sr.make_expression(c, G, 1, "cont", np.float32)
    g = spatial.lattice(c, None, k, "STD", True)
    ident = np.stack([np.arange(n)] * 2)
    res = spatial.autocorr(x, g, mode="both", permutations=[ident], return_sims=True)[0]
    for m in ("moran", "geary"):
        assert res[m]["sims"].shape == (2, G)
        assert all(np.array_equal(row, res[m]["stat"]) for row in res[m]["sims"]), m      # bit for bit
        assert np.array_equal(res[m]["count_sim"], np.zeros(G))                            # 2 of 2 >= stat, folded to 0
        assert np.array_equal(res[m]["var_sim"], np.zeros(G))                              # (s + s) / 2 = s exactly
    gen = spatial.autocorr(x, g, mode="both", n_perms=9, seed=2, return_sims=True, return_permutations=True)[0]
    rep = spatial.autocorr(x, g, mode="both", permutations=[gen["permutations"]], return_sims=True)[0]
    for m in ("moran", "geary"):
        for key in ("sims", "pval_sim", "pval_z_sim", "var_sim", "mean_sim", "count_sim"):
            assert np.array_equal(gen[m][key], rep[m][key], equal_nan=True), (m, key)


# ------------------------------------------------------------------------------------------------------ invariants
def same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for key in a:
            same(a[key], b[key], f"{path}.{key}")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path


def test_batch_is_bit_identical_to_single_calls_and_runs_repeat():
    from mclstexp_amd import spatial
    sizes, k, G = [150, 9, 4097, 293], 8, 11
    cs = [coords_of(n, "jitter", seed=s) for s, n in enumerate(sizes)]
    xs = [special_genes(sr.make_expression(c, G, 7 + s, "counts" if s % 2 else "cont", np.float32), np.random.default_rng(s))
          for s, c in enumerate(cs)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    kw = dict(mode="both", n_perms=6, seed=4, return_sims=True, return_permutations=True)
    gb = spatial.lattice(np.concatenate(cs), off, k, "STD", True)
    batch = spatial.autocorr(np.concatenate(xs), gb, **kw)
    again = spatial.autocorr(np.concatenate(xs), spatial.lattice(np.concatenate(cs), off, k, "STD", True), **kw)
    for s, n in enumerate(sizes):
        g1 = spatial.lattice(cs[s], None, k, "STD", True)
        a, b = int(off[s]), int(off[s + 1])
        for key in ("nbr", "w", "deg"):
            assert torch.equal(gb[key][a:b], g1[key]), (s, key)
        for key in ("S0", "S1", "S2"):
            assert gb[key][s] == g1[key][0], (s, key)
        same(batch[s], spatial.autocorr(xs[s], g1, **kw)[0], f"slide {s}")
        same(batch[s], again[s], f"run 2, slide {s}")
    via = spatial.autocorr_slides(xs, cs, k, "STD", True, **kw)
    for s in range(len(sizes)):
        same(batch[s], via[s], f"autocorr_slides, slide {s}")


# ------------------------------------------------------------------------------------------------ recovery and CLI
SHUFFLE_MAX_Z = 1.3216          # the restatement alone: max |z_norm| of I over the genes of the shuffled "mid" slide


def test_recovery_and_cli(tmp_path):
    from mclstexp_amd import spatial
    coords, x = sr.make_case("mid")
    n, G = x.shape
    shuffled = x[np.random.default_rng(SHUFFLE_SEED).permutation(n)]
    ref = sr.autocorr(shuffled, coords, 8, "NA", True)
    zmax = float(np.abs(ref["moran"]["z_norm"]).max())
    assert abs(zmax - SHUFFLE_MAX_Z) < 1e-3 and zmax < 5
    rec = spatial.svg_recovery([x], [x], [coords], n_top=4)
    assert rec["pearson"][0] == 1.0 and rec["overlap"][0] == 4 and rec["jaccard"][0] == 1.0 and rec["n_top"] == 4
    rec = spatial.svg_recovery([shuffled, x], [x, x], [coords, coords], n_top=4, mode="geary")
    assert rec["overlap"][1] == 4 and rec["pearson"][1] == 1.0
    got = spatial.autocorr_slides([shuffled], [coords])[0]
    assert np.abs(got["moran"]["z_norm"]).max() < 5
    true = sr.autocorr(x, coords, 8, "NA", True)
    want = sr.recovery(ref["geary"]["stat"], true["geary"]["stat"], 4, "geary")
    assert abs(rec["pearson"][0] - want[0]) < 1e-9 and (rec["overlap"][0], rec["jaccard"][0]) == want[1:]
    assert true["moran"]["z_norm"].max() > 5                     # the unshuffled slide does hold spatial genes
    # the CLI in a child process, on files stored gene-major
    np.save(tmp_path / "p.npy", shuffled.T)
    np.save(tmp_path / "t.npy", x.T)
    np.save(tmp_path / "c.npy", coords)
    np.save(tmp_path / "g.npy", np.array([f"G{j}" for j in range(G)]))
    out = subprocess.run([sys.executable, "-m", "mclstexp_amd.spatial", "--pred", str(tmp_path / "p.npy"), "--true",
                          str(tmp_path / "t.npy"), "--coords", str(tmp_path / "c.npy"), "--genes", str(tmp_path / "g.npy"),
                          "--mode", "both", "--n_perms", "10", "--seed", "2", "--top", "4", "--out_dir", str(tmp_path / "o")],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith(f"slide 0 n = {n} k = 8 S0 = {n}") and lines[0].count("(") == 6 and "G" in lines[0]
    assert sum(line.startswith("recovery (") for line in lines) == 2
    saved = np.load(tmp_path / "o" / "0" / spatial.OUT_FILE)
    direct = spatial.autocorr_slides([shuffled], [coords], mode="both", n_perms=10, seed=2)[0]
    for key in ("moran_stat", "geary_stat", "moran_pval_sim", "geary_pval_z_sim", "moran_pval_norm_adj"):
        m, sub = key.split("_", 1)
        assert np.array_equal(saved[key], direct[m][sub], equal_nan=True), key
    assert int(saved["n"]) == n and float(saved["S0"]) == float(n)
