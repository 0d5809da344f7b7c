"""CPU: the numpy restatement tests/hotspot_reference.py against independent formulas (tests/golden/hotspot.npz, written by
tests/golden/gen_hotspot_goldens.py), the stated properties of the conditional draws, and the host rules of
mclstexp_amd.hotspot.  Header / ctypes agreement of the mcl_hotspot_* entry points comes from tests/test_capi_symbols.py."""
import os
import sys

import numpy as np
import pytest

import hotspot_reference as hr
import spatial_reference as sr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_hotspot_goldens as gen  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(hr.GOLDEN))


def close(a, b, rtol=1e-10, atol=1e-12):
    return np.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


# ------------------------------------------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("name", ["small", "mid"])
@pytest.mark.parametrize("std", [False, True])
def test_restatement_matches_the_dense_formulas(golden, name, std):
    c, x = sr.make_case(name)
    g = sr.lattice(c, 8, "STD", std)
    pairs = gen.dense_pairs(x.shape[1])
    r = hr.local_stats(x, g["nbr"], g["w"], pairs)
    key = f"{name}.{'r' if std else 'b'}."
    assert close(r["local_i"], golden[key + "local_i"])
    assert close(r["lag"], golden[key + "lag"])
    uni = pairs[:, 0] == pairs[:, 1]
    assert close(r["gi_z"][:, uni], golden[key + "gi_z"][:, uni])
    assert np.isnan(r["gi_z"][:, ~uni]).all()                      # Gi* is univariate
    # and the dense formulas as they are computed today
    d = hr.dense_local(x, g["nbr"], g["w"], pairs)
    assert close(d["local_i"], golden[key + "local_i"])


def test_normal_tail_against_scipy(golden):
    z = golden["tail.z"]
    p, nl = sr.normal_tail(z)
    rel = (2 * z * z + 64) * hr.EPS                                 # the condition of sf at z, as the GPU bounds take it
    assert (np.abs(p - golden["tail.sf"]) <= rel * golden["tail.sf"]).all()
    assert (np.abs(nl + np.log10(golden["tail.sf"])) <= rel / np.log(10.0) + 16 * hr.EPS * nl).all()


@pytest.mark.parametrize("name,prune,std", [("small", "NA", True), ("mid", "STD", False), ("wide", "Grid", True)])
def test_sum_identity(name, prune, std):
    """sum_i I_i = I S0 (n - 1) / n with autocorr's global I."""
    c, x = sr.make_case(name)
    g = sr.lattice(c, 8, prune, std)
    n = x.shape[0]
    r = hr.local_stats(x, g["nbr"], g["w"])
    I, _ = sr.statistics(x, g["nbr"], g["w"], g["S0"])
    assert np.allclose(r["local_i"].sum(axis=0), I * g["S0"] * (n - 1) / n, rtol=1e-11, atol=1e-12)


def test_quadrants_edge_cases_and_labels():
    c, x = sr.make_case("small")
    x = x.copy()
    x[:, 0] = 2.5                                                   # a constant gene
    g = sr.lattice(sr.make_coords(7, 7, 2, integer=True), 8, "Grid", True)
    n = g["nbr"].shape[0]
    x = np.resize(x, (n, x.shape[1]))
    x[:, 0] = 2.5
    g["w"][3] = 0.0                                                 # an isolated spot
    r = hr.local_stats(x, g["nbr"], g["w"], n_perms=19, seed=1, alpha=0.1)
    for key in hr.FLOATS:
        assert np.isnan(r[key][:, 0]).all(), key
    assert (r["cluster"][:, 0] == 0).all() and (r["quadrant"][:, 0] == 0).all()
    assert (r["lag"][3] == 0).all() and (r["local_i"][3, 1:] == 0).all() and (r["pval_sim"][3, 1:] == 1.0).all()
    za, L, q = r["za"][:, 1:], r["lag"][:, 1:], r["quadrant"][:, 1:]
    assert ((q == 1) == ((za > 0) & (L > 0))).all() and ((q == 3) == ((za < 0) & (L < 0))).all()
    assert ((q == 2) == ((za < 0) & (L > 0))).all() and ((q == 4) == ((za > 0) & (L < 0))).all()
    assert ((r["cluster"] == 0) | (r["cluster"] == r["quadrant"])).all()
    assert ((r["cluster"][:, 1:] != 0) == ((r["pval_sim"][:, 1:] <= 0.1) & (q != 0))).all()
    assert (r["count_ge"] + r["count_le"] >= 19).all()
    # the complete graph: Gi* is NaN
    g2 = sr.lattice(sr.make_coords(3, 3, 1), 8, "NA", False)
    r2 = hr.local_stats(x[:9], g2["nbr"], g2["w"])
    assert np.isnan(r2["gi_z"]).all() and np.isfinite(r2["local_i"][:, 1:]).all()


def test_ties_count_on_both_sides():
    """Count-like data: a tied sim is counted in count_ge and in count_le, and a spot whose every sim ties gets p = 1."""
    c = sr.make_coords(8, 8, 3)
    x = sr.make_expression(c, 3, 5, kind="counts")
    x[:, 2] = 0.0
    x[0, 2] = 1.0                                                   # exact zeros but for one spot
    g = sr.lattice(c, 4, "NA", False)
    r = hr.local_stats(x, g["nbr"], g["w"], n_perms=5, seed=2)
    assert (r["count_ge"] + r["count_le"] > 5).any()
    every = (r["count_ge"][:, 2] == 5) & (r["count_le"][:, 2] == 5)
    assert every.any() and (r["pval_sim"][every, 2] == 1.0).all()


# ------------------------------------------------------------------------------------------------------------ draws
def test_draw_tables_are_the_recorded_ones(golden):
    for seed, n, d in gen.DRAW_TRIPLES:
        tb = hr.draw_table(seed, gen.DRAW_P, n, np.full(n, d), d)
        assert np.array_equal(tb, golden[f"draws.{seed}.{n}.{d}"].astype(np.int64)), (seed, n, d)


@pytest.mark.parametrize("n,k", [(2, 1), (9, 8), (40, 8), (257, 3), (300, 64)])
def test_every_draw_is_distinct_in_range_and_not_the_spot(n, k):
    deg = np.random.default_rng(n).integers(0, min(k, n - 1) + 1, size=n)
    deg[0] = min(k, n - 1)
    tb = hr.draw_table(5, 7, n, deg, k)
    assert hr.check_table(tb, deg)
    assert not hr.check_table(np.where(tb == hr.PAD, 0, tb), deg) or (deg == k).all()


def test_a_draw_depends_on_seed_p_i_n_d_alone():
    n, k = 61, 8
    deg = np.random.default_rng(0).integers(0, k + 1, size=n)
    tb = hr.draw_table(9, 5, n, deg, k)
    # spot by spot with a constant degree vector: the same rows
    for d in np.unique(deg):
        one = hr.draw_table(9, 5, n, np.full(n, d), k)
        assert np.array_equal(one[:, deg == d], tb[:, deg == d])
    # draw p alone: the prefix of a longer run
    assert np.array_equal(hr.draw_table(9, 3, n, deg, k), tb[:3])
    # the statistics of a gene do not depend on the other genes of the call, nor on the slide's place in a batch (the
    # restatement takes one slide at a time; the device test compares a batch against each slide alone)
    c = sr.make_coords(8, 8, 1)[:n]
    x = sr.make_expression(c, 4, 3)
    g = sr.lattice(c, k, "STD", True)
    ra = hr.local_stats(x, g["nbr"], g["w"], n_perms=9, seed=4)
    rb = hr.local_stats(x, g["nbr"], g["w"], pairs=[[2, 2]], n_perms=9, seed=4)
    for key in ("count_ge", "count_le", "sum1", "sum2", "local_i", "z_sim"):
        assert np.array_equal(ra[key][:, 2], rb[key][:, 0], equal_nan=True), key
    assert (hr.draw_table(9, 5, n, deg, k) != hr.draw_table(10, 5, n, deg, k)).any()


def test_marginal_uniformity(golden):
    """n = 40, d = 8, P = 4000, seed 0: every other spot's frequency lies within 5 standard deviations of d / (n - 1).
    Largest deviation of the restatement: 3.46 standard deviations (seeds 1 and 2: 3.15 and 3.50)."""
    worst = gen.uniformity(**gen.UNIFORM)
    assert worst < 5.0
    assert worst == pytest.approx(float(golden["uniform.worst"]), abs=1e-12)


def test_recorded_behaviour_of_the_restatement(golden):
    """The inputs of the two behavioural GPU tests satisfy them on the restatement alone."""
    c, x, interior, outside = hr.planted_case()
    g = sr.lattice(c, 8, "NA", True)
    r = hr.local_stats(x, g["nbr"], g["w"], n_perms=gen.N_PERMS, seed=0, alpha=0.05)
    assert (r["cluster"][interior, 0] == 1).all() and int(golden["planted.interior_hh"]) == interior.sum() == 16
    assert int((r["cluster"][outside, 0] == 1).sum()) == int(golden["planted.outside_hh"]) == 6
    assert float(golden["shuffle.self_jaccard_hot"]) == 1.0
    assert float(golden["shuffle.mean_jaccard_hot"]) < 0.1 and abs(float(golden["shuffle.mean_pearson"])) < 0.2


# ------------------------------------------------------------------------------------------------------- host rules
def test_host_validation_errors():
    from mclstexp_amd import hotspot as hs
    graph = {"nbr": None, "w": None, "offsets": np.array([0, 10]), "offsets_device": None, "k": 3}
    assert hs.check_local((10, 4), graph, 5, 0, 0.05, False) == (10, 4, 5, 0, 0.05)
    for bad in (dict(shape=(10,)), dict(shape=(11, 4)), dict(n_perms=-1), dict(n_perms=70000), dict(seed=-1), dict(alpha=1.5),
                dict(alpha="x"), dict(return_draws=1), dict(graph={"nbr": 1})):
        kw = dict(shape=(10, 4), graph=graph, n_perms=5, seed=0, alpha=0.05, return_draws=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            hs.check_local(**kw)
    assert np.array_equal(hs.check_pairs(None, None, 3), [[0, 0], [1, 1], [2, 2]])
    assert np.array_equal(hs.check_pairs(None, [2, 0], 3), [[2, 2], [0, 0]])
    assert hs.check_pairs([[0, 2]], None, 3).dtype == np.int32
    for pairs, genes in (([[0, 3]], None), ([[0, -1]], None), ([[0, 1, 2]], None), ([[0.0, 1.0]], None), (None, [3]),
                         (None, []), ([[0, 1]], [0])):
        with pytest.raises(ValueError):
            hs.check_pairs(pairs, genes, 3)
    with pytest.raises(ValueError, match="row 1"):
        hs.check_pairs([[0, 1], [0, 7]], None, 3)
    # draws: what the restatement generates passes, in the device's layout
    sizes, k = np.array([5, 7]), 3
    degs = [np.array([3, 2, 0, 3, 1]), np.full(7, 3)]
    tabs = [hr.draw_table(1, 4, int(n), d, k) for n, d in zip(sizes, degs)]
    flat = hs.check_draws(tabs, sizes, k)
    assert flat.dtype == np.int16 and flat.size == 4 * 12 * k
    assert np.array_equal(flat[:4 * 5 * k].reshape(4, 5, k), tabs[0])

    def broken(fn):
        t = [a.copy() for a in tabs]
        fn(t)
        return t
    cases = [lambda t: t.pop(), lambda t: t.__setitem__(0, t[0][:3]), lambda t: t.__setitem__(1, t[1][:, :, :2]),
             lambda t: t.__setitem__(0, t[0].astype(np.float64)), lambda t: t[1].__setitem__((0, 2, 0), 2),      # the spot itself
             lambda t: t[1].__setitem__((1, 0, 1), 7), lambda t: t[1].__setitem__((1, 0, 1), t[1][1, 0, 0]),     # range, twice
             lambda t: t[0].__setitem__((0, 1, 0), hr.PAD)]                                                      # a hole
    for fn in cases:
        with pytest.raises(ValueError):
            hs.check_draws(broken(fn), sizes, k)
    with pytest.raises(ValueError, match=r"draws\[1\]: draw 1 of spot 0"):
        hs.check_draws(broken(cases[5]), sizes, k)
    with pytest.raises(ValueError, match="complex"):
        hs.colocalisation(None, graph, [(0, (1, 2))])
    with pytest.raises(ValueError):
        hs.hotspots([{"local_i": 0}], 0, 0)
    with pytest.raises(ValueError):
        hs.hotspot_recovery([np.zeros((4, 2))], [np.zeros((5, 2))], [np.zeros((4, 2))])


def test_compare_and_hotspots_on_the_host():
    from mclstexp_amd import hotspot as hs
    c, x = sr.make_case("mid")
    g = sr.lattice(c, 8, "NA", True)
    rt = hr.local_stats(x, g["nbr"], g["w"], n_perms=49, seed=0)
    rp = hr.local_stats(x[::-1], g["nbr"], g["w"], n_perms=49, seed=0)
    mine, ref = hs.compare(rp, rt), hr.recovery(rp, rt)
    for key in ref:
        assert np.array_equal(mine[key], ref[key], equal_nan=True), key
    same = hs.compare(rt, rt, "moran")
    assert np.allclose(same["pearson"], 1.0) and (same["agreement"] == 1.0).all()
    assert np.array_equal(hs.hotspots([rt], 0, 1), np.flatnonzero(rt["cluster"][:, 1] == 1))
    assert np.array_equal(hs.hotspots([rt], 0, 1, kind="cold"), np.flatnonzero(rt["cluster"][:, 1] == 3))


def test_cli_argument_parsing():
    from mclstexp_amd import hotspot as hs
    a = hs.parse_args(["--pred", "p0.npy", "p1.npy", "--coords", "c0.npy", "c1.npy"])
    assert (a.k, a.prune, a.n_perms, a.seed, a.alpha, a.true, a.select, a.pairs, a.out_dir) == (8, "NA", 999, 0, 0.05, None, None,
                                                                                                 None, None)
    a = hs.parse_args(["--pred", "p.npy", "--coords", "c.npy", "--true", "t.npy", "--genes", "g.npy", "--select", "A", "B",
                       "--pairs", "lr.tsv", "--k", "6", "--prune", "Grid", "--n_perms", "99", "--seed", "3", "--alpha", "0.01",
                       "--out_dir", "out"])
    assert (a.k, a.prune, a.n_perms, a.seed, a.alpha, a.select, a.pairs, a.out_dir) == (6, "Grid", 99, 3, 0.01, ["A", "B"],
                                                                                       "lr.tsv", "out")
    for argv in (["--pred", "p.npy", "--coords", "c.npy", "d.npy"], ["--pred", "p.npy", "--coords", "c.npy", "--k", "65"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--n_perms", "0"], ["--pred", "p.npy", "--coords", "c.npy", "--alpha", "2"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--prune", "x"], ["--pred", "p.npy", "--coords", "c.npy", "--pairs", "f"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--true", "a.npy", "b.npy"]):
        with pytest.raises(SystemExit):
            hs.parse_args(argv)
    assert np.array_equal(hs.select_columns(["B", "2"], ["A", "B", "C"], 3), [1, 2])
    assert hs.select_columns(None, None, 3) is None
    with pytest.raises(ValueError):
        hs.select_columns(["Z"], ["A"], 1)


def test_argument_errors_of_the_entry_points_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    for n in (2, 100, 3242, 3243, 9728, 9729, 16384):
        assert lib.mcl_hotspot_columns(n) == sr.columns(n) == lib.mcl_spatial_columns(n), n
    assert lib.mcl_hotspot_columns(1) == -1 and lib.mcl_hotspot_columns(16385) == -1
    assert lib.mcl_hotspot_table_bytes(100, 8, 7) >= 100 * 8 * 7 * 2
    assert lib.mcl_hotspot_table_bytes(100, 65, 7) == -1 and lib.mcl_hotspot_table_bytes(100, 8, 0) == -1
    assert lib.mcl_hotspot_moments(None, 0, 0, None, 1, 10, 3, 10, None, 3, None, None, None, None) == -1
    assert lib.mcl_hotspot_draws(None, 1, 10, 10, 8, None, 5, 0, None, None) == -1
