"""GPU: mclstexp_amd.rank (csrc/rank.hip) against the Python-int restatement (tests/rank_reference.py) and scipy's stored
results (tests/golden/rank.npz): exact integers, rho and tau within 4 eps, ties and edge values, invariances, the limits,
device-side validation and the composition with evaluate / genes."""
import numpy as np
import pytest
import torch

import rank_reference as rr
from rank_reference import EPS, GOLDEN, P_FLOOR, T_P_REL, case_inputs, normal_p_bound

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
KEYS = ("spearman", "spearman_pval", "spearman_neglog10_pval", "kendall", "kendall_pval", "kendall_neglog10_pval")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def batch(z):
    """The batch's inputs (gene 2's pred zeros alternate in sign: a tie all the same) and its restatement, computed once."""
    pred, true = case_inputs(z, "batch")
    pred = pred.copy()
    zero = np.flatnonzero(pred[:, 2] == 0)
    pred[zero[::2], 2] = -0.0
    assert np.signbit(pred[:, 2]).any() and (pred[:, 2] == 0).sum() >= pred.shape[0] // 2
    off = z["batch.offsets"]
    ref = rr.matrix_stats(pred, true, off)
    for v in ref.values():
        v.setflags(write=False)
    return pred, true, off, ref


def dev(a, dtype, pad=0):
    """``a`` on the device as ``dtype``, with ``pad`` unused columns behind every row."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if not pad:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=dtype, device="cuda")   # never read
    buf[:, :t.shape[1]].copy_(t)
    return buf[:, :t.shape[1]]


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


def check_against(got, ref, want, dev_rho, dev_tau, sizes):
    """``got`` (device results on the host) against the restatement ``ref`` and scipy's ``want``; shapes agree."""
    assert np.array_equal(got["ints"], ref["ints"])                       # every integer, bit for bit
    for key, r, d in (("spearman", "rho", dev_rho), ("kendall", "tau", dev_tau)):
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref[r]))
        ok = ~np.isnan(ref[r])
        worst = np.abs(got[key][ok] - ref[r][ok]).max()
        print(f"{key}: max |device - restatement| = {worst:.3g}, max |device - scipy| = "
              f"{np.abs(got[key][ok] - want[r][ok]).max():.3g}")
        # the derived bound is 4 eps (three conversions, two square roots, a product and a division, |value| <= 1); the same
        # integers through the same correctly rounded operations give the same bits, on every case measured: asserted
        assert worst == 0.0 and np.array_equal(got[key][ok], ref[r][ok])
        assert np.abs(got[key][ok] - want[r][ok]).max() <= d + 4 * EPS
    n = np.broadcast_to(np.asarray(sizes).reshape((-1,) + (1,) * (got["spearman"].ndim - 1)), got["spearman"].shape)
    p, rp = got["spearman_pval"], ref["rho_p"]
    assert np.array_equal(np.isnan(p), np.isnan(rp))
    big = ~np.isnan(rp) & (rp >= P_FLOOR)
    assert (np.abs(p[big] - rp[big]) / rp[big]).max() <= T_P_REL
    nl, rnl = got["spearman_neglog10_pval"], ref["rho_nl"]
    assert np.array_equal(np.isposinf(nl), np.isposinf(rnl))
    fin = np.isfinite(rnl)
    assert np.abs(nl[fin] - rnl[fin]).max() <= 1e-9
    sp = want["rho_p"]
    cmp = big & ~np.isnan(sp) & (n > 2)
    assert (np.abs(p[cmp] - sp[cmp]) / sp[cmp]).max() <= T_P_REL
    tp, rtp = got["kendall_pval"], ref["tau_p"]
    assert np.array_equal(np.isnan(tp), np.isnan(rtp)) and np.isnan(tp[n < 3]).all()
    ok = ~np.isnan(rtp) & (rtp >= P_FLOOR)
    zs = np.sqrt(2.0) * np.abs(_erfcinv(rtp[ok]))
    assert np.all(np.abs(tp[ok] - rtp[ok]) <= normal_p_bound(zs, rtp[ok]))
    assert np.all(np.abs(tp[ok] - want["tau_p"][ok]) <= normal_p_bound(zs, rtp[ok]))
    tnl = got["kendall_neglog10_pval"]
    assert np.all(np.isfinite(tnl[~np.isnan(rtp)]))
    assert np.abs(tnl[ok] - ref["tau_nl"][ok]).max() <= 1e-9 * np.maximum(1.0, ref["tau_nl"][ok]).max()


def _erfcinv(p):
    from scipy import special
    return special.erfcinv(p)


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("G, dp, dt, pad", [(33, F32, F64, 5), (7, F64, F32, 0), (1, F32, F32, 3), (33, F64, F64, 0),
                                            (33, F32, F32, 0)])
def test_batch_matches_restatement_and_scipy(z, batch, G, dp, dt, pad):
    """Slides of 2, 3, 63, 64, 65, 257 and 1025 spots in one call; G = 1, 7, 33 (column tiles that do not divide G); a row
    stride larger than G; every dtype pairing."""
    from mclstexp_amd import rank
    pred, true, off, ref = batch
    got = host(rank.rank_device(dev(pred[:, :G], dp, pad), dev(true[:, :G], dt, pad), off.tolist()))
    want = {k: z[f"batch.{k}"][:, :G] for k in ("rho", "rho_p", "tau", "tau_p")}
    check_against(got, {k: v[:, :G] for k, v in ref.items()}, want, float(z["batch.dev_rho"]), float(z["batch.dev_tau"]),
                  np.diff(off))


def test_ties_and_edge_values(z, batch):
    from mclstexp_amd import rank
    pred, true, off, _ = batch
    assert ((pred[:, 0] == 0).mean() > 0.5) and ((true[:, 0] == 0).mean() > 0.5)          # the zero-inflated gene
    g = host(rank.rank_device(dev(pred, F32), dev(true, F32), off.tolist()))
    for k in KEYS:                                                                         # gene 1: a constant side
        assert np.isnan(g[k][:, 1]).all(), k
    big = np.diff(off) > 2
    assert not np.isnan(g["spearman"][np.diff(off) > 3][:, [0, 2, 3, 4]]).any()
    assert (g["spearman"][:, 3] == 1.0).all() and (g["kendall"][:, 3] == 1.0).all()        # gene 3: pred == true
    assert (g["spearman_pval"][big, 3] == 0.0).all() and np.isposinf(g["spearman_neglog10_pval"][big, 3]).all()
    assert (g["spearman"][:, 4] == -1.0).all() and (g["kendall"][:, 4] == -1.0).all()      # gene 4: pred == -true
    two = np.flatnonzero(np.diff(off) == 2)[0]                                             # n = 2
    d = ~np.isnan(g["spearman"][two])
    assert d.sum() > 3 and (np.abs(g["kendall"][two][d]) == 1.0).all() and np.isnan(g["kendall_pval"][two]).all()
    assert (g["spearman_pval"][two][d] == 1.0).all() and (g["spearman_neglog10_pval"][two][d] == 0.0).all()
    # -0.0 ties +0.0: the signs change nothing
    assert np.signbit(pred[:, 2]).any()
    plus = host(rank.rank_device(dev(np.where(pred[:, 2:3] == 0, 0.0, pred[:, 2:3]), F32), dev(true[:, 2:3], F32),
                                 off.tolist()))
    assert same_bits({k: v[:, 0] for k, v in plus.items()}, {k: v[:, 2] for k, v in g.items()})


def test_tau_off_skips_the_pair_walk(batch):
    from mclstexp_amd import rank
    pred, true, off, ref = batch
    a = host(rank.rank_device(dev(pred, F32), dev(true, F64), off.tolist(), tau=False))
    b = host(rank.rank_device(dev(pred, F32), dev(true, F64), off.tolist(), tau=True))
    assert sorted(a) == ["ints", "spearman", "spearman_neglog10_pval", "spearman_pval"]
    assert np.array_equal(a["ints"][..., :10], ref["ints"][..., :10]) and not a["ints"][..., 10:].any()
    assert same_bits({k: a[k] for k in a if k != "ints"}, {k: b[k] for k in a if k != "ints"})


# ------------------------------------------------------------------------------------------------ invariance
def test_slide_alone_and_row_permuted_are_bit_identical(batch):
    from mclstexp_amd import rank
    pred, true, off, _ = batch
    whole = host(rank.rank_device(dev(pred, F32, 2), dev(true, F64), off.tolist()))
    rng = np.random.default_rng(3)
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        alone = host(rank.rank_device(dev(pred[lo:hi], F32), dev(true[lo:hi], F64), None))
        assert same_bits({k: v[0] for k, v in alone.items()}, {k: v[s] for k, v in whole.items()}), s
        perm = rng.permutation(hi - lo)
        moved = host(rank.rank_device(dev(pred[lo:hi][perm], F32), dev(true[lo:hi][perm], F64), [0, hi - lo]))
        assert same_bits(moved, alone), s


def test_spots_axis_equals_genes_axis_of_the_transpose(z):
    from mclstexp_amd import rank
    pred, true = case_inputs(z, "spots")                                   # (40, 33)
    for dp, dt, pad in ((F32, F32, 0), (F64, F32, 7)):
        by_row = host(rank.rank_device(dev(pred, dp, pad), dev(true, dt, pad), None, axis="spots"))
        by_col = host(rank.rank_device(dev(pred.T, dp), dev(true.T, dt), None, axis="genes"))
        assert by_row["spearman"].shape == (40,) and by_col["spearman"].shape == (1, 40)
        assert same_bits(by_row, {k: v[0] for k, v in by_col.items()})
    ref = rr.matrix_stats(pred, true, axis="spots")
    want = {k: z[f"spots.{k}"] for k in ("rho", "rho_p", "tau", "tau_p")}
    check_against(by_row, ref, want, float(z["spots.dev_rho"]), float(z["spots.dev_tau"]), [33])


# ------------------------------------------------------------------------------------------------ limits
def test_sixteen_thousand_elements_in_one_problem(z):
    """One pair of 16384 float32 elements with ties: a single workgroup holding 128 KiB of keys and ranks."""
    from mclstexp_amd import rank
    pred, true = case_inputs(z, "limit")
    assert pred.size == rank.MAX_ELEMENTS_F32 and np.unique(pred).size < pred.size and np.unique(true).size < true.size
    g = host(rank.rank_device(dev(pred[:, None], F32), dev(true[:, None], F32), None))
    assert np.array_equal(g["ints"][0, 0], z["limit.ints"])
    rho, tau, zs = rr.finish(z["limit.ints"])
    assert g["spearman"][0, 0] == rho and g["kendall"][0, 0] == tau                        # bit-equal, as everywhere
    assert abs(rho - float(z["limit.rho"][0])) <= float(z["limit.dev_rho"]) + 4 * EPS
    assert abs(tau - float(z["limit.tau"][0])) <= float(z["limit.dev_tau"]) + 4 * EPS
    # both p-values underflow here (rho ~ 0.7 over 16384 elements); -log10 p stays finite
    assert g["spearman_pval"][0, 0] == float(z["limit.rho_p"][0]) == 0.0 and g["kendall_pval"][0, 0] == float(z["limit.tau_p"][0]) == 0.0
    assert np.isfinite(g["spearman_neglog10_pval"][0, 0]) and g["spearman_neglog10_pval"][0, 0] > 300
    tnl = float(rr.normal_tail(np.array([zs]), True)[1][0])
    assert abs(g["kendall_neglog10_pval"][0, 0] - tnl) <= 1e-9 * tnl


def test_float64_limit_and_one_element_over(z):
    from mclstexp_amd import rank
    from scipy import stats
    pred, true = case_inputs(z, "limit")
    n = rank.MAX_ELEMENTS_F64
    g = host(rank.rank_device(dev(pred[:n, None], F64), dev(true[:n, None], F32), None))
    sp, kt = stats.spearmanr(pred[:n], true[:n]), stats.kendalltau(pred[:n], true[:n], method="asymptotic")
    assert abs(g["spearman"][0, 0] - sp.statistic) <= 8 * EPS and abs(g["kendall"][0, 0] - kt.statistic) <= 8 * EPS
    assert g["ints"][0, 0, 0] == n
    for m, dp, dt in ((16385, F32, F32), (8193, F64, F32), (8193, F32, F64)):              # raised before any launch
        with pytest.raises(ValueError, match=str(m - 1)):
            rank.rank_device(torch.zeros((m, 1), dtype=dp, device="cuda"), torch.zeros((m, 1), dtype=dt, device="cuda"), None)
    with pytest.raises(ValueError, match="16384"):
        rank.rank_device(torch.zeros((4, 16385), device="cuda"), torch.zeros((4, 16385), device="cuda"), None, axis="spots")
    with pytest.raises(ValueError):
        rank.rank_device(torch.zeros((5, 2), device="cuda"), torch.zeros((5, 2), device="cuda"), [0, 1, 5])
    with pytest.raises(ValueError, match="offsets must be None"):                          # rows are ranked one by one
        rank.rank_device(torch.zeros((5, 2), device="cuda"), torch.zeros((5, 2), device="cuda"), [0, 5], axis="spots")


# ------------------------------------------------------------------------------------------------ validation
def test_non_finite_values_raise_and_the_call_returns(batch):
    """Argument checks on the device: a status word, never a fault; the next call works."""
    from mclstexp_amd import rank
    pred, true, off, ref = batch
    lo = int(off[3])                                                       # slides 3, 4, 5 as a batch of three
    sub = (off[3:7] - lo).tolist()
    p, t = pred[lo:int(off[6])].copy(), true[lo:int(off[6])].copy()
    bad = p.copy()
    bad[sub[2] + 11, 6] = np.nan                                           # in slide 2 of the three
    with pytest.raises(ValueError, match="slide 2 holds non-finite"):
        rank.rank_device(dev(bad, F32), dev(t, F64), sub)
    bad_t = t.copy()
    bad_t[sub[1] + 1, 0] = np.inf
    with pytest.raises(ValueError, match="slide 1 holds non-finite"):
        rank.rank_device(dev(p, F32), dev(bad_t, F64), sub)
    with pytest.raises(ValueError, match="row 17 holds non-finite"):
        rank.rank_device(dev(bad[sub[2] - 6:sub[2] + 20], F64), dev(t[sub[2] - 6:sub[2] + 20], F64), None, axis="spots")
    good = host(rank.rank_device(dev(p, F32), dev(t, F64), sub))
    assert np.array_equal(good["ints"], ref["ints"][3:6])


# ------------------------------------------------------------------------------------------------ composition
def test_score_folds_composes_with_evaluate_and_genes(z, batch):
    from mclstexp_amd import evaluate, genes, rank
    pred, true, off, ref = batch
    preds = [pred[off[s]:off[s + 1]].astype(np.float32) for s in range(len(off) - 1)]
    trues = [true[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    res = rank.score_folds(preds, trues, n_heg=5)
    pcc = evaluate.score_folds(preds, trues, n_heg=5)
    for s, (f, e) in enumerate(zip(res["folds"], pcc["folds"])):
        assert np.array_equal(f["heg_genes"], e["heg_genes"])
        for key, r in (("spearman", "rho"), ("kendall", "tau")):
            assert np.allclose(f[key], ref[r][s], rtol=0, atol=4 * EPS, equal_nan=True)
        want = rr.summary(f["spearman"], f["kendall"], f["heg_genes"])
        have = (f["heg_spearman"], f["hvg_spearman"], f["heg_kendall"], f["hvg_kendall"], f["n_valid"])
        assert np.array_equal(np.array(have), np.array(want), equal_nan=True), s          # gene-index order: the same bits
        ok = ~np.isnan(f["spearman"])
        assert f["n_valid"] == ok.sum() <= 32 and not ok[1]                              # the constant gene is left out
        assert abs(f["hvg_spearman"] - f["spearman"][ok].mean()) <= 8 * EPS
        if not np.isin(1, f["heg_genes"]):
            assert abs(f["heg_spearman"] - np.mean(f["spearman"][np.sort(f["heg_genes"])])) <= 4 * EPS
    for k in rank.SUMMARY_KEYS:
        assert np.array_equal(res[k], np.mean([f[k] for f in res["folds"]]), equal_nan=True)
    one = rank.score(preds[4], trues[4], n_heg=5, tau=False)
    assert np.array_equal(one["spearman"], res["folds"][4]["spearman"], equal_nan=True) and "kendall" not in one
    assert np.isnan(one["heg_kendall"]) and one["heg_spearman"] == res["folds"][4]["heg_spearman"]
    # the (S, G) matrices are the layout genes.rank_genes takes: a rank-based top-gene table
    nl = np.stack([f["spearman_neglog10_pval"] for f in res["folds"]])
    rho = np.stack([f["spearman"] for f in res["folds"]])
    table = genes.rank_genes(nl, rho, top_n=3)
    assert sorted(table["order"].tolist()) == list(range(33)) and table["n_defined"][1] == 0 and len(table["top"]) == 3
    assert table["order"][-1] == 1 and np.isposinf(table["mean"][3])                     # undefined last; pred == true first


def test_get_R_matches_the_reference(z, batch):
    """The reference's own get_R(..., func=spearmanr) on both dims, stored beside scipy's values."""
    from mclstexp_amd import rank
    pred, true, off, _ = batch
    s = int(z["ref.slide"])
    lo, hi = int(off[s]), int(off[s + 1])
    r1, p1 = rank.get_R(pred[lo:hi], true[lo:hi].astype(np.float32), dim=1, func="spearmanr")
    assert np.array_equal(np.isnan(r1), np.isnan(z["ref.r1"]))
    ok = ~np.isnan(r1)
    assert np.abs(r1[ok] - z["ref.r1"][ok]).max() <= float(z["batch.dev_rho"]) + 4 * EPS
    big = ok & (z["ref.p1"] >= P_FLOOR)
    assert (np.abs(p1[big] - z["ref.p1"][big]) / z["ref.p1"][big]).max() <= T_P_REL and (p1[ok & ~big] < 2 * P_FLOOR).all()
    ps, ts = case_inputs(z, "spots")

    class Data:                                                            # what get_R reads of an AnnData
        def __init__(self, x):
            self.X, self.shape = x, x.shape

    r0, p0 = rank.get_R(Data(ps.astype(np.float32)), Data(ts), dim=0, func="spearmanr")
    assert np.abs(r0 - z["ref.r0"]).max() <= float(z["spots.dev_rho"]) + 4 * EPS
    assert (np.abs(p0 - z["ref.p0"]) / z["ref.p0"]).max() <= T_P_REL
    rk, pk = rank.get_R(ps, ts, dim=0, func="kendalltau")
    assert np.abs(rk - z["spots.tau"]).max() <= float(z["spots.dev_tau"]) + 4 * EPS
    spot = rank.spot_rank(ps, ts)
    assert np.array_equal(spot["spearman"], r0) and np.array_equal(spot["kendall"], rk) and np.array_equal(spot["kendall_pval"], pk)
