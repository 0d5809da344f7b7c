"""GPU: mclstexp_amd.markers (csrc/markers.hip) against the numpy restatement tests/markers_reference.py, which
tests/test_markers_host.py pins to scipy and mpmath.

Bounds (derived, not tuned; eps = 2^-52):
  rank sums R2, tie terms T, group sizes, non-zero counts, pts      exact (array_equal)
  Wilcoxon score                                                    8 ulp: a fixed expression of those integers
  Wilcoxon p                                                        ((8 z^2 + c0) eps) relative + 1e-290; c0 = 4 x the
                                                                    restatement's recorded error against scipy / mpmath
  -log10 p                                                          the p bound / ln 10 + 4 x the restatement's recorded
                                                                    relative error against mpmath x the value
  means                                                             (ceil(n / 4) + 2) eps sum|x| / n_g: the kernel sums a
                                                                    quarter of the rows in row order, then (q0 + q1) + (q2 + q3)
  variances                                                         ((ceil(n / 4) + 6) eps sum d^2 + n_g dmean^2) / (n_g - 1)
  Welch t, nu                                                       first-order propagation of the moment bounds
  Welch p                                                           |p(t +- dt, nu +- dnu) - p(t, nu)| by the restatement +
                                                                    c0t eps p, c0t = 4 x its recorded error against mpmath
  pvals_adj                                                         the largest p bound of the group (BH is monotone and
                                                                    1-homogeneous in p)
  names                                                             the stable order of the device's own scores, exactly; the
                                                                    scipy-derived order on the fixtures with the gap condition

Measured on MI355X, largest error / bound over the cases of each test (every test prints its rows with -s):

  test                          means   vars    Wilcoxon score  Wilcoxon p  -log10 p  Welch t  Welch p  pvals_adj  lfc
  slide sizes, G in {1, 7, 785} 0       0.093   0 (bit-equal)   0.037       0.18      0.0068   0.18     0.11       0.008
  batch of four slides          0       0.12    0               0.024       0.24      0.021    0.24     0.16       0.018
  scipy fixtures                0.029   0.055   0               0.029       0.13      0.019    0.13     0.065      0.025
  n = 4000, p underflows        0.0024  0.0029  0               0           0.0013    0.0018   0        0          0.0019
  recovery / CLI                0       0.076   0               0.020       0.017     -        -        0.013      0.015"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import markers_reference as mr
from golden.gen_markers_goldens import MP_CASES, SCIPY_CASES

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
LN10 = np.log(10.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(mr.GOLDEN)


@pytest.fixture(scope="module")
def consts(golden):
    names = sorted(SCIPY_CASES)
    c0 = 4 * max(max(float(golden[f"{n}.err_p"]), float(golden[f"{n}.err_p_mp"]), float(golden[f"{n}.err_p_tc"]))
                 for n in names) / EPS
    c0t = 4 * max(max(float(golden[f"{n}.err_p_t"]), float(golden[f"{n}.err_p_t_mp"])) for n in names) / EPS
    big = next(iter(MP_CASES))
    return {"c0": c0, "c0t": c0t, "nl_w": 4 * float(golden[f"{big}.err_nl_w"]), "nl_t": 4 * float(golden[f"{big}.err_nl_t"])}


def padded(x, extra=5):
    """x as a device view with a row stride larger than its width."""
    wide = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.from_numpy(x[:1]).dtype, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def ratio(err, bound):
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = r[~np.isnan(r)]
    return float(r.max()) if r.size else 0.0


def check_slide(dev, x, labels, k, consts, method="wilcoxon", tie_correct=False, n_genes=None, rankby_abs=False, what=""):
    """One slide of the device result against the restatement, every bound of the module docstring."""
    from mclstexp_amd import markers  # noqa: F401
    ref = mr.rank_genes_groups(x, labels, k, method, tie_correct, n_genes, rankby_abs)
    keep = labels >= 0
    xs, ls = x[keep].astype(np.float64), labels[keep]
    n, G = xs.shape
    for a, b in (("rank_sums2", "R2"), ("tie_terms", "T"), ("group_sizes", "group_sizes"), ("nnz", "nnz"),
                 ("nnz_rest", "nnz_rest"), ("pts", "pts"), ("pts_rest", "pts_rest")):
        assert np.array_equal(dev[a], ref[b], equal_nan=True), (what, a)
    assert dev["n_valid"] == ref["n_valid"]
    m = (n + 3) // 4
    worst = {}
    dmean, dvar = {}, {}
    with np.errstate(all="ignore"):
        for side, sel in (("", lambda g: ls == g), ("_rest", lambda g: ls != g)):
            bm, bv = np.zeros((k, G)), np.zeros((k, G))
            for g in range(k):
                part = xs[sel(g)]
                cnt = part.shape[0]
                if cnt:
                    bm[g] = (m + 2) * EPS * np.abs(part).sum(axis=0) / cnt
                if cnt >= 2:
                    d = part - ref["means" + side][g]
                    bv[g] = ((m + 6) * EPS * (d * d).sum(axis=0) + cnt * bm[g] ** 2) / (cnt - 1)
            dmean[side], dvar[side] = bm, bv
            for key, b in (("means", bm), ("vars", bv)):
                got, want = dev[key + side], ref[key + side]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (what, key + side)
                err = np.abs(got - want)
                assert not (err > b).any(), (what, key + side, float(np.nanmax(err)))
                worst[key + side] = ratio(err, b)
        z = ref["full_scores"]
        got_s, got_p, got_nl = dev["full_scores"], dev["full_pvals"], dev["full_neglog10_pvals"]
        if method == "wilcoxon":
            b_s = 8 * EPS * np.abs(z)
            b_prel = (8 * z * z + consts["c0"]) * EPS
            b_p = b_prel * ref["full_pvals"] + 1e-290
            b_nl = b_prel / LN10 + consts["nl_w"] * np.abs(ref["full_neglog10_pvals"])
        else:
            ng = ref["group_sizes"].astype(np.float64)[:, None]
            nr = ng if method == "t-test_overestim_var" else ref["n_valid"] - ng
            a, b = ref["vars"] / ng, ref["vars_rest"] / nr
            den = np.sqrt(a + b)
            dsum = dvar[""] / ng + dvar["_rest"] / nr
            b_s = (dmean[""] + dmean["_rest"]) / den + np.abs(z) * (0.5 * dsum / (a + b) + 8 * EPS)
            nu = ((a + b) * (a + b)) / ((a * a) / (ng - 1.0) + (b * b) / (nr - 1.0))
            da, db = dvar[""] / ng, dvar["_rest"] / nr
            b_nu = nu * (2 * dsum / (a + b) + 2 * (a * da / (ng - 1.0) + b * db / (nr - 1.0)) /
                         ((a * a) / (ng - 1.0) + (b * b) / (nr - 1.0)) + 16 * EPS)
            bad = np.isnan(z) | np.isnan(nu) | np.isnan(b_s)
            zz, nn = np.where(bad, 0.0, z), np.where(bad, 1.0, nu)
            bs, bn = np.where(bad, 0.0, b_s), np.where(bad, 0.0, b_nu)
            p0, nl0 = mr.student_p(zz, nn)
            b_p, b_nl = consts["c0t"] * EPS * p0 + 1e-290, consts["nl_t"] * np.abs(nl0) + consts["c0t"] * EPS / LN10
            for dz, dn in ((bs, 0), (-bs, 0), (0, bn), (0, -bn)):
                p1, nl1 = mr.student_p(zz + dz, np.maximum(nn + dn, 1e-3))
                b_p, b_nl = b_p + np.abs(p1 - p0), b_nl + np.where(np.isfinite(nl0), np.abs(nl1 - nl0), 0.0)
            b_s = np.where(bad, 0.0, b_s)
        for key, got, want, bound in (("scores", got_s, z, b_s), ("pvals", got_p, ref["full_pvals"], b_p),
                                      ("neglog10_pvals", got_nl, ref["full_neglog10_pvals"], b_nl)):
            same_inf = np.isinf(want) & (got == want)
            err = np.where(same_inf, 0.0, np.abs(got - want))
            assert not np.isnan(got).any() and not (err > bound).any(), (what, key, float(np.nanmax(err / bound)))
            worst[key] = ratio(err, bound)
        rel_p = np.where(ref["full_pvals"] > 1e-250, b_p / ref["full_pvals"], 0.0)      # (an underflowed p moves nothing)
        b_adj = rel_p.max(axis=1, keepdims=True) * ref["full_pvals_adj"] + 1e-290
        err = np.abs(dev["full_pvals_adj"] - ref["full_pvals_adj"])
        assert not (err > b_adj).any(), (what, "pvals_adj", float((err / b_adj).max()))
        worst["pvals_adj"] = ratio(err, b_adj)
        ex = np.exp(ref["means"]), np.exp(ref["means_rest"])
        b_l = (ex[0] * dmean[""] / np.abs(np.expm1(ref["means"]) + 1e-9) +
               ex[1] * dmean["_rest"] / np.abs(np.expm1(ref["means_rest"]) + 1e-9)) / np.log(2.0) + \
            16 * EPS * (np.abs(ref["full_logfoldchanges"]) + 1)
        got, want = dev["full_logfoldchanges"], ref["full_logfoldchanges"]
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
        assert not (np.abs(got - want)[fin] > b_l[fin]).any(), (what, "logfoldchanges")
        worst["logfoldchanges"] = ratio(np.abs(got - want)[fin], b_l[fin])
    # the order: the stable order of the device's own scores; the ordered columns are gathers of the full ones
    v = np.abs(got_s) if rankby_abs else got_s
    top = dev["names"].shape[1]
    assert top == (G if n_genes is None else min(n_genes, G))
    order = np.stack([np.argsort(-v[g], kind="stable")[:top] for g in range(k)]) if k else np.zeros((0, top), np.int64)
    assert dev["names"].dtype == np.int64 and np.array_equal(dev["names"], order), (what, "names")
    for key in ("scores", "pvals", "pvals_adj", "neglog10_pvals", "logfoldchanges"):
        assert np.array_equal(dev[key], np.take_along_axis(dev["full_" + key], order, axis=1), equal_nan=True), (what, key)
    print(f"{what} {method} tc={tie_correct} n={n} G={G} k={k}: err/bound " +
          " ".join(f"{a}={b:.2g}" for a, b in worst.items()))
    return ref


def run_one(x, labels, k, consts, what, on_device=True, **kw):
    from mclstexp_amd import markers
    res = markers.rank_genes_groups(padded(x) if on_device else x, labels, None, k, **kw)
    assert len(res) == 1
    return res[0], check_slide(res[0], x, labels, k, consts, what=what, **kw)


def same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        va, vb = np.asarray(a[key]), np.asarray(b[key])
        assert va.shape == vb.shape and va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), key


# --------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 257, 1000])
def test_slide_sizes_around_the_wave_and_the_workgroup(consts, n):
    k = min(3, n)
    for i, (method, tc, dtype, kind) in enumerate((("wilcoxon", True, np.float32, "grid"), ("wilcoxon", False, np.float64, "cont"),
                                                   ("t-test", False, np.float32, "counts"),
                                                   ("t-test_overestim_var", False, np.float64, "cont"))):
        x, labels = mr.make_case(n, 7, k, seed=100 + n + i, kind=kind, dtype=dtype)
        run_one(x, labels, k, consts, f"sizes[{n}]", method=method, tie_correct=tc)


def test_largest_slide_and_one_row_more(consts):
    from mclstexp_amd import markers
    x, labels = mr.make_case(16384, 8, 3, seed=5, kind="zeros", dtype=np.float64)
    run_one(x, labels, 3, consts, "n=16384 fp64", tie_correct=True)
    run_one(x.astype(np.float32), labels, 3, consts, "n=16384 fp32", method="t-test")
    with pytest.raises(ValueError, match="16384"):
        markers.rank_genes_groups(np.zeros((16385, 8), np.float32), np.zeros(16385, np.int32), None, 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties(consts, dtype):
    n = 1500                                           # P = 2048: not a power of two, several columns per workgroup
    rng = np.random.default_rng(9)
    x = np.empty((n, 6), dtype=dtype)
    x[:, 0] = 1.25                                     # all equal: score 0, p 1, c = 0 with tie_correct
    x[:, 1] = rng.gamma(2.0, 1.0, n) * (rng.random(n) < 0.1)          # 90 % zeros
    x[:, 2] = rng.poisson(2.0, n)                      # integer counts
    x[:, 3] = np.where(rng.random(n) < 0.5, -0.0, 0.0)                # -0.0 beside +0.0 ...
    x[::7, 3] = rng.normal(size=x[::7, 3].shape)                      # ... between negative and positive values
    run = np.concatenate([np.arange(40) - 100.0, np.full(n - 80, 0.5), np.arange(40) + 100.0])
    x[:, 4] = rng.permutation(run)                     # one tie run across every internal tile boundary of the sort
    x[:, 5] = rng.normal(size=n)                       # no ties
    labels = rng.integers(0, 4, n).astype(np.int32)
    for tc in (False, True):
        dev, ref = run_one(x, labels, 4, consts, f"ties[{np.dtype(dtype).name}]", tie_correct=tc)
        assert (dev["full_scores"][:, 0] == 0).all() and (dev["full_pvals"][:, 0] == 1).all()
        assert dev["tie_terms"][0] == n ** 3 - n and dev["tie_terms"][5] == 0
        assert dev["tie_terms"][4] == (n - 80) ** 3 - (n - 80)
    run_one(x, labels, 4, consts, f"ties[{np.dtype(dtype).name}]", method="t-test")


def test_groups(consts):
    from mclstexp_amd import markers
    x, labels = mr.make_case(300, 7, 2, seed=21, kind="grid", dtype=np.float32)
    for method in ("wilcoxon", "t-test"):
        dev, _ = run_one(x, np.zeros(300, np.int32), 1, consts, "k=1", method=method)       # empty rest
        assert (dev["full_scores"] == 0).all() and (dev["full_pvals"] == 1).all() and (dev["full_pvals_adj"] == 1).all()
        run_one(x, labels, 2, consts, "k=2", method=method)
    x37, l37 = mr.make_case(400, 40, 37, seed=22, kind="cont", dtype=np.float64)
    run_one(x37, l37, 37, consts, "k=37", tie_correct=True)
    run_one(x37, l37, 37, consts, "k=37", method="t-test", n_genes=5, rankby_abs=True)
    lone = labels.copy()
    lone[lone == 2] = 0
    lone[17] = 2                                        # a group of one spot; label 3 is carried by nobody
    for method in ("wilcoxon", "t-test", "t-test_overestim_var"):
        dev, _ = run_one(x, lone, 5, consts, "one spot / nobody", method=method)
        assert dev["group_sizes"].tolist()[2:] == [1, 0, 0]
        assert (dev["full_scores"][3:] == 0).all() and (dev["full_pvals"][3:] == 1).all()
        if method != "wilcoxon":
            assert (dev["full_scores"][2] == 0).all() and (dev["full_pvals"][2] == 1).all()
    # rows labelled -1: the slide with those rows removed, bit for bit
    xd, ld_ = mr.make_case(257, 7, 3, seed=23, kind="grid", dtype=np.float32, drop=0.3)
    keep = ld_ >= 0
    assert 0 < keep.sum() < 257
    for method in ("wilcoxon", "t-test"):
        a = markers.rank_genes_groups(padded(xd), ld_, None, 3, method=method, tie_correct=True)[0]
        b = markers.rank_genes_groups(padded(xd[keep]), ld_[keep], None, 3, method=method, tie_correct=True)[0]
        same(a, b)
        check_slide(a, xd, ld_, 3, consts, method=method, tie_correct=True, what="dropped rows")


@pytest.mark.parametrize("G", [1, 7, 785])
def test_gene_counts_with_a_padded_row_stride(consts, G):
    x, labels = mr.make_case(333, G, 6, seed=30 + G, kind="grid", dtype=np.float32)
    run_one(x, labels, 6, consts, f"G={G}", tie_correct=True)
    run_one(x, labels, 6, consts, f"G={G}", method="t-test", n_genes=min(G, 10))
    run_one(x.astype(np.float64), labels, 6, consts, f"G={G} host fp64", on_device=False, rankby_abs=True)


def test_a_batch_is_its_slides_alone_and_runs_repeat(consts):
    from mclstexp_amd import markers
    shapes = [(64, 2), (700, 6), (2, 1), (1025, 37)]
    parts = [mr.make_case(n, 33, k, seed=40 + i, kind=("grid", "zeros", "cont", "counts")[i], dtype=np.float32, drop=0.05 * i)
             for i, (n, k) in enumerate(shapes)]
    x = np.concatenate([p[0] for p in parts])
    labels = np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum([n for n, _ in shapes])])
    ks = [k for _, k in shapes]
    for method in ("wilcoxon", "t-test"):
        batch = markers.rank_genes_groups(padded(x), labels, off, ks, method=method, tie_correct=True)
        again = markers.rank_genes_groups(padded(x), labels, off, ks, method=method, tie_correct=True)
        for s, (xs, ls) in enumerate(parts):
            alone = markers.rank_genes_groups(padded(xs), ls, None, ks[s], method=method, tie_correct=True)[0]
            same(batch[s], alone)
            same(batch[s], again[s])
            check_slide(batch[s], xs, ls, ks[s], consts, method=method, tie_correct=True, what=f"batch[{s}]")


def test_bad_values_and_labels_raise():
    from mclstexp_amd import markers
    x, labels = mr.make_case(100, 5, 3, seed=50, kind="cont", dtype=np.float32)
    for v in (np.nan, np.inf, -np.inf):
        bad = x.copy()
        bad[77, 3] = v
        with pytest.raises(ValueError, match="non-finite"):
            markers.rank_genes_groups(bad, labels, None, 3)
    bad = x.copy()
    bad[5, 0] = np.nan
    dropped = labels.copy()
    dropped[5] = -1
    markers.rank_genes_groups(bad, dropped, None, 3)                    # a dropped row is not looked at
    for v in (3, 255, -2):
        lab = labels.copy()
        lab[9] = v
        with pytest.raises(ValueError, match="group ids outside"):
            markers.rank_genes_groups(x, lab, None, 3)
    two = np.concatenate([x, x])
    lab = np.concatenate([labels, np.minimum(labels, 1)])
    lab[150] = 2                                                         # fine in slide 0, beyond k in slide 1
    with pytest.raises(ValueError, match="slide 1"):
        markers.rank_genes_groups(two, lab, [0, 100, 200], [3, 2])


@pytest.mark.parametrize("name", sorted(SCIPY_CASES))
def test_scipy_fixtures_values_and_order(golden, consts, name):
    kw = SCIPY_CASES[name]
    x, labels = mr.make_case(**kw)
    k = kw["k"]
    dev, _ = run_one(x, labels, k, consts, name)
    z = golden[f"{name}.z"]
    assert not (np.abs(dev["full_scores"] - z) > 8 * EPS * np.abs(z)).any()
    assert np.array_equal(dev["names"], golden[f"{name}.order"])
    ls = labels[labels >= 0]
    assert np.array_equal(dev["rank_sums2"], np.stack([golden[f"{name}.rank2"][ls == g].sum(axis=0) for g in range(k)]))
    assert not (np.abs(dev["full_pvals"] - golden[f"{name}.p"]) > (8 * z * z + consts["c0"]) * EPS * golden[f"{name}.p"] + 1e-290).any()
    tc, _ = run_one(x, labels, k, consts, name, tie_correct=True)
    assert not (np.abs(tc["full_pvals"] - golden[f"{name}.p_tc"]) >
                (8 * tc["full_scores"] ** 2 + consts["c0"]) * EPS * golden[f"{name}.p_tc"] + 1e-290).any()
    t, _ = run_one(x, labels, k, consts, name, method="t-test")
    assert np.array_equal(t["names"], golden[f"{name}.order_t"])


def test_log_space_where_p_underflows(golden, consts):
    name, kw = next(iter(MP_CASES.items()))
    x, labels = mr.make_case(**kw)
    w, _ = run_one(x, labels, kw["k"], consts, name)
    assert (w["full_pvals"] == 0).any() and np.isfinite(w["full_neglog10_pvals"]).all()
    assert np.array_equal(w["full_scores"] == 0, golden[f"{name}.z"] == 0)
    z = golden[f"{name}.z"]
    assert not (np.abs(w["full_neglog10_pvals"] - golden[f"{name}.nl_w"]) >
                (8 * z * z + consts["c0"]) * EPS / LN10 + consts["nl_w"] * golden[f"{name}.nl_w"]).any()
    t, _ = run_one(x, labels, kw["k"], consts, name, method="t-test")
    assert np.isfinite(t["full_neglog10_pvals"]).all() and t["full_neglog10_pvals"].max() > 100


def test_recovery_and_cli_end_to_end(tmp_path, consts):
    from mclstexp_amd import markers
    shapes = [(120, 3), (90, 2)]
    trues, preds, labs, names = [], [], [], [np.array(["a", "b", "undetermined", "c"]), np.array(["x", "y"])]
    rng = np.random.default_rng(60)
    for i, (n, k) in enumerate(shapes):
        x, l = mr.make_case(n, 30, k, seed=60 + i, kind="cont", dtype=np.float32)
        trues.append(x)
        preds.append((x + 0.3 * rng.gamma(2.0, 0.5, x.shape)).astype(np.float32))
        code = l.copy()
        if i == 0:
            code[code == 2] = 3
            code[::11] = 2                              # some undetermined spots
        labs.append(names[i][code])
    rec = markers.marker_recovery(preds, trues, labs, n_top=8)
    for i, (n, k) in enumerate(shapes):
        codes, ks, cats = markers.encode_slides([labs[i]])
        assert int(ks[0]) == k
        o, j = mr.marker_recovery(preds[i], trues[i], codes, k, n_top=8)
        assert np.array_equal(rec["overlap"][i], o) and np.array_equal(rec["jaccard"][i], j)
        check_slide(rec["pred"][i] | {}, preds[i], codes, k, consts, n_genes=8, what=f"recovery[{i}]")
    assert rec["mean_jaccard"] == float(np.concatenate(rec["jaccard"]).mean()) and 0 < rec["mean_jaccard"] <= 1
    assert markers.top_markers(rec["true"], 0, 3).tolist() == np.unique(rec["true"][0]["names"][:, :3]).tolist()
    args = []
    for flag, arrs in (("--pred", preds), ("--true", trues), ("--labels", labs)):
        args.append(flag)
        for i, a in enumerate(arrs):
            path = str(tmp_path / f"{flag[2:]}{i}.npy")
            np.save(path, a.T if a.ndim == 2 else a)
            args.append(path)
    out = subprocess.run([sys.executable, "-m", "mclstexp_amd.markers", *args, "--top", "8", "--out_dir", str(tmp_path / "out")],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 5 + 5 + 1 and lines[0].startswith("slide 0 group a (n = ")
    assert lines[-1] == f"mean overlap {rec['mean_overlap']:.4f} / 8, mean Jaccard {rec['mean_jaccard']:.4f}"
    for i in range(2):
        z = np.load(str(tmp_path / "out" / str(i) / markers.OUT_FILE))
        full = markers.marker_slides([preds[i]], [labs[i]])[0]
        assert np.array_equal(z["names"], full["names"]) and np.array_equal(z["names"][:, :8], rec["pred"][i]["names"])
        assert z["categories"].tolist() == [c for c in names[i].tolist() if c != "undetermined"]
