"""GPU: mclstexp_amd.ligrec (csrc/ligrec.hip) against the numpy restatement tests/ligrec_reference.py, which
tests/test_ligrec_host.py pins to pandas ``groupby`` and ``scipy.stats.false_discovery_control``.

Bounds.  On the QUANTISED data (multiples of 2^-12 below 16: every sum of at most 16384 values is exact in fp64 in any order,
and +, / are correctly rounded on both sides) everything must be ``array_equal`` to the restatement: order, sizes, nnz,
defined, count, pvalues, means, group_means and the rest.  On unquantised data a group sum of m spots travels through at most
L = ceil(m / 64) + 6 additions of the stated order (its lane's chain, six tree levels) and one division; device and
restatement both carry that error, hence the leading 2: group_means within 2 (L + 2) eps relative, and means = (m1 + m2) / 2
(one more addition of non-negative numbers, an exact halving) within the same bound with L the slide's longest chain.
Values are >= 0: no cancellation.  Derived, not tuned; eps = 2^-52.

Every kernel of the hot path is run: test_every_column_count_and_groups_beyond_one_pass puts slides on both sides of every
boundary of mcl_ligrec_columns (C = 8, 4, 2, 1) into one call, with a partial last column tile and groups of 256, 257, 513 and
thousands of kept spots (a wave's gather loop takes 256 positions a trip).

Measured on MI355X, largest error / bound over the slides of test_unquantised_within_the_derived_bound (printed with -s):
group_means 0, means 0 -- the restatement follows the kernel's order, so the sums came out bit-equal.

The planted signal of test_planted_signal (PLANTED_SEED = 1, 200 spots, P = 200): the restatement gives p(A->B, 0->1) = 0.0
and p(A->B, 1->0) = 1.0.  The spot-shuffled prediction of test_recovery_and_cli (slides make_planted(4) and
make_planted(5, n=150), SHUFFLE_SEED = 1, P = 100): the restatement gives Jaccard 1.0 of the measured matrices against
themselves (4 significant entries a slide) and 0.0 for the shuffled ones (Pearson 0.657 and 0.654)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ligrec_reference as lr
from mclstexp_amd import ligrec as lg

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 64
SEED = 3
PLANTED_SEED = 1
SHUFFLE_SEED = 1
EXACT = ("means", "pvalues", "pvalues_adj", "defined", "count", "group_means", "group_frac", "nnz", "expressed", "sizes",
         "order", "used_genes", "interactions")
# (n, K, empty group, group of one spot, share labelled -1): two groups of one spot; K = 1 with all 257 spots kept in one
# group (one past the 256 gather slots of a wave's pass); more than 1024 rows
BATCH = [(2, 2, None, None, 0.1), (37, 2, None, None, 0.1), (143, 7, 3, 6, 0.1), (257, 1, None, None, 0.0),
         (1025, 7, None, 2, 0.1)]
# The column counts.  (n, K, share labelled -1) -> kept spots: 256, 257 and 513 in ONE group (the second and third trip of a
# wave's gather loop and their tails), then both sides of every boundary of mcl_ligrec_columns: 2432 | 2433 (C = 8 | 4),
# 4864 | 4865 (4 | 2), 9728 | 9729 (2 | 1), with groups far larger than 256 and some spots dropped
COLUMN_SLIDES = [(256, 1, 0.0), (257, 1, 0.0), (513, 1, 0.0), (2432, 2, 0.0), (2703, 3, 0.1), (4864, 2, 0.0), (5406, 2, 0.1),
                 (9728, 3, 0.0), (9729, 3, 0.0)]
COLUMN_KEPT = [256, 257, 513, 2432, 2433, 4864, 4865, 9728, 9729]
COLUMN_C = [8, 8, 8, 8, 4, 4, 2, 2, 1]
# 9 distinct genes: no multiple of 2, 4 or 8, so the last column tile of every kernel is a partial one
COLUMN_INTERACTIONS = [(0, 1), (2, 3), (4, 4), (5, 11), (10, 6)]


def padded(x, extra=5):
    """x as a device view with a row stride larger than its width."""
    wide = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), dtype=torch.from_numpy(x[:1]).dtype, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def make_batch(quantised):
    slides = [lr.make_slide(n, K, 10 + i, quantised=quantised, empty=e, single=s, drop=d)
              for i, (n, K, e, s, d) in enumerate(BATCH)]
    assert int((slides[3][1] >= 0).sum()) == 257
    x = np.concatenate([s[0] for s in slides])
    labels = np.concatenate([s[1] for s in slides])
    off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in slides])]).astype(np.int64)
    return slides, x, labels, off, np.array([b[1] for b in BATCH])


def same(got, want, what):
    for key in EXACT:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, key)
    assert (got["n"], got["k"], got["n_perms"]) == (want["n"], want["k"], want["n_perms"]), what


@pytest.fixture(scope="module")
def quantised():
    """The quantised batch and the restatement of every slide per threshold, computed once."""
    slides, x, labels, off, ks = make_batch(True)
    refs = {}

    def ref(threshold):
        if threshold not in refs:
            refs[threshold] = [lr.ligrec(sx, sl, lr.INTERACTIONS, K, n_perms=P, seed=SEED, threshold=threshold)
                               for (sx, sl), K in zip(slides, ks)]
        return refs[threshold]
    return slides, x, labels, off, ks, ref


@pytest.mark.parametrize("threshold,dtype,strided", [(0.1, np.float64, False), (0.1, np.float32, True),
                                                     (0.0, np.float64, True), (1.0, np.float32, False)])
def test_exact_on_quantised_data(quantised, threshold, dtype, strided):
    slides, x, labels, off, ks, ref = quantised
    xs = x.astype(dtype)
    assert np.array_equal(xs.astype(np.float64), x)                      # (the quantised values are exact in fp32)
    res = lg.ligrec(padded(xs) if strided else xs, labels, lr.INTERACTIONS, off, ks, n_perms=P, seed=SEED,
                    threshold=threshold, return_permutations=True)
    want = ref(threshold)
    assert len(res) == len(BATCH)
    for s, (r, w) in enumerate(zip(res, want)):
        same(r, w, (s, threshold))
        assert np.array_equal(r["permutations"], w["permutations"]), s
        assert r["means"].shape == (9, ks[s], ks[s])
    assert res[0]["sizes"].tolist() == [1, 1] and res[2]["sizes"][3] == 0 and res[2]["sizes"][6] == 1
    assert any(np.isfinite(r["pvalues"]).any() for r in res)
    if threshold == 0.1:                                                  # the gene expressed in exactly 0.1 * size spots
        u10 = int(np.searchsorted(res[1]["used_genes"], 10))
        assert res[1]["nnz"][0, u10] == 2 and res[1]["sizes"][0] == 20 and res[1]["expressed"][0, u10]


def test_policies_and_axes_on_quantised_data(quantised):
    slides, x, labels, off, ks, ref = quantised
    for policy, axis in (("all", "interactions"), ("min", None)):
        res = lg.ligrec(x, labels, lr.INTERACTIONS, off, ks, n_perms=8, seed=SEED, corr_axis=axis, complex_policy=policy)
        for s, ((sx, sl), K) in enumerate(zip(slides, ks)):
            same(res[s], lr.ligrec(sx, sl, lr.INTERACTIONS, K, n_perms=8, seed=SEED, corr_axis=axis, complex_policy=policy),
                 (s, policy))


def test_identity_replay_reproduces_the_observed_path():
    slides, x, labels, off, ks = make_batch(False)
    perms = [np.tile(np.arange(int((sl >= 0).sum())), (3, 1)) for _, sl in slides]
    res = lg.ligrec(x, labels, lr.INTERACTIONS, off, ks, permutations=perms)
    for r in res:
        assert r["n_perms"] == 3
        finite = np.isfinite(r["means"])
        assert finite.any() and (r["count"][finite] == 3).all()
        assert (r["count"][~finite] == 0).all()
        assert (r["pvalues"][r["defined"]] == 1.0).all()


def test_unquantised_within_the_derived_bound():
    slides, x, labels, off, ks = make_batch(False)
    res = lg.ligrec(x, labels, lr.INTERACTIONS, off, ks, n_perms=0)
    worst = {"group_means": 0.0, "means": 0.0}
    for s, ((sx, sl), K) in enumerate(zip(slides, ks)):
        w = lr.ligrec(sx, sl, lr.INTERACTIONS, K, n_perms=0)
        chains = np.array([lr.chain(int(m)) for m in w["sizes"]], dtype=np.float64)
        bounds = {"group_means": 2 * (chains[:, None] + 2) * EPS * np.abs(w["group_means"]),
                  "means": 2 * (chains.max() + 2) * EPS * np.abs(w["means"])}
        for key, bound in bounds.items():
            got, want = res[s][key], w[key]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (s, key)
            ok = ~np.isnan(want)
            err = np.abs(got[ok] - want[ok])
            assert not (err > bound[ok]).any(), (s, key)
            with np.errstate(all="ignore"):
                ratio = np.where(err == 0, 0.0, err / bound[ok])
            worst[key] = max(worst[key], float(ratio.max()) if ratio.size else 0.0)
        for key in ("order", "sizes", "nnz", "defined", "expressed"):
            assert np.array_equal(res[s][key], w[key]), (s, key)
    print("largest error / bound:", worst)


def test_255_groups():
    x, labels = lr.make_slide(300, 255, 21)
    assert np.unique(labels).size == 255
    res = lg.ligrec(x, labels, lr.INTERACTIONS, k=255, n_perms=2, seed=SEED)
    same(res[0], lr.ligrec(x, labels, lr.INTERACTIONS, 255, n_perms=2, seed=SEED), "K = 255")


def test_largest_slide_one_column_per_workgroup():
    x, labels = lr.make_slide(16384, 3, 22, drop=0.0)
    assert lr.columns(int((labels >= 0).sum())) == 1
    inter = [(0, 1)]
    res = lg.ligrec(x, labels, inter, n_perms=3, seed=SEED, return_permutations=True)
    w = lr.ligrec(x, labels, inter, 3, n_perms=3, seed=SEED)
    same(res[0], w, "n = 16384")
    assert res[0]["used_genes"].tolist() == [0, 1] and np.array_equal(res[0]["permutations"], w["permutations"])


def test_every_column_count_and_groups_beyond_one_pass():
    """One call whose slides need all four kernels (column_mask has four bits; every launch skips the other kernels'
    slides), with 9 used genes (a partial last tile under C = 2, 4 and 8) and groups of 256, 257, 513 and thousands of
    spots: exact on quantised data.  A C = 4 and a C = 2 slide alone are bit-identical to themselves in the batch."""
    slides = [lr.make_slide(n, K, 40 + i, drop=d) for i, (n, K, d) in enumerate(COLUMN_SLIDES)]
    kept = [int((sl >= 0).sum()) for _, sl in slides]
    assert kept == COLUMN_KEPT and [lr.columns(n) for n in kept] == COLUMN_C
    x = np.concatenate([s[0] for s in slides])
    labels = np.concatenate([s[1] for s in slides])
    off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in slides])]).astype(np.int64)
    ks = np.array([c[1] for c in COLUMN_SLIDES])
    kw = dict(n_perms=3, seed=SEED)
    res = lg.ligrec(padded(x.astype(np.float32)), labels, COLUMN_INTERACTIONS, off, ks, return_permutations=True, **kw)
    for s, ((sx, sl), K) in enumerate(zip(slides, ks)):
        w = lr.ligrec(sx, sl, COLUMN_INTERACTIONS, int(K), **kw)
        assert w["used_genes"].size == 9 and w["sizes"].max() >= 256
        same(res[s], w, ("columns", s))
        assert np.array_equal(res[s]["permutations"], w["permutations"]), s
    for s in (1, 4, 6):
        alone = lg.ligrec(slides[s][0], slides[s][1], COLUMN_INTERACTIONS, k=int(ks[s]), **kw)[0]
        same(res[s], alone, ("alone", s))
    # the device-label path launches every kernel (it cannot know the kept counts): the same results
    dev = lg.ligrec(x, torch.from_numpy(labels.astype(np.int32)).cuda(), COLUMN_INTERACTIONS, off, ks, **kw)
    for a, b in zip(res, dev):
        same(a, b, "device labels")


def test_batch_against_alone_and_run_to_run():
    slides, x, labels, off, ks = make_batch(False)
    kw = dict(n_perms=16, seed=SEED)
    batch = lg.ligrec(x, labels, lr.INTERACTIONS, off, ks, **kw)
    again = lg.ligrec(x, labels, lr.INTERACTIONS, off, ks, **kw)
    for s in (2, 4):
        alone = lg.ligrec(slides[s][0], slides[s][1], lr.INTERACTIONS, k=int(ks[s]), **kw)[0]
        same(batch[s], alone, ("alone", s))
    for a, b in zip(batch, again):
        same(a, b, "run to run")


def test_bad_input_raises_and_names_the_slide():
    slides, x, labels, off, ks = make_batch(True)
    first = int(off[2])
    lab = labels.copy()
    lab[first + 5] = 7                                                   # slide 2 has k = 7: ids 0 .. 6
    with pytest.raises(ValueError, match=r"labels: slide 2 holds 1 group ids outside"):
        lg.ligrec(x, lab, lr.INTERACTIONS, off, ks, n_perms=2)
    lab = labels.copy()
    lab[int(off[1]) + 1] = -2
    with pytest.raises(ValueError, match=r"labels: slide 1 holds 1 group ids outside"):
        lg.ligrec(x, lab, lr.INTERACTIONS, off, ks, n_perms=2)
    kept = np.flatnonzero(labels[first:int(off[3])] >= 0)
    xb = x.copy()
    xb[first + kept[3], 4] = np.nan
    with pytest.raises(ValueError, match=r"x: slide 2 holds 1 non-finite values"):
        lg.ligrec(xb, labels, lr.INTERACTIONS, off, ks, n_perms=2)
    xb = x.copy()
    xb[first + kept[0], 0] = -0.5
    with pytest.raises(ValueError, match=r"x: slide 2 holds 1 negative values"):
        lg.ligrec(xb, labels, lr.INTERACTIONS, off, ks, n_perms=2)
    # a dropped spot and an unused gene are not part of the analysis
    xb = x.copy()
    xb[first + np.flatnonzero(labels[first:int(off[3])] < 0)[0], 0] = np.nan
    assert len(lg.ligrec(xb, labels, [(0, 1)], off, ks, n_perms=2)) == len(BATCH)
    # the library refuses what lies beyond its limits without a launch
    from mclstexp_amd._lib import call
    assert call("mcl_ligrec_columns", 16384) == 1 and call("mcl_ligrec_chunk", 32, 6, 300, 1000) == 582
    with pytest.raises(RuntimeError, match="rejected"):
        call("mcl_ligrec_chunk", 1, 256, 4, 10)


def test_planted_signal():
    x, labels = lr.make_planted(PLANTED_SEED)
    r = lg.ligrec(x, labels, lr.PLANTED, n_perms=200, seed=PLANTED_SEED)[0]
    assert r["n"] == 200 and r["k"] == 2
    assert r["pvalues"][0, 0, 1] <= 0.01 and r["pvalues"][0, 1, 0] >= 0.9
    w = lr.ligrec(x, labels, lr.PLANTED, 2, n_perms=200, seed=PLANTED_SEED)
    same(r, w, "planted")
    top = lg.top_interactions([r], 0, 4)
    assert np.array_equal(top, lr.top_interactions(w, 4))
    assert sorted(map(tuple, top.tolist())) == [(0, 0, 1), (1, 1, 0), (5, 0, 0), (6, 1, 1)]      # A and B where they are high


def test_recovery_and_cli(tmp_path):
    trues = [lr.make_planted(4), lr.make_planted(5, n=150)]
    mats, labs = [t[0] for t in trues], [t[1] for t in trues]
    rec = lg.interaction_recovery(mats, mats, labs, lr.PLANTED, n_perms=100, seed=0)
    assert np.all(np.abs(rec["pearson"] - 1.0) <= 4 * EPS) and (rec["jaccard"] == 1.0).all()      # (r: one sqrt, one division)
    assert rec["overlap"].tolist() == [4, 4] and rec["mean_jaccard"] == 1.0 and rec["mean_recall"] == 1.0
    rng = np.random.default_rng(SHUFFLE_SEED)
    shuffled = [m[rng.permutation(m.shape[0])] for m in mats]
    low = lg.interaction_recovery(shuffled, mats, labs, lr.PLANTED, n_perms=100, seed=0)
    assert (low["jaccard"] < rec["jaccard"]).all() and low["mean_jaccard"] == 0.0 and (low["pearson"] < 0.9).all()
    for s in range(2):
        want = lr.recovery(lr.ligrec(shuffled[s], labs[s], lr.PLANTED, 2, n_perms=100, seed=0),
                           lr.ligrec(mats[s], labs[s], lr.PLANTED, 2, n_perms=100, seed=0))
        assert abs(low["pearson"][s] - want[0]) <= 64 * EPS and low["overlap"][s] == want[1]
    # the CLI in a fresh process: string annotations with undetermined spots, gene names, a complex, a pair outside the panel
    genes = np.array([f"G{j}" for j in range(8)])
    pred_files, true_files, label_files = [], [], []
    for s, (m, lab) in enumerate(zip(mats, labs)):
        names = np.where(lab == 0, "tumour", "stroma").astype(object)
        names[:3] = "undetermined"
        for kind, arr, files in (("pred", shuffled[s], pred_files), ("true", m, true_files)):
            files.append(str(tmp_path / f"{kind}{s}.npy"))
            np.save(files[-1], np.ascontiguousarray(arr.T))
        label_files.append(str(tmp_path / f"labels{s}.npy"))
        np.save(label_files[-1], names, allow_pickle=True)
    np.save(tmp_path / "genes.npy", genes)
    (tmp_path / "pairs.tsv").write_text("source\ttarget\nG0\tG1\nG1\tG0\nG2_G3\tG4\nG0\tNOPE\nG0\tG1\n")
    out_dir = tmp_path / "out"
    cmd = [sys.executable, "-m", "mclstexp_amd.ligrec", "--pred", *pred_files, "--true", *true_files, "--labels", *label_files,
           "--pairs", str(tmp_path / "pairs.tsv"), "--genes", str(tmp_path / "genes.npy"), "--n_perms", "50", "--seed", "2",
           "--top", "3", "--out_dir", str(out_dir)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "3 interactions (1 pairs with a gene outside the panel and 1 duplicates dropped)" in run.stdout
    assert "slide 1 n = 147 k = 2 perms = 50" in run.stdout and "recovery (alpha 0.05, adjusted)" in run.stdout
    for s in range(2):
        z = np.load(out_dir / str(s) / lg.OUT_FILE, allow_pickle=True)
        lab = np.where(np.arange(labs[s].size) < 3, -1, np.where(labs[s] == 0, 1, 0))      # sorted: stroma 0, tumour 1
        w = lr.ligrec(shuffled[s], lab, [(0, 1), (1, 0), ((2, 3), 4)], 2, n_perms=50, seed=2)
        assert z["categories"].tolist() == ["stroma", "tumour"]
        for key in ("means", "pvalues", "pvalues_adj", "count", "defined", "sizes", "interactions"):
            assert np.array_equal(z[key], w[key], equal_nan=z[key].dtype.kind == "f"), (s, key)
