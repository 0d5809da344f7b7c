"""GPU: mclstexp_amd.nmf against the numpy restatement tests/nmf_reference.py and scikit-learn's recorded results
(tests/golden/nmf.npz; the inputs are regenerated from their seeds).

One iteration is bounded element by element in relative terms: every sum is over non-negative terms, so the bound is derived
(``nmf_reference.step_bounds``), not fitted.  Thirty iterations are held to 8 x the restatement's own
re-ordering spread, which the generator stored per case; the margin is over the reference's spread, never the device's.
The stop rule, bit identity (segment alone / stacked, start alone / beside others, run to run, fp32 / its fp64
up-conversion), the monotone objective, ``transform``, the input checks and ``program_recovery`` follow."""
import os

import numpy as np
import pytest

import nmf_reference as nr
from conftest import GOLDEN_DIR
from mclstexp_amd import nmf

pytestmark = pytest.mark.gpu
TAG = {"frobenius": "f", "kullback-leibler": "kl"}
ALL = nr.CASES + (nr.STACKED,)
PAIRS = [(c, loss) for c in ALL for loss in nr.LOSSES]
IDS = [f"{c[0]}-{TAG[loss]}" for c, loss in PAIRS]
MARGIN = 8.0
OFF = np.array(nr.STACKED_OFFSETS)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "nmf.npz"))


_CACHE = {}


def data(c):
    if c[0] not in _CACHE:
        _CACHE[c[0]] = nr.make_case(*c[1:])
    return _CACHE[c[0]]


def reference(c, loss, iters=nr.ITERS):
    """The restatement's (W, H) of a case after ``iters`` iterations, computed once and shared."""
    key = (c[0], loss, iters)
    if key not in _CACHE:
        _CACHE[key] = nr.fit(*data(c), loss, iters, 0.0)[:2]
    return _CACHE[key]


def device_run(c, loss, iters=nr.ITERS):
    key = ("dev", c[0], loss, iters)
    if key not in _CACHE:
        X, W0, H0 = data(c)
        _CACHE[key] = nmf.nmf(X, c[3], init=(W0, H0), beta_loss=loss, max_iter=iters, tol=0.0, return_all=True)
    return _CACHE[key]


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def same(a, b, keys=("W", "H", "err", "n_iter", "converged", "programs", "usage", "dominant")):
    for key in keys:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), key


# --------------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("case,loss", PAIRS, ids=IDS)
def test_one_iteration_element_by_element(case, loss):
    X, W0, H0 = data(case)
    rows, G, k = case[1:4]
    got = nmf.nmf(X, k, init=(W0, H0), beta_loss=loss, max_iter=1, tol=0.0)
    W1 = nr.update_w(X, W0, H0, loss)
    H1 = nr.update_h(X, W1, H0, loss)
    bw, bh = nr.step_bounds(rows, G, k, loss)
    for name, g, w, b in (("W", got["W"], W1, bw), ("H", got["H"][0], H1, bh)):
        nz = w != 0
        worst = float((np.abs(g - w)[nz] / w[nz]).max())
        print(f"{case[0]} {TAG[loss]} new {name}: worst relative error {worst / nr.EPS:.2f} eps, bound {b / nr.EPS:.0f} eps")
        assert g.shape == w.shape and g.dtype == np.float64
        assert np.array_equal(g == 0, w == 0), name                       # exact zeros stay exact zeros, and only they
        assert (np.abs(g - w) <= b * w).all(), (name, worst / nr.EPS)
    assert (got["W"][min(3, rows - 1)] == 0).all() and (got["H"][0][:, 2] == 0).all() and (got["H"][0][:, G - 1] == 0).all()
    assert got["n_iter"].tolist() == [1] and got["converged"].tolist() == [0] and got["best_start"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------- thirty steps
@pytest.mark.parametrize("case,loss", [(c, l) for c in nr.CASES for l in nr.LOSSES],
                         ids=[f"{c[0]}-{TAG[l]}" for c in nr.CASES for l in nr.LOSSES])
def test_thirty_iterations_within_the_reorder_spread(case, loss, golden):
    X, W0, H0 = data(case)
    got, (W, H) = device_run(case, loss), reference(case, loss)
    sw, sh = golden[f"{case[0]}.{TAG[loss]}.spread"]
    dw, dh = rel(got["W"], W), rel(got["H"][0], H)
    print(f"{case[0]} {TAG[loss]}: W {dw / nr.EPS:.1f} eps = {dw / sw:.2f} of the spread ({sw / nr.EPS:.1f} eps), "
          f"H {dh / nr.EPS:.1f} eps = {dh / sh:.2f} of the spread ({sh / nr.EPS:.1f} eps)")
    assert dw <= MARGIN * sw and dh <= MARGIN * sh
    stride = nr.W_STRIDE.get(case[0], 1)                                  # and against scikit-learn itself
    assert rel(got["W"][::stride], golden[f"{case[0]}.{TAG[loss]}.W"]) <= MARGIN * sw + 64 * nr.EPS
    assert rel(got["H"][0][:, ::nr.H_STRIDE.get(case[0], 1)], golden[f"{case[0]}.{TAG[loss]}.H"]) <= MARGIN * sh + 64 * nr.EPS
    want = nr.error(X, got["W"], got["H"][0], loss)
    assert abs(got["err"][0] - want) <= nr.error_bound(X, got["W"], got["H"][0], loss)
    assert (got["W"][3] == 0).all() and (got["H"][0][:, 2] == 0).all() and np.isfinite(got["W"]).all()
    prog, usage, dom = nr.normalise(got["W"], got["H"][0])
    assert (np.abs(got["programs"][0] - prog) <= 2 * case[2] * nr.EPS * prog).all()
    assert (np.abs(got["usage"] - usage) <= 2 * case[2] * nr.EPS * usage).all()
    top2 = np.sort(usage, axis=1)[:, -2:] if case[3] > 1 else np.concatenate([np.zeros_like(usage), usage], axis=1)
    clear = (top2[:, 1] - top2[:, 0] > 4 * case[2] * nr.EPS * top2[:, 1]) | (dom < 0)
    assert got["dominant"].dtype == np.int32 and np.array_equal(got["dominant"][clear], dom[clear]) and got["dominant"][3] == -1


@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_stacked_segments_spread_and_bit_identity(loss, golden):
    X, W0, H0 = data(nr.STACKED)
    k = nr.STACKED[3]
    H3 = np.stack([H0, H0, H0])
    got = nmf.nmf(X, k, offsets=OFF, init=(W0, H3), beta_loss=loss, max_iter=nr.ITERS, tol=0.0)
    assert got["H"].shape == (3, k, X.shape[1]) and got["err"].shape == (3,)
    for j in range(3):
        sl = slice(OFF[j], OFF[j + 1])
        W, H = nr.fit(X[sl], W0[sl], H0, loss, nr.ITERS, 0.0)[:2]
        sw, sh = golden[f"{nr.STACKED[0]}.{j}.{TAG[loss]}.spread"]
        dw, dh = rel(got["W"][sl], W), rel(got["H"][j], H)
        print(f"segment {j} {TAG[loss]}: W {dw / sw:.2f}, H {dh / sh:.2f} of the spread ({sw / nr.EPS:.1f}, {sh / nr.EPS:.1f} eps)")
        assert dw <= MARGIN * sw and dh <= MARGIN * sh
        alone = nmf.nmf(X[sl], k, init=(W0[sl], H0), beta_loss=loss, max_iter=nr.ITERS, tol=0.0)
        assert np.array_equal(alone["W"], got["W"][sl]) and np.array_equal(alone["H"][0], got["H"][j])
        assert alone["err"][0] == got["err"][j] and np.array_equal(alone["usage"], got["usage"][sl])
        assert np.array_equal(alone["dominant"], got["dominant"][sl]) and np.array_equal(alone["programs"][0], got["programs"][j])


# -------------------------------------------------------------------------------------------------------- stop rule
@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_stop_rule_is_sklearns(loss, golden):
    X, W0, H0 = nr.case(nr.STOP_CASE)
    tol = float(golden[f"stop.{TAG[loss]}.tol"])
    got = nmf.nmf(X, W0.shape[1], init=(W0, H0), beta_loss=loss, max_iter=nr.STOP_MAX_ITER, tol=tol, return_all=True)
    assert int(got["n_iter"][0]) == int(golden[f"stop.{TAG[loss]}.n_iter"])
    assert int(got["converged"][0]) == int(golden[f"stop.{TAG[loss]}.converged"])
    assert abs(got["err"][0] - nr.error(X, got["W"], got["H"][0], loss)) <= nr.error_bound(X, got["W"], got["H"][0], loss)
    hist = got["history_all"][0, 0]
    taken = int(got["n_iter"][0]) // 10 + 1
    assert np.isfinite(hist[:taken]).all() and np.isnan(hist[taken:]).all() and hist[taken - 1] == got["err"][0]
    # the cap: tol > 0 and the rule never fires -> n_iter = max_iter, not converged
    capped = nmf.nmf(X, W0.shape[1], init=(W0, H0), beta_loss=loss, max_iter=20, tol=1e-300)
    assert capped["n_iter"].tolist() == [20] and capped["converged"].tolist() == [0]


# ----------------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_starts_runs_and_input_width_are_bit_identical(loss):
    X, W0, H0 = data(nr.STACKED)
    rows, G, k = nr.STACKED[1:4]
    rng = np.random.RandomState(5)
    Ws = np.stack([W0 * rng.uniform(0.5, 1.5, W0.shape) for _ in range(3)])
    Hs = np.stack([np.stack([H0 * rng.uniform(0.5, 1.5, H0.shape) for _ in range(3)]) for _ in range(3)])   # (start, segment)
    kw = dict(offsets=OFF, beta_loss=loss, max_iter=20, tol=1e-3, return_all=True)
    three = nmf.nmf(X, k, init=(Ws, Hs), **kw)
    again = nmf.nmf(X, k, init=(Ws, Hs), **kw)
    same(three, again, ("W", "H", "err", "n_iter", "converged", "programs", "usage", "dominant", "W_all", "H_all", "err_all"))
    assert three["W_all"].shape == (3, rows, k) and three["H_all"].shape == (3, 3, k, G)
    for s in range(3):
        one = nmf.nmf(X, k, init=(Ws[s], Hs[s]), **kw)
        assert np.array_equal(one["W"], three["W_all"][s]) and np.array_equal(one["H"], three["H_all"][:, s])
        assert np.array_equal(one["err"], three["err_all"][:, s]) and np.array_equal(one["n_iter"], three["n_iter_all"][:, s])
    best = three["best_start"]
    assert np.array_equal(best, np.argmin(three["err_all"], axis=1))
    for j in range(3):
        assert np.array_equal(three["H"][j], three["H_all"][j, best[j]])
        assert np.array_equal(three["W"][OFF[j]:OFF[j + 1]], three["W_all"][best[j], OFF[j]:OFF[j + 1]])
    # fp32 input with ld > G (the padding is never read: it holds NaN) = its fp64 up-conversion
    pad = np.full((rows, G + 3), np.nan, dtype=np.float32)
    pad[:, :G] = X.astype(np.float32)
    a = nmf.nmf(pad, k, ld=G + 3, n_genes=G, init=(Ws[0], Hs[0]), **kw)
    b = nmf.nmf(pad[:, :G].astype(np.float64), k, init=(Ws[0], Hs[0]), **kw)
    same(a, b)
    # the random start: scikit-learn's stream per segment and start
    r = nmf.nmf(X, k, offsets=OFF, beta_loss=loss, n_init=2, seed=3, max_iter=1, tol=0.0, return_all=True)
    W1, H1 = nr.random_init(X[OFF[1]:OFF[2]], k, 4)
    Wr = nr.update_w(X[OFF[1]:OFF[2]], W1, H1, loss)
    bw = nr.step_bounds(rows, G, k, loss)[0]
    assert (np.abs(r["W_all"][1, OFF[1]:OFF[2]] - Wr) <= bw * Wr).all()


# -------------------------------------------------------------------------------------------------------- objective
@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_objective_does_not_rise(loss):
    for c, off in ((nr.CASES[1], None), (nr.STACKED, OFF)):
        X, W0, H0 = data(c)
        G, k = c[2], c[3]
        init = (W0, H0) if off is None else (W0, np.stack([H0] * 3))
        got = nmf.nmf(X, k, offsets=off, init=init, beta_loss=loss, max_iter=60, tol=1e-300, return_all=True)
        hist = got["history_all"][:, 0]
        assert hist.shape[1] == 7 and np.isfinite(hist).all() and (got["err_init_all"][:, 0] == hist[:, 0]).all()
        rise = hist[:, 1:] - hist[:, :-1]
        print(f"{c[0]} {TAG[loss]}: error {hist[0, 0]:.6g} -> {hist[0, -1]:.6g}")
        assert (rise <= (G + k) * nr.EPS * hist[:, :-1]).all() and (hist[:, -1] < hist[:, 0]).all()


# -------------------------------------------------------------------------------------------------------- transform
@pytest.mark.parametrize("loss", nr.LOSSES, ids=list(TAG.values()))
def test_transform_is_sklearns(loss, golden):
    X, _, _ = nr.case(nr.TRANSFORM_CASE)
    H = golden[f"transform.{TAG[loss]}.H"]
    got = nmf.transform(X, H, beta_loss=loss, max_iter=nr.TRANSFORM_ITERS, tol=0.0)
    spread = float(golden[f"transform.{TAG[loss]}.spread"])
    d_sk = rel(got["W"], golden[f"transform.{TAG[loss]}.W"])
    d_ref = rel(got["W"], nr.transform(X, H, loss, nr.TRANSFORM_ITERS, 0.0)[0])
    print(f"transform {TAG[loss]}: {d_ref / spread:.2f} of the spread ({spread / nr.EPS:.1f} eps) from the restatement, "
          f"{d_sk / spread:.2f} from scikit-learn")
    assert d_ref <= MARGIN * spread and d_sk <= MARGIN * spread + 64 * nr.EPS
    assert got["n_iter"].tolist() == [nr.TRANSFORM_ITERS] and (got["W"][3] == 0).all()
    # per segment, H shared: bit-identical to the segment alone
    Xs, _, _ = data(nr.STACKED)
    st = nmf.transform(Xs, H, offsets=OFF, beta_loss=loss, max_iter=20, tol=1e-3)
    for j in range(3):
        sl = slice(OFF[j], OFF[j + 1])
        one = nmf.transform(Xs[sl], H, beta_loss=loss, max_iter=20, tol=1e-3)
        assert np.array_equal(one["W"], st["W"][sl]) and one["n_iter"][0] == st["n_iter"][j] and one["err"][0] == st["err"][j]
        assert np.array_equal(one["usage"], st["usage"][sl]) and np.array_equal(one["dominant"], st["dominant"][sl])


# ----------------------------------------------------------------------------------------------------- input checks
def test_negative_and_non_finite_input_raise_naming_the_row():
    X, W0, H0 = data(nr.CASES[0])
    for value, dtype in ((np.nan, np.float64), (-1e-3, np.float32), (np.inf, np.float64)):
        bad = X.astype(dtype)
        bad[41, 7] = value
        bad[55, 0] = value
        with pytest.raises(ValueError, match="row 41 "):
            nmf.nmf(bad, 5, init=(W0, H0), max_iter=1)
        with pytest.raises(ValueError, match="row 41 "):
            nmf.transform(bad, H0, max_iter=1)


# -------------------------------------------------------------------------------------------------------------- CLI
def test_cli_prints_programs_and_writes_the_files(tmp_path, capsys):
    X, _, _ = data(nr.STACKED)
    k = nr.STACKED[3]
    rng = np.random.RandomState(4)
    pred, true = [], []
    for j in range(1, 3):                                                  # gene-major files, as the other CLIs read them
        t = X[OFF[j]:OFF[j + 1]]
        for lst, name, m in ((true, "t", t), (pred, "p", t * rng.uniform(0.8, 1.2, t.shape))):
            lst.append(str(tmp_path / f"{name}{j}.npy"))
            np.save(lst[-1], np.ascontiguousarray(m.T))
    names = tmp_path / "genes.npy"
    np.save(names, np.array([f"g{i}" for i in range(X.shape[1])]))
    out = tmp_path / "out"
    argv = ["--pred", *pred, "--true", *true, "--k", str(k), "--n_init", "2", "--max_iter", "20", "--genes", str(names),
            "--top", "3", "--out_dir", str(out)]
    assert nmf.main(argv) == 0
    text = capsys.readouterr().out.splitlines()
    assert sum(line.startswith("program ") for line in text) == k and text[-1].startswith("recovery: mean usage Pearson")
    assert all(tok.strip().startswith("g") for line in text if line.startswith("program ") for tok in line.split(": ")[1].split(","))
    z = np.load(out / nmf.OUT_FILE)
    want = nmf.nmf_slides([np.load(p).T for p in pred], k, True, n_init=2, max_iter=20)
    for key in nmf.KEYS:
        assert np.array_equal(z[key], want[key]), key
    assert z["slide_offsets"].tolist() == [0, 63, 363] and z["genes"][5] == "g5"
    assert np.array_equal(np.load(out / "1" / "usage.npy"), want["usage"][63:]) and sorted(os.listdir(out)) == ["0", "1", nmf.OUT_FILE]


# --------------------------------------------------------------------------------------------------------- recovery
def test_program_recovery_matches_the_host_score():
    X, _, _ = data(nr.STACKED)
    G, k = nr.STACKED[2], nr.STACKED[3]
    trues = [X[OFF[j]:OFF[j + 1]] for j in range(3)]
    rng = np.random.RandomState(9)
    preds = [t * rng.uniform(0.7, 1.3, t.shape) for t in trues]
    kw = dict(max_iter=nr.ITERS, tol=0.0, seed=2)
    rec = nmf.program_recovery(preds, trues, k, n_top=8, **kw)
    # the same score from the restatement's factors alone: fit the measured matrix, transform the predicted one under the
    # restatement's own H (nothing of the device enters the reference)
    Xt, Xp = np.concatenate(trues), np.concatenate(preds)
    W0t, H0t = nr.random_init(Xt, k, 2)
    Wt, Ht = nr.fit(Xt, W0t, H0t, "frobenius", nr.ITERS, 0.0)[:2]
    Wp, Hp = nr.fit(Xp, *nr.random_init(Xp, k, 2), "frobenius", nr.ITERS, 0.0)[:2]
    Wu = nr.transform(Xp, Ht, "frobenius", nr.ITERS, 0.0)[0]
    pt, ut, dt = nr.normalise(Wt, Ht)
    pp, _, _ = nr.normalise(Wp, Hp)
    _, uu, du = nr.normalise(Wu, Ht)
    want = nmf.usage_scores(uu, ut, du, dt, OFF)
    # the tolerance: 8 x the restatement's own re-ordering spread of this whole chain (fit, transform under the fitted H,
    # usage), i.e. the same chain with rows and genes permuted, carried through the scores
    rng = np.random.RandomState(1)
    pr, pg = rng.permutation(Xt.shape[0]), rng.permutation(G)
    Wt2, Ht2 = nr.fit(Xt[pr][:, pg], W0t[pr], H0t[:, pg], "frobenius", nr.ITERS, 0.0)[:2]
    Wu2 = nr.transform(Xp[pr][:, pg], Ht2, "frobenius", nr.ITERS, 0.0)[0]
    ut2, uu2 = nr.normalise(Wt2, Ht2)[1], nr.normalise(Wu2, Ht2)[1]
    eta = MARGIN * max(np.abs(ut2 - ut[pr]).max(), np.abs(uu2 - uu[pr]).max())
    sw, sh = nr.permuted_spread(Xt, W0t, H0t, "frobenius", nr.ITERS)
    sw2, sh2 = nr.permuted_spread(Xp, *nr.random_init(Xp, k, 2), "frobenius", nr.ITERS)
    delta = MARGIN * max(sw, sh, sw2, sh2)
    assert 0 < eta <= 1e-10 * ut.max()
    assert np.abs(rec["true"]["usage"] - ut).max() <= eta and np.abs(rec["pred_under_true"]["usage"] - uu).max() <= eta

    def sigma(u, c):
        return np.sqrt(((u[c] - u[c].mean(axis=0)) ** 2).mean(axis=0))
    cuts = [slice(OFF[j], OFF[j + 1]) for j in range(3)]
    sig = np.stack([np.minimum(sigma(ut, c), sigma(uu, c)) for c in cuts])
    fin = np.isfinite(want["pearson"])
    assert fin.all() and (sig > 0).all()
    tol_r = 8 * eta / sig                                                  # r is a ratio of centred sums: 4 terms, 2 x slack
    print(f"recovery: mean Pearson {rec['mean_pearson']:.4f}, agreement {rec['mean_dominant_agreement']:.4f}, mean cosine "
          f"{rec['mean_cosine']:.4f}; usage tolerance {eta:.3g}, tolerance on r at the most {tol_r.max():.3g}")
    assert tol_r.max() <= 1e-9                                             # (the tolerances themselves are bounded)
    assert np.isfinite(rec["pearson"]).all() and (np.abs(rec["pearson"] - want["pearson"]) <= tol_r).all()
    tol_p = 8 * eta / np.minimum(sigma(ut, slice(None)), sigma(uu, slice(None)))
    assert tol_p.max() <= 1e-9 and (np.abs(rec["pearson_pooled"] - want["pearson_pooled"]) <= tol_p).all()
    gap_t, gap_u = (np.sort(u, axis=1)[:, -1] - np.sort(u, axis=1)[:, -2] for u in (ut, uu))
    zero = (ut.max(axis=1) == 0) | (uu.max(axis=1) == 0)                   # a zero row: dominant -1 on both sides, exactly
    clear = ((gap_t > 2 * eta) & (gap_u > 2 * eta)) | zero
    assert (~clear).sum() <= 3 and np.array_equal(rec["true"]["dominant"][clear], dt[clear])
    assert np.array_equal(rec["pred_under_true"]["dominant"][clear], du[clear])
    assert abs(rec["dominant_agreement_pooled"] - want["dominant_agreement_pooled"]) <= (~clear).sum() / clear.size
    assert (np.abs(rec["dominant_agreement"] - want["dominant_agreement"]) <= (~clear).sum() / np.diff(OFF)).all()
    pairs, cos = nmf.match_programs(pt, pp)
    tol_c = 4 * delta * np.sqrt(G) * max(pt.max(), pp.max()) / min(np.sqrt((p * p).sum(axis=1)).min() for p in (pt, pp))
    assert np.array_equal(rec["matching"], pairs) and np.abs(rec["cosine"] - cos).max() <= tol_c
    assert rec["top_overlap"].shape == (k,) and (rec["top_jaccard"] <= 1).all()
    # measured against measured: the same fit twice, so every matched cosine is 1 and every top list the same
    same_rec = nmf.program_recovery(trues, trues, k, n_top=8, **kw)
    assert np.abs(same_rec["cosine"] - 1.0).max() <= (G + 4) * nr.EPS and (same_rec["top_overlap"] == 8).all()
    assert same_rec["matching"][:, 0].tolist() == same_rec["matching"][:, 1].tolist()
    # the programs are signatures deconv.nnls accepts as they are
    from mclstexp_amd import deconv
    d = deconv.nnls(Xt, rec["true"]["programs"][0])
    assert d["coef"].shape == (Xt.shape[0], k) and (d["coef"] >= 0).all()
