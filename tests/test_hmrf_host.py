"""CPU: the numpy restatement tests/hmrf_reference.py (the yardstick of tests/test_hmrf_gpu.py) against independent dense
formulas recorded in tests/golden/hmrf.npz by tests/golden/gen_hmrf_goldens.py (scipy 1.15.3) -- the field as W @ Q, the
densities by ``scipy.stats.multivariate_normal.logpdf``, every log-sum-exp by ``scipy.special.logsumexp``, the refine rule
by ``numpy.bincount`` -- and against tests/mixture_reference.py, which tests/test_mixture_host.py pins to sklearn; then the
conditions that keep the GPU test from hiding a failure, the host-side argument checks of mclstexp_amd.hmrf and its CLI.

Tolerances against the dense formulas, to first order from the stated orders (eps = 2^-52; both sides carry the error):
  field (kw products, one running sum; the dense product adds exact zeros)   bf = 2 (kw + 1) eps sum_c |w q|
  weighted log prob g: scipy decomposes the covariance and forms the quadratic form, the restatement factors it and
    multiplies by the factor: four operations, each relatively accurate to (D + 2) kappa eps on terms no larger than
    2 (1 + |g|), kappa the condition number of the covariance                 bg = 16 (D + 2) kappa eps (1 + |g|)
  v = g + (beta f)                                                            bv = bg + beta bf + 4 eps (|g| + beta f)
  lse (max subtracted, K terms, exp and log one ulp each)                     bl = max_k bv + 2 (K + 8) eps (1 + |lse|)
  za                                                                          bz = beta max_k bf + 2 (K + 8) eps (1 + |za|)
  log_resp                                                                    bv + bl + 2 eps |log_resp|
  score = mean (lse - za)                                                     mean (bl + bz) + 2 (n / 256 + 10) eps mean |lse - za|
Labels, n_iter, converged, the refine rule and ARI are compared for equality; the agreement sums hold at most n kw terms of
one sign: 2 (n kw + 1) eps relative."""
import os

import numpy as np
import pytest

import hmrf_reference as hr
import mixture_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmrf.npz")
EPS = 2.0 ** -52
TOL = 1e-3
FITS = [(name, ctype) for name in hr.FIT_CASES for ctype in hr.make_case(name)["types"]]
TEACHER = [(name, ctype) for name in ("A", "C", "G") for ctype in (mr.TYPES if name != "G" else ("full",))]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def fits():
    """The restatement's fit of every fixture and type, computed once."""
    return {(name, ctype): hr.ref_fit(name, ctype) for name, ctype in FITS}


def within(got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    assert float(r.max()) <= 1.0, float(r.max())
    return float(r.max())


@pytest.mark.parametrize("name", hr.FIT_CASES)
def test_fixture_is_the_recorded_one(name, golden):
    c = hr.make_case(name)
    assert np.allclose(hr.checksum(c), golden[name + "/checksum"], rtol=1e-12, atol=0), \
        "numpy's generator no longer reproduces the recorded fixture"
    n = c["x"].shape[0]
    assert c["nbr"].min() >= 0 and c["nbr"].max() < n
    if name == "A":
        assert n == 132 and n % 16 == 4 and (c["w"] == 1.0).all()
    if name == "C":
        deg = (c["w"] != 0).sum(axis=1)
        assert 75 <= n <= 85 and deg.min() < deg.max() and (c["w"] == 0).any(), "pruned slots and unequal degrees"
        assert np.allclose(c["w"].sum(axis=1), 1.0)
    if name == "E":
        assert ((c["w"] != 0).sum(axis=1) == 0).sum() >= 3, "several rows of degree 0"


@pytest.mark.parametrize("name,ctype", FITS)
def test_recorded_fit_is_reproduced(name, ctype, golden, fits):
    key, f = f"{name}/{ctype}/", fits[(name, ctype)]
    assert f["n_iter"] == int(golden[key + "n_iter"]) and f["converged"] == int(golden[key + "converged"])
    assert np.array_equal(f["labels"], golden[key + "labels"].astype(np.int32))
    for field in ("lower_bounds", "weights", "means", "score"):      # the same code on another libm: a few roundings
        assert np.allclose(f[field], golden[key + field], rtol=0, atol=1e-10), field


# ------------------------------------------------------------------------------- 1. against the dense formulas
@pytest.mark.parametrize("name,ctype", TEACHER)
def test_restated_estep_is_the_dense_formulas(name, ctype, golden):
    t = hr.teacher_case(name)
    w, mu, pc, cov = t["params"][ctype]
    x, beta = t["x"], t["beta"]
    n, D = x.shape
    K, kw = w.size, t["nbr"].shape[1]
    e = hr.estep(x, w, mu, pc, ctype, t["nbr"], t["w"], t["q"], beta)
    key = f"{name}/{ctype}/dense_"
    assert not e["bad"]
    kappa = 1.0
    for k in range(K):
        if ctype in ("full", "tied"):
            kappa = max(kappa, np.linalg.cond(cov[k] if ctype == "full" else cov))
        elif ctype == "diag":
            kappa = max(kappa, cov[k].max() / cov[k].min())
    bf = 2 * (kw + 1) * EPS * e["field"]                              # w, q >= 0: sum |w q| is the field itself
    bg = 16 * (D + 2) * kappa * EPS * (1 + np.abs(e["wlp"]))
    bv = bg + beta * bf + 4 * EPS * (np.abs(e["wlp"]) + beta * e["field"])
    bl = bv.max(axis=1) + 2 * (K + 8) * EPS * (1 + np.abs(e["lse"]))
    bz = beta * bf.max(axis=1) + 2 * (K + 8) * EPS * (1 + np.abs(e["za"]))
    rows = {"field": within(e["field"], golden[key + "field"], np.maximum(bf, 1e-300)),
            "wlp": within(e["wlp"], golden[key + "wlp"], bg), "lse": within(e["lse"], golden[key + "lse"], bl),
            "za": within(e["za"], golden[key + "za"], bz),
            "log_resp": within(e["log_resp"], golden[key + "log_resp"], bv + bl[:, None] + 2 * EPS * np.abs(e["log_resp"])),
            "score": within(e["score"], golden[key + "score"],
                            (bl + bz).mean() + 2 * (n / 256 + 10) * EPS * np.abs(e["lse"] - e["za"]).mean())}
    assert np.isfinite(e["log_resp"]).all() and np.isfinite(e["lse"]).all() and np.isfinite(e["za"]).all()
    print(f"  {name} {ctype}: " + " ".join(f"{k}={v:.2g}" for k, v in rows.items()))


# -------------------------------------------------------------------------------- 2. beta = 0 is the mixture
@pytest.mark.parametrize("name,ctype", FITS)
def test_beta_zero_is_the_mixture_bit_for_bit(name, ctype):
    c = hr.make_case(name)
    f = hr.ref_fit(name, ctype, beta=0.0)
    g = mr.fit(c["x"], c["K"], c["init"], ctype)
    assert f["status"] == 0 and g["status"] == 0 and f["n_iter"] == g["n_iter"] and f["converged"] == g["converged"]
    for field in ("labels", "resp", "log_resp", "weights", "means", "covariances", "precisions_cholesky", "lse"):
        assert np.array_equal(f[field], g[field]), field
    assert abs(f["lower_bound"] - g["lower_bound"]) <= 64 * c["K"] * EPS * (1 + abs(g["lower_bound"]))
    assert (f["field"] >= 0).all() and f["field"].max() <= (c["w"].sum(axis=1).max()) * (1 + 64 * EPS)


def test_zero_weight_slide_is_the_mixture():
    c = hr.make_case("E")
    f = hr.fit(c["x"], c["K"], c["init"], c["nbr"], np.zeros_like(c["w"]), c["beta"])
    g = mr.fit(c["x"], c["K"], c["init"], "full")
    for field in ("labels", "resp", "weights", "means", "covariances", "precisions_cholesky"):
        assert np.array_equal(f[field], g[field]), field
    assert f["n_iter"] == g["n_iter"] and not f["field"].any()


def test_row_standardised_weights_need_beta_times_the_degree():
    """Binary weights at beta and row-standardised weights at beta k walk through the same fit on a full k = 8 list."""
    c = hr.make_case("A")
    a = hr.fit(c["x"], c["K"], c["init"], c["nbr"], c["w"], 0.5)
    b = hr.fit(c["x"], c["K"], c["init"], c["nbr"], c["w"] / 8.0, 4.0)          # 1 / 8 and x 8 are exact
    assert a["n_iter"] == b["n_iter"] and np.array_equal(a["labels"], b["labels"])
    assert np.allclose(a["resp"], b["resp"], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------ 3. the fixtures decide clearly
@pytest.mark.parametrize("name,ctype", FITS)
def test_fixture_conditions(name, ctype, fits):
    f = fits[(name, ctype)]
    assert f["status"] == 0 and f["converged"] == 1
    change = np.abs(np.diff(np.concatenate([[-np.inf], f["lower_bounds"]])))
    assert change[-1] < 0.9 * TOL and (change[:-1] > 1.1 * TOL).all(), change
    assert mr.top_two_gap(f["log_resp"]).min() >= 1e-6


def test_case_i_does_not_converge_and_case_h_fails():
    i = hr.ref_fit("A", "full", max_iter=3)
    assert i["status"] == 0 and i["n_iter"] == 3 and i["converged"] == 0
    change = np.abs(np.diff(np.concatenate([[-np.inf], i["lower_bounds"]])))
    assert (change > 1.1 * TOL).all() and mr.top_two_gap(i["log_resp"]).min() >= 1e-6
    h = hr.make_h()
    f = hr.fit(h["x"], h["K"], h["init"], h["nbr"], h["w"], h["beta"], "full", reg=0.0)
    assert f["status"] == 1 and np.isnan(f["lower_bound"])
    assert int((h["init"] == 2).sum()) == 1


def test_a_bad_neighbour_index_counts_as_pruned_and_is_flagged():
    c = hr.make_case("A")
    nbr = c["nbr"].copy()
    nbr[5, 2], nbr[9, 0] = 132, -1
    w = c["w"].copy()
    f = hr.fit(c["x"], c["K"], c["init"], nbr, w, c["beta"])
    w[5, 2] = w[9, 0] = 0.0
    g = hr.fit(c["x"], c["K"], c["init"], c["nbr"], w, c["beta"])
    assert f["status"] == hr.BAD_INDEX and g["status"] == 0
    assert np.array_equal(f["resp"], g["resp"]) and f["lower_bound"] == g["lower_bound"]


# -------------------------------------------------------------------------------------------- 4. the recovery case
def test_case_b_recovers_the_planted_stripes(golden):
    c = hr.make_case("B")
    f1, f0 = hr.ref_fit("B", "full"), hr.ref_fit("B", "full", beta=0.0)
    a1, a0 = hr.ari(f1["labels"], c["truth"]), hr.ari(f0["labels"], c["truth"])
    e1, e0 = hr.edge_sums(f1["labels"], c["nbr"], c["w"]), hr.edge_sums(f0["labels"], c["nbr"], c["w"])
    rec = golden["B/recovery"]
    assert a1 == rec[0] and a0 == rec[1] and e1[0] / e1[1] == rec[2] and e0[0] / e0[1] == rec[3]
    assert a1 >= a0 + 0.3 and e1[0] / e1[1] > e0[0] / e0[1]
    assert hr.ari(c["truth"], c["truth"]) == 1.0 and abs(hr.ari(c["truth"], np.arange(340) % 4)) < 0.05
    print(f"  case B: ARI {a1:.3f} at beta = 1 against {a0:.3f} at beta = 0; edge agreement {rec[2]:.3f} against {rec[3]:.3f}")


# -------------------------------------------------------------------------------- 5. refine rule, agreement sums
@pytest.mark.parametrize("name", ["A", "C"])
def test_refine_and_agreement_are_the_bincount_form(name, golden):
    c = hr.make_case(name)
    lab = hr.label_case(name)
    assert np.array_equal(lab, golden[name + "/refine_in"].astype(np.int32)) and (lab == -1).any() and (lab == 1000).any()
    out, changed = hr.refine(lab, c["nbr"], c["w"])
    want = golden[name + "/refine_bincount"].astype(np.int32)
    assert np.array_equal(out, want) and changed == int((want != lab).sum()) and changed > 0
    assert (out[lab < 0] == -1).all()
    n, kw = c["nbr"].shape
    got = np.array(hr.edge_sums(lab, c["nbr"], c["w"]))
    assert np.all(np.abs(got - golden[name + "/agreement_dense"]) <= 2 * (n * kw + 1) * EPS * golden[name + "/agreement_dense"])
    assert 0 < got[0] < got[1]


def test_refine_rule_by_hand():
    nbr = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 5], [4, 0, 1]], dtype=np.int32)
    w = np.ones((6, 3))
    out, changed = hr.refine(np.array([7, 2, 2, 2, -1, 9]), nbr, w)
    assert out.tolist() == [2, 2, 2, 2, -1, 9] and changed == 1      # spot 5: neighbours -1, 7, 2: no majority
    out, _ = hr.refine(np.array([5, 1, 1, 3]), nbr[:4], w[:4])
    assert out.tolist() == [1, 1, 1, 1]                                # spots 0 and 3: alone, and 1 has 2 of m = 3
    out, _ = hr.refine(np.array([5, 1, 3, 3]), nbr[:4], np.array([[1, 1, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1.0]]))
    assert out.tolist() == [5, 3, 3, 3]                                # spot 0: m = 2, counts 1 : 1 : 1, 2 x 1 > 2 fails


# ------------------------------------------------------------------------------------------ 6. argument validation
@pytest.fixture
def host_only(monkeypatch):
    from mclstexp_amd import hmrf
    monkeypatch.setattr(hmrf, "device", lambda who: pytest.fail("the device was touched"))
    return hmrf


def graph_of(c):
    return {"nbr": c["nbr"], "w": c["w"], "offsets": [0, c["x"].shape[0]]}


def test_argument_errors_come_before_the_device(host_only):
    h, c = host_only, hr.make_case("A")
    x, g, n = c["x"], graph_of(c), 132
    bad = [
        (dict(z=x[:, 0]), "2-D"), (dict(z=np.zeros((n, 65))), "65 columns"), (dict(graph={"nbr": c["nbr"]}), "spatial.lattice"),
        (dict(graph=dict(g, offsets=[0, 100])), "offsets"), (dict(graph=dict(g, w=c["w"][:, :4])), "nbr and w"),
        (dict(graph=dict(g, nbr=c["nbr"].astype(np.float64))), "integers"),
        (dict(graph=dict(g, w=np.where(c["w"] > 0, np.nan, 0.0))), "finite"),
        (dict(graph=dict(g, nbr=np.zeros((n, 65), np.int32), w=np.zeros((n, 65)))), "65 neighbour slots"),
        (dict(k=0), "k must lie"), (dict(graph=dict(g, offsets=[0, 10, 132]), k=[11, 3]), "exceeds"),
        (dict(k=[3, 3]), "segments"), (dict(beta=-0.5), "finite and >= 0"),
        (dict(beta=float("inf")), "finite and >= 0"), (dict(beta=[1.0, 2.0]), "2 values for 1 slides"),
        (dict(beta="strong"), "beta must be a number"), (dict(covariance_type="round"), "covariance_type"),
        (dict(tol=-1.0), "tol"), (dict(max_iter=0), "max_iter"), (dict(reg_covar=-1e-6), "reg_covar"), (dict(n_init=0), "n_init"),
        (dict(init_labels=np.zeros((2, 100), np.int32)), "init_labels"),
    ]
    for kw, match in bad:
        args = dict(z=x, graph=g, k=3)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            h.hmrf(**args)
    with pytest.raises(ValueError, match="16384"):
        big = 16385
        h.hmrf(np.zeros((big, 2)), {"nbr": np.zeros((big, 1), np.int32), "w": np.zeros((big, 1)), "offsets": [0, big]}, 2)
    for kw, match in [(dict(betas=[]), "at least one"), (dict(betas=[0.0, -1.0]), "finite and >= 0"), (dict(k=0), "k must lie"),
                      (dict(covariance_type="round"), "covariance_type"), (dict(n_init=0), "n_init")]:
        args = dict(z=x, graph=g, k=3, betas=[0.0, 1.0])
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            h.scan_beta(**args)
    lab = hr.label_case("A")
    for fn in (h.refine_labels, h.edge_agreement):
        with pytest.raises(ValueError, match="offsets must run"):
            fn(lab[:100], g)
        with pytest.raises(ValueError, match=r"expected a \(132,\) vector"):
            fn(lab[:, None], g)
        with pytest.raises(ValueError, match="integer labels"):
            fn(lab.astype(np.float64), g)
        with pytest.raises(ValueError, match="-1 for a spot"):
            fn(np.where(lab < 0, -2, lab), g)
        with pytest.raises(ValueError, match="spatial.lattice"):
            fn(lab, {"nbr": c["nbr"], "w": c["w"]})
    with pytest.raises(ValueError, match="n_iter"):
        h.refine_labels(lab, g, 0)
    model = {"covariance_type": "full", "k": np.array([3]), "weights": None, "means": None, "precisions_cholesky": None}
    with pytest.raises(ValueError, match="covariance_type"):
        h.estep(x, dict(model, covariance_type="round"), g, np.zeros((n, 3)))
    with pytest.raises(ValueError, match="2-D"):
        h.estep(x[:, 0], model, g, np.zeros((n, 3)))
    with pytest.raises(ValueError, match="finite and >= 0"):
        h.estep(x, model, g, np.zeros((n, 3)), beta=-1.0)
    preds, coords = [np.zeros((n, 20))], [c["coords"]]
    with pytest.raises(ValueError, match="at least one slide"):
        h.domains_slides([], [])
    with pytest.raises(ValueError, match="one coordinate array"):
        h.domains_slides(preds, coords + coords)
    with pytest.raises(ValueError, match=r"coords must be \(132, 2\)"):
        h.domains_slides(preds, [c["coords"][:100]])
    with pytest.raises(ValueError, match="one measured matrix"):
        h.domains_slides(preds, coords, trues=[])
    with pytest.raises(ValueError, match="differ in spots"):
        h.domains_slides(preds, coords, trues=[np.zeros((100, 20))])
    with pytest.raises(ValueError, match="finite and >= 0"):
        h.domains_slides(preds, coords, beta=-1.0)


def test_no_gpu_error_names_the_module(monkeypatch):
    import torch
    from mclstexp_amd import hmrf
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c = hr.make_case("A")
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.hmrf: no GPU available"):
        hmrf.hmrf(c["x"], graph_of(c), 3, init_labels=c["init"])
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.hmrf: no GPU available"):
        hmrf.edge_agreement(hr.label_case("A"), graph_of(c))


def test_entry_points_check_their_arguments_without_a_gpu():
    import ctypes as C
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_hmrf_workspace_bytes(100, 2, 3, 9, 4) == lib.mcl_gmm_workspace_bytes(100, 2, 3, 9, 4) + 8 * 3 * 100 * 4
    assert lib.mcl_hmrf_workspace_bytes(100, 2, 3, 65, 4) == -1 and lib.mcl_hmrf_workspace_bytes(0, 1, 1, 1, 1) == -1
    assert lib.mcl_label_refine(None, 1, 1, None, None, None, 1, None, None, None) == -1
    assert lib.mcl_edge_agreement(None, 1, 1, None, None, None, 1, None, None) == -1
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert lib.mcl_label_refine(p, 1, 1, p, p, p, 1, p, p, None) == -1, "labels_out must not alias labels"
    assert lib.mcl_label_refine(p, 1, 1, p, p, p, 65, p + 8, p, None) == -2
    assert lib.mcl_edge_agreement(p, 1, 1, p, p, p, 65, p, None) == -2


# ---------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_arguments():
    from mclstexp_amd import hmrf
    a = hmrf.parse_args(["--pred", "p0.npy", "p1.npy", "--coords", "c0.npy", "c1.npy", "--true", "t0.npy", "t1.npy", "--k", "5",
                         "--beta", "2", "--scan", "0", "0.5", "1", "--refine", "2", "--out_dir", "out"])
    assert a.pred == ["p0.npy", "p1.npy"] and a.coords == ["c0.npy", "c1.npy"] and a.true == ["t0.npy", "t1.npy"]
    assert a.k == 5 and a.beta == 2.0 and a.scan == [0.0, 0.5, 1.0] and a.refine == 2 and a.out_dir == "out"
    d = hmrf.parse_args(["--pred", "p.npy", "--coords", "c.npy"])
    assert d.k is None and tuple(d.k_range) == (2, 12) and d.beta == 1.0 and d.scan is None and d.refine == 0
    assert d.lattice_k == 8 and d.prune == "NA" and d.covariance_type == "full"
    for argv in (["--pred", "p.npy"], ["--pred", "a.npy", "b.npy", "--coords", "c.npy"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--true", "t0.npy", "t1.npy"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--beta", "-1"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--scan", "1", "nan"],
                 ["--pred", "p.npy", "--coords", "c.npy", "--refine", "-1"]):
        with pytest.raises(SystemExit):
            hmrf.parse_args(argv)
    res = {"slides": [{"k": 3, "beta": 1.0, "n_iter": 7, "converged": 1, "edge_agreement": 0.9, "gmm_edge_agreement": 0.5,
                       "silhouette": 0.25, "calinski_harabasz": 10.5, "davies_bouldin": 1.5, "ari": 0.75, "nmi": 0.5}]}
    assert hmrf.format_report(res) == ("slide 0: k: 3, beta: 1.0, n_iter: 7, converged: 1, edge_agreement: 0.9 (gmm: 0.5), "
                                       "silhouette: 0.25, CH: 10.5, DB: 1.5, ARI: 0.75, NMI: 0.5")
