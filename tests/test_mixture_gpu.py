"""GPU: mclstexp_amd.mixture (csrc/mixture.hip) against the numpy restatement tests/mixture_reference.py, which
tests/test_mixture_host.py pins to sklearn's own results.  Parity with mclust or an R release is unpinned.

One teacher-forced E-step and M-step: bounds derived to first order from the stated orders, not tuned (eps = 2^-52; device
and restatement both carry the error, hence the leading 2; they read the same inputs, so x - mu is the same on both sides):
  y_j = sum_d (x - mu)_d P_dj             by = 2 (D + 1) eps sum_d |(x - mu)_d P_dj|
  ss = ||y||^2                            bss = sum_j 2 |y_j| by_j + 2 (D + 2) eps ss
  log det P_k (D logs, one ulp each)      bld = 2 (D + 1) eps sum_j |log P_jj|
  weighted log prob                       bw = bss / 2 + bld + 2 eps |log w| + 6 eps (|D log 2 pi + ss| / 2 + |log det| + |log w|)
  log_prob_norm (max subtracted; a |a| exp(-|a|) <= 1 / e)       bl = max_k bw + 2 (K + 8) eps (1 + |lse|)
  log_resp                                bw + bl + 2 eps |log_resp|;  resp: resp x that + 2 eps resp
  score (thread-strided sums, tree)       mean bl + 2 (n / 256 + 10) eps mean |lse|
  labels                                  equal on every row whose top-two gap exceeds twice the row's log_resp bound
  resp = exp(log_resp) (one ulp each)     br = 2 eps resp
  n_k (n terms, running sum)              bn = 2 (n + 1) eps n_k
  means                                   bm = 2 (n + 2) eps sum_i r |x| / n_k + |mu| (bn / n_k + 2 eps)
  weights                                 w (2 bn / n_k + 2 (K + 2) eps)
  covariances, full                       (2 (n + 4) eps sum_i r |d_a| |d_b| + bm_a sum_i r |d_b| + bm_b sum_i r |d_a|) / n_k
                                          + |C_ab| (bn / n_k + 4 eps),  d = x - mu
  tied                                    (2 (n + 1) eps sum_i |x_a x_b| + bs + 2 eps (|X^T X| + |s|)) / sum n_k + |C| (bn / n_k + 2 eps),
                                          bs = sum_k (bn_k |mu_a mu_b| + n_k (bm_a |mu_b| + |mu_a| bm_b)) + 2 (K + 2) eps sum_k n_k |mu_a mu_b|
  diag                                    2 (n + 2) eps sum_i r x^2 / n_k + (sum_i r x^2 / n_k) (bn / n_k + 2 eps) + 2 |mu| bm
                                          + 6 eps (sum_i r x^2 / n_k + mu^2);  spherical: its mean over d + 2 (D + 1) eps mean |.|
  precisions_cholesky, diag / spherical   P (bC / (2 C) + 4 eps)
  full / tied (Cholesky, then its inverse: dP = -P dL^T P, ||dL||_F <= kappa ||dC||_F / (sqrt 2 ||L||_2))
                                          ||P||_2^2 ||L||_2 kappa / sqrt 2 (||bC||_F + 4 (D + 2) eps ||C||_F) / ||C||_2
                                          + 4 (D + 2) eps kappa max |P|
Measured on MI355X, largest error / bound over the three teacher-forced fixtures x four types (every test prints its rows
with -s); integer outputs are equal:
  log_prob_norm 0.014   log_resp 0.033   resp 0.016   score 0 (bit-equal)
  weights 0.00013       means 0.0022     covariances 0.0012   precisions_cholesky 0.002

Full fits on the six fixtures x four types: n_iter, converged and restart are equal; the floats lie inside 16 x the largest
deviation from the restatement measured on MI355X over all fixtures and types (FIT_MEASURED; absolute, *_rel relative to
the largest magnitude of the array).  Labels are equal on every row whose restatement top-two gap exceeds twice the
log_resp allowance; the fixtures leave out no row (their smallest gap is 1.0e-2).

Validity: bounds 2 (n + D + 8) eps relative on every distance sum, so 4 (n + D + 8) eps on a silhouette value and on its
mean; CH and DB carry the centroid error as well: 8 (n + D + 8) eps (1 + max |x| / rms distance to the centroid) relative.
There is only sqrt, +, -, x and / in it, and the restatement follows the kernel's orders: every silhouette value, mean,
CH and DB came out bit-equal on MI355X in every case below (ratio 0)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mixture_reference as mr

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 16.0
FIT_MEASURED = {"lower_bound": 1.5e-14, "score": 1.5e-14, "weights": 2.0e-16, "means": 3.8e-15, "covariances": 2.2e-14,
                "precisions_cholesky_rel": 4.6e-12, "bic_rel": 2.3e-16, "aic_rel": 2.4e-16, "resp": 2.5e-14,
                "log_resp_rel": 8.9e-12, "log_prob_norm_rel": 1.7e-13}


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else v


def ratio(got, want, bound):
    """Largest |got - want| / bound; asserts it is <= 1 and that NaN sits where the restatement has it."""
    got, want = np.asarray(host(got), np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound[ok])
    worst = float(r.max()) if r.size else 0.0
    assert worst <= 1.0, worst
    return worst


def deviation(got, want, name):
    """Largest |got - want|; *_rel: over the largest magnitude of the array; log_resp_rel: over max(1, |log_resp|) element by
    element (a far component's log_resp is -1e3 and carries the rounding of that magnitude)."""
    got, want = np.asarray(host(got), np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    if name == "log_resp_rel":
        return float(np.max(err / np.maximum(1.0, np.abs(want))))
    return float(np.max(err)) / (float(np.max(np.abs(want))) if name.endswith("_rel") else 1.0)


def assert_measured(rows, scale=1.0):
    for name, err in rows.items():
        assert err <= scale * MARGIN * FIT_MEASURED[name], (name, err, scale * MARGIN * FIT_MEASURED[name])


@pytest.fixture(scope="module")
def mixture():
    from mclstexp_amd import mixture as m
    return m


@pytest.fixture(scope="module")
def ref_fits():
    """The restatement's fit of every fixture and type, computed once and left unchanged."""
    out = {}
    for case in mr.CASES:
        x, init, _ = mr.make_case(*case)
        for ctype in mr.TYPES:
            out[(mr.case_name(case), ctype)] = mr.fit(x, case[2], init, ctype)
    return out


# ------------------------------------------------------------------------------------------ one E-step, one M-step
def estep_bounds(x, w, mu, pc, ctype, e):
    n, D = x.shape
    K = w.size
    bw = np.empty((n, K))
    for k in range(K):
        diff = x - mu[k]
        if ctype in ("full", "tied"):
            P = pc[k] if ctype == "full" else pc
            y = diff @ P
            by = 2 * (D + 1) * EPS * (np.abs(diff) @ np.abs(P))
            logs = np.log(np.diag(P))
        else:
            p = pc[k] if ctype == "diag" else np.full(D, pc[k])
            y = diff * p
            by = 4 * EPS * np.abs(y)
            logs = np.log(p)
        ss = (y * y).sum(axis=1)
        bss = (2 * np.abs(y) * by).sum(axis=1) + 2 * (D + 2) * EPS * ss
        bld = 2 * (D + 1) * EPS * np.abs(logs).sum()
        lw = abs(np.log(w[k]))
        bw[:, k] = bss / 2 + bld + 2 * EPS * lw + 6 * EPS * (np.abs(D * mr.LOG_2PI + ss) / 2 + abs(logs.sum()) + lw)
    bl = bw.max(axis=1) + 2 * (K + 8) * EPS * (1 + np.abs(e["lse"]))
    blr = bw + bl[:, None] + 2 * EPS * np.abs(e["log_resp"])
    return {"log_prob_norm": bl, "log_resp": blr, "resp": e["resp"] * blr + 2 * EPS * e["resp"],
            "score": bl.mean() + 2 * (n / 256 + 10) * EPS * np.abs(e["lse"]).mean()}


def chol_bound(C, bC, P):
    D = C.shape[0]
    lam = np.linalg.eigvalsh(C)
    kappa, nC = lam[-1] / lam[0], lam[-1]
    nb = np.linalg.norm(bC) + 4 * (D + 2) * EPS * np.linalg.norm(C)
    return (1.0 / lam[0]) * np.sqrt(lam[-1]) * kappa / np.sqrt(2.0) * nb / nC + 4 * (D + 2) * EPS * kappa * np.abs(P).max()


def mstep_bounds(x, resp, ctype, w, mu, cov, pc):
    n, D = x.shape
    K = resp.shape[1]
    nk = resp.sum(axis=0) + 10 * EPS
    bn = 2 * (n + 1) * EPS * nk
    bm = 2 * (n + 2) * EPS * (resp.T @ np.abs(x)) / nk[:, None] + np.abs(mu) * (bn / nk + 2 * EPS)[:, None]
    out = {"weights": w * (2 * bn / nk + 2 * (K + 2) * EPS), "means": bm}
    if ctype == "full":
        bC, bP = np.empty_like(cov), np.empty_like(pc)
        for k in range(K):
            d = np.abs(x - mu[k])
            s1 = resp[:, k] @ d
            sab = (resp[:, k:k + 1] * d).T @ d
            bC[k] = (2 * (n + 4) * EPS * sab + np.outer(bm[k], s1) + np.outer(s1, bm[k])) / nk[k] \
                + np.abs(cov[k]) * (bn[k] / nk[k] + 4 * EPS)
            bP[k] = chol_bound(cov[k], bC[k], pc[k])
    elif ctype == "tied":
        amu = np.abs(mu)
        bs = np.einsum("k,ka,kb->ab", bn, amu, amu) + np.einsum("k,ka,kb->ab", nk, bm, amu) \
            + np.einsum("k,ka,kb->ab", nk, amu, bm) + 2 * (K + 2) * EPS * np.einsum("k,ka,kb->ab", nk, amu, amu)
        xtx, s = x.T @ x, np.einsum("k,ka,kb->ab", nk, mu, mu)
        bC = (2 * (n + 1) * EPS * (np.abs(x).T @ np.abs(x)) + bs + 2 * EPS * (np.abs(xtx) + np.abs(s))) / nk.sum() \
            + np.abs(cov) * ((bn / nk).max() + 2 * EPS)
        bP = chol_bound(cov, bC, pc)
    else:
        m2 = (resp.T @ (x * x)) / nk[:, None]
        bd = 2 * (n + 2) * EPS * m2 + m2 * (bn / nk + 2 * EPS)[:, None] + 2 * np.abs(mu) * bm + 6 * EPS * (m2 + mu * mu)
        bC = bd if ctype == "diag" else bd.mean(axis=1) + 2 * (D + 1) * EPS * (m2 + mu * mu).mean(axis=1)
        bP = pc * (bC / (2 * cov) + 4 * EPS)
    out.update(covariances=bC, precisions_cholesky=bP)
    return out


TEACHER = [mr.CASES[0], mr.CASES[2], mr.CASES[3]]


@pytest.mark.parametrize("ctype", mr.TYPES)
@pytest.mark.parametrize("case", TEACHER, ids=mr.case_name)
def test_one_estep_and_mstep_teacher_forced(case, ctype, mixture, ref_fits, capsys):
    """The E-step through ``predict`` from the restatement's fitted parameters, the M-step through ``m_step`` from the
    restatement's log_resp; the module docstring holds the bounds and the measured ratios."""
    n, D, K, _ = case
    x, _, _ = mr.make_case(*case)
    f = ref_fits[(mr.case_name(case), ctype)]
    dev = torch.device("cuda")
    model = {"weights": torch.from_numpy(f["weights"][None]).to(dev), "means": torch.from_numpy(f["means"][None]).to(dev),
             "precisions_cholesky": torch.from_numpy(np.ascontiguousarray(f["precisions_cholesky"])[None]).to(dev),
             "k": np.array([K]), "covariance_type": ctype}
    e = mr.estep(x, f["weights"], f["means"], f["precisions_cholesky"], ctype)
    be = estep_bounds(x, f["weights"], f["means"], f["precisions_cholesky"], ctype, e)
    p = mixture.predict(x, model)
    rows = {name: ratio(p[name], e[{"log_prob_norm": "lse"}.get(name, name)], be[name])
            for name in ("log_prob_norm", "log_resp", "resp")}
    rows["score"] = ratio(p["score"], np.array([e["score"]]), be["score"])
    sure = mr.top_two_gap(e["log_resp"]) > 2 * be["log_resp"].max(axis=1)
    assert sure.mean() >= 0.99
    assert np.array_equal(host(p["labels"])[sure], e["labels"][sure])
    w, mu, cov, pc, failed = mr.mstep(x, e["resp"], 1e-6, ctype)
    assert not failed
    bm = mstep_bounds(x, e["resp"], ctype, w, mu, cov, pc)
    m = mixture.m_step(x, e["log_resp"], K, None, ctype, 1e-6)
    assert int(host(m["status"])[0]) == 0
    for name, want in (("weights", w), ("means", mu), ("covariances", cov), ("precisions_cholesky", pc)):
        rows["m_" + name] = ratio(host(m[name])[0], want, bm[name])
    with capsys.disabled():
        print(f"\n  teacher-forced {mr.case_name(case)} {ctype}: " + " ".join(f"{k}={v:.2g}" for k, v in rows.items()))


# ------------------------------------------------------------------------------------------------------ full fits
def sure_rows(log_resp, scale=1.0):
    """Rows whose top-two gap exceeds twice the log_resp allowance (relative to max(1, |log_resp|) of the runner-up)."""
    if log_resp.shape[1] < 2:
        return np.ones(log_resp.shape[0], dtype=bool)
    second = np.sort(log_resp, axis=1)[:, -2]
    return mr.top_two_gap(log_resp) > 2 * scale * MARGIN * FIT_MEASURED["log_resp_rel"] * np.maximum(1.0, np.abs(second))


@pytest.mark.parametrize("ctype", mr.TYPES)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_name)
def test_fit_and_predict_on_the_fixtures(case, ctype, mixture, ref_fits, capsys):
    n, D, K, _ = case
    x, init, _ = mr.make_case(*case)
    f = ref_fits[(mr.case_name(case), ctype)]
    r = mixture.gmm(x, K, None, ctype, init_labels=init)
    assert int(host(r["n_iter"])[0]) == f["n_iter"] and int(host(r["converged"])[0]) == f["converged"]
    assert int(host(r["restart"])[0]) == 0 and int(host(r["status"])[0]) == 0
    rows = {name: deviation(host(r[name])[0], f[name], name) for name in ("lower_bound", "weights", "means", "covariances")}
    rows["precisions_cholesky_rel"] = deviation(host(r["precisions_cholesky"])[0], f["precisions_cholesky"],
                                                "precisions_cholesky_rel")
    rows["score"] = deviation(host(r["score_all"])[0, 0], f["score"], "score")
    rows["bic_rel"] = deviation(host(r["bic"])[0], f["bic"], "bic_rel")
    rows["aic_rel"] = deviation(host(r["aic"])[0], f["aic"], "aic_rel")
    rows["resp"] = deviation(r["resp"], f["resp"], "resp")
    p = mixture.predict(x, r)
    rows["log_resp_rel"] = deviation(p["log_resp"], f["log_resp"], "log_resp_rel")
    rows["log_prob_norm_rel"] = deviation(p["log_prob_norm"], f["lse"], "log_prob_norm_rel")
    with capsys.disabled():
        print(f"\n  fit {mr.case_name(case)} {ctype}: " + " ".join(f"{k}={v:.2g}" for k, v in rows.items()))
    assert_measured(rows)
    sure = sure_rows(f["log_resp"])
    assert sure.all(), "the fixtures leave out no row"
    assert np.array_equal(host(r["labels"])[sure], f["labels"][sure])
    # predict on the training rows is the fit's final E-step, bit for bit
    assert torch.equal(p["labels"], r["labels"]) and torch.equal(p["resp"], r["resp"])
    assert torch.equal(mixture.score_samples(x, r), p["log_prob_norm"])
    assert torch.equal(p["score"], r["score_all"][:, 0])


# ---------------------------------------------------------------------------------------------------- edge shapes
def compare_fit(mixture, x, K, init, ctype, scale=1.0, **kw):
    """Device fit against the restatement: integers equal, floats inside scale x the fits' allowance."""
    f = mr.fit(x, K, init, ctype, tol=kw.get("tol", 1e-3), max_iter=kw.get("max_iter", 100), reg=kw.get("reg_covar", 1e-6))
    r = mixture.gmm(x, K, None, ctype, init_labels=init, **kw)
    assert f["status"] == 0 and int(host(r["status"])[0]) == 0
    assert int(host(r["n_iter"])[0]) == f["n_iter"] and int(host(r["converged"])[0]) == f["converged"]
    rows = {key: deviation(host(r[name])[0], f[name], key)
            for name, key in (("lower_bound", "lower_bound"), ("weights", "weights"), ("means", "means"),
                              ("covariances", "covariances"), ("precisions_cholesky", "precisions_cholesky_rel"),
                              ("bic", "bic_rel"), ("aic", "aic_rel"))}
    print("  edge fit", x.shape, K, ctype, " ".join(f"{k}={v:.2g}" for k, v in rows.items()))
    assert_measured(rows, scale)
    worst = max(err / (scale * MARGIN * FIT_MEASURED[key]) for key, err in rows.items())
    sure = sure_rows(f["log_resp"], scale)
    assert sure.mean() >= 0.99
    assert np.array_equal(host(r["labels"])[sure], f["labels"][sure])
    return r, f, worst


@pytest.mark.parametrize("ctype", mr.TYPES)
def test_edge_n_equals_k_and_two_rows(ctype, mixture):
    """n = K: every covariance is reg_covar alone.  n = 2 with K = 1.  tied at n = K: the covariance is X^T X - sum n_k mu
    mu^T = 0 + rounding, divided into reg_covar: a relative error of eps max |x|^2 / reg_covar ~ 1e-9 where the fixtures
    have ~ 1e-14, hence the allowance x 1e5 there."""
    x, _, _ = mr.make_case(5, 3, 5, 3.0)
    r, f, _ = compare_fit(mixture, x, 5, np.arange(5, dtype=np.int32), ctype, scale=1e5 if ctype == "tied" else 1.0)
    if ctype != "tied":
        c = host(r["covariances"])[0]
        want = {"full": 1e-6 * np.broadcast_to(np.eye(3), (5, 3, 3)), "diag": np.full((5, 3), 1e-6),
                "spherical": np.full(5, 1e-6)}[ctype]
        # diag / spherical: sklearn's avg_X2 - means^2 + reg_covar leaves the rounding of x^2 behind
        assert np.allclose(c, want, rtol=0, atol=1e-18 if ctype == "full" else 16 * EPS * np.abs(x).max() ** 2)
    # two rows, one component: the full / tied scatter has rank 1, the rest is reg_covar (condition number ~ 1e7)
    x2, _, _ = mr.make_case(2, 4, 1, 1.0)
    compare_fit(mixture, x2, 1, np.zeros(2, dtype=np.int32), ctype, scale=1e6 if ctype in ("full", "tied") else 1.0)


@pytest.mark.parametrize("ctype", mr.TYPES)
def test_edge_largest_footprint(ctype, mixture, capsys):
    """D = 64 with K = 64 at n = 130: the largest LDS / workspace footprint; two or three rows per component, so the full
    covariances are reg_covar apart from rank <= 2 (condition number ~ 1e7 - 1e8): the allowance is scaled by 1e6, the
    condition number over that of the fixtures (<= ~ 1e2)."""
    x, _, _ = mr.make_case(130, 64, 64, 3.0)
    init = (np.arange(130) % 64).astype(np.int32)
    _, _, worst = compare_fit(mixture, x, 64, init, ctype, scale=1e6 if ctype in ("full", "tied") else 1.0, max_iter=2)
    with capsys.disabled():
        print(f"\n  D = K = 64, n = 130, {ctype}: largest error / allowance {worst:.2g}")


@pytest.mark.parametrize("ctype", mr.TYPES)
def test_edge_emptied_component(ctype, mixture):
    """No row starts in the last component: n_k = 10 eps, its mean is 0 / 10 eps."""
    x, init, _ = mr.make_case(143, 9, 6, 2.0)
    init = np.where(init == 5, 0, init).astype(np.int32)
    r, f, _ = compare_fit(mixture, x, 6, init, ctype)


def test_edge_ill_defined_covariance_names_the_slide(mixture):
    """reg_covar = 0 with a one-point cluster: the status word, a ValueError naming the slide; the other slides of the batch
    are what they are alone."""
    xs, inits = [], []
    for i, case in enumerate([(40, 3, 3, 4.0), (41, 3, 3, 4.0), (57, 3, 3, 4.0)]):
        x, init, _ = mr.make_case(*case)
        if i == 1:
            init = np.where(init == 2, 0, init).astype(np.int32)
            init[7] = 2
        xs.append(x)
        inits.append(init)
    z, init = np.concatenate(xs), np.concatenate(inits)
    off = [0, 40, 81, 138]
    with pytest.raises(ValueError, match="slide 1: ill-defined"):
        mixture.gmm(z, 3, off, "full", init_labels=init, reg_covar=0.0)
    r = mixture.gmm(z, 3, off, "full", init_labels=init, reg_covar=0.0, check=False)
    assert host(r["status"]).tolist() == [0, 1, 0]
    assert np.isnan(host(r["lower_bound"])[1]) and (host(r["labels"])[40:81] == -1).all()
    assert mr.fit(xs[1], 3, inits[1], "full", reg=0.0)["status"] == 1
    for s in (0, 2):
        one = mixture.gmm(xs[s], 3, None, "full", init_labels=inits[s], reg_covar=0.0)
        assert torch.equal(one["labels"], r["labels"][off[s]:off[s + 1]])
        assert torch.equal(one["resp"], r["resp"][off[s]:off[s + 1]])
        for name in ("weights", "means", "covariances", "precisions_cholesky", "lower_bound", "bic", "n_iter"):
            assert torch.equal(one[name][0], r[name][s]), name


def test_edge_one_large_slide(mixture):
    """One 16 384 x 9, K = 7 slide at max_iter = 3."""
    x, init, _ = mr.make_case(16384, 9, 7, 2.0)
    compare_fit(mixture, x, 7, init, "full", max_iter=3)


# ------------------------------------------------------------------------------------------------ batch invariance
@pytest.mark.parametrize("ctype", mr.TYPES)
def test_batch_invariance_and_reproducibility(ctype, mixture):
    sizes, ks = [2, 17, 257, 1000, 4097], [1, 3, 4, 5, 7]
    xs = [mr.make_case(n, 9, k, 2.0, seed=3)[0] for n, k in zip(sizes, ks)]
    z = np.concatenate(xs)
    off = np.concatenate([[0], np.cumsum(sizes)])
    a = mixture.gmm(z, ks, off, ctype, n_init=2, seed=5, max_iter=8)
    b = mixture.gmm(z, ks, off, ctype, n_init=2, seed=5, max_iter=8)
    names = ("labels", "resp", "weights", "means", "covariances", "precisions_cholesky", "lower_bound", "n_iter", "converged",
             "bic", "aic", "restart", "labels_all", "lower_bound_all", "score_all")
    for name in names:
        assert torch.equal(a[name], b[name]), name                        # two runs
    assert (host(a["status"]) == 0).all()
    for s, (n, k) in enumerate(zip(sizes, ks)):
        one = mixture.gmm(xs[s], k, None, ctype, init_labels=a["init_labels"][:, off[s]:off[s + 1]].contiguous(), max_iter=8)
        assert torch.equal(one["labels"], a["labels"][off[s]:off[s + 1]])
        assert torch.equal(one["resp"][:, :k], a["resp"][off[s]:off[s + 1], :k])
        for name in ("lower_bound", "n_iter", "converged", "bic", "aic", "restart", "lower_bound_all", "score_all"):
            assert torch.equal(one[name][0], a[name][s]), name
        assert torch.equal(one["weights"][0], a["weights"][s, :k]) and torch.equal(one["means"][0], a["means"][s, :k])
        for name in ("covariances", "precisions_cholesky"):
            want = a[name][s] if ctype == "tied" else a[name][s, :k]
            assert torch.equal(one[name][0], want), name


# ---------------------------------------------------------------------------------------------------------- select_k
BIC_GAP = 20.0      # asserted on the restatement's table; it has 23.6 and 29.2 on the two slides (k = 4 is the runner-up)


def test_select_k_picks_the_restatements_k(mixture, capsys):
    """Three well-separated blobs in 2-D, 300 rows, two slides: BIC has a clear minimum at 3."""
    r = np.random.default_rng(11)
    slides = []
    for s in range(2):
        c = np.array([[0.0, 0.0], [8.0, 0.0], [0.0, 8.0]]) + s
        slides.append(np.concatenate([c[i] + r.standard_normal((100, 2)) for i in range(3)]))
    z = np.concatenate(slides)
    off = [0, 300, 600]
    cand = [1, 2, 3, 4, 5]
    res = mixture.select_k(z, cand, off, n_init=2, seed=1)
    assert res["table"].shape == (2, 5) and len(res["fits"]) == 1, "every candidate in one call"
    fit = res["fits"][0]
    init = host(fit["init_labels"])
    table = np.empty((2, 5))
    for ci, k in enumerate(cand):
        for s in range(2):
            seg = ci * 2 + s
            sl = slice(int(fit["offsets"][seg]), int(fit["offsets"][seg + 1]))
            fs = [mr.fit(slides[s], k, init[rr, sl], "full") for rr in range(2)]
            best = max(range(2), key=lambda rr: (fs[rr]["lower_bound"], -rr))
            table[s, ci] = fs[best]["bic"]
    order = np.sort(table, axis=1)
    gap = order[:, 1] - order[:, 0]
    assert (np.argmin(table, axis=1) == 2).all() and (gap >= BIC_GAP).all(), (table, gap)
    assert res["k"].tolist() == [3, 3]
    assert np.abs(res["table"] - table).max() <= BIC_GAP / 4, "a quarter of the gap cannot move the pick"
    m = res["model"]
    assert torch.equal(m["labels"], torch.cat([fit["labels"][1200:1500], fit["labels"][1500:1800]]))
    p = mixture.predict(z, m, off)
    assert torch.equal(p["labels"], m["labels"]) and torch.equal(p["resp"], m["resp"])
    with capsys.disabled():
        print(f"\n  select_k: restatement BIC gap to the runner-up per slide {gap.tolist()}")


# ---------------------------------------------------------------------------------------------------------- validity
def validity_case(n, D, kind, seed=0):
    r = np.random.default_rng([seed, n, D])
    x = r.standard_normal((n, D)) * 2.0 + 3.0
    if kind == "two":
        lab = np.arange(n) % 2
    elif kind == "many":                          # up to 1024 label values, singletons among them
        lab = r.integers(0, 1024, n)
        lab[0] = 1023
        if n >= 2048:
            lab[:1024] = np.arange(1024)          # all 1024 label values
    elif kind == "dropped":
        lab = r.integers(0, 5, n)
        lab[r.random(n) < 0.2] = -1
        lab[:3] = [0, 1, 4]
        lab[3] = 777                              # a cluster of one row
    elif kind == "one":
        lab = np.full(n, 3)
    else:                                         # every row its own cluster
        lab = np.arange(n) % 1024
    return x, lab.astype(np.int32)


VALIDITY = [(2, 3, "two"), (3, 1, "two"), (17, 9, "dropped"), (257, 9, "dropped"), (300, 64, "many"), (1000, 17, "many"),
            (4097, 9, "dropped"), (4097, 9, "many"), (40, 3, "one"), (40, 3, "each")]


@pytest.mark.parametrize("n,D,kind", VALIDITY)
def test_validity(n, D, kind, mixture, capsys):
    x, lab = validity_case(n, D, kind)
    w = mr.validity(x, lab)
    v = mixture.validity(x, lab)
    s = host(v["silhouette_samples"])
    if kind in ("one", "each") or n == 2:
        assert np.isnan(w["silhouette"]), "the restatement refuses it too"
        assert np.isnan(s).all() and np.isnan(v["silhouette"][0]) and np.isnan(v["calinski_harabasz"][0]) \
            and np.isnan(v["davies_bouldin"][0])
        return
    b = 4 * (n + D + 8) * EPS
    kept = lab >= 0
    rms = np.sqrt(max(np.var(x[kept], axis=0).sum(), 1e-300))
    bc = 8 * (n + D + 8) * EPS * (1 + np.abs(x).max() / rms)
    rows = {"silhouette_samples": ratio(s, w["silhouette_samples"], b),
            "silhouette": ratio(v["silhouette"], np.array([w["silhouette"]]), b),
            "calinski_harabasz": ratio(v["calinski_harabasz"], np.array([w["calinski_harabasz"]]),
                                       bc * w["calinski_harabasz"]),
            "davies_bouldin": ratio(v["davies_bouldin"], np.array([w["davies_bouldin"]]), bc * w["davies_bouldin"])}
    assert np.array_equal(np.isnan(s), ~kept)
    if kind == "dropped":
        assert s[3] == 0.0
    with capsys.disabled():
        print(f"\n  validity n = {n}, D = {D}, {kind}: " + " ".join(f"{k}={r:.2g}" for k, r in rows.items())
              + ("  (bit-equal)" if not any(rows.values()) else ""))


def test_validity_batch_is_the_slides_alone(mixture):
    parts = [validity_case(n, 9, kind) for n, kind in ((2, "two"), (257, "dropped"), (40, "one"), (1000, "many"))]
    z, lab = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])])
    v = mixture.validity(z, lab, off)
    for i, (x, l) in enumerate(parts):
        one = mixture.validity(x, l)
        assert np.array_equal(host(one["silhouette_samples"]), host(v["silhouette_samples"][off[i]:off[i + 1]]),
                              equal_nan=True)
        for name in ("silhouette", "calinski_harabasz", "davies_bouldin"):
            assert np.array_equal(one[name], v[name][i:i + 1], equal_nan=True), name


# ------------------------------------------------------------------------------- slides end to end, cluster(), CLI
@pytest.fixture(scope="module")
def slides():
    from mclstexp_amd import synth
    return [synth.make_cluster_case(n, 120, k, seed=s, sep=3.0) for s, (n, k) in enumerate([(300, 3), (420, 4)])]


def test_cluster_slides_method_gmm(mixture, slides):
    from mclstexp_amd import cluster
    preds, labels = [c["pred"] for c in slides], [c["label"] for c in slides]
    km = cluster.cluster_slides(preds, labels, n_init=2, seed=3)
    gm = cluster.cluster_slides(preds, labels, n_init=2, seed=3, method="gmm")
    with pytest.raises(ValueError, match="method"):
        cluster.cluster_slides(preds, labels, method="mclust")
    for i, (c, a, b) in enumerate(zip(slides, km["slides"], gm["slides"])):
        idx, codes, k = cluster.encode_labels(c["label"])
        assert b["k"] == k and b["p"].shape == a["p"].shape and b["p"].min() >= 0 and b["p"].max() < k
        assert np.isnan(b["inertia"]) and np.isfinite(b["lower_bound"]) and np.isfinite(b["bic"])
        # the same pipeline by hand: PCA scores -> k-means starts -> mixture
        z = cluster.pca_scores(c["pred"][idx])
        st = cluster.kmeans(z, k, n_init=2, seed=3, segment_base=i)
        want = mixture.gmm(z, k, init_labels=st["labels_all"])
        assert np.array_equal(host(want["labels"]), b["p"])
        ari, nmi = cluster.cluster_scores(codes, b["p"])
        assert b["ari_raw"] == float(ari[0]) and b["nmi_raw"] == float(nmi[0])
        assert b["ari"] > 0.5, "well-separated synthetic domains are recovered"
    p, ari, nmi = cluster.cluster(preds[0], labels[0], n_init=2, seed=3, method="gmm")
    assert np.array_equal(p, gm["slides"][0]["p"]) and ari == gm["slides"][0]["ari"]


def test_domains_slides_and_cli(mixture, slides, tmp_path):
    preds = [c["pred"] for c in slides]
    r = np.random.default_rng(0)
    trues = [p + 0.05 * r.standard_normal(p.shape) for p in preds]
    res = mixture.domains_slides(preds, trues, k_range=(2, 5), n_init=2, seed=1)
    for c, s in zip(slides, res["slides"]):
        n = c["pred"].shape[0]
        assert 2 <= s["k"] <= 5 and s["labels"].shape == (n,) and s["proba"].shape == (n, s["k"])
        assert np.allclose(s["proba"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.array_equal(np.argmax(s["proba"], axis=1), s["labels"])
        for name in ("bic", "silhouette", "calinski_harabasz", "davies_bouldin", "ari", "nmi", "true_bic"):
            assert np.isfinite(s[name]), name
        assert -1.0 <= s["silhouette"] <= 1.0 and 0.0 <= s["nmi"] <= 1.0
    fixed = mixture.domains_slides(preds, k=[3, 4], n_init=2, seed=1)
    assert [s["k"] for s in fixed["slides"]] == [3, 4] and "ari" not in fixed["slides"][0]
    # the CLI in a fresh process: files written, the printed numbers are the API's
    files = []
    for i, (p, t) in enumerate(zip(preds, trues)):
        files.append((str(tmp_path / f"p{i}.npy"), str(tmp_path / f"t{i}.npy")))
        np.save(files[-1][0], p)
        np.save(files[-1][1], t)
    out_dir = tmp_path / "out"
    cmd = [sys.executable, "-m", "mclstexp_amd.mixture", "--pred", *[f[0] for f in files], "--true", *[f[1] for f in files],
           "--k_range", "2", "5", "--n_init", "2", "--seed", "1", "--out_dir", str(out_dir)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == mixture.format_report(res)
    for i, s in enumerate(res["slides"]):
        assert np.array_equal(np.load(out_dir / str(i) / "gmm_labels.npy"), s["labels"])
        assert np.array_equal(np.load(out_dir / str(i) / "gmm_proba.npy"), s["proba"])
