"""GPU: mclstexp_amd.deconv against ``scipy.optimize.nnls`` (tests/golden/deconv.npz; the inputs are regenerated from
their seeds) and the numpy restatement tests/deconv_reference.py.

The coefficient bound is the perturbation bound of the normal equations under the rounding of c, 4 (G + T) eps || |S| |x_i|
||_2 / lambda_min(A), with lambda_min from ``numpy.linalg.eigvalsh``; it is asserted for every spot of every case, none
left out.  The cases are the smallest shapes at which the kernels can go wrong: T = 1; odd G below one MFMA tile; G a tile
multiple; T not a multiple of 16; T at the limit (with kappa_2(A) about 3e6 and without); G < 2 T.  The r2 tolerance, which
the bound above does not cover, is the rounding of the residual's sum of squares taken in two orders
(``deconv_reference.r2_bound``)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deconv_reference as dr
from conftest import GOLDEN_DIR, ROOT
from mclstexp_amd import _lib
from mclstexp_amd import deconv as dc

pytestmark = pytest.mark.gpu
IDS = [dr.case_name(*c) for c in dr.CASES]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "deconv.npz"))


@pytest.fixture(scope="module")
def runs():
    """{case: (S, x, the device's result)}: every case solved once."""
    out = {}
    for c in dr.CASES:
        S, x = dr.make_case(c[0], c[1], c[2], dr.case_seed(*c[:3]), c[3])
        out[c] = (S, x, dc.nnls(x, S))
    return out


def same(a, b, what=""):
    for key in dc.KEYS:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (what, key)


# ----------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("case", dr.CASES, ids=IDS)
def test_coef_within_the_bound_of_scipy_and_kkt(case, runs, golden):
    S, x, got = runs[case]
    T = case[1]
    want = golden[f"{dr.case_name(*case)}.coef"]
    err, bound = np.abs(got["coef"] - want).max(axis=1), dr.coef_bound(x, S)
    print(f"{dr.case_name(*case)}: worst |coef - scipy| / bound = {float((err[bound > 0] / bound[bound > 0]).max()):.4f}, "
          f"n_iter max {int(got['n_iter'].max())}")
    assert got["coef"].shape == want.shape and got["coef"].dtype == np.float64
    assert (err <= bound).all(), int(np.argmax(err - bound))
    dr.check_kkt(x, S, got["coef"])
    assert got["converged"].dtype == np.uint8 and (got["converged"] == 1).all()
    assert got["n_iter"].dtype == np.int32 and (got["n_iter"] <= 3 * T).all() and (got["n_iter"][2:] >= 1).all()


@pytest.mark.parametrize("case", dr.CASES, ids=IDS)
def test_other_outputs(case, runs, golden):
    S, x, got = runs[case]
    G, T = case[0], case[1]
    bound = dr.coef_bound(x, S)
    assert (np.abs(got["rnorm"] - golden[f"{dr.case_name(*case)}.rnorm"]) <= dr.rnorm_bound(x, S)).all()
    q = np.einsum("ij,ij->i", x, x)
    rnorm, r2, prop, dom = dr.residual(x, S, got["coef"], q)
    tol = dr.r2_bound(x, S, got["coef"], q)
    assert np.isnan(got["r2"][0]) and (np.abs(got["r2"][1:] - r2[1:]) <= tol[1:]).all()
    assert (np.abs(got["proportions"] - prop) <= 4 * T * dr.EPS).all()
    top2 = np.sort(prop, axis=1)[:, -2:] if T > 1 else np.concatenate([np.zeros_like(prop), prop], axis=1)
    clear = (top2[:, 1] - top2[:, 0] > 4 * T * dr.EPS) | (dom < 0)
    assert got["dominant"].dtype == np.int32 and np.array_equal(got["dominant"][clear], dom[clear])
    # the special rows: all zero, all negative, a vertex
    assert (got["coef"][:2] == 0.0).all() and (got["dominant"][:2] == -1).all() and (got["proportions"][:2] == 0.0).all()
    assert (got["n_iter"][:2] == 0).all() and got["rnorm"][0] == 0.0
    assert abs(got["coef"][2, 0] - 1.0) <= bound[2] and got["dominant"][2] == 0


def test_gram_and_factor(runs):
    S, x, _ = runs[dr.CASES[5]]
    d = dc.nnls_device(x, S)
    A, L = d["gram"].cpu().numpy(), d["cholesky"].cpu().numpy()
    T, G = S.shape
    assert np.array_equal(A, A.T)
    assert (np.abs(A - S @ S.T) <= 2 * G * dr.EPS * (np.abs(S) @ np.abs(S).T)).all()
    assert (np.triu(L, 1) == 0).all() and (np.abs(L @ L.T - A) <= 4 * T * dr.EPS * np.sqrt(np.outer(np.diag(A), np.diag(A)))).all()
    c, q, _ = dr.products(x, S)
    assert (np.abs(d["c"].cpu().numpy() - c) <= 2 * G * dr.EPS * (np.abs(x) @ np.abs(S).T)).all()
    assert (np.abs(d["q"].cpu().numpy() - q) <= 2 * G * dr.EPS * q).all()
    for t in (1, 2, 8, 20, 33, 47, 64):
        assert _lib.call("mcl_nnls_solve_waves", t) == dr.solve_waves(t)


def test_fp32_input_with_a_leading_dimension(runs, golden):
    """x is exactly representable in fp32: converted on load it is the same fp64 matrix, so every output is bit-identical
    to the fp64 run; the three columns behind G hold NaN and are never read."""
    case = dr.CASES[3]
    S, x, got = runs[case]
    n, G = x.shape
    padded = np.full((n, G + 3), np.nan, dtype=np.float32)
    padded[:, :G] = x
    assert np.array_equal(padded[:, :G].astype(np.float64), x)
    same(dc.nnls(padded, S, ld=G + 3), got, "host fp32")
    xt = torch.from_numpy(padded).cuda()
    same(dc.nnls(xt, S, ld=G + 3), got, "device fp32")
    same(dc.nnls(xt[:, :G], torch.from_numpy(S).cuda()), got, "a strided device view")
    with pytest.raises(ValueError, match="expected"):
        dc.nnls(padded, S)


def test_slides_of_2_37_and_986_rows_in_one_call(golden):
    G, T, n, col = dr.SLIDES_CASE
    S, x = dr.make_case(G, T, n, dr.case_seed(G, T, n), col)
    cuts = np.concatenate([[0], np.cumsum(dr.SLIDES)])
    assert cuts[-1] == n == 1025
    res = dc.deconvolve_slides([x[a:b] for a, b in zip(cuts[:-1], cuts[1:])], S)
    whole = dc.nnls(x, S)
    want, bound = golden[f"{dr.case_name(*dr.SLIDES_CASE)}.coef"], dr.coef_bound(x, S)
    for s, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        same(res[s], {key: v[a:b] for key, v in whole.items()}, f"slide {s}")
        assert (np.abs(res[s]["coef"] - want[a:b]).max(axis=1) <= bound[a:b]).all()
    dr.check_kkt(x, S, whole["coef"])
    assert whole["converged"].all()


# ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("case", [dr.CASES[1], dr.CASES[5]], ids=[IDS[1], IDS[5]])
def test_bit_identical_again_alone_and_permuted(case, runs):
    S, x, got = runs[case]
    same(dc.nnls(x, S), got, "second run")
    for i in (0, 1, 2, 3, x.shape[0] // 2, x.shape[0] - 1):
        same(dc.nnls(x[i:i + 1], S), {key: v[i:i + 1] for key, v in got.items()}, f"spot {i} alone")
    perm = np.random.default_rng(0).permutation(x.shape[0])
    same(dc.nnls(x[perm], S), {key: v[perm] for key, v in got.items()}, "permuted rows")


# ---------------------------------------------------------------------------------------------- errors, not faults
@pytest.fixture()
def launched(monkeypatch):
    names = []

    def spy(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(dc, "call", spy)
    return names


def test_bad_signatures_and_spots_are_value_errors(runs, launched):
    S, x, _ = runs[dr.CASES[3]]
    dup = S.copy()
    dup[7] = dup[4]
    with pytest.raises(ValueError, match="type 7 "):
        dc.nnls(x, dup)
    zero = S.copy()
    zero[3] = 0.0
    with pytest.raises(ValueError, match="type 3 "):
        dc.nnls(x, zero)
    nan = S.copy()
    nan[11, 170] = np.nan
    with pytest.raises(ValueError, match="type 11 holds a non-finite"):
        dc.nnls(x, nan)
    inf = S.copy()
    inf[0, 0] = np.inf
    with pytest.raises(ValueError, match="type 0 holds a non-finite"):
        dc.nnls(x, inf)
    bad = x.copy()
    bad[150, 3] = np.nan
    bad[77, 170] = np.inf
    with pytest.raises(ValueError, match="row 77 "):
        dc.nnls(bad, S)
    assert "mcl_nnls_gram" in launched and "mcl_nnls_solve" not in launched and "mcl_nnls_residual" not in launched
    with pytest.raises(ValueError, match="types"):
        dc.nnls(np.zeros((4, 70)), np.ones((65, 70)))
    with pytest.raises(ValueError, match="genes"):
        dc.nnls(np.zeros((4, 19)), np.ones((20, 19)))
    assert len(launched) == 10
    dc.nnls(x[:5], S)
    assert launched[-4:] == ["mcl_nnls_gram", "mcl_nnls_products", "mcl_nnls_solve", "mcl_nnls_residual"]


# ------------------------------------------------------------------------------------------------------------ chain
def planted(seed=0):
    """Two slides whose spots are their group's profile plus noise that cancels within every group pooled over both."""
    rng = np.random.default_rng(seed)
    K, G, pairs = 4, 31, 40
    P = rng.gamma(2.0, 1.0, size=(K, G)) + 0.1
    rows, labs = [], []
    for g in range(K):
        e = 0.3 * rng.standard_normal((pairs + 3 * g, G))
        rows += [P[g] + e, P[g] - e]
        labs += [np.full(2 * e.shape[0], g)]
    x, lab = np.concatenate(rows), np.concatenate(labs)
    order = rng.permutation(x.shape[0])
    x, lab = x[order], lab[order]
    cut = 131
    names = np.array(["tumour", "stroma", "immune", "fat"])[lab]
    return P, [x[:cut], x[cut:]], [lab[:cut], lab[cut:]], [names[:cut], names[cut:]]


def test_signatures_from_groups_recovers_planted_profiles():
    P, mats, labs, names = planted()
    S, cats = dc.signatures_from_groups(mats, labs)
    assert cats.tolist() == [0, 1, 2, 3] and np.abs(S - P).max() <= 1e-12
    drop = [v.astype("U12") for v in names]
    drop[0][:5] = "undetermined"
    keep = [np.ones(v.size, dtype=bool) for v in names]
    keep[0][:5] = False
    S2, cats2 = dc.signatures_from_groups(mats, drop)
    assert cats2.tolist() == ["fat", "immune", "stroma", "tumour"]
    x, lab = np.concatenate([m[k] for m, k in zip(mats, keep)]), np.concatenate([v[k] for v, k in zip(names, keep)])
    want = np.stack([x[lab == c].mean(axis=0) for c in cats2])
    assert np.abs(S2 - want).max() <= 1e-12
    with pytest.raises(ValueError, match="occurs on no slide"):
        dc.signatures_from_groups(mats, [np.where(v == 1, 5, v) for v in labs])


def test_recovery_of_the_truth_by_itself_is_perfect():
    P, mats, labs, _ = planted()
    rec = dc.deconvolution_recovery(mats, mats, P)
    varies = np.stack([r["proportions"].std(axis=0) > 0 for r in rec["true"]])
    assert varies.any() and (np.abs(rec["pearson"][varies] - 1.0) <= 1e-12).all() and np.isnan(rec["pearson"][~varies]).all()
    assert (rec["dominant_agreement"] == 1.0).all() and (rec["rmse"] == 0.0).all()
    assert abs(rec["mean_pearson"] - 1.0) <= 1e-12 and rec["mean_dominant_agreement"] == 1.0 and rec["mean_rmse"] == 0.0
    # the planted groups dominate their spots
    agree = np.mean(np.concatenate([r["dominant"] for r in rec["true"]]) == np.concatenate(labs))
    assert agree > 0.9
    assert dc.top_types(rec["true"], 0, 2).shape == (2,)


def test_cli_writes_the_file_and_prints_the_recovery_line(tmp_path):
    P, mats, labs, _ = planted()
    rng = np.random.default_rng(3)
    args = [sys.executable, "-m", "mclstexp_amd.deconv", "--pred"]
    for kind in ("pred", "true", "labels"):
        if kind != "pred":
            args.append(f"--{kind}")
        for i, (m, lab) in enumerate(zip(mats, labs)):
            path = str(tmp_path / f"{kind}{i}.npy")
            np.save(path, lab if kind == "labels" else (m + (0.05 * rng.standard_normal(m.shape) if kind == "pred" else 0)).T)
            args.append(path)
    out = tmp_path / "out"
    r = subprocess.run(args + ["--out_dir", str(out), "--top", "2"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("slide 0 n = 131 ") and lines[-1].startswith("recovery: mean Pearson ")
    assert float(lines[-1].split("mean dominant agreement ")[1].split(",")[0]) > 0.9
    for i, m in enumerate(mats):
        z = np.load(out / str(i) / dc.OUT_FILE)
        assert z["coef"].shape == (m.shape[0], 4) and z["signatures"].shape == (4, 31) and z["types"].tolist() == ["0", "1", "2", "3"]
        assert set(dc.KEYS) <= set(z.files)
