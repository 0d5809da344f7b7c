"""The device eigensolver on the MI355X (mclstexp_amd.eig, csrc/eig.hip) against numpy.linalg.eigh inside the method's
backward-error bounds (tests/eig_reference.py states them), its determinism, and the PCA that uses it
(``cluster.pca_device(solver="device")``) against sklearn's results (tests/golden/cluster.npz).  pytest -m gpu."""
import numpy as np
import pytest
import torch

import cluster_reference as cr
import eig_reference as er
from mclstexp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = tuple(f"m{m}" for m in er.SIZES) + er.SPECTRA + ("zero",)
DEGENERATE = ("rank30", "pairs", "close", "diag10", "zero")      # only the spanned subspace is compared
assert set(CASES) == set(er.SEPARATED) | set(DEGENERATE)


@pytest.fixture(scope="module")
def eg():
    from mclstexp_amd import _lib, eig
    _lib.lib()  # must load: no fallback
    return eig


@pytest.fixture(scope="module")
def matrices():
    g = np.load(er.GOLDEN)
    return {n: er.unpack(g[f"{n}.a"]) for n in CASES}


@pytest.fixture(scope="module")
def numpy_eigh(matrices):
    """numpy's full decomposition of every case, descending, computed once."""
    out = {}
    for n, a in matrices.items():
        w, v = np.linalg.eigh(a)
        out[n] = (w[::-1].copy(), v[:, ::-1].copy())
    return out


def _h(t):
    return t.cpu().numpy()


def _run(eg, a, k, **kw):
    res = eg.eigh_top(a, k, **kw)
    return _h(res["values"])[0], _h(res["vectors"][0]), res["certificate"][0]


# ------------------------------------------------------------------------------------------------ 1. against numpy
@pytest.mark.parametrize("name", CASES)
def test_eigenpairs_against_numpy(eg, matrices, numpy_eigh, name):
    a = matrices[name]
    m = a.shape[0]
    w, v = numpy_eigh[name]
    norm2 = max(abs(w[0]), abs(w[-1]))
    bl, br, bo = er.bounds(m, norm2)
    for k in er.counts(m):
        lam, z, cert = _run(eg, a, k)
        assert lam.shape == (k,) and z.shape == (m, k)
        dl = np.abs(lam - w[:k]).max()
        res = np.sqrt(((a @ z - z * lam) ** 2).sum(axis=0)).max()
        orth = np.abs(z.T @ z - np.eye(k)).max()
        print(f"{name} m {m} k {k}: |dlam| {dl:.2e} / {bl:.2e}  residual {res:.2e} / {br:.2e}  orthogonality {orth:.2e} / "
              f"{bo:.2e}  certificate {cert[0]:.2e} {cert[1]:.2e} / {64 * m * er.EPS:.2e}")
        assert (np.diff(lam) <= 0).all(), "descending"
        assert dl <= bl and res <= br and orth <= bo
        assert er.sign_rule_holds(z) and np.array_equal(er.fix_signs(z), z)
        assert (cert <= 64.0 * m * er.EPS).all()
        if name in er.SEPARATED:
            # both this solver's and numpy's vector carry a residual <= 4 m eps |A|: each is within residual / gap of the
            # true eigenvector (gap: the distance to the nearest other eigenvalue), together 8 m eps |A| / gap
            for i in range(k):
                gap = np.abs(np.delete(w, i) - w[i]).min() if m > 1 else np.inf
                ref = v[:, i] * (1.0 if v[:, i] @ z[:, i] >= 0 else -1.0)
                err = np.sqrt(((z[:, i] - ref) ** 2).sum())
                assert err <= 8.0 * m * er.EPS * norm2 / gap, (name, k, i, err, gap)
        else:
            # the subspace of the leading kk <= k vectors, kk the largest count that does not cut a cluster (the gap
            # below it is >= 1e-3 |A|): Davis-Kahan with the residual matrix's norm <= sqrt(kk) x the largest residual,
            # for both bases: |P_Z - P_V|_2 <= 8 m eps |A| sqrt(kk) / gap; and each basis is orthonormal to 4 m eps per
            # entry of Z^T Z - I, kk x that in the 2-norm
            kk = max([c for c in range(1, min(k, m - 1) + 1) if w[c - 1] - w[c] >= 1e-3 * norm2 > 0.0] + ([k] if k == m else [0]))
            if kk:
                gap = w[kk - 1] - w[kk] if kk < m else np.inf
                diff = np.linalg.norm(z[:, :kk] @ z[:, :kk].T - v[:, :kk] @ v[:, :kk].T, 2)
                print(f"    subspace of the first {kk}: |P_Z - P_V|_2 = {diff:.2e}, gap {gap:.2e}")
                assert diff <= 8.0 * m * er.EPS * norm2 * np.sqrt(kk) / gap + 8.0 * m * er.EPS * kk, (name, k, kk, diff)


def test_largest_order_with_the_most_pairs(eg):
    """m = 4096, k = 64: the full LDS column of the back-transformation, 16 rows per thread in the Gram-Schmidt kernel, about
    12 300 launches.  A = H_u H_v diag(w) H_v H_u with two Householder reflectors, so the spectrum w = 1 .. 4096 and the
    eigenvectors H_u H_v e_i are known without a host eigh of this size; forming A rounds every entry a few times, which moves
    an eigenvalue by a few eps |A|_F <= a few sqrt(m) eps |A|_2, far inside 4 m eps |A|_2.  The 64 leading eigenvalues are
    1 / 4096 of |A| apart: all of them share one Gram-Schmidt group."""
    m, k = 4096, 64
    rng = np.random.default_rng(4096)
    w = np.arange(float(m), 0.0, -1.0)                       # descending
    q = np.eye(m)
    for _ in range(2):
        u = rng.standard_normal(m)
        u /= np.sqrt(u @ u)
        q -= 2.0 * np.outer(q @ u, u)                        # q <- q H_u
    a = (q * w) @ q.T
    a = 0.5 * (a + a.T)
    lam, z, cert = _run(eg, torch.from_numpy(a).to(DEV), k, overwrite=True)
    bl, br, bo = er.bounds(m, float(m))
    dl = np.abs(lam - w[:k]).max()
    res = np.sqrt(((a @ z - z * lam) ** 2).sum(axis=0)).max()
    orth = np.abs(z.T @ z - np.eye(k)).max()
    print(f"m {m} k {k}: |dlam| {dl:.2e} / {bl:.2e}  residual {res:.2e} / {br:.2e}  orthogonality {orth:.2e} / {bo:.2e}  "
          f"certificate {cert[0]:.2e} {cert[1]:.2e} / {64 * m * er.EPS:.2e}")
    assert dl <= bl and res <= br and orth <= bo
    assert er.sign_rule_holds(z)
    assert (cert <= 64.0 * m * er.EPS).all()
    ref = q[:, :k] * np.where((q[:, :k] * z).sum(axis=0) < 0, -1.0, 1.0)
    err = np.sqrt(((z - ref) ** 2).sum(axis=0)).max()
    print(f"    vectors against H_u H_v e_i: {err:.2e} / {8.0 * m * er.EPS * m / 1.0:.2e}")
    assert err <= 8.0 * m * er.EPS * float(m) / 1.0          # 8 m eps |A|_2 / gap, gap = 1


def test_host_and_device_inputs_of_either_width_agree(eg, matrices):
    a = matrices["m65"]
    lam, z, _ = _run(eg, a, 9)
    lam_d, z_d, _ = _run(eg, torch.from_numpy(a).to(DEV), 9)
    assert lam.tobytes() == lam_d.tobytes() and z.tobytes() == z_d.tobytes()
    a32 = a.astype(np.float32)
    a32 = np.maximum(a32, a32.T)                                     # exactly symmetric in fp32
    lam32, z32, _ = _run(eg, a32, 9)
    want, zw, _ = _run(eg, a32.astype(np.float64), 9)
    assert lam32.tobytes() == want.tobytes() and z32.tobytes() == zw.tobytes()
    lam32d, z32d, _ = _run(eg, torch.from_numpy(a32).to(DEV), 9)
    assert lam32d.tobytes() == want.tobytes() and z32d.tobytes() == zw.tobytes()


# ---------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("sizes,k", [(er.BATCH, 2), ((17, 130, 65), 9), ((64, 130), 64)])
def test_slide_inside_a_batch_is_bit_identical_to_the_slide_alone(eg, matrices, sizes, k):
    mats = [matrices[f"m{m}"] for m in sizes]
    flat_h = np.concatenate([a.reshape(-1) for a in mats])
    flat = torch.from_numpy(flat_h).to(DEV)
    res = eg.eigh_top(flat, k, sizes=sizes)
    assert np.array_equal(_h(flat), flat_h), "overwrite=False leaves the input as it was"
    assert tuple(res["values"].shape) == (len(sizes), k) and res["certificate"].shape == (len(sizes), 2)
    again = eg.eigh_top(flat, k, sizes=sizes)
    assert _h(res["values"]).tobytes() == _h(again["values"]).tobytes(), "run to run"
    for s, a in enumerate(mats):
        assert tuple(res["vectors"][s].shape) == (a.shape[0], k)
        assert _h(res["vectors"][s]).tobytes() == _h(again["vectors"][s]).tobytes(), "run to run"
        lam, z, cert = _run(eg, a, k)
        assert _h(res["values"])[s].tobytes() == lam.tobytes(), (s, "values")
        assert _h(res["vectors"][s]).tobytes() == z.tobytes(), (s, "vectors")
        assert res["certificate"][s].tobytes() == cert.tobytes(), (s, "certificate")
    over = eg.eigh_top(flat, k, sizes=sizes, overwrite=True)
    assert _h(over["values"]).tobytes() == _h(res["values"]).tobytes()
    assert not np.array_equal(_h(flat), flat_h), "overwrite=True works in place"


def test_certificate_guard_names_the_slide(eg, matrices):
    bad = np.full((17, 17), np.nan)
    flat = torch.from_numpy(np.concatenate([matrices["m17"].reshape(-1), bad.reshape(-1)])).to(DEV)
    with pytest.raises(RuntimeError, match="slide 1"):
        eg.eigh_top(flat, 3, sizes=[17, 17])


# ----------------------------------------------------------------------------------------------------------- 3. PCA
@pytest.fixture(scope="module")
def cl():
    from mclstexp_amd import cluster
    return cluster


@pytest.fixture(scope="module")
def cluster_golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {n: synth.make_cluster_case(**kw) for n, kw in cr.CLUSTER_CASES.items()}


@pytest.fixture
def no_host_eigh(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("numpy.linalg.eigh was called: the device solver must not go through the host")
    monkeypatch.setattr(np.linalg, "eigh", refuse)


@pytest.mark.parametrize("name", sorted(cr.CLUSTER_CASES))
def test_pca_with_the_device_solver_against_fixture(cl, cluster_golden, cases, no_host_eigh, name):
    x, _, _ = cr.kept(cases[name])
    ref = cluster_golden[f"{name}.scores"]
    res = cl.pca_device(x, solver="device")
    z = _h(res["scores"])
    err = np.abs(cr.align_signs(z, ref) - ref).max()
    print(f"{name}: n {x.shape[0]} G {x.shape[1]} max|dZ| / max|Z| = {err / np.abs(ref).max():.2e}")
    assert err <= 1e-9 * np.abs(ref).max()
    assert cr.sign_rule_holds(x, z), "the loading of largest magnitude must be positive"
    ev = res["explained_variance"][0]
    assert np.abs(ev - cluster_golden[f"{name}.explained_variance"]).max() <= 1e-9 * ev.max()


def test_cluster_slides_with_the_device_solver(cl, cluster_golden, cases, no_host_eigh):
    res = cl.cluster_slides([cases[n]["pred"] for n in cr.SLIDES], [cases[n]["label"] for n in cr.SLIDES],
                            seed_rows=[cluster_golden[f"{n}.seed_rows"] for n in cr.SLIDES], solver="device")
    for s, n in zip(res["slides"], cr.SLIDES):
        assert np.array_equal(s["p"], cluster_golden[f"{n}.labels"]), n
        assert (s["ari"], s["nmi"]) == (float(cluster_golden[f"{n}.ari"]), float(cluster_golden[f"{n}.nmi"]))
    assert res["ari"] == float(np.mean([float(cluster_golden[f"{n}.ari"]) for n in cr.SLIDES]))


def test_device_pca_launches_own_kernels_only(cl, cases, no_host_eigh):
    from mclstexp_amd import kernel_audit
    xs = [cr.kept(cases[n])[0] for n in cr.SLIDES]
    cl.pca_scores_slides(xs, solver="device")   # warm-up
    ks = kernel_audit.step_kernels(lambda: cl.pca_scores_slides(xs, solver="device"))
    assert not kernel_audit.foreign(ks), kernel_audit.foreign(ks)
    for want in ("pca_mean_kernel", "pca_gram_kernel", "eig_setup_kernel", "eig_house_kernel", "eig_symv_kernel",
                 "eig_rank2_kernel", "eig_bisect_kernel", "eig_factor_kernel", "eig_solve_kernel", "eig_ortho_kernel",
                 "eig_cert_kernel", "eig_cert_reduce_kernel", "eig_back_kernel", "pca_loadings_kernel", "pca_sign_kernel",
                 "pca_scores_kernel"):
        assert any(want in k for k in ks), (want, sorted(ks))
