"""GPU: csrc/tsne.hip through mclstexp_amd.tsne against the numpy restatement (tests/tsne_reference.py) on the cases of
tests/golden/tsne.npz: teacher-forced affinities, gradient and update, short trajectories, determinism, and full runs
bounded by sklearn's own final KL.  Comparisons with the restatement allow 4 x the uncertainty the fixture recorded for that
quantity; the elementwise update step allows the roundings its formula has.

On an MI355X, with the KL formed as sum K_i + log(sum Q) sum p', test_joint_probabilities and test_gradient_and_kl[a-d]
passed and test_gradient_and_kl[e] missed at Y0, plain: KL 5.03e-16 of the 4.44e-16 allowed (gradient 1.28e-15 of 1.15e-14).
numpy gives the same 5.03e-16 for that form; the per-row form ts_finish_kernel now uses gives 1.26e-16 there in numpy and
stays inside every case's bound.  The kernel in that form, and the tests below test_gradient_and_kl, have not yet run on
an MI355X."""
import numpy as np
import pytest
import torch

import tsne_reference as tr
from mclstexp_amd import cluster, tsne

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(tr.GOLDEN)


@pytest.fixture(scope="module")
def ref(z):
    """name -> {f32: [(P, beta) per segment]} of the restatement, computed once."""
    out = {}
    for name, (sizes, _, perplexity) in tr.CASES.items():
        off = tr.offsets_of(name)
        X = np.asarray(z[f"{name}_X"], dtype=np.float64)
        out[name] = {f32: [tr.joint_probabilities(X[off[s]:off[s + 1]], perplexity, f32) for s in range(len(sizes))]
                     for f32 in (False, True)}
    return out


def _segments(res):
    """[(P_s, beta_s)] as numpy from a joint_probabilities result."""
    P, beta = res["P"].cpu().numpy(), res["beta"].cpu().numpy()
    off, poff = res["offsets"], res["pair_offsets"]
    return [(P[poff[s]:poff[s + 1]].reshape(off[s + 1] - off[s], -1), beta[off[s]:off[s + 1]])
            for s in range(off.size - 1)]


# ---------------------------------------------------------------------------------------------------- teacher-forced
@pytest.mark.parametrize("f32", (False, True), ids=("f64dist", "f32dist"))
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_joint_probabilities(z, ref, name, f32):
    res = tsne.joint_probabilities(z[f"{name}_X"], tr.offsets_of(name), tr.CASES[name][2], float32_distances=f32)
    tag = "f32" if f32 else "f64"
    tol_P, tol_b = 4 * float(z[f"err_{name}_P_{tag}"]), 4 * float(z[f"err_{name}_beta_{tag}"])
    for (P, beta), (P_ref, beta_ref) in zip(_segments(res), ref[name][f32]):
        print(name, tag, "P", tr.rel(P, P_ref), "of", tol_P, "beta", tr.rel(beta, beta_ref), "of", tol_b)
        assert np.array_equal(P, P.T) and not P.diagonal().any()
        assert tr.rel(P, P_ref) <= tol_P
        assert tr.rel(beta, beta_ref) <= tol_b


@pytest.mark.parametrize("name", tr.SINGLE)
def test_gradient_and_kl(z, ref, name):
    P = ref[name][True][0][0]
    for where in ("Y0", "Ymid"):
        for ex, tag in ((1.0, "plain"), (12.0, "exag")):
            Y = z[f"{name}_{where}"]
            g, kl = tsne.gradient(P, Y, None, ex)
            g_ref, kl_ref, _ = tr.gradient(P, Y, ex)
            eg, ek = tr.rel(g.cpu().numpy(), g_ref), abs(float(kl.cpu()[0]) - kl_ref) / abs(kl_ref)
            print(name, where, tag, "grad", eg, "of", 4 * float(z[f"err_{name}_grad_{where}_{tag}"]), "kl", ek, "of",
                  4 * float(z[f"err_{name}_kl_{where}_{tag}"]))
            assert eg <= 4 * float(z[f"err_{name}_grad_{where}_{tag}"])
            assert ek <= 4 * float(z[f"err_{name}_kl_{where}_{tag}"])
    g, kl = tsne.gradient(torch.from_numpy(P).cuda(), z[f"{name}_Y0"], None, 1.0, kl=False)
    assert kl is None and tr.rel(g.cpu().numpy(), tr.gradient(P, z[f"{name}_Y0"], 1.0)[0]) <= 4 * float(
        z[f"err_{name}_grad_Y0_plain"])


def test_gradient_of_a_batch_with_one_exaggeration_per_segment(z, ref):
    off = tr.offsets_of("f")
    Ps = [p for p, _ in ref["f"][False]]
    Y = z["f_Y0"] * 1e3
    ex = [1.0, 12.0, 4.0]
    g, kl = tsne.gradient(np.concatenate([p.ravel() for p in Ps]), Y, off, ex)
    g, kl = g.cpu().numpy(), kl.cpu().numpy()
    for s in range(3):                                   # each segment is the same slide alone, bit for bit
        g1, kl1 = tsne.gradient(Ps[s], Y[off[s]:off[s + 1]], None, ex[s])
        assert np.array_equal(g[off[s]:off[s + 1]], g1.cpu().numpy()) and kl[s] == float(kl1.cpu()[0])
        assert np.abs(g1.cpu().numpy()).max() > 0 and np.isfinite(kl[s])


@pytest.mark.parametrize("name", "ac")
def test_one_update_step(z, name):
    """From a recorded (Y, grad, update, gains) state; the step is elementwise, so the bound is a few roundings."""
    Y, g, u, ga = z[f"{name}_Ymid"], z[f"{name}_step_grad"], z[f"{name}_step_update"], z[f"{name}_step_gains"]
    for momentum, lr in ((0.5, 50.0), (0.8, 200.0)):
        want = tr.step(Y, g, u, ga, momentum, lr)
        got = tsne.update(Y, g, u, ga, None, momentum, lr)
        assert np.array_equal(got[2].cpu().numpy(), want[2])                       # gains: exact
        assert tr.rel(got[1].cpu().numpy(), want[1]) <= 4 * 2.0 ** -52
        assert tr.rel(got[0].cpu().numpy(), want[0]) <= 4 * 2.0 ** -52
        terms = 2 * Y.shape[0]                         # a sum of positive terms in another order: (terms - 1) roundings
        assert abs(float(got[3].cpu()[0]) - want[3]) <= terms * 2.0 ** -53 * want[3]


# -------------------------------------------------------------------------------------------------- short trajectory
@pytest.mark.parametrize("name", tr.SINGLE)
def test_short_trajectory(z, ref, name):
    L = int(z[f"{name}_trajectory_len"])
    want = tr.run(ref[name][False][0][0], z[f"{name}_Y0"], L, keep=(1, 10, L))
    for k in (1, 10, L):
        res = tsne.tsne(z[f"{name}_X"], perplexity=tr.CASES[name][2], init=z[f"{name}_Y0"], n_iter=k)
        e = tr.rel(res["embedding"].cpu().numpy(), want["trace"][k])
        print(name, "iteration", k, e, "of", 4 * float(z[f"err_{name}_Y{k}"]))
        assert e <= 4 * float(z[f"err_{name}_Y{k}"])
        assert res["n_iter"].tolist() == [k] and np.isfinite(res["kl_divergence"]).all()


# ------------------------------------------------------------------------------------------------------- determinism
def test_batch_is_bit_identical_to_its_slides_and_to_its_repeat(z):
    X, off, perplexity = z["f_X"], tr.offsets_of("f"), tr.CASES["f"][2]
    assert X.dtype == np.float32
    wide = torch.zeros((X.shape[0], 16), dtype=torch.float32)
    wide[:, :9] = torch.from_numpy(X)
    strided = wide.cuda()[:, :9]                                     # fp32 on the device with a row stride of 16
    kw = dict(perplexity=perplexity, init=z["f_Y0"], n_iter=120)
    a = tsne.tsne(strided, off, **kw)
    b = tsne.tsne(strided, off, **kw)
    c = tsne.tsne(X.astype(np.float64), off, **kw)                   # the same values, contiguous fp64 from the host
    Ya = a["embedding"].cpu().numpy()
    assert np.isfinite(Ya).all() and np.abs(Ya).max() > 1e-3
    for other in (b, c):
        assert np.array_equal(Ya, other["embedding"].cpu().numpy())
        assert np.array_equal(a["beta"].cpu().numpy(), other["beta"].cpu().numpy())
        assert np.array_equal(a["kl_divergence"], other["kl_divergence"])
    for s in range(3):
        lo, hi = off[s], off[s + 1]
        alone = tsne.tsne(X[lo:hi], None, perplexity=perplexity, init=z["f_Y0"][lo:hi], n_iter=120)
        assert np.array_equal(alone["embedding"].cpu().numpy(), Ya[lo:hi]), s
        assert alone["kl_divergence"][0] == a["kl_divergence"][s]


# ---------------------------------------------------------------------------------------------------------- full run
@pytest.mark.parametrize("name", "bc")
def test_full_run_reaches_sklearns_kl(z, name):
    res = tsne.tsne(z[f"{name}_X"], perplexity=tr.CASES[name][2], init=z[f"{name}_Y0"], n_iter=1000)
    bound = float(z[f"{name}_full_kl"].mean()) * (1.0 + 2.0 * float(z[f"{name}_full_spread"]))
    print(name, "KL", res["kl_divergence"], "bound", bound, "n_iter", res["n_iter"])
    assert res["kl_divergence"][0] <= bound
    assert 250 < int(res["n_iter"][0]) <= 1000
    Y = res["embedding"].cpu().numpy()
    assert tr.nn_purity(Y, z[f"{name}_labels"].astype(np.int64)) == 1.0
    # the reported KL belongs to the embedding before its last step: the KL of the returned one is within the
    # run-to-run spread of it (a single late step moves it by far less than four starts 1e-6 apart do)
    kl = float(tsne.gradient(tsne.joint_probabilities(z[f"{name}_X"], None, tr.CASES[name][2])["P"], Y)[1].cpu()[0])
    assert abs(kl - res["kl_divergence"][0]) <= float(z[f"{name}_full_spread"]) * kl


@pytest.fixture(scope="module")
def slides():
    rng = np.random.RandomState(4)
    out = []
    for n in (90, 75):
        centres = 5.0 * rng.standard_normal((3, 40))
        lab = np.arange(n) % 3
        out.append(((centres[lab] + rng.standard_normal((n, 40))).astype(np.float32), lab))
    return out


def test_embed_slides(slides):
    res = tsne.embed_slides([x for x, _ in slides], perplexity=15.0, n_iter=300)
    assert [tuple(y.shape) for y in res["slides"]] == [(90, 2), (75, 2)] and res["offsets"].tolist() == [0, 90, 165]
    assert torch.isfinite(res["embedding"]).all() and np.isfinite(res["kl_divergence"]).all()
    for y, (_, lab) in zip(res["slides"], slides):
        assert tr.nn_purity(y.cpu().numpy(), lab) == 1.0
    rnd = tsne.embed_slides([x for x, _ in slides], perplexity=15.0, n_iter=60, init="random", random_state=2)
    assert torch.isfinite(rnd["embedding"]).all()


def test_cluster_slides_with_tsne_changes_nothing_else(slides):
    preds = [x for x, _ in slides]
    labels = [np.array(["x", "y", "undetermined"])[lab] for _, lab in slides]
    seeds = [np.array([0, 1]), np.array([0, 1])]
    plain = cluster.cluster_slides(preds, labels, seed_rows=seeds)
    with_t = cluster.cluster_slides(preds, labels, seed_rows=seeds, tsne={"perplexity": 10.0, "n_iter": 100})
    for a, b, (_, lab) in zip(plain["slides"], with_t["slides"], slides):
        assert "tsne" not in a and b["tsne"].shape == (int((lab != 2).sum()), 2) and np.isfinite(b["tsne"]).all()
        assert np.array_equal(a["p"], b["p"]) and a["ari_raw"] == b["ari_raw"] and a["nmi_raw"] == b["nmi_raw"]
        assert a["ari"] == b["ari"] and a["nmi"] == b["nmi"]
    assert plain["ari"] == with_t["ari"] and plain["nmi"] == with_t["nmi"]
    p, ari, nmi, emb = cluster.cluster(preds[0], labels[0], seed_rows=seeds[0], tsne={"perplexity": 10.0, "n_iter": 60})
    assert (ari, nmi) == (plain["slides"][0]["ari"], plain["slides"][0]["nmi"]) and emb.shape == (60, 2)
