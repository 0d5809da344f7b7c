"""Spatial-domain clustering on the MI355X (mclstexp_amd.cluster, csrc/cluster.hip) against sklearn's results for the
reference's cluster() (tests/golden/cluster.npz) and the fp64 restatement (tests/cluster_reference.py).  pytest -m gpu."""
import numpy as np
import pytest
import torch

import cluster_reference as cr
from mclstexp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def cl():
    from mclstexp_amd import _lib, cluster
    _lib.lib()  # must load: no fallback
    return cluster


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {n: synth.make_cluster_case(**kw) for n, kw in cr.CLUSTER_CASES.items()}


def _h(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. PCA
@pytest.mark.parametrize("name", sorted(cr.CLUSTER_CASES))
def test_pca_scores_against_fixture(cl, golden, cases, name):
    x, _, _ = cr.kept(cases[name])
    ref = golden[f"{name}.scores"]
    res = cl.pca_device(x)
    z = _h(res["scores"])
    err = np.abs(cr.align_signs(z, ref) - ref).max()
    print(f"{name}: n {x.shape[0]} G {x.shape[1]} ({'primal' if x.shape[0] >= x.shape[1] else 'dual'}) "
          f"max|dZ| / max|Z| = {err / np.abs(ref).max():.2e}")
    assert err <= 1e-9 * np.abs(ref).max()
    assert cr.sign_rule_holds(x, z), "the loading of largest magnitude must be positive"
    ev = res["explained_variance"][0]
    assert np.abs(ev - golden[f"{name}.explained_variance"]).max() <= 1e-9 * ev.max()


def test_pca_hits_both_forms(cases):
    shapes = [cr.kept(cases[n])[0].shape for n in cr.CLUSTER_CASES]
    assert any(n >= g for n, g in shapes) and any(n < g for n, g in shapes)


# ------------------------------------------------------------------------------------------------- 2. k-means replay
@pytest.mark.parametrize("tol,key", [(1e-4, ""), (0.0, "tol0_")])
@pytest.mark.parametrize("name", sorted(cr.CLUSTER_CASES))
def test_kmeans_replays_the_reference_run(cl, golden, name, tol, key):
    z = golden[f"{name}.scores"]
    k = int(cr.CLUSTER_CASES[name]["k"])
    res = cl.kmeans(z, k, seed_rows=golden[f"{name}.seed_rows"], tol=tol)
    want_inertia = float(golden[f"{name}.{key}inertia"])
    got_inertia = float(res["inertia"][0])
    print(f"{name} tol {tol}: n_iter {int(res['n_iter'][0])} inertia rel "
          f"{abs(got_inertia - want_inertia) / want_inertia:.2e}")
    assert np.array_equal(_h(res["labels"]), golden[f"{name}.{key}labels"])
    assert int(res["n_iter"][0]) == int(golden[f"{name}.{key}n_iter"])
    assert abs(got_inertia - want_inertia) <= 1e-12 * want_inertia
    assert np.abs(_h(res["centers"])[0] - golden[f"{name}.{key}centers"]).max() <= 1e-12 * np.abs(z).max()
    assert np.array_equal(_h(res["seed_rows"])[0, 0], golden[f"{name}.seed_rows"])
    assert int(res["restart"][0]) == 0


def test_kmeans_segmented_replay(cl, golden):
    """Three fixture cases stacked, each with its own k: every segment equals the reference's run."""
    zs = [golden[f"{n}.scores"] for n in cr.SEGMENTED]
    off = np.concatenate([[0], np.cumsum([z.shape[0] for z in zs])])
    ks = [cr.CLUSTER_CASES[n]["k"] for n in cr.SEGMENTED]
    res = cl.kmeans(np.concatenate(zs), ks, offsets=off, seed_rows=[golden[f"{n}.seed_rows"] for n in cr.SEGMENTED])
    lab = _h(res["labels"])
    for s, n in enumerate(cr.SEGMENTED):
        assert np.array_equal(lab[off[s]:off[s + 1]], golden[f"{n}.labels"]), n
        assert int(res["n_iter"][s]) == int(golden[f"{n}.n_iter"])
        assert abs(float(res["inertia"][s]) - float(golden[f"{n}.inertia"])) <= 1e-12 * float(golden[f"{n}.inertia"])
        assert np.abs(_h(res["centers"])[s, :ks[s]] - golden[f"{n}.centers"]).max() <= 1e-12 * np.abs(zs[s]).max()


# --------------------------------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("name", sorted(cr.CLUSTER_CASES))
def test_cluster_end_to_end(cl, golden, cases, name):
    d = cases[name]
    p, ari, nmi = cl.cluster(d["pred"], d["label"], seed_rows=golden[f"{name}.seed_rows"])
    print(f"{name}: ARI: {ari}, NMI: {nmi}")
    assert np.array_equal(p, golden[f"{name}.labels"]), "no relabelling: the same seed rows give the same numbering"
    assert (ari, nmi) == (float(golden[f"{name}.ari"]), float(golden[f"{name}.nmi"]))


def test_cluster_slides_end_to_end(cl, golden, cases):
    res = cl.cluster_slides([cases[n]["pred"] for n in cr.SLIDES], [cases[n]["label"] for n in cr.SLIDES],
                            seed_rows=[golden[f"{n}.seed_rows"] for n in cr.SLIDES])
    for s, n in zip(res["slides"], cr.SLIDES):
        assert np.array_equal(s["p"], golden[f"{n}.labels"]), n
        assert (s["ari"], s["nmi"]) == (float(golden[f"{n}.ari"]), float(golden[f"{n}.nmi"]))
        assert abs(s["ari_raw"] - float(golden[f"{n}.ari_raw"])) <= 1e-12
    assert res["ari"] == float(np.mean([float(golden[f"{n}.ari"]) for n in cr.SLIDES]))


# -------------------------------------------------------------------------------------------------------- 4. scores
def test_cluster_scores_hand_made_pairs(cl, golden):
    for i, (name, a, b) in enumerate(cr.label_pairs()):
        ari, nmi = cl.cluster_scores(a, b)
        assert abs(ari[0] - golden["pairs.ari"][i]) <= 1e-12, (name, ari[0], golden["pairs.ari"][i])
        assert abs(nmi[0] - golden["pairs.nmi"][i]) <= 1e-12, (name, nmi[0], golden["pairs.nmi"][i])


def test_cluster_scores_case_labelings_segmented(cl, golden, cases):
    names = sorted(cr.CLUSTER_CASES)
    truth = [cr.kept(cases[n])[2] for n in names]
    pred = [golden[f"{n}.labels"] for n in names]
    off = np.concatenate([[0], np.cumsum([t.size for t in truth])])
    ari, nmi = cl.cluster_scores(np.concatenate(truth), np.concatenate(pred), off)
    for s, n in enumerate(names):
        assert abs(ari[s] - float(golden[f"{n}.ari_raw"])) <= 1e-12, n
        assert abs(nmi[s] - float(golden[f"{n}.nmi_raw"])) <= 1e-12, n
        one = cl.cluster_scores(truth[s], torch.from_numpy(pred[s]).to(DEV))
        assert (one[0][0], one[1][0]) == (ari[s], nmi[s]), "a segment alone is bit-identical"


def test_cluster_scores_outside_the_domain_is_nan(cl):
    a = torch.arange(200, dtype=torch.int32, device=DEV)            # 200 x 200 classes: beyond the LDS table
    ari, nmi = cl.cluster_scores(a, a)
    assert np.isnan(ari[0]) and np.isnan(nmi[0])
    bad = torch.tensor([0, 5000, 1], dtype=torch.int32, device=DEV)  # a device label outside [0, 1024)
    ari, nmi = cl.cluster_scores(bad, bad)
    assert np.isnan(ari[0]) and np.isnan(nmi[0])


# --------------------------------------------------------------------------------------------------- 5. own seeding
def _bits(res, keys=("labels", "centers", "inertia", "n_iter", "restart", "inertia_all", "seed_rows")):
    return [_h(res[k]).tobytes() for k in keys]


def test_own_seeding_is_reproducible_and_selects_the_best_restart(cl, golden):
    z = golden["c1500.scores"]
    a = cl.kmeans(z, 10, n_init=8, seed=3)
    assert _bits(a) == _bits(cl.kmeans(z, 10, n_init=8, seed=3)), "run to run"
    assert _bits(a) != _bits(cl.kmeans(z, 10, n_init=8, seed=4)), "the seed matters"
    all_in = _h(a["inertia_all"])[0]
    r = int(a["restart"][0])
    assert float(a["inertia"][0]) == all_in.min() and r == int(np.argmin(all_in))
    assert np.array_equal(_h(a["labels"]), _h(a["labels_all"])[r])
    rows = _h(a["seed_rows"])[0]
    assert rows.shape == (8, 10) and rows.min() >= 0 and rows.max() < z.shape[0]
    assert all(len(set(rr.tolist())) == 10 for rr in rows), "k-means++ never picks a row twice"
    assert len({tuple(rr.tolist()) for rr in rows}) > 1, "restarts draw different seeds"
    # identical restarts (given seed rows) tie: the lowest r wins
    same = np.tile(golden["c1500.seed_rows"], (3, 1))
    t = cl.kmeans(z, 10, seed_rows=same)
    assert int(t["restart"][0]) == 0 and len(set(_h(t["inertia_all"])[0].tolist())) == 1


def test_slide_inside_a_batch_is_bit_identical_to_the_slide_alone(cl, cases):
    preds = [cases[n]["pred"] for n in cr.SLIDES]
    labels = [cases[n]["label"] for n in cr.SLIDES]
    batch = cl.cluster_slides(preds, labels, n_init=4, seed=5)
    assert [s["p"].tobytes() for s in batch["slides"]] == \
        [s["p"].tobytes() for s in cl.cluster_slides(preds, labels, n_init=4, seed=5)["slides"]]
    for i in range(3):   # the generator is keyed by the segment's number: segment_base places the lone slide
        alone = cl.cluster_slides([preds[i]], [labels[i]], n_init=4, seed=5, segment_base=i)["slides"][0]
        got = batch["slides"][i]
        assert alone["p"].tobytes() == got["p"].tobytes(), i
        for k in ("ari_raw", "nmi_raw", "inertia", "n_iter", "restart"):
            assert alone[k] == got[k], (i, k)


def test_own_seeding_on_the_separable_case(cl, golden, cases):
    z = golden["sep.scores"]
    truth = cr.kept(cases["sep"])[2]
    res = cl.kmeans(z, 4, n_init=8, seed=0)
    for r in range(8):
        ari, _ = cl.cluster_scores(truth, _h(res["labels_all"])[r])
        assert ari[0] == 1.0, (r, ari[0])


@pytest.mark.parametrize("name", cr.NOISY)
def test_own_seeding_best_of_8_against_sklearn(cl, golden, name):
    """Best-of-8 inertia of the kernel's own k-means++ <= 1.02 x the fixture's (sklearn, random_state=0, one run).
    1.02: sklearn's own k-means++ with 20 independent sets of 8 seeds gave best-of-8 / fixture between 0.990 and 1.0038 on
    these cases, single uniformly seeded runs 1.05 - 1.14; sklearn seeds greedily and the kernel does not, hence the room
    above 1.004.  Measured on the MI355X (seed 0): c346 0.99988, c613 1.00000, c3200 0.99817, c250 0.99906, c1500 0.99365;
    single restarts ranged 0.9936 - 1.0544."""
    z = golden[f"{name}.scores"]
    res = cl.kmeans(z, int(cr.CLUSTER_CASES[name]["k"]), n_init=8, seed=0)
    ratio = float(res["inertia"][0]) / float(golden[f"{name}.inertia"])
    print(f"{name}: best-of-8 / fixture inertia = {ratio:.5f}; per restart "
          f"{np.round(_h(res['inertia_all'])[0] / float(golden[f'{name}.inertia']), 4).tolist()}")
    assert ratio <= 1.02


# ------------------------------------------------------------------------------------ 6. fp32, views, emptied cluster
def test_fp32_input_and_strided_view(cl):
    d = synth.make_cluster_case(333, 150, 5, seed=21, sep=0.3, undetermined_frac=0.0)
    x32 = d["pred"].astype(np.float32)
    want, _, _ = cr.pca_scores(x32)
    z = _h(cl.pca_scores(x32))
    assert np.abs(cr.align_signs(z, want) - want).max() <= 1e-9 * np.abs(want).max()
    assert cr.sign_rule_holds(x32, z)
    wide = torch.full((333, 163), 7.0, dtype=torch.float64, device=DEV)
    wide[:, :150] = torch.from_numpy(d["pred"])
    view = wide[:, :150]                                     # row-major, leading dimension 163
    want64, _, _ = cr.pca_scores(d["pred"])
    zv = cl.pca_scores(view)
    assert np.array_equal(_h(zv), _h(cl.pca_scores(d["pred"]))), "a view gives the bits of the contiguous matrix"
    assert np.abs(cr.align_signs(_h(zv), want64) - want64).max() <= 1e-9 * np.abs(want64).max()
    # k-means on a strided view of the scores, odd D, against the restatement
    zw = torch.full((333, 12), -3.0, dtype=torch.float64, device=DEV)
    zw[:, :9] = zv
    rows = np.array([5, 77, 140, 201, 310])
    zh = _h(zv)
    ref = cr.lloyd(zh, zh[rows])
    if ref["min_margin"] >= 1e-9:
        got = cl.kmeans(zw[:, :9], 5, seed_rows=rows)
        assert np.array_equal(_h(got["labels"]), ref["labels"]) and int(got["n_iter"][0]) == ref["n_iter"]
        assert abs(float(got["inertia"][0]) - ref["inertia"]) <= 1e-12 * ref["inertia"]
    # odd shapes: two dual segments and one primal one in a call, n_comps 3
    xs = [synth.make_cluster_case(n, 70, 3, seed=30 + n, sep=0.4, undetermined_frac=0.0)["pred"] for n in (17, 129, 64)]
    zz = cl.pca_scores_slides(xs, n_comps=3)
    for x, zi in zip(xs, zz):
        w = cr.pca_scores(x, 3)[0]
        assert np.abs(cr.align_signs(_h(zi), w) - w).max() <= 1e-9 * np.abs(w).max()
        assert np.array_equal(_h(zi), _h(cl.pca_scores(x, n_comps=3))), "a slide alone is bit-identical"


def test_emptied_cluster_is_refilled(cl, golden):
    z = golden["c613.scores"].copy()
    z[10] = z[3]                                              # two seed rows that are the same point
    res = cl.kmeans(z, 4, seed_rows=np.array([3, 10, 200, 400]))
    lab = _h(res["labels"])
    assert sorted(set(lab.tolist())) == [0, 1, 2, 3], "K non-empty clusters"
    assert np.isfinite(float(res["inertia"][0])) and 1 <= int(res["n_iter"][0]) <= 300
    ref = cr.lloyd(z, z[[3, 10, 200, 400]])
    assert ref["ever_empty"]
    if ref["min_margin"] >= 1e-9:
        assert np.array_equal(lab, ref["labels"]) and int(res["n_iter"][0]) == ref["n_iter"]


def test_max_iter_is_reported(cl, golden):
    res = cl.kmeans(golden["c3200.scores"], 7, seed_rows=golden["c3200.seed_rows"], max_iter=5)
    assert int(res["n_iter"][0]) == 5


# --------------------------------------------------------------------------------------------------- 7. own kernels
def test_clustering_launches_own_kernels_only(cl, cases):
    from mclstexp_amd import kernel_audit
    preds = [cases[n]["pred"] for n in cr.SLIDES]
    labels = [cases[n]["label"] for n in cr.SLIDES]
    cl.cluster_slides(preds, labels, n_init=2)   # warm-up
    ks = kernel_audit.step_kernels(lambda: cl.cluster_slides(preds, labels, n_init=2))
    assert not kernel_audit.foreign(ks), kernel_audit.foreign(ks)
    for want in ("pca_mean_kernel", "pca_gram_kernel", "pca_loadings_kernel", "pca_sign_kernel", "pca_scores_kernel",
                 "kmeans_kernel", "kmeans_select_kernel", "cluster_scores_kernel"):
        assert any(want in k for k in ks), (want, sorted(ks))
