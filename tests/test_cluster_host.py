"""CPU: the host side of mclstexp_amd.cluster -- argument validation before any launch, the C entry points' checks, the CLI
-- and the in-test fp64 restatement (tests/cluster_reference.py) against sklearn's own results for the reference's
cluster() (tests/golden/cluster.npz)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_reference as cr
from mclstexp_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.mark.parametrize("name", sorted(cr.CLUSTER_CASES))
def test_restatement_matches_reference_fixture(golden, name):
    z = golden
    x, labels, _ = cr.kept(synth.make_cluster_case(**cr.CLUSTER_CASES[name]))
    scores, ev, _ = cr.pca_scores(x)
    ref = z[f"{name}.scores"]
    assert scores.shape == ref.shape
    assert np.abs(cr.align_signs(scores, ref) - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.array_equal(np.sign(scores[0]), np.sign(ref[0])), "sign rule differs from sklearn's"
    assert cr.sign_rule_holds(x, scores)
    assert np.abs(ev - z[f"{name}.explained_variance"]).max() <= 1e-10 * ev.max()
    rows = z[f"{name}.seed_rows"]
    for tol, key in ((1e-4, ""), (0.0, "tol0_")):
        got = cr.lloyd(ref, ref[rows], tol)
        assert np.array_equal(got["labels"], z[f"{name}.{key}labels"]), (name, tol)
        assert got["n_iter"] == int(z[f"{name}.{key}n_iter"])
        assert abs(got["inertia"] - float(z[f"{name}.{key}inertia"])) <= 1e-12 * got["inertia"]
        assert np.abs(got["centers"] - z[f"{name}.{key}centers"]).max() <= 1e-12 * np.abs(ref).max()
    ari, nmi = cr.ari_nmi(labels, z[f"{name}.labels"])
    assert abs(ari - float(z[f"{name}.ari_raw"])) <= 1e-12 and abs(nmi - float(z[f"{name}.nmi_raw"])) <= 1e-12
    assert round(ari, 3) == float(z[f"{name}.ari"]) and round(nmi, 3) == float(z[f"{name}.nmi"])


def test_restatement_scores_match_the_hand_made_pairs(golden):
    for i, (name, a, b) in enumerate(cr.label_pairs()):
        ari, nmi = cr.ari_nmi(a, b)
        assert abs(ari - golden["pairs.ari"][i]) <= 1e-12, name
        assert abs(nmi - golden["pairs.nmi"][i]) <= 1e-12, name


def test_fixture_holds_arrays_only_and_covers_both_pca_forms(golden):
    for k in golden.files:
        assert golden[k].dtype.kind in "fi", k
    shapes = {n: (int((synth.make_cluster_case(**kw)["label"] != "undetermined").sum()), kw["genes"])
              for n, kw in cr.CLUSTER_CASES.items()}
    assert any(n >= g for n, g in shapes.values()) and any(n < g for n, g in shapes.values())
    assert float(golden["sep.ari"]) == 1.0
    assert [round(float(golden[f"{n}.ari"]), 2) for n in cr.NOISY] == [0.88, 0.71, 0.58, 0.3, 0.22]


def test_make_cluster_case():
    d = synth.make_cluster_case(200, 50, 4, seed=9, sep=0.5, undetermined_frac=0.25)
    assert d["pred"].shape == (200, 50) and d["pred"].dtype == np.float64 and (d["pred"] >= 0).all()
    und = d["label"] == "undetermined"
    assert 20 < und.sum() < 80
    assert np.array_equal(d["label"][~und].astype(np.int64), d["truth"][~und])
    again = synth.make_cluster_case(200, 50, 4, seed=9, sep=0.5, undetermined_frac=0.25)
    assert np.array_equal(d["pred"], again["pred"]) and np.array_equal(d["label"], again["label"])


def test_entry_points_reject_bad_arguments_before_any_launch():
    from mclstexp_amd import _lib
    lib = _lib.load()
    P = C.c_void_p(64)   # never dereferenced: every call below must be rejected on the host

    def gram(x=P, ld=8, dt=1, off=P, S=2, G=8, mr=5, goff=P, mean=P, g=P):
        return lib.mcl_pca_gram(x, ld, dt, off, S, G, mr, goff, mean, g, None)

    for kw in ({"x": None}, {"off": None}, {"goff": None}, {"mean": None}, {"g": None}, {"S": 0}, {"G": 0}, {"mr": 0},
               {"ld": 7}, {"dt": 2}):
        assert gram(**kw) == -1, kw
    assert gram(S=70000) == -2

    def proj(x=P, ld=8, dt=0, off=P, S=1, G=8, mr=5, nc=3, mean=P, ev=P, eoff=P, ew=P, ld_=P, sg=P, z=P):
        return lib.mcl_pca_project(x, ld, dt, off, S, G, mr, nc, mean, ev, eoff, ew, ld_, sg, z, None)

    for kw in ({"x": None}, {"off": None}, {"mean": None}, {"ev": None}, {"eoff": None}, {"ew": None}, {"ld_": None},
               {"sg": None}, {"z": None}, {"nc": 0}, {"ld": 3}, {"dt": -1}, {"S": 0}):
        assert proj(**kw) == -1, kw
    assert proj(nc=65) == -2

    def km(z=P, ld=9, off=P, S=1, rows=100, D=9, k=P, kmax=4, R=1, seeds=None, seed=0, base=0, tol=1e-4, it=300,
           so=P, la=P, ca=P, ia=P, na=P, work=P, lab=P, cen=P, ine=P, nit=P, rs=P):
        return lib.mcl_kmeans(z, ld, off, S, rows, D, k, kmax, R, seeds, seed, base, tol, it, so, la, ca, ia, na, work,
                              lab, cen, ine, nit, rs, None)

    for kw in ({"z": None}, {"off": None}, {"k": None}, {"so": None}, {"la": None}, {"ca": None}, {"ia": None},
               {"na": None}, {"work": None}, {"lab": None}, {"cen": None}, {"ine": None}, {"nit": None}, {"rs": None},
               {"S": 0}, {"rows": 0}, {"D": 0}, {"kmax": 0}, {"R": 0}, {"ld": 8}, {"it": 0}, {"tol": -1.0},
               {"tol": float("nan")}):
        assert km(**kw) == -1, kw
    assert km(D=65, ld=65) == -2 and km(kmax=65) == -2

    def sc(a=P, b=P, off=P, S=1, mr=10, out=P):
        return lib.mcl_cluster_scores(a, b, off, S, mr, out, None)

    for kw in ({"a": None}, {"b": None}, {"off": None}, {"out": None}, {"S": 0}, {"mr": 0}):
        assert sc(**kw) == -1, kw
    assert sc(mr=50001) == -2


@pytest.fixture
def fake_gpu(monkeypatch):
    """Argument checks run before the device is asked for: with validation passing, the next thing is the missing GPU."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_python_validation_raises_before_any_launch(fake_gpu):
    from mclstexp_amd import cluster
    z = np.zeros((20, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.kmeans(z, 3)
    for off in ([0, 5, 19], [1, 20], [0, 10, 10, 20], [0.0, 20.0], [[0, 20]]):
        with pytest.raises(ValueError):
            cluster.kmeans(z, 3, offsets=off)
    with pytest.raises(ValueError, match="exceeds"):
        cluster.kmeans(z, [3, 9], offsets=[0, 12, 20])           # k > n_s in the second segment
    with pytest.raises(ValueError):
        cluster.kmeans(z, 65)                                      # K > 64
    with pytest.raises(ValueError):
        cluster.kmeans(np.zeros((200, 65)), 3)                     # D > 64
    with pytest.raises(ValueError):
        cluster.kmeans(z, [3, 3])                                  # one k per segment
    with pytest.raises(ValueError):
        cluster.kmeans(z, 3, seed_rows=np.array([0, 5, 20]))       # a seed row outside the segment
    with pytest.raises(ValueError):
        cluster.kmeans(z, 3, seed_rows=np.array([0, 5]))           # fewer seed rows than clusters
    with pytest.raises(ValueError):
        cluster.kmeans(z, 3, tol=-1.0)
    with pytest.raises(ValueError):
        cluster.kmeans(np.zeros(20), 3)
    with pytest.raises(ValueError, match="length"):
        cluster.cluster_scores(np.zeros(5, dtype=np.int64), np.zeros(6, dtype=np.int64))
    with pytest.raises(ValueError):
        cluster.pca_scores(np.zeros((30, 12)), n_comps=65)
    with pytest.raises(ValueError):
        cluster.pca_scores(np.zeros((9, 12)), n_comps=9)           # needs more than n_comps spots
    with pytest.raises(ValueError):
        cluster.pca_scores(np.zeros((30, 12)), offsets=[0, 31])
    with pytest.raises(ValueError):
        cluster.cluster(np.zeros((10, 12)), np.array(["a"] * 9))   # one label per spot
    with pytest.raises(ValueError):
        cluster.cluster(np.zeros((10, 12)), np.array(["undetermined"] * 10))
    with pytest.raises(ValueError):
        cluster.cluster_slides([np.zeros((10, 12))], [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.cluster(np.zeros((40, 12)), np.array(["a", "b"] * 20))


def test_label_values_are_checked_on_the_host(monkeypatch):
    import torch
    from mclstexp_amd import cluster
    dev = torch.device("cpu")
    with pytest.raises(ValueError):
        cluster._labels_i32(np.array([0, 1024]), "a", dev)
    with pytest.raises(ValueError):
        cluster._labels_i32(np.array([-1, 3]), "a", dev)
    with pytest.raises(ValueError):
        cluster._labels_i32(np.array([0.0, 1.0]), "a", dev)
    assert cluster._labels_i32(np.array([0, 1023]), "a", dev).dtype == torch.int32


def test_encode_labels_is_the_reference_bookkeeping():
    from mclstexp_amd import cluster
    lab = np.array(["tumor", "undetermined", "fat", "tumor", "immune", "undetermined"])
    idx, codes, k = cluster.encode_labels(lab)
    assert idx.tolist() == [True, False, True, True, True, False]
    assert k == len(set(lab[idx])) == 3
    assert codes.tolist() == [2, 0, 2, 1] and codes.dtype == np.int32
    idx, codes, k = cluster.encode_labels(np.array([3, 1, 3, 7]))          # integer labels: nothing is 'undetermined'
    assert idx.all() and k == 3 and codes.tolist() == [1, 0, 1, 2]


def test_seed_rows_layouts():
    from mclstexp_amd import cluster
    seg = np.array([10, 8])
    ks = np.array([3, 2], dtype=np.int32)
    a = cluster._seed_array([np.array([[0, 1, 2], [3, 4, 5]]), np.array([[7, 6], [0, 1]])], ks, seg)
    assert a.shape == (2, 2, 3) and a[1, 0].tolist() == [7, 6, 0] and a[0, 1].tolist() == [3, 4, 5]
    assert cluster._seed_array(np.array([4, 5, 6]), ks[:1], seg[:1]).tolist() == [[[4, 5, 6]]]
    assert cluster._seed_array([np.array([4, 5, 6])], ks[:1], seg[:1]).tolist() == [[[4, 5, 6]]]
    with pytest.raises(ValueError):
        cluster._seed_array([np.array([0, 1, 2])], ks, seg)                # one entry for two segments


def test_cli_arguments_and_help():
    from mclstexp_amd import cluster
    a = cluster.parse_args(["--pred", "p1.npy", "p2.npy", "--labels", "l1.npy", "l2.npy", "--n_init", "8"])
    assert (a.pred, a.labels, a.n_init, a.json, a.n_comps) == (["p1.npy", "p2.npy"], ["l1.npy", "l2.npy"], 8, None, 9)
    for bad in (["--pred", "p.npy"], ["--labels", "l.npy"], ["--pred", "a.npy", "b.npy", "--labels", "l.npy"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(bad)
    proc = subprocess.run([sys.executable, "-m", "mclstexp_amd.cluster", "--help"], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "--n_init" in proc.stdout and "--labels" in proc.stdout
    txt = cluster.format_report({"slides": [{"ari": 0.381, "nmi": 0.429}, {"ari": 1.0, "nmi": 0.5}], "ari": 0.6905,
                                 "nmi": 0.4645})
    assert txt.splitlines() == ["ARI: 0.381, NMI: 0.429", "ARI: 1.0, NMI: 0.5", "mean ARI: 0.691, mean NMI: 0.465"]
