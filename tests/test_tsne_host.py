"""CPU: the host side of mclstexp_amd.tsne (argument rules, initialisations, learning rate, stopping schedule, CLI) and the
numpy restatement of DESIGN 6.10 against sklearn's own functions as tests/golden/tsne.npz records them.  Fails where
mclstexp_amd.tsne does not exist."""
import numpy as np
import pytest
import torch

import tsne_reference as tr
from mclstexp_amd import tsne


@pytest.fixture(scope="module")
def z():
    return np.load(tr.GOLDEN)


@pytest.fixture(scope="module")
def joint(z):
    """name -> (P, beta) of the restatement, (float32 distances, fp64 distances)."""
    return {n: (tr.joint_probabilities(z[f"{n}_X"], tr.CASES[n][2], True),
                tr.joint_probabilities(z[f"{n}_X"], tr.CASES[n][2], False)) for n in tr.SINGLE}


@pytest.mark.parametrize("name", tr.SINGLE)
def test_restated_affinities_are_sklearns(z, joint, name):
    """P on float32-rounded distances (sklearn's arithmetic) <= 1e-13 of max P; full matrices for the two smallest
    cases, row sums and a fixed sample of entries for the others."""
    P = joint[name][0][0]
    n = P.shape[0]
    scale = float(z[f"{name}_sk_P_max"])
    C, _ = tr.binary_search(tr.sq_distances(z[f"{name}_X"], True), tr.CASES[name][2])
    if z[f"{name}_sk_P"].ndim == 2:
        got_P, got_C = P, C
    else:
        ii, jj = tr.sample_index(n)
        got_P, got_C = P[ii, jj], C[ii, jj]
    assert np.max(np.abs(got_P - z[f"{name}_sk_P"])) / scale <= 1e-13
    assert np.max(np.abs(got_C - z[f"{name}_sk_C"])) / np.max(z[f"{name}_sk_C"]) <= 1e-13
    assert np.max(np.abs(P.sum(axis=1) - z[f"{name}_sk_P_rowsum"])) / np.max(z[f"{name}_sk_P_rowsum"]) <= 1e-13
    assert np.array_equal(P, P.T) and not P.diagonal().any() and P[~np.eye(n, dtype=bool)].min() >= tr.EPS


def test_float32_rounding_of_distances_matters(z, joint):
    """The two distance modes are different arithmetic (1e-8 .. 1e-6 apart), so the flag is not decoration."""
    for name in "abc":
        (P32, _), (P64, _) = joint[name]
        assert 1e-9 < tr.rel(P32, P64) < 1e-5


@pytest.mark.parametrize("name", tr.SINGLE)
def test_restated_gradient_and_kl_are_sklearns(z, joint, name):
    P = joint[name][0][0]
    for where in ("Y0", "Ymid"):
        for ex, tag in ((1.0, "plain"), (12.0, "exag")):
            g, kl, min_q = tr.gradient(P, z[f"{name}_{where}"], ex)
            assert tr.rel(g, z[f"{name}_sk_grad_{where}_{tag}"]) <= 1e-12, (where, tag)
            assert abs(kl - float(z[f"{name}_sk_kl_{where}_{tag}"])) <= 1e-12 * abs(float(z[f"{name}_sk_kl_{where}_{tag}"]))
            assert min_q > tr.EPS


@pytest.mark.parametrize("name", tr.SINGLE)
def test_restated_trajectory_is_sklearns(z, joint, name):
    """sklearn's own float64 _gradient_descent at iterations 1, 10 and the recorded length, within 4 x the recorded
    uncertainty of the restatement (the trajectories are chaotic: the length is where that stays below 1e-6)."""
    L = int(z[f"{name}_trajectory_len"])
    assert L in (20, 30, 40, 50, 60)
    r = tr.run(joint[name][1][0], z[f"{name}_Y0"], L, keep=(1, 10, L))
    for k in (1, 10, L):
        assert tr.rel(r["trace"][k], z[f"{name}_sk_Y{k}"]) <= 4 * float(z[f"err_{name}_Y{k}"]), k
    assert r["min_q"] > tr.EPS


def test_fixture_holds_the_guards(z):
    for k in z.files:
        if k.startswith("err_"):
            limit = 1e-6 if "_Y" in k and not k.endswith(("_Y1", "_Y10")) and "grad" not in k and "kl" not in k else 1e-11
            assert 2.0 ** -53 <= float(z[k]) <= limit, k
    assert int(z["clamp_checks"]) > 8000
    for name in "bc":
        assert z[f"{name}_full_kl"].shape == (4,) and 0 < float(z[f"{name}_full_spread"]) < 0.1
    X = z["e_X"]
    assert np.array_equal(X[7], X[3]) and np.array_equal(X[64], X[0]) and z["f_X"].dtype == np.float32


# ------------------------------------------------------------------------------------------------------ host rules
def test_random_init_is_sklearns_draw():
    seg = np.array([37, 130])
    rng = np.random.RandomState(3)
    want = np.concatenate([1e-4 * rng.standard_normal(size=(n, 2)).astype(np.float32) for n in seg])
    got = tsne.random_init(seg, 3)
    assert want.dtype == np.float32 and got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))


def test_pca_init_scaling():
    rng = np.random.RandomState(0)
    s = rng.standard_normal((50, 2)) * [3.0, 0.5]
    off = np.array([0, 20, 50])
    y = tsne.scale_pca_init(s, off)
    for a, b in ((0, 20), (20, 50)):
        assert abs(np.std(y[a:b, 0]) - 1e-4) < 1e-18
        assert np.allclose(y[a:b], s[a:b] / np.std(s[a:b, 0]) * 1e-4, rtol=1e-15)


def test_learning_rate_rule():
    seg = np.array([33, 2400, 9269])
    assert tsne.learning_rates("auto", seg, 12.0).tolist() == [50.0, 50.0, 9269 / 12.0 / 4.0]
    assert tsne.learning_rates(1000, seg, 12.0).tolist() == [1000.0] * 3
    for bad in ("fast", 0.0, -1.0):
        with pytest.raises(ValueError, match="learning_rate"):
            tsne.learning_rates(bad, seg, 12.0)
    assert tr.learning_rate(9269) == 9269 / 48.0 and tr.learning_rate(130) == 50.0


def test_schedule_is_sklearns_two_calls():
    seg = np.array([100, 200])
    sc = tsne.Schedule(seg, 1000, 12.0, np.array([50.0, 60.0]))
    assert sc.params().tolist() == [[12.0, 0.5, 50.0, 1.0, 0.0], [12.0, 0.5, 60.0, 1.0, 0.0]]
    assert [it for it in range(1000) if sc.wants_error(it)] == list(range(49, 1000, 50))
    assert tsne.Schedule(seg, 60, 12.0, np.ones(2)).wants_error(59)
    big = np.array([1.0, 1.0])
    assert not sc.begin(0) and not sc.check(49, np.array([5.0, 5.0]), big) and not sc.begin(249)
    assert sc.begin(250)                                    # both move on: plain P, momentum 0.8, update / gains reset
    assert sc.params().tolist() == [[1.0, 0.8, 50.0, 1.0, 1.0], [1.0, 0.8, 60.0, 1.0, 1.0]]
    assert sc.after_update() and not sc.after_update() and sc.params()[:, 4].tolist() == [0.0, 0.0]
    assert sc.best_iter.tolist() == [250, 250]              # the bookkeeping of the first phase is forgotten
    assert not sc.check(299, np.array([2.0, 2.0]), big)
    # segment 0 improves, segment 1 does not: stopped once more than 300 iterations passed since its best
    for it in range(349, 600, 50):
        assert not sc.check(it, np.array([2.0 - it * 1e-3, 3.0]), big)
    assert sc.check(649, np.array([1.0, 3.0]), big)         # 649 - 299 > 300
    assert sc.active.tolist() == [True, False] and sc.n_iter.tolist() == [1000, 650] and sc.kl.tolist() == [1.0, 3.0]
    assert sc.check(699, np.array([0.9, 7.0]), np.array([1e-15, 1.0]))     # gradient norm 1e-7.5 <= 1e-7
    assert not sc.active.any() and sc.n_iter.tolist() == [700, 650] and sc.kl.tolist() == [0.9, 3.0]
    # a stop in the first phase starts the second at the next iteration, as sklearn's it + 1
    sc = tsne.Schedule(seg, 1000, 12.0, np.ones(2))
    assert sc.check(99, np.array([1.0, 1.0]), np.array([1e-16, 1.0]))
    assert sc.phase.tolist() == [1, 0] and sc.active.all() and sc.best_iter.tolist() == [100, 99]
    assert sc.params()[:, [0, 1, 4]].tolist() == [[1.0, 0.8, 1.0], [12.0, 0.5, 0.0]]
    # the last iteration reports its error without testing convergence
    sc = tsne.Schedule(seg, 30, 12.0, np.ones(2))
    assert sc.wants_error(29) and not sc.check(29, np.array([4.0, 5.0]), np.array([0.0, 0.0]))
    assert sc.kl.tolist() == [4.0, 5.0] and sc.active.all() and sc.n_iter.tolist() == [30, 30]


def test_argument_errors():
    X = np.random.RandomState(0).rand(40, 6)
    with pytest.raises(ValueError, match="perplexity must be positive and less than the rows of every segment"):
        tsne.tsne(X, perplexity=40.0)
    with pytest.raises(ValueError, match="perplexity"):
        tsne.tsne(X, offsets=[0, 30, 40], perplexity=10.0)
    with pytest.raises(ValueError, match=r"init: expected a \(40, 2\) array"):
        tsne.tsne(X, perplexity=5.0, init=np.zeros((40, 3)))
    with pytest.raises(ValueError, match="init must be"):
        tsne.tsne(X, perplexity=5.0, init="spectral")
    with pytest.raises(ValueError, match="init='pca' needs D >= 3"):
        tsne.tsne(X[:, :2], perplexity=5.0)
    with pytest.raises(ValueError, match="x has 65 columns"):
        tsne.tsne(np.zeros((40, 65)), perplexity=5.0)
    with pytest.raises(ValueError, match="2-D"):
        tsne.tsne(np.zeros(40), perplexity=5.0)
    with pytest.raises(ValueError, match=r"2 \.\. 16384 rows"):
        tsne.tsne(np.zeros((16385, 3), dtype=np.float32), perplexity=5.0)
    with pytest.raises(ValueError, match="at most 2\\^31"):
        tsne.validate_offsets(np.arange(0, 16384 * 9 + 1, 16384), 16384 * 9)
    with pytest.raises(ValueError, match="offsets must run from 0"):
        tsne.tsne(X, offsets=[0, 20, 39], perplexity=5.0)
    with pytest.raises(ValueError, match="n_iter"):
        tsne.tsne(X, perplexity=5.0, n_iter=0)
    with pytest.raises(ValueError, match="early_exaggeration"):
        tsne.tsne(X, perplexity=5.0, early_exaggeration=0.5)
    with pytest.raises(ValueError, match="learning_rate"):
        tsne.tsne(X, perplexity=5.0, learning_rate="scanpy")
    with pytest.raises(ValueError, match="P holds 9 entries"):
        tsne.gradient(np.zeros((3, 3)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="perplexity"):
        tsne.joint_probabilities(X, None, 40.0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised without a GPU")
def test_no_gpu_error_names_the_module():
    X = np.random.RandomState(0).rand(40, 6)
    for call in (lambda: tsne.tsne(X, perplexity=5.0), lambda: tsne.tsne(X, perplexity=5.0, init="random"),
                 lambda: tsne.joint_probabilities(X, None, 5.0), lambda: tsne.gradient(np.zeros((40, 40)), np.zeros((40, 2))),
                 lambda: tsne.embed_slides([X, X], n_pcs=3, perplexity=5.0)):
        with pytest.raises(RuntimeError, match=r"mclstexp_amd\.(tsne|cluster): no GPU available"):
            call()


def test_cli_parsing():
    a = tsne.parse_args(["--pred", "1.npy", "2.npy", "--labels", "a.npy", "b.npy", "--perplexity", "20", "--out_dir", "o"])
    assert a.pred == ["1.npy", "2.npy"] and a.labels == ["a.npy", "b.npy"] and a.perplexity == 20.0 and a.n_pcs == 9
    assert a.learning_rate == "auto" and a.n_iter == 1000 and a.init == "pca" and a.out_dir == "o"
    assert tsne.parse_args(["--pred", "1.npy", "--learning_rate", "1000"]).learning_rate == 1000.0
    assert tsne.parse_args(["--pred", "1.npy"]).labels is None
    with pytest.raises(SystemExit):
        tsne.parse_args(["--pred", "1.npy", "2.npy", "--labels", "a.npy"])
    with pytest.raises(SystemExit):
        tsne.parse_args(["--pred", "1.npy", "--learning_rate", "quick"])
    from mclstexp_amd import cluster
    c = cluster.parse_args(["--pred", "1.npy", "--labels", "a.npy", "--tsne", "emb.npz"])
    assert c.tsne == "emb.npz" and cluster.parse_args(["--pred", "1.npy", "--labels", "a.npy"]).tsne is None


def test_cli_refuses_mismatched_labels(tmp_path):
    p, lab = str(tmp_path / "p.npy"), str(tmp_path / "l.npy")
    np.save(p, np.zeros((12, 5)))
    np.save(lab, np.array(["a"] * 11))
    with pytest.raises(ValueError, match="slide 0: prediction .12, 5. and 11 labels"):
        tsne.main(["--pred", p, "--labels", lab, "--out_dir", str(tmp_path / "o")])


def test_capi_symbols_and_argument_errors_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_abi_version() == 13 == _lib.ABI_VERSION
    for s in ("mcl_tsne_workspace_doubles", "mcl_tsne_affinities", "mcl_tsne_gradient", "mcl_tsne_update"):
        assert s in _lib.PROTOTYPES and hasattr(lib, s)
    assert _lib._RESTYPES["mcl_tsne_workspace_doubles"] is _lib.C.c_int64
    assert lib.mcl_tsne_workspace_doubles(9269, 1) >= 7 * 9269 + 1 and lib.mcl_tsne_workspace_doubles(0, 1) == 0
    assert lib.mcl_tsne_affinities(None, 9, 1, 9, None, None, 1, 40, 40, 40, 1600, 5.0, 0, None, None, None, None) == -1
    assert lib.mcl_tsne_gradient(None, None, None, None, 1, 40, 40, 40, 1600, None, 1, None, None, None, None) == -1
    assert lib.mcl_tsne_update(None, None, 1, 40, 40, 40, None, None, None, None, None, None) == -1
    # inconsistent sizes and limits are refused before any launch, whatever the pointers
    one = _lib.C.c_void_p(8)
    assert lib.mcl_tsne_gradient(one, one, one, one, 1, 40, 41, 40, 1600, one, 0, one, one, None, None) == -1
    assert lib.mcl_tsne_gradient(one, one, one, one, 1, 16385, 16385, 16385, 16385 ** 2, one, 0, one, one, None, None) == -2
    assert lib.mcl_tsne_gradient(one, one, one, one, 9, 9 * 16384, 16384, 16384, 9 * 16384 ** 2, one, 0, one, one, None,
                                 None) == -2
    assert lib.mcl_tsne_affinities(one, 65, 1, 65, one, one, 1, 40, 40, 40, 1600, 5.0, 0, one, one, one, None) == -2
    assert lib.mcl_tsne_affinities(one, 9, 1, 9, one, one, 1, 40, 40, 40, 1600, 40.0, 0, one, one, one, None) == -1
