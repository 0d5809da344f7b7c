"""CPU: the host side of mclstexp_amd.harmony (argument rules, permutations, block split, label encoding, CLI) and the
numpy restatement against tests/golden/harmony.npz.  Fails where mclstexp_amd.harmony does not exist."""
import numpy as np
import pytest
import torch

import harmony_reference as hr
from mclstexp_amd import harmony


@pytest.fixture(scope="module")
def z():
    return np.load(hr.GOLDEN)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_restatement_reproduces_the_fixture(z, name):
    """1e-12 relative, not bit equality: BLAS thread counts differ between machines."""
    r = hr.run_case(name, z)
    assert r["kmeans_rounds"].tolist() == z[f"{name}_kmeans_rounds"].tolist()
    assert r["converged"] == bool(z[f"{name}_converged"]) and r["orders_used"] == int(z[f"{name}_orders_used"])
    assert _rel(r["objective_kmeans"], z[f"{name}_objective_kmeans"]) <= 1e-12
    assert _rel(r["objective_harmony"], z[f"{name}_objective_harmony"]) <= 1e-12
    stride = {"c": 16, "e": 2}.get(name, 1)
    assert _rel(r["Z_corr"][::stride], z[f"{name}_Z_corr"]) <= 1e-12


def test_restatement_steps_of_case_a(z):
    r = hr.run_case("a", z, trace=True)
    assert _rel(np.stack([s["terms"] for s in r["steps"]]), z["a_terms"]) <= 1e-12
    assert _rel(np.stack([s["E"] for s in r["steps"]]), z["a_E"]) <= 1e-12
    assert _rel(np.stack([s["O"] for s in r["steps"]]), z["a_O"]) <= 1e-12


@pytest.mark.parametrize("name", "abc")
def test_restatement_intermediates(z, name):
    """Y, D, S, R after the blocks 0, 1, 2 and the last, E, O, the terms, M, W and Z_corr of the first and last k-means
    iteration and correction: the state the GPU tests hand the kernels is the stored one (W on the scale of Z_corr)."""
    got = hr.stored_slices(name, hr.run_case(name, z, trace=True))
    assert len(got) == 26 and any(k.endswith("R_block19") for k in got)
    for k, v in got.items():
        if k.endswith("_W"):
            scale = np.max(np.abs(z[k.replace("_W", "_Z_corr")]))
            assert np.max(np.abs(v - z[k])) / scale <= 1e-12, k
        else:
            assert v.shape == z[k].shape and _rel(v, z[k]) <= 1e-12, k


def test_one_batch_leaves_the_matrix_alone(z):
    r = hr.run_case("d", z)
    Z = hr.make_case("d")[0]
    assert np.max(np.abs(r["Z_corr"] - Z)) / np.max(np.abs(Z)) <= 4 * float(z["err_d_Z_corr"])


def test_fixture_holds_the_guards(z):
    for name in hr.CASES:
        for q in hr.QUANTITIES:
            assert 0 < float(z[f"err_{name}_{q}"]) < 1e-11, (name, q)
    for name in "abc":                                     # an early k-means stop and an early harmony stop
        assert bool(z[f"{name}_converged"]) and (z[f"{name}_kmeans_rounds"] < 19).any()
    assert not bool(z["e_converged"]) and z["e_kmeans_rounds"].tolist() == [4, 4]


def test_permutations_and_block_split_are_numpys():
    N = 611
    np.random.seed(0)
    want = []
    for _ in range(3):
        o = np.arange(N)
        np.random.shuffle(o)
        want.append(o)
    rng = np.random.RandomState(0)
    for w in want:
        got = harmony.draw_order(rng, N)
        assert got.dtype == np.int32 and np.array_equal(got, w)
    for n, bs in ((611, 0.05), (203, 0.05), (3000, 0.05), (40, 0.3), (7, 1.0)):
        nb = harmony.n_blocks(bs)
        parts = np.array_split(np.arange(n), nb)
        assert harmony.block_bounds(n, nb).tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    assert harmony.n_blocks(0.05) == 20 and harmony.n_blocks(0.3) == 4


def test_default_nclust():
    assert [harmony.default_nclust(n) for n in (15, 45, 75, 2985, 3015, 9269)] == [0, 2, 2, 100, 100, 100]
    assert [harmony.default_nclust(n) for n in (611, 2955, 2985)] == [20, 98, 100]


def test_label_encoding_order():
    codes, levels = harmony.encode_batch(["2.0", "0.0", "1.0", "0.0", "10.0"])
    assert levels.tolist() == ["0.0", "1.0", "10.0", "2.0"] and codes.tolist() == [3, 0, 1, 0, 2]   # get_dummies' order
    codes, levels = harmony.encode_batch(np.array([5, 3, 5, 9]))
    assert levels.tolist() == [3, 5, 9] and codes.tolist() == [1, 0, 1, 2] and codes.dtype == np.int32


def test_transposition_rule():
    a = np.zeros((7, 3))
    assert harmony.orient(a, 7) is a
    assert harmony.orient(a.T, 7).shape == (7, 3)
    sq = np.zeros((5, 5))
    assert harmony.orient(sq, 5) is sq                      # both fit: taken as cells x features
    with pytest.raises(ValueError, match="no axis of 4 cells"):
        harmony.orient(a, 4)


def test_convergence_tests():
    assert harmony.converged_kmeans([10.0, 9.0, 8.99999, 8.99998, 8.99997], 1e-5)
    assert not harmony.converged_kmeans([10.0, 9.0, 8.0, 7.0, 6.0], 1e-5)
    assert harmony.converged_harmony([5.0, 6.0], 1e-4)      # an increase stops the run: no absolute value
    assert not harmony.converged_harmony([6.0, 5.0], 1e-4)


def test_argument_errors():
    Z = np.random.RandomState(0).rand(40, 6)
    b = np.arange(40) % 2
    with pytest.raises(ValueError, match="exceeds the number of cells"):
        harmony.run_harmony(Z, b, nclust=41)
    with pytest.raises(ValueError, match="nclust must be >= 1"):
        harmony.run_harmony(Z[:14], b[:14])                 # round(14 / 30) = 0
    with pytest.raises(ValueError, match=r"update_orders\[0\]: expected 40 integers"):
        harmony.run_harmony(Z, b, nclust=3, update_orders=[np.arange(39)])
    with pytest.raises(ValueError, match="not a permutation"):
        harmony.run_harmony(Z, b, nclust=3, update_orders=[np.zeros(40, dtype=np.int64)])
    with pytest.raises(ValueError, match="init_centroids"):
        harmony.run_harmony(Z, b, nclust=3, init_centroids=np.zeros((4, 6)))
    with pytest.raises(ValueError, match="seed_rows"):
        harmony.run_harmony(Z, b, nclust=3, seed_rows=[0, 0, 1])
    with pytest.raises(ValueError, match="theta"):
        harmony.run_harmony(Z, b, nclust=3, theta=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="no axis of 40 cells"):
        harmony.run_harmony(Z[:30], b, nclust=3)
    with pytest.raises(ValueError, match="batch 1 has 0 cells"):
        harmony.correct_slides([np.zeros((6, 20)), np.zeros((6, 0))])
    with pytest.raises(ValueError, match="slide 1 has 5 genes"):
        harmony.correct_slides([np.zeros((6, 20)), np.zeros((5, 20))])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised without a GPU")
def test_no_gpu_error_names_the_module():
    Z = np.random.RandomState(0).rand(40, 6)
    with pytest.raises(RuntimeError, match=r"mclstexp_amd\.harmony: no GPU available"):
        harmony.run_harmony(Z, np.arange(40) % 2, nclust=3)


def test_cli_parses_and_refuses_mismatched_gene_counts(tmp_path):
    a = harmony.parse_args(["--matrices", "1.npy", "2.npy", "--out_dir", "o", "--theta", "1"])
    assert a.matrices == ["1.npy", "2.npy"] and a.theta == 1.0 and a.max_iter_harmony == 10 and a.nclust is None
    p1, p2 = str(tmp_path / "1.npy"), str(tmp_path / "2.npy")
    np.save(p1, np.zeros((6, 20)))
    np.save(p2, np.zeros((5, 20)))
    with pytest.raises(ValueError, match="expected .G, N. with G = 6"):
        harmony.main(["--matrices", p1, p2, "--out_dir", str(tmp_path / "o")])


def test_capi_argument_errors_without_gpu():
    from mclstexp_amd import _lib
    lib = _lib.load()
    assert lib.mcl_harmony_normalize(None, 0, 1, 4, 4, 1, None, None, None) == -1
    assert lib.mcl_harmony_centroids(None, None, None, 4, 4, 4, 0, 1, None, None, None) == -1
    assert lib.mcl_harmony_dist(None, None, 4, 4, 4, 0, None, None) == -1
    assert lib.mcl_harmony_softmax(None, 4, 4, 0.1, 1, None, None) == -1
    assert lib.mcl_harmony_moments(None, None, 4, 4, 2, None, None, None, None) == -1
    assert lib.mcl_harmony_update_block(None, None, None, None, 4, 4, 2, 2, 0, 2, None, None, None, None, None) == -1
    assert lib.mcl_harmony_objective(None, None, None, None, None, None, 4, 4, 2, 0.1, None, None, None) == -1
    assert lib.mcl_harmony_ridge(None, None, None, 4, 2, 4, None, None) == -1
    assert lib.mcl_harmony_apply(None, None, None, None, 4, 4, 2, 4, None, None) == -1
    assert lib.mcl_harmony_lloyd(None, 4, 4, 4, None, 25, None, None, None, None, None, None) == -1
    assert lib.mcl_harmony_workspace_doubles(9269, 100, 3467, 4) > 0
