"""Writes tests/golden/tsne.npz: sklearn's own exact-path functions (sklearn 1.7.2: _binary_search_perplexity,
_joint_probabilities, _kl_divergence, _gradient_descent driven with float64 parameters) on the cases of
tests/tsne_reference.py, and the restatement's own uncertainty per compared quantity.

    python tests/golden/gen_tsne_goldens.py

err_<case>_<quantity>: the larger of the restatement's deviation from an np.longdouble run and from a run on inputs
perturbed by 1e-15 relative, both relative to max |value| and floored at 2^-53 (the format's own rounding).  Full P is
stored for the two smallest cases only; the others keep row sums and a fixed sample of entries."""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import _utils
from sklearn.manifold._t_sne import _gradient_descent, _joint_probabilities, _kl_divergence

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsne_reference as tr  # noqa: E402

LD = np.longdouble
FLOOR = 2.0 ** -53
FULL_P = ("a", "d")
E = 12.0
clamp_engaged = []


def perturb(a, seed):
    rng = np.random.RandomState(seed)
    return np.asarray(a, dtype=np.float64) * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=np.shape(a)))


def err(base, *others):
    scale = np.max(np.abs(base))
    return max(FLOOR, *(float(np.max(np.abs(np.asarray(o, dtype=LD) - base)) / scale) for o in others))


def objective(n):
    """sklearn's _kl_divergence, noting whether its clamp Q = max(q, eps) would engage."""
    def f(params, P, dof, n_samples, n_components, **kw):
        Y = params.reshape(n, 2)
        d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
        w = 1.0 / (1.0 + d)
        np.fill_diagonal(w, 0.0)
        q = w / w.sum()
        clamp_engaged.append(bool((q[~np.eye(n, dtype=bool)] < tr.EPS).any()))
        return _kl_divergence(params, P, dof, n_samples, n_components, **kw)
    return f


def sk_descent(P, Y0, n_iter, lr):
    """sklearn's all-float64 trajectory under the exaggerated phase's settings, to iteration n_iter."""
    n = Y0.shape[0]
    p, kl, it = _gradient_descent(objective(n), Y0.astype(np.float64).ravel().copy(), it=0, max_iter=n_iter,
                                  n_iter_check=tr.CHECK_EVERY, n_iter_without_progress=250, momentum=0.5, learning_rate=lr,
                                  min_gain=0.01, min_grad_norm=1e-7, verbose=0,
                                  args=[squareform(P * E, checks=False), 1.0, n, 2], kwargs={})
    assert it == n_iter - 1
    return p.reshape(n, 2), kl


def sk_full(P, Y0, lr, n_iter=1000):
    """TSNE._tsne's two calls with float64 parameters."""
    n = Y0.shape[0]
    obj = objective(n)
    common = dict(n_iter_check=tr.CHECK_EVERY, learning_rate=lr, min_gain=0.01, min_grad_norm=1e-7, verbose=0, kwargs={})
    p, kl, it = _gradient_descent(obj, Y0.astype(np.float64).ravel().copy(), it=0, max_iter=tr.EXPLORATION_ITERS,
                                  n_iter_without_progress=250, momentum=0.5,
                                  args=[squareform(P * E, checks=False), 1.0, n, 2], **common)
    p, kl, it = _gradient_descent(obj, p, it=it + 1, max_iter=n_iter, n_iter_without_progress=300, momentum=0.8,
                                  args=[squareform(P, checks=False), 1.0, n, 2], **common)
    return p.reshape(n, 2), kl, it


def main():
    out = {}
    for name, (sizes, D, perplexity) in tr.CASES.items():
        X, lab = tr.make_case(name)
        off = tr.offsets_of(name)
        out[f"{name}_X"], out[f"{name}_labels"] = X, lab.astype(np.int8)
        rng = np.random.RandomState(7 + ord(name))
        Y0 = (1e-4 * rng.standard_normal((X.shape[0], 2)).astype(np.float32)).astype(np.float64)
        out[f"{name}_Y0"] = Y0
        e_P, e_beta = {False: FLOOR, True: FLOOR}, {False: FLOOR, True: FLOOR}
        for s in range(len(sizes)):
            Xs = np.asarray(X[off[s]:off[s + 1]], dtype=np.float64)
            for f32 in (False, True):
                P, beta = tr.joint_probabilities(Xs, perplexity, f32)
                P_ld, beta_ld = tr.joint_probabilities(Xs.astype(LD), perplexity, f32, LD)
                P_pt, beta_pt = tr.joint_probabilities(perturb(Xs, 11), perplexity, f32)
                e_P[f32] = max(e_P[f32], err(P, P_ld, P_pt))
                e_beta[f32] = max(e_beta[f32], err(beta, beta_ld, beta_pt))
        for f32, tag in ((False, "f64"), (True, "f32")):
            out[f"err_{name}_P_{tag}"], out[f"err_{name}_beta_{tag}"] = e_P[f32], e_beta[f32]
        if name not in tr.SINGLE:
            continue
        n = sizes[0]
        lr = tr.learning_rate(n, E)

        # ---- sklearn's affinities on the float32-rounded distances (its own arithmetic)
        d32 = tr.sq_distances(X, True).astype(np.float32)
        sk_C = np.asarray(_utils._binary_search_perplexity(d32, perplexity, 0))
        sk_P = squareform(_joint_probabilities(d32, perplexity, 0))
        ii, jj = tr.sample_index(n)
        out[f"{name}_sk_P"] = sk_P if name in FULL_P else sk_P[ii, jj]
        out[f"{name}_sk_C"] = sk_C if name in FULL_P else sk_C[ii, jj]
        out[f"{name}_sk_P_rowsum"], out[f"{name}_sk_P_max"] = sk_P.sum(axis=1), sk_P.max()

        # ---- gradients and KL at Y0 and at a mid-run Y, plain and exaggerated, on sklearn's P
        P32, _ = tr.joint_probabilities(X, perplexity, True)
        P64, _ = tr.joint_probabilities(X, perplexity, False)
        Ymid, _ = sk_descent(P64, Y0, 30, lr)
        out[f"{name}_Ymid"] = Ymid
        for where, Y in (("Y0", Y0), ("Ymid", Ymid)):
            for ex, tag in ((1.0, "plain"), (E, "exag")):
                kl, g = _kl_divergence(Y.ravel().copy(), squareform(sk_P * ex, checks=False), 1.0, n, 2)
                out[f"{name}_sk_grad_{where}_{tag}"], out[f"{name}_sk_kl_{where}_{tag}"] = g.reshape(n, 2), kl
                g0, k0, _ = tr.gradient(P32, Y, ex)
                g1, k1, _ = tr.gradient(P32.astype(LD), Y.astype(LD), ex, LD)
                g2, k2, _ = tr.gradient(joint_sym(perturb(P32, 12)), perturb(Y, 13), ex)
                out[f"err_{name}_grad_{where}_{tag}"] = err(g0, g1, g2)
                out[f"err_{name}_kl_{where}_{tag}"] = err(np.array([k0]), np.array([k1]), np.array([k2]))

        # ---- one update step from a mid-run state
        st = np.random.RandomState(5)
        g_mid = tr.gradient(P64, Ymid, E)[0]
        upd, gains = 1e-3 * st.standard_normal((n, 2)), st.choice([0.01, 0.8, 1.0, 1.2, 2.4], size=(n, 2))
        out[f"{name}_step_grad"], out[f"{name}_step_update"], out[f"{name}_step_gains"] = g_mid, upd, gains

        # ---- sklearn's float64 trajectory for the first 60 iterations, and how far the restatement can be trusted
        marks = tuple(range(10, tr.TRAJECTORY + 1, 10))
        keep = (1,) + marks
        base = tr.run(P64, Y0, tr.TRAJECTORY, E, keep=keep)
        P_ld, _ = tr.joint_probabilities(X.astype(LD), perplexity, False, LD)
        ld = tr.run(P_ld, Y0.astype(LD), tr.TRAJECTORY, E, keep=keep, dtype=LD)
        pt = tr.run(tr.joint_probabilities(perturb(X, 11), perplexity)[0], perturb(Y0, 14), tr.TRAJECTORY, E, keep=keep)
        dev = {k: err(base["trace"][k], ld["trace"][k], pt["trace"][k]) for k in keep}
        length = tr.TRAJECTORY
        while length > 10 and dev[length] > 1e-6:
            length -= 10
        assert dev[length] <= 1e-6, (name, dev)
        out[f"{name}_trajectory_len"] = length
        for k in (1, 10, length):
            out[f"{name}_sk_Y{k}"] = sk_descent(P64, Y0, k, lr)[0]
            out[f"err_{name}_Y{k}"] = dev[k]
        print(name, "trajectory length", length, {k: f"{v:.2e}" for k, v in dev.items()})

        # ---- full runs: cases b and c, four starts 1e-6 apart
        if name in "bc":
            kls = []
            for t in range(4):
                Yt = Y0 * (1.0 + 1e-6 * np.random.RandomState(100 + t).standard_normal(Y0.shape))
                Yf, kl, it = sk_full(P64, Yt, lr)
                assert tr.nn_purity(Yf, lab) == 1.0, (name, t)
                kls.append(kl)
            kls = np.array(kls)
            out[f"{name}_full_kl"], out[f"{name}_full_spread"] = kls, (kls.max() - kls.min()) / kls.mean()
            print(name, "final KL", kls, "spread", out[f"{name}_full_spread"])
    assert clamp_engaged and not any(clamp_engaged), "sklearn's clamp on Q engaged on a recorded trajectory"
    out["clamp_checks"] = len(clamp_engaged)
    np.savez_compressed(tr.GOLDEN, **out)
    print("wrote", tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes")
    for k in sorted(out):
        if k.startswith("err_"):
            print(f"  {k} = {float(out[k]):.3e}")


def joint_sym(P):
    """A perturbed P made symmetric again (the kernels and sklearn both read a symmetric P)."""
    return (P + P.T) / 2


if __name__ == "__main__":
    main()
