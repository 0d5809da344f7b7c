"""The float64 Adam restatement the GPU tests use (tests/adam_reference.py), checked on the CPU: against torch.optim.Adam in
float64, and -- with a plain unfused fp32 evaluation standing in for a correct kernel -- that the per-element bounds leave room."""
import numpy as np
import pytest
import torch

import adam_reference as ar

B1, B2, EPS = 0.9, 0.999, 1e-8


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_step64_is_torch_adam(wd):
    """Six steps of torch.optim.Adam (L2-coupled decay, single tensor) on float64 tensors, the learning rate changed after
    step 3, compared with step64 in two ways, both to 1e-14.

    Free-running (step64 fed its own trajectory): parameters and both moments agree normwise, max |difference| / max |value|.
    Step by step (step64 fed torch's state before the step, so nothing accumulates): every ELEMENT agrees relative to the size
    of the terms it is summed from -- a = |g| + wd |p|; |m_old| + a for exp_avg; b2 v_old + (1 - b2) a^2 for exp_avg_sq;
    |p_old| + (lr / bc1) (|m_old| + a) / (sqrt(V) / sqrt(bc2) + eps) for p -- so an element near zero is held to the rounding
    of its terms and is not excused by a large neighbour, while a cancellation in g + wd p or in the moment is not held
    against either side."""
    rng = np.random.default_rng(5)
    n = 4099
    p0 = rng.standard_normal(n)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    tp, tm, tv = p0.copy(), np.zeros(n), np.zeros(n)            # torch's state before the step
    lr = 1e-3
    for t in range(1, 7):
        if t == 4:
            lr = 3e-4
            opt.param_groups[0]["lr"] = lr
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[param]
        got = (param.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
        p, m, v = ar.step64(p, g, m, v, lr, B1, B2, EPS, wd, t)
        for name, x, want in zip(("p", "exp_avg", "exp_avg_sq"), got, (p, m, v)):
            rel = np.abs(x - want).max() / np.abs(want).max()
            assert rel <= 1e-14, f"step {t} wd {wd}: {name} differs from torch.optim.Adam by {rel:.3e} normwise"
        P, M, V = ar.step64(tp, g, tm, tv, lr, B1, B2, EPS, wd, t)
        a = np.abs(g) + wd * np.abs(tp)
        sm = np.abs(tm) + a
        sv = B2 * tv + (1 - B2) * a * a
        sp = np.abs(tp) + lr / (1 - B1 ** t) * sm / (np.sqrt(V) / np.sqrt(1 - B2 ** t) + EPS)
        for name, x, want, scale in zip(("p", "exp_avg", "exp_avg_sq"), got, (P, M, V), (sp, sm, sv)):
            assert np.all(scale > 0)
            rel = (np.abs(x - want) / scale).max()
            assert rel <= 1e-14, f"step {t} wd {wd}: an element of {name} differs from torch.optim.Adam by {rel:.3e} of its scale"
        tp, tm, tv = got


@pytest.mark.parametrize("lr,wd", [(1e-4, 1e-3), (1e-2, 0.0)])
@pytest.mark.parametrize("t", [1, 7, 1000, 8191, 100000])
def test_unfused_fp32_uses_at_most_half_of_each_bound(t, lr, wd):
    """step32 (one rounding per operation, no fused multiply-add) on the planted-cancellation inputs stays within half of
    the m and the v bound: they leave 2x room over a correct unfused fp32 implementation, whatever a GPU does.

    For p "half of the bound" cannot be asked of any fp32 implementation: the last operation, p - d, is rounded to fp32, and a
    correctly rounded result is off by up to half an ulp of P, which reaches u/2 |P| just above a power of two.  That alone is
    half of the bound's first term u |P'|, so with any error at all in d the ratio to the whole bound passes 0.5 (measured
    here: 0.50 to 0.54).  What a correct unfused implementation can reach follows from counting roundings of u/2 each: one
    for p - d, and seven in d = lr_bc1 (m / (sqrt(v) rs2 + eps)) -- the rounded constants rs2 and eps (they act on the two
    terms of the denominator, whose weights sum to one: one rounding), lr_bc1, sqrt, multiply, add, divide, multiply -- so
    |error| <= u/2 |P'| + 3.5 u |d'| to first order, which is at most max(1/2, 3.5/4) = 0.875 of
    u |P'| + 4 u |d'|.  That derived figure is asserted; the kernel fuses three of these operations and rounds less."""
    p, g, m, v = ar.planted_inputs(1 << 19, wd, seed=t)
    P, M, V = ar.step32(p, g, m, v, lr, B1, B2, EPS, wd, t)
    rp, rm, rv = ar.ratios(p, g, m, v, P, M, V, lr, B1, B2, EPS, wd, t)
    print(f"step32 t={t} lr={lr} wd={wd}: worst ratio p {rp:.3f} m {rm:.3f} v {rv:.3f}")
    assert ar.within((rm, rv), 0.5)
    assert ar.within((rp,), 0.875)


def test_zero_scale_elements_exist_and_are_exact():
    """With wd = 0 the planted inputs hold elements whose m and v scales are exactly 0 (g = 0, m = 0; v = 0): the bounds are 0
    there, so the comparison is an equality -- and a perturbed result is reported as an infinite ratio."""
    p, g, m, v = ar.planted_inputs(1000, 0.0, seed=1)
    (M, V, _, _), (bm, bv, _) = ar.bounds(p, g, m, v, m, v, 1e-2, B1, B2, EPS, 0.0, 2)
    assert (bm == 0).sum() > 0 and (bv == 0).sum() > 0
    assert np.all(M[bm == 0] == 0) and np.all(V[bv == 0] == 0)
    P, M32, V32 = ar.step32(p, g, m, v, 1e-2, B1, B2, EPS, 0.0, 2)
    assert ar.within(ar.ratios(p, g, m, v, P, M32, V32, 1e-2, B1, B2, EPS, 0.0, 2))
    M32 = M32.copy()
    M32[np.flatnonzero(bm == 0)[0]] = 1e-30
    assert ar.ratios(p, g, m, v, P, M32, V32, 1e-2, B1, B2, EPS, 0.0, 2)[1] == np.inf


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_results_are_outside_every_bound(bad):
    """One NaN or infinity in p, m or v -- alone, or in all three at once -- gives an infinite ratio for that quantity, and
    `within` refuses it: a NaN bound (p is judged against the implementation's own moments) hides nothing."""
    lr, wd, t = 1e-4, 1e-3, 2
    p, g, m, v = ar.planted_inputs(1000, wd, seed=2)
    good = ar.step32(p, g, m, v, lr, B1, B2, EPS, wd, t)
    assert ar.within(ar.ratios(p, g, m, v, *good, lr, B1, B2, EPS, wd, t))
    for which in ((0,), (1,), (2,), (0, 1, 2)):
        for whole in (False, True):
            got = [x.copy() for x in good]
            for k in which:
                if whole:
                    got[k][:] = bad
                else:
                    got[k][5] = bad
            r = ar.ratios(p, g, m, v, *got, lr, B1, B2, EPS, wd, t)
            assert all(r[k] == np.inf for k in which), f"{bad} in {which} (whole array: {whole}) gives ratios {r}"
            assert not ar.within(r)
    assert not ar.within((0.1, float("nan"), 0.1)) and not ar.within((float("nan"),))


def test_bounds_see_a_wrong_update():
    """The errors the loose trajectory checks let through are far outside the bounds: eps scaled by 1/sqrt(bc2), bc2 taken
    from t - 1, and a dropped weight-decay term."""
    lr, wd, t = 1e-4, 1e-3, 2
    p, g, m, v = ar.planted_inputs(100003, wd, seed=3)
    f = np.float32
    c = [f(x) for x in ar.consts64(lr, B1, B2, EPS, wd, t)]
    P, M, V = ar.step32(p, g, m, v, lr, B1, B2, EPS, wd, t)
    bad_eps = p - c[0] * (M / (np.sqrt(V) * c[7] + c[5] * c[7]))
    assert ar.ratios(p, g, m, v, bad_eps, M, V, lr, B1, B2, EPS, wd, t)[0] > 1
    rs_prev = f(ar.consts64(lr, B1, B2, EPS, wd, t - 1)[7])
    bad_bc2 = p - c[0] * (M / (np.sqrt(V) * rs_prev + c[5]))
    assert ar.ratios(p, g, m, v, bad_bc2, M, V, lr, B1, B2, EPS, wd, t)[0] > 1
    P0, M0, V0 = ar.step32(p, g, m, v, lr, B1, B2, EPS, 0.0, t)
    _, rm, rv = ar.ratios(p, g, m, v, P0, M0, V0, lr, B1, B2, EPS, wd, t)
    assert rm > 1 and rv > 1


def test_consts64_closed_forms_at_step_one():
    lr, wd = 3e-4, 1e-3
    c = ar.consts64(lr, B1, B2, EPS, wd, 1)
    want = [lr / (1 - B1), B1, B2, 1 - B1, 1 - B2, EPS, wd, 1 / np.sqrt(1 - B2)]
    assert c.dtype == np.float64 and c.shape == (8,)
    np.testing.assert_allclose(c, want, rtol=4e-16, atol=0)
    assert c[1] == B1 and c[2] == B2 and c[3] == 1 - B1 and c[4] == 1 - B2 and c[5] == EPS and c[6] == wd
