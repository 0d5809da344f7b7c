"""tests/stem_reference.py checked on the CPU, in the three parts of tests/test_dense_reference_host.py: with every rounding
point switched off it is fp64 autograd of the torchvision formulas (norm -> relu -> maxpool; norm -> relu -> conv -> avgpool with
the pool and the convolution commuted; conv0; norm5 + global pool; odd maps with floor pooling); a float32 emulation of each
kernel in a DIFFERENT legal accumulation order stays inside every bound and reproduces every exact output bit for bit; and every
mutant of the emulation exceeds a bound or breaks bit equality."""
import numpy as np
import pytest
import torch

import dense_reference as dr
import stem_reference as sr

EPS = 1e-5
F = np.float32


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)
    assert err <= 1e-12, f"{what}: {err:.3e} of max"


def _tt(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)


def _nchw(a):
    return a.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _live(prm, rng):
    """No dead channel: keep every gradient alive."""
    prm["beta"] = rng.normal(0, 0.3, prm["beta"].shape)
    prm["gamma"][2] = 0.9
    return prm


def _batch_stats(prm, x2d):
    (m, v, r), _ = sr.bn_stats(x2d, EPS, 1)
    prm["mean"], prm["rstd"] = m, r
    return prm


# ------------------------------------------------------------------------------------------------------------ 1. autograd
def test_fma32v_is_fma32():
    rng = np.random.default_rng(0)
    n = 4000
    a = dr.f32(rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n))
    b = dr.f32(rng.normal(size=n))
    c = dr.f32(rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n))
    # exact ties of the fp32 result, off by one float64 rounding: c = the midpoint minus a*b plus a sliver
    a[:50], b[:50] = 1.0, 1.0 + 2.0 ** -23
    c[:50] = dr.f32(2.0 ** -24 * (1 + 2.0 ** -20) * rng.choice([-1.0, 1.0], 50))
    assert np.array_equal(sr.fma32v(a, b, c), dr.fma32(a, b, c))
    assert np.array_equal(sr.add32(a, c), dr.fma32(a, 1.0, c))


@pytest.mark.parametrize("N,H,W,C", [(2, 7, 5, 8), (1, 6, 8, 16)])
def test_stem_tail_without_rounding_is_autograd(N, H, W, C):
    """norm0 -> relu0 -> pool0 and its backward (max-pool gather, then the BatchNorm backward) against fp64 autograd."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=(N, H, W, C))
    prm = _batch_stats(_live(sr.stem_params(C, 3), rng), x.reshape(-1, C))
    xt, gt, bt = _tt(x), _tt(prm["gamma"]), _tt(prm["beta"])
    a = torch.relu(torch.nn.functional.batch_norm(_nchw(xt), None, None, gt, bt, True, 0.0, EPS))
    y = torch.nn.functional.max_pool2d(a, 3, 2, 1)
    dy = rng.normal(size=_nhwc(y).shape)
    (y * _nchw(torch.tensor(dy))).sum().backward()
    ym, idx = sr.bn_act_maxpool_fwd(x, prm, rounding=False)
    _close(ym, _nhwc(y), "pooled")
    g = sr.maxpool_bwd(idx, dy, H, W, rounding=False)
    gi = np.where(sr.relu_mask(x, prm, rounding=False), g, 0.0).reshape(-1, C)
    s = sr.bn_bwd_sums(gi, x.reshape(-1, C), prm, 0.0)
    _close(s["dgamma"][0], gt.grad.numpy(), "dgamma")
    _close(s["dbeta"][0], bt.grad.numpy(), "dbeta")
    dx, _ = sr.bn_bwd_dx(gi, x.reshape(-1, C), prm, s["coef"][0], 1, rounding=False)
    _close(dx, xt.grad.numpy().reshape(-1, C), "dx")


@pytest.mark.parametrize("N,H,W,C,Co", [(2, 4, 6, 16, 8), (3, 5, 7, 16, 8)])
def test_transition_without_rounding_is_autograd(N, H, W, C, Co):
    """torchvision's norm -> relu -> conv -> AvgPool2d(2, 2) against the commuted norm -> relu -> pool -> conv, forward and
    backward; the odd map pools with floor."""
    rng = np.random.default_rng(2)
    x = rng.normal(size=(N, H, W, C))
    Wt = rng.normal(0, 0.3, (Co, C))
    prm = _batch_stats(_live(sr.stem_params(C, 4), rng), x.reshape(-1, C))
    xt, gt, bt, wt = _tt(x), _tt(prm["gamma"]), _tt(prm["beta"]), _tt(Wt)
    a = torch.relu(torch.nn.functional.batch_norm(_nchw(xt), None, None, gt, bt, True, 0.0, EPS))
    y = torch.nn.functional.avg_pool2d(torch.nn.functional.conv2d(a, wt[:, :, None, None]), 2, 2)
    dy = rng.normal(size=_nhwc(y).shape)
    (y * _nchw(torch.tensor(dy))).sum().backward()
    p = sr.bn_act_avgpool_fwd(x, prm, rounding=False)
    _close(p.reshape(-1, C) @ Wt.T, _nhwc(y).reshape(-1, Co), "y")
    _close(dr.conv1x1_wrw(dy.reshape(-1, Co), p.reshape(-1, C))[0] - 0.0, wt.grad.numpy(), "dW")
    dp = (dy.reshape(-1, Co) @ Wt).reshape(N, H // 2, W // 2, C)
    gi = sr.pool_gradient(dp, x, prm, H, W, rounding=False)
    s = sr.bn_bwd_sums(gi, x.reshape(-1, C), prm, 0.0)
    _close(s["dgamma"][0], gt.grad.numpy(), "dgamma")
    _close(s["dbeta"][0], bt.grad.numpy(), "dbeta")
    dx, _ = sr.bn_bwd_dx(gi, x.reshape(-1, C), prm, s["coef"][0], 1, rounding=False)
    _close(dx, xt.grad.numpy().reshape(-1, C), "dx")


def test_avgpool_without_rounding_is_autograd():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 4, 6, 8))
    xt = _tt(x)
    y = torch.nn.functional.avg_pool2d(_nchw(xt), 2, 2)
    dy = rng.normal(size=_nhwc(y).shape)
    (y * _nchw(torch.tensor(dy))).sum().backward()
    _close(sr.avgpool_fwd(x, rounding=False), _nhwc(y), "avgpool")
    _close(sr.avgpool_bwd(dy, 4, 6), xt.grad.numpy(), "avgpool backward")


def test_conv0_without_rounding_is_autograd():
    rng = np.random.default_rng(6)
    N, H, W = 2, 8, 16
    x, Wt = rng.normal(size=(N, H, W, 3)), rng.normal(0, 0.1, (64, 7, 7, 3))
    xt, wt = _tt(x), _tt(Wt)
    y = torch.nn.functional.conv2d(_nchw(xt), _nchw(wt), stride=2, padding=3)
    dy = rng.normal(size=_nhwc(y).shape)
    (y * _nchw(torch.tensor(dy))).sum().backward()
    _close(sr.conv0_fwd(x, Wt)[0], _nhwc(y).reshape(-1, 64), "conv0")
    _close(sr.conv0_wrw(x, dy.reshape(-1, 64), N, H, W)[0] - 0.0, wt.grad.numpy().reshape(64, 147), "conv0 dW")
    (m, v, r), _ = sr.stats_tiles_unshifted(_nhwc(y).reshape(-1, 64), EPS, W)
    _close(m, _nhwc(y).reshape(-1, 64).mean(0), "conv0 mean")
    _close(v, _nhwc(y).reshape(-1, 64).var(0), "conv0 var")


def test_norm5_pool_without_rounding_is_autograd():
    rng = np.random.default_rng(7)
    B, HW, C = 3, 9, 16
    x = rng.normal(size=(B, HW, C))
    prm = _batch_stats(_live(sr.stem_params(C, 8), rng), x.reshape(-1, C))
    xt, gt, bt = _tt(x), _tt(prm["gamma"]), _tt(prm["beta"])
    a = torch.nn.functional.batch_norm(xt.permute(0, 2, 1), None, None, gt, bt, True, 0.0, EPS)
    out = a.mean(2)
    g = rng.normal(size=(B, C))
    (out * torch.tensor(g)).sum().backward()
    f = sr.bn_gap_fwd(x, prm, rounding=False)
    _close(f["out"][0], out.detach().numpy(), "out")
    s = sr.bn_gap_bwd_sums(g, f["xmean"][0], prm, HW)
    _close(s["dgamma"][0], gt.grad.numpy(), "dgamma")
    _close(s["dbeta"][0], bt.grad.numpy(), "dbeta")
    _close(sr.bn_gap_bwd_dx(g, x, prm, s["coef"][0], rounding=False)[0], xt.grad.numpy(), "dx")


# ------------------------------------------------------------------------------------------------------------ 2. fp32 emulation
def _store(v, trunc=False):
    return dr.bf16_trunc_bits(v) if trunc else dr.bf16_bits(v)


def emu_prologue(prm):
    g, b, m, r = (np.asarray(prm[k], dtype=F) for k in ("gamma", "beta", "mean", "rstd"))
    sc = g * r
    return sc, dr.fma32(-m.astype(np.float64), sc.astype(np.float64), b.astype(np.float64)).astype(F)


def emu_t(x, prm):
    """fmaf(x, sc, sh) through dense_reference.fma32 (exact rational comparison), not through stem_reference.fma32v."""
    sc, sh = emu_prologue(prm)
    return dr.fma32(np.asarray(x, dtype=np.float64), sc.astype(np.float64), sh.astype(np.float64)).astype(F)


def emu_colsum(v, rpb, rpi):
    """Per-channel sum of v (S, C) fp32 in a legal order that is not the kernel's: inside a block of rpb rows a thread adds its
    rows (r % rpi equal) LAST row first, the rpi threads are merged LAST first, the blocks are added in double."""
    S, C = v.shape
    nb = -(-S // rpb)
    pad = np.zeros((nb * rpb, C), dtype=F)
    pad[:S] = v
    rt = rpb // rpi if rpb % rpi == 0 else -(-rpb // rpi)
    blk = np.zeros((nb, rt * rpi, C), dtype=F)
    blk[:, :rpb] = pad.reshape(nb, rpb, C)
    blk = blk.reshape(nb, rt, rpi, C)
    th = np.zeros((nb, rpi, C), dtype=F)
    for i in reversed(range(rt)):
        th = th + blk[:, i]
    tot = np.zeros((nb, C), dtype=F)
    for q in reversed(range(rpi)):
        tot = tot + th[:, q]
    return tot.astype(np.float64).sum(0)


def _rp(S, C, dtype):
    nb, rpb, tiles = sr.plan(S, C, dtype)
    assert tiles == 1
    return rpb, sr.NTH // (C // (8 if dtype == 1 else 4))


def emu_stats(x, dtype):
    x32 = np.asarray(x, dtype=F)
    S, C = x32.shape
    d = x32 - x32[0]
    rpb, rpi = _rp(S, C, dtype)
    a, b = emu_colsum(d, rpb, rpi), emu_colsum(d * d, rpb, rpi)
    m = a / S
    v = np.maximum(b / S - m * m, 0.0)
    return dr.f32(x32[0].astype(np.float64) + m), dr.f32(v), dr.f32(1.0 / np.sqrt(v + np.float64(F(EPS))))


def emu_bwd(g, x, prm, dtype, prior=None, le_zero=True, coef_div=None, contract=False, trunc=False, relu=1):
    """act_bwd_reduce / finalize / dx in fp32 from the unmasked gradient g (S, C): (dgamma, dbeta, coef, dx bits or values).
    le_zero False (mutant): the mask tests t < 0.  coef_div (mutant): what coef divides by.  contract: xhat*c2 fused into the
    subtraction (the other legal form)."""
    g32, x32 = np.asarray(g, dtype=F), np.asarray(x, dtype=F)
    S, C = x32.shape
    t = emu_t(x, prm)
    gi = np.where((t <= 0 if le_zero else t < 0) & bool(relu), F(0), g32)
    mu, rs = np.asarray(prm["mean"], dtype=F), np.asarray(prm["rstd"], dtype=F)
    sc, _ = emu_prologue(prm)
    xh = (x32 - mu) * rs
    rpb, rpi = _rp(S, C, dtype)
    a, b = emu_colsum(gi, rpb, rpi), emu_colsum(gi * xh, rpb, rpi)
    div = S if coef_div is None else coef_div
    coef = np.stack([a / div, b / div], 1).astype(F)
    c1, c2 = coef[:, 0], coef[:, 1]
    if contract:
        inner = sr.fma32v(-xh.astype(np.float64), c2.astype(np.float64), (gi - c1).astype(np.float64)).astype(F)
    else:
        inner = (gi - c1) - xh * c2
    d = sc * inner
    if prior is not None:
        d = np.asarray(prior, dtype=F) + d
    out = d.astype(np.float64)
    return b.astype(F).astype(np.float64), a.astype(F).astype(np.float64), coef.astype(np.float64), \
        (dr.bits_to_f64(_store(out, trunc)) if dtype == 1 else out)


_bn_case = sr.bn_case


HOST_BN = [(1, 1, 8), (1, 777, 40), (0, 333, 64), (1, 50, 2048)]


@pytest.mark.parametrize("dtype,S,C", HOST_BN)
def test_emulated_bn_kernels(dtype, S, C):
    prm, x, dy = _bn_case(dtype, S, C)
    # exact: forward, both relu settings, through an independent fmaf
    for relu in (0, 1):
        t = emu_t(x, prm)
        want = sr.store_bits(np.maximum(t, F(0)) if relu else t, dtype)
        assert np.array_equal(sr.store_bits(sr.bn_act_fwd(x, prm, relu), dtype), want), f"bn_act_fwd relu={relu}"
    assert np.array_equal(sr.relu_mask(x, prm), emu_t(x, prm) > 0), "ReLU mask"
    # bounded: statistics
    got = emu_stats(x, dtype)
    refs, bounds = sr.bn_stats(x, EPS, dtype)
    ws = [dr.worst(o, r, b)[0] for o, r, b in zip(got, refs, bounds)]
    # bounded: backward, both contraction forms, with and without accumulation
    L = sr.chain(S, C, dtype)
    rep = []
    for relu in (0, 1):
        gm = np.where(sr.relu_mask(x, prm), dy, 0.0) if relu else dy
        for contract in (False, True):
            prior = sr.stem_gradients((S, C), 14, dtype) if contract else None
            dg, db, coef, dx = emu_bwd(dy, x, prm, dtype, prior=prior, contract=contract, relu=relu)
            s = sr.bn_bwd_sums(gm, x, prm, L)
            w = [dr.worst(dg, *s["dgamma"])[0], dr.worst(db, *s["dbeta"])[0], dr.worst(coef, *s["coef"])[0],
                 dr.worst(dx, *sr.bn_bwd_dx(gm, x, prm, coef, dtype, prior=prior))[0]]
            rep.append(max(w))
            assert max(w) <= 1.0, f"relu={relu} contract={contract}: dgamma, dbeta, coef, dx = {w}"
    print(f"bn emulation dtype={dtype} S={S} C={C}: statistics {max(ws):.3f}, backward {max(rep):.3f}")
    assert max(ws) <= 1.0


def emu_avgpool(v32):
    N, H, W, C = v32.shape
    a, b, c, d = sr._win4(v32, H, W)
    return F(0.25) * ((a + b) + (c + d))


@pytest.mark.parametrize("N,H,W,C", sr.AVGPOOL_BN_SHAPES[:3] + sr.AVGPOOL_SHAPES)
def test_emulated_avgpool_kernels(N, H, W, C):
    prm = sr.stem_params(C, 21 + C)
    x = sr.stem_activations((N, H, W, C), prm, 22 + H)
    want = _store(emu_avgpool(np.maximum(emu_t(x, prm), F(0))))
    assert np.array_equal(dr.bf16_bits(sr.bn_act_avgpool_fwd(x, prm)), want), "bn_act_avgpool_fwd"
    assert np.array_equal(dr.bf16_bits(sr.avgpool_fwd(x)), _store(emu_avgpool(x.astype(F)))), "avgpool forward"
    dp = sr.stem_gradients((N, H // 2, W // 2, C), 23 + W)
    up = np.zeros((N, H, W, C), dtype=F)
    for yy in range(2 * (H // 2)):
        for xx in range(2 * (W // 2)):
            up[:, yy, xx] = dp[:, yy // 2, xx // 2].astype(F) * F(0.25)
    assert np.array_equal(dr.bf16_bits(sr.avgpool_bwd(dp, H, W)), _store(up)), "avgpool backward"
    S = N * H * W
    x2 = x.reshape(S, C)
    dg, db, coef, dx = emu_bwd(up.reshape(S, C), x2, prm, 1)
    gi = sr.pool_gradient(dp, x, prm, H, W)
    s = sr.bn_bwd_sums(gi, x2, prm, sr.chain(S, C, 1))
    w = [dr.worst(dg, *s["dgamma"])[0], dr.worst(db, *s["dbeta"])[0], dr.worst(coef, *s["coef"])[0],
         dr.worst(dx, *sr.bn_bwd_dx(gi, x2, prm, coef, 1))[0]]
    print(f"avgpool emulation {(N, H, W, C)}: dgamma, dbeta, coef, dx = " + ", ".join(f"{v:.3f}" for v in w))
    assert max(w) <= 1.0


def emu_maxpool(v32, last_wins=False):
    """The scalar loop of the kernel, pixel by pixel."""
    N, H, W, C = v32.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, idx = np.zeros((N, OH, OW, C), dtype=F), np.zeros((N, OH, OW, C), dtype=np.uint8)
    for oy in range(OH):
        for ox in range(OW):
            m = np.full((N, C), -np.inf, dtype=F)
            am = np.zeros((N, C), dtype=np.uint8)
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if 0 <= iy < H and 0 <= ix < W:
                        v = v32[:, iy, ix]
                        take = v >= m if last_wins else v > m
                        m, am = np.where(take, v, m), np.where(take, np.uint8(ky * 3 + kx), am)
            y[:, oy, ox], idx[:, oy, ox] = m, am
    return y, idx


def emu_maxpool_bwd(idx, dy_buf, lddy, C, N, H, W, ignore_ld=False):
    """Scatter form (the kernel gathers): window by window in ascending (oy, ox), which visits the windows of one pixel in the
    kernel's order.  dy_buf: the flat buffer with row stride lddy.  ignore_ld (mutant): reads it with stride C."""
    OH, OW = idx.shape[1:3]
    ld = C if ignore_ld else lddy
    dx = np.zeros((N, H, W, C), dtype=F)
    for n in range(N):
        for oy in range(OH):
            for ox in range(OW):
                op = (n * OH + oy) * OW + ox
                g = dy_buf[op * ld:op * ld + C].astype(F)
                for c in range(C):
                    ky, kx = divmod(int(idx[n, oy, ox, c]), 3)
                    dx[n, 2 * oy - 1 + ky, 2 * ox - 1 + kx, c] += g[c]
    return dx


def _maxpool_case(N, H, W, C, lddy):
    prm = sr.stem_params(C, 31 + C)
    x = sr.stem_activations((N, H, W, C), prm, 32 + H * W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    buf = sr.stem_gradients((N * OH * OW, lddy), 33 + W)
    return prm, x, buf, buf[:, :C].reshape(N, OH, OW, C)


@pytest.mark.parametrize("N,H,W,C,lddy", [s for s in sr.MAXPOOL_SHAPES if s[0] * s[1] * s[2] * s[3] <= 8000])
def test_emulated_maxpool_kernels(N, H, W, C, lddy):
    prm, x, buf, dy = _maxpool_case(N, H, W, C, lddy)
    xz = x.copy()
    xz[..., 2] = np.where(np.random.default_rng(1).random(x.shape[:-1]) < 0.5, -0.0, 0.0)     # zeros of both signs
    for v64, v32, what in ((xz, xz.astype(F), "maxpool"), (np.maximum(sr.bn_t(x, prm), 0.0), np.maximum(emu_t(x, prm), F(0)), "bn")):
        m, idx = sr.maxpool_fwd(v64)
        ye, ie = emu_maxpool(v32)
        assert np.array_equal(idx, ie), f"{what}: idx"
        assert np.array_equal(dr.bf16_bits(m), _store(ye)), f"{what}: y"
    assert np.array_equal(dr.bf16_bits(sr.maxpool_bwd(idx, dy, H, W)), _store(emu_maxpool_bwd(idx, buf.reshape(-1), lddy, C, N, H, W)))


def emu_conv0(x, Wt, mutant=False):
    A = sr.conv0_patches(x, top_reads_row0=mutant).astype(F)
    return A @ np.asarray(Wt, dtype=F).reshape(64, 147).T


def emu_tile_stats(v, n):
    v32 = np.asarray(v, dtype=F)
    P, C = v32.shape
    t = v32.reshape(P // n, n, C)[:, ::-1]
    s1, s2 = np.zeros((P // n, C), dtype=F), np.zeros((P // n, C), dtype=F)
    for i in range(n):
        s1, s2 = s1 + t[:, i], s2 + t[:, i] * t[:, i]
    m2 = (s2 - s1 * s1 / F(n)).astype(np.float64)
    s1 = s1.astype(np.float64)
    tot, q = s1.sum(0), (m2 + s1 * s1 / n).sum(0)
    var = np.maximum((q - tot * tot / P) / P, 0.0)
    return dr.f32(tot / P), dr.f32(var), dr.f32(1.0 / np.sqrt(var + EPS))


@pytest.mark.parametrize("N,H,W", sr.CONV0_SHAPES[:4] + [(9, 20, 8), (155, 20, 8)])
def test_emulated_conv0(N, H, W):
    x, Wt = sr.conv0_case(N, H, W)
    ref, bound = sr.conv0_fwd(x, Wt)
    y = dr.bits_to_f64(_store(emu_conv0(x, Wt).astype(np.float64)))
    wy = dr.worst(y, ref, bound)[0]
    b, n, allowed = dr.bias(y, ref)
    refs, bounds = sr.stats_tiles_unshifted(y, EPS, W)
    wst = max(dr.worst(o, r, e)[0] for o, r, e in zip(emu_tile_stats(y, W), refs, bounds))
    dy = sr.stem_gradients((N * (H // 2) * (W // 2), 64), 41 + W)
    A = sr.conv0_patches(x).astype(F)
    prior = dr.f32(np.random.default_rng(3).normal(0, 0.5, (64, 147)))
    ww = max(dr.worst((dy.astype(F).T @ A).astype(np.float64), *sr.conv0_wrw(x, dy, N, H, W))[0],
             dr.worst((prior.astype(F) + dy.astype(F).T @ A).astype(np.float64), *sr.conv0_wrw(x, dy, N, H, W, prior=prior))[0])
    print(f"conv0 emulation {(N, H, W)}: y {wy:.3f} bias {b:+.4f} statistics {wst:.3f} dW {ww:.3f}")
    assert max(wy, wst, ww) <= 1.0 and abs(b) <= allowed


def emu_gap(x, prm, g, HW):
    x32 = np.asarray(x, dtype=F)
    sc, _ = emu_prologue(prm)
    gam, beta, mu, rs = (np.asarray(prm[k], dtype=F) for k in ("gamma", "beta", "mean", "rstd"))
    acc = np.zeros((x32.shape[0], x32.shape[2]), dtype=F)
    for s in reversed(range(HW)):
        acc = acc + x32[:, s]
    m = acc * (F(1) / F(HW))
    out = (m - mu) * sc + beta
    g32 = np.asarray(g, dtype=F)
    xh = ((m - mu) * rs).astype(np.float64)
    a, q = g32.astype(np.float64).sum(0), (g32.astype(np.float64) * xh).sum(0)
    S = x32.shape[0] * HW
    coef = np.stack([a / S, q / S], 1).astype(F)
    dx = gam * rs * (g32[:, None, :] * (F(1) / F(HW)) - coef[:, 0] - (x32 - mu) * rs * coef[:, 1])
    return out, m, q.astype(F), a.astype(F), coef, dr.bits_to_f64(_store(dx.astype(np.float64)))


@pytest.mark.parametrize("B,HW,C", [s[:3] for s in sr.GAP_SHAPES])
def test_emulated_norm5_pool(B, HW, C):
    prm = sr.stem_params(C, 51 + C)
    x = sr.stem_activations((B, HW, C), prm, 52 + HW)
    g = dr.f32(np.random.default_rng(53).normal(1e-3, 1e-2, (B, C)))
    out, m, dg, db, coef, dx = emu_gap(x, prm, g, HW)
    f = sr.bn_gap_fwd(x, prm)
    s = sr.bn_gap_bwd_sums(g, m, prm, HW)
    w = [dr.worst(out, *f["out"])[0], dr.worst(m, *f["xmean"])[0], dr.worst(dg, *s["dgamma"])[0], dr.worst(db, *s["dbeta"])[0],
         dr.worst(coef, *s["coef"])[0], dr.worst(dx, *sr.bn_gap_bwd_dx(g, x, prm, coef))[0]]
    print(f"norm5 + pool emulation {(B, HW, C)}: out, xmean, dgamma, dbeta, coef, dx = " + ", ".join(f"{v:.3f}" for v in w))
    assert max(w) <= 1.0


@pytest.mark.parametrize("Sq,C,Co", sr.DP_SHAPES)
def test_emulated_transition_dp(Sq, C, Co):
    dy, Wt = sr.stem_gradients((Sq, Co), 61), dr.weights((Co, C), C, 62)
    dp = dr.bits_to_f64(_store((dy.astype(F) @ Wt.astype(F)).astype(np.float64)))
    ref, bound = sr.transition_dp(dy, Wt)
    w = dr.worst(dp, ref, bound)[0]
    b, n, allowed = dr.bias(dp, ref)
    print(f"transition dp emulation {(Sq, C, Co)}: {w:.3f}, bias {b:+.4f}")
    assert w <= 1.0 and abs(b) <= allowed


def test_plan_restated():
    """plan() at the shapes the issue names: the capped branch (1050 row blocks -> 934), the second channel tile."""
    assert sr.plan(8400, 1000, 0) == (934, 9, 1)
    assert sr.plan(333, 1028, 0)[2] == 2 and sr.plan(50, 2056, 1)[2] == 2
    assert sr.plan(777, 40, 1) == (2, 408, 1)
    L = sr.chain(50, 2056, 1)
    assert L[0] == 8 + 1 + 4 and L[-1] == 1 + 256 + 4


# ------------------------------------------------------------------------------------------------------------ 3. mutants
def _mutants():
    """name -> (caught, detail)."""
    res = {}
    dtype, S, C = 1, 777, 40
    prm, x, dy = _bn_case(dtype, S, C)
    L = sr.chain(S, C, dtype)
    gm = np.where(sr.relu_mask(x, prm), dy, 0.0)
    s = sr.bn_bwd_sums(gm, x, prm, L)

    def dx_worst(out, coef):
        return dr.worst(out, *sr.bn_bwd_dx(gm, x, prm, coef, dtype))[0]

    good = emu_bwd(dy, x, prm, dtype)
    assert dx_worst(good[3], good[2]) <= 1.0 and dr.worst(good[2], *s["coef"])[0] <= 1.0

    # 1. truncation: bits of an exact output, bound and bias of a bounded one
    t = sr.bn_act_fwd(x, prm, 1)
    bits_differ = not np.array_equal(dr.bf16_trunc_bits(t), dr.bf16_bits(t))
    m = emu_bwd(dy, x, prm, dtype, trunc=True)
    ref, _ = sr.bn_bwd_dx(gm, x, prm, m[2], dtype)
    b, n, allowed = dr.bias(m[3], ref)
    res["bf16 truncation instead of nearest-even"] = (bits_differ and abs(b) > allowed and b < -0.9,
                                                      f"bits differ {bits_differ}, dx {dx_worst(m[3], m[2]):.2f} of bound, bias {b:+.3f}")
    # 2. last maximum instead of first
    N, H, W, Cm, ld = 3, 17, 9, 64, 64
    pm, xm_, buf, dym = _maxpool_case(N, H, W, Cm, ld)
    v = np.maximum(sr.bn_t(xm_, pm), 0.0)
    _, idx = sr.maxpool_fwd(v)
    _, idx_last = emu_maxpool(v.astype(F), last_wins=True)
    res["last maximum instead of first"] = (not np.array_equal(idx, idx_last), f"{int((idx != idx_last).sum())} arg-max bytes differ")
    # 3. mask < 0 instead of <= 0
    m = emu_bwd(dy, x, prm, dtype, le_zero=False)
    res["mask < 0 instead of <= 0"] = (dx_worst(m[3], m[2]) > 1.0, f"dx {dx_worst(m[3], m[2]):.1f} of bound")
    # 4 .. 6, 9: the transition backward on an odd map
    N, H, W, Ct = 3, 5, 9, 64
    pt = sr.stem_params(Ct, 71)
    xt = sr.stem_activations((N, H, W, Ct), pt, 72)
    dp = sr.stem_gradients((N, H // 2, W // 2, Ct), 73)
    St = N * H * W
    x2 = xt.reshape(St, Ct)
    gi = sr.pool_gradient(dp, xt, pt, H, W)
    st = sr.bn_bwd_sums(gi, x2, pt, sr.chain(St, Ct, 1))

    def tr(g_unmasked, **kw):
        dg, db, coef, dx = emu_bwd(g_unmasked.reshape(St, Ct), x2, pt, 1, **kw)
        return max(dr.worst(coef, *st["coef"])[0], dr.worst(dx, *sr.bn_bwd_dx(gi, x2, pt, coef, 1))[0],
                   dr.worst(dg, *st["dgamma"])[0], dr.worst(db, *st["dbeta"])[0])

    assert tr(sr.avgpool_bwd(dp, H, W)) <= 1.0
    up = sr.avgpool_bwd(dp, H, W)
    up[:, H - 1], up[:, :, W - 1] = up[:, H - 2], up[:, :, W - 2]
    w = tr(up)
    res["pooled gradient given to the unpaired last row / column"] = (w > 1.0, f"{w:.1f} of a bound")
    w = tr(sr.avgpool_bwd(dp, H, W), coef_div=N * (H // 2) * 2 * (W // 2) * 2)
    res["mean terms over the pooled pixels instead of all S"] = (w > 1.0, f"{w:.1f} of a bound")
    w = tr(sr.avgpool_bwd(dp, H, W, drop_quarter=True))
    bits = not np.array_equal(dr.bf16_bits(sr.avgpool_bwd(dp, H, W, drop_quarter=True)), dr.bf16_bits(sr.avgpool_bwd(dp, H, W)))
    res["the /4 of the average pool dropped in the backward"] = (w > 1.0 and bits, f"{w:.1f} of a bound, bits differ {bits}")
    rpb = sr.plan(S, C, dtype)[1]
    m = emu_bwd(dy, x, prm, dtype, coef_div=rpb)
    w = dr.worst(m[2], *s["coef"])[0]
    res["coef divided by the block's rows instead of S"] = (w > 1.0, f"coef {w:.1f} of bound")
    # 7, 8: conv0
    N, H, W = 3, 12, 40
    xc, Wc = sr.conv0_case(N, H, W)
    ref, bound = sr.conv0_fwd(xc, Wc)
    ym = dr.bits_to_f64(_store(emu_conv0(xc, Wc, mutant=True).astype(np.float64)))
    w = dr.worst(ym, ref, bound)[0]
    res["conv0: the top row's first tap reads row 0 instead of zero"] = (w > 1.0, f"y {w:.1f} of bound")
    acc = emu_conv0(xc, Wc).astype(np.float64)
    y = dr.bits_to_f64(_store(acc))
    refs, bounds = sr.stats_tiles_unshifted(y, EPS, W)
    assert max(dr.worst(o, r, e)[0] for o, r, e in zip(emu_tile_stats(y, W), refs, bounds)) <= 1.0
    w = max(dr.worst(o, r, e)[0] for o, r, e in zip(emu_tile_stats(acc, W), refs, bounds))
    res["statistics of the unrounded instead of the stored y"] = (w > 1.0, f"{w:.1f} of a bound")
    # 10. max-pool backward that ignores lddy
    N, H, W, Cm, ld = 2, 6, 10, 40, 64
    pm, xm_, buf, dym = _maxpool_case(N, H, W, Cm, ld)
    _, idx = sr.bn_act_maxpool_fwd(xm_, pm)
    want = dr.bf16_bits(sr.maxpool_bwd(idx, dym, H, W))
    assert np.array_equal(want, _store(emu_maxpool_bwd(idx, buf.reshape(-1), ld, Cm, N, H, W)))
    got = _store(emu_maxpool_bwd(idx, buf.reshape(-1), ld, Cm, N, H, W, ignore_ld=True))
    res["a max-pool backward that ignores lddy"] = (not np.array_equal(want, got), f"{int((want != got).sum())} elements differ in bits")
    return res


def test_every_mutant_is_caught():
    res = _mutants()
    for name, (caught, detail) in res.items():
        print(f"{name:62s} {'caught' if caught else 'MISSED'}   {detail}")
    assert len(res) == 10
    for name, (caught, detail) in res.items():
        assert caught, f"mutant not caught: {name} ({detail})"
