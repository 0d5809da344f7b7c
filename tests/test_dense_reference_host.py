"""tests/dense_reference.py checked on the CPU: with every rounding point switched off it is fp64 autograd of the torchvision
_DenseLayer formulas (train-mode batch norm); an fp32 emulation of each kernel's arithmetic (torch fp32 matmul, the same rounding
points) stays inside every bound at every shape the GPU tests use; the ambiguous share of the prologue stays under its cap; and
value-only mutants of the emulation each exceed a bound (the table says which of them the older whole-tensor tolerance
|err| <= rel*max|ref| lets through)."""
import numpy as np
import pytest
import torch

import dense_reference as dr

EPS = 1e-5
OLD_TOL = {"z": 6e-3, "y": 6e-3, "gbuf": 8e-3, "dz": 1.2e-2}      # assert_close_scaled's rel in the older dense-layer tests


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _mm(a, b):
    """fp32 matmul of float64-held values."""
    return (_t(a) @ _t(b)).numpy().astype(np.float64)


def _store(v, trunc=False):
    return dr.bits_to_f64(dr.bf16_trunc_bits(v) if trunc else dr.bf16_bits(v))


def emu_conv1x1(x, prm, W1, trunc=False, drop_last_k=False):
    p = dr.Prologue(x, *dr.bn(prm))
    a = p.a.copy()
    if drop_last_k:
        a[:, -1] = 0.0
    return _store(_mm(a, W1.T), trunc)


def emu_conv3x3(z, B, H, W, prm, W2, leak_tap=False):
    """leak_tap: tap (1, 2) of the pixels in the last column reads the flat neighbour p + 1 instead of zero."""
    p = dr.Prologue(z, *dr.bn(prm))
    S = B * H * W
    ap = dr._pad(p.a, B, H, W)
    acc = np.zeros((S, 32), dtype=np.float32)
    for ky, kx, sy, sx in dr._taps(H, W):
        acc = (acc + _mm(ap[:, sy, sx, :].reshape(S, -1), W2[:, ky, kx, :].T)).astype(np.float32)
    if leak_tap:
        last = np.nonzero((np.arange(S) % W == W - 1) & (np.arange(S) + 1 < S))[0]
        acc[last] = (acc[last] + _mm(p.a[last + 1], W2[:, 1, 2, :].T)).astype(np.float32)
    return _store(acc.astype(np.float64))


def emu_tail(dy, B, H, W, W2, z, prm, drop_c2=False, rows=False):
    """(g2, dz, dgamma2, dbeta2) in fp32 with the flat kernel's rounding points, or the row-walking form's dgamma2 =
    rstd*(sum g2*z - mean*sum g2)."""
    p = dr.Prologue(z, *dr.bn(prm))
    S = B * H * W
    dp = dr._pad(dy, B, H, W)
    acc = np.zeros((S, 128), dtype=np.float32)
    for ky, kx, _, _ in dr._taps(H, W):
        acc = (acc + _mm(dp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, :].reshape(S, -1), W2[:, ky, kx, :])).astype(np.float32)
    g2 = _store(np.where(p.mask, acc, 0.0))
    f = np.float32
    mu, rs, gam = (v.astype(f) for v in (prm["mean"], prm["rstd"], prm["gamma"]))
    zh = (z.astype(f) - mu) * rs
    db = _t(g2).sum(0).numpy()
    dg = (_t(g2) * torch.from_numpy(zh)).sum(0).numpy()
    if rows:
        dg = (rs * ((_t(g2) * _t(z)).sum(0).numpy() - mu * db)).astype(f)
    c1, c2 = (db.astype(np.float64) / S).astype(f), (dg.astype(np.float64) / S).astype(f)
    if drop_c2:
        c2 = np.zeros_like(c2)
    dz = (gam * rs) * (g2.astype(f) - c1 - zh * c2)
    return g2, _store(dz), dg.astype(np.float64), db.astype(np.float64)


def emu_head(dz, W1, x, prm, gbuf, mean_scale=1.0):
    """(gbuf', dgamma, dbeta) of mcl_dense_bn1_bwd in fp32."""
    p = dr.Prologue(x, *dr.bn(prm))
    S = x.shape[0]
    f = np.float32
    g = np.where(p.mask, _mm(dz, W1), 0.0).astype(f)
    mu, rs, sc = prm["mean"].astype(f), prm["rstd"].astype(f), p.sc.astype(f)
    xf = x.astype(f)
    s1 = _t(g).sum(0).numpy()
    s2 = rs * ((_t(g) * _t(xf)).sum(0).numpy() - mu * s1)
    c1 = ((s1.astype(np.float64) / S) * mean_scale).astype(f)
    c2 = (s2.astype(np.float64) / S).astype(f)
    ka = -sc * c2 * rs
    kb = -ka * mu - sc * c1
    delta = _store(sc * g + (ka * xf + kb))
    return _store(gbuf + delta), s2.astype(np.float64), s1.astype(np.float64)


def emu_delta(dz, W1, x, prm, c1, c2, premultiplied=False):
    """The fp32 delta of bn1_bwd_kernel<1> (premultiplied False) / <2> (True) before its bf16 store, the means given."""
    p = dr.Prologue(x, *dr.bn(prm))
    f = np.float32
    g = np.where(p.mask, _mm(dz, W1), 0.0).astype(f)
    mu, rs, sc = prm["mean"].astype(f), prm["rstd"].astype(f), p.sc.astype(f)
    s = np.ones_like(sc) if premultiplied else sc
    ka = -s * np.asarray(c2, dtype=f) * rs
    kb = -ka * mu - s * np.asarray(c1, dtype=f)
    return (sc * g + (ka * x.astype(f) + kb)).astype(f)


def emu_bn1_wrw(dz, W1, x, prm):
    """The Gram form in fp32: (dW1, dgamma, dbeta)."""
    p = dr.Prologue(x, *dr.bn(prm))
    f = np.float32
    m = p.mask.astype(np.float64)
    R, Qx = _mm(dz.T, m).astype(f), _mm(dz.T, m * x).astype(f)
    g, b, mu, rs = (prm[k].astype(f) for k in ("gamma", "beta", "mean", "rstd"))
    Q = rs * (Qx - mu * R)
    W = W1.astype(f)
    return (g * Q + b * R).astype(np.float64), (W * Q).sum(0).astype(np.float64), (W * R).sum(0).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ cases
conv1x1_case, tail_case, head_case = dr.conv1x1_case, dr.tail_case, dr.head_case     # the GPU tests' own data


def emu_stats_tiles(v, bm):
    """tile_stats scheme in fp32: per tile shifted sums, fmaf(n, shift, s1), s2 - s1^2/n; Chan's merge in double."""
    f = np.float32
    S = v.shape[0]
    tot, q = 0.0, 0.0
    for r0 in range(0, S, bm):
        t = v[r0:r0 + bm].astype(f)
        n = f(t.shape[0])
        d = (t - t[0]).astype(f)
        s1, s2 = _t(d).sum(0).numpy(), _t(d * d).sum(0).numpy()
        ts = (n * t[0] + s1).astype(f)
        m2 = (s2 - s1 * s1 / n).astype(f)
        tot = tot + ts.astype(np.float64)
        q = q + m2.astype(np.float64) + ts.astype(np.float64) ** 2 / float(n)
    m = tot / S
    var = np.maximum((q - tot * tot / S) / S, 0.0)
    return dr.f32(m), dr.f32(var), dr.f32(1.0 / np.sqrt(var + EPS))


def emu_stats_sums(v, nmax):
    """raw-sums scheme in fp32: per unit of nmax pixels sum v, sum v^2; added in double."""
    S = v.shape[0]
    tot, q = 0.0, 0.0
    for r0 in range(0, S, nmax):
        t = _t(v[r0:r0 + nmax])
        tot = tot + t.sum(0).numpy().astype(np.float64)
        q = q + (t * t).sum(0).numpy().astype(np.float64)
    m = tot / S
    var = np.maximum((q - tot * tot / S) / S, 0.0)
    return dr.f32(m), dr.f32(var), dr.f32(1.0 / np.sqrt(var + EPS))


def _stats_worst(got, refs_bounds):
    refs, bounds = refs_bounds
    return max(dr.worst(o, r, b)[0] for o, r, b in zip(got, refs, bounds))


def _amb_ok(p, what):
    assert p.amb_share <= dr.AMB_CAP, f"{what}: ambiguous share {p.amb_share:.2e} over the cap {dr.AMB_CAP:g}: change the seed"


# ------------------------------------------------------------------------------------------------------------ autograd
def _layer_autograd(xs, prms1, W1s, prms2, W2s, B, H, W, dys):
    """fp64 autograd of consecutive _DenseLayers on one concat buffer: xs (S, C0) block input; layer l reads C0 + 32 l channels.
    Loss = sum_l <y_l, dys[l]> + what the later layers make of y_l.  Returns per-layer tensors and gradients."""
    S = B * H * W
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    x0 = tt(xs)
    feats, keep = [x0], []
    loss = 0.0
    for l, (p1, W1, p2, W2) in enumerate(zip(prms1, W1s, prms2, W2s)):
        buf = torch.cat(feats, 1)
        g1, b1, g2, b2 = tt(p1["gamma"]), tt(p1["beta"]), tt(p2["gamma"]), tt(p2["beta"])
        w1, w2 = tt(W1), tt(W2)
        a = torch.relu(torch.nn.functional.batch_norm(buf, None, None, g1, b1, True, 0.0, EPS))
        z = a @ w1.T
        z.retain_grad()
        a2 = torch.relu(torch.nn.functional.batch_norm(z, None, None, g2, b2, True, 0.0, EPS))
        y = torch.nn.functional.conv2d(a2.reshape(B, H, W, 128).permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2), padding=1)
        y = y.permute(0, 2, 3, 1).reshape(S, 32)
        y.retain_grad()
        loss = loss + (y * torch.tensor(dys[l])).sum()
        feats.append(y)
        keep.append(dict(buf=buf, z=z, y=y, g1=g1, b1=b1, g2=g2, b2=b2, w1=w1, w2=w2))
    loss.backward()
    return x0, keep


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    err = float(np.abs(a - b).max()) / scale
    assert err <= 1e-12, f"{what}: {err:.3e} of max"


@pytest.mark.parametrize("B,H,W,C0,layers", [(2, 5, 3, 16, 1), (3, 4, 6, 24, 2)])
def test_restatement_without_rounding_is_autograd(B, H, W, C0, layers):
    """Forward and every gradient of one layer, and of two layers sharing a concat buffer (the second layer's head adds into the
    gradient channels the first layer's tail then consumes), against fp64 autograd to 1e-12 of max."""
    S = B * H * W
    rng = np.random.default_rng(7)
    xs = rng.normal(size=(S, C0))
    prms1 = [dr.layer_params(C0 + 32 * l, 10 + l) for l in range(layers)]
    prms2 = [dr.layer_params(128, 20 + l) for l in range(layers)]
    for p in prms1 + prms2:
        p["beta"] = p["beta"] * 0.0 + rng.normal(0, 0.3, p["beta"].shape)      # no dead channel: keep every gradient alive
    W1s = [rng.normal(0, 0.2, (128, C0 + 32 * l)) for l in range(layers)]
    W2s = [rng.normal(0, 0.1, (32, 3, 3, 128)) for l in range(layers)]
    dys = [rng.normal(size=(S, 32)) for _ in range(layers)]
    x0, keep = _layer_autograd(xs, prms1, W1s, prms2, W2s, B, H, W, dys)

    # forward, layer by layer, statistics from the restatement's own tensors
    buf = xs.copy()
    fwd = []
    for l in range(layers):
        m1, v1, r1 = dr.stats_ref(buf, EPS)
        z, _, p1 = dr.conv1x1_fwd(buf, prms1[l]["gamma"], prms1[l]["beta"], m1, r1, W1s[l], rounding=False)
        m2, v2, r2 = dr.stats_ref(z, EPS)
        y, _, p2 = dr.conv3x3_fwd(z, B, H, W, prms2[l]["gamma"], prms2[l]["beta"], m2, r2, W2s[l], rounding=False)
        _close(z, keep[l]["z"].detach().numpy(), f"z{l}")
        _close(y, keep[l]["y"].detach().numpy(), f"y{l}")
        fwd.append(dict(x=buf, z=z, st1=(m1, r1), st2=(m2, r2), a=p1.a, a2=p2.a))
        buf = np.concatenate([buf, y], 1)
    # backward, last layer first, on one gradient buffer
    C = buf.shape[1]
    gbuf = np.zeros((S, C))
    for l in range(layers):
        gbuf[:, C0 + 32 * l:C0 + 32 * (l + 1)] = dys[l]
    for l in reversed(range(layers)):
        Cl = C0 + 32 * l
        f = fwd[l]
        dy = gbuf[:, Cl:Cl + 32]
        _close(dy, keep[l]["y"].grad.numpy(), f"dy{l}")
        g2, _, _ = dr.tail_g2(dy, B, H, W, W2s[l], f["z"], prms2[l]["gamma"], prms2[l]["beta"], *f["st2"], rounding=False)
        t = dr.tail_from_g2(g2, f["z"], prms2[l]["gamma"], *f["st2"], 128, False, rounding=False)
        dz = t["dz"][0]
        _close(dz, keep[l]["z"].grad.numpy(), f"dz{l}")
        _close(t["dgamma"][0], keep[l]["g2"].grad.numpy(), f"dgamma2 {l}")
        _close(t["dbeta"][0], keep[l]["b2"].grad.numpy(), f"dbeta2 {l}")
        _close(dr.conv3x3_wrw(dy, f["a2"], B, H, W)[0], keep[l]["w2"].grad.numpy(), f"dW2 {l}")
        _close(dr.conv1x1_wrw(dz, f["a"])[0], keep[l]["w1"].grad.numpy(), f"dW1 {l}")
        h = dr.Head(dz, W1s[l], f["x"], prms1[l]["gamma"], prms1[l]["beta"], *f["st1"], rounding=False)
        _close(h.dgamma, keep[l]["g1"].grad.numpy(), f"dgamma1 {l}")
        _close(h.dbeta, keep[l]["b1"].grad.numpy(), f"dbeta1 {l}")
        gbuf[:, :Cl] += h.delta()[0]
    _close(gbuf[:, :C0], x0.grad.numpy(), "block-input gradient")


# ------------------------------------------------------------------------------------------------------------ emulation in bounds
@pytest.mark.parametrize("S,K", [(s[0], s[1]) for s in dr.CONV1X1_SHAPES])
def test_emulated_conv1x1_within_bounds(S, K):
    prm, x, W1 = conv1x1_case(S, K)
    ref, bound, p = dr.conv1x1_fwd(x, *dr.bn(prm), W1)
    _amb_ok(p, f"conv1x1 ({S},{K})")
    z = emu_conv1x1(x, prm, W1)
    w, at = dr.worst(z, ref, bound)
    b, n, allowed = dr.bias(z, ref)
    print(f"conv1x1 emulation ({S},{K}): worst ratio {w:.3f} at {at}, ambiguous share {p.amb_share:.2e}, bias {b:+.4f} (N={n})")
    assert w <= 1.0
    assert abs(b) <= allowed
    bm = 128 if S >= 32768 else 64
    ws = _stats_worst(emu_stats_tiles(z, bm), dr.stats_tiles(z, EPS, bm))
    print(f"conv1x1 emulation ({S},{K}): statistics of z, tile scheme ({bm} rows): worst ratio {ws:.3f}")
    assert ws <= 1.0


@pytest.mark.parametrize("B,H,W", [s[:3] for s in dr.CONV3X3_FLAT + dr.CONV3X3_ROWS])
def test_emulated_tail_within_bounds(B, H, W):
    prm, z, W2, dy = tail_case(B, H, W)
    ref, bound, p = dr.conv3x3_fwd(z, B, H, W, *dr.bn(prm), W2)
    _amb_ok(p, f"conv3x3 ({B},{H},{W})")
    y = emu_conv3x3(z, B, H, W, prm, W2)
    wy, at = dr.worst(y, ref, bound)
    gref, gbound, _ = dr.tail_g2(dy, B, H, W, W2, z, *dr.bn(prm))
    rows = dr.rows_applicable(H, W)
    g2, dz, dg, db = emu_tail(dy, B, H, W, W2, z, prm, rows=rows)
    wg, _ = dr.worst(g2, gref, gbound)
    t = dr.tail_from_g2(g2, z, prm["gamma"], prm["mean"], prm["rstd"], dr.bwd_rows_unit_pixels(B, H, W) if rows else 128, rows)
    if rows:
        n = dr.fwd_rows_unit_pixels(B, H, W)
        wst = _stats_worst(emu_stats_sums(y, n), dr.stats_sums(y, EPS, n))
    else:
        wst = _stats_worst(emu_stats_tiles(y, 128), dr.stats_tiles(y, EPS, 128))
    wz, _ = dr.worst(dz, *t["dz"])
    wdg, _ = dr.worst(dg, *t["dgamma"])
    wdb, _ = dr.worst(db, *t["dbeta"])
    print(f"tail emulation ({B},{H},{W}): worst ratio y {wy:.3f} g2 {wg:.3f} dz {wz:.3f} dgamma2 {wdg:.3f} dbeta2 {wdb:.3f}, "
          f"statistics of y ({'raw sums' if rows else 'tiles'}) {wst:.3f}, ambiguous share {p.amb_share:.2e}")
    assert max(wy, wg, wz, wdg, wdb, wst) <= 1.0


@pytest.mark.parametrize("S,C", [s[:2] for s in dr.HEAD_SHAPES + dr.PAIR_SHAPES])
def test_emulated_head_within_bounds(S, C):
    prm, x, W1, dz, gbuf = head_case(S, C)
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    _amb_ok(h.p, f"head ({S},{C})")
    out, dg, db = emu_head(dz, W1, x, prm, gbuf)
    ref, bound = dr.gbuf_add(gbuf, *h.delta())
    wg, at = dr.worst(out, ref, bound)
    pg = h.param_grads()
    wdg, _ = dr.worst(dg, *pg["dgamma"])
    wdb, _ = dr.worst(db, *pg["dbeta"])
    print(f"head emulation ({S},{C}): worst ratio gbuf {wg:.3f} at {at} dgamma {wdg:.3f} dbeta {wdb:.3f}, "
          f"ambiguous share {h.p.amb_share:.2e}")
    assert max(wg, wdg, wdb) <= 1.0


_pair_case = dr.pair_case


def _emu_pair(S, C, twice=False, stale=False):
    """Worst ratios of the emulated two-layer forms: (pair, single-pass second pass).  twice: each layer's delta rounded to bf16
    before the two are added.  stale: the second pass of the single-pass sequence ignores the previous pass's mean terms."""
    prmA, prmB, x, gb, dzA, dzB, W1A, W1B = _pair_case(S, C)
    hA, hB = dr.Head(dzA, W1A, x, *dr.bn(prmA)), dr.Head(dzB, W1B, x[:, :C], *dr.bn(prmB))
    cA, cB = (dr.f32(np.stack([h.c1, h.c2], 1)) for h in (hA, hB))
    dA = emu_delta(dzA, W1A, x, prmA, cA[:, 0], cA[:, 1])[:, :C]
    dB = emu_delta(dzB, W1B, x[:, :C], prmB, cB[:, 0], cB[:, 1])
    d = _store(dA) + _store(dB) if twice else (dA + dB).astype(np.float32)
    out_pair = out = _store(gb[:, :C] + _store(d))
    w_pair = dr.worst(out, *dr.gbuf_add(gb[:, :C], *dr.pair_delta(hA, cA[:C], hB, cB, C)))[0]
    # single pass: layer A's terms (premultiplied by gamma*rstd) reach layer B's pass one pass late
    kA, _ = dr.head_kacc(hA, prmA["gamma"])
    kA = dr.f32(kA)
    z = np.zeros(C)
    used = np.zeros_like(kA[:C]) if stale else kA[:C]
    out = _store(gb[:, :C] + _store(emu_delta(dzB, W1B, x[:, :C], prmB, used[:, 0], used[:, 1], premultiplied=True)))
    w_sp = dr.worst(out, *dr.gbuf_add(gb[:, :C], *hB.delta(kA[:C, 0], kA[:C, 1], z, z, premultiplied=True)))[0]
    ref_pair = gb[:, :C] + dr.pair_delta(hA, cA[:C], hB, cB, C)[0]
    ref_sp = gb[:, :C] + hB.delta(kA[:C, 0], kA[:C, 1], z, z, premultiplied=True)[0]
    return w_pair, w_sp, hA.p.amb_share, (out_pair, ref_pair), (out, ref_sp)


@pytest.mark.parametrize("S,C", [s[:2] for s in dr.PAIR_SHAPES + dr.HEAD_SHAPES])
def test_emulated_pair_and_single_pass_within_bounds(S, C):
    w_pair, w_sp, amb, _, _ = _emu_pair(S, C)
    print(f"two-layer emulation ({S},{C}): worst ratio pair {w_pair:.3f}, single pass with previous terms {w_sp:.3f}, "
          f"ambiguous share {amb:.2e}")
    assert amb <= dr.AMB_CAP
    assert max(w_pair, w_sp) <= 1.0


@pytest.mark.parametrize("S,C", [s[:2] for s in dr.HEAD_SHAPES])
def test_emulated_gram_form_within_bounds(S, C):
    prm, x, W1, dz, _ = head_case(S, C)
    r = dr.bn1_wrw(dz, W1, x, *dr.bn(prm), dr.wrw_slab_terms(S))
    dW, dg, db = emu_bn1_wrw(dz, W1, x, prm)
    ws = [dr.worst(o, *r[k])[0] for o, k in ((dW, "dW"), (dg, "dgamma"), (db, "dbeta"))]
    # the Gram form is the same sums as the two-pass head, and dz^T of the unrounded activation
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    _close(r["dbeta"][0], h.dbeta, "dbeta, Gram form vs head")
    _close(r["dgamma"][0], h.dgamma, "dgamma, Gram form vs head")
    print(f"Gram-form emulation ({S},{C}): worst ratio dW1 {ws[0]:.3f} dgamma {ws[1]:.3f} dbeta {ws[2]:.3f}")
    assert max(ws) <= 1.0


@pytest.mark.parametrize("what,shape", [("3x3", s) for s in dr.WRW3_SHAPES] + [("1x1", s) for s in dr.WRW1_SHAPES])
def test_emulated_weight_gradients_within_bounds(what, shape):
    if what == "3x3":
        B, H, W = shape
        S = B * H * W
        prm, z, _, dy = tail_case(B, H, W)
        p = dr.Prologue(z, *dr.bn(prm))
        ref, e = dr.conv3x3_wrw(dy, p.a, B, H, W, e_a=p.amb_w, nterms=dr.wrw3_terms(S))
        ap = dr._pad(p.a, B, H, W)
        out = np.stack([_mm(dy.T, ap[:, sy, sx, :].reshape(S, -1)) for _, _, sy, sx in dr._taps(H, W)], 1).reshape(32, 3, 3, 128)
    else:
        S, M, N = shape
        prm, a, dz = dr.wrw1_case(S, M, N)
        p = dr.Prologue(a, *dr.bn(prm))
        ref, e = dr.conv1x1_wrw(dz, p.a, e_a=p.amb_w, nterms=dr.wrw_slab_terms(S))
        out = _mm(dz.T, p.a)
    w, at = dr.worst(out, ref, e)
    print(f"weight-gradient emulation {what} {shape}: worst ratio {w:.4f}, ambiguous share {p.amb_share:.2e}")
    assert p.amb_share <= dr.AMB_CAP and w <= 1.0


# ------------------------------------------------------------------------------------------------------------ mutants
def _old_passes(out, ref, rel):
    """assert_close_scaled of the older tests against the float64 reference."""
    return bool(np.abs(out - ref).max() <= rel * np.abs(ref).max() + 1e-12)


def _mutants():
    """name -> (worst ratio against the bound, passes the older whole-tensor tolerance)."""
    res = {}
    prm, x, W1 = conv1x1_case(300, 96)
    ref, bound, _ = dr.conv1x1_fwd(x, *dr.bn(prm), W1)
    z = emu_conv1x1(x, prm, W1, trunc=True)
    res["truncated output rounding (z)"] = (dr.worst(z, ref, bound)[0], _old_passes(z, ref, OLD_TOL["z"]), dr.bias(z, ref)[0])
    z = emu_conv1x1(x, prm, W1, drop_last_k=True)
    res["one K-tail channel dropped (z)"] = (dr.worst(z, ref, bound)[0], _old_passes(z, ref, OLD_TOL["z"]), None)

    B, H, W = 3, 10, 6
    prm, zz, W2, dy = tail_case(B, H, W)
    ref, bound, _ = dr.conv3x3_fwd(zz, B, H, W, *dr.bn(prm), W2)
    y = emu_conv3x3(zz, B, H, W, prm, W2, leak_tap=True)
    res["one border tap not zeroed (y)"] = (dr.worst(y, ref, bound)[0], _old_passes(y, ref, OLD_TOL["y"]), None)
    g2, _, _, _ = emu_tail(dy, B, H, W, W2, zz, prm)
    _, dzm, _, _ = emu_tail(dy, B, H, W, W2, zz, prm, drop_c2=True)
    t = dr.tail_from_g2(g2, zz, prm["gamma"], prm["mean"], prm["rstd"], 128, False)
    res["c2 term dropped (dz)"] = (dr.worst(dzm, *t["dz"])[0], _old_passes(dzm, t["dz"][0], OLD_TOL["dz"]), None)

    prm, x, W1, dz, gbuf = head_case(300, 96)
    # a non-zero mean of g, as in training (the loss gradient of a layer is not centred): dz with an offset
    dz = dr.bf16(dz + 3e-3)
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    ref, bound = dr.gbuf_add(gbuf, *h.delta())
    out, _, _ = emu_head(dz, W1, x, prm, gbuf, mean_scale=1.02)
    res["mean term scaled by 1.02 (gbuf)"] = (dr.worst(out, ref, bound)[0], _old_passes(out, ref, OLD_TOL["gbuf"]), None)
    good = _emu_pair(300, 96)
    m = _emu_pair(300, 96, stale=True)
    res["stale kprev (gbuf, single pass)"] = (m[1], _old_passes(*m[4], OLD_TOL["gbuf"]), None)
    m = _emu_pair(300, 96, twice=True)
    res["pair form rounded twice (gbuf)"] = (m[0], _old_passes(*m[3], OLD_TOL["gbuf"]), None)
    assert max(good[:2]) <= 1.0
    return res


def test_every_mutant_exceeds_a_bound():
    res = _mutants()
    print("mutant                                   worst ratio   older tolerance")
    for name, (w, old, b) in res.items():
        extra = f"   bias {b:+.3f}" if b is not None else ""
        print(f"{name:40s} {w:11.2f}   {'passes' if old else 'fails'}{extra}")
        assert w > 1.0, f"mutant not caught: {name} (worst ratio {w:.3f})"
    assert res["truncated output rounding (z)"][2] < -0.9
