"""The row-tile WALK of the BatchNorm-1 dx kernels (bn1_bwd_kernel<1>, <2> and bn1_dx_pair_kernel): a workgroup keeps one
column tile and walks the 64-row tiles blockIdx.x, blockIdx.x + gridDim.x, ..., requesting the next tile's operands while it
works on the current one.  The shapes of test_dense_exact_gpu.py (S <= 300) give every workgroup ONE tile, so the walk has
tests of its own here, with the same discipline: every buffer between guard words, NaN sentinels in every column and output a
launch may not use, guards and untouched regions bit-unchanged afterwards, every output finite.

The launch rule these shapes are derived from (csrc/dense_bwd.hip, the hosts of the four entry points):

    nrt = ceil(S / 64) row tiles,  nct = ceil(nc / 128) column tiles (nc = the channels of the launch),
    gx  = min(ceil(gcap / nct), nrt) workgroups per column tile,
    gcap = 512 if S >= 50000 else 768   (mcl_dense_bn1_dx, _dx_window, _dx_sums);   gcap = 512   (mcl_dense_bn1_dx_pair).

Workgroup b of a column tile walks the tiles b, b + gx, ...: ceil or floor of nrt / gx of them.  _walk() restates the rule and
every walking test asserts what it needs of it (three tiles or more for every workgroup, one more for some, a ragged last tile);
if the rule changes, re-derive S."""
import numpy as np
import pytest
import torch

import dense_reference as dr
from test_dense_exact_gpu import L, Mat, _check, _st, _within, out_vec, vec  # noqa: F401  (L is the library fixture)

pytestmark = pytest.mark.gpu

BLOCK = 2048          # rows per call of the blocked form: 32 row tiles <= gx for every shape here -> one tile per workgroup


def _walk(S, nc, pair=False):
    """(gx, fewest, most row tiles a workgroup walks, rows of the last tile) under the launch rule in the module docstring."""
    nrt, nct = -(-S // 64), -(-nc // 128)
    gcap = 512 if (pair or S >= 50000) else 768
    gx = min(-(-gcap // nct), nrt)
    return gx, nrt // gx, -(-nrt // gx), S - 64 * (nrt - 1)


def _assert_walks(S, nc, pair=False):
    gx, lo, hi, last = _walk(S, nc, pair)
    assert lo >= 3 and hi == lo + 1 and 0 < last < 64, (gx, lo, hi, last)
    for r0 in range(0, S, BLOCK):                      # the blocked form: one tile per workgroup
        assert _walk(min(BLOCK, S - r0), nc, pair)[2] == 1


def _rows(m, r0):
    """Device address of row r0 of a Mat (column 0)."""
    return m.ptr() + m.isz * r0 * m.ld


def _blocks(S):
    return [(r0, min(BLOCK, S - r0)) for r0 in range(0, S, BLOCK)]


def _same_bits(what, a, b):
    assert torch.equal(a.base, b.base), f"{what}: the walked call and the 2048-row calls differ in " \
                                        f"{int((a.base != b.base).sum())} words"


def _finite(what, m, c0, n):
    assert np.isfinite(m.get(c0, n)).all(), f"{what}: non-finite output"


def _coef(C, seed):
    """Plausible (mean g, mean g*xhat) per channel, fp32 values, (C, 2)."""
    return dr.f32(np.random.default_rng(seed).normal(0.0, 2e-3, (C, 2)))


# ---------------------------------------------------------------------------------------------------- 1. walk invariance
@pytest.fixture(scope="module")
def head_walk():
    """C = 1000 of ld = 1032 (8 column tiles, the last with 104 valid channels), S = 18533 = 289 * 64 + 37."""
    S, C, ld = 18533, 1000, 1032
    prm, x, W1, dz, gb = dr.head_case(S, C)
    return S, C, ld, prm, x, W1, dz, gb


def test_dx_walk_invariance(L, head_walk):
    """mcl_dense_bn1_dx on S rows == the same call on consecutive 2048-row blocks, bit for bit (the result is row-local).
    gx = min(ceil(768 / 8), 290) = 96: workgroups walk 3 or 4 tiles, the last tile has 37 rows."""
    S, C, ld, prm, x, W1, dz, gb = head_walk
    _assert_walks(S, C)
    xb, dzb, wb = Mat(S, ld).set(0, x).freeze(), Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(0, W1).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    cb = vec(_coef(C, 11).reshape(-1)).freeze()
    full, blocked = Mat(S, ld).set(0, gb).freeze(), Mat(S, ld).set(0, gb)
    _check(L.mcl_dense_bn1_dx(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], cb.ptr(), full.ptr(), ld, _st()),
           "mcl_dense_bn1_dx")
    for r0, n in _blocks(S):
        _check(L.mcl_dense_bn1_dx(_rows(dzb, r0), wb.ptr(), C, _rows(xb, r0), ld, n, *[p.ptr() for p in pv], cb.ptr(),
                                  _rows(blocked, r0), ld, _st()), "mcl_dense_bn1_dx (block)")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1"), (cb, "coef")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    full.unchanged("gbuf", 0, C)
    _finite("gbuf", full, 0, C)
    _same_bits("mcl_dense_bn1_dx", full, blocked)


def test_dx_sums_walk_invariance(L, head_walk):
    """The gradient-buffer columns of mcl_dense_bn1_dx_sums (have_prev = 1), as above; each block call gets a fresh copy of the
    previous pass's terms because finalize overwrites them."""
    S, C, ld, prm, x, W1, dz, gb = head_walk
    _assert_walks(S, C)
    xb, dzb, wb = Mat(S, ld).set(0, x).freeze(), Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(0, W1).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    kin = _coef(C, 12).reshape(-1)
    full, blocked = Mat(S, ld).set(0, gb).freeze(), Mat(S, ld).set(0, gb)

    def call(r0, n, gbuf):
        ws = Mat(1, int(L.mcl_dense_bn1_bwd_workspace_floats(n, C)), "f32").freeze()
        dgb, dbb, kp = out_vec(C).freeze(), out_vec(C).freeze(), vec(kin).freeze()
        _check(L.mcl_dense_bn1_dx_sums(_rows(dzb, r0), wb.ptr(), C, _rows(xb, r0), ld, n, *[p.ptr() for p in pv], ws.ptr(),
                                       dgb.ptr(), dbb.ptr(), 0, kp.ptr(), 1, _rows(gbuf, r0), ld, _st()), "mcl_dense_bn1_dx_sums")
        torch.cuda.synchronize()
        for b, w in ((ws, ws.ld), (dgb, C), (dbb, C), (kp, 2 * C)):
            b.unchanged("output", 0, w)
            _finite("sums", b, 0, w if b is not ws else 2 * C * (-(-n // 64)))

    call(0, S, full)
    for r0, n in _blocks(S):
        call(r0, n, blocked)
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    full.unchanged("gbuf", 0, C)
    _finite("gbuf", full, 0, C)
    _same_bits("mcl_dense_bn1_dx_sums", full, blocked)


def test_dx_pair_walk_invariance(L):
    """mcl_dense_bn1_dx_pair, C = 1000 (layer A reads 1032), S = 18533: gx = min(ceil(512 / 8), 290) = 64, workgroups walk 4
    or 5 tiles."""
    S, C = 18533, 1000
    C2 = ld = C + 32
    gx, lo, hi, last = _walk(S, C, pair=True)
    assert (lo, hi) == (4, 5) and 0 < last < 64
    _assert_walks(S, C, pair=True)
    prmA, prmB, x, gb, dzA, dzB, W1A, W1B = dr.pair_case(S, C)
    xb = Mat(S, ld).set(0, x).freeze()
    bufs = dict(dzA=Mat(S, 128).set(0, dzA), dzB=Mat(S, 128).set(0, dzB), WA=Mat(128, C2).set(0, W1A), WB=Mat(128, C).set(0, W1B),
                gA=vec(prmA["gamma"]), bA=vec(prmA["beta"]), gB=vec(prmB["gamma"]), bB=vec(prmB["beta"]),
                mu=vec(prmA["mean"]), rs=vec(prmA["rstd"]), cA=vec(_coef(C2, 13).reshape(-1)), cB=vec(_coef(C, 14).reshape(-1)))
    for b in bufs.values():
        b.freeze()
    P = {k: b.ptr() for k, b in bufs.items()}
    full, blocked = Mat(S, ld).set(0, gb).freeze(), Mat(S, ld).set(0, gb)
    for r0, n, gbuf in [(0, S, full)] + [(r0, n, blocked) for r0, n in _blocks(S)]:
        _check(L.mcl_dense_bn1_dx_pair(_rows(bufs["dzA"], r0), P["WA"], C2, P["gA"], P["bA"], P["cA"], _rows(bufs["dzB"], r0),
                                       P["WB"], P["gB"], P["bB"], P["cB"], C, _rows(xb, r0), ld, n, P["mu"], P["rs"],
                                       _rows(gbuf, r0), ld, _st()), "mcl_dense_bn1_dx_pair")
    torch.cuda.synchronize()
    xb.unchanged("x")
    for k, b in bufs.items():
        b.unchanged(k)
    full.unchanged("gbuf", 0, C)
    _finite("gbuf", full, 0, C)
    _same_bits("mcl_dense_bn1_dx_pair", full, blocked)


def test_dx_window_walk_invariance(L):
    """mcl_dense_bn1_dx_window, window (32, 32) of C = 64, S = 98405 = 1537 * 64 + 37: one column tile, the S >= 50000 branch,
    gx = min(512, 1538) = 512, workgroups walk 3 or 4 tiles.  Only the window's columns of x, W1 and gbuf hold numbers."""
    S, C, c0, nc = 98405, 64, 32, 32
    _assert_walks(S, nc)
    assert _walk(S, nc)[0] == 512
    prm, x, W1, dz, gb = dr.head_case(S, C)
    xb = Mat(S, C).set(c0, x[:, c0:]).freeze()
    dzb, wb = Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(c0, W1[:, c0:]).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    cb = vec(_coef(C, 15).reshape(-1)).freeze()
    full, blocked = Mat(S, C).set(c0, gb[:, c0:]).freeze(), Mat(S, C).set(c0, gb[:, c0:])
    for r0, n, gbuf in [(0, S, full)] + [(r0, n, blocked) for r0, n in _blocks(S)]:
        _check(L.mcl_dense_bn1_dx_window(_rows(dzb, r0), wb.ptr(), C, c0, nc, _rows(xb, r0), C, n, *[p.ptr() for p in pv],
                                         cb.ptr(), _rows(gbuf, r0), C, _st()), "mcl_dense_bn1_dx_window")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1"), (cb, "coef")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    full.unchanged("gbuf", c0, nc)
    _finite("gbuf", full, c0, nc)
    _same_bits("mcl_dense_bn1_dx_window", full, blocked)


# ---------------------------------------------------------------------------------------------------- 2. sums at a walking shape
def test_dx_sums_walking_shape(L):
    """dgamma, dbeta and the pending mean terms of mcl_dense_bn1_dx_sums at C = 520, S = 29669 = 463 * 64 + 37 (5 column tiles,
    gx = min(ceil(768 / 5), 464) = 154: workgroups walk 3 or 4 tiles) against the float64 restatement with its own bounds."""
    S, C, ld = 29669, 520, 520
    _assert_walks(S, C)
    assert _walk(S, C)[0] == 154
    prm, x, W1, dz, gb = dr.head_case(S, C)
    xb, gbb = Mat(S, ld).set(0, x).freeze(), Mat(S, ld).set(0, gb).freeze()
    dzb, wb = Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(0, W1).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    ws = Mat(1, int(L.mcl_dense_bn1_bwd_workspace_floats(S, C)), "f32").freeze()
    prior = [dr.f32(np.full(C, 0.5)), dr.f32(np.full(C, -0.25))]
    dgb, dbb = vec(prior[0]).freeze(), vec(prior[1]).freeze()
    kprev = vec(_coef(C, 16).reshape(-1)).freeze()
    _check(L.mcl_dense_bn1_dx_sums(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], ws.ptr(), dgb.ptr(), dbb.ptr(),
                                   1, kprev.ptr(), 1, gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_sums")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    for b, n in ((gbb, C), (ws, ws.ld), (dgb, C), (dbb, C), (kprev, 2 * C)):
        b.unchanged("output", 0, n)
    _finite("gbuf", gbb, 0, C)
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    assert h.p.amb_share <= dr.AMB_CAP
    rep = []
    pg = h.param_grads()
    for nm, buf, pr in (("dgamma", dgb, prior[0]), ("dbeta", dbb, prior[1])):
        ref, e = pg[nm]
        _within(nm, buf.get()[0], pr + ref, e + dr.U * np.abs(pr + ref), rep)
    kref, ke = dr.head_kacc(h, prm["gamma"])
    _within("kacc", kprev.get()[0].reshape(C, 2), kref, ke, rep)
    print(f"bn1_dx_sums S={S} C={C}: " + ", ".join(rep))


# ---------------------------------------------------------------------------------------------------- 3. edges against fp64
EDGES = [(S, C) for S in (1, 64, 65) for C in (8, 136)]     # a lone partial tile, an exactly full one, a second tile of one row


@pytest.mark.parametrize("S,C", EDGES)
def test_edges_dx_and_sums(L, S, C):
    """mcl_dense_bn1_dx and mcl_dense_bn1_dx_sums (have_prev = 1) against the float64 restatement with its derived bounds."""
    ld = C + 24
    prm, x, W1, dz, gb = dr.head_case(S, C)
    h = dr.Head(dz, W1, x, *dr.bn(prm))
    assert h.p.amb_share <= dr.AMB_CAP
    z = np.zeros(C)
    xb = Mat(S, ld).set(0, x).freeze()
    dzb, wb = Mat(S, 128).set(0, dz).freeze(), Mat(128, C).set(0, W1).freeze()
    pv = [vec(prm[k]).freeze() for k in ("gamma", "beta", "mean", "rstd")]
    rep = []
    # dx with given means
    coef = dr.f32(np.stack([h.c1, h.c2], 1))
    cb, gbb = vec(coef.reshape(-1)).freeze(), Mat(S, ld).set(0, gb).freeze()
    _check(L.mcl_dense_bn1_dx(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], cb.ptr(), gbb.ptr(), ld, _st()),
           "mcl_dense_bn1_dx")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf", 0, C)
    cb.unchanged("coef")
    _within("dx: gbuf", gbb.get(0, C), *dr.gbuf_add(gb, *h.delta(coef[:, 0], coef[:, 1], z, z)), rep)
    # the single pass, subtracting given terms of a previous pass
    kin = _coef(C, 17 + S)
    kprev, gbb = vec(kin.reshape(-1)).freeze(), Mat(S, ld).set(0, gb).freeze()
    ws = Mat(1, int(L.mcl_dense_bn1_bwd_workspace_floats(S, C)), "f32").freeze()
    prior = [dr.f32(np.full(C, 0.5)), dr.f32(np.full(C, -0.25))]
    dgb, dbb = vec(prior[0]).freeze(), vec(prior[1]).freeze()
    _check(L.mcl_dense_bn1_dx_sums(dzb.ptr(), wb.ptr(), C, xb.ptr(), ld, S, *[p.ptr() for p in pv], ws.ptr(), dgb.ptr(), dbb.ptr(),
                                   1, kprev.ptr(), 1, gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_sums")
    torch.cuda.synchronize()
    for b, nm in [(xb, "x"), (dzb, "dz"), (wb, "W1")] + [(p, "bn operand") for p in pv]:
        b.unchanged(nm)
    for b, n in ((gbb, C), (ws, ws.ld), (dgb, C), (dbb, C), (kprev, 2 * C)):
        b.unchanged("output", 0, n)
    _within("sums: gbuf", gbb.get(0, C), *dr.gbuf_add(gb, *h.delta(kin[:, 0], kin[:, 1], z, z, premultiplied=True)), rep)
    pg = h.param_grads()
    for nm, buf, pr in (("dgamma", dgb, prior[0]), ("dbeta", dbb, prior[1])):
        ref, e = pg[nm]
        _within(f"sums: {nm}", buf.get()[0], pr + ref, e + dr.U * np.abs(pr + ref), rep)
    _within("sums: kacc", kprev.get()[0].reshape(C, 2), *dr.head_kacc(h, prm["gamma"]), rep)
    print(f"bn1 edges S={S} C={C}: " + ", ".join(rep))


@pytest.mark.parametrize("S,C", EDGES)
def test_edges_window_and_pair(L, S, C):
    """mcl_dense_bn1_dx_window and mcl_dense_bn1_dx_pair against the float64 restatement with its derived bounds."""
    C2 = C + 32
    ld = C2 + 24
    prmA, prmB, x, gb, dzA, dzB, W1A, W1B = dr.pair_case(S, C)
    hA = dr.Head(dzA, W1A, x, *dr.bn(prmA))
    hB = dr.Head(dzB, W1B, x[:, :C], *dr.bn(prmB))
    assert max(hA.p.amb_share, hB.p.amb_share) <= dr.AMB_CAP
    coefA, coefB = (dr.f32(np.stack([h.c1, h.c2], 1)) for h in (hA, hB))
    xb, gbb = Mat(S, ld).set(0, x).freeze(), Mat(S, ld).set(0, gb).freeze()
    bufs = dict(dzA=Mat(S, 128).set(0, dzA), dzB=Mat(S, 128).set(0, dzB), WA=Mat(128, C2).set(0, W1A), WB=Mat(128, C).set(0, W1B),
                gA=vec(prmA["gamma"]), bA=vec(prmA["beta"]), gB=vec(prmB["gamma"]), bB=vec(prmB["beta"]),
                mu=vec(prmA["mean"]), rs=vec(prmA["rstd"]), cA=vec(coefA.reshape(-1)), cB=vec(coefB.reshape(-1)))
    for b in bufs.values():
        b.freeze()
    P = {k: b.ptr() for k, b in bufs.items()}
    _check(L.mcl_dense_bn1_dx_window(P["dzA"], P["WA"], C2, C, 32, xb.ptr(), ld, S, P["gA"], P["bA"], P["mu"], P["rs"], P["cA"],
                                     gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_window")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf (window)", C, 32)
    rep = []
    z = np.zeros(C2)
    dA = hA.delta(coefA[:, 0], coefA[:, 1], z, z)
    _within("window", gbb.get(C, 32), *dr.gbuf_add(gb[:, C:], dA[0][:, C:], dA[1][:, C:]), rep)
    gbb.freeze()
    _check(L.mcl_dense_bn1_dx_pair(P["dzA"], P["WA"], C2, P["gA"], P["bA"], P["cA"], P["dzB"], P["WB"], P["gB"], P["bB"], P["cB"],
                                   C, xb.ptr(), ld, S, P["mu"], P["rs"], gbb.ptr(), ld, _st()), "mcl_dense_bn1_dx_pair")
    torch.cuda.synchronize()
    gbb.unchanged("gbuf (pair)", 0, C)
    xb.unchanged("x")
    for k, b in bufs.items():
        b.unchanged(k)
    _within("pair", gbb.get(0, C), *dr.gbuf_add(gb[:, :C], *dr.pair_delta(hA, coefA[:C], hB, coefB, C)), rep)
    print(f"bn1 edges window + pair S={S} C={C}: " + ", ".join(rep))
