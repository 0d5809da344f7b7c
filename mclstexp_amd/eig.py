"""The leading eigenpairs of symmetric matrices on the MI355X (csrc/eig.hip): a batched, deterministic fp64
solver for the k <= 64 largest eigenvalues and their eigenvectors of dense symmetric matrices of order <= 4096.

The method is direct (LAPACK ``dsyevx``-shaped): Householder tridiagonalisation, bisection on the Sturm count, block
inverse iteration, back-transformation.  It has no convergence parameter; the schedule is a fixed sequence of about 3 m
launches on the current stream.  All slides of a call run through the same launches; a slide inside a batch is
bit-identical to the same slide alone, and a run is bit-reproducible.  The only synchronisation is reading the
certificate back (S x 2 doubles).  No CPU fallback: without a GPU / the HIP library ``eigh_top`` raises ``RuntimeError``.

``cluster.pca_device(..., solver="device")`` feeds the Gram matrices of the PCA straight into ``solve`` below.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._arrays import ArrayLike, Tensor, cumulative_offsets, device, empty, upload
from ._lib import call

MAX_M = 4096         # order of a matrix (csrc/eig.hip: a column of Z sits in LDS)
MAX_K = 64           # eigenpairs per matrix
MAX_SLIDES = 65535   # grid.y
EPS = 2.0 ** -52
GUARD = 64.0         # the certificate may reach GUARD * m * eps: a guard against garbage, not a tuning knob
ALL_STAGES = 7


def check_sizes(sizes: Sequence[int], k: int) -> np.ndarray:
    """The limits of the solver, checked on the host: 1 <= m_s <= 4096, 1 <= k <= min(64, every m_s), S <= 65535."""
    m = np.asarray(sizes)
    if m.ndim != 1 or m.size < 1 or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"sizes must be a 1-D integer array of S >= 1 orders, got {sizes!r}")
    if m.size > MAX_SLIDES:
        raise ValueError(f"at most {MAX_SLIDES} matrices per call, got {m.size}")
    if (m < 1).any() or (m > MAX_M).any():
        raise ValueError(f"every matrix needs an order in 1 .. {MAX_M}; orders {m.tolist()}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an int, got {k!r}")
    if k < 1 or k > min(MAX_K, int(m.min())):
        raise ValueError(f"k must lie in 1 .. min({MAX_K}, smallest order = {int(m.min())}), got {k}")
    return m.astype(np.int32)


def solve(a: Tensor, a_offsets: np.ndarray, sizes: np.ndarray, k: int, evec_offsets: Optional[np.ndarray] = None,
          a_offsets_d: Optional[Tensor] = None) -> Dict[str, object]:
    """Enqueue the whole solve on the flat fp64 device buffer ``a`` (slide s: row-major m_s x m_s at ``a_offsets[s]``,
    OVERWRITTEN) and return device ``values`` (S, k), ``vectors_flat`` (row-major (m_s, k) at ``evec_offsets[s]``),
    ``evec_offsets`` (device), ``certificate`` (S, 2) -- nothing is read back here."""
    dev = a.device
    m = check_sizes(sizes, k)
    S, max_m, sum_m = int(m.size), int(m.max()), int(m.sum())
    eoff = cumulative_offsets(m.astype(np.int64) * k) if evec_offsets is None else evec_offsets
    e = empty(dev)
    values, cert = e((S, k), torch.float64), e((S, 2), torch.float64)
    vectors = e((int(eoff[-1]),), torch.float64)
    work = e((int(call("mcl_sym_eig_workspace_bytes", S, max_m, sum_m, k)) // 8 + 1,), torch.float64)
    aoff_d = upload(a_offsets, dev) if a_offsets_d is None else a_offsets_d
    eoff_d, m_d = upload(eoff, dev), upload(m, dev)
    call("mcl_sym_eig_top", a, aoff_d, m_d, S, max_m, sum_m, k, ALL_STAGES, values, vectors, eoff_d, cert, work)
    return {"values": values, "vectors_flat": vectors, "evec_offsets": eoff_d, "evec_offsets_host": eoff,
            "certificate": cert, "sizes": m}


def check_certificate(cert: np.ndarray, sizes: np.ndarray) -> None:
    """Raise ``RuntimeError`` naming the first slide whose certificate exceeds 64 m eps (or is not finite)."""
    bound = GUARD * sizes.astype(np.float64) * EPS
    bad = ~(cert <= bound[:, None]).all(axis=1)
    if bad.any():
        s = int(np.flatnonzero(bad)[0])
        raise RuntimeError(f"eigh_top: slide {s} (order {int(sizes[s])}) failed its certificate: residual / |T| = "
                           f"{cert[s, 0]:.3e}, max |Z^T Z - I| = {cert[s, 1]:.3e}, allowed {bound[s]:.3e}")


def _one_matrix(a: ArrayLike) -> Tensor:
    t = a if isinstance(a, Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"a: expected one square matrix, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        if t.is_cuda:
            raise ValueError(f"a: device matrices must be float32 or float64, got {t.dtype}")
        t = t.to(torch.float64)
    return t


def eigh_top(a: ArrayLike, k: int, sizes: Optional[Sequence[int]] = None, overwrite: bool = False) -> Dict[str, object]:
    """The k largest eigenvalues (descending) and their eigenvectors.

    ``a``: one symmetric matrix (host or device, fp32 / fp64), or -- with ``sizes`` -- a flat fp64 device buffer that
    holds the row-major m_s x m_s matrices one after the other.  The input is copied unless ``overwrite=True`` (a flat fp64
    device buffer, or one contiguous fp64 device matrix, is then destroyed).  Returns device ``values`` (S, k), ``vectors``
    (one (m_s, k) view per slide; every vector's component of largest magnitude is positive) and the host ``certificate``
    (S, 2): max_i |T z_i - lambda_i z_i| / |T| and max |Z^T Z - I| of the tridiagonal problem, computed on the device.
    Raises ``ValueError`` for arguments outside the solver's limits before the GPU is touched, and ``RuntimeError`` naming
    the slide if a certificate value exceeds 64 m eps."""
    if sizes is None:
        t = _one_matrix(a)
        m = check_sizes([int(t.shape[0])], k)
        if not t.is_cuda and not torch.equal(t, t.T):
            raise ValueError("a: the matrix is not symmetric (a host matrix is checked; a device matrix is taken as given)")
        dev = device("eig")
        if t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and overwrite:
            flat = t.view(-1)
        else:
            flat = torch.empty((t.numel(),), device=dev, dtype=torch.float64)
            flat.view(tuple(t.shape)).copy_(t if t.is_cuda else t.to(torch.float64))
    else:
        m = check_sizes(sizes, k)
        if not isinstance(a, Tensor) or a.dim() != 1:
            raise ValueError("a: with sizes, expected a flat 1-D device buffer of the matrices one after the other")
        need = int((m.astype(np.int64) ** 2).sum())
        if a.numel() != need:
            raise ValueError(f"a: sizes {m.tolist()} need {need} elements, the buffer holds {a.numel()}")
        if a.dtype != torch.float64:
            raise ValueError(f"a: a flat buffer must be float64, got {a.dtype}")
        if not a.is_cuda:
            raise ValueError("a: a flat buffer must be a device tensor")
        dev = device("eig")
        if overwrite and a.is_contiguous():
            flat = a
        else:
            flat = torch.empty((need,), device=dev, dtype=torch.float64)
            flat.copy_(a)
    aoff = cumulative_offsets(m.astype(np.int64) ** 2)
    res = solve(flat, aoff, m, int(k))
    cert = res["certificate"].cpu().numpy()             # the one synchronisation
    check_certificate(cert, m)
    eoff = res["evec_offsets_host"]
    vecs = [res["vectors_flat"][int(eoff[s]):int(eoff[s + 1])].view(int(m[s]), int(k)) for s in range(m.size)]
    return {"values": res["values"], "vectors": vecs, "certificate": cert}
