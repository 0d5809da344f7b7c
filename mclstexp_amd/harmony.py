"""Harmony batch correction on the MI355X: the step of BLEEP's protocol between HVG selection and training.

Reference: baselines/Bleep/preprocess.ipynb of the reference, last code cell -- the four slides' ``hvg_matrix.npy`` are
concatenated, ``harmonypy.run_harmony(d, meta_data=df, vars_use=["dataset"])`` corrects them, and ``harmony_matrix.npy`` is
written per slide; BLEEP trains on, retrieves from and is scored against those files.

harmonypy is not installed where this was written, so parity with one of its releases is not pinned; what is pinned is the
arithmetic DESIGN 6.9 states (and ``tests/harmony_reference.py`` restates in numpy): soft k-means on unit rows with the
diversity penalty, blockwise update of R, ridge correction per cluster, harmonypy's two convergence tests.  Things to know:

* ``theta`` defaults to 2 (the Harmony paper and the R package); some harmonypy releases default to 1: ``theta`` is the knob
  for matching a given release.
* The first normalisation divides every cell by its own maximum before the L2 norm, as harmonypy does: a cell whose maximum
  is 0 becomes NaN (and poisons the run, as there), a negative maximum flips the cell's sign, a NaN in a cell makes the
  whole cell NaN (``numpy.max`` propagates it).
* harmonypy seeds Y with sklearn's ``KMeans(init="k-means++", n_init=10, max_iter=25)``.  That is not reproduced: pass its
  centroids as ``init_centroids``, or a hard Lloyd k-means runs on the device (argmax of Zc Y^T, means, an emptied cluster
  keeps its centroid, 25 iterations) from ``seed_rows`` or K distinct rows drawn from ``RandomState(random_state)``.
* The block permutations are drawn on the host from ``np.random.RandomState(random_state)`` -- the legacy stream harmonypy's
  ``np.random.seed`` + ``np.random.shuffle`` uses -- and uploaded as int32; ``update_orders`` replays given ones.
* One batch variable only.  K <= 128, at most 31 batches, N K < 2^31.
* The host reads three doubles (the objective's terms) once per k-means iteration to decide the convergence tests; that
  synchronisation is accepted.

Everything on the device is fp64, atomics-free and bit-reproducible run to run.  No CPU fallback.

    python -m mclstexp_amd.harmony --matrices 1/hvg_matrix.npy 2/hvg_matrix.npy ... --out_dir D [--theta T] [...]
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._arrays import FLOAT_CODE, ArrayLike, Tensor, device, empty, load_gene_major, matrix, upload
from ._lib import call

MAX_K, MAX_B = 128, 31
LLOYD_ITERS = 25                       # harmonypy's max_iter of its k-means initialisation
OUT_FILE = "harmony_matrix.npy"


@dataclass
class HarmonyResult:
    Z_corr: Tensor                     # (N, d) fp64, device
    R: Tensor                          # (N, K) fp64, device
    Y: Tensor                          # (K, d) fp64, device
    objective_kmeans: List[float]
    objective_harmony: List[float]
    kmeans_rounds: List[int]
    converged: bool


# ------------------------------------------------------------------------------------------------------- host rules
def default_nclust(N: int) -> int:
    """harmonypy's ``np.min([np.round(N / 30.0), 100]).astype(int)`` (round half to even)."""
    return int(min(np.round(N / 30.0), 100))


def n_blocks(block_size: float) -> int:
    return int(math.ceil(1.0 / block_size))


def block_bounds(N: int, nb: int) -> np.ndarray:
    """The nb + 1 boundaries of ``np.array_split(np.arange(N), nb)``: the first N mod nb blocks hold one more cell."""
    base, extra = divmod(N, nb)
    sizes = np.full(nb, base, dtype=np.int64)
    sizes[:extra] += 1
    return np.concatenate([[0], np.cumsum(sizes)])


def draw_order(rng: np.random.RandomState, N: int) -> np.ndarray:
    """One ``np.random.shuffle(np.arange(N))`` of the legacy stream, as int32."""
    order = np.arange(N)
    rng.shuffle(order)
    return order.astype(np.int32)


def encode_batch(batch: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """Labels -> (int32 codes, the sorted unique labels): the column order of ``pd.get_dummies``."""
    b = np.asarray(batch)
    if b.ndim != 1 or b.size == 0:
        raise ValueError(f"batch must be a non-empty 1-D sequence of labels, got shape {b.shape}")
    levels, codes = np.unique(b, return_inverse=True)
    return codes.astype(np.int32).reshape(-1), levels


def orient(data: ArrayLike, N: int) -> ArrayLike:
    """harmonypy's rule: ``data`` is cells x features; when only its second axis has N entries it is transposed."""
    if len(data.shape) != 2:
        raise ValueError(f"data: expected a 2-D array, got shape {tuple(data.shape)}")
    if data.shape[0] == N:
        return data
    if data.shape[1] == N:
        return data.T
    raise ValueError(f"data {tuple(data.shape)} has no axis of {N} cells (the length of batch)")


def _per_batch(v: Union[float, Sequence[float]], B: int, name: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,):
        raise ValueError(f"{name}: a number or one value per batch ({B}), got shape {a.shape}")
    return a.copy()


def converged_kmeans(obj: Sequence[float], eps: float) -> bool:
    """harmonypy's check_convergence(0): windows of three over the last four k-means objectives."""
    old = new = 0.0
    for i in range(3):
        old += obj[-2 - i]
        new += obj[-1 - i]
    return abs(old - new) / abs(old) < eps


def converged_harmony(obj: Sequence[float], eps: float) -> bool:
    """harmonypy's check_convergence(1): no absolute value on the numerator."""
    return (obj[-2] - obj[-1]) / abs(obj[-2]) < eps


def _check_orders(update_orders, N: int) -> Optional[List[np.ndarray]]:
    if update_orders is None:
        return None
    out = []
    for i, o in enumerate(update_orders):
        o = np.asarray(o)
        if o.shape != (N,) or not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f"update_orders[{i}]: expected {N} integers, got shape {o.shape} of {o.dtype}")
        if not np.array_equal(np.sort(o), np.arange(N)):
            raise ValueError(f"update_orders[{i}] is not a permutation of 0 .. {N - 1}")
        out.append(o.astype(np.int32))
    return out


# ----------------------------------------------------------------------------------------------------------- device
class _Device:
    """The buffers of one run and one method per entry point (each a thin call: no arithmetic on the host)."""

    def __init__(self, N: int, K: int, d: int, B: int, dev: torch.device):
        self.N, self.K, self.d, self.B, self.dev = N, K, d, B, dev
        self.lib = _lib.lib()            # (tests/test_harmony_gpu.py calls single entry points through it)
        e = empty(dev)
        f8 = torch.float64
        self.work = e((max(int(call("mcl_harmony_workspace_doubles", N, K, d, B)), 8),), f8)
        self.D, self.S, self.R = e((N, K), f8), e((N, K), f8), e((N, K), f8)
        self.Y = e((K, d), f8)
        self.E, self.O = e((K, B), f8), e((K, B), f8)
        self.obj = e((3,), f8)

    def normalize(self, z: Tensor, by_max: bool, z64: Optional[Tensor], zc: Tensor) -> None:
        call("mcl_harmony_normalize", z, z.stride(0), FLOAT_CODE[z.dtype], self.N, self.d, by_max, z64, zc)

    def centroids(self, zc: Tensor) -> None:
        call("mcl_harmony_centroids", self.R, zc, None, self.N, self.K, self.d, 0, 1, self.work, self.Y)

    def moe_sums(self, z: Tensor, batch: Tensor, out: Tensor) -> None:
        call("mcl_harmony_centroids", self.R, z, batch, self.N, self.K, self.d, self.B, 0, self.work, out)

    def dist(self, zc: Tensor) -> None:
        call("mcl_harmony_dist", zc, self.Y, self.N, self.K, self.d, 0, self.D)

    def softmax(self, sigma: float, normalize: bool, out: Tensor) -> None:
        call("mcl_harmony_softmax", self.D, self.N, self.K, sigma, normalize, out)

    def moments(self, batch: Tensor, pr: Tensor) -> None:
        call("mcl_harmony_moments", self.R, batch, self.N, self.K, self.B, pr, self.E, self.O)

    def update_blocks(self, batch: Tensor, order: Tensor, nb: int, theta: Tensor, pr: Tensor) -> None:
        call("mcl_harmony_update_block", self.R, self.S, batch, order,
             self.N, self.K, self.B, nb, 0, nb, theta, pr, self.E, self.O)

    def objective(self, batch: Tensor, theta: Tensor, sigma: float) -> float:
        call("mcl_harmony_objective", self.R, self.D, batch, self.E, self.O,
             theta, self.N, self.K, self.B, sigma, self.work, self.obj)
        t = self.obj.cpu().numpy()                      # the one synchronisation per k-means iteration
        return float(t[0] + t[1] + t[2])

    def ridge(self, M: Tensor, lamb: Tensor, W: Tensor) -> None:
        call("mcl_harmony_ridge", self.O, M, lamb, self.K, self.B, self.d, W)

    def apply(self, z: Tensor, W: Tensor, batch: Tensor, out: Tensor) -> None:
        call("mcl_harmony_apply", z, self.R, W, batch, self.N, self.K, self.B, self.d, out)

    def lloyd(self, zc: Tensor, seeds: Tensor) -> None:
        e = empty(self.dev)
        labels, sums = e((self.N,), torch.int32), e((self.K, self.d), torch.float64)
        call("mcl_harmony_lloyd", zc, self.N, self.K, self.d, seeds, LLOYD_ITERS, labels, self.D, sums, self.work, self.Y)


def run_harmony(data: ArrayLike, batch: Sequence, *, theta: Union[float, Sequence[float]] = 2.0,
                lamb: Union[float, Sequence[float]] = 1.0, sigma: float = 0.1, nclust: Optional[int] = None,
                tau: float = 0, block_size: float = 0.05, max_iter_harmony: int = 10, max_iter_kmeans: int = 20,
                epsilon_cluster: float = 1e-5, epsilon_harmony: float = 1e-4, random_state: int = 0,
                init_centroids: Optional[ArrayLike] = None, seed_rows: Optional[Sequence[int]] = None,
                update_orders: Optional[Sequence[Sequence[int]]] = None) -> HarmonyResult:
    """Harmony on (N, d) ``data`` (fp32 / fp64, host or device; (d, N) is transposed when only that fits) with one batch
    label per cell (any labels, encoded by sorted unique value; cells need not be sorted by batch).  See the module
    docstring for the parameters that differ from harmonypy's and DESIGN 6.9 for the arithmetic."""
    codes, levels = encode_batch(batch)
    N, B = int(codes.size), int(levels.size)
    data = orient(data, N)
    d = int(data.shape[1])
    K = default_nclust(N) if nclust is None else int(nclust)
    if K < 1:
        raise ValueError(f"nclust must be >= 1, got {K} (N = {N})")
    if K > N:
        raise ValueError(f"nclust = {K} exceeds the number of cells ({N})")
    if not 0.0 < block_size <= 1.0:
        raise ValueError(f"block_size must be in (0, 1], got {block_size}")
    if max_iter_kmeans < 1 or max_iter_harmony < 0:
        raise ValueError("max_iter_kmeans must be >= 1 and max_iter_harmony >= 0")
    if not sigma > 0:
        raise ValueError(f"sigma must be > 0, got {sigma}")
    nb = n_blocks(block_size)
    if nb > N:
        raise ValueError(f"block_size {block_size} cuts {N} cells into {nb} blocks: some would be empty")
    counts = np.bincount(codes, minlength=B)
    th, lm = _per_batch(theta, B, "theta"), _per_batch(lamb, B, "lamb")
    if (counts == 0).any():
        raise ValueError(f"batch {int(np.argmin(counts))} has 0 cells")
    if tau > 0:
        th = th * (1.0 - np.exp(-(counts / (K * tau)) ** 2))
    orders = _check_orders(update_orders, N)
    if init_centroids is not None and tuple(init_centroids.shape) != (K, d):
        raise ValueError(f"init_centroids: expected ({K}, {d}), got {tuple(init_centroids.shape)}")
    if seed_rows is not None:
        sr = np.asarray(seed_rows)
        if sr.shape != (K,) or not np.issubdtype(sr.dtype, np.integer) or sr.min() < 0 or sr.max() >= N \
                or np.unique(sr).size != K:
            raise ValueError(f"seed_rows: expected {K} distinct rows in [0, {N})")
    dev = device("harmony")
    if K > MAX_K or B > MAX_B or N * K >= 2 ** 31:
        raise RuntimeError(f"mclstexp_amd.harmony: K = {K} (<= {MAX_K}), {B} batches (<= {MAX_B}) or N K = {N * K} "
                           "(< 2^31) is beyond the kernels' limits")
    rng = np.random.RandomState(random_state)

    z_in = matrix(data, "data", dev, FLOAT_CODE, torch.float64)
    e = empty(dev)
    f8 = torch.float64
    g = _Device(N, K, d, B, dev)
    z_orig, zc, z_corr = e((N, d), f8), e((N, d), f8), e((N, d), f8)
    batch_d = upload(codes, dev)
    theta_d, lamb_d, pr_d = upload(th, dev), upload(lm, dev), upload(counts / float(N), dev)
    g.normalize(z_in, True, z_orig, zc)

    # 1. initialisation
    if init_centroids is not None:
        y0 = matrix(init_centroids, "init_centroids", dev, (torch.float64,), torch.float64, dense=True)
        call("mcl_harmony_normalize", y0, d, 1, K, d, 0, None, g.Y)
    else:
        rows = np.asarray(seed_rows) if seed_rows is not None else rng.choice(N, K, replace=False)
        g.lloyd(zc, upload(rows.astype(np.int32), dev))
    g.dist(zc)
    g.softmax(sigma, True, g.R)
    g.moments(batch_d, pr_d)
    obj_k: List[float] = [g.objective(batch_d, theta_d, sigma)]
    obj_h: List[float] = [obj_k[0]]
    rounds: List[int] = []
    converged = False
    M, W = e((K, B + 1, d), f8), e((K, B + 1, d), f8)
    n_order = 0
    for _ in range(max_iter_harmony):
        # 2. clustering round
        i = 0
        for i in range(max_iter_kmeans):
            g.centroids(zc)
            g.dist(zc)
            g.softmax(sigma, False, g.S)
            if orders is None:
                order = draw_order(rng, N)
            else:
                if n_order >= len(orders):
                    raise ValueError(f"update_orders holds {len(orders)} permutations; the run needs more")
                order = orders[n_order]
            n_order += 1
            g.update_blocks(batch_d, upload(order, dev), nb, theta_d, pr_d)
            obj_k.append(g.objective(batch_d, theta_d, sigma))
            if i > 3 and converged_kmeans(obj_k, epsilon_cluster):
                break
        rounds.append(i)
        obj_h.append(obj_k[-1])
        # 3. correction
        g.moe_sums(z_orig, batch_d, M)
        g.ridge(M, lamb_d, W)
        g.apply(z_orig, W, batch_d, z_corr)
        g.normalize(z_corr, False, None, zc)
        # 4. stopping
        if converged_harmony(obj_h, epsilon_harmony):
            converged = True
            break
    if max_iter_harmony == 0:
        z_corr.copy_(z_orig)
    if orders is not None and n_order != len(orders):
        raise ValueError(f"update_orders holds {len(orders)} permutations; the run used {n_order}")
    return HarmonyResult(z_corr, g.R, g.Y, obj_k, obj_h, rounds, converged)


def correct_slides(matrices: Sequence[ArrayLike], layout: str = "genes_by_cells", return_result: bool = False, **params):
    """The notebook cell: the slides' matrices concatenated, Harmony with the slide index as the batch, the result split
    back per slide.  ``layout="genes_by_cells"`` (the layout of ``hvg_matrix.npy``: (genes, cells) in and out) or
    ``"cells_by_genes"``.  Returns numpy float64 matrices in the given layout; with ``return_result`` also the
    ``HarmonyResult`` of the run."""
    if layout not in ("genes_by_cells", "cells_by_genes"):
        raise ValueError(f"layout must be 'genes_by_cells' or 'cells_by_genes', got {layout!r}")
    if not matrices:
        raise ValueError("need at least one slide")
    mats = [np.asarray(m) for m in matrices]
    for i, m in enumerate(mats):
        if m.ndim != 2:
            raise ValueError(f"slide {i}: expected a 2-D matrix, got shape {m.shape}")
        if 0 in m.shape:
            raise ValueError(f"batch {i} has 0 cells (slide {i} is {m.shape})")
    if layout == "genes_by_cells":
        mats = [m.T for m in mats]
    for i, m in enumerate(mats):
        if m.shape[1] != mats[0].shape[1]:
            raise ValueError(f"slide {i} has {m.shape[1]} genes, slide 0 has {mats[0].shape[1]}")
    dtype = np.float32 if all(m.dtype == np.float32 for m in mats) else np.float64
    data = np.concatenate([m.astype(dtype, copy=False) for m in mats], axis=0)
    # the notebook's labels are "0.0", "1.0", ...; their sorted order is the slide order for up to 10 slides, which the
    # integer index reproduces for any number
    batch = np.concatenate([np.full(m.shape[0], i, dtype=np.int64) for i, m in enumerate(mats)])
    res = run_harmony(data, batch, **params)
    out = res.Z_corr.cpu().numpy()
    bounds = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])])
    parts = [out[bounds[i]:bounds[i + 1]] for i in range(len(mats))]
    parts = [np.ascontiguousarray(p.T) if layout == "genes_by_cells" else p for p in parts]
    return (parts, res) if return_result else parts


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.harmony",
                                description="Harmony batch correction of per-slide hvg_matrix.npy files "
                                            "(BLEEP's preprocess.ipynb, last cell)")
    p.add_argument("--matrices", required=True, nargs="+", help="one (genes, cells) .npy per slide, in slide order")
    p.add_argument("--out_dir", required=True, help=f"writes OUT_DIR/<slide number from 1>/{OUT_FILE}, (genes, cells)")
    p.add_argument("--theta", type=float, default=2.0)
    p.add_argument("--lamb", type=float, default=1.0)
    p.add_argument("--sigma", type=float, default=0.1)
    p.add_argument("--nclust", type=int, default=None)
    p.add_argument("--tau", type=float, default=0.0)
    p.add_argument("--block_size", type=float, default=0.05)
    p.add_argument("--max_iter_harmony", type=int, default=10)
    p.add_argument("--max_iter_kmeans", type=int, default=20)
    p.add_argument("--epsilon_cluster", type=float, default=1e-5)
    p.add_argument("--epsilon_harmony", type=float, default=1e-4)
    p.add_argument("--random_state", type=int, default=0)
    return p.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    mats = [m.T for m in load_gene_major(a.matrices)]            # back to (genes, cells); load_gene_major checks G
    params = {k: getattr(a, k) for k in ("theta", "lamb", "sigma", "nclust", "tau", "block_size", "max_iter_harmony",
                                         "max_iter_kmeans", "epsilon_cluster", "epsilon_harmony", "random_state")}
    out, res = correct_slides(mats, "genes_by_cells", return_result=True, **params)
    for i, (m, o) in enumerate(zip(mats, out)):
        path = os.path.join(a.out_dir, str(i + 1))
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, OUT_FILE), o)
        print(f"slide {i + 1}: {tuple(m.shape)} -> {os.path.join(path, OUT_FILE)} {tuple(o.shape)}")
    for r, (it, obj) in enumerate(zip(res.kmeans_rounds, res.objective_harmony[1:])):
        print(f"round {r + 1}: {it + 1} k-means iterations, objective {obj:.10g}")
    print(f"converged: {res.converged}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
