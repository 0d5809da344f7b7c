"""The spot neighbourhood graph on the MI355X: what ``sc.pp.neighbors`` leaves in ``obsp["distances"]`` and
``obsp["connectivities"]`` for UMAP and Leiden -- the step of BLEEP's ``visualize_umap_clusters``
(baselines/Bleep/BLEEP_inference.ipynb: ``sc.pp.pca(n_comps=50)``, ``sc.pp.neighbors(n_neighbors=150, n_pcs=50)``) that
follows the PCA -- for all slides of an evaluation per call.

What is computed is stated in DESIGN 6.11 and restated in numpy by ``tests/neighbors_reference.py``: the exact k nearest
rows of every row under the Euclidean distance (``n_neighbors`` counts the row itself, as in scanpy), umap-learn's
``smooth_knn_dist`` (rho, sigma) and ``compute_membership_strengths`` with the fuzzy union, as one CSR per segment (slide)
of the row-stacked input.  Things to know:

* Exact at every size: scanpy switches to approximate NN-descent from 4096 observations up; this module never does.
  2 <= n_neighbors <= 256, n_neighbors <= n_s, 2 <= n_s <= 16384 rows per segment, D <= 64.
* Distances are direct sums of squared differences in fp64 (sklearn's brute force uses the Gram form; umap-learn holds
  float32).  Ties in the distance, duplicates included, go to the smaller row index.
* The host reads one integer per segment, the number of stored connectivities, between the two phases of
  ``mcl_knn_connectivities``; nothing else leaves the device.
* The UMAP layout of the graph is ``mclstexp_amd.umap``, its Leiden clustering ``mclstexp_amd.leiden``; ``to_scipy`` hands
  the two matrices to any other consumer.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible run to run; a slide inside a batch
is bit-identical to the same slide alone.  No CPU fallback.

    python -m mclstexp_amd.neighbors --pred P1.npy ... [--raw] [--n_neighbors 150] [--n_pcs 50] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _arrays, cluster
from . import preprocess as _pre       # expression_graph has an argument of the module's name
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_columns, cumulative_offsets, dense, device, empty, matrix,
                      upload)
from ._lib import call

MAX_DIM = 64             # csrc/neighbors.hip
MAX_ROWS = 16384         # per segment: one row of distances lives in LDS
MAX_NEIGHBORS = 256
MAX_SEGMENTS = 65535
N_NEIGHBORS = 150        # BLEEP_inference.ipynb visualize_umap_clusters
N_PCS = 50
N_TOP_GENES = 1024
OUT_FILE = "neighbors.npz"


# ------------------------------------------------------------------------------------------------------- host rules
def validate_offsets(offsets: Optional[Sequence[int]], rows: int, n_neighbors: int) -> np.ndarray:
    """offsets[0] = 0, offsets[-1] = rows, every segment holds 2 .. 16384 rows and at least ``n_neighbors`` of them."""
    k = validate_neighbors(n_neighbors)
    off = _arrays.validate_offsets(offsets, rows, 2, MAX_ROWS, max_segments=MAX_SEGMENTS, none_is_one=True)
    seg = np.diff(off)
    if (seg < k).any():
        raise ValueError(f"n_neighbors = {k} counts the row itself and needs at least {k} rows in every segment; "
                         f"segment sizes {seg.tolist()}")
    return off


def validate_neighbors(n_neighbors: int) -> int:
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)):
        raise ValueError(f"n_neighbors must be an integer, got {n_neighbors!r}")
    if n_neighbors < 2 or n_neighbors > MAX_NEIGHBORS:
        raise ValueError(f"n_neighbors must lie in 2 .. {MAX_NEIGHBORS}, got {n_neighbors}")
    return int(n_neighbors)


def _check_x(x: ArrayLike, offsets, n_neighbors: int) -> np.ndarray:
    rows, _ = check_columns(x, MAX_DIM)
    return validate_offsets(offsets, rows, n_neighbors)


# ----------------------------------------------------------------------------------------------------------- device
class _Plan:
    """The offsets of one call on the device, the scalars the entry points are sized by, and the workspace."""

    def __init__(self, off: np.ndarray, k: int, dev: torch.device):
        seg = np.diff(off)
        self.off, self.seg, self.k, self.dev = off, seg, int(k), dev
        self.S, self.rows = int(seg.size), int(off[-1])
        self.min_n, self.max_n = int(seg.min()), int(seg.max())
        self.off_d = upload(off, dev)
        self.work = empty(dev)((max(int(call("mcl_knn_workspace_bytes", self.rows, self.k)), 8) // 8 + 1,), torch.float64)

    def _sizes(self):
        return self.S, self.rows, self.min_n, self.max_n, self.k

    def knn(self, xd: Tensor, idx: Tensor, dist: Tensor) -> None:
        call("mcl_knn_exact", xd, xd.stride(0), FLOAT_CODE[xd.dtype], int(xd.shape[1]), self.off_d, *self._sizes(), idx, dist)

    def smooth(self, dist: Tensor, rho: Tensor, sigma: Tensor) -> None:
        call("mcl_knn_smooth", dist, self.off_d, *self._sizes(), self.work, rho, sigma)

    def connectivities(self, idx: Tensor, dist: Tensor, rho: Tensor, sigma: Tensor, mix: float):
        """(indptr, indices, data, nnz_offsets): the count, the one read of S integers, the fill."""
        e = empty(self.dev)
        indptr, nnz = e((self.rows + self.S,), torch.int64), e((self.S,), torch.int64)

        def phase(which, nnz_off, total, indices, data):
            call("mcl_knn_connectivities", idx, dist, rho, sigma, self.off_d, *self._sizes(),
                 float(mix), which, self.work, indptr, nnz, nnz_off, total, indices, data)
        phase(0, None, 0, None, None)
        counts = nnz.cpu().numpy()                     # the one synchronisation
        if (counts < 0).any():
            raise RuntimeError("mcl_knn_connectivities skipped a segment: the offsets on the device do not match the host's")
        nnz_off = cumulative_offsets(counts)
        total = int(nnz_off[-1])
        indices, data = e((max(total, 1),), torch.int32), e((max(total, 1),), torch.float64)
        nnz_off_d = upload(nnz_off, self.dev)
        phase(1, nnz_off_d, total, indices, data)
        return indptr, indices[:total], data[:total], nnz_off


def knn(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_neighbors: int = 15) -> Tuple[Tensor, Tensor]:
    """The exact ``n_neighbors`` nearest rows of every row inside its segment of the row-stacked (rows, D <= 64) matrix
    ``x`` (fp32 / fp64, host or device, a row stride allowed): device ``(indices, distances)``, (rows, n_neighbors) int32
    (segment-local) and fp64.  Position 0 is the row itself at distance 0; the others ascend in (distance, index)."""
    off = _check_x(x, offsets, n_neighbors)
    dev = device("neighbors")
    plan = _Plan(off, n_neighbors, dev)
    xd = matrix(x, "x", dev, FLOAT_CODE, torch.float64)
    e = empty(dev)
    idx, dist = e((plan.rows, plan.k), torch.int32), e((plan.rows, plan.k), torch.float64)
    plan.knn(xd, idx, dist)
    return idx, dist


def smooth(knn_distances: ArrayLike, offsets: Optional[Sequence[int]] = None) -> Tuple[Tensor, Tensor]:
    """umap-learn's ``smooth_knn_dist`` of given (rows, k) neighbour distances: device ``(rho, sigma)``, (rows,) fp64."""
    rows, k = _list_shape(knn_distances, "knn_distances")
    off = validate_offsets(offsets, rows, k)
    dev = device("neighbors")
    plan = _Plan(off, k, dev)
    dist = dense(knn_distances, "knn_distances", (rows, k), torch.float64, dev)
    e = empty(dev)
    rho, sigma = e((rows,), torch.float64), e((rows,), torch.float64)
    plan.smooth(dist, rho, sigma)
    return rho, sigma


def connectivities(knn_indices: ArrayLike, knn_distances: ArrayLike, rho: ArrayLike, sigma: ArrayLike,
                   offsets: Optional[Sequence[int]] = None, set_op_mix_ratio: float = 1.0) -> Dict[str, object]:
    """The fuzzy union of given neighbour lists and (rho, sigma): device ``indptr`` (rows + S), ``indices``, ``data`` and
    host ``offsets``, ``nnz_offsets`` (see ``neighbors``)."""
    rows, k = _list_shape(knn_indices, "knn_indices")
    off = validate_offsets(offsets, rows, k)
    mix = _check_mix(set_op_mix_ratio)
    for a, name, shape in ((knn_distances, "knn_distances", (rows, k)), (rho, "rho", (rows,)), (sigma, "sigma", (rows,))):
        if tuple(a.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(a.shape)}")
    dev = device("neighbors")
    plan = _Plan(off, k, dev)
    idx = dense(knn_indices, "knn_indices", (rows, k), torch.int32, dev)
    dist = dense(knn_distances, "knn_distances", (rows, k), torch.float64, dev)
    r, s = dense(rho, "rho", (rows,), torch.float64, dev), dense(sigma, "sigma", (rows,), torch.float64, dev)
    indptr, indices, data, nnz_off = plan.connectivities(idx, dist, r, s, mix)
    return {"indptr": indptr, "indices": indices, "data": data, "offsets": off, "nnz_offsets": nnz_off}


def _list_shape(a: ArrayLike, name: str) -> Tuple[int, int]:
    if len(a.shape) != 2:
        raise ValueError(f"{name}: expected a 2-D (rows, n_neighbors) array, got shape {tuple(a.shape)}")
    return int(a.shape[0]), validate_neighbors(int(a.shape[1]))


def _check_mix(set_op_mix_ratio: float) -> float:
    mix = float(set_op_mix_ratio)
    if not 0.0 <= mix <= 1.0:
        raise ValueError(f"set_op_mix_ratio must lie in 0 .. 1, got {set_op_mix_ratio}")
    return mix


def neighbors(x: ArrayLike, offsets: Optional[Sequence[int]] = None, n_neighbors: int = 15,
              set_op_mix_ratio: float = 1.0) -> Dict[str, object]:
    """The neighbourhood graph of every segment of the row-stacked (rows, D <= 64) matrix ``x`` (see the module
    docstring).  Device tensors: ``knn_indices`` (rows, k) int32 and ``knn_distances`` (rows, k) fp64, ``rho`` and
    ``sigma`` (rows,), the connectivities as ``indptr`` (rows + S) int64, ``indices`` int32 and ``data`` fp64 -- segment
    s is the CSR ``indptr[offsets[s] + s : offsets[s + 1] + s + 1]`` (starting at 0) over
    ``indices / data[nnz_offsets[s] : nnz_offsets[s + 1]]``, columns segment-local and ascending.  Host: ``offsets``,
    ``nnz_offsets``."""
    off = _check_x(x, offsets, n_neighbors)
    mix = _check_mix(set_op_mix_ratio)
    dev = device("neighbors")
    plan = _Plan(off, n_neighbors, dev)
    xd = matrix(x, "x", dev, FLOAT_CODE, torch.float64)
    e = empty(dev)
    idx, dist = e((plan.rows, plan.k), torch.int32), e((plan.rows, plan.k), torch.float64)
    rho, sigma = e((plan.rows,), torch.float64), e((plan.rows,), torch.float64)
    plan.knn(xd, idx, dist)
    plan.smooth(dist, rho, sigma)
    indptr, indices, data, nnz_off = plan.connectivities(idx, dist, rho, sigma, mix)
    return {"knn_indices": idx, "knn_distances": dist, "rho": rho, "sigma": sigma, "indptr": indptr, "indices": indices,
            "data": data, "offsets": off, "nnz_offsets": nnz_off}


def _host(t) -> np.ndarray:
    return t.cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)


def to_scipy(res: Dict[str, object], segment: int = 0):
    """``(distances, connectivities)`` of one segment as ``scipy.sparse.csr_matrix`` (n_s, n_s) with scanpy's conventions:
    ``distances`` holds the neighbours other than the row itself at a distance above 0 (scanpy's ``eliminate_zeros``),
    ``connectivities`` is symmetric; both have sorted column indices."""
    from scipy import sparse
    off, nnz_off = res["offsets"], res["nnz_offsets"]
    S = len(off) - 1
    if not 0 <= segment < S:
        raise ValueError(f"segment must lie in 0 .. {S - 1}, got {segment}")
    lo, hi = int(off[segment]), int(off[segment + 1])
    n = hi - lo
    indptr = _host(res["indptr"])[lo + segment:hi + segment + 1]
    a, b = int(nnz_off[segment]), int(nnz_off[segment + 1])
    conn = sparse.csr_matrix((_host(res["data"])[a:b], _host(res["indices"])[a:b], indptr), shape=(n, n))
    idx, dist = _host(res["knn_indices"])[lo:hi], _host(res["knn_distances"])[lo:hi]
    k = idx.shape[1]
    rows = np.repeat(np.arange(n), k)
    keep = (idx.ravel() != rows) & (dist.ravel() > 0)
    d = sparse.csr_matrix((dist.ravel()[keep], (rows[keep], idx.ravel()[keep])), shape=(n, n))
    d.sort_indices()
    return d, conn


# ---------------------------------------------------------------------------------------------------- the notebook
def expression_graph(expr: ArrayLike, batch_idx=None, preprocess: bool = True, normalize_and_log: bool = True,
                     n_top_genes: int = N_TOP_GENES, n_pcs: int = N_PCS, n_neighbors: int = N_NEIGHBORS,
                     pca_solver: str = "host") -> Dict[str, object]:
    """``visualize_umap_clusters`` up to and including ``sc.pp.neighbors`` on one (spots, genes) matrix.
    ``preprocess=True``: the flags of ``preprocess.gene_stats`` (normalize_total, log1p, highly_variable_genes), the
    notebook's ``n_top_genes:  N`` line, then the PCA (``cluster.pca_device``, ``n_pcs`` components) of the flagged
    columns as ``preprocess.expression_matrices`` log-normalises them (log10(c / rowsum 1e4 + 1), the row sum over the
    flagged genes: this library's expression matrix, not scanpy's ln(c / size x median + 1) over all genes), then the
    graph.  ``preprocess=False``: the PCA of the matrix as given.  Returns ``neighbors``' dict plus ``scores`` (spots,
    n_pcs), ``highly_variable`` ((genes,) bool on the device, or None) and ``batch_idx`` as it was passed.
    ``pca_solver``: the PCA's eigensolver, ``"host"`` or ``"device"`` (``cluster.pca_device``'s ``solver``)."""
    if pca_solver not in cluster.SOLVERS:
        raise ValueError(f"pca_solver must be one of {cluster.SOLVERS}, got {pca_solver!r}")
    if preprocess and not normalize_and_log:
        raise ValueError("preprocess=True with normalize_and_log=False is not available: preprocess.gene_stats normalises "
                         "and takes the logarithm by construction (pass counts, or preprocess=False for a ready matrix)")
    if len(expr.shape) != 2:
        raise ValueError(f"expr: expected a 2-D (spots, genes) array, got shape {tuple(expr.shape)}")
    validate_offsets(None, int(expr.shape[0]), n_neighbors)
    hv = None
    x = expr
    if preprocess:
        counts = _pre._SlideSet([expr], device("neighbors")).tensors[0]      # one upload for both calls
        hv = _pre.gene_stats([counts], None, n_top_genes)["highly_variable"][0]
        genes = np.flatnonzero(hv.cpu().numpy())
        print("n_top_genes: ", int(genes.size))
        x = _pre.expression_matrices([counts], None, genes)[0].T
    scores = cluster.pca_device(x, None, n_pcs, pca_solver)["scores"]
    res = neighbors(scores, None, n_neighbors)
    res.update(scores=scores, highly_variable=hv, batch_idx=batch_idx)
    return res


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.neighbors",
                                description="PCA + the exact neighbourhood graph of expression matrices, one graph per "
                                            "slide (BLEEP's visualize_umap_clusters: sc.pp.pca, sc.pp.neighbors)")
    p.add_argument("--pred", required=True, nargs="+", help="one gene-major (genes, spots) .npy per slide")
    p.add_argument("--raw", action="store_true",
                   help="the files hold counts: select highly variable genes and log-normalise them first")
    p.add_argument("--n_top_genes", type=int, default=N_TOP_GENES, help="with --raw")
    p.add_argument("--n_neighbors", type=int, default=N_NEIGHBORS)
    p.add_argument("--n_pcs", type=int, default=N_PCS)
    p.add_argument("--out_dir", default=".", help=f"writes OUT_DIR/<slide number from 1>/{OUT_FILE}")
    a = p.parse_args(argv)
    if not 2 <= a.n_neighbors <= MAX_NEIGHBORS:
        p.error(f"--n_neighbors must lie in 2 .. {MAX_NEIGHBORS}, got {a.n_neighbors}")
    if not 1 <= a.n_pcs <= MAX_DIM:
        p.error(f"--n_pcs must lie in 1 .. {MAX_DIM}, got {a.n_pcs}")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    for i, m in enumerate(_arrays.load_gene_major(a.pred)):
        res = expression_graph(np.ascontiguousarray(m), preprocess=a.raw, n_top_genes=a.n_top_genes, n_pcs=a.n_pcs,
                               n_neighbors=a.n_neighbors)
        d, c = to_scipy(res, 0)
        path = os.path.join(a.out_dir, str(i + 1))
        os.makedirs(path, exist_ok=True)
        np.savez(os.path.join(path, OUT_FILE), knn_indices=res["knn_indices"].cpu().numpy(),
                 knn_distances=res["knn_distances"].cpu().numpy(), distances_indptr=d.indptr, distances_indices=d.indices,
                 distances_data=d.data, connectivities_indptr=c.indptr, connectivities_indices=c.indices,
                 connectivities_data=c.data)
        sigma = res["sigma"].cpu().numpy()
        print(f"slide {i + 1}: {m.shape[0]} spots, k {a.n_neighbors}, nnz {c.nnz}, sigma {sigma.min():.6g} .. "
              f"{sigma.max():.6g} -> {os.path.join(path, OUT_FILE)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
