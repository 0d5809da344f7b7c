"""Spatial autocorrelation on the MI355X: Moran's I and Geary's C of every gene on the spot lattice graph, what
``squidpy.gr.spatial_autocorr`` (esda's ``Moran`` / ``Geary``) leaves per gene -- the statistic, its analytic z and p under
normality, a permutation test -- for all slides of an evaluation per call, and the number the feature exists for: does a
predicted gene vary across the tissue the way the measured gene does (``svg_recovery``)?  The graph is the reference's
``calcADJ(coord, k, 'euclidean', pruneTag)`` (baselines/His2ST/graph_construction.py) as a fixed-width neighbour list.

What is computed is stated in DESIGN 6.16 and restated in numpy by ``tests/spatial_reference.py``, which is pinned to
``calcADJ`` itself, to dense-matrix formulas, to scipy and to mpmath.  squidpy and esda are not installed: parity with a
release of either is unpinned.  Things to know:

* ``lattice``: the k nearest other spots of every spot (``neighbors.knn``: exact Euclidean distance, ties to the smaller
  index -- ``calcADJ``'s unstable ``argsort`` leaves them open); ``prune`` "NA" keeps all k, "STD" keeps d <= mean +
  population std of the row's k distances, "Grid" keeps d <= 2.  Kept edges weigh 1, or 1 / deg with ``row_standardise``
  (squidpy's ``transformation=True``, esda's "r"); a pruned slot keeps its index and weighs 0.  1 <= k <= 64,
  k + 1 <= n_s <= 16384.  A given list (``nbr=``, ``w=``) must be binary or row-standardised: any other weights are refused,
  because the in-weight sums of S2 are only order-independent for those two.
* ``autocorr``: I, C, E and Var under normality, ``z_norm``, ``pval_norm`` = sf(|z|) (``two_tailed``: twice that),
  ``neglog10_pval_norm`` in log space (finite where p underflows), Benjamini-Hochberg over the genes of a slide.  A constant
  gene is NaN in every output (and counts as p = 1 in the adjustment of the others).  G <= 16384.
* Permutations relabel the spots of a slide and are shared by its genes; permutation p is a pure function of (seed, p, n)
  -- not of the slide's place in the batch, and not squidpy's random stream.  The sims come from the same kernel and
  summation order as the observed value: the identity permutation reproduces it bit for bit.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible run to run; a slide inside a batch
is bit-identical to the same slide alone.  No CPU fallback: without a GPU / the HIP library these functions raise
``RuntimeError``.

    python -m mclstexp_amd.spatial --pred P1.npy ... --coords C1.npy ... [--true T1.npy ...] [--k 8] [--prune NA|STD|Grid]
                                   [--mode moran|geary|both] [--n_perms 100] [--seed 0] [--genes names.npy] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import neighbors
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_flag, check_int, cumulative_offsets, dense, device, empty,
                      load_gene_major, matrix, stack_rows, upload, validate_offsets)
from ._lib import call

MAX_ROWS = 16384         # csrc/spatial.hip: 14 index bits in a permutation key, uint16 tables
MAX_K = 64
MAX_GENES = 16384
MAX_SLIDES = 32767
MAX_PERMS = 65535
PRUNES = {"NA": 0, "STD": 1, "Grid": 2}
MODES = ("moran", "geary", "both")
OUT_FILE = "spatial_autocorr.npz"
TOP_N = 50
_STATUS = ("offsets that do not match the host's", "neighbour indices outside the slide",
           "weights that are negative or not finite", "neighbours listed twice in a row")
_PER_GENE = ("stat", "z_norm", "pval_norm", "neglog10_pval_norm", "pval_norm_adj", "pval_sim", "pval_z_sim", "mean_sim",
             "var_sim", "count_sim")


# ------------------------------------------------------------------------------------------------------- host rules
def check_lattice(shape: Sequence[int], offsets, k, prune, row_standardise):
    """The limits of ``lattice``, checked on the host before the GPU is touched.  Returns (offsets int64, k, prune code)."""
    if len(shape) != 2 or int(shape[1]) != 2:
        raise ValueError(f"coords: expected a (rows, 2) array, got shape {tuple(shape)}")
    k = check_int(k, "k", 1, MAX_K)
    if prune not in PRUNES:
        raise ValueError(f"prune must be one of {sorted(PRUNES)}, got {prune!r}")
    check_flag(row_standardise, "row_standardise")
    off = validate_offsets(offsets, int(shape[0]), min_rows=2, max_rows=MAX_ROWS, max_segments=MAX_SLIDES, none_is_one=True,
                           noun="slide")
    seg = np.diff(off)
    if (seg < k + 1).any():
        raise ValueError(f"k = {k} neighbours need at least {k + 1} spots in every slide; slide sizes {seg.tolist()}")
    return off, k, PRUNES[prune]


def check_autocorr(shape: Sequence[int], graph, mode, n_perms, seed, two_tailed, return_sims):
    if not isinstance(graph, dict) or not {"nbr", "w", "consts", "offsets", "k"} <= set(graph):
        raise ValueError("graph: expected what lattice() returns")
    if len(shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(shape)}")
    rows, G = int(shape[0]), int(shape[1])
    if G < 1 or G > MAX_GENES:
        raise ValueError(f"1 .. {MAX_GENES} genes per call, got {G}")
    if rows != int(graph["offsets"][-1]):
        raise ValueError(f"x has {rows} rows, the graph {int(graph['offsets'][-1])}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {list(MODES)}, got {mode!r}")
    P = check_int(n_perms, "n_perms", 0, MAX_PERMS)
    seed = check_int(seed, "seed", 0, 2 ** 64 - 1)
    check_flag(two_tailed, "two_tailed")
    check_flag(return_sims, "return_sims")
    return rows, G, P, seed


def check_permutations(permutations, sizes: np.ndarray) -> np.ndarray:
    """``permutations``: one (P, n_s) integer array per slide, every row a permutation of 0 .. n_s - 1, one P for all
    slides.  Returns the table in the device's layout: the slides' blocks one after the other, as int16."""
    if not isinstance(permutations, (list, tuple)) or len(permutations) != sizes.size:
        raise ValueError(f"permutations: expected a list of {sizes.size} arrays, one (P, n_s) array per slide")
    parts, P = [], None
    for s, (a, n) in enumerate(zip(permutations, sizes)):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != n or not np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
            raise ValueError(f"permutations[{s}]: expected an integer (P, {int(n)}) array, got shape {a.shape} dtype {a.dtype}")
        if P is None:
            P = a.shape[0]
        if a.shape[0] != P or P < 1 or P > MAX_PERMS:
            raise ValueError(f"permutations[{s}]: every slide needs the same 1 .. {MAX_PERMS} permutations, got {a.shape[0]}")
        if not np.array_equal(np.sort(a, axis=1), np.broadcast_to(np.arange(n), a.shape)):
            bad = int(np.flatnonzero((np.sort(a, axis=1) != np.arange(n)).any(axis=1))[0])
            raise ValueError(f"permutations[{s}]: row {bad} is not a permutation of 0 .. {int(n) - 1}")
        parts.append(a.astype(np.int16).ravel())
    return np.concatenate(parts)


# ----------------------------------------------------------------------------------------------------------- device
def lattice(coords: Optional[ArrayLike] = None, offsets: Optional[Sequence[int]] = None, k: int = 8, prune: str = "NA",
            row_standardise: bool = True, nbr: Optional[ArrayLike] = None, w: Optional[ArrayLike] = None) -> Dict[str, object]:
    """The spot lattice graph of every slide of the row-stacked (rows, 2) ``coords`` (fp32 / fp64 on host or device, or
    host integers), or -- with ``nbr=`` and ``w=`` of shape (rows, k), segment-local indices -- a given neighbour list,
    validated.  Returns device ``nbr`` (rows, k) int32, ``w`` (rows, k) fp64, ``deg`` (rows,) int32 and ``consts`` (S, 3),
    and on the host ``S0``, ``S1``, ``S2`` (S,), ``offsets``, ``k``, ``prune``, ``row_standardise``.  The one read-back is
    the status words and the constants."""
    given = nbr is not None or w is not None
    if given:
        if nbr is None or w is None or coords is not None:
            raise ValueError("a given graph needs both nbr= and w= and no coords")
        if len(nbr.shape) != 2:
            raise ValueError(f"nbr: expected a 2-D (rows, k) array, got shape {tuple(nbr.shape)}")
        rows, k = int(nbr.shape[0]), check_int(int(nbr.shape[1]), "k", 1, MAX_K)
        off = validate_offsets(offsets, rows, min_rows=2, max_rows=MAX_ROWS, max_segments=MAX_SLIDES, none_is_one=True,
                               noun="slide")
        code = 0
        if not isinstance(w, Tensor) and not np.isfinite(np.asarray(w, dtype=np.float64)).all():
            raise ValueError("w: weights must be finite")
    else:
        if coords is None:
            raise ValueError("lattice needs coords, or a given graph (nbr= and w=)")
        if not isinstance(coords, Tensor):
            coords = np.asarray(coords)
            if np.issubdtype(coords.dtype, np.integer):
                coords = coords.astype(np.float64)
        off, k, code = check_lattice(tuple(coords.shape), offsets, k, prune, row_standardise)
        rows = int(off[-1])
    dev = device("spatial")
    e = empty(dev)
    S, max_n = int(off.size - 1), int(np.diff(off).max())
    if given:
        nbr_d = dense(nbr, "nbr", (rows, k), torch.int32, dev, copy=True, integer=True)      # copies: the kernel's outputs
        w_d = dense(w, "w", (rows, k), torch.float64, dev, copy=True, integer=False)         # alias nothing
        idx = dist = None
    else:
        idx, dist = neighbors.knn(coords, off, k + 1)
        nbr_d, w_d = e((rows, k), torch.int32), e((rows, k), torch.float64)
    deg, consts, status = e((rows,), torch.int32), e((S, 3), torch.float64), e((S, 6), torch.int32)
    work = e((int(call("mcl_spatial_workspace_bytes", rows, k + 1, 0)) // 8 + 1,), torch.float64)
    off_d = upload(off, dev)
    call("mcl_spatial_lattice", idx, dist, off_d, S, rows, max_n, k, code, int(bool(row_standardise)), int(given), work,
         nbr_d, w_d, deg, consts, status)
    bad = status.cpu().numpy()                                  # the one synchronisation
    for col, what in enumerate(_STATUS):
        if bad[:, col].any():
            s = int(np.flatnonzero(bad[:, col])[0])
            raise ValueError(f"lattice: slide {s} holds {what}" + (f" ({int(bad[s, col])})" if col else ""))
    mixed = (bad[:, 4] != 0) & (bad[:, 5] != 0)
    if mixed.any():
        raise ValueError(f"w: slide {int(np.flatnonzero(mixed)[0])} is neither binary (every kept weight 1) nor "
                         "row-standardised (every kept weight 1 / deg): S2 would depend on the summation order")
    c = consts.cpu().numpy()
    return {"nbr": nbr_d, "w": w_d, "deg": deg, "consts": consts, "S0": c[:, 0].copy(), "S1": c[:, 1].copy(),
            "S2": c[:, 2].copy(), "offsets": off, "offsets_device": off_d, "k": k, "prune": None if given else prune,
            "row_standardise": bool((bad[:, 4] != 0).any()) if given else bool(row_standardise)}


def autocorr_device(x: ArrayLike, graph: Dict[str, object], n_perms: int = 0, seed: int = 0, permutations=None,
                    two_tailed: bool = False) -> Dict[str, object]:
    """``autocorr`` with everything left on the device.  The (2, S, G) tensors hold Moran's I first, Geary's C second:
    ``stat``, ``z_norm``, ``pval_norm``, ``neglog10_pval_norm``, ``pval_norm_adj`` and, with permutations, ``pval_sim``,
    ``pval_z_sim``, ``mean_sim``, ``var_sim``, ``count_sim`` (int32) and ``sims`` (2, S, P, G); ``mean`` and ``den`` are
    (S, G); ``table`` is the int16 view of the permutation table (slide s: (P, n_s) at element P * offsets[s])."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    rows, G, P, seed = check_autocorr(shape, graph, "both", n_perms, seed, two_tailed, False)
    off, k = graph["offsets"], int(graph["k"])
    sizes = np.diff(off)
    host_table = None
    if permutations is not None:
        host_table = check_permutations(permutations, sizes)
        P = host_table.size // rows
    dev = device("spatial")
    xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
    S, max_n = int(sizes.size), int(sizes.max())
    e = empty(dev)
    f64, i32 = torch.float64, torch.int32
    mask = 0
    for n in np.unique(sizes):
        mask |= 1 << int(call("mcl_spatial_columns", int(n)))
    code, ld = FLOAT_CODE[xd.dtype], int(xd.stride(0))
    off_d = graph["offsets_device"]
    status = torch.zeros((S,), device=dev, dtype=i32)
    mean, den, stat = e((S, G), f64), e((S, G), f64), e((2, S, G), f64)
    call("mcl_spatial_stats", xd, ld, code, off_d, S, rows, G, max_n, k, mask, graph["nbr"], graph["w"], graph["consts"],
         None, 1, mean, den, stat, status)
    zn, pv, nl, adj = (e((2, S, G), f64) for _ in range(4))
    prank, scratch = e((2, S, G), i32), e((2, S, G), f64)
    call("mcl_spatial_moments", off_d, S, rows, G, max_n, graph["consts"], stat, int(bool(two_tailed)), prank, scratch, zn,
         pv, nl, adj)
    out = {"stat": stat, "mean": mean, "den": den, "z_norm": zn, "pval_norm": pv, "neglog10_pval_norm": nl,
           "pval_norm_adj": adj, "n_perms": P}
    if P:
        work = e((int(call("mcl_spatial_workspace_bytes", rows, 0, P)) // 8 + 1,), f64)
        table = work.view(torch.int16)[:P * rows]
        if host_table is None:
            call("mcl_spatial_permutations", off_d, S, rows, max_n, P, seed, work)
        else:
            table.copy_(torch.from_numpy(host_table))
        sims = e((2, S, P, G), f64)
        call("mcl_spatial_stats", xd, ld, code, off_d, S, rows, G, max_n, k, mask, graph["nbr"], graph["w"],
             graph["consts"], work, P, None, None, sims, status)
        count = e((2, S, G), i32)
        ps, pz, ms, vs = (e((2, S, G), f64) for _ in range(4))
        call("mcl_spatial_perm_summary", S, G, P, stat, sims, int(bool(two_tailed)), count, ps, pz, ms, vs)
        out.update({"sims": sims, "count_sim": count, "pval_sim": ps, "pval_z_sim": pz, "mean_sim": ms, "var_sim": vs,
                    "table": table, "workspace": work})
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad.any():
        s = int(np.flatnonzero(bad)[0])
        raise ValueError(f"x: slide {s} holds non-finite values")
    return out


def expected_moments(n: int, S0: float, S1: float, S2: float) -> Dict[str, float]:
    """E and Var of I and C under normality (esda's ``EI`` / ``VI_norm`` / ``EC`` / ``VC_norm``), on the host."""
    n = float(n)
    EI = -1.0 / (n - 1.0)
    VI = ((n * n) * S1 - n * S2 + 3.0 * S0 * S0) / ((n * n - 1.0) * S0 * S0) - EI * EI
    VC = ((2.0 * S1 + S2) * (n - 1.0) - 4.0 * S0 * S0) / ((2.0 * (n + 1.0)) * S0 * S0)
    return {"EI": EI, "VI": VI, "EC": 1.0, "VC": VC}


def autocorr(x: ArrayLike, graph: Dict[str, object], mode: str = "moran", n_perms: int = 0, seed: int = 0,
             permutations=None, return_sims: bool = False, two_tailed: bool = False,
             return_permutations: bool = False) -> List[Dict[str, object]]:
    """Moran's I and / or Geary's C of every gene of every slide.

    ``x``: row-stacked (rows, G), float32 or float64, host or device, a row stride allowed.  ``graph``: what ``lattice``
    returned for the same rows.  ``n_perms``: permutations of the spots per slide (0: none), generated from ``seed``, or
    replayed from ``permutations`` (one (P, n_s) integer array per slide).  Returns one dict per slide: ``n``, ``k``,
    ``S0``, ``S1``, ``S2``, ``mean`` and ``den`` (G,), and under ``"moran"`` / ``"geary"`` (as ``mode`` asks) a dict of
    (G,) arrays ``stat``, ``z_norm``, ``pval_norm``, ``neglog10_pval_norm``, ``pval_norm_adj``, the scalars ``expected`` and
    ``var_norm``, and with permutations ``pval_sim``, ``pval_z_sim``, ``mean_sim``, ``var_sim``, ``count_sim`` (and ``sims``
    (P, G) with ``return_sims``).  ``return_permutations`` adds ``permutations`` (P, n) per slide."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    check_autocorr(shape, graph, mode, n_perms, seed, two_tailed, return_sims)
    check_flag(return_permutations, "return_permutations")
    d = autocorr_device(x, graph, n_perms, seed, permutations, two_tailed)
    P, off = int(d["n_perms"]), graph["offsets"]
    keys = [key for key in _PER_GENE if key in d]
    host = {key: d[key].cpu().numpy() for key in keys + ["mean", "den"]}
    sims = d["sims"].cpu().numpy() if P and return_sims else None
    table = d["table"].cpu().numpy() if P and return_permutations else None
    out = []
    for s in range(off.size - 1):
        n = int(off[s + 1] - off[s])
        S0, S1, S2 = (float(graph[key][s]) for key in ("S0", "S1", "S2"))
        mom = expected_moments(n, S0, S1, S2)
        one = {"n": n, "k": int(graph["k"]), "S0": S0, "S1": S1, "S2": S2, "mean": host["mean"][s], "den": host["den"][s],
               "n_perms": P}
        for which, name, ex, var in ((0, "moran", "EI", "VI"), (1, "geary", "EC", "VC")):
            if mode not in (name, "both"):
                continue
            r = {key: host[key][which, s] for key in keys}
            r["expected"], r["var_norm"] = mom[ex], mom[var]
            if sims is not None:
                r["sims"] = sims[which, s]
            one[name] = r
        if table is not None:
            one["permutations"] = table[P * int(off[s]):P * int(off[s + 1])].reshape(P, n).astype(np.int64)
        out.append(one)
    return out


def autocorr_slides(matrices: Sequence[ArrayLike], coords: Sequence[ArrayLike], k: int = 8, prune: str = "NA",
                    row_standardise: bool = True, **kw) -> List[Dict[str, object]]:
    """``autocorr`` of one (spots, genes) matrix and one (spots, 2) coordinate array per slide."""
    if len(matrices) != len(coords) or not len(matrices):
        raise ValueError(f"need one coordinate array per slide and >= 1 slide; got {len(matrices)} and {len(coords)}")
    cs = []
    for i, (m, c) in enumerate(zip(matrices, coords)):
        c = c.cpu().numpy() if isinstance(c, Tensor) else np.asarray(c)
        if len(m.shape) != 2 or c.ndim != 2 or c.shape != (m.shape[0], 2):
            raise ValueError(f"slide {i}: matrix {tuple(m.shape)} and coordinates {tuple(c.shape)} do not match")
        cs.append(c.astype(np.float64))
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    check_lattice((int(off[-1]), 2), off, k, prune, row_standardise)
    dev = device("spatial")
    x, off = stack_rows(matrices, "matrices", dev)
    graph = lattice(np.concatenate(cs), off, k, prune, row_standardise)
    return autocorr(x, graph, **kw)


def _key(mode: str) -> str:
    if mode not in ("moran", "geary"):
        raise ValueError(f"mode must be 'moran' or 'geary' here, got {mode!r}")
    return mode


def rank_genes(stat: np.ndarray, mode: str = "moran") -> np.ndarray:
    """Gene indices by descending I (ascending C), equal values by gene index, NaN last."""
    v = np.asarray(stat, dtype=np.float64)
    key = np.where(np.isnan(v), np.inf, -v if _key(mode) == "moran" else v)
    return np.argsort(key, kind="stable")


def top_genes(res: Sequence[Dict[str, object]], slide: int, n: int = TOP_N, mode: str = "moran") -> np.ndarray:
    """The indices of the ``n`` most autocorrelated genes of one slide, most first."""
    stat = res[slide][_key(mode)]["stat"]
    return rank_genes(stat, mode)[:max(1, min(int(n), stat.size))]


def pearson(a: np.ndarray, b: np.ndarray) -> float:
    """Pearson r over the genes where both statistics are defined (host: G numbers)."""
    ok = np.isfinite(a) & np.isfinite(b)
    if ok.sum() < 2:
        return float("nan")
    da, db = a[ok] - a[ok].mean(), b[ok] - b[ok].mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else float("nan")


def svg_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], coords: Sequence[ArrayLike], n_top: int = TOP_N,
                 mode: str = "moran", **kw) -> Dict[str, object]:
    """Do the predicted values vary across the tissue the way the measured ones do?  Per slide: ``pearson``, the
    correlation over genes between the statistic of the predicted and of the measured matrix, and ``overlap`` /
    ``jaccard`` of their ``n_top`` most autocorrelated genes.  Also ``mean_pearson``, ``mean_overlap``, ``mean_jaccard``,
    ``n_top`` and the two results ``pred`` / ``true``."""
    _key(mode)
    if len(preds) != len(trues):
        raise ValueError(f"need one measured matrix per prediction; got {len(preds)} and {len(trues)}")
    for i, (p, t) in enumerate(zip(preds, trues)):
        if tuple(p.shape) != tuple(t.shape):
            raise ValueError(f"slide {i}: pred {tuple(p.shape)} and true {tuple(t.shape)} differ in shape")
    if isinstance(n_top, bool) or not isinstance(n_top, (int, np.integer)) or n_top < 1:
        raise ValueError(f"n_top must be a positive integer, got {n_top!r}")
    rp = autocorr_slides(preds, coords, mode=mode, **kw)
    rt = autocorr_slides(trues, coords, mode=mode, **kw)
    top = min(int(n_top), int(rp[0][mode]["stat"].size))
    r, overlap, jaccard = [], [], []
    for s in range(len(rp)):
        a, b = top_genes(rp, s, top, mode), top_genes(rt, s, top, mode)
        o = np.intersect1d(a, b).size
        r.append(pearson(rp[s][mode]["stat"], rt[s][mode]["stat"]))
        overlap.append(int(o))
        jaccard.append(o / np.union1d(a, b).size)
    return {"pearson": np.asarray(r), "overlap": np.asarray(overlap, dtype=np.int64), "jaccard": np.asarray(jaccard),
            "mean_pearson": float(np.mean(r)), "mean_overlap": float(np.mean(overlap)),
            "mean_jaccard": float(np.mean(jaccard)), "n_top": top, "mode": mode, "pred": rp, "true": rt}


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.spatial",
                                description="Moran's I / Geary's C of every gene on the spot lattice graph "
                                            "(squidpy.gr.spatial_autocorr) and how well predictions recover the spatially "
                                            "variable genes of the measured matrix")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--coords", required=True, nargs="+", help="one (N, 2) coordinate array per slide")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery line")
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--prune", default="NA", choices=list(PRUNES))
    p.add_argument("--no_row_standardise", action="store_true", help="binary weights instead of 1 / deg")
    p.add_argument("--mode", default="moran", choices=list(MODES))
    p.add_argument("--n_perms", type=int, default=100)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--two_tailed", action="store_true")
    p.add_argument("--top", type=int, default=TOP_N, help="genes the recovery overlap is scored on")
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the gene index)")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if len(a.coords) != len(a.pred):
        p.error(f"{len(a.coords)} --coords files for {len(a.pred)} --pred files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.k < 1 or a.k > MAX_K:
        p.error(f"--k must lie in 1 .. {MAX_K}")
    if a.n_perms < 0 or a.n_perms > MAX_PERMS:
        p.error(f"--n_perms must lie in 0 .. {MAX_PERMS}")
    if a.seed < 0:
        p.error("--seed must be >= 0")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def format_slides(res: Sequence[Dict[str, object]], genes: Optional[Sequence[str]], mode: str, top: int = 5) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        for m in ("moran", "geary"):
            if m not in r:
                continue
            cells = [f"{genes[j] if genes is not None else j} ({r[m]['stat'][j]:.4f}, {r[m]['neglog10_pval_norm'][j]:.2f})"
                     for j in top_genes(res, s, top, m)]
            lines.append(f"slide {s} n = {r['n']} k = {r['k']} S0 = {r['S0']:.6g} {'I' if m == 'moran' else 'C'} "
                         f"(-log10 p): " + ", ".join(cells))
    return lines


def format_recovery(rec: Dict[str, object]) -> List[str]:
    lines = [f"slide {s}: Pearson {rec['pearson'][s]:.4f}, overlap {int(rec['overlap'][s])} / {rec['n_top']}, "
             f"Jaccard {rec['jaccard'][s]:.4f}" for s in range(len(rec["pearson"]))]
    lines.append(f"recovery ({rec['mode']}): mean Pearson {rec['mean_pearson']:.4f}, mean overlap {rec['mean_overlap']:.4f} / "
                 f"{rec['n_top']}, mean Jaccard {rec['mean_jaccard']:.4f}")
    return lines


def flatten(r: Dict[str, object]) -> Dict[str, np.ndarray]:
    """One slide's result as flat arrays for ``np.savez``: ``moran_stat``, ``geary_pval_sim``, ..."""
    flat = {}
    for key, v in r.items():
        if isinstance(v, dict):
            flat.update({f"{key}_{sub}": np.asarray(val) for sub, val in v.items()})
        else:
            flat[key] = np.asarray(v)
    return flat


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    coords = [np.load(f) for f in args.coords]
    G = preds[0].shape[1]
    genes = None
    if args.genes is not None:
        genes = [str(v) for v in np.load(args.genes, allow_pickle=True).reshape(-1)]
        if len(genes) != G:
            raise ValueError(f"{args.genes}: {len(genes)} gene names for {G} genes")
    kw = dict(k=args.k, prune=args.prune, row_standardise=not args.no_row_standardise, n_perms=args.n_perms,
              seed=args.seed, two_tailed=args.two_tailed)
    res = autocorr_slides(preds, coords, mode=args.mode, **kw)
    print("\n".join(format_slides(res, genes, args.mode)))
    if args.out_dir is not None:
        for i, r in enumerate(res):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, OUT_FILE), **flatten(r))
    if args.true is not None:
        trues = load_gene_major(args.true)
        for m in ("moran", "geary"):
            if args.mode in (m, "both"):
                print("\n".join(format_recovery(svg_recovery(preds, trues, coords, n_top=min(args.top, G), mode=m, **kw))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
