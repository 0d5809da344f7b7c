"""How spot groups are arranged in the tissue, on the MI355X: what ``squidpy.gr.nhood_enrichment``, ``interaction_matrix``
and ``co_occurrence`` compute from group labels, the spot lattice and the coordinates -- which groups sit next to which more
often than under permuted labels, and how the chance of meeting a group changes with distance -- for all slides of an
evaluation per call, and the number the feature exists for: are predicted domains arranged in the tissue the way the
measured ones are (``arrangement_recovery``)?  The groups are whatever labels a slide carries: ``cluster`` / ``mixture`` /
``hmrf`` domains, ``leiden`` communities or the pathologist's annotation.

What is computed is stated in DESIGN 6.20 and restated in numpy by ``tests/nhood_reference.py``, which is pinned to dense
matrix products, ``pandas.crosstab`` and ``scipy.spatial.distance.cdist``.  squidpy is not installed: parity with a release
is unpinned, and neither its random stream nor its default radii are reproduced.  Things to know:

* Spots labelled -1 are dropped from everything; an edge or a pair with a dropped end does not exist (the graph is not
  rebuilt).
* ``count[c1, c2]`` = the neighbour slots (spot i, slot c) with ``w != 0``, label(i) = c1 and label(nbr) = c2.  Slots are
  directed: the matrix is symmetric only if the list is.  Weights other than zero or non-zero are ignored.
* Permutation p of a slide of n kept spots is ``mcl_spatial_permutations``' pure function of (seed, p, n), applied as
  ``ligrec`` applies it (group sizes are preserved); the observed count is the same kernel with the identity.
* ``zscore`` = (P count - S1) / sqrt(P S2 - S1^2) with S1, S2 the exact integer sum and sum of squares of the permuted counts:
  numerator and radicand are formed exactly, each converted to fp64 once; NaN where the radicand is 0.  ``perm_mean`` = S1 / P,
  ``perm_std`` = sqrt(P S2 - S1^2) / P.  ``pval_enriched`` = #(count_p >= count) / P, ``pval_depleted`` = #(count_p <= count) /
  P: nothing is added to numerator or denominator (``ligrec``'s rule), so p may be 0.
* ``pairs[t, c1, c2]`` = the ordered pairs i != j of kept spots with d^2 <= r_t r_t (coincident spots count);
  ``occ`` = (pairs / row) / (col / tot) = P(c2 | within r_t of c1) / P(c2), NaN where a denominator is 0.  ``radii`` an int T:
  ``linspace(R / T, R, T)`` per slide, R half the diagonal of the bounding box of the slide's kept spots (1 when they have
  no extent); that needs coordinates and labels on the host and copies device ones there.
* 2 <= n_s <= 16384 spots per slide, k <= 255 groups, <= 64 neighbour slots, n_perms <= 65535, <= 64 radii, <= 32767 slides,
  S k^2 and S T k^2 < 2^31: ``ValueError`` before a launch.  The kept spots of a slide may number 0 or 1 (counts 0, z and occ
  NaN, the identity as the only permutation).

Every count is an integer and bit-reproducible; a slide inside a batch is bit-identical to the same slide alone.  No CPU
fallback: without a GPU / the HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.nhood --labels L1.npy ... --coords C1.npy ... [--true_labels T1.npy ...] [--k 8]
                                 [--prune NA|STD|Grid] [--n_perms 1000] [--radii 50] [--seed 0] [--top 10] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import markers, spatial
from ._arrays import (ArrayLike, Tensor, check_flag, check_int, cumulative_offsets, device, empty, nanmean, upload,
                      validate_offsets)
from ._lib import call
from .ligrec import kept_sizes

MAX_ROWS = 16384         # csrc/nhood.hip: the uint16 permutation tables and neighbour lists
MAX_GROUPS = 255
MAX_SLOTS = 64
MAX_SLIDES = 32767
MAX_PERMS = 65535
MAX_RADII = 64
MAX_TOTAL = (1 << 31) - 1
DEFAULT_RADII = 50
OUT_FILE = "nhood.npz"
TOP_N = 10


# ------------------------------------------------------------------------------------------------------- host rules
def check_graph(graph) -> tuple:
    """Shapes and dtypes of the neighbour list, on the host.  Returns (offsets int64, rows, kw)."""
    if not isinstance(graph, dict) or any(name not in graph for name in ("nbr", "w", "offsets")):
        raise ValueError("graph: expected what spatial.lattice returns (nbr, w, offsets)")
    nbr, w = graph["nbr"], graph["w"]
    if len(nbr.shape) != 2 or tuple(w.shape) != tuple(nbr.shape):
        raise ValueError(f"graph: nbr and w must both be (rows, kw), got {tuple(nbr.shape)} and {tuple(w.shape)}")
    rows, kw = int(nbr.shape[0]), int(nbr.shape[1])
    if kw < 1 or kw > MAX_SLOTS:
        raise ValueError(f"graph: {kw} neighbour slots per spot; the kernel handles 1 .. {MAX_SLOTS}")
    if isinstance(nbr, Tensor):
        if nbr.dtype != torch.int32:
            raise ValueError(f"graph: nbr must be int32, got {nbr.dtype}")
    elif not np.issubdtype(np.asarray(nbr).dtype, np.integer):
        raise ValueError(f"graph: nbr must hold integers, got {np.asarray(nbr).dtype}")
    if isinstance(w, Tensor) and w.dtype != torch.float64:
        raise ValueError(f"graph: w must be float64, got {w.dtype}")
    off = validate_offsets(graph["offsets"], rows, min_rows=2, max_rows=MAX_ROWS, max_segments=MAX_SLIDES, noun="slide")
    return off, rows, kw


def check_labels(labels, rows: int, offsets: np.ndarray, k):
    """k per slide (int32) and, for host labels, their range: a label outside -1 .. k - 1 names its slide."""
    S = offsets.size - 1
    if isinstance(labels, Tensor):
        if k is None:
            raise ValueError("k: needed when the labels are a device tensor")
        if labels.dtype != torch.int32 or tuple(labels.shape) != (rows,):
            raise ValueError(f"labels: a tensor must be int32 of shape ({rows},), got {labels.dtype} {tuple(labels.shape)}")
        return markers.check_k(k, S)
    lab = np.asarray(labels)
    if lab.shape != (rows,) or not np.issubdtype(lab.dtype, np.integer) or lab.dtype == np.bool_:
        raise ValueError(f"labels: expected {rows} integer group ids (-1: not part of the analysis), got shape {lab.shape} "
                         f"dtype {lab.dtype}")
    kk = markers.check_k(markers.infer_k(lab, offsets) if k is None else k, S)
    for s in range(S):
        seg = lab[offsets[s]:offsets[s + 1]]
        bad = int(((seg < -1) | (seg >= int(kk[s]))).sum())
        if bad:
            raise ValueError(f"labels: slide {s} holds {bad} group ids outside -1 .. {int(kk[s]) - 1}")
    return kk


def check_cells(S: int, kmax: int, planes: int, what: str) -> None:
    if S * planes * kmax * kmax > MAX_TOTAL:
        raise ValueError(f"{what}: {S} slides x {planes} x {kmax}^2 cells; at most {MAX_TOTAL} per call")


def check_radii(radii) -> np.ndarray:
    """An explicit ``radii=``: finite, positive, increasing, at most 64 of them."""
    try:
        r = np.asarray(radii, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"radii: expected an int or a 1-D array of radii, got {radii!r}") from None
    if r.ndim != 1 or r.size < 1 or r.size > MAX_RADII:
        raise ValueError(f"radii: expected 1 .. {MAX_RADII} radii in a 1-D array, got shape {r.shape}")
    if not np.isfinite(r).all() or (r <= 0).any() or (np.diff(r) <= 0).any():
        raise ValueError("radii: must be finite, positive and increasing")
    return r


def default_radii(coords: np.ndarray, T: int) -> np.ndarray:
    """``linspace(R / T, R, T)``, R half the diagonal of the bounding box of ``coords`` (the kept spots of one slide) in fp64;
    R = 1 when they have no extent."""
    R = 0.0
    if coords.shape[0]:
        d = coords.max(axis=0) - coords.min(axis=0)
        R = 0.5 * float(np.sqrt(d[0] * d[0] + d[1] * d[1]))
    if not R > 0.0:
        R = 1.0
    return np.linspace(R / float(T), R, T)


def zscore(count: np.ndarray, S1: np.ndarray, S2: np.ndarray, P: int):
    """(z, perm_mean, perm_std) from the exact integers: numerator P count - S1 and radicand P S2 - S1^2 are formed with
    Python integers (P S2 passes 2^63), converted to fp64 once each; one sqrt, one division; NaN where the radicand is 0."""
    c, s1, s2 = (np.asarray(v).astype(object) for v in (count, S1, S2))
    num = (int(P) * c - s1).astype(np.float64)
    rad = (int(P) * s2 - s1 * s1).astype(np.float64)
    root = np.sqrt(rad)
    with np.errstate(all="ignore"):
        z = np.where(rad == 0.0, np.nan, num / root)
    return z, s1.astype(np.float64) / float(P), root / float(P)


def greedy_match(table) -> np.ndarray:
    """Groups matched on a contingency table: the largest cell first (ties: the smaller (row, column)), its row and column
    leave, until no positive cell is left.  Returns the (m, 2) matched (row, column) in the order taken."""
    t = np.array(table, dtype=np.int64, ndmin=2)
    out = []
    while t.size and t.max() > 0:
        r, c = divmod(int(np.argmax(t)), t.shape[1])
        out.append((r, c))
        t[r, :] = -1
        t[:, c] = -1
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


# ----------------------------------------------------------------------------------------------------------- device
def _prepare(labels, rows: int, off: np.ndarray, kk: np.ndarray, dev: torch.device) -> Dict[str, object]:
    lab_d = markers.device_labels(labels, rows, dev)
    S, max_n, kmax = int(off.size - 1), int(np.diff(off).max()), int(kk.max())
    e = empty(dev)
    i32 = torch.int32
    off_d, k_d = upload(off, dev), upload(kk, dev)
    order, start, koff, status = e((rows,), i32), e((S, kmax + 1), i32), e((S + 1,), torch.int64), e((S, 4), i32)
    call("mcl_ligrec_prepare", off_d, lab_d, k_d, S, rows, max_n, kmax, order, start, koff, status)
    return {"offsets_device": off_d, "k_device": k_d, "order": order, "start": start, "kept_offsets": koff, "status": status,
            "S": S, "max_n": max_n, "kmax": kmax}


def _raise_status(status: Tensor) -> None:
    bad = status.cpu().numpy()                                  # the one synchronisation
    if bad[:, 0].any():
        raise ValueError(f"slide {int(np.flatnonzero(bad[:, 0])[0])}: offsets or a group count the device refuses")
    for col, name, what in ((1, "labels", "group ids outside -1 .. k - 1"),
                            (2, "graph", "kept neighbour indices outside the slide (indices are local to the slide)"),
                            (3, "coords", "non-finite coordinates")):
        if bad[:, col].any():
            s = int(np.flatnonzero(bad[:, col])[0])
            raise ValueError(f"{name}: slide {s} holds {int(bad[s, col])} {what}")


def nhood_device(labels, graph: Dict[str, object], k=None, n_perms: int = 1000, seed: int = 0,
                 permutations=None) -> Dict[str, object]:
    """``nhood_enrichment`` with everything left on the device, stacked over the slides with the largest k as the group
    stride: ``count`` (S, kmax, kmax) int32, ``stats`` (S, 4, kmax, kmax) int64 (sum and sum of squares of the permuted
    counts, #(>= count), #(<= count); absent with ``n_perms`` 0), ``order`` (rows,), ``start`` (S, kmax + 1),
    ``kept_offsets`` (S + 1,), ``status`` and, with permutations, ``table`` (the uint16 tables as int16); on the host
    ``offsets``, ``k``, ``n_perms``.  The one read-back is the status."""
    off, rows, kw = check_graph(graph)
    P = check_int(n_perms, "n_perms", 0, MAX_PERMS)
    seed = check_int(seed, "seed", 0, 2 ** 64 - 1)
    kk = check_labels(labels, rows, off, k)
    S, kmax = int(off.size - 1), int(kk.max())
    check_cells(S, kmax, 1, "nhood")
    host_table = None
    if permutations is not None:
        if isinstance(labels, Tensor):
            raise ValueError("permutations: replaying tables needs host labels (the kept spots per slide size them)")
        host_table = spatial.check_permutations(permutations, kept_sizes(labels, off))
        P = len(permutations[0])
    dev = device("nhood")
    nbr, w = graph["nbr"], graph["w"]
    nbr_d = nbr.to(dev).contiguous() if isinstance(nbr, Tensor) else upload(np.asarray(nbr).astype(np.int32), dev)
    w_d = w.to(dev).contiguous() if isinstance(w, Tensor) else upload(np.asarray(w, dtype=np.float64), dev)
    prep = _prepare(labels, rows, off, kk, dev)
    e = empty(dev)
    max_n = prep["max_n"]
    work = e((int(call("mcl_nhood_workspace_bytes", rows, kw)) // 8 + 1,), torch.float64)
    count = e((S, kmax, kmax), torch.int32)
    out = {"count": count, "order": prep["order"], "start": prep["start"], "kept_offsets": prep["kept_offsets"],
           "status": prep["status"], "offsets": off, "k": kk, "n_perms": P}
    table_work = stats = None
    if P:
        table_work = e((int(call("mcl_spatial_workspace_bytes", rows, 0, P)) // 8 + 1,), torch.float64)
        table = table_work.view(torch.int16)[:P * rows]
        if host_table is None:
            call("mcl_spatial_permutations", prep["kept_offsets"], S, rows, max_n, P, seed, table_work)
        elif host_table.size:
            table[:host_table.size].copy_(torch.from_numpy(host_table))
        stats = e((S, 4, kmax, kmax), torch.int64)
        out.update({"stats": stats, "table": table, "workspace": table_work})
    call("mcl_nhood_counts", prep["offsets_device"], prep["kept_offsets"], prep["order"], prep["start"], prep["k_device"], S,
         rows, max_n, kmax, nbr_d, w_d, kw, table_work, P, work, count, stats, prep["status"])
    _raise_status(prep["status"])
    return out


def _slides(d: Dict[str, object], keys: Sequence[str]):
    host = {key: d[key].cpu().numpy() for key in keys}
    off, kk = d["offsets"], d["k"]
    for s in range(off.size - 1):
        K = int(kk[s])
        start = host["start"][s, :K + 1]
        yield s, K, np.diff(start).astype(np.int64), int(start[K]), host


def nhood_enrichment(labels, graph: Dict[str, object], k=None, n_perms: int = 1000, seed: int = 0,
                     permutations=None) -> List[Dict[str, object]]:
    """Which groups sit next to which on the graph more often than under permuted labels.

    ``labels``: (rows,) integers, within slide s in [0, k[s]), -1 = dropped; host or device int32 (then ``k`` is needed).
    ``graph``: what ``spatial.lattice`` returns (or a dict of ``nbr`` (rows, kw) slide-local indices, ``w`` (rows, kw), 0 =
    pruned, and ``offsets``).  ``n_perms`` permutations are generated from ``seed`` or replayed from ``permutations`` (one
    (P, n kept) integer array per slide).  Returns one dict per slide: ``count`` (K, K) int64 and, with permutations,
    ``zscore``, ``perm_mean``, ``perm_std``, ``pval_enriched``, ``pval_depleted`` (K, K) fp64, ``n_ge``, ``n_le`` (int64);
    always ``sizes`` (K,), ``n``, ``k``, ``n_perms``."""
    d = nhood_device(labels, graph, k, n_perms, seed, permutations)
    P = int(d["n_perms"])
    out = []
    for s, K, sizes, n, host in _slides(d, ("count", "start") + (("stats",) if P else ())):
        one = {"count": host["count"][s, :K, :K].astype(np.int64), "sizes": sizes, "n": n, "k": K, "n_perms": P}
        if P:
            S1, S2, n_ge, n_le = (host["stats"][s, q, :K, :K].copy() for q in range(4))
            z, mean, std = zscore(one["count"], S1, S2, P)
            one.update({"zscore": z, "perm_mean": mean, "perm_std": std, "perm_sum": S1, "perm_sumsq": S2, "n_ge": n_ge,
                        "n_le": n_le, "pval_enriched": n_ge / float(P), "pval_depleted": n_le / float(P)})
        out.append(one)
    return out


def interaction_matrix(labels, graph: Dict[str, object], k=None, normalized: bool = False) -> List[np.ndarray]:
    """``count`` of every slide; ``normalized``: every row divided by its sum (NaN where that is 0)."""
    check_flag(normalized, "normalized")
    res = nhood_enrichment(labels, graph, k, n_perms=0)
    if not normalized:
        return [r["count"] for r in res]
    out = []
    for r in res:
        c = r["count"].astype(np.float64)
        tot = c.sum(axis=1, keepdims=True)
        with np.errstate(all="ignore"):
            out.append(np.where(tot == 0.0, np.nan, c / tot))
    return out


def _coords(coords: ArrayLike, dev: Optional[torch.device]):
    """(host fp64 array or None, device fp64 tensor or None) of (rows, 2) coordinates, converted as ``lattice`` does."""
    if isinstance(coords, Tensor):
        if coords.dim() != 2 or coords.shape[1] != 2:
            raise ValueError(f"coords: expected a (rows, 2) array, got shape {tuple(coords.shape)}")
        if coords.is_cuda:
            if coords.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"coords: device tensors must be float32 or float64, got {coords.dtype}")
            if dev is None:
                return None, coords
            out = torch.empty(tuple(coords.shape), device=dev, dtype=torch.float64)
            out.copy_(coords)
            return None, out
        coords = coords.numpy()
    c = np.asarray(coords)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError(f"coords: expected a (rows, 2) array, got shape {c.shape}")
    if not (np.issubdtype(c.dtype, np.integer) or np.issubdtype(c.dtype, np.floating)) or c.dtype == np.bool_:
        raise ValueError(f"coords: expected numbers, got dtype {c.dtype}")
    return np.ascontiguousarray(c.astype(np.float64)), None


def co_occurrence(coords: ArrayLike, labels, offsets: Optional[Sequence[int]] = None, k=None,
                  radii=DEFAULT_RADII) -> List[Dict[str, object]]:
    """How the chance of meeting group c2 changes within a radius of group c1.

    ``coords``: row-stacked (rows, 2), fp32 / fp64 on host or device, or host integers.  ``labels``, ``k`` as for
    ``nhood_enrichment``; ``offsets``: the S + 1 slide boundaries (default: one slide).  ``radii``: an increasing array shared
    by all slides, or their number T (per slide ``linspace(R / T, R, T)``, R half the bounding-box diagonal of its kept
    spots).  Returns one dict per slide: ``pairs`` (T, K, K) int64, ``occ`` (T, K, K) fp64, ``radii`` (T,), ``sizes``, ``n``,
    ``k``."""
    shape = tuple(coords.shape) if hasattr(coords, "shape") else np.asarray(coords).shape
    if len(shape) != 2 or int(shape[1]) != 2:
        raise ValueError(f"coords: expected a (rows, 2) array, got shape {tuple(shape)}")
    rows = int(shape[0])
    off = validate_offsets(offsets, rows, min_rows=2, max_rows=MAX_ROWS, max_segments=MAX_SLIDES, none_is_one=True,
                           noun="slide")
    S = int(off.size - 1)
    kk = check_labels(labels, rows, off, k)
    kmax = int(kk.max())
    host_c, dev_c = _coords(coords, None)
    if host_c is not None:
        for s in range(S):
            if not np.isfinite(host_c[off[s]:off[s + 1]]).all():
                raise ValueError(f"coords: slide {s} holds non-finite coordinates")
    if isinstance(radii, (int, np.integer)) and not isinstance(radii, (bool, np.bool_)):
        T = check_int(radii, "radii", 1, MAX_RADII)
        check_cells(S, kmax, T, "co_occurrence")
        c = host_c if host_c is not None else dev_c.cpu().numpy().astype(np.float64)
        lab = labels.cpu().numpy() if isinstance(labels, Tensor) else np.asarray(labels)
        if not np.isfinite(c).all():
            bad = int(np.flatnonzero([not np.isfinite(c[off[s]:off[s + 1]]).all() for s in range(S)])[0])
            raise ValueError(f"coords: slide {bad} holds non-finite coordinates")
        rad = np.stack([default_radii(c[off[s]:off[s + 1]][lab[off[s]:off[s + 1]] >= 0], T) for s in range(S)])
    else:
        r = check_radii(radii)
        T = int(r.size)
        check_cells(S, kmax, T, "co_occurrence")
        rad = np.broadcast_to(r, (S, T)).copy()
    dev = device("nhood")
    c_d = upload(host_c, dev) if host_c is not None else _coords(dev_c, dev)[1]
    prep = _prepare(labels, rows, off, kk, dev)
    e = empty(dev)
    work = e((int(call("mcl_cooccur_workspace_bytes", rows)) // 8 + 1,), torch.float64)
    r2_d = upload(rad * rad, dev)                               # r_t r_t, rounded once
    pairs, occ = e((S, T, kmax, kmax), torch.int32), e((S, T, kmax, kmax), torch.float64)
    call("mcl_cooccur_counts", c_d, prep["offsets_device"], prep["order"], prep["start"], prep["k_device"], S, rows,
         prep["max_n"], kmax, r2_d, T, work, pairs, prep["status"])
    call("mcl_cooccur_scores", prep["k_device"], S, kmax, T, pairs, occ)
    _raise_status(prep["status"])
    d = {"pairs": pairs, "occ": occ, "start": prep["start"], "offsets": off, "k": kk}
    return [{"pairs": host["pairs"][s, :, :K, :K].astype(np.int64), "occ": host["occ"][s, :, :K, :K].copy(),
             "radii": rad[s].copy(), "sizes": sizes, "n": n, "k": K}
            for s, K, sizes, n, host in _slides(d, ("pairs", "occ", "start"))]


def arrangement_slides(annotations: Sequence[Sequence], coords: Sequence[ArrayLike], k_graph: int = 8, prune: str = "NA",
                       n_perms: int = 1000, seed: int = 0, radii=DEFAULT_RADII,
                       undetermined="undetermined") -> List[Dict[str, object]]:
    """Neighbourhood enrichment and co-occurrence of one label vector and one (spots, 2) coordinate array per slide, on
    the lattice ``spatial.lattice(coords, k=k_graph, prune=prune)``.  String labels are encoded as ``markers.encode_slides``
    does (sorted distinct values; ``undetermined`` becomes -1).  Every slide's dict holds what ``nhood_enrichment`` and
    ``co_occurrence`` return, and ``categories``, the label of each group."""
    if len(annotations) != len(coords) or not len(coords):
        raise ValueError(f"need one label vector per slide and >= 1 slide; got {len(coords)} coords and {len(annotations)}")
    cs = []
    for i, (c, lab) in enumerate(zip(coords, annotations)):
        c = c.cpu().numpy() if isinstance(c, Tensor) else np.asarray(c)
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] != len(lab):
            raise ValueError(f"slide {i}: coords {c.shape} and {len(lab)} labels do not match")
        cs.append(c.astype(np.float64))
    codes, ks, cats = markers.encode_slides(annotations, undetermined)
    off = cumulative_offsets([c.shape[0] for c in cs])
    stacked = np.concatenate(cs)
    check_labels(codes, int(off[-1]), off, ks)
    graph = spatial.lattice(stacked, off, k=k_graph, prune=prune)
    nh = nhood_enrichment(codes, graph, ks, n_perms, seed)
    cc = co_occurrence(stacked, codes, off, ks, radii)
    out = []
    for a, b, c in zip(nh, cc, cats):
        one = dict(a)
        one.update({"pairs": b["pairs"], "occ": b["occ"], "radii": b["radii"], "categories": c})
        out.append(one)
    return out


# --------------------------------------------------------------------------------------------------------- recovery
def top_pairs(res: Sequence[Dict[str, object]], slide: int, n: int = TOP_N) -> np.ndarray:
    """(c1, c2) of the ``n`` largest |z| of one slide (fewer when fewer are finite): ties by index."""
    z = res[slide]["zscore"]
    flat = np.flatnonzero(np.isfinite(z.ravel()))
    keys = np.lexsort((flat, -np.abs(z.ravel()[flat])))
    pick = flat[keys[:max(0, int(n))]]
    return np.stack(np.unravel_index(pick, z.shape), axis=1).astype(np.int64) if pick.size else np.zeros((0, 2), np.int64)


def contingency(pred: np.ndarray, true: np.ndarray, kp: int, kt: int) -> np.ndarray:
    """table[p, t] = the spots with predicted group p and measured group t (both >= 0)."""
    ok = (pred >= 0) & (true >= 0)
    table = np.zeros((kp, kt), dtype=np.int64)
    np.add.at(table, (pred[ok], true[ok]), 1)
    return table


def recovery_scores(rp: Dict[str, object], rt: Dict[str, object], match: np.ndarray) -> Dict[str, float]:
    """``pearson_z``, ``sign_agreement`` and ``pearson_occ`` of two slides' results over the matched groups."""
    nan = float("nan")
    if match.shape[0] == 0:
        return {"pearson_z": nan, "sign_agreement": nan, "pearson_occ": nan, "n_cells": 0}
    p, t = match[:, 0], match[:, 1]
    zp, zt = rp["zscore"][np.ix_(p, p)], rt["zscore"][np.ix_(t, t)]
    ok = np.isfinite(zp) & np.isfinite(zt)
    sign = float((np.sign(zp[ok]) == np.sign(zt[ok])).mean()) if ok.any() else nan
    with np.errstate(all="ignore"):
        op, ot = np.log2(rp["occ"][:, p][:, :, p]), np.log2(rt["occ"][:, t][:, :, t])
    occ = spatial.pearson(op, ot) if op.shape == ot.shape else nan
    return {"pearson_z": spatial.pearson(zp, zt), "sign_agreement": sign, "pearson_occ": occ, "n_cells": int(ok.sum())}


def arrangement_recovery(pred_labels: Sequence[Sequence], true_labels: Sequence[Sequence], coords: Sequence[ArrayLike],
                         **kw) -> Dict[str, object]:
    """Are the predicted domains arranged in the tissue the way the measured ones are?  Both label sets are analysed on
    the same spots, lattice and permutations (``arrangement_slides``; a shared explicit ``radii=`` compares the same
    distances).  Per slide the groups are matched greedily on the contingency table (``greedy_match``: largest cell first,
    ties to the smaller (row, column); unmatched groups are left out), then over the matched cells that are finite on both
    sides: ``pearson_z``, ``sign_agreement`` (the share of cells whose z has the same sign) and ``pearson_occ`` (over log2
    occ of all radii).  Also ``matching`` (one (m, 2) array of (predicted, measured) group per slide), ``n_cells``, the
    ``mean_*`` of each score and the two results ``pred`` / ``true``."""
    if len(pred_labels) != len(true_labels) or len(pred_labels) != len(coords):
        raise ValueError(f"need one predicted and one measured label vector per slide; got {len(pred_labels)}, "
                         f"{len(true_labels)} and {len(coords)} coords")
    for i, (a, b) in enumerate(zip(pred_labels, true_labels)):
        if len(a) != len(b):
            raise ValueError(f"slide {i}: {len(a)} predicted and {len(b)} measured labels")
    if kw.get("n_perms", 1000) == 0:
        raise ValueError("arrangement_recovery compares z-scores: n_perms must be >= 1")
    und = kw.get("undetermined", "undetermined")
    rp = arrangement_slides(pred_labels, coords, **kw)
    rt = arrangement_slides(true_labels, coords, **kw)
    cp, _, _ = markers.encode_slides(pred_labels, und)
    ct, _, _ = markers.encode_slides(true_labels, und)
    off = cumulative_offsets([len(a) for a in pred_labels])
    cols = {key: [] for key in ("pearson_z", "sign_agreement", "pearson_occ", "n_cells")}
    matching = []
    for s, (a, b) in enumerate(zip(rp, rt)):
        table = contingency(cp[off[s]:off[s + 1]], ct[off[s]:off[s + 1]], a["k"], b["k"])
        match = greedy_match(table)
        matching.append(match)
        for key, v in recovery_scores(a, b, match).items():
            cols[key].append(v)
    out = {key: np.asarray(v) for key, v in cols.items()}
    out.update({f"mean_{key}": nanmean(out[key]) for key in ("pearson_z", "sign_agreement", "pearson_occ")})
    out.update({"matching": matching, "pred": rp, "true": rt})
    return out


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.nhood",
                                description="Neighbourhood enrichment and co-occurrence of spot groups (squidpy.gr."
                                            "nhood_enrichment / co_occurrence) and how well predicted domains recover the "
                                            "arrangement of the measured ones")
    p.add_argument("--labels", required=True, nargs="+",
                   help="one label vector per slide: leiden.npy as the Leiden CLI writes it, or an annotation array")
    p.add_argument("--coords", required=True, nargs="+", help="one (N, 2) coordinate array per slide, in slide order")
    p.add_argument("--true_labels", default=None, nargs="+", help="the measured labels: also print the recovery line")
    p.add_argument("--k", type=int, default=8, help="neighbours per spot of the lattice")
    p.add_argument("--prune", default="NA", choices=sorted(spatial.PRUNES))
    p.add_argument("--n_perms", type=int, default=1000)
    p.add_argument("--radii", type=int, default=DEFAULT_RADII, help="radii per slide")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--top", type=int, default=TOP_N, help="group pairs to print per slide and direction")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if len(a.coords) != len(a.labels):
        p.error(f"{len(a.coords)} --coords files for {len(a.labels)} --labels files")
    if a.true_labels is not None and len(a.true_labels) != len(a.labels):
        p.error(f"{len(a.true_labels)} --true_labels files for {len(a.labels)} --labels files")
    if a.k < 1 or a.k > spatial.MAX_K:
        p.error(f"--k must lie in 1 .. {spatial.MAX_K}")
    if a.n_perms < 1 or a.n_perms > MAX_PERMS:
        p.error(f"--n_perms must lie in 1 .. {MAX_PERMS}")
    if a.radii < 1 or a.radii > MAX_RADII:
        p.error(f"--radii must lie in 1 .. {MAX_RADII}")
    if a.seed < 0:
        p.error("--seed must be >= 0")
    if a.top < 1:
        p.error("--top must be >= 1")
    return a


def format_slides(res: Sequence[Dict[str, object]], top: int) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        cats, z = r["categories"], r["zscore"]
        flat = np.flatnonzero(np.isfinite(z.ravel()))
        lines.append(f"slide {s} n = {r['n']} k = {r['k']} perms = {r['n_perms']}")
        for name, keys in (("enriched", np.lexsort((flat, -z.ravel()[flat]))), ("depleted", np.lexsort((flat, z.ravel()[flat])))):
            cells = []
            for e in flat[keys[:top]]:
                c1, c2 = divmod(int(e), z.shape[1])
                p = r["pval_enriched" if name == "enriched" else "pval_depleted"][c1, c2]
                cells.append(f"{cats[c1]}->{cats[c2]} (z {z[c1, c2]:.3f}, count {int(r['count'][c1, c2])}, p {p:.4f})")
            lines.append(f"  most {name}: " + (", ".join(cells) or "nothing defined"))
    return lines


def format_recovery(rec: Dict[str, object]) -> List[str]:
    lines = [f"slide {s}: {len(rec['matching'][s])} groups matched, Pearson z {rec['pearson_z'][s]:.4f}, sign agreement "
             f"{rec['sign_agreement'][s]:.4f}, Pearson log2 occ {rec['pearson_occ'][s]:.4f}" for s in range(len(rec["pearson_z"]))]
    lines.append(f"recovery: mean Pearson z {rec['mean_pearson_z']:.4f}, mean sign agreement {rec['mean_sign_agreement']:.4f}, "
                 f"mean Pearson log2 occ {rec['mean_pearson_occ']:.4f}")
    return lines


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    labels = [np.load(f, allow_pickle=True).reshape(-1) for f in args.labels]
    coords = [np.load(f) for f in args.coords]
    kw = dict(k_graph=args.k, prune=args.prune, n_perms=args.n_perms, seed=args.seed, radii=args.radii)
    if args.true_labels is not None:
        trues = [np.load(f, allow_pickle=True).reshape(-1) for f in args.true_labels]
        rec = arrangement_recovery(labels, trues, coords, **kw)
        res = rec["pred"]
    else:
        rec, res = None, arrangement_slides(labels, coords, **kw)
    print("\n".join(format_slides(res, args.top)))
    if args.out_dir is not None:
        for i, r in enumerate(res):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, OUT_FILE), **{key: np.asarray(v) for key, v in r.items()})
    if rec is not None:
        print("\n".join(format_recovery(rec)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
