"""Ligand-receptor permutation test on the MI355X: what ``squidpy.gr.ligrec`` (the CellPhoneDB test) computes from an
expression matrix and group labels -- for every interaction (ligand gene, receptor gene) and every ordered pair of groups
the mean of the two group means, and how often it is reached when the labels are permuted -- for all slides of an
evaluation per call, and the number the feature exists for: do predicted expression values call the same interactions
between the same domains as the measured ones (``interaction_recovery``)?  The groups are whatever labels a slide carries:
``cluster`` / ``mixture`` / ``hmrf`` domains, ``leiden`` communities or the pathologist's annotation.

What is computed is stated in DESIGN 6.19 and restated in numpy by ``tests/ligrec_reference.py``, which is pinned to a
pandas ``groupby`` statement and to ``scipy.stats.false_discovery_control``.  No interaction database is shipped or
fetched: the user supplies the pairs (``resolve_pairs`` turns gene names into columns).  squidpy, omnipath and CellPhoneDB
are not installed: parity with a release of any of them is unpinned.  Things to know:

* Spots labelled -1 are dropped from everything, exactly as if the slide had been subset first.
* ``means[i, c1, c2]`` = (mean of gene a_i in group c1 + mean of gene b_i in group c2) / 2 where both are > 0, else 0.
  ``pvalues`` = count / n_perms, count = #((m1' + m2') / 2 >= (m1 + m2) / 2) over the permutations (``>=``, nothing is added
  to numerator or denominator, so p may be 0); NaN where a mean is not > 0 or a gene is expressed (> 0) in fewer than
  ``threshold`` of the spots of its group.  An empty group (``k`` larger than the labels used) gives NaN means.
* Permutation p of a slide of n kept spots is ``mcl_spatial_permutations``' pure function of (seed, p, n): group c receives
  the spots at positions start_c .. end_c of the permuted (label, spot)-sorted order.  The observed values come from the
  same kernel and summation order with the identity permutation.
* ``pvalues_adj`` is Benjamini-Hochberg over the finite p-values along ``corr_axis``: ``"clusters"`` (per interaction over
  the group pairs, squidpy's default), ``"interactions"`` (per group pair) or None (off).  It runs on the host.
* A side of an interaction may be a tuple of gene columns (a complex): ``complex_policy="min"`` takes, per slide, the member
  of lowest mean over the kept spots (ties: the smaller column), ``"all"`` expands the product.
* 2 <= n_s <= 16384 spots per slide, k <= 255 groups, G <= 16384 genes, n_perms <= 65535, at most 65535 interactions,
  I k^2 <= 2^24 per slide and S I k^2 < 2^31: ``ValueError`` before a launch.  The kept spots of a slide may number 0 or 1
  (NaN means and nothing defined; the identity as the only permutation).  A label outside [-1, k), a non-finite or a
  negative value is counted on the device and raises ``ValueError`` at the one synchronisation.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible run to run; a slide inside a batch
is bit-identical to the same slide alone.  No CPU fallback: without a GPU / the HIP library these functions raise
``RuntimeError``.

    python -m mclstexp_amd.ligrec --pred P1.npy ... --labels L1.npy ... --pairs pairs.tsv --genes names.npy
                                  [--true T1.npy ...] [--n_perms 1000] [--threshold 0.1] [--seed 0] [--alpha 0.05]
                                  [--top 10] [--out_dir D]
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import markers, spatial
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_flag, check_int, cumulative_offsets, device, empty,
                      load_gene_major, matrix, nanmean, stack_rows, upload)
from ._lib import call

MAX_ROWS = 16384         # csrc/ligrec.hip: the uint16 permutation tables of csrc/spatial.hip
MAX_GROUPS = 255
MAX_GENES = 16384
MAX_SLIDES = 32767
MAX_PERMS = 65535
MAX_INTERACTIONS = 65535
MAX_CELLS = 1 << 24      # I * k^2 per slide
MAX_TOTAL = (1 << 31) - 1
CORR_AXES = ("clusters", "interactions", None)
POLICIES = ("min", "all")
OUT_FILE = "ligrec.npz"
TOP_N = 10
_ALL_COLUMNS = (1 << 1) | (1 << 2) | (1 << 4) | (1 << 8)


# ------------------------------------------------------------------------------------------------------- host rules
def _side(v, G: int, what: str) -> tuple:
    members = tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else (v,)
    if not members:
        raise ValueError(f"{what}: an empty complex")
    out = []
    for m in members:
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 0 or m >= G:
            raise ValueError(f"{what}: expected gene columns in 0 .. {G - 1}, got {m!r}")
        out.append(int(m))
    return tuple(sorted(set(out)))


def prepare_interactions(interactions, G: int, complex_policy: str = "min"):
    """Index preparation on the host.  ``interactions``: a sequence of (source, target), each a gene column or a tuple of
    columns (a complex).  Returns (sides, used, member_offsets, members): ``sides`` the I (source columns, target columns)
    after the policy (``"all"``: the product, one column a side), ``used`` the ascending distinct columns, and per side
    the positions of its columns in ``used`` (``members[member_offsets[2 i + t]:member_offsets[2 i + t + 1]]``)."""
    if complex_policy not in POLICIES:
        raise ValueError(f"complex_policy must be one of {list(POLICIES)}, got {complex_policy!r}")
    try:
        rows = [tuple(r) for r in interactions]
    except TypeError:
        raise ValueError("interactions: expected a sequence of (source, target) pairs") from None
    if not rows or any(len(r) != 2 for r in rows):
        raise ValueError("interactions: expected at least one (source, target) pair")
    sides = []
    for i, (a, b) in enumerate(rows):
        sa, sb = _side(a, G, f"interactions[{i}] source"), _side(b, G, f"interactions[{i}] target")
        if complex_policy == "all":
            sides.extend(((u,), (v,)) for u, v in itertools.product(sa, sb))
        else:
            sides.append((sa, sb))
    if len(sides) > MAX_INTERACTIONS:
        raise ValueError(f"at most {MAX_INTERACTIONS} interactions per call, got {len(sides)}")
    used = np.unique(np.fromiter((g for s in sides for t in s for g in t), dtype=np.int64)).astype(np.int32)
    moff, members = [0], []
    for s in sides:
        for t in s:
            members.extend(np.searchsorted(used, t).tolist())
            moff.append(len(members))
    return sides, used, np.asarray(moff, dtype=np.int32), np.asarray(members, dtype=np.int32)


def check_options(n_perms, seed, threshold, corr_axis, return_permutations=False):
    P = check_int(n_perms, "n_perms", 0, MAX_PERMS)
    seed = check_int(seed, "seed", 0, 2 ** 64 - 1)
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(threshold) <= 1.0:
        raise ValueError(f"threshold must be a number in 0 .. 1, got {threshold!r}")
    if corr_axis not in CORR_AXES:
        raise ValueError(f"corr_axis must be one of {list(CORR_AXES)}, got {corr_axis!r}")
    check_flag(return_permutations, "return_permutations")
    return P, seed, float(threshold)


def check_problem(shape: Sequence[int], offsets, k, labels, n_interactions: int):
    """The limits, checked on the host before the GPU is touched.  Returns (offsets int64, k int32)."""
    off, kk = markers.check_problem(shape, offsets, k, labels)
    if off.size - 1 > MAX_SLIDES:
        raise ValueError(f"at most {MAX_SLIDES} slides per call")
    cells = int(n_interactions) * int(kk.max()) ** 2
    if cells > MAX_CELLS or cells * (off.size - 1) > MAX_TOTAL:
        raise ValueError(f"interactions x k^2 = {cells} per slide: at most {MAX_CELLS}, and {MAX_TOTAL} over all slides")
    return off, kk


def kept_sizes(labels, offsets: np.ndarray) -> np.ndarray:
    lab = np.asarray(labels)
    return np.array([int((lab[offsets[s]:offsets[s + 1]] >= 0).sum()) for s in range(offsets.size - 1)], dtype=np.int64)


def bh(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg over the finite entries of a vector (``scipy.stats.false_discovery_control``); NaN stays NaN."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    ok = np.flatnonzero(np.isfinite(p))
    if ok.size:
        q = p[ok]
        order = np.argsort(q, kind="stable")
        scaled = q[order] * (float(ok.size) / np.arange(1, ok.size + 1).astype(np.float64))
        adj = np.empty(ok.size)
        adj[order] = np.minimum(1.0, np.minimum.accumulate(scaled[::-1])[::-1])
        out[ok] = adj
    return out


def adjust(pvalues: np.ndarray, corr_axis) -> np.ndarray:
    """``pvalues`` (I, K, K) -> ``pvalues_adj``: BH per interaction (``"clusters"``), per group pair (``"interactions"``)."""
    I, K = pvalues.shape[0], pvalues.shape[1]
    if corr_axis is None:
        return np.full(pvalues.shape, np.nan)
    flat = pvalues.reshape(I, K * K)
    if corr_axis == "clusters":
        return np.stack([bh(r) for r in flat]).reshape(pvalues.shape) if I else pvalues.copy()
    return np.stack([bh(c) for c in flat.T], axis=1).reshape(pvalues.shape) if K else pvalues.copy()


# ----------------------------------------------------------------------------------------------------------- device
def ligrec_device(x: ArrayLike, labels, interactions, offsets: Optional[Sequence[int]] = None, k=None, n_perms: int = 1000,
                  seed: int = 0, threshold: float = 0.1, permutations=None, complex_policy: str = "min") -> Dict[str, object]:
    """``ligrec`` with everything left on the device, stacked over the slides with the largest k as the group stride:
    ``means`` (S, I, kmax, kmax) fp64, ``defined`` and ``count`` (int32) of that shape, ``pairs`` (S, I, 2) (positions in
    ``used`` of the two genes taken), ``sum``, ``group_means``, ``group_frac`` (S, kmax, U) fp64, ``nnz`` (int32), ``order``
    (rows,), ``start`` (S, kmax + 1), ``kept_offsets`` (S + 1,), ``status`` and, with permutations, ``table`` (the uint16
    tables as int16); on the host ``offsets``, ``k``, ``used``, ``sides``, ``n_perms``.  The one read-back is the status."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    if len(shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(shape)}")
    sides, used, moff, members = prepare_interactions(interactions, int(shape[1]), complex_policy)
    P, seed, threshold = check_options(n_perms, seed, threshold, "clusters")
    off, kk = check_problem(shape, offsets, k, labels, len(sides))
    rows, G = int(shape[0]), int(shape[1])
    sizes = np.diff(off)
    host_labels = not isinstance(labels, Tensor)
    host_table = None
    if permutations is not None:
        if not host_labels:
            raise ValueError("permutations: replaying tables needs host labels (the kept spots per slide size them)")
        host_table = spatial.check_permutations(permutations, kept_sizes(labels, off))
        P = len(permutations[0])
    dev = device("ligrec")
    xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
    lab_d = markers.device_labels(labels, rows, dev)
    S, max_n, kmax, U, I = int(sizes.size), int(sizes.max()), int(kk.max()), int(used.size), len(sides)
    mask = _ALL_COLUMNS
    if host_labels:
        mask = 0
        for n in np.unique(kept_sizes(labels, off)):
            mask |= 1 << int(call("mcl_ligrec_columns", int(n)))
    code, ld = FLOAT_CODE[xd.dtype], int(xd.stride(0))
    e = empty(dev)
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    off_d, k_d, used_d = upload(off, dev), upload(kk, dev), upload(used, dev)
    moff_d, mem_d = upload(moff, dev), upload(members, dev)
    order, start, koff, status = e((rows,), i32), e((S, kmax + 1), i32), e((S + 1,), i64), e((S, 4), i32)
    call("mcl_ligrec_prepare", off_d, lab_d, k_d, S, rows, max_n, kmax, order, start, koff, status)
    gsum, gmean, gfrac, nnz = e((S, kmax, U), f64), e((S, kmax, U), f64), e((S, kmax, U), f64), e((S, kmax, U), i32)
    call("mcl_ligrec_group_means", xd, ld, code, off_d, koff, order, start, k_d, S, rows, G, max_n, kmax, used_d, U, mask,
         None, 1, 0, 1, 1, gsum, nnz, gmean, gfrac, None, status)
    pairs = e((S, I, 2), i32)
    means, defined, count = e((S, I, kmax, kmax), f64), e((S, I, kmax, kmax), i32), e((S, I, kmax, kmax), i32)
    call("mcl_ligrec_observed", S, I, kmax, U, k_d, start, gsum, nnz, gmean, moff_d, mem_d, threshold, pairs, means,
         defined, count)
    out = {"means": means, "defined": defined, "count": count, "pairs": pairs, "sum": gsum, "nnz": nnz, "group_means": gmean,
           "group_frac": gfrac, "order": order, "start": start, "kept_offsets": koff, "status": status, "offsets": off,
           "k": kk, "used": used, "sides": sides, "n_perms": P, "threshold": threshold}
    if P:
        work = e((int(call("mcl_spatial_workspace_bytes", rows, 0, P)) // 8 + 1,), f64)
        table = work.view(torch.int16)[:P * rows]
        if host_table is None:
            call("mcl_spatial_permutations", koff, S, rows, max_n, P, seed, work)
        elif host_table.size:
            table[:host_table.size].copy_(torch.from_numpy(host_table))
        chunk = int(call("mcl_ligrec_chunk", S, kmax, U, P))
        pm = e((int(call("mcl_ligrec_workspace_bytes", S, kmax, U, P)) // 8 + 1,), f64)
        for p0 in range(0, P, chunk):                          # enqueued back to back: nothing synchronises in between
            pc = min(chunk, P - p0)
            call("mcl_ligrec_group_means", xd, ld, code, off_d, koff, order, start, k_d, S, rows, G, max_n, kmax, used_d, U,
                 mask, work, P, p0, pc, chunk, None, None, None, None, pm, status)
            call("mcl_ligrec_count", S, I, kmax, U, k_d, gmean, pairs, pm, chunk, pc, count)
        out.update({"table": table, "workspace": work, "chunk": chunk})
    bad = status.cpu().numpy()                                  # the one synchronisation
    for col, what in ((0, "offsets or a group count the device refuses"), (1, "group ids outside -1 .. k - 1"),
                      (2, "non-finite values"), (3, "negative values")):
        if bad[:, col].any():
            s = int(np.flatnonzero(bad[:, col])[0])
            name = "labels" if col == 1 else "x"
            raise ValueError(f"{name}: slide {s} holds {int(bad[s, col])} {what}" if col else f"slide {s}: {what}")
    return out


def ligrec(x: ArrayLike, labels, interactions, offsets: Optional[Sequence[int]] = None, k=None, n_perms: int = 1000,
           seed: int = 0, threshold: float = 0.1, permutations=None, corr_axis="clusters", complex_policy: str = "min",
           return_permutations: bool = False) -> List[Dict[str, object]]:
    """The permutation test of every interaction between every ordered pair of groups of every slide.

    ``x``: row-stacked (rows, G), float32 or float64, host or device, a row stride allowed, values >= 0.  ``labels``: (rows,)
    integers, within slide s in [0, k[s]), -1 = dropped.  ``interactions``: (source, target) gene columns, a side possibly a
    tuple (a complex).  ``offsets``: the S + 1 slide boundaries (default: one slide).  ``k``: groups per slide (default: the
    largest label + 1).  ``n_perms`` permutations are generated from ``seed`` or replayed from ``permutations`` (one
    (P, n kept) integer array per slide).  Returns one dict per slide: ``means``, ``pvalues``, ``pvalues_adj`` (I, K, K),
    ``defined`` (bool), ``count`` (int32), ``group_means``, ``group_frac``, ``nnz``, ``expressed`` (K, U), ``sizes`` (K,),
    ``order`` (n,), ``used_genes`` (U,), ``interactions`` (I, 2: the gene columns taken), ``n``, ``k``, ``n_perms`` (and
    ``permutations`` (P, n) with ``return_permutations``)."""
    check_options(n_perms, seed, threshold, corr_axis, return_permutations)
    d = ligrec_device(x, labels, interactions, offsets, k, n_perms, seed, threshold, permutations, complex_policy)
    P, off, kk, used = int(d["n_perms"]), d["offsets"], d["k"], d["used"]
    host = {key: d[key].cpu().numpy() for key in ("means", "defined", "count", "pairs", "nnz", "group_means", "group_frac",
                                                  "order", "start", "kept_offsets")}
    table = d["table"].cpu().numpy() if P and return_permutations else None
    out = []
    for s in range(off.size - 1):
        K = int(kk[s])
        start = host["start"][s, :K + 1]
        sizes, n = np.diff(start).astype(np.int64), int(start[K])
        defined = host["defined"][s, :, :K, :K] != 0
        count = host["count"][s, :, :K, :K].copy()
        with np.errstate(all="ignore"):
            pvalues = np.where(defined, count / float(P), np.nan) if P else np.full(count.shape, np.nan)
        nnz = host["nnz"][s, :K]
        one = {"means": host["means"][s, :, :K, :K].copy(), "pvalues": pvalues, "pvalues_adj": adjust(pvalues, corr_axis),
               "defined": defined, "count": count, "group_means": host["group_means"][s, :K].copy(),
               "group_frac": host["group_frac"][s, :K].copy(), "nnz": nnz.copy(),
               "expressed": nnz >= d["threshold"] * sizes[:, None].astype(np.float64), "sizes": sizes,
               "order": host["order"][off[s]:off[s] + n].astype(np.int64), "used_genes": used.astype(np.int64),
               "interactions": used[host["pairs"][s]].astype(np.int64), "n": n, "k": K, "n_perms": P}
        if table is not None:
            a = P * int(host["kept_offsets"][s])
            one["permutations"] = table[a:a + P * n].reshape(P, n).astype(np.int64)
        out.append(one)
    return out


def ligrec_slides(matrices: Sequence[ArrayLike], labels: Sequence[Sequence], interactions, undetermined="undetermined",
                  **kw) -> List[Dict[str, object]]:
    """``ligrec`` of one (spots, genes) matrix and one label vector per slide.  String labels are encoded as
    ``markers.encode_slides`` does (sorted distinct values; ``undetermined`` becomes -1); every slide's dict also carries
    ``categories``, the label of each group."""
    if len(matrices) != len(labels) or not len(matrices):
        raise ValueError(f"need one label vector per slide and >= 1 slide; got {len(matrices)} and {len(labels)}")
    for i, (m, lab) in enumerate(zip(matrices, labels)):
        if len(m.shape) != 2 or m.shape[0] != len(lab):
            raise ValueError(f"slide {i}: matrix {tuple(m.shape)} and {len(lab)} labels do not match")
    codes, ks, cats = markers.encode_slides(labels, undetermined)
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    G = int(matrices[0].shape[1])
    sides = prepare_interactions(interactions, G, kw.get("complex_policy", "min"))[0]
    check_problem((int(off[-1]), G), off, ks, None, len(sides))
    check_options(kw.get("n_perms", 1000), kw.get("seed", 0), kw.get("threshold", 0.1), kw.get("corr_axis", "clusters"))
    dev = device("ligrec")
    x, off = stack_rows(matrices, "matrices", dev)
    res = ligrec(x, codes, interactions, off, ks, **kw)
    for r, c in zip(res, cats):
        r["categories"] = c
    return res


# --------------------------------------------------------------------------------------------------------- recovery
def top_interactions(res: Sequence[Dict[str, object]], slide: int, n: int = TOP_N) -> np.ndarray:
    """(i, c1, c2) of the ``n`` smallest p-values of one slide (fewer when fewer are defined): ties by the larger mean,
    then by index."""
    p, m = res[slide]["pvalues"], res[slide]["means"]
    flat = np.flatnonzero(np.isfinite(p.ravel()))
    keys = np.lexsort((flat, -m.ravel()[flat], p.ravel()[flat]))
    pick = flat[keys[:max(0, int(n))]]
    return np.stack(np.unravel_index(pick, p.shape), axis=1).astype(np.int64) if pick.size else np.zeros((0, 3), np.int64)


def significant(r: Dict[str, object], alpha: float, adjusted: bool) -> np.ndarray:
    p = r["pvalues_adj"] if adjusted else r["pvalues"]
    with np.errstate(invalid="ignore"):
        return np.isfinite(p) & (p < alpha)


def interaction_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], labels: Sequence[Sequence], interactions,
                         alpha: float = 0.05, **kw) -> Dict[str, object]:
    """Do the predicted values call the interactions the measured ones call?  Both matrices are tested under the same
    labels, permutations and interactions.  Per slide: ``pearson`` between ``means(pred)`` and ``means(true)`` over the
    entries defined in both, and ``overlap``, ``jaccard``, ``precision``, ``recall`` of the significant sets (``pvalues <
    alpha``, or ``pvalues_adj`` when ``corr_axis`` is set; NaN where a denominator is 0).  Also ``n_pred``, ``n_true``, the
    ``mean_*`` of each, ``alpha`` and the two results ``pred`` / ``true``."""
    if len(preds) != len(trues):
        raise ValueError(f"need one measured matrix per prediction; got {len(preds)} and {len(trues)}")
    for i, (p, t) in enumerate(zip(preds, trues)):
        if tuple(p.shape) != tuple(t.shape):
            raise ValueError(f"slide {i}: pred {tuple(p.shape)} and true {tuple(t.shape)} differ in shape")
    if isinstance(alpha, bool) or not isinstance(alpha, (float, np.floating)) or not 0.0 < alpha <= 1.0:
        raise ValueError(f"alpha must be a float in (0, 1], got {alpha!r}")
    adjusted = kw.get("corr_axis", "clusters") is not None
    rp = ligrec_slides(preds, labels, interactions, **kw)
    rt = ligrec_slides(trues, labels, interactions, **kw)
    cols = {key: [] for key in ("pearson", "overlap", "jaccard", "precision", "recall", "n_pred", "n_true")}
    for a, b in zip(rp, rt):
        both = a["defined"] & b["defined"]
        cols["pearson"].append(spatial.pearson(np.where(both, a["means"], np.nan), np.where(both, b["means"], np.nan)))
        sa, sb = significant(a, alpha, adjusted), significant(b, alpha, adjusted)
        o, u = int((sa & sb).sum()), int((sa | sb).sum())
        cols["overlap"].append(o)
        cols["n_pred"].append(int(sa.sum()))
        cols["n_true"].append(int(sb.sum()))
        cols["jaccard"].append(o / u if u else float("nan"))
        cols["precision"].append(o / int(sa.sum()) if sa.any() else float("nan"))
        cols["recall"].append(o / int(sb.sum()) if sb.any() else float("nan"))
    out = {key: np.asarray(v) for key, v in cols.items()}
    out.update({f"mean_{key}": nanmean(out[key]) for key in ("pearson", "overlap", "jaccard", "precision", "recall")})
    out.update({"alpha": float(alpha), "adjusted": adjusted, "pred": rp, "true": rt})
    return out


# ------------------------------------------------------------------------------------------------------------ names
def resolve_pairs(pairs, gene_names: Sequence[str]) -> Dict[str, object]:
    """Two columns of gene names -> column indices.  A name found in ``gene_names`` is that gene; any other name is read as
    a complex whose members are joined by ``_`` (as CellPhoneDB and squidpy write them).  A pair with a gene outside the
    panel is dropped, and so is a pair that resolves to one already kept.  Returns ``interactions`` (what ``ligrec`` takes:
    an int or a tuple of ints a side), ``names`` (the kept (source, target) names), ``kept`` (their row numbers),
    ``n_missing`` and ``n_duplicates``."""
    index = {}
    for j, g in enumerate(gene_names):
        index.setdefault(str(g), j)

    def one(name):
        name = str(name).strip()
        if name in index:
            return index[name]
        parts = [q for q in name.split("_") if q]
        if len(parts) < 2 or any(q not in index for q in parts):
            return None
        cols = tuple(sorted({index[q] for q in parts}))
        return cols[0] if len(cols) == 1 else cols

    inter, names, kept, seen, missing, dup = [], [], [], set(), 0, 0
    for r, row in enumerate(pairs):
        row = tuple(row)
        if len(row) != 2:
            raise ValueError(f"pairs[{r}]: expected (source, target), got {row!r}")
        a, b = one(row[0]), one(row[1])
        if a is None or b is None:
            missing += 1
        elif (a, b) in seen:
            dup += 1
        else:
            seen.add((a, b))
            inter.append((a, b))
            names.append((str(row[0]).strip(), str(row[1]).strip()))
            kept.append(r)
    return {"interactions": inter, "names": names, "kept": np.asarray(kept, dtype=np.int64), "n_missing": missing,
            "n_duplicates": dup}


def read_pairs(path: str) -> List[tuple]:
    """The (source, target) names of a two-column tab- or comma-separated file; ``#`` lines and a ``source target`` header
    are skipped."""
    rows = []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            cells = [c.strip() for c in (line.split("\t") if "\t" in line else line.split(","))]
            if len(cells) < 2:
                raise ValueError(f"{path}: expected two columns, got {line!r}")
            if not rows and cells[0].lower() in ("source", "ligand") and cells[1].lower() in ("target", "receptor"):
                continue
            rows.append((cells[0], cells[1]))
    return rows


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.ligrec",
                                description="Ligand-receptor permutation test between spot groups (squidpy.gr.ligrec) and how "
                                            "well predictions recover the interactions of the measured matrix")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--labels", required=True, nargs="+",
                   help="one label vector per slide: leiden.npy as the Leiden CLI writes it, or an annotation array")
    p.add_argument("--pairs", required=True, help="two columns of gene names (source, target), tab- or comma-separated")
    p.add_argument("--genes", required=True, help=".npy of the G gene names")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery line")
    p.add_argument("--n_perms", type=int, default=1000)
    p.add_argument("--threshold", type=float, default=0.1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--alpha", type=float, default=0.05)
    p.add_argument("--corr_axis", default="clusters", choices=["clusters", "interactions", "none"])
    p.add_argument("--complex_policy", default="min", choices=list(POLICIES))
    p.add_argument("--top", type=int, default=TOP_N, help="interactions to print per slide")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if len(a.labels) != len(a.pred):
        p.error(f"{len(a.labels)} --labels files for {len(a.pred)} --pred files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.n_perms < 0 or a.n_perms > MAX_PERMS:
        p.error(f"--n_perms must lie in 0 .. {MAX_PERMS}")
    if not 0.0 <= a.threshold <= 1.0:
        p.error("--threshold must lie in 0 .. 1")
    if a.seed < 0:
        p.error("--seed must be >= 0")
    if not 0.0 < a.alpha <= 1.0:
        p.error("--alpha must lie in (0, 1]")
    if a.top < 1:
        p.error("--top must be >= 1")
    a.corr_axis = None if a.corr_axis == "none" else a.corr_axis
    return a


def format_slides(res: Sequence[Dict[str, object]], genes: Sequence[str], top: int) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        cats = r.get("categories", np.arange(r["k"]))
        cells = []
        for i, c1, c2 in top_interactions(res, s, top):
            a, b = r["interactions"][i]
            cells.append(f"{genes[a]}->{genes[b]} {cats[c1]}->{cats[c2]} (p {r['pvalues'][i, c1, c2]:.4f}, mean "
                         f"{r['means'][i, c1, c2]:.4f})")
        lines.append(f"slide {s} n = {r['n']} k = {r['k']} perms = {r['n_perms']}: " + (", ".join(cells) or "nothing defined"))
    return lines


def format_recovery(rec: Dict[str, object]) -> List[str]:
    lines = [f"slide {s}: Pearson {rec['pearson'][s]:.4f}, overlap {int(rec['overlap'][s])} (pred {int(rec['n_pred'][s])}, "
             f"true {int(rec['n_true'][s])}), Jaccard {rec['jaccard'][s]:.4f}, precision {rec['precision'][s]:.4f}, recall "
             f"{rec['recall'][s]:.4f}" for s in range(len(rec["pearson"]))]
    lines.append(f"recovery (alpha {rec['alpha']:g}{', adjusted' if rec['adjusted'] else ''}): mean Pearson "
                 f"{rec['mean_pearson']:.4f}, mean Jaccard {rec['mean_jaccard']:.4f}, mean precision "
                 f"{rec['mean_precision']:.4f}, mean recall {rec['mean_recall']:.4f}")
    return lines


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    labels = [np.load(f, allow_pickle=True).reshape(-1) for f in args.labels]
    G = preds[0].shape[1]
    genes = [str(v) for v in np.load(args.genes, allow_pickle=True).reshape(-1)]
    if len(genes) != G:
        raise ValueError(f"{args.genes}: {len(genes)} gene names for {G} genes")
    resolved = resolve_pairs(read_pairs(args.pairs), genes)
    print(f"{len(resolved['interactions'])} interactions ({resolved['n_missing']} pairs with a gene outside the panel and "
          f"{resolved['n_duplicates']} duplicates dropped)")
    if not resolved["interactions"]:
        raise ValueError(f"{args.pairs}: no pair lies inside the gene panel")
    kw = dict(n_perms=args.n_perms, seed=args.seed, threshold=args.threshold, corr_axis=args.corr_axis,
              complex_policy=args.complex_policy)
    res = ligrec_slides(preds, labels, resolved["interactions"], **kw)
    print("\n".join(format_slides(res, genes, args.top)))
    if args.out_dir is not None:
        for i, r in enumerate(res):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, OUT_FILE), **{key: np.asarray(v) for key, v in r.items()})
    if args.true is not None:
        trues = load_gene_major(args.true)
        print("\n".join(format_recovery(interaction_recovery(preds, trues, labels, resolved["interactions"],
                                                             alpha=args.alpha, **kw))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
