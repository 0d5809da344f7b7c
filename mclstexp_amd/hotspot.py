"""Local spatial statistics on the MI355X: WHERE does a gene vary across the tissue?  Local Moran's I_i (esda's
``Moran_Local``, and ``Moran_Local_BV`` for a pair of columns), Getis-Ord Gi*, the Moran quadrant and the hot / cold spot
label of every (spot, gene) under a conditional permutation test, for all slides of an evaluation per call -- and the
number the feature exists for: does a predicted gene put its hot spot where the measured gene has it (``hotspot_recovery``)?
``colocalisation`` is the bivariate form over ligand-receptor column pairs.

What is computed is stated in DESIGN 6.22 and restated in numpy by ``tests/hotspot_reference.py``, which is pinned to dense
W-matrix formulas and to scipy.  esda and squidpy are not installed: parity with a release of either is unpinned.  Things
to know:

* The graph is ``spatial.lattice``'s.  For a pair (a, b) the column a is held at the spot and column b is lagged over its
  kept neighbours; (j, j) is the univariate case.  ``local_i`` = (n - 1) z_a (w L) / den_a (a != b: / sqrt(den_a den_b)),
  ``quadrant`` 1 HH, 2 LH, 3 LL, 4 HL (0 where a sign is zero), ``gi_z`` with binary star weights whatever the graph's
  standardisation (univariate only; NaN at n = d_i + 1), its one-tailed normal p and -log10 p in log space.
* The permutation test is CONDITIONAL: spot i keeps its value and its d_i neighbours are redrawn from the other n - 1
  spots without replacement.  Draw (p, i) is a pure function of (seed, p, i, n, d_i) -- not of the gene, of the slide's
  place in the batch or of the launch, and not esda's random stream.  ``pval_sim`` = (min(count_ge, count_le) + 1) /
  (P + 1) counts ties on both sides: a spot whose every sim ties gets p = 1 where esda gives 1 / (P + 1).
* ``cluster`` = the quadrant where ``pval_sim`` <= alpha, else 0.  No FDR across spots is computed.
* A constant column is NaN in every floating output and 0 in ``quadrant`` / ``cluster``; a spot without kept neighbours
  has L = 0, I = 0 and p = 1.

Everything on the device is fp64, free of floating-point atomics and bit-reproducible run to run; a slide inside a batch
is bit-identical to the same slide alone.  No CPU fallback: without a GPU / the HIP library these functions raise
``RuntimeError``.

    python -m mclstexp_amd.hotspot --pred P1.npy ... --coords C1.npy ... [--true T1.npy ...] [--genes names.npy]
                                   [--select NAME ...] [--pairs pairs.tsv] [--k 8] [--prune NA|STD|Grid] [--n_perms 999]
                                   [--seed 0] [--alpha 0.05] [--out_dir D]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import spatial
from ._arrays import (FLOAT_CODE, ArrayLike, Tensor, check_flag, check_int, cumulative_offsets, device, empty,
                      load_gene_major, matrix, nanmean, stack_rows, upload)
from ._lib import call

MAX_ROWS, MAX_K, MAX_GENES, MAX_PERMS = spatial.MAX_ROWS, spatial.MAX_K, spatial.MAX_GENES, spatial.MAX_PERMS
MAX_PAIRS = 16384
OUT_FILE = "hotspot.npz"
PAD = -1                 # a draw table's slots past d_i (0xFFFF on the device)
HH, LH, LL, HL = 1, 2, 3, 4
_STATUS = ("offsets that do not match the host's", "non-finite values", "pair columns outside the matrix",
           "draws that do not fit the graph (d_i spots other than i per row, then padding)")
_OBSERVED = ("local_i", "quadrant", "gi_z", "gi_pval_norm", "gi_neglog10_pval_norm", "lag")
_PERMUTED = ("pval_sim", "mean_sim", "var_sim", "z_sim", "cluster", "count_ge", "count_le", "sum_sim", "sumsq_sim")


# ------------------------------------------------------------------------------------------------------- host rules
def check_pairs(pairs, genes, G: int) -> np.ndarray:
    """The (M, 2) int32 (held, lagged) columns of a call: ``pairs`` as given, else (g, g) for every g of ``genes``, else
    for every column."""
    if pairs is not None and genes is not None:
        raise ValueError("give pairs= or genes=, not both")
    if pairs is None:
        g = np.arange(G) if genes is None else np.asarray(genes)
        if g.ndim != 1 or g.size < 1 or not np.issubdtype(g.dtype, np.integer) or g.dtype == np.bool_:
            raise ValueError(f"genes: expected a 1-D integer array of >= 1 columns, got {g!r}")
        pr = np.stack([g, g], axis=1)
    else:
        pr = np.asarray(pairs)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] < 1 or not np.issubdtype(pr.dtype, np.integer) or pr.dtype == np.bool_:
            raise ValueError(f"pairs: expected an integer (M, 2) array of (held, lagged) columns, got shape {pr.shape} "
                             f"dtype {pr.dtype}")
    if pr.shape[0] > MAX_PAIRS:
        raise ValueError(f"1 .. {MAX_PAIRS} pairs per call, got {pr.shape[0]}")
    if (pr < 0).any() or (pr >= G).any():
        bad = int(np.flatnonzero(((pr < 0) | (pr >= G)).any(axis=1))[0])
        raise ValueError(f"pairs: row {bad} = {pr[bad].tolist()} names a column outside 0 .. {G - 1}")
    return np.ascontiguousarray(pr.astype(np.int32))


def check_local(shape: Sequence[int], graph, n_perms, seed, alpha, return_draws):
    if not isinstance(graph, dict) or not {"nbr", "w", "offsets", "offsets_device", "k"} <= set(graph):
        raise ValueError("graph: expected what spatial.lattice() returns")
    if len(shape) != 2:
        raise ValueError(f"x: expected a 2-D (rows, genes) matrix, got shape {tuple(shape)}")
    rows, G = int(shape[0]), int(shape[1])
    if G < 1 or G > MAX_GENES:
        raise ValueError(f"1 .. {MAX_GENES} genes per call, got {G}")
    if rows != int(graph["offsets"][-1]):
        raise ValueError(f"x has {rows} rows, the graph {int(graph['offsets'][-1])}")
    P = check_int(n_perms, "n_perms", 0, MAX_PERMS)
    seed = check_int(seed, "seed", 0, 2 ** 64 - 1)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.floating)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha must be a number in 0 .. 1, got {alpha!r}")
    check_flag(return_draws, "return_draws")
    return rows, G, P, seed, float(alpha)


def check_draws(draws, sizes: np.ndarray, k: int) -> np.ndarray:
    """``draws``: one (P, n_s, k) integer array per slide, one P for all slides; row (p, i) lists distinct spots of
    0 .. n_s - 1 other than i, then -1 in the slots that are left (their number must be the spot's kept neighbours: that
    is checked on the device, which knows them).  Returns the table in the device's layout as int16."""
    if not isinstance(draws, (list, tuple)) or len(draws) != sizes.size:
        raise ValueError(f"draws: expected a list of {sizes.size} arrays, one (P, n_s, {k}) array per slide")
    parts, P = [], None
    for s, (a, n) in enumerate(zip(draws, sizes)):
        a = np.asarray(a)
        if a.ndim != 3 or a.shape[1:] != (n, k) or not np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
            raise ValueError(f"draws[{s}]: expected an integer (P, {int(n)}, {k}) array, got shape {a.shape} dtype {a.dtype}")
        if P is None:
            P = a.shape[0]
        if a.shape[0] != P or P < 1 or P > MAX_PERMS:
            raise ValueError(f"draws[{s}]: every slide needs the same 1 .. {MAX_PERMS} draws, got {a.shape[0]}")
        a = a.astype(np.int64)
        live = a != PAD
        own = np.arange(n)[None, :, None]
        wrong = (live & ((a < 0) | (a >= n) | (a == own))) | (live[:, :, 1:] & ~live[:, :, :-1]).any(axis=2, keepdims=True)
        srt = np.sort(np.where(live, a, -2 - np.arange(k)[None, None, :]), axis=2)
        wrong = wrong.any(axis=2) | (np.diff(srt, axis=2) == 0).any(axis=2)
        if wrong.any():
            p, i = (int(v[0]) for v in np.nonzero(wrong))
            raise ValueError(f"draws[{s}]: draw {p} of spot {i} is not a list of distinct spots of 0 .. {int(n) - 1} other "
                             f"than {i} followed by {PAD}")
        parts.append(a.astype(np.int16).ravel())
    return np.concatenate(parts)


# ----------------------------------------------------------------------------------------------------------- device
def local_stats_device(x: ArrayLike, graph: Dict[str, object], pairs=None, genes=None, n_perms: int = 0, seed: int = 0,
                       draws=None, alpha: float = 0.05, return_draws: bool = False) -> Dict[str, object]:
    """``local_stats`` with everything left on the device: (rows, M) tensors ``local_i``, ``quadrant`` (int8), ``gi_z``,
    ``gi_pval_norm``, ``gi_neglog10_pval_norm``, ``lag`` and, with permutations, ``pval_sim``, ``mean_sim``, ``var_sim``,
    ``z_sim``, ``cluster`` (int8), ``count_ge``, ``count_le`` (int32), ``sum_sim``, ``sumsq_sim`` (of the L^p); ``mean``,
    ``den``, ``mean_lag``, ``den_lag`` (S, M); ``deg`` (rows,) int32; ``pairs`` (M, 2) int32; with ``return_draws`` or
    ``draws=`` the int16 view ``table`` (slide s: (P, n_s, k) at element P * k * offsets[s]).  ``pairs`` may be a device
    int32 tensor: its columns are then checked on the device."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    rows, G, P, seed, alpha = check_local(shape, graph, n_perms, seed, alpha, return_draws)
    off, k = graph["offsets"], int(graph["k"])
    sizes = np.diff(off)
    dev = device("hotspot")
    if isinstance(pairs, Tensor):
        if genes is not None or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_cuda \
                or not pairs.is_contiguous() or not 1 <= pairs.shape[0] <= MAX_PAIRS:
            raise ValueError("pairs: a device tensor must be a contiguous int32 (M, 2) tensor, 1 <= M <= "
                             f"{MAX_PAIRS}, without genes=")
        pairs_d = pairs
    else:
        pairs_d = None
        host_pairs = check_pairs(pairs, genes, G)
    host_table = None
    if draws is not None:
        host_table = check_draws(draws, sizes, k)
        P = host_table.size // (rows * k)
    if pairs_d is None:
        pairs_d = upload(host_pairs, dev)
    M = int(pairs_d.shape[0])
    xd = matrix(x, "x", dev, FLOAT_CODE, lambda t: torch.float32 if t.dtype == torch.float16 else torch.float64)
    S, max_n = int(sizes.size), int(sizes.max())
    e = empty(dev)
    f64, i32, i8 = torch.float64, torch.int32, torch.int8
    mask = 0
    for n in np.unique(sizes):
        mask |= 1 << int(call("mcl_hotspot_columns", int(n)))
    code, ld = FLOAT_CODE[xd.dtype], int(xd.stride(0))
    off_d = graph["offsets_device"]
    status = torch.zeros((S, 4), device=dev, dtype=i32)
    mom_mean, mom_den = e((2, S, M), f64), e((2, S, M), f64)
    call("mcl_hotspot_moments", xd, ld, code, off_d, S, rows, G, max_n, pairs_d, M, mom_mean, mom_den, status)
    table = work = None
    if P and (host_table is not None or return_draws):
        work = e((int(call("mcl_hotspot_table_bytes", rows, k, P)) // 8 + 1,), f64)
        table = work.view(torch.int16)[:P * rows * k]
        if host_table is None:
            call("mcl_hotspot_draws", off_d, S, rows, max_n, k, graph["w"], P, seed, work)
        else:
            table.copy_(torch.from_numpy(host_table))
    lag, deg, wbar = e((rows, M), f64), e((rows,), i32), e((rows,), f64)
    ge = le = s1 = s2 = None
    if P:
        ge, le, s1, s2 = e((rows, M), i32), e((rows, M), i32), e((rows, M), f64), e((rows, M), f64)
    call("mcl_hotspot_permute", xd, ld, code, off_d, S, rows, G, max_n, k, mask, graph["nbr"], graph["w"], pairs_d, M,
         mom_mean, mom_den, work, P, seed, lag, ge, le, s1, s2, deg, wbar, status)
    li, quad = e((rows, M), f64), e((rows, M), i8)
    gz, gp, gl = (e((rows, M), f64) for _ in range(3))
    ps = ms = vs = zs = cl = None
    if P:
        ps, ms, vs, zs = (e((rows, M), f64) for _ in range(4))
        cl = e((rows, M), i8)
    call("mcl_hotspot_finalise", xd, ld, code, off_d, S, rows, G, max_n, pairs_d, M, mom_mean, mom_den, deg, wbar, lag, ge, le,
         s1, s2, P, alpha, li, quad, gz, gp, gl, ps, ms, vs, zs, cl)
    out = {"local_i": li, "quadrant": quad, "gi_z": gz, "gi_pval_norm": gp, "gi_neglog10_pval_norm": gl, "lag": lag,
           "mean": mom_mean[0], "den": mom_den[0], "mean_lag": mom_mean[1], "den_lag": mom_den[1], "deg": deg, "wbar": wbar,
           "pairs": pairs_d, "n_perms": P, "alpha": alpha}
    if P:
        out.update({"pval_sim": ps, "mean_sim": ms, "var_sim": vs, "z_sim": zs, "cluster": cl, "count_ge": ge, "count_le": le,
                    "sum_sim": s1, "sumsq_sim": s2})
        if table is not None:
            out.update({"table": table, "workspace": work})
    bad = status.cpu().numpy()                                  # the one synchronisation
    for col, what in enumerate(_STATUS):
        if bad[:, col].any():
            s = int(np.flatnonzero(bad[:, col])[0])
            raise ValueError(f"local_stats: slide {s} holds {what}" + (f" ({int(bad[s, col])})" if col else ""))
    return out


def local_stats(x: ArrayLike, graph: Dict[str, object], pairs=None, genes=None, n_perms: int = 0, seed: int = 0, draws=None,
                alpha: float = 0.05, return_draws: bool = False) -> List[Dict[str, object]]:
    """Local Moran, Getis-Ord Gi* and the hot / cold spot labels of every (spot, pair) of every slide.

    ``x``: row-stacked (rows, G), float32 or float64, host or device, a row stride allowed.  ``graph``: what
    ``spatial.lattice`` returned for the same rows.  ``pairs``: (M, 2) (held, lagged) columns; ``genes``: the columns of a
    univariate run (default: all).  ``n_perms``: conditional draws per spot (0: none), generated from ``seed`` or replayed
    from ``draws`` (one (P, n_s, k) integer array per slide, -1 past d_i).  Returns one dict per slide: ``n``, ``k``,
    ``pairs`` (M, 2), ``mean``, ``den``, ``mean_lag``, ``den_lag`` (M,), ``deg`` (n,), the (n, M) arrays ``local_i``,
    ``quadrant``, ``gi_z``, ``gi_pval_norm``, ``gi_neglog10_pval_norm``, ``lag`` and with permutations ``pval_sim``,
    ``mean_sim``, ``var_sim``, ``z_sim``, ``cluster``, ``count_ge``, ``count_le``, ``sum_sim``, ``sumsq_sim`` (and
    ``draws`` (P, n, k) with ``return_draws``)."""
    d = local_stats_device(x, graph, pairs, genes, n_perms, seed, draws, alpha, return_draws)
    P, off, k = int(d["n_perms"]), graph["offsets"], int(graph["k"])
    keys = [key for key in _OBSERVED + _PERMUTED if key in d]
    host = {key: d[key].cpu().numpy() for key in keys + ["mean", "den", "mean_lag", "den_lag", "deg", "pairs"]}
    table = d["table"].cpu().numpy() if return_draws and "table" in d else None
    out = []
    for s in range(off.size - 1):
        a, b = int(off[s]), int(off[s + 1])
        one = {"n": b - a, "k": k, "n_perms": P, "alpha": d["alpha"], "pairs": host["pairs"].astype(np.int64),
               "deg": host["deg"][a:b]}
        one.update({key: host[key][s] for key in ("mean", "den", "mean_lag", "den_lag")})
        one.update({key: host[key][a:b] for key in keys})
        if table is not None:
            one["draws"] = table[P * k * a:P * k * b].reshape(P, b - a, k).astype(np.int64)
        out.append(one)
    return out


def _stack(matrices: Sequence[ArrayLike], coords: Sequence[ArrayLike], k, prune, row_standardise):
    if len(matrices) != len(coords) or not len(matrices):
        raise ValueError(f"need one coordinate array per slide and >= 1 slide; got {len(matrices)} and {len(coords)}")
    cs = []
    for i, (m, c) in enumerate(zip(matrices, coords)):
        c = c.cpu().numpy() if isinstance(c, Tensor) else np.asarray(c)
        if len(m.shape) != 2 or c.ndim != 2 or c.shape != (m.shape[0], 2):
            raise ValueError(f"slide {i}: matrix {tuple(m.shape)} and coordinates {tuple(c.shape)} do not match")
        cs.append(c.astype(np.float64))
    off = cumulative_offsets([int(m.shape[0]) for m in matrices])
    spatial.check_lattice((int(off[-1]), 2), off, k, prune, row_standardise)
    return np.concatenate(cs), off


def local_stats_slides(matrices: Sequence[ArrayLike], coords: Sequence[ArrayLike], k: int = 8, prune: str = "NA",
                       row_standardise: bool = True, **kw) -> List[Dict[str, object]]:
    """``local_stats`` of one (spots, genes) matrix and one (spots, 2) coordinate array per slide."""
    c, off = _stack(matrices, coords, k, prune, row_standardise)
    dev = device("hotspot")
    x, off = stack_rows(matrices, "matrices", dev)
    graph = spatial.lattice(c, off, k, prune, row_standardise)
    return local_stats(x, graph, **kw)


def hotspots(res: Sequence[Dict[str, object]], slide: int, gene: int, kind: str = "hot") -> np.ndarray:
    """The spot indices of one slide labelled HH for column ``gene`` of the result (``kind="cold"``: LL)."""
    if kind not in ("hot", "cold"):
        raise ValueError(f"kind must be 'hot' or 'cold', got {kind!r}")
    if "cluster" not in res[slide]:
        raise ValueError("the result holds no labels: run local_stats with n_perms > 0")
    return np.flatnonzero(res[slide]["cluster"][:, gene] == (HH if kind == "hot" else LL))


def pearson(a: np.ndarray, b: np.ndarray) -> float:
    """Pearson r over the spots where both statistics are defined (host: n numbers)."""
    return spatial.pearson(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def compare(rp: Dict[str, object], rt: Dict[str, object], stat: str = "gi") -> Dict[str, np.ndarray]:
    """Per gene between the results of one slide: ``pearson`` over spots of ``gi_z`` (``stat="moran"``: of I),
    ``agreement`` (the share of spots with the same label), ``overlap_hot`` / ``jaccard_hot`` of the HH sets and
    ``overlap_cold`` / ``jaccard_cold`` of the LL sets.  A gene that is NaN on either side is NaN; the Jaccard index of
    two empty sets is NaN."""
    key = "gi_z" if stat == "gi" else "local_i"
    M = rp[key].shape[1]
    out = {name: np.full(M, np.nan) for name in ("pearson", "agreement", "jaccard_hot", "jaccard_cold")}
    out["overlap_hot"], out["overlap_cold"] = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for m in range(M):
        if np.isnan(rp[key][:, m]).all() or np.isnan(rt[key][:, m]).all():
            continue
        out["pearson"][m] = pearson(rp[key][:, m], rt[key][:, m])
        out["agreement"][m] = float((rp["cluster"][:, m] == rt["cluster"][:, m]).mean())
        for name, label in (("hot", HH), ("cold", LL)):
            A, B = rp["cluster"][:, m] == label, rt["cluster"][:, m] == label
            out["overlap_" + name][m] = int((A & B).sum())
            if (A | B).any():
                out["jaccard_" + name][m] = (A & B).sum() / (A | B).sum()
    return out


def hotspot_recovery(preds: Sequence[ArrayLike], trues: Sequence[ArrayLike], coords: Sequence[ArrayLike], alpha: float = 0.05,
                     stat: str = "gi", n_perms: int = 199, **kw) -> Dict[str, object]:
    """Does a predicted gene put its hot spots where the measured gene has them?  Per slide and gene (lists of (M,)
    arrays): ``pearson``, ``agreement``, ``overlap_hot``, ``jaccard_hot``, ``overlap_cold``, ``jaccard_cold`` (``compare``);
    their means over the genes and slides where they are defined (``mean_pearson``, ...), ``n_nan`` (the (slide, gene)
    cells left out of ``mean_pearson``) and the two results ``pred`` / ``true``."""
    if stat not in ("gi", "moran"):
        raise ValueError(f"stat must be 'gi' or 'moran', got {stat!r}")
    if len(preds) != len(trues):
        raise ValueError(f"need one measured matrix per prediction; got {len(preds)} and {len(trues)}")
    for i, (p, t) in enumerate(zip(preds, trues)):
        if tuple(p.shape) != tuple(t.shape):
            raise ValueError(f"slide {i}: pred {tuple(p.shape)} and true {tuple(t.shape)} differ in shape")
    check_int(n_perms, "n_perms", 1, MAX_PERMS)                 # the labels need draws
    if stat == "gi" and kw.get("pairs") is not None:
        raise ValueError("stat='gi' is univariate: give genes=, not pairs=")
    rp = local_stats_slides(preds, coords, alpha=alpha, n_perms=n_perms, **kw)
    rt = local_stats_slides(trues, coords, alpha=alpha, n_perms=n_perms, **kw)
    per = [compare(a, b, stat) for a, b in zip(rp, rt)]
    out = {key: [c[key] for c in per] for key in per[0]}
    for key in ("pearson", "agreement", "jaccard_hot", "jaccard_cold"):
        out["mean_" + key] = nanmean(np.concatenate(out[key]))
    for key in ("overlap_hot", "overlap_cold"):
        out["mean_" + key] = float(np.mean(np.concatenate(out[key])))
    out.update({"n_nan": int(np.isnan(np.concatenate(out["pearson"])).sum()), "stat": stat, "alpha": float(alpha),
                "pred": rp, "true": rt})
    return out


def colocalisation(x: ArrayLike, graph: Dict[str, object], pairs, n_perms: int = 199, seed: int = 0,
                   alpha: float = 0.05) -> List[Dict[str, object]]:
    """Bivariate local Moran of ligand-receptor column pairs: is the receptor high around the spots where the ligand is
    high?  ``pairs``: (ligand column, receptor column) rows, or ``ligrec.resolve_pairs(...)["interactions"]`` -- single
    genes a side; a pair with a complex is a ``ValueError``.  Returns per slide ``local_i`` (n, M) = I_bv, ``pval_sim``,
    ``quadrant``, ``cluster`` and ``share_hh`` (M,): the share of spots labelled HH at ``alpha``."""
    rows = []
    for r, row in enumerate(pairs):
        row = tuple(row)
        if len(row) != 2:
            raise ValueError(f"pairs[{r}]: expected (ligand, receptor), got {row!r}")
        for side in row:
            if isinstance(side, (tuple, list, np.ndarray)):
                raise ValueError(f"pairs[{r}]: {row!r} holds a complex; colocalisation takes single genes a side")
            check_int(side, f"pairs[{r}]", 0)
        rows.append((int(row[0]), int(row[1])))
    if not rows:
        raise ValueError("pairs: need at least one pair")
    check_int(n_perms, "n_perms", 1, MAX_PERMS)
    res = local_stats(x, graph, pairs=np.asarray(rows, dtype=np.int64), n_perms=n_perms, seed=seed, alpha=alpha)
    return [{"n": r["n"], "pairs": r["pairs"], "local_i": r["local_i"], "pval_sim": r["pval_sim"], "quadrant": r["quadrant"],
             "cluster": r["cluster"], "share_hh": (r["cluster"] == HH).mean(axis=0)} for r in res]


# --------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.hotspot",
                                description="Local Moran, Getis-Ord Gi* and hot / cold spot labels of every gene on the "
                                            "spot lattice graph, and how well predictions put the hot spots where the "
                                            "measured matrix has them")
    p.add_argument("--pred", required=True, nargs="+", help="one expression matrix per slide, (G, N), in slide order")
    p.add_argument("--coords", required=True, nargs="+", help="one (N, 2) coordinate array per slide")
    p.add_argument("--true", default=None, nargs="+", help="the measured matrices, (G, N): also print the recovery line")
    p.add_argument("--genes", default=None, help=".npy of G gene names (default: the gene index)")
    p.add_argument("--select", default=None, nargs="+", help="the genes to analyse, by name (with --genes) or index")
    p.add_argument("--pairs", default=None, help="two-column file of (ligand, receptor) names: also the colocalisation")
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--prune", default="NA", choices=list(spatial.PRUNES))
    p.add_argument("--no_row_standardise", action="store_true", help="binary weights instead of 1 / deg")
    p.add_argument("--n_perms", type=int, default=999)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--alpha", type=float, default=0.05)
    p.add_argument("--top", type=int, default=5, help="genes listed per slide")
    p.add_argument("--out_dir", default=None, help=f"writes <out_dir>/<i>/{OUT_FILE}")
    a = p.parse_args(argv)
    if len(a.coords) != len(a.pred):
        p.error(f"{len(a.coords)} --coords files for {len(a.pred)} --pred files")
    if a.true is not None and len(a.true) != len(a.pred):
        p.error(f"{len(a.true)} --true files for {len(a.pred)} --pred files")
    if a.k < 1 or a.k > MAX_K:
        p.error(f"--k must lie in 1 .. {MAX_K}")
    if a.n_perms < 1 or a.n_perms > MAX_PERMS:
        p.error(f"--n_perms must lie in 1 .. {MAX_PERMS}")
    if a.seed < 0:
        p.error("--seed must be >= 0")
    if not 0.0 <= a.alpha <= 1.0:
        p.error("--alpha must lie in 0 .. 1")
    if a.top < 1:
        p.error("--top must be >= 1")
    if a.pairs is not None and a.genes is None:
        p.error("--pairs names genes: it needs --genes")
    return a


def select_columns(select: Optional[Sequence[str]], names: Optional[Sequence[str]], G: int) -> Optional[np.ndarray]:
    """--select as column indices: names looked up in ``names``, else integers."""
    if select is None:
        return None
    cols = []
    for v in select:
        if names is not None and v in names:
            cols.append(list(names).index(v))
        elif v.lstrip("-").isdigit() and 0 <= int(v) < G:
            cols.append(int(v))
        else:
            raise ValueError(f"--select {v}: neither a gene name nor a column in 0 .. {G - 1}")
    return np.asarray(cols, dtype=np.int64)


def format_slides(res: Sequence[Dict[str, object]], names: Optional[Sequence[str]], top: int = 5) -> List[str]:
    lines = []
    for s, r in enumerate(res):
        hh = (r["cluster"] == HH).sum(axis=0)
        order = np.argsort(-hh, kind="stable")[:max(1, min(top, hh.size))]
        cells = [f"{names[int(r['pairs'][m, 0])] if names is not None else int(r['pairs'][m, 0])} ({int(hh[m])})" for m in order]
        lines.append(f"slide {s} n = {r['n']} k = {r['k']} draws = {r['n_perms']} alpha = {r['alpha']:g} genes by HH spots: "
                     + ", ".join(cells))
    return lines


def format_recovery(rec: Dict[str, object]) -> str:
    return (f"recovery ({rec['stat']}): mean Pearson {rec['mean_pearson']:.4f}, label agreement {rec['mean_agreement']:.4f}, "
            f"HH Jaccard {rec['mean_jaccard_hot']:.4f}, LL Jaccard {rec['mean_jaccard_cold']:.4f}, "
            f"{rec['n_nan']} undefined genes left out")


def main(argv: Optional[Sequence[str]] = None) -> int:
    from . import ligrec
    args = parse_args(argv)
    preds = load_gene_major(args.pred)
    coords = [np.load(f) for f in args.coords]
    G = preds[0].shape[1]
    names = None
    if args.genes is not None:
        names = [str(v) for v in np.load(args.genes, allow_pickle=True).reshape(-1)]
        if len(names) != G:
            raise ValueError(f"{args.genes}: {len(names)} gene names for {G} genes")
    cols = select_columns(args.select, names, G)
    kw = dict(k=args.k, prune=args.prune, row_standardise=not args.no_row_standardise, n_perms=args.n_perms, seed=args.seed,
              genes=cols)
    res = local_stats_slides(preds, coords, alpha=args.alpha, **kw)
    print("\n".join(format_slides(res, names, args.top)))
    extra = [{} for _ in res]
    if args.pairs is not None:
        rp = ligrec.resolve_pairs(ligrec.read_pairs(args.pairs), names)
        c, off = _stack(preds, coords, args.k, args.prune, not args.no_row_standardise)
        x, off = stack_rows(preds, "matrices", device("hotspot"))
        graph = spatial.lattice(c, off, args.k, args.prune, not args.no_row_standardise)
        co = colocalisation(x, graph, rp["interactions"], n_perms=args.n_perms, seed=args.seed, alpha=args.alpha)
        for s, r in enumerate(co):
            best = np.argsort(-r["share_hh"], kind="stable")[:args.top]
            print(f"slide {s} colocalisation, share of spots HH: "
                  + ", ".join(f"{rp['names'][m][0]}-{rp['names'][m][1]} ({r['share_hh'][m]:.3f})" for m in best))
            extra[s] = {"coloc_" + key: np.asarray(r[key]) for key in ("pairs", "local_i", "pval_sim", "cluster", "share_hh")}
    if args.out_dir is not None:
        for i, r in enumerate(res):
            d = os.path.join(args.out_dir, str(i))
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, OUT_FILE), **{key: np.asarray(v) for key, v in r.items()}, **extra[i])
    if args.true is not None:
        trues = load_gene_major(args.true)
        print(format_recovery(hotspot_recovery(preds, trues, coords, alpha=args.alpha, **kw)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
