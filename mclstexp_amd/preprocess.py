"""Raw count tables -> highly variable genes -> ``preprocessed_matrix.npy`` on the MI355X: the stage the reference runs
on the CPU with scanpy and scprep before anything else (/root/reference/hvg_her2st.py, hvg_cscc.py, hvg_visium.py):

    per slide   sc.pp.normalize_total; sc.pp.log1p; sc.pp.highly_variable_genes(n_top_genes=1000)   (Seurat flavour)
    pooling     union / intersection of the per-slide flags, a fixed gene list forced into the union
    matrices    adata[:, genes].X.T -> scprep.transform.log(scprep.normalize.library_size_normalize(.))

All slides of a dataset go through ONE ``mcl_hvg_stats`` call and ONE ``mcl_expression_matrices`` call
(csrc/preprocess.hip): every slide keeps its own (spots, genes) matrix, fp32 or int32, and an optional int32 column map
picks its columns of the shared genes, so the host makes no subset copy.  Everything of the statistics is fp64 with fixed
summation orders: a slide inside a batch is bit-identical to the same slide alone, run to run.  scanpy's fp32
``log1p`` -> ``expm1`` round trip is the identity and is NOT reproduced (measured gap of ``dispersions_norm`` between the
two forms on the fixture: <= 7.5e-7, no bin and no flag changes).  Parity with scanpy itself is unpinned (it
is absent where the fixture is made); pinned is a line-by-line restatement over pandas' own ``cut`` / ``groupby``
(tests/hvg_reference.py -> tests/golden/hvg.npz).

The matrix of a slide is log10(c / rowsum * 1e4 + 1) with the row sum taken over the SELECTED genes of a spot (the
library size after subsetting), written transposed as (genes, spots) -- the layout of ``preprocessed_matrix.npy`` that
``mclstexp_amd.evaluate --expressions`` reads.  Host side on purpose: gene NAMES (``shared_genes``: duplicates made
unique as anndata's ``var_names_make_unique`` does, then the SORTED intersection -- the reference's ``list(set)`` order is
arbitrary) and file handling.  Reading .tsv / .mtx / 10x folders is out of scope.  No CPU fallback: without a GPU / the
HIP library these functions raise ``RuntimeError``.

    python -m mclstexp_amd.preprocess --counts A.npy B.npy ... [--genes A.txt B.txt ...] [--gene_list L.npy|L.txt]
                                      --out_dir D [--n_top_genes N] [--select list|union|intersection] [--json OUT]
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._arrays import ArrayLike, Tensor, cumulative_offsets, device, empty, matrix, upload, write_json
from ._lib import call

N_TOP_GENES = 1000       # hvg_her2st.py:24
MAX_ROWS = 50000         # spots per slide (as mclstexp_amd.cluster)
MAX_SLIDES = 65535
MAX_GENES = 1 << 20      # shared genes per call, and selected genes per matrix
RESCALE = 1e4            # scprep.normalize.library_size_normalize
_DTYPE_CODE = {torch.float32: 0, torch.int32: 1}
STATUS_TEXT = {1: "the gene means are all equal (or not finite): pandas.cut's special case is not reproduced",
               2: "no spot holds a count", 4: "no gene has a defined normalised dispersion",
               8: "a column map entry lies outside the slide's columns"}


# ------------------------------------------------------------------------------------------------- host bookkeeping
def make_unique(names: Sequence[str]) -> List[str]:
    """anndata's ``var_names_make_unique`` (join "-"): the first occurrence keeps its name, later ones get -1, -2, ...,
    skipping suffixes that would collide with a name already present."""
    names = [str(n) for n in names]
    taken = set(names)
    seen: Dict[str, int] = {}
    out = []
    for n in names:
        if n not in seen:
            seen[n] = 0
            out.append(n)
            continue
        while True:
            seen[n] += 1
            cand = f"{n}-{seen[n]}"
            if cand not in taken:
                break
        taken.add(cand)
        out.append(cand)
    return out


def shared_genes(name_lists: Sequence[Sequence[str]]) -> Tuple[List[str], List[np.ndarray]]:
    """(shared, colmaps): the SORTED intersection of the slides' gene names (after ``make_unique``) and, per slide, the
    int32 column of every shared gene.  The reference's ``list(set.intersection(...))`` has no defined order; sorting
    makes the output reproducible and is the documented order of every per-gene result of this module."""
    if not len(name_lists):
        raise ValueError("shared_genes: need at least one list of gene names")
    uniq = [make_unique(n) for n in name_lists]
    common = set(uniq[0])
    for u in uniq[1:]:
        common &= set(u)
    shared = sorted(common)
    if not shared:
        raise ValueError("shared_genes: the slides share no gene name")
    maps = []
    for u in uniq:
        col = {n: i for i, n in enumerate(u)}
        maps.append(np.array([col[n] for n in shared], dtype=np.int32))
    return shared, maps


# ------------------------------------------------------------------------------------------------------ slide sets
def _slide(x: ArrayLike, name: str, dev: torch.device, dtype: Optional[torch.dtype] = None) -> Tensor:
    """A row-major float32 / int32 device matrix (no copy when it already is one).  Host arrays of other dtypes are
    converted on the host: integers to int32, everything else to float32.  ``dtype``: the one dtype to end up with."""
    def host_dtype(t: Tensor) -> torch.dtype:
        want = dtype or (torch.float32 if (t.dtype.is_floating_point or t.dtype == torch.bool) else torch.int32)
        if want == torch.int32 and t.numel() and (int(t.max()) > 2 ** 31 - 1 or int(t.min()) < -2 ** 31):
            raise ValueError(f"{name}: counts do not fit int32")
        return want
    return matrix(x, name, dev, (dtype,) if dtype is not None else _DTYPE_CODE, host_dtype)


def _check_shapes(slides: Sequence[ArrayLike]) -> np.ndarray:
    """The slides' widths, after the checks that need no device: 1 .. 65 535 slides of 2 .. 50 000 spots each."""
    if not len(slides):
        raise ValueError("slides: need at least one slide")
    if len(slides) > MAX_SLIDES:
        raise ValueError(f"at most {MAX_SLIDES} slides per call")
    for i, x in enumerate(slides):
        shape = tuple(x.shape) if hasattr(x, "shape") else ()
        if len(shape) != 2:
            raise ValueError(f"slides[{i}]: expected a 2-D (spots, genes) count matrix, got shape {shape}")
        if shape[0] < 2 or shape[0] > MAX_ROWS or shape[1] < 1:
            raise ValueError(f"slides[{i}]: needs 2 .. {MAX_ROWS} spots and >= 1 gene, got {shape}")
    return np.array([int(x.shape[1]) for x in slides], dtype=np.int64)


class _SlideSet:
    """The device-resident descriptor arrays of mcl_hvg_stats / mcl_expression_matrices and the tensors they point at."""

    def __init__(self, slides: Sequence[ArrayLike], dev: torch.device):
        _check_shapes(slides)
        first = [_slide(x, f"slides[{i}]", dev) if isinstance(x, Tensor) and x.is_cuda else None
                 for i, x in enumerate(slides)]
        kinds = {t.dtype for t in first if t is not None}
        if len(kinds) > 1:
            raise ValueError("device slides must share one dtype (float32 or int32)")
        if kinds:
            dtype = kinds.pop()
        else:
            host = [x if isinstance(x, Tensor) else torch.as_tensor(np.asarray(x)) for x in slides]
            ints = all(not (t.dtype.is_floating_point or t.dtype == torch.bool) for t in host)
            dtype = torch.int32 if ints else torch.float32
        self.tensors = [t if t is not None else _slide(x, f"slides[{i}]", dev, dtype)
                        for i, (x, t) in enumerate(zip(slides, first))]
        self.dtype = _DTYPE_CODE[dtype]
        self.S = len(self.tensors)
        self.rows = np.array([t.shape[0] for t in self.tensors], dtype=np.int32)
        self.ncols = np.array([t.shape[1] for t in self.tensors], dtype=np.int32)
        self.row_off = cumulative_offsets(self.rows)
        self.d_ptr = upload(np.array([t.data_ptr() for t in self.tensors], dtype=np.int64), dev)
        self.d_ld = upload(np.array([t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in self.tensors], dtype=np.int64),
                           dev)
        self.d_rows, self.d_ncols, self.d_row_off = (upload(a, dev) for a in (self.rows, self.ncols, self.row_off))
        self.dev = dev

    def args(self):
        return (self.d_ptr.data_ptr(), self.d_ld.data_ptr(), self.d_rows.data_ptr(), self.d_ncols.data_ptr(),
                self.d_row_off.data_ptr(), self.dtype)


def _column_maps(colmaps, ncols: np.ndarray, what: str = "colmaps") -> Tuple[Optional[np.ndarray], int]:
    """(S, G) int32 host array (None: gene g is column g of every slide) and G, checked against the slides' widths."""
    S = ncols.size
    if colmaps is None:
        if (ncols != ncols[0]).any():
            raise ValueError(f"slides of different widths {ncols.tolist()} need {what} (see shared_genes)")
        return None, int(ncols[0])
    if len(colmaps) != S:
        raise ValueError(f"{what}: {len(colmaps)} maps for {S} slides")
    rows = []
    for s, m in enumerate(colmaps):
        a = np.arange(ncols[s], dtype=np.int32) if m is None else np.asarray(m)
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what}[{s}]: expected a 1-D integer vector, got {a.dtype} {a.shape}")
        if a.size and (a.min() < 0 or a.max() >= ncols[s]):
            raise ValueError(f"{what}[{s}]: columns must lie in 0 .. {ncols[s] - 1}")
        rows.append(a.astype(np.int32))
    if len({a.size for a in rows}) != 1:
        raise ValueError(f"{what}: every slide must map the same number of genes, got {[a.size for a in rows]}")
    return np.stack(rows), int(rows[0].size)


# ------------------------------------------------------------------------------------------------------ statistics
def _stats_args(slides, colmaps, n_top_genes) -> Tuple[int, Optional[np.ndarray], int]:
    n_top_genes = int(n_top_genes)
    if n_top_genes < 1:
        raise ValueError(f"n_top_genes must be >= 1, got {n_top_genes}")
    cm, G = _column_maps(colmaps, _check_shapes(slides))
    if G < 2 or G > MAX_GENES:
        raise ValueError(f"the number of shared genes must lie in 2 .. {MAX_GENES}, got {G}")
    return n_top_genes, cm, G


def gene_stats(slides: Sequence[ArrayLike], colmaps: Optional[Sequence[Optional[ArrayLike]]] = None,
               n_top_genes: int = N_TOP_GENES) -> Dict[str, Tensor]:
    """normalize_total -> log1p -> highly_variable_genes(flavor="seurat", n_bins=20, n_top_genes) of every slide in one
    call.  ``slides[i]``: (spots_i, genes_i) counts, float32 or int32 (other host dtypes are converted on the host);
    ``colmaps[i]``: the columns of the G shared genes in slide i (``shared_genes``), None = the slides share their
    columns.  Device tensors: ``means``, ``dispersions``, ``dispersions_norm`` (S, G) fp64, ``mean_bin`` (S, G) int32,
    ``highly_variable`` (S, G) bool, ``cutoff``, ``target_sum`` (S,) fp64.  One read-back (the per-slide status word):
    a slide whose gene means are all equal, that holds no count or no defined dispersion raises ``ValueError``."""
    n_top_genes, cm, G = _stats_args(slides, colmaps, n_top_genes)
    dev = device("preprocess")
    ss = _SlideSet(slides, dev)
    S = ss.S
    cm_d = upload(cm, dev) if cm is not None else None
    e = empty(dev)
    res = {"means": e((S, G), torch.float64), "dispersions": e((S, G), torch.float64),
           "dispersions_norm": e((S, G), torch.float64), "mean_bin": e((S, G), torch.int32),
           "highly_variable": e((S, G), torch.bool), "cutoff": e((S,), torch.float64),
           "target_sum": e((S,), torch.float64)}
    work = e((int(ss.row_off[-1]),), torch.float64)
    status = e((S,), torch.int32)
    call("mcl_hvg_stats", *ss.args(), cm_d, S, G, int(ss.rows.max()), n_top_genes, work, res["means"], res["dispersions"],
         res["dispersions_norm"], res["mean_bin"], res["highly_variable"], res["cutoff"], res["target_sum"], status)
    st = status.cpu().numpy()                        # the one synchronisation
    if st.any():
        s = int(np.flatnonzero(st)[0])
        why = "; ".join(t for b, t in STATUS_TEXT.items() if st[s] & b)
        raise ValueError(f"slide {s}: {why}")
    return res


def pool(highly_variable: ArrayLike, extra: Optional[ArrayLike] = None) -> Tuple[Tensor, Tensor]:
    """(union, intersection), (G,) bool on the device, of the (S, G) per-slide flags; ``extra`` (gene indices) is forced
    into the union, as ``hvg_union[gene_list] = True`` does (hvg_her2st.py:64)."""
    hv = highly_variable if isinstance(highly_variable, Tensor) else torch.as_tensor(np.asarray(highly_variable))
    if hv.dim() != 2 or hv.dtype not in (torch.bool, torch.uint8) or hv.shape[0] < 1 or hv.shape[1] < 1:
        raise ValueError(f"highly_variable: expected a non-empty (S, G) bool array, got {hv.dtype} {tuple(hv.shape)}")
    S, G = int(hv.shape[0]), int(hv.shape[1])
    ex = None
    if extra is not None:
        ex = np.asarray(extra.cpu() if isinstance(extra, Tensor) else extra)
        if ex.ndim != 1 or not np.issubdtype(ex.dtype, np.integer):
            raise ValueError(f"extra: expected a 1-D vector of gene indices, got {ex.dtype} {ex.shape}")
        if ex.size and (ex.min() < 0 or ex.max() >= G):
            raise ValueError(f"extra: gene indices must lie in 0 .. {G - 1}")
        ex = ex.astype(np.int32)
    dev = device("preprocess")
    hv = hv.to(dev).contiguous()
    ex_d = upload(ex, dev) if ex is not None and ex.size else None
    uni, inter = torch.empty((G,), device=dev, dtype=torch.bool), torch.empty((G,), device=dev, dtype=torch.bool)
    call("mcl_hvg_pool", hv, S, G, ex_d, int(ex.size) if ex_d is not None else 0, uni, inter)
    return uni, inter


def expression_matrices(slides: Sequence[ArrayLike], colmaps: Optional[Sequence[Optional[ArrayLike]]],
                        genes: ArrayLike) -> List[Tensor]:
    """One (len(genes), spots_i) fp32 device matrix per slide, all slides in one launch: the columns ``genes`` (indices
    into the shared genes, i.e. through ``colmaps``) as log10(c / rowsum * 1e4 + 1), the row sum over the chosen genes
    only, transposed into the layout of ``preprocessed_matrix.npy``.  A spot without a count stays zero."""
    g = np.asarray(genes.cpu() if isinstance(genes, Tensor) else genes)
    if g.dtype == bool:
        g = np.flatnonzero(g)
    if g.ndim != 1 or not np.issubdtype(g.dtype, np.integer) or g.size < 1 or g.size > MAX_GENES:
        raise ValueError(f"genes: expected 1 .. {MAX_GENES} gene indices (or a bool mask), got {g.dtype} {g.shape}")
    cm, G = _column_maps(colmaps, _check_shapes(slides))
    if g.min() < 0 or g.max() >= G:
        raise ValueError(f"genes: indices must lie in 0 .. {G - 1}")
    S, K = len(slides), int(g.size)
    sel = cm[:, g] if cm is not None else np.broadcast_to(g.astype(np.int32), (S, K))
    dev = device("preprocess")
    ss = _SlideSet(slides, dev)
    sel_d = upload(np.asarray(sel, dtype=np.int32), dev)
    out = torch.empty((K * int(ss.row_off[-1]),), device=dev, dtype=torch.float32)
    call("mcl_expression_matrices", *ss.args(), sel_d, S, K, int(ss.rows.max()), float(RESCALE), out)
    return [out[K * int(ss.row_off[s]):K * int(ss.row_off[s + 1])].view(K, int(ss.rows[s])) for s in range(S)]


# ------------------------------------------------------------------------------------------------------ the scripts
def _gene_indices(gene_list, shared: Optional[List[str]], G: int) -> np.ndarray:
    a = np.asarray(gene_list)
    if a.ndim != 1 or a.size < 1:
        raise ValueError("gene_list: expected a non-empty 1-D list of gene names or indices")
    if np.issubdtype(a.dtype, np.integer):
        if a.min() < 0 or a.max() >= G:
            raise ValueError(f"gene_list: indices must lie in 0 .. {G - 1}")
        return a.astype(np.int64)
    if shared is None:
        raise ValueError("gene_list holds names: gene names per slide (names=...) are needed to resolve them")
    pos = {n: i for i, n in enumerate(shared)}
    missing = [str(n) for n in a if str(n) not in pos]
    if missing:
        raise ValueError(f"gene_list: {len(missing)} genes are not shared by all slides, e.g. {missing[:5]}")
    return np.array([pos[str(n)] for n in a], dtype=np.int64)


def run(slides: Sequence[ArrayLike], names: Optional[Sequence[Sequence[str]]] = None, n_top_genes: int = N_TOP_GENES,
        gene_list=None, select: str = "list") -> Dict[str, object]:
    """The hvg_*.py scripts for one dataset.  ``slides[i]``: (spots_i, genes_i) counts; ``names[i]``: its gene names
    (None: all slides share their columns); ``gene_list``: names (or indices into the shared genes) forced into the
    union; ``select``: which genes the matrices hold -- "list" (``gene_list`` in its order, hvg_her2st.py:107),
    "union" (hvg_cscc.py:65) or "intersection", the latter two in shared-gene order.  Returns ``matrices`` (one
    (genes, spots_i) fp32 device tensor per slide), ``genes`` (indices into the shared genes), ``gene_names`` (or None),
    ``shared`` (the shared names or None), ``union`` / ``intersection`` (G,) bool device tensors (the union with
    ``gene_list`` forced in), ``n_union`` / ``n_intersection`` (the counts the scripts print, before forcing) and
    ``stats`` (``gene_stats``)."""
    if select not in ("list", "union", "intersection"):
        raise ValueError(f"select must be 'list', 'union' or 'intersection', got {select!r}")
    if select == "list" and gene_list is None:
        raise ValueError("select='list' needs gene_list")
    shared = colmaps = None
    if names is not None:
        if len(names) != len(slides):
            raise ValueError(f"{len(names)} name lists for {len(slides)} slides")
        for i, (x, n) in enumerate(zip(slides, names)):
            if len(x.shape) != 2 or x.shape[1] != len(n):
                raise ValueError(f"slide {i}: {tuple(x.shape)} counts but {len(n)} gene names")
        shared, colmaps = shared_genes(names)
    _, _, G = _stats_args(slides, colmaps, n_top_genes)
    forced = _gene_indices(gene_list, shared, G) if gene_list is not None else None
    tensors = _SlideSet(slides, device("preprocess")).tensors          # one upload for both calls
    stats = gene_stats(tensors, colmaps, n_top_genes)
    uni, inter = pool(stats["highly_variable"])
    n_union, n_inter = int(uni.cpu().numpy().sum()), int(inter.cpu().numpy().sum())
    if forced is not None:
        uni, inter = pool(stats["highly_variable"], forced)
    if select == "list":
        genes = forced
    else:
        genes = np.flatnonzero((uni if select == "union" else inter).cpu().numpy())
        if genes.size == 0:
            raise ValueError(f"the {select} of the highly variable genes is empty")
    mats = expression_matrices(tensors, colmaps, genes)
    return {"matrices": mats, "genes": genes, "gene_names": [shared[i] for i in genes] if shared is not None else None,
            "shared": shared, "union": uni, "intersection": inter, "n_union": n_union, "n_intersection": n_inter,
            "stats": stats}


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m mclstexp_amd.preprocess",
                                description="HVG selection and the preprocessed expression matrices of a dataset "
                                            "(the reference's hvg_her2st.py / hvg_cscc.py / hvg_visium.py)")
    p.add_argument("--counts", required=True, nargs="+", help="one (spots, genes) .npy of raw counts per slide")
    p.add_argument("--genes", nargs="+", default=None,
                   help="one text file of gene names (one per line, column order) per slide; omitted: the slides "
                        "share their columns")
    p.add_argument("--gene_list", default=None,
                   help=".npy (no pickle) or .txt of the genes forced into the union: names, or indices without --genes")
    p.add_argument("--out_dir", required=True, help="writes OUT_DIR/<slide>/preprocessed_matrix.npy")
    p.add_argument("--n_top_genes", type=int, default=N_TOP_GENES)
    p.add_argument("--select", choices=("list", "union", "intersection"), default=None,
                   help="the genes of the matrices (default: list with --gene_list, else union)")
    p.add_argument("--json", default=None, help="also write the selection and per-slide cut-offs to this file")
    a = p.parse_args(argv)
    if a.genes is not None and len(a.genes) != len(a.counts):
        p.error(f"{len(a.counts)} --counts files but {len(a.genes)} --genes files")
    if a.select is None:
        a.select = "list" if a.gene_list else "union"
    if a.select == "list" and not a.gene_list:
        p.error("--select list needs --gene_list")
    stems = [slide_name(f) for f in a.counts]
    if len(set(stems)) != len(stems):
        p.error(f"slide names (file names without extension) must differ: {stems}")
    return a


def slide_name(path: str) -> str:
    return os.path.splitext(os.path.basename(path))[0]


def read_names(path: str) -> List[str]:
    with open(path, encoding="utf-8") as fh:
        return [ln.strip() for ln in fh if ln.strip()]


def read_gene_list(path: str):
    if path.endswith(".npy"):
        return np.load(path, allow_pickle=False)
    names = read_names(path)
    return np.array([int(n) for n in names]) if names and all(n.lstrip("-").isdigit() for n in names) else names


def format_report(res: Dict[str, object]) -> str:
    """The two lines hvg_her2st.py:51-52 prints."""
    return f"Number of HVGs:  {res['n_union']}\nNumber of HVGs (intersection):  {res['n_intersection']}"


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    slides = [np.load(f) for f in a.counts]
    names = [read_names(f) for f in a.genes] if a.genes else None
    gene_list = read_gene_list(a.gene_list) if a.gene_list else None
    res = run(slides, names, a.n_top_genes, gene_list, a.select)
    print(format_report(res))
    for f, m in zip(a.counts, res["matrices"]):
        d = os.path.join(a.out_dir, slide_name(f))
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "preprocessed_matrix.npy"), m.cpu().numpy())
        print(f"{slide_name(f)}: {tuple(m.shape)}")
    if a.json:
        doc = {"n_union": res["n_union"], "n_intersection": res["n_intersection"], "select": a.select,
               "n_top_genes": a.n_top_genes, "genes": np.asarray(res["genes"]).tolist(), "gene_names": res["gene_names"],
               "slides": [slide_name(f) for f in a.counts],
               "cutoff": res["stats"]["cutoff"].cpu().numpy().tolist(),
               "target_sum": res["stats"]["target_sum"].cpu().numpy().tolist()}
        write_json(a.json, doc)
    return 0


if __name__ == "__main__":
    sys.exit(main())
