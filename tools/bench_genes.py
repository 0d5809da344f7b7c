#!/usr/bin/env python3
"""Micro-benchmark of the gene-significance table (mclstexp_amd.genes) on one MI355X against the way the reference's
tutorial computes it on the host: one ``scipy.stats.pearsonr`` call per gene and slide (what its get_R loops over), then
the pandas table (tests/genes_reference.py ``tutorial_table``).  Per shape: ``mcl_pearson_pvalue`` and ``mcl_gene_rank``
alone on device-resident matrices (HIP events), ``significance_table`` end to end on device-resident per-slide tensors
(stacking, r, p, rank, results to the host; host clock around a device synchronise), and the host loop, run once.  One
JSON line.

    python tools/bench_genes.py
"""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch
from scipy.stats import pearsonr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_eval import device_ms, host_ms  # noqa: E402
from genes_reference import reference_neglog10, tutorial_table  # noqa: E402
from mclstexp_amd import evaluate, genes, synth  # noqa: E402

SHAPES = [  # name, slide sizes, genes
    ("her2st: 32 slides x 785 genes", [300 + 13 * (i % 9) for i in range(32)], 785),
    ("10x-like: 9 slides x 685 genes", [2400 + 310 * (i % 9) for i in range(9)], 685),
]


def host_loop(preds, trues):
    """The tutorial's computation: pearsonr per gene per slide, -log10 p, the pandas table."""
    r, p = [], []
    for a, b in zip(preds, trues):
        rp = [pearsonr(a[:, g], b[:, g]) for g in range(a.shape[1])]
        r.append(np.array([x[0] for x in rp])), p.append(np.array([x[1] for x in rp]))
    r, p = np.stack(r), np.stack(p)
    S, G = r.shape
    tutorial_table(reference_neglog10(p), r, [str(g) for g in range(G)], [str(s) for s in range(S)])
    return p


def main():
    dev = torch.device("cuda")
    shapes = []
    for name, sizes, G in SHAPES:
        d = synth.make_eval_case(sizes, G, seed=1)
        off = d["offsets"]
        pred = torch.from_numpy(d["pred"]).float().to(dev)
        true = torch.from_numpy(d["true"]).float().to(dev)
        preds = [pred[off[s]:off[s + 1]] for s in range(len(sizes))]
        trues = [true[off[s]:off[s + 1]] for s in range(len(sizes))]
        r = evaluate.metrics_device(pred, true, off)["r"]
        off_d = torch.from_numpy(off).to(dev)
        p, nl = genes.pvalues_device(r, off_d)
        t_p = device_ms(lambda: genes.pvalues_device(r, off_d))
        t_rank = host_ms(lambda: genes.rank_genes(nl, r))
        t_table = host_ms(lambda: genes.significance_table(preds, trues))
        p_np = [x.cpu().double().numpy() for x in preds]
        t_np = [x.cpu().double().numpy() for x in trues]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            p_host = host_loop(p_np, t_np)
            t_host = (time.perf_counter() - t0) * 1e3
        shapes.append({"shape": name, "rows": int(off[-1]), "genes": G, "slides": len(sizes),
                       "pearson_pvalue_call_ms": round(t_p, 4), "rank_genes_ms": round(t_rank, 4),
                       "significance_table_ms": round(t_table, 4), "host_pearsonr_pandas_ms": round(t_host, 1),
                       "host_p_underflowed": int((p_host == 0.0).sum()),
                       "device_neglog10p_finite": int(np.isfinite(nl.cpu().numpy()).sum()), "elements": len(sizes) * G})
    print(json.dumps({"bench": "gene_significance", "device": torch.cuda.get_device_name(0), "shapes": shapes}), flush=True)


if __name__ == "__main__":
    main()
