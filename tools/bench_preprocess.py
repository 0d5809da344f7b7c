#!/usr/bin/env python3
"""Micro-benchmark of the count-table preprocessing (mclstexp_amd.preprocess) on one MI355X at the reference's dataset
sizes.  Per shape: the one ``mcl_hvg_stats`` call (HIP events around the C entry point: its four launches),
``gene_stats`` end to end (descriptor upload, the call, the status read-back; host clock), the one
``mcl_expression_matrices`` call, and for scale the same moments as separate torch calls on the device (cast to fp64,
row sums, median, divide, ``mean``, ``var`` per slide).  Bytes: the statistics read every count twice (library sizes,
moments); the matrices read the chosen columns twice and write them once; GB/s against the 8 TB/s HBM peak DESIGN.md
uses.  Counts are Poisson draws made on the device (speed does not depend on the values).  One JSON line per shape.

    python tools/bench_preprocess.py [--small]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mclstexp_amd import _lib, preprocess  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [  # name, spots per slide, genes, genes kept in the matrices
    ("her2st: 32 slides x ~400 spots x 15000 genes", [340 + 17 * (i % 8) for i in range(32)], 15000, 785),
    ("visium: 9 slides x ~4000 spots x 30000 genes", [3600 + 100 * (i % 9) for i in range(9)], 30000, 3467),
]
SMALL = [("small: 4 slides x ~300 spots x 2000 genes", [250, 300, 350, 400], 2000, 171)]


def make_slides(sizes, G, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    mean = torch.exp(torch.rand(G, device=dev, generator=g) * 6.5 - 4.0)
    out = []
    for n in sizes:
        depth = 0.5 + 1.5 * torch.rand(n, 1, device=dev, generator=g)
        out.append(torch.poisson(depth * mean[None, :], generator=g).to(torch.int32))
    return out


def abi_ms(name, fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    with _lib.AbiTimer([name]) as t:
        for _ in range(iters):
            fn()
    return t.summary()[name]["avg_ms"]


def host_ms(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def torch_moments(slides):
    for c in slides:
        x = c.double()
        s = x.sum(1)
        f = s / s[s > 0].median()
        f[f == 0] = 1.0
        x = x / f[:, None]
        x.mean(0), x.var(0)


def main():
    dev = torch.device("cuda")
    for name, sizes, G, K in (SMALL if "--small" in sys.argv else SHAPES):
        slides = make_slides(sizes, G, dev)
        genes = np.sort(np.random.default_rng(0).choice(G, K, replace=False))
        counts = int(sum(sizes)) * G
        t_stats = abi_ms("mcl_hvg_stats", lambda: preprocess.gene_stats(slides))
        t_e2e = host_ms(lambda: preprocess.gene_stats(slides))
        t_mats = abi_ms("mcl_expression_matrices", lambda: preprocess.expression_matrices(slides, None, genes))
        t_torch = host_ms(lambda: torch_moments(slides), iters=3, warm=1)
        stats_bytes = 2 * counts * 4 + len(sizes) * G * (3 * 8 + 4 + 1)
        mats_bytes = 3 * int(sum(sizes)) * K * 4
        gbs = lambda b, ms: b / (ms * 1e-3) / 1e9  # noqa: E731
        print(json.dumps({"shape": name, "slides": len(sizes), "spots": int(sum(sizes)), "genes": G, "kept": K,
                          "hvg_stats_call_ms": round(t_stats, 4), "gene_stats_end_to_end_ms": round(t_e2e, 4),
                          "hvg_stats_GBps": round(gbs(stats_bytes, t_stats), 1),
                          "hvg_stats_frac_of_hbm_peak": round(gbs(stats_bytes, t_stats) / HBM_PEAK_GBS, 4),
                          "expression_matrices_call_ms": round(t_mats, 4),
                          "expression_matrices_GBps": round(gbs(mats_bytes, t_mats), 1),
                          "torch_moments_ms": round(t_torch, 3)}), flush=True)
        del slides
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
