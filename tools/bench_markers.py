#!/usr/bin/env python3
"""Micro-benchmark of marker-gene ranking (mclstexp_amd.markers, Wilcoxon, all genes) on one MI355X, on two workloads: 32
HER2ST-sized slides (300 - 700 spots x 785 genes, 6 groups) and one 4000 x 3467 slide with 8 groups, fp32 on the device.

Per workload, after warm-up, medians of repeated runs: ``rank_genes_groups_device`` end to end (host clock around a device
synchronise; it includes the allocations, the uploads of offsets / labels and the status read-back), each of the four
entry points alone (HIP events on the launch stream), and the rank kernel's time against reading ``x`` once at the HBM rate
(6.29 TB/s, the measured float4-copy rate of the MI355X).  Beside them the host time of the same quantities on the same
machine, run once: ``scipy.stats.rankdata`` per column, then the restatement tests/markers_reference.py.  One JSON line;
``--out profiles/markers.json`` records it.

    python tools/bench_markers.py [--out FILE] [--no_host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import markers_reference as mr  # noqa: E402
from mclstexp_amd import _lib, markers  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
ENTRY_POINTS = ["mcl_marker_stats", "mcl_marker_rank_sums", "mcl_marker_test", "mcl_marker_rank_adjust"]
WORKLOADS = [  # name, slide sizes, genes, groups
    ("her2st: 32 slides x 785 genes, 6 groups", [300 + 50 * (i % 9) for i in range(32)], 785, 6),
    ("one 4000 x 3467 slide, 8 groups", [4000], 3467, 8),
]


def make(sizes, G, k, seed):
    parts = [mr.make_case(n, G, k, seed + i, kind="zeros" if i % 2 else "cont", dtype=np.float32) for i, n in enumerate(sizes)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def host_seconds(x, labels, off, k):
    t0 = time.perf_counter()
    for s in range(off.size - 1):
        xs = x[off[s]:off[s + 1]].astype(np.float64)
        for j in range(xs.shape[1]):
            stats.rankdata(xs[:, j])
    t1 = time.perf_counter()
    for s in range(off.size - 1):
        mr.rank_genes_groups(x[off[s]:off[s + 1]], labels[off[s]:off[s + 1]], k)
    return t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    results = []
    for name, sizes, G, k in WORKLOADS:
        x, labels = make(sizes, G, k, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        xd = torch.from_numpy(x).cuda()
        ks = [k] * len(sizes)

        def run():
            return markers.rank_genes_groups_device(xd, labels, off, ks)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        wall, per = [], {n: [] for n in ENTRY_POINTS}
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        for _ in range(args.runs):
            with _lib.AbiTimer(ENTRY_POINTS) as t:
                run()
            for n, rec in t.summary().items():
                per[n].append(rec["total_ms"])
        rank_ms = statistics.median(per["mcl_marker_rank_sums"])
        read_ms = x.nbytes / HBM_BYTES_PER_S * 1e3
        r = {"workload": name, "rows": int(off[-1]), "genes": G, "groups": k, "dtype": "float32",
             "end_to_end_ms": statistics.median(wall),
             "entry_points_ms": {n: statistics.median(v) for n, v in per.items()},
             "x_bytes": int(x.nbytes), "read_x_once_at_hbm_rate_ms": read_ms, "rank_kernel_over_read_once": rank_ms / read_ms}
        if not args.no_host:
            t_rank, t_rest = host_seconds(x, labels, off, k)
            r.update(host_rankdata_per_column_ms=t_rank * 1e3, host_restatement_ms=t_rest * 1e3)
        results.append(r)
    doc = {"bench": "markers", "device": torch.cuda.get_device_name(0), "runs": args.runs, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "results": results}
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
