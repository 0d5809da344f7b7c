#!/usr/bin/env python3
"""Micro-benchmark of rank scoring (mclstexp_amd.rank: Spearman's rho, Kendall's tau-b) on one MI355X, on two workloads: 32
HER2ST-sized slides (300 - 700 spots x 785 genes, 15 500 rows) and one 4000 x 3467 slide, fp32 on the device,
zero-inflated on every other slide.

Per workload, after warm-up, medians of ``--runs`` (20) runs: ``rank_device`` end to end (host clock around a device
synchronise; it includes the allocations, the offsets' upload and the status read-back) and each entry point alone (HIP
events on the launch stream), with and without tau, and for ``axis="spots"``.  The rank and the pair phase share one launch
(``mcl_rank_stats``; the ranks never leave LDS), so the rank phase is that launch without tau and the pair phase the
difference to the launch with it.  Two yardsticks: the rank phase against the marker rank kernel's recorded time on the same
shapes (profiles/markers.json: one sort with a 1-byte payload there, two sorts with a 2-byte payload here), and the pair
phase's pairs per second against the rate at which the LDS serves broadcast reads (one ds_read_b32 per wave and 64 pairs,
two LDS cycles each, 256 CUs at 2.4 GHz).  Beside them the host time of the same quantities on the same machine:
``scipy.stats.spearmanr`` and ``kendalltau`` column by column on 16 processes, measured before the GPU is opened.  One JSON
line; ``--out profiles/rank.json`` records it.

    python tools/bench_rank.py [--out FILE] [--no_host] [--runs 20]
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_PROCESSES = 16
CUS, CLOCK_HZ = 256, 2.4e9
LDS_BROADCAST_PAIRS_PER_S = CUS * CLOCK_HZ / 2 * 64        # one ds_read_b32 wave instruction = 2 LDS cycles, 64 pairs
MARKERS_PROFILE = os.path.join(ROOT, "profiles", "markers.json")
ENTRY_POINTS = ["mcl_rank_stats", "mcl_rank_finish", "mcl_pearson_pvalue"]
WORKLOADS = [  # key, name, slide sizes, genes
    ("her2st", "her2st: 32 slides x 785 genes", [300 + 50 * (i % 9) for i in range(32)], 785),
    ("visium", "one 4000 x 3467 slide", [4000], 3467),
]


def marker_rank_ms():
    """{workload key: the marker rank kernel's recorded ms} read from profiles/markers.json, matched by (rows, genes)."""
    with open(MARKERS_PROFILE) as fh:
        recorded = {(r["rows"], r["genes"]): r["entry_points_ms"]["mcl_marker_rank_sums"] for r in json.load(fh)["results"]}
    return {key: recorded[(sum(sizes), G)] for key, _, sizes, G in WORKLOADS}


def make(sizes, G, seed):
    """float32 (rows, G) pred / true: log-normalised-count-like, every other slide zero-inflated."""
    rng = np.random.default_rng(seed)
    ps, ts = [], []
    for i, n in enumerate(sizes):
        base = rng.normal(size=(n, G))
        t = np.log1p(np.round(np.exp(base + 1.0)))
        p = np.maximum(base + 1.0 + 0.8 * rng.normal(size=(n, G)), 0.0)
        if i % 2:
            t[rng.random((n, G)) < 0.5] = 0.0
        ps.append(p.astype(np.float32)), ts.append(t.astype(np.float32))
    return np.concatenate(ps), np.concatenate(ts)


_HOST = {}


def _host_column(job):
    from scipy import stats
    s, g, tau = job
    pred, true, off = _HOST["pred"], _HOST["true"], _HOST["off"]
    x, y = pred[off[s]:off[s + 1], g], true[off[s]:off[s + 1], g]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = stats.spearmanr(x, y).statistic
        if tau:
            stats.kendalltau(x, y, method="asymptotic")
    return r


def host_seconds(pred, true, off):
    """(spearmanr only, spearmanr + kendalltau) wall seconds of the scipy loop on HOST_PROCESSES forked processes."""
    _HOST.update(pred=pred, true=true, off=off)
    out = []
    with multiprocessing.get_context("fork").Pool(HOST_PROCESSES) as pool:
        pool.map(_host_column, [(0, g % pred.shape[1], True) for g in range(4 * HOST_PROCESSES)], chunksize=1)   # imports
        for tau in (False, True):
            jobs = [(s, g, tau) for s in range(off.size - 1) for g in range(pred.shape[1])]
            t0 = time.perf_counter()
            pool.map(_host_column, jobs, chunksize=64)
            out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    marker_ms = marker_rank_ms()
    data, host = {}, {}
    for key, _, sizes, G in WORKLOADS:                      # the host loop first: its processes never see the GPU
        pred, true = make(sizes, G, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        data[key] = (pred, true, off)
        if not args.no_host:
            host[key] = host_seconds(pred, true, off)

    import torch
    from mclstexp_amd import _lib, rank

    def measure(run):
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
        return statistics.median(wall), {n: statistics.median(v) for n, v in per.items()}

    results = []
    for key, name, sizes, G in WORKLOADS:
        pred, true, off = data[key]
        pd, td, offl = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda(), off.tolist()
        r = {"workload": name, "rows": int(off[-1]), "genes": G, "dtype": "float32"}
        for label, axis, tau in (("genes_tau", "genes", True), ("genes_no_tau", "genes", False),
                                 ("spots_tau", "spots", True), ("spots_no_tau", "spots", False)):
            wall, per = measure(lambda: rank.rank_device(pd, td, offl if axis == "genes" else None, axis, tau))
            r[label] = {"end_to_end_ms": wall, "entry_points_ms": per}
        n = np.diff(off).astype(np.float64)
        for axis, pairs in (("genes", float((n * (n - 1) / 2).sum() * G)), ("spots", float(off[-1]) * G * (G - 1) / 2)):
            rank_ms = r[f"{axis}_no_tau"]["entry_points_ms"]["mcl_rank_stats"]
            pair_ms = r[f"{axis}_tau"]["entry_points_ms"]["mcl_rank_stats"] - rank_ms
            r[f"{axis}_phases"] = {"rank_phase_ms": rank_ms, "pair_phase_ms": pair_ms, "pairs": pairs,
                                   "pairs_per_s": pairs / (pair_ms * 1e-3),
                                   "of_lds_broadcast_rate": pairs / (pair_ms * 1e-3) / LDS_BROADCAST_PAIRS_PER_S}
        r["marker_rank_kernel_ms"] = marker_ms[key]
        r["rank_phase_over_marker_rank_kernel"] = r["genes_phases"]["rank_phase_ms"] / marker_ms[key]
        if key in host:
            r.update(host_processes=HOST_PROCESSES, host_spearmanr_ms=host[key][0] * 1e3,
                     host_spearmanr_kendalltau_ms=host[key][1] * 1e3)
        results.append(r)
    doc = {"bench": "rank", "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "lds_broadcast_pairs_per_s": LDS_BROADCAST_PAIRS_PER_S, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
