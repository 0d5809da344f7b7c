#!/usr/bin/env python3
"""Micro-benchmark of the ligand-receptor permutation test (mclstexp_amd.ligrec) on one MI355X, on the two workloads the
other evaluation modules report -- 32 HER2ST-sized slides (300 - 700 spots x 785 genes, 15500 spots in all, 6 groups) and one
4000 x 3467 slide with 8 groups -- with 1000 permutations and 300 interactions over 200 genes, fp32 on the device.

Per workload, after warm-up, medians of repeated runs: ``ligrec_device`` end to end (host clock around a device synchronise;
it includes the index preparation, the allocations, the uploads and the status read-back), and each stage alone by HIP
events on the launch stream: ``mcl_ligrec_prepare``, the identity pass (the first ``mcl_ligrec_group_means`` call), the table
generation (``mcl_spatial_permutations``), the permuted passes (the other ``mcl_ligrec_group_means`` calls, THE HOT KERNEL),
``mcl_ligrec_observed`` and ``mcl_ligrec_count``.  For the hot kernel the achieved LDS read rate -- the P n fp64 values of
every column a workgroup holds (padding columns of the last tile included) over the pass time -- is given as a fraction of
the chip's ``ds_read_b64`` peak (150 TB/s), beside the table bytes it requests through L2 (one uint16 per (tile,
permutation, spot)).  HBM bytes were not read from counters.

The yardstick is the numpy restatement (tests/ligrec_reference.py: gather, group sums in the stated order, means, the
comparisons) on the host of the same machine, on at most 16 threads (one permutation per task).  It is timed on
``--host_perms`` permutations per workload and reported per permutation; the figure for P permutations is that times P and
is labelled as an extrapolation.

    python tools/bench_ligrec.py [--out FILE] [--no_host] [--perms 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ligrec_reference as lr  # noqa: E402
import spatial_reference as sr  # noqa: E402
from mclstexp_amd import _lib, ligrec  # noqa: E402

LDS_PEAK_BYTES_PER_S = 150e12      # ds_read_b64, every CU streaming
ENTRY_POINTS = ["mcl_ligrec_prepare", "mcl_ligrec_group_means", "mcl_spatial_permutations", "mcl_ligrec_observed",
                "mcl_ligrec_count"]
N_INTERACTIONS, N_GENES_USED = 300, 200
WORKLOADS = [  # name, slide sizes, genes, groups
    ("her2st: 32 slides x 785 genes, 6 groups", [300 + 50 * (i % 9) for i in range(32)], 785, 6),
    ("one 4000 x 3467 slide, 8 groups", [4000], 3467, 8),
]


def make(sizes, G, K, seed):
    rng = np.random.default_rng(seed)
    xs, labs = [], []
    for n in sizes:
        lab = rng.integers(0, K, n)
        x = rng.gamma(2.0, 1.0, (n, G)) * (rng.random((n, G)) < 0.5)
        x = x * (1.0 + 0.5 * ((lab[:, None] % 3) == (np.arange(G)[None, :] % 3)))
        xs.append(x.astype(np.float32))
        labs.append(lab.astype(np.int64))
    pool = rng.choice(G, N_GENES_USED, replace=False)
    inter = [(int(a), int(b)) for a, b in zip(rng.choice(pool, N_INTERACTIONS), rng.choice(pool, N_INTERACTIONS))]
    return np.concatenate(xs), np.concatenate(labs), inter


def host_ms_per_permutation(x, labels, off, inter, K, perms_timed, threads=16):
    """The restatement on the host: per slide the sorted used columns once, then per permutation the group sums in the
    stated order, the means and the comparisons."""
    sides = lr.expand(inter)
    used = lr.used_columns(sides)
    slides = []
    for s in range(off.size - 1):
        lab = labels[off[s]:off[s + 1]]
        order, start = lr.prepare(lab, K)
        xs = x[off[s]:off[s + 1]].astype(np.float64)[order][:, used]
        sums, _ = lr.group_stats(xs, start)
        mean = lr.group_means(sums, start)
        pairs = lr.choose(sides, used, sums, order.size)
        ia, ib = pairs[:, 0], pairs[:, 1]
        obs = (mean[:, ia].T[:, :, None] + mean[:, ib].T[:, None, :]) / 2.0
        slides.append((xs, start, ia, ib, obs))

    def one(p):
        out = []
        for xs, start, ia, ib, obs in slides:
            ps, _ = lr.group_stats(xs, start, sr.permutation(0, p, xs.shape[0]))
            pm = lr.group_means(ps, start)
            out.append((pm[:, ia].T[:, :, None] + pm[:, ib].T[:, None, :]) / 2.0 >= obs)
        return out
    one(0)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(perms_timed)))
    return (time.perf_counter() - t0) * 1e3 / perms_timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--perms", type=int, nargs="+", default=[1000])
    ap.add_argument("--host_perms", type=int, default=16)
    args = ap.parse_args()
    results = []
    for name, sizes, G, K in WORKLOADS:
        x, labels, inter = make(sizes, G, K, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        xd = torch.from_numpy(x).cuda()
        U = int(lr.used_columns(lr.expand(inter)).size)
        host = None if args.no_host else host_ms_per_permutation(x, labels, off, inter, K, args.host_perms)
        for P in args.perms:
            def run():
                return ligrec.ligrec_device(xd, labels, inter, off, K, n_perms=P, seed=0)
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            wall, per, ident, hot = [], {n: [] for n in ENTRY_POINTS}, [], []
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            for _ in range(args.runs):
                with _lib.AbiTimer(ENTRY_POINTS) as t:
                    run()
                summ = t.summary()
                for n, rec in summ.items():
                    per[n].append(rec["total_ms"])
                ident.append(summ["mcl_ligrec_group_means"]["ms"][0])
                hot.append(sum(summ["mcl_ligrec_group_means"]["ms"][1:]))
            med = {n: statistics.median(v) for n, v in per.items() if v}
            hot_ms = statistics.median(hot)
            n_arr = np.asarray(sizes, dtype=np.float64)
            cols = np.array([lr.columns(int(n)) for n in sizes], dtype=np.float64)
            tiles = np.ceil(U / cols)
            lds_bytes = float((P * n_arr * tiles * cols * 8).sum())
            l2_bytes = float((P * n_arr * tiles * 2).sum())
            r = {"workload": name, "rows": int(off[-1]), "genes": G, "groups": K, "interactions": len(inter), "used_genes": U,
                 "n_perms": P, "dtype": "float32", "chunk": int(d["chunk"]), "end_to_end_ms": statistics.median(wall),
                 "prepare_ms": med["mcl_ligrec_prepare"], "identity_pass_ms": statistics.median(ident),
                 "table_generation_ms": med["mcl_spatial_permutations"], "hot_kernel_ms": hot_ms,
                 "observed_ms": med["mcl_ligrec_observed"], "count_ms": med["mcl_ligrec_count"],
                 "additions": float((P * n_arr * U).sum()), "lds_read_bytes": lds_bytes,
                 "lds_read_bytes_per_s": lds_bytes / (hot_ms * 1e-3),
                 "lds_read_fraction_of_peak": lds_bytes / (hot_ms * 1e-3) / LDS_PEAK_BYTES_PER_S,
                 "l2_requested_table_bytes": l2_bytes, "hbm_bytes_measured": None}
            if host is not None:
                r.update(host_threads=16, host_perms_timed=args.host_perms, host_ms_per_permutation=host,
                         host_ms_extrapolated_to_n_perms=host * P, end_to_end_speedup_over_host_extrapolated=host * P / r["end_to_end_ms"],
                         hot_plus_count_speedup_over_host_extrapolated=host * P / (hot_ms + med["mcl_ligrec_count"]))
            results.append(r)
            print(f"{name}, P = {P}: end to end {r['end_to_end_ms']:.2f} ms, hot kernel {hot_ms:.2f} ms, count "
                  f"{r['count_ms']:.2f} ms", file=sys.stderr, flush=True)
    doc = {"bench": "ligrec", "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "lds_peak_bytes_per_s": LDS_PEAK_BYTES_PER_S, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
