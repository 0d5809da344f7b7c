#!/usr/bin/env python3
"""Micro-benchmark of the local spatial statistics (mclstexp_amd.hotspot: local Moran, Gi*, conditional permutation test;
k = 8, row-standardised, 999 draws, all genes, univariate) on one MI355X, on two workloads -- 32 HER2ST-sized slides
(300 - 700 spots x 785 genes, 15500 spots in all) and one 4000 x 3467 slide --, fp32 on the device.

Per workload, after warm-up, medians of ``--runs`` (20) runs: ``local_stats_device`` end to end on a graph that is already
built (host clock around a device synchronise; it includes the allocations, the pair upload and the status read-back), and
each stage alone by HIP events on the launch stream: ``mcl_hotspot_moments``, ``mcl_hotspot_permute`` (THE HOT KERNEL, draws
generated in the kernel) and ``mcl_hotspot_finalise``.  The same is timed with the draws materialised first and streamed
from the table (``mcl_hotspot_draws`` + ``mcl_hotspot_permute`` reading it): the alternative DESIGN 6.22 weighs.  For the hot
kernel the achieved LDS gather rate -- the (P + 1) n d G fp64 values the workgroups read out of LDS, over its time -- is given
as a fraction of the chip's ``ds_read_b64`` peak (150 TB/s).  No counter was read.

The yardstick is the same computation on the host of the same machine: ``tests/hotspot_reference.py``'s permutation pass
(numpy gathers, one (slide, 128-gene block) per task) on 16 threads.  It is timed on ``--host_draws`` draws per workload and
reported per draw; the figure for 999 draws is that times 999 and is labelled as an extrapolation.

    python tools/bench_hotspot.py [--out FILE] [--no_host] [--runs 20]
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
import hotspot_reference as hr  # noqa: E402
import spatial_reference as sr  # noqa: E402
from bench_spatial import WORKLOADS, make  # noqa: E402
from mclstexp_amd import _lib, hotspot, spatial  # noqa: E402

LDS_PEAK_BYTES_PER_S = 150e12      # ds_read_b64, every CU streaming
K, P = 8, 999
ENTRY_POINTS = ["mcl_hotspot_moments", "mcl_hotspot_draws", "mcl_hotspot_permute", "mcl_hotspot_finalise"]
BLOCK = 128


def host_ms_per_draw(x, off, nbr, w, draws_timed, threads=16):
    """The restatement's permutation pass on the host, one (slide, gene block) per task."""
    tasks = []
    for s in range(off.size - 1):
        a, b = int(off[s]), int(off[s + 1])
        _, _, z = sr.centre(x[a:b].astype(np.float64))
        L, kept, _ = hr.neighbour_sum(z, nbr[a:b], w[a:b])
        deg = np.minimum(kept, b - a - 1)
        table = hr.draw_table(0, draws_timed, b - a, deg, K)
        for j in range(0, z.shape[1], BLOCK):
            tasks.append((np.ascontiguousarray(z[:, j:j + BLOCK]), np.ascontiguousarray(L[:, j:j + BLOCK]), deg, table))
    hr.permutation_pass(*tasks[0])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(lambda t: hr.permutation_pass(*t)[:4], tasks))
    return (time.perf_counter() - t0) * 1e3 / draws_timed


def timed(run, runs):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    wall, per = [], {n: [] for n in ENTRY_POINTS}
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    for _ in range(runs):
        with _lib.AbiTimer(ENTRY_POINTS) as t:
            run()
        for n, rec in t.summary().items():
            per[n].append(rec["total_ms"])
    return statistics.median(wall), {n: statistics.median(v) for n, v in per.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host_draws", type=int, default=4)
    args = ap.parse_args()
    results = []
    for name, sizes, G in WORKLOADS:
        coords, x = make(sizes, G, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        xd = torch.from_numpy(x).cuda()
        g = spatial.lattice(torch.from_numpy(coords).cuda(), off, K, "NA", True)
        wall, med = timed(lambda: hotspot.local_stats_device(xd, g, n_perms=P, seed=0), args.runs)
        wall_t, med_t = timed(lambda: hotspot.local_stats_device(xd, g, n_perms=P, seed=0, return_draws=True), args.runs)
        n_arr = np.asarray(sizes, dtype=np.float64)
        gathered = float(((P + 1) * n_arr * K * G * 8).sum())
        hot = med["mcl_hotspot_permute"]
        r = {"workload": name, "rows": int(off[-1]), "genes": G, "k": K, "n_perms": P, "dtype": "float32",
             "end_to_end_ms": wall, "moments_ms": med["mcl_hotspot_moments"], "hot_kernel_ms": hot,
             "finalise_ms": med["mcl_hotspot_finalise"], "gathers": float((P * n_arr * K * G).sum()),
             "lds_gathered_bytes": gathered, "lds_gather_bytes_per_s": gathered / (hot * 1e-3),
             "lds_gather_fraction_of_peak": gathered / (hot * 1e-3) / LDS_PEAK_BYTES_PER_S,
             "materialised_end_to_end_ms": wall_t, "materialised_draws_ms": med_t["mcl_hotspot_draws"],
             "materialised_hot_kernel_ms": med_t["mcl_hotspot_permute"],
             "materialised_table_bytes": float(P * n_arr.sum() * K * 2), "hbm_bytes_measured": None}
        if not args.no_host:
            host = host_ms_per_draw(x, off, g["nbr"].cpu().numpy(), g["w"].cpu().numpy(), args.host_draws)
            r.update(host_threads=16, host_draws_timed=args.host_draws, host_ms_per_draw=host,
                     host_ms_extrapolated_to_n_perms=host * P, hot_kernel_speedup_over_host_extrapolated=host * P / hot)
        results.append(r)
        print(f"{name}: end to end {wall:.2f} ms, hot kernel {hot:.2f} ms (table streamed: {med_t['mcl_hotspot_permute']:.2f} "
              f"+ {med_t['mcl_hotspot_draws']:.2f} ms)", file=sys.stderr, flush=True)
    doc = {"bench": "hotspot", "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "lds_peak_bytes_per_s": LDS_PEAK_BYTES_PER_S, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
