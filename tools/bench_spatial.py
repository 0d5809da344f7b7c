#!/usr/bin/env python3
"""Micro-benchmark of the spatial autocorrelation (mclstexp_amd.spatial, k = 8, row-standardised, Moran and Geary together)
on one MI355X, on two workloads -- 32 HER2ST-sized slides (300 - 700 spots x 785 genes, 15500 spots in all) and one
4000 x 3467 slide -- with P = 100 and P = 1000 permutations, fp32 on the device.

Per workload and P, after warm-up, medians of repeated runs: ``lattice`` + ``autocorr_device`` end to end (host clock around
a device synchronise; it includes the kNN search, the allocations, the uploads and the status read-backs), and each stage
alone by HIP events on the launch stream: the graph (``mcl_knn_exact`` + ``mcl_spatial_lattice``), the observed pass (the
first ``mcl_spatial_stats`` call), the table generation (``mcl_spatial_permutations``), the permutation pass (the second
``mcl_spatial_stats`` call), the moments and the summary.  For the permutation pass the achieved LDS gather rate -- the
P n (k + 1) G fp64 values a workgroup reads out of LDS, over the pass time -- is given as a fraction of the chip's
``ds_read_b64`` peak (150 TB/s), beside the bytes the pass requests through L2 (table, nbr and w once per (workgroup,
permutation)) and the HBM floor "x once + table".  HBM bytes were not read from counters.

The yardstick is the same computation on the host of the same machine: ``scipy.sparse`` W against the gathered, centred
matrix, on at most 16 threads (one permutation per task).  It is timed on ``--host_perms`` permutations per workload and
reported per permutation; the figure for P permutations is that times P and is labelled as an extrapolation.

    python tools/bench_spatial.py [--out FILE] [--no_host] [--perms 100 1000]
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
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spatial_reference as sr  # noqa: E402
from mclstexp_amd import _lib, spatial  # noqa: E402

LDS_PEAK_BYTES_PER_S = 150e12      # ds_read_b64, every CU streaming
HBM_BYTES_PER_S = 6.29e12
K = 8
ENTRY_POINTS = ["mcl_knn_exact", "mcl_spatial_lattice", "mcl_spatial_stats", "mcl_spatial_permutations",
                "mcl_spatial_moments", "mcl_spatial_perm_summary"]
WORKLOADS = [  # name, slide sizes, genes
    ("her2st: 32 slides x 785 genes", [300 + 50 * (i % 9) for i in range(32)], 785),
    ("one 4000 x 3467 slide", [4000], 3467),
]


def make(sizes, G, seed):
    cs, xs = [], []
    for i, n in enumerate(sizes):
        side = int(np.ceil(np.sqrt(n * 1.1)))
        c = sr.make_coords(side, side, seed + i)
        c = c[np.random.default_rng(seed + i).permutation(c.shape[0])[:n]]
        rng = np.random.default_rng(seed + 1000 + i)
        u = c / c.max()
        smooth = np.sin(3.0 * u[:, :1] + rng.uniform(0, 6, (1, G))) * np.linspace(1, 0, G)[None]
        xs.append((smooth + rng.normal(size=(n, G)) + 2.5).astype(np.float32))
        cs.append(c)
    return np.concatenate(cs), np.concatenate(xs)


def host_ms_per_permutation(coords, x, off, perms_timed, threads=16):
    """The restatement's sparse form on the host: per slide W (CSR) against the gathered centred matrix; I and C."""
    slides = []
    for s in range(off.size - 1):
        g = sr.lattice(coords[off[s]:off[s + 1]], K, "NA", True)
        n = g["nbr"].shape[0]
        W = sparse.csr_matrix((g["w"].ravel(), g["nbr"].ravel(), np.arange(0, n * K + 1, K)), shape=(n, n))
        xs = x[off[s]:off[s + 1]].astype(np.float64)
        z = xs - xs.mean(axis=0)
        slides.append((W, np.asarray(W.sum(axis=1)).ravel()[:, None], np.asarray(W.sum(axis=0)).ravel()[:, None], z,
                       (z * z).sum(axis=0), g["S0"]))

    def one(p):
        out = []
        for W, rs, cs, z, den, S0 in slides:
            n = z.shape[0]
            zp = z[sr.permutation(0, p, n)]
            lag = W @ zp
            nI = (zp * lag).sum(axis=0)
            z2 = zp * zp
            nC = (rs * z2).sum(axis=0) - 2.0 * nI + (cs * z2).sum(axis=0)
            out.append(((n / S0) * nI / den, ((n - 1) / (2 * S0)) * nC / den))
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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--perms", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--host_perms", type=int, default=16)
    args = ap.parse_args()
    results = []
    for name, sizes, G in WORKLOADS:
        coords, x = make(sizes, G, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(coords).cuda()
        host = None if args.no_host else host_ms_per_permutation(coords, x, off, args.host_perms)
        for P in args.perms:
            def run():
                g = spatial.lattice(cd, off, K, "NA", True)
                return spatial.autocorr_device(xd, g, n_perms=P, seed=0)
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            wall, per = [], {n: [] for n in ENTRY_POINTS}
            obs, perm = [], []
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            for _ in range(args.runs):
                with _lib.AbiTimer(ENTRY_POINTS) as t:
                    run()
                summ = t.summary()
                for n, rec in summ.items():
                    per[n].append(rec["total_ms"])
                obs.append(summ["mcl_spatial_stats"]["ms"][0])
                perm.append(summ["mcl_spatial_stats"]["ms"][1])
            med = {n: statistics.median(v) for n, v in per.items() if v}
            perm_ms = statistics.median(perm)
            n_arr = np.asarray(sizes, dtype=np.float64)
            cols = np.array([sr.columns(int(n)) for n in sizes], dtype=np.float64)
            groups = np.ceil(G / cols)
            gathered = float((P * n_arr * (K + 1) * G * 8).sum())
            l2_bytes = float((groups * P * n_arr * (2 * (K + 1) + K * 12)).sum())     # table (uint16) + nbr + w per (workgroup, p)
            floor = float(x.nbytes + P * n_arr.sum() * 2)
            r = {"workload": name, "rows": int(off[-1]), "genes": G, "k": K, "n_perms": P, "dtype": "float32",
                 "end_to_end_ms": statistics.median(wall),
                 "graph_ms": med["mcl_knn_exact"] + med["mcl_spatial_lattice"], "observed_pass_ms": statistics.median(obs),
                 "table_generation_ms": med["mcl_spatial_permutations"], "permutation_pass_ms": perm_ms,
                 "moments_ms": med["mcl_spatial_moments"], "summary_ms": med["mcl_spatial_perm_summary"],
                 "multiply_adds": float((P * n_arr * K * G).sum()),
                 "lds_gathered_bytes": gathered, "lds_gather_bytes_per_s": gathered / (perm_ms * 1e-3),
                 "lds_gather_fraction_of_peak": gathered / (perm_ms * 1e-3) / LDS_PEAK_BYTES_PER_S,
                 "l2_requested_bytes": l2_bytes, "hbm_floor_bytes_x_once_plus_table": floor,
                 "hbm_floor_ms": floor / HBM_BYTES_PER_S * 1e3, "hbm_bytes_measured": None}
            if host is not None:
                r.update(host_threads=16, host_perms_timed=args.host_perms, host_ms_per_permutation=host,
                         host_ms_extrapolated_to_n_perms=host * P,
                         permutation_pass_speedup_over_host_extrapolated=host * P / perm_ms)
            results.append(r)
            print(f"{name}, P = {P}: end to end {r['end_to_end_ms']:.2f} ms, permutation pass {perm_ms:.2f} ms", file=sys.stderr,
                  flush=True)
    doc = {"bench": "spatial", "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "lds_peak_bytes_per_s": LDS_PEAK_BYTES_PER_S, "hbm_bytes_per_s": HBM_BYTES_PER_S, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
