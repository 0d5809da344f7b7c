#!/usr/bin/env python3
"""Micro-benchmark of the neighbourhood enrichment and co-occurrence of spot groups (mclstexp_amd.nhood) on one MI355X, on
the workloads the other evaluation modules report -- 32 HER2ST-sized slides (300 - 700 spots, 15500 in all, 6 groups) -- and
on one 4000-spot and one 16384-spot slide with 8 groups: the lattice of 8 neighbours, 1000 permutations, 50 radii.

Per workload, after warm-up, medians of repeated runs: ``nhood_device`` and ``co_occurrence`` end to end (host clock around a
device synchronise; allocations, uploads, the status read-back and, for ``co_occurrence``, the host's default radii and the
per-slide slicing of the results included; the lattice is built before), and each entry point alone by HIP events on the
launch stream: ``mcl_ligrec_prepare``, ``mcl_spatial_permutations``, ``mcl_nhood_counts`` (the compaction of the neighbour
list, the identity pass and the permuted passes: one unit; the same call with ``n_perms = 0`` gives the first two, the
difference THE HOT KERNEL), ``mcl_cooccur_counts`` (gather + THE PAIR KERNEL) and ``mcl_cooccur_scores``.  Rates: slot visits
per second of the hot kernel (P x slots x source-group tiles over its time) and ordered pairs per second of the pair kernel
(the sum of n^2 over its time).  No hardware counter was read.

The yardstick is the numpy restatement (tests/nhood_reference.py) on the host of the same machine, on at most 16 threads
(one permutation per task): the relabelling and the slot histogram are timed on ``--host_perms`` permutations and reported
per permutation; the figure for P permutations is that times P and is labelled as an extrapolation.  The pair pass of the
restatement is timed in full up to 4096 spots a slide; for a larger slide it is timed on its first 4096 spots and scaled by
the ratio of the pair counts, labelled as an extrapolation too.

    python tools/bench_nhood.py [--out FILE] [--no_host] [--perms 1000]
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
import nhood_reference as nh  # noqa: E402
import spatial_reference as sr  # noqa: E402
from mclstexp_amd import _lib, nhood, spatial  # noqa: E402

ENTRY_POINTS = ["mcl_ligrec_prepare", "mcl_spatial_permutations", "mcl_nhood_counts", "mcl_cooccur_counts", "mcl_cooccur_scores"]
K_GRAPH, RADII, HOST_PAIR_SPOTS = 8, 50, 4096
WORKLOADS = [  # name, slide sizes, groups
    ("her2st: 32 slides, 6 groups", [300 + 50 * (i % 9) for i in range(32)], 6),
    ("one 4000-spot slide, 8 groups", [4000], 8),
    ("one 16384-spot slide, 8 groups", [16384], 8),
]


def make(sizes, K, seed):
    """Jittered square lattices; the groups are K vertical bands with a fifth of the spots relabelled at random."""
    rng = np.random.default_rng(seed)
    cs, labs = [], []
    for n in sizes:
        side = int(np.ceil(np.sqrt(n)))
        c = sr.make_coords(side, side, int(rng.integers(1 << 30)))[:n]
        lab = np.minimum((c[:, 0] + 0.5) * K / side, K - 1).astype(np.int64).clip(0)
        noise = rng.random(n) < 0.2
        lab[noise] = rng.integers(0, K, int(noise.sum()))
        cs.append(c)
        labs.append(lab)
    return np.concatenate(cs), np.concatenate(labs)


def host_nhood_ms_per_permutation(labels, nbr, w, off, K, perms_timed, threads=16):
    slides = []
    for s in range(off.size - 1):
        lab = labels[off[s]:off[s + 1]]
        order, start = lr.prepare(lab, K)
        slides.append((lab, order, start, nbr[off[s]:off[s + 1]], w[off[s]:off[s + 1]]))

    def one(p):
        return [nh.counts(nh.relabel(lab, order, start, sr.permutation(0, p, order.size)), nb, ww, K)[0]
                for lab, order, start, nb, ww in slides]
    one(0)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(perms_timed)))
    return (time.perf_counter() - t0) * 1e3 / perms_timed


def host_pairs_ms(coords, labels, off, K, radii):
    """(ms, extrapolated?) of the restatement's pair pass over all slides."""
    ms, extrapolated = 0.0, False
    for s in range(off.size - 1):
        c, lab = coords[off[s]:off[s + 1]], labels[off[s]:off[s + 1]]
        m = min(c.shape[0], HOST_PAIR_SPOTS)
        t0 = time.perf_counter()
        nh.pair_counts(c[:m], lab[:m], K, radii[s])
        dt = (time.perf_counter() - t0) * 1e3
        if m < c.shape[0]:
            dt, extrapolated = dt * (c.shape[0] / m) ** 2, True
        ms += dt
    return ms, extrapolated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--host_perms", type=int, default=8)
    args = ap.parse_args()
    P = args.perms
    results = []
    for name, sizes, K in WORKLOADS:
        coords, labels = make(sizes, K, seed=1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        graph = spatial.lattice(coords, off, k=K_GRAPH, prune="NA")
        nbr, w = graph["nbr"].cpu().numpy(), graph["w"].cpu().numpy()
        S = len(sizes)

        def run_nhood(p=P):
            return nhood.nhood_device(labels, graph, K, n_perms=p, seed=0)

        def run_cc():
            return nhood.co_occurrence(coords, labels, off, K, radii=RADII)

        for _ in range(2):
            run_nhood()
            cc = run_cc()
        torch.cuda.synchronize()
        wall_n, wall_c, per, ident = [], [], {n: [] for n in ENTRY_POINTS}, []
        for _ in range(args.runs):
            for fn, wall in ((run_nhood, wall_n), (run_cc, wall_c)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
        for _ in range(args.runs):
            with _lib.AbiTimer(ENTRY_POINTS) as t:
                run_nhood()
                run_cc()
            for n, rec in t.summary().items():
                per[n].append(rec["total_ms"])
            with _lib.AbiTimer(["mcl_nhood_counts"]) as t:
                run_nhood(0)
            ident.append(t.summary()["mcl_nhood_counts"]["total_ms"])
        med = {n: statistics.median(v) for n, v in per.items() if v}
        n_arr = np.asarray(sizes, dtype=np.float64)
        tiles = np.array([-(-K // nh.tile_rows(n, K)) for n in sizes], dtype=np.float64)
        hot_ms = med["mcl_nhood_counts"] - statistics.median(ident)
        visits = float((P * n_arr * K_GRAPH * tiles).sum())
        pairs = float((n_arr * n_arr).sum())
        r = {"workload": name, "rows": int(off[-1]), "slides": S, "groups": K, "graph_k": K_GRAPH, "n_perms": P, "radii": RADII,
             "neighbour_list_staged_in_lds": [bool(nh.staged(n, K, K_GRAPH)) for n in sorted(set(sizes))],
             "nhood_end_to_end_ms": statistics.median(wall_n), "co_occurrence_end_to_end_ms": statistics.median(wall_c),
             "prepare_ms_both_calls": med["mcl_ligrec_prepare"], "table_generation_ms": med["mcl_spatial_permutations"],
             "nhood_counts_ms": med["mcl_nhood_counts"], "compact_and_identity_ms": statistics.median(ident),
             "hot_kernel_ms": hot_ms, "slot_visits": visits, "slot_visits_per_s": visits / (hot_ms * 1e-3),
             "cooccur_counts_ms": med["mcl_cooccur_counts"], "cooccur_scores_ms": med["mcl_cooccur_scores"],
             "ordered_pairs": pairs, "ordered_pairs_per_s": pairs / (med["mcl_cooccur_counts"] * 1e-3),
             "counters_read": None}
        if not args.no_host:
            host = host_nhood_ms_per_permutation(labels, nbr, w, off, K, args.host_perms)
            hp, extrapolated = host_pairs_ms(coords, labels, off, K, [c["radii"] for c in cc])
            r.update(host_threads=16, host_perms_timed=args.host_perms, host_nhood_ms_per_permutation=host,
                     host_nhood_ms_extrapolated_to_n_perms=host * P,
                     nhood_end_to_end_speedup_over_host_extrapolated=host * P / r["nhood_end_to_end_ms"],
                     host_pairs_ms=hp, host_pairs_extrapolated_from_4096_spots=extrapolated,
                     co_occurrence_end_to_end_speedup_over_host=hp / r["co_occurrence_end_to_end_ms"])
        results.append(r)
        print(f"{name}: nhood end to end {r['nhood_end_to_end_ms']:.2f} ms (hot kernel {hot_ms:.2f} ms), co-occurrence "
              f"{r['co_occurrence_end_to_end_ms']:.2f} ms (pair kernel {r['cooccur_counts_ms']:.2f} ms)", file=sys.stderr, flush=True)
    doc = {"bench": "nhood", "device": torch.cuda.get_device_name(0), "runs": args.runs, "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
