"""Leiden clustering (mclstexp_amd.leiden: csrc/leiden.hip) at two shapes on synthetic Gaussian blobs: BLEEP's (9269 rows as
one slide, D = 50, k = 150) and 8 slides of 3000 rows.  Prints one JSON line and, with --out, writes it: per shape the
wall time of leiden() (median, smallest and largest of --calls calls after a warm-up; it ends in device reads, so the clock
covers the device), the counters, and the sweep launch group of level 0 timed alone with HIP events on the launch stream
(mcl_leiden_move_sweeps with one sweep: ld_zero_move, ld_sweep, ld_tally_move, ld_q_move) with the bytes it must read and the
rate that gives.  The graph is built once by neighbors.neighbors and is not in any figure.  There is no pass / fail time.

A level-0 sweep must read, per stored entry, the column index (4 bytes) and the fixed-point weight (8) in ld_sweep and again
in ld_tally_move, and per row two row pointers (16), k_i (8) and the label (4); the gathered labels and tot_c are not counted
(they hit in cache or they do not: this is the floor).

    python tools/bench_leiden.py [--out profiles/leiden_bench.txt] [--calls 5] [--networkx]

--networkx adds, for orientation, the CPU time of networkx.community.louvain_communities (seed 0) on the same graphs where
networkx is installed (minutes at these sizes).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"bleep_9269": (np.array([9269]), 50, 150), "eight_3000": (np.array([3000] * 8), 50, 150)}


def blobs(seg, D, seed=0):
    rng = np.random.RandomState(seed)
    xs = []
    for n in seg:
        centres = 4.0 * rng.standard_normal((7, D))
        xs.append(centres[np.arange(n) % 7] + rng.standard_normal((n, D)))
    return np.concatenate(xs)


def sweep_bytes(rows, nnz):
    return 2 * nnz * (4 + 8) + rows * (16 + 8 + 4) * 2


def run(calls, with_networkx):
    import torch
    from mclstexp_amd import _lib, leiden, neighbors
    doc = {}
    for name, (seg, D, k) in SHAPES.items():
        x = torch.from_numpy(blobs(seg, D)).cuda()
        off = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
        graph = neighbors.neighbors(x, off, k)
        rows, nnz = int(off[-1]), int(graph["nnz_offsets"][-1])
        res = leiden.leiden(graph)
        walls = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = leiden.leiden(graph)
            walls.append(1e3 * (time.perf_counter() - t0))
        walls.sort()
        r = leiden._Run(graph, 1.0)                              # the level-0 sweep group alone, from singletons
        st = r.init(None, None)
        n_cur, long_rows = r._sizes(st, 0)
        with _lib.AbiTimer(["mcl_leiden_move_sweeps"]) as t:
            for _ in range(4):
                _lib.call("mcl_leiden_move_sweeps", 1, 0, n_cur, long_rows, r.max_sweeps, *r.graph_args, r.gamma, r.work)
        ms = t.summary()["mcl_leiden_move_sweeps"]["ms"]
        need = sweep_bytes(rows, nnz)
        entry = {"segments": int(seg.size), "rows": rows, "k": k, "nnz": nnz, "leiden_wall_ms_median": walls[len(walls) // 2],
                 "leiden_wall_ms_min": walls[0], "leiden_wall_ms_max": walls[-1],
                 "n_clusters": res["n_clusters"].tolist(), "modularity": res["modularity"].tolist(),
                 "levels": res["levels"].tolist(), "sweeps": res["sweeps"].tolist(), "rounds": res["rounds"].tolist(),
                 "iterations": res["iterations"].tolist(), "first_sweeps_ms": ms, "sweep_ms": min(ms),
                 "sweep_bytes": need, "sweep_GBps": need / (1e6 * min(ms))}
        entry["wall_ms_per_sweep_launch"] = entry["leiden_wall_ms_median"] / max(1, int(res["sweeps"].max()))
        if with_networkx:
            import networkx as nx
            total = 0.0
            qs = []
            for s in range(seg.size):
                g = nx.from_scipy_sparse_array(neighbors.to_scipy(graph, s)[1])
                t0 = time.perf_counter()
                comms = nx.community.louvain_communities(g, weight="weight", seed=0)
                total += time.perf_counter() - t0
                qs.append(nx.community.modularity(g, comms, weight="weight"))
            entry["networkx_louvain_cpu_ms"], entry["networkx_louvain_modularity"] = 1e3 * total, qs
        doc[name] = entry
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--networkx", action="store_true")
    a = ap.parse_args()
    line = json.dumps({"gpu": run(a.calls, a.networkx), "gpu_note": "one MI355X; wall clock around leiden(), HIP events for the sweep"})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
