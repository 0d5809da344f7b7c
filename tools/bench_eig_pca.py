"""cluster.pca_device with solver="host" (numpy.linalg.eigh of every Gram matrix, the default) against solver="device"
(mclstexp_amd.eig: csrc/eig.hip) at three shapes of synthetic expression data (synth.make_cluster_case):

    her2st_32     32 slides, spots drawn from 300 .. 700, 785 genes, n_comps 9   (a HER2ST evaluation)
    visium        one slide 4000 x 3467, n_comps 50                              (m = 3467)
    wide_3200     one slide 3200 x 685, n_comps 50

Prints one JSON line and, with --out, writes it.  Per shape: the wall time of pca_device for either solver (alternating
calls after a warm-up of both, a device synchronise before the clock stops; median, smallest, largest of --calls), the
largest difference of the scores between the two relative to max |Z|, and the device solver's three stages timed with HIP
events on the launch stream (mcl_sym_eig_top with stages = 1, 2, 4 on a fresh Gram matrix; best of --calls).  For the
tridiagonalisation the bytes its two streaming kernels must move are stated next to the stage's time: per column with a
trailing block of n = m - j - 1 rows, eig_symv_kernel reads 8 n^2 bytes and eig_rank2_kernel reads and writes 16 n^2; the
stage also holds one eig_house_kernel launch per column, so bytes / time is a lower bound of the kernels' own rate (a
kernel trace gives that: rocprofv3 --kernel-trace --stats -- python tools/bench_eig_pca.py --shapes visium --calls 1).
There is no pass / fail time.

    python tools/bench_eig_pca.py [--out profiles/eig_pca.json] [--calls 5] [--shapes her2st_32 visium wide_3200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("her2st_32", "visium", "wide_3200")


def shape(name):
    """(list of (spots, genes) matrices, n_comps)."""
    from mclstexp_amd import synth

    def slide(n, g, seed):
        return synth.make_cluster_case(n, g, 7, seed=seed, sep=0.1, undetermined_frac=0.0)["pred"]
    if name == "her2st_32":
        spots = np.random.RandomState(0).randint(300, 701, size=32)
        return [slide(int(n), 785, 100 + i) for i, n in enumerate(spots)], 9
    if name == "visium":
        return [slide(4000, 3467, 7)], 50
    if name == "wide_3200":
        return [slide(3200, 685, 8)], 50
    raise ValueError(name)


def stream_bytes(m):
    n = np.arange(2, m, dtype=np.float64)                # trailing orders n = m - 1 .. 2 of the columns j = 0 .. m - 3
    return float(24.0 * (n * n).sum())


def run(names, calls):
    import torch
    from mclstexp_amd import _arrays, _lib, cluster, eig
    doc = {}
    for name in names:
        xs, n_comps = shape(name)
        dev = _arrays.device("bench")
        x, off = _arrays.stack_rows(xs, "xs", dev)
        seg = np.diff(off)
        m = np.minimum(seg, x.shape[1]).astype(np.int32)
        res = {s: cluster.pca_device(x, off, n_comps, solver=s) for s in cluster.SOLVERS}       # warm-up of both
        torch.cuda.synchronize()
        zh, zd = (res[s]["scores"].cpu().numpy() for s in cluster.SOLVERS)
        walls = {s: [] for s in cluster.SOLVERS}
        for _ in range(calls):
            for s in cluster.SOLVERS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cluster.pca_device(x, off, n_comps, solver=s)
                torch.cuda.synchronize()
                walls[s].append(1e3 * (time.perf_counter() - t0))
        # the device solver's stages on a fresh Gram matrix each time
        S, G = int(m.size), int(x.shape[1])
        goff, eoff = _arrays.cumulative_offsets(m.astype(np.int64) ** 2), _arrays.cumulative_offsets(m.astype(np.int64) * n_comps)
        off_d, goff_d, eoff_d, m_d = (_arrays.upload(a, dev) for a in (off, goff, eoff, m))
        e = _arrays.empty(dev)
        mean, gram = e((S, G), torch.float64), e((int(goff[-1]),), torch.float64)
        values, cert, vectors = e((S, n_comps), torch.float64), e((S, 2), torch.float64), e((int(eoff[-1]),), torch.float64)
        max_m, sum_m = int(m.max()), int(m.sum())
        work = e((int(_lib.call("mcl_sym_eig_workspace_bytes", S, max_m, sum_m, n_comps)) // 8 + 1,), torch.float64)
        stages = {1: [], 2: [], 4: []}
        for _ in range(calls):
            _lib.call("mcl_pca_gram", x, x.stride(0), _arrays.FLOAT_CODE[x.dtype], off_d, S, G, int(seg.max()), goff_d, mean, gram)
            for st in (1, 2, 4):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                _lib.call("mcl_sym_eig_top", gram, goff_d, m_d, S, max_m, sum_m, n_comps, st, values, vectors, eoff_d, cert,
                          work)
                ev[1].record()
                torch.cuda.synchronize()
                stages[st].append(ev[0].elapsed_time(ev[1]))
        eig.check_certificate(cert.cpu().numpy(), m)
        need = sum(stream_bytes(int(v)) for v in m)
        entry = {"slides": S, "spots": seg.tolist(), "genes": G, "n_comps": n_comps, "m": m.tolist(),
                 "max_score_difference_rel": float(np.abs(zd - zh).max() / np.abs(zh).max()),
                 "certificate_max": [float(v) for v in cert.cpu().numpy().max(axis=0)],
                 "launches": 1 + 3 * max(max_m - 2, 0) + 1 + 10 + 1,
                 "tridiagonalisation_ms": min(stages[1]), "bisection_and_vectors_ms": min(stages[2]),
                 "back_transformation_ms": min(stages[4]), "tridiagonalisation_stream_bytes": need,
                 "tridiagonalisation_GBps_lower_bound": need / (1e6 * min(stages[1]))}
        for s in cluster.SOLVERS:
            w = sorted(walls[s])
            entry[f"pca_device_{s}_ms"] = {"median": w[len(w) // 2], "min": w[0], "max": w[-1]}
        doc[name] = entry
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=SHAPES)
    a = ap.parse_args()
    line = json.dumps({"gpu": run(a.shapes, a.calls),
                       "gpu_note": "one MI355X; wall clock around pca_device with a device synchronise, HIP events for the stages"})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
