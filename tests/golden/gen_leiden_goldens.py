"""Writes tests/golden/leiden.npz: what the restatement (tests/leiden_reference.py) gives on its case table, and the yardstick
it is measured against.  The graphs are regenerated from neighbors_reference and leiden_reference.case_graphs, not stored.

    python tests/golden/gen_leiden_goldens.py

Per case, slide s and resolution g (key prefix <case>_<s>_<g>_): labels, n_clusters, modularity, levels, sweeps,
accepted_sweeps, rounds, iterations, trace (Q after every accepted sweep, over all levels and iterations), refine_trace (per
refinement a NaN, Q of the singletons, then Q after every accepted round), margin (the smallest non-zero relative margin that
decided anything: best gain against the runner-up, a gain against staying or against zero, Q against the Q before) and
nx_modularity (networkx.community.modularity of those labels on the float64 weights).  For the cases of BOUNDED also
louvain: networkx.community.louvain_communities' Q over the seeds NX_SEEDS (networkx 3.4.2).  clusters_by_resolution: the
n_clusters of RESOLUTION_CASE at its resolutions in ascending order.

Refuses to write unless, on every run: every accepted step raised Q, every community is connected, the labels are ordered by
size, margin >= 1e-10, the restatement's Q is within 1e-12 of networkx's, Q >= min - (max - min) of the recorded Louvain
runs, and n_clusters does not fall as the resolution grows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import leiden_reference as lr  # noqa: E402


def key(name, s, g):
    return f"{name}_{s}_{g}_"


def bound(louvain):
    return float(louvain.min() - (louvain.max() - louvain.min()))


def main():
    out = {}
    for name, resolutions in lr.CASES.items():
        for s, m in enumerate(lr.case_graphs(name)):
            for g in resolutions:
                r = lr.run(m, g)
                k = key(name, s, g)
                for seq in [r["trace"]] + r["refine_trace"]:
                    assert all(b > a for a, b in zip(seq, seq[1:])), (k, "an accepted step did not raise Q")
                r["refine_trace"] = np.concatenate([[np.nan] + seq for seq in r["refine_trace"]]) if r["refine_trace"] else []
                assert lr.connected(m, r["labels"]), (k, "a community is not connected")
                sizes = np.bincount(r["labels"])
                assert (np.diff(sizes) <= 0).all(), (k, "labels are not ordered by size")
                assert r["margin"] >= 1e-10, (k, r["margin"])
                nxq = lr.nx_modularity(m, r["labels"], g) if m.nnz else 0.0
                assert abs(nxq - r["modularity"]) <= 1e-12, (k, nxq, r["modularity"])
                for field in ("labels", "n_clusters", "modularity", "levels", "sweeps", "accepted_sweeps", "rounds",
                              "iterations", "trace", "refine_trace", "margin"):
                    out[k + field] = np.asarray(r[field])
                out[k + "nx_modularity"] = np.float64(nxq)
                line = f"{k[:-1]}: n {m.shape[0]} clusters {r['n_clusters']} Q {r['modularity']:.10f} margin {r['margin']:.3g}"
                if name in lr.BOUNDED:
                    lou = lr.nx_louvain(m, g)
                    assert r["modularity"] >= bound(lou), (k, r["modularity"], bound(lou))
                    out[k + "louvain"] = lou
                    line += f" louvain {lou.min():.10f} .. {lou.max():.10f} bound {bound(lou):.10f}"
                print(line)
    name = lr.RESOLUTION_CASE
    counts = [int(out[key(name, 0, g) + "n_clusters"]) for g in sorted(lr.CASES[name])]
    assert counts == sorted(counts), counts
    out["clusters_by_resolution"] = np.asarray(counts)
    np.savez_compressed(lr.GOLDEN, **out)
    print("wrote", lr.GOLDEN, os.path.getsize(lr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
