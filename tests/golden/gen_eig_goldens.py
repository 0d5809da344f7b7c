"""Writes tests/golden/eig.npz: the case matrices of tests/eig_reference.py and what the restatement gives on them.

    python tests/golden/gen_eig_goldens.py

Per case <name>: <name>.a, the upper triangle of the symmetric matrix row by row (eig_reference.unpack rebuilds it); per k of
eig_reference.counts(m): <name>.k<k>.values (k,) descending and <name>.k<k>.certificate (2,); the vectors (m, k) as
<name>.k<k>.vectors for the k of eig_reference.stored_vectors (the largest count; 9 for the hard spectra, whose matrices
fill most of the file).  The Gram matrices of cluster_reference's GRAM_CASES are checked at k = 9, 50 and 64 and not stored.

Refuses to write unless the restatement satisfies, for every case and k, against numpy.linalg.eigh (eps = 2^-52):
|d lambda| <= 4 m eps |A|_2, max |A z - lambda z|_2 <= 4 m eps |A|_2, max |Z^T Z - I| <= 4 m eps, the sign rule, and a
certificate below the guard 64 m eps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import cluster_reference as cr  # noqa: E402
import eig_reference as er  # noqa: E402
from mclstexp_amd import synth  # noqa: E402


def check(name, a, k):
    lam, z, cert = er.eigh_top(a, k)
    m = a.shape[0]
    dl, res, orth, norm2, _, _ = er.errors(a, lam, z)
    bl, br, bo = er.bounds(m, norm2)
    print(f"{name}: m {m} k {k} |dlam| {dl:.2e} / {bl:.2e}  res {res:.2e} / {br:.2e}  orth {orth:.2e} / {bo:.2e}  "
          f"cert {cert[0]:.2e} {cert[1]:.2e}")
    assert dl <= bl and res <= br and orth <= bo, (name, k, "outside the method's bounds")
    assert er.sign_rule_holds(z), (name, k, "sign rule")
    assert (cert <= 64.0 * m * er.EPS).all(), (name, k, cert)
    return lam, z, cert


def main():
    out = {}
    for name, a in er.case_matrices().items():
        assert np.array_equal(a, a.T), name
        out[f"{name}.a"] = er.pack(a)
        assert np.array_equal(er.unpack(out[f"{name}.a"]), a), name
        for k in er.counts(a.shape[0]):
            lam, z, cert = check(name, a, k)
            out[f"{name}.k{k}.values"], out[f"{name}.k{k}.certificate"] = lam, cert
            if k == er.stored_vectors(name, a.shape[0]):
                out[f"{name}.k{k}.vectors"] = z
    for name in er.GRAM_CASES:
        a = er.gram_matrix(cr.kept(synth.make_cluster_case(**cr.CLUSTER_CASES[name]))[0])
        for k in (9, 50, 64):
            check("gram_" + name, a, k)
    np.savez_compressed(er.GOLDEN, **out)
    size = os.path.getsize(er.GOLDEN)
    print("wrote", er.GOLDEN, size, "bytes")
    assert size <= 1 << 20, "the fixture must stay below 1 MiB"


if __name__ == "__main__":
    main()
