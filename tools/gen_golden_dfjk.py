#!/usr/bin/env python
"""
tools/gen_golden_dfjk.py -- capture tests/golden/G39_dfjk.npz from the REFERENCE's get_jk_from_eri_7d
(routine/pbc_helper.py:314-359), imported through oracle/shim.py like oracle/gen_golden.py does.  TEST INFRASTRUCTURE ONLY;
needs the reference tree, so it runs in the build container only:

    python tools/gen_golden_dfjk.py

Mesh (3,1,1), nao 16, naux 6.  DF blocks with the pair relation B^(j,i)[L,r,t] = conj(B^(i,j)[L,t,r]) (only i <= j stored), one
RHF and one two-spin random Hermitian density (not time-reversal symmetric), the 7-index ERI
eri_7d[i,j,k][p,q,r,t] = sum_L B^(i,j)[L,p,q] B^(k,l)[L,r,t] (l from momentum conservation; built here, not stored) and the
reference's vj, vk.  Arrays only.
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import shim  # noqa: E402
from tests import dfjk_ref  # noqa: E402

MESH, NAO, NAUX = (3, 1, 1), 16, 6


def main():
    shim.install()
    shim.quiet()
    from libdmet.routine import pbc_helper as rp
    rng = np.random.default_rng(39)
    nk = int(np.prod(MESH))
    stored = {}
    for i in range(nk):
        for j in range(i, nk):
            b = (rng.standard_normal((NAUX, NAO, NAO)) + 1j * rng.standard_normal((NAUX, NAO, NAO))) / NAO
            if i == j:
                b = 0.5 * (b + b.conj().transpose(0, 2, 1))
            stored[(i, j)] = b
    blocks = dfjk_ref.expand_pairs(stored, nk)

    def herm(*shape):
        d = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        return 0.5 * (d + d.conj().swapaxes(-1, -2))
    dm_rhf, dm_uhf = herm(nk, NAO, NAO), herm(2, nk, NAO, NAO)

    # 1-D mesh in fftfreq order: index arithmetic modulo nk is momentum conservation, k_i - k_j + k_k - k_l = 0
    eri_7d = np.zeros((nk, nk, nk, NAO, NAO, NAO, NAO), dtype=np.complex128)
    for i in range(nk):
        for j in range(nk):
            for k in range(nk):
                l = (i - j + k) % nk
                eri_7d[i, j, k] = np.einsum("Lpq,Lrt->pqrt", blocks[(i, j)], blocks[(k, l)])
    out = {"mesh": np.asarray(MESH), "nao": np.asarray(NAO), "naux": np.asarray(NAUX), "dm_rhf": dm_rhf, "dm_uhf": dm_uhf}
    for (i, j), b in stored.items():
        out["B_%d_%d" % (i, j)] = b
    for tag, dm in (("rhf", dm_rhf), ("uhf", dm_uhf)):
        vj, vk = rp.get_jk_from_eri_7d(eri_7d, dm)
        out["vj_" + tag], out["vk_" + tag] = vj, vk
        rj, rk = dfjk_ref.get_jk(lambda a, b: blocks[(a, b)], dm)
        print(tag, "restatement vs reference:", np.abs(rj - vj).max() / np.abs(vj).max(), np.abs(rk - vk).max() / np.abs(vk).max())
    path = os.path.join(ROOT, "tests", "golden", "G39_dfjk.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
