"""Times one product sigma = H c of the device FCI at (12,6,6), (14,7,7) and, slabbed, (16,8,8).

    python tools/fci_lab.py [n,na,nb ...]

Per shape: a warm-up product, then REPS products timed one by one with HIP events; the median and the spread are printed.  A second
round of REPS products runs under the per-family profile of the library (events around every launch): `misc` is the two gather
kernels (fci_d_kernel, fci_s_kernel), `fit` the product with the integral supermatrix (dmk_dgemm_batched).  Rates: the gathers
against their minimal traffic (D written once, c read once per alpha link; G read once per link of sigma, sigma written once) and
the 6.3 TB/s copy rate; the product against its flop count 2 M (M + 1) Ndet and the 78.6 TF f64 matrix roof.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from libdmet_preview_amd import _lib
from libdmet_preview_amd._lib import lib

REPS = 5
COPY_RATE, F64_ROOF = 6.3e12, 78.6e12


def lab(ctx, n, na, nb, spin=1):
    rng = np.random.default_rng(n)
    h1 = rng.standard_normal((n, n))
    h1 = 0.5 * (h1 + h1.T)
    A = rng.standard_normal((4, n, n))
    A = 0.5 * (A + A.transpose(0, 2, 1))
    g = (0.05 / n) * np.einsum("Pij,Pkl->ijkl", A, A)
    d_h1, d_g = ctx.to_device(h1), ctx.to_device(g)
    h = C.c_void_p()
    ctx.check(lib.dmk_fci_create(ctx.h, n, na, nb, spin, d_h1.ptr, d_g.ptr, None, None, 0.0, 2, 0, C.byref(h)))
    info = (C.c_int64 * 4)()
    ctx.check(lib.dmk_fci_info(h, info))
    Na, Nb, rows, slabs = [int(x) for x in info]
    ndet = Na * Nb
    c, s = ctx.empty((ndet,), np.float64), ctx.empty((ndet,), np.float64)
    ctx.check(lib.dmk_fci_get(h, 1, c.ptr))            # the diagonal: a dense vector of the right size
    ctx.check(lib.dmk_fci_sigma(h, c.ptr, s.ptr))      # warm-up
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        ctx.check(lib.dmk_fci_sigma(h, c.ptr, s.ptr))
        ms.append(ctx.timer_stop())
    ctx.profile(True)
    ctx.profile_read()
    for _ in range(REPS):
        ctx.check(lib.dmk_fci_sigma(h, c.ptr, s.ptr))
    ctx.sync()
    fam = ctx.profile_read()
    ctx.profile(False)
    t_g, t_p = fam["misc"][0] / REPS * 1e-3, fam["fit"][0] / REPS * 1e-3
    n2 = n * n
    M = spin * n2
    links = na * (n - na + 1) + nb * (n - nb + 1)
    gather_bytes = 8.0 * ndet * ((M + 1) + links + 1 + links + 1)
    flops = 2.0 * M * (M + 1) * ndet
    print("(%d, %d, %d) spin %d: %d x %d = %d determinants, %d alpha rows in flight, %d slab(s)" % (n, na, nb, spin, Na, Nb, ndet, rows, slabs))
    print("  sigma        median %.3f ms (min %.3f, max %.3f) over %d" % (np.median(ms), min(ms), max(ms), REPS))
    print("  gathers      %.3f ms  %d launches  %.2f TB/s of minimal traffic = %.1f%% of the copy rate"
          % (t_g * 1e3, fam["misc"][1] // REPS, gather_bytes / t_g / 1e12, 100.0 * gather_bytes / t_g / COPY_RATE))
    print("  product      %.3f ms  %d launches  %.2f TFLOP/s = %.1f%% of the f64 matrix roof"
          % (t_p * 1e3, fam["fit"][1] // REPS, flops / t_p / 1e12, 100.0 * flops / t_p / F64_ROOF))
    print("  bound by     %s" % ("the product" if t_p > t_g else "the gathers"), flush=True)
    lib.dmk_fci_free(h)
    for x in (c, s, d_h1, d_g):
        x.free()
    ctx.trim()


if __name__ == "__main__":
    shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:]] or [(12, 6, 6), (14, 7, 7), (16, 8, 8)]
    ctx = _lib.get_ctx()
    for shp in shapes:
        lab(ctx, *shp)
