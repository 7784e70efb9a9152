"""A/B of two builds of the eigensolvers, bit for bit.

  LIBDMETK_SO=<library> python tools/eigh_ab.py run out.npz     every w and Vt of the cases below, seeded inputs
  python tools/eigh_ab.py compare a.npz b.npz                   numpy.array_equal array by array; exit status 1 on a difference

Run each library in a fresh process.  Cases: the complex route (dmk_eigh_batched: every instantiation of eigh_kernel, the
resident tridiagonalisation with tri_eigpairs_kernel, its repair pass under DMK_EIGH_INJECT, eigh_kernel's own first pass
under DMK_EIGH_TRIPAIRS=0), the real route (dmk_eigh_batched_real, n = 2049 through the many-workgroup solver) and the
handle interface of the many-workgroup solver (dmk_eighl_factor / _vectors).
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def _wilkinson(m):
    d = np.abs(np.arange(2 * m + 1) - m).astype(float)
    return np.diag(d) + np.diag(np.ones(2 * m), 1) + np.diag(np.ones(2 * m), -1)


def _glued(blocks, glue):
    n = sum(b.shape[0] for b in blocks)
    T = np.zeros((n, n))
    o = 0
    for b in blocks:
        k = b.shape[0]
        T[o:o + k, o:o + k] = b
        if o + k < n:
            T[o + k - 1, o + k] = T[o + k, o + k - 1] = glue
        o += k
    return T


def clustered():
    return [_wilkinson(10), _glued([_wilkinson(10)] * 9, 1e-9), _glued([_wilkinson(10)] * 4, 1e-13),
            _glued([np.diag([1.0, 1.0, 1.0]) + 1e-7 * (np.eye(3, k=1) + np.eye(3, k=-1))] * 5, 1e-7)]


def _herm(rng, batch, n, real):
    A = rng.standard_normal((batch, n, n)) + (0 if real else 1j * rng.standard_normal((batch, n, n)))
    return A + A.conj().transpose(0, 2, 1)


def run(path):
    from libdmet_preview_amd import _lib
    from libdmet_preview_amd._lib import lib
    ctx = _lib.get_ctx()
    out = {}

    def env(inject=None, tripairs=None):
        for k, v in (("DMK_EIGH_INJECT", inject), ("DMK_EIGH_TRIPAIRS", tripairs)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def cplx(tag, A, add=None):
        batch, n = A.shape[:2]
        dA = ctx.to_device(A.astype(np.complex128))
        dadd = ctx.to_device(add) if add is not None else None
        dw, dV = ctx.empty((batch, n), np.float64), ctx.empty((batch, n, n), np.complex128)
        ctx.check(lib.dmk_eigh_batched(ctx.h, n, batch, dA.ptr, dadd.ptr if dadd is not None else None, 0, dw.ptr, dV.ptr))
        out[tag + "/w"], out[tag + "/Vt"] = dw.get(), dV.get()

    def real(tag, A):
        batch, n = A.shape[:2]
        dA = ctx.to_device(np.ascontiguousarray(A, dtype=np.float64))
        dw, dV = ctx.empty((batch, n), np.float64), ctx.empty((batch, n, n), np.float64)
        ctx.check(lib.dmk_eigh_batched_real(ctx.h, n, batch, dA.ptr, dw.ptr, dV.ptr))
        out[tag + "/w"], out[tag + "/Vt"] = dw.get(), dV.get()

    def large(tag, A, lda=None, idx=None):
        n = A.shape[0]
        lda = n if lda is None else lda
        buf = np.full((n, lda), 7.5)
        buf[:, :n] = A
        idx = np.ascontiguousarray(np.arange(n) if idx is None else idx, dtype=np.int32)
        dA, dw, dV = ctx.to_device(buf), ctx.empty((n,), np.float64), ctx.empty((len(idx), n), np.float64)
        h = C.c_void_p()
        ctx.check(lib.dmk_eighl_factor(ctx.h, n, dA.ptr, lda, dw.ptr, C.byref(h)))
        try:
            ctx.check(lib.dmk_eighl_vectors(h, len(idx), idx.ctypes.data_as(C.c_void_p), dV.ptr))
        finally:
            lib.dmk_eighl_free(h)
        out[tag + "/w"], out[tag + "/Vt"] = dw.get(), dV.get()

    mats = clustered()
    env()
    for n in (1, 2, 3, 33, 64, 65, 136, 200):
        cplx("c128/n%d" % n, _herm(np.random.default_rng(n), 3, n, False))
    for n in (65, 136, 200):
        rng = np.random.default_rng(1000 + n)
        add = rng.standard_normal((n, n))
        cplx("c128/n%d_add" % n, _herm(rng, 3, n, False), add + add.T)
    for n in (256, 257, 300):
        cplx("c128/n%d" % n, _herm(np.random.default_rng(n), 2, n, False))
    A136 = _herm(np.random.default_rng(136), 3, 136, False)
    for label, kw in (("", {}), ("_inject3", {"inject": 3}), ("_tripairs0", {"tripairs": 0})):
        env(**kw)
        for T in mats:
            cplx("c128/clustered%d%s" % (T.shape[0], label), T[None])
        if label:
            cplx("c128/n136" + label, A136)
    env()
    for n, batch in ((2, 2), (64, 2), (65, 2), (300, 2), (1100, 1)):
        real("f64/n%d" % n, _herm(np.random.default_rng(2000 + n), batch, n, True))
    for label, kw in (("", {}), ("_inject3", {"inject": 3})):
        env(**kw)
        for T in mats:
            real("f64/clustered%d%s" % (T.shape[0], label), T[None])
    env()
    for n in (2, 33):
        large("large/n%d" % n, _herm(np.random.default_rng(3000 + n), 1, n, True)[0])
    large("large/n65_lda72", _herm(np.random.default_rng(3065), 1, 65, True)[0], lda=72)
    large("large/clustered189", mats[1])
    rng = np.random.default_rng(3300)
    large("large/n300_subset40", _herm(rng, 1, 300, True)[0], idx=np.sort(rng.choice(300, 40, replace=False)))
    real("f64/n2049", _herm(np.random.default_rng(2049), 1, 2049, True))
    np.savez(path, **out)
    print("%d arrays of %d cases -> %s" % (len(out), len(out) // 2, path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two files hold different cases"
    diff = []
    for k in sorted(a.files):
        if not np.array_equal(a[k], b[k]):
            diff.append(k)
            print("DIFFERS %-34s max |a - b| = %.3e" % (k, np.abs(a[k] - b[k]).max()))
    print("%d of %d arrays differ" % (len(diff), len(a.files)))
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
