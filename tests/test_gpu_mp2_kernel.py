"""
dmk_mp2_rhf / dmk_mp2_uhf on SYNTHETIC input through the C ABI: no SCF and no transform in front of the kernels, so
the shapes are free -- one occupied or one virtual orbital, very unequal spin channels, the [j][i][b][a] copy of t_ab at many
(oa, ob, va, vb), the workspace carve with and without caller-provided amplitudes -- and the refusals of the C entries.

Input    (ia|jb) = L^T L / 12 of a random L (12, o v), exactly symmetric for the restricted and same-spin blocks (the kernel's
         t_ij^ab = t_ji^ba), La^T Lb / 12 for the opposite-spin one; occupied levels in [-1.5, -0.5], virtual in [0.5, 1.5] with one
         exactly repeated level each, so every denominator is <= -2; e_vir is an 8-byte offset into the array of e_occ
         (tests/mp2_ref.py synthetic_g, synthetic_levels).
Reference  the literal formulas of tests/mp2_ref.py (rmp2_from_g / ump2_from_g) at np.longdouble.
Bounds   per element, derived (mp2_ref.rmp2_bounds / ump2_bounds, eps = 2^-52, evaluated in np.longdouble):
           amplitudes  16 eps |t_ref|
           energy      (N + 64) eps sum |t~ g|
           densities   (L + 64) eps S + 2 eps on the diagonal
         tests/test_host_mp2.py holds numpy's float64 evaluation to the same bounds without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

from tests import mp2_ref as M

pytestmark = pytest.mark.gpu

DMK_ERR_INVALID = -1
LD = np.longdouble

RHF_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (7, 16), (17, 33), (33, 17)]
UHF_SHAPES = [(1, 1, 1, 1), (1, 4, 3, 2), (3, 2, 1, 4), (5, 9, 2, 12), (17, 16, 16, 17), (33, 7, 6, 34)]


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _g4(V, o1, v1, o2, v2):
    """rows (i, a), columns (j, b) -> g[i, j, a, b]"""
    return V.reshape(o1, v1, o2, v2).transpose(0, 2, 1, 3)


def _vir(d_e, o):
    from libdmet_preview_amd._lib import c_vp
    return c_vp(d_e.address + 8 * o)


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def _run_rhf(ctx, o, v, V, e, with_t2):
    from libdmet_preview_amd._lib import lib
    d_V, d_e = ctx.to_device(V), ctx.to_device(e)
    nan = lambda *shape: ctx.to_device(np.full(shape, np.nan))
    d_ec, d_oo, d_vv = nan(1), nan(o, o), nan(v, v)
    d_t = nan(o, o, v, v) if with_t2 else None
    ctx.check(lib.dmk_mp2_rhf(ctx.h, o, v, d_V.ptr, d_e.ptr, _vir(d_e, o), d_ec.ptr, d_oo.ptr, d_vv.ptr, d_t.ptr if with_t2 else None))
    return {"e_corr": d_ec.get(), "doo": d_oo.get(), "dvv": d_vv.get(), "t2": d_t.get() if with_t2 else None}


def _run_uhf(ctx, shape, Vs, ea, eb, with_t2):
    from libdmet_preview_amd._lib import lib
    oa, va, ob, vb = shape
    d_V = [ctx.to_device(x) for x in Vs]                      # aa, bb, ab
    d_ea, d_eb = ctx.to_device(ea), ctx.to_device(eb)
    nan = lambda *s: ctx.to_device(np.full(s, np.nan))
    d_ec, d_d = nan(1), [nan(oa, oa), nan(va, va), nan(ob, ob), nan(vb, vb)]
    d_t = [nan(oa, oa, va, va), nan(oa, ob, va, vb), nan(ob, ob, vb, vb)] if with_t2 else [None] * 3
    p = lambda a: a.ptr if a is not None else None
    ctx.check(lib.dmk_mp2_uhf(ctx.h, oa, va, ob, vb, d_V[0].ptr, d_V[1].ptr, d_V[2].ptr, d_ea.ptr, _vir(d_ea, oa), d_eb.ptr,
                              _vir(d_eb, ob), d_ec.ptr, d_d[0].ptr, d_d[1].ptr, d_d[2].ptr, d_d[3].ptr, p(d_t[0]), p(d_t[1]), p(d_t[2])))
    out = {"e_corr": d_ec.get()}
    out.update({k: a.get() for k, a in zip(("doo_a", "dvv_a", "doo_b", "dvv_b"), d_d)})
    out["t2"] = tuple(a.get() for a in d_t) if with_t2 else None
    return out


def test_rmp2_on_synthetic_integrals(ctx):
    worst = {}
    for o, v in RHF_SHAPES:
        rng = np.random.default_rng(1000 * o + v)
        V, e = M.synthetic_g(rng, o * v), M.synthetic_levels(rng, o, v)
        g = _g4(V, o, v, o, v)
        ref = M.rmp2_from_g(g.astype(LD), e[:o].astype(LD), e[o:].astype(LD))
        bound = M.rmp2_bounds(g, ref)
        got = _run_rhf(ctx, o, v, V, e, True)
        assert got["t2"].shape == (o, o, v, v) and all(np.isfinite(got[k]).all() for k in ("e_corr", "doo", "dvv", "t2"))
        got["e_corr"] = got["e_corr"][0]
        r = M.ratios(got, ref, bound)
        trace = np.trace(got["doo"].astype(LD)) + np.trace(got["dvv"].astype(LD))
        r["trace"] = float(abs(trace - 2 * o) / (np.trace(bound["doo"]) + np.trace(bound["dvv"])))
        print("rmp2 (o, v) = (%d, %d): e_corr = %.12f  err / bound: %s" % (o, v, got["e_corr"], "  ".join("%s %.3f" % kv for kv in r.items())))
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert max(r.values()) <= 1.0, ((o, v), r)
        # without the caller's amplitudes (they are carved from the workspace): the same bits
        again = _run_rhf(ctx, o, v, V, e, False)
        assert _bits_equal([again[k] for k in ("e_corr", "doo", "dvv")], [np.atleast_1d(got["e_corr"]), got["doo"], got["dvv"]])
    print("rmp2 largest err / bound: %s" % "  ".join("%s %.3f" % kv for kv in worst.items()))


def test_ump2_on_synthetic_integrals(ctx):
    worst = {}
    for shape in UHF_SHAPES:
        oa, va, ob, vb = shape
        rng = np.random.default_rng(sum(x * 100 ** k for k, x in enumerate(shape)))
        Vaa, Vbb, Vab = M.synthetic_g(rng, oa * va), M.synthetic_g(rng, ob * vb), M.synthetic_g(rng, oa * va, ob * vb)
        ea, eb = M.synthetic_levels(rng, oa, va), M.synthetic_levels(rng, ob, vb)
        gaa, gbb, gab = _g4(Vaa, oa, va, oa, va), _g4(Vbb, ob, vb, ob, vb), _g4(Vab, oa, va, ob, vb)
        ref = M.ump2_from_g(gaa.astype(LD), gab.astype(LD), gbb.astype(LD), ea[:oa].astype(LD), ea[oa:].astype(LD), eb[:ob].astype(LD),
                            eb[ob:].astype(LD))
        bound = M.ump2_bounds(gaa, gab, gbb, ref)
        got = _run_uhf(ctx, shape, (Vaa, Vbb, Vab), ea, eb, True)
        assert [x.shape for x in got["t2"]] == [(oa, oa, va, va), (oa, ob, va, vb), (ob, ob, vb, vb)]
        assert all(np.isfinite(x).all() for k, x in got.items() if k != "t2") and all(np.isfinite(x).all() for x in got["t2"])
        got["e_corr"] = got["e_corr"][0]
        r = M.ratios(got, ref, bound)
        for s, n_s in (("a", oa), ("b", ob)):
            trace = np.trace(got["doo_" + s].astype(LD)) + np.trace(got["dvv_" + s].astype(LD))
            r["trace_" + s] = float(abs(trace - n_s) / (np.trace(bound["doo_" + s]) + np.trace(bound["dvv_" + s])))
        print("ump2 (oa, va, ob, vb) = %s: e_corr = %.12f  err / bound: %s" % (shape, got["e_corr"], "  ".join("%s %.3f" % kv for kv in r.items())))
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert max(r.values()) <= 1.0, (shape, r)
        keys = ("e_corr", "doo_a", "dvv_a", "doo_b", "dvv_b")
        again = _run_uhf(ctx, shape, (Vaa, Vbb, Vab), ea, eb, False)
        assert _bits_equal([again[k] for k in keys], [np.atleast_1d(got[k]) for k in keys])
    print("ump2 largest err / bound: %s" % "  ".join("%s %.3f" % kv for kv in worst.items()))


def test_refusals_of_the_c_entries(ctx):
    """DMK_ERR_INVALID with every output untouched (bit for bit): nocc or nvir of 0, each required pointer NULL in turn, nocc nvir^2
    beyond 2^31 (checked before any allocation: the arrays passed are tiny) and a NULL context."""
    from libdmet_preview_amd._lib import lib
    o, v = 2, 3
    rng = np.random.default_rng(3)
    V, e = M.synthetic_g(rng, o * v), M.synthetic_levels(rng, o, v)
    d_V, d_e = ctx.to_device(V), ctx.to_device(e)
    sentinel = np.full(o * o * v * v, -7.25)
    outs = [ctx.to_device(sentinel) for _ in range(8)]          # e_corr, four densities, three amplitude arrays (all oversized)
    untouched = lambda: all(np.array_equal(a.get(), sentinel) for a in outs)

    def rhf(h=ctx.h, nocc=o, nvir=v, drop=None):
        args = [d_V.ptr, d_e.ptr, _vir(d_e, o), outs[0].ptr, outs[1].ptr, outs[2].ptr]
        if drop is not None:
            args[drop] = None
        return lib.dmk_mp2_rhf(h, nocc, nvir, *(args + [outs[5].ptr]))

    def uhf(h=ctx.h, dims=(o, v, o, v), drop=None):
        args = [d_V.ptr, d_V.ptr, d_V.ptr, d_e.ptr, _vir(d_e, o), d_e.ptr, _vir(d_e, o), outs[0].ptr, outs[1].ptr, outs[2].ptr,
                outs[3].ptr, outs[4].ptr]
        if drop is not None:
            args[drop] = None
        return lib.dmk_mp2_uhf(h, *(list(dims) + args + [outs[5].ptr, outs[6].ptr, outs[7].ptr]))

    assert rhf(nocc=0) == DMK_ERR_INVALID and rhf(nvir=0) == DMK_ERR_INVALID and rhf(nocc=-1) == DMK_ERR_INVALID
    for drop in range(6):
        assert rhf(drop=drop) == DMK_ERR_INVALID, drop
    assert rhf(nocc=1, nvir=46341) == DMK_ERR_INVALID             # 46341^2 = 2^31 + 4633: the guard precedes the allocation
    assert rhf(h=None) == DMK_ERR_INVALID
    for k in range(4):
        dims = [o, v, o, v]
        dims[k] = 0
        assert uhf(dims=dims) == DMK_ERR_INVALID, dims
    for drop in range(12):
        assert uhf(drop=drop) == DMK_ERR_INVALID, drop
    assert uhf(dims=(1, 46341, 1, 1)) == DMK_ERR_INVALID and uhf(dims=(1, 1, 1, 46341)) == DMK_ERR_INVALID
    assert uhf(h=None) == DMK_ERR_INVALID
    ctx.sync()
    assert untouched()
    # the same argument lists, complete: accepted, and the outputs do change
    assert rhf() == 0 and uhf() == 0
    ctx.sync()
    assert not np.array_equal(outs[0].get()[:1], sentinel[:1]) and not np.array_equal(outs[5].get(), sentinel)
