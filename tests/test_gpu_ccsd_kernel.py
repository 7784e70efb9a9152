"""
dmk_cc_ladder_s4 alone, through the C ABI:   out[r][a][b] = beta out[r][a][b] + alpha sum_cd tau[r][c][d] (ac|bd)
on a 4-fold PACKED random block (rows pair(a,c), columns pair(b,d), pitch npair + 3) that is NOT symmetric under bra <-> ket.

Reference  the literal contraction over the unpacked v^4 tensor at np.longdouble (one matrix product per shape, shared by the cases).
Bound      per element, computed here in np.longdouble with eps = 2^-52 (c = 1 as in mp2_ref.rmp2_bounds, whose contraction terms are
           (L + 64) eps S with L the contraction length):
               K eps |alpha| S,   K = v^2,  S = sum_cd |tau| |W|          the fused-multiply-add chain of the matrix cores
             + eps (|alpha| S + |beta out_0|)   only where beta != 0       the scaling by beta and the final addition
Shapes     one element; v below, at and above the K chunk of 16 and the 64-wide tile; m off the 64-row tile and over many
           workgroups; v = 65 (two column tiles, chunks on both sides of the diagonal of the triangle).

Wide, exactly  v = 64, 97, 113, 129 with INTEGER data: the packed block, tau and out_0 are integers in [-8, 8] held as float64, so
           every partial sum is an integer below 64 v^2 < 2^21: any summation order, the fused-multiply-add chain of the matrix
           cores included, is exact, and the device must return the bits of a plain float64 numpy reference (one a at a time: the
           rows pair(a, c) gathered, their columns expanded through an index table to [(c, d)][b], one matrix product with tau; v^4
           is never held).  The loader runs its lanes along b only where a chunk starts at d0 >= n0 + 32, which at v <= 65 happens
           in column tile n0 = 0 alone: v = 97 and 113 put such chunks (d0 = 96, 112) into tile n0 = 64, v = 129 adds a third column
           tile with a single valid column, v = 64 is the full tile without an edge.  (alpha, beta) = (1, 0) and (-2, 1); pitch
           npair + 3 with a NaN pad.
"""
import functools

import numpy as np
import pytest

from tests import scf_ref as R

pytestmark = pytest.mark.gpu

DMK_ERR_INVALID = -1
LD = np.longdouble
EPS = LD(2.0) ** -52
SHAPES = [(1, 1), (1, 2), (4, 3), (9, 15), (9, 16), (17, 17), (1024, 33), (5, 65)]
PAD = 3


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@functools.lru_cache(maxsize=None)
def _case(m, v):
    """(packed block with pitch, tau, out_0, reference sum, sum over absolute values): one per shape, never modified."""
    rng = np.random.default_rng(1000 * m + v)
    npair = v * (v + 1) // 2
    Wp = np.zeros((npair, npair + PAD))
    Wp[:, :npair] = rng.standard_normal((npair, npair))
    Wp[:, npair:] = np.nan                                             # the pitch is never read
    # Rows: 64 random ones; row r beyond them is row r % 64 times +-2^k with k and the sign set by r // 64 -- every row of tau differs,
    # every 64-row tile holds all of them at a scale of its own, and the np.longdouble product (which numpy evaluates without BLAS)
    # is needed for 64 rows only: a power of two scales a row of the exact result exactly.
    nb = min(m, 64)
    base = rng.standard_normal((nb, v, v))
    tile = np.arange(m) // 64
    scale = (2.0 ** (tile % 16)) * np.where(tile % 2 == 1, -1.0, 1.0)
    tau = base[np.arange(m) % nb] * scale[:, None, None]
    out0 = rng.standard_normal((m, v, v))
    g = R.restore_s1(Wp[:, :npair], v)                                # g[a, c, b, d] = (ac|bd)
    assert np.abs(g - g.transpose(2, 3, 0, 1)).max() > 0.1 or v == 1  # no bra <-> ket symmetry
    B = g.transpose(1, 3, 0, 2).reshape(v * v, v * v)                 # [(c, d)][(a, b)]
    ref = (base.reshape(nb, v * v).astype(LD) @ B.astype(LD)).reshape(nb, v, v)
    S = (np.abs(base.reshape(nb, v * v)).astype(LD) @ np.abs(B).astype(LD)).reshape(nb, v, v)
    sc = scale.astype(LD)[:, None, None]
    return Wp, tau, out0, sc * ref[np.arange(m) % nb], np.abs(sc) * S[np.arange(m) % nb]


def _ladder(ctx, m, v, d_W, ld, d_tau, alpha, beta, out0):
    from libdmet_preview_amd._lib import lib
    d_out = ctx.to_device(out0)
    ctx.check(lib.dmk_cc_ladder_s4(ctx.h, m, v, d_W.ptr, ld, d_tau.ptr, alpha, beta, d_out.ptr))
    ctx.sync()
    return d_out.get()


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 1.0)])
@pytest.mark.parametrize("m,v", SHAPES)
def test_ladder_against_the_unpacked_einsum(ctx, m, v, alpha, beta):
    Wp, tau, out0, ref, S = _case(m, v)
    npair = v * (v + 1) // 2
    d_W, d_tau = ctx.to_device(Wp), ctx.to_device(tau)
    start = out0 if beta != 0.0 else np.full_like(out0, np.nan)       # beta = 0 never reads out
    got = _ladder(ctx, m, v, d_W, npair + PAD, d_tau, alpha, beta, start)
    want = LD(alpha) * ref + (LD(beta) * out0.astype(LD) if beta != 0.0 else 0)
    bound = LD(v * v) * EPS * abs(alpha) * S
    if beta != 0.0:
        bound = bound + EPS * (abs(alpha) * S + np.abs(LD(beta) * out0.astype(LD)))
    ratio = float(np.max(np.abs(got.astype(LD) - want) / bound))
    print("m = %d, v = %d, alpha = %g, beta = %g: max |err| / bound = %.3f, max |err| = %.3e"
          % (m, v, alpha, beta, ratio, float(np.abs(got - want).max())))
    assert np.all(np.isfinite(got)) and ratio <= 1.0
    again = _ladder(ctx, m, v, d_W, npair + PAD, d_tau, alpha, beta, start)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))     # two calls, the same bits


def _integers(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _exact_ladder(Wp, tau, v):
    """sum_cd tau[r][c][d] (ac|bd) as (m, v, v) in float64, from the packed block, one a at a time."""
    m = tau.shape[0]
    idx = np.zeros((v, v), dtype=np.int64)
    i, j = np.tril_indices(v)
    idx[i, j] = idx[j, i] = np.arange(len(i))
    T = tau.reshape(m, v * v)
    out = np.empty((m, v, v))
    for a in range(v):
        B = Wp[idx[a]][:, idx.reshape(-1)]                            # B[c][(d, b)] = (ac|bd): row pair(a, c), column pair(b, d)
        out[:, a, :] = T @ B.reshape(v * v, v)
    return out


@pytest.mark.parametrize("v,ms", [(64, (2, 65)), (97, (2, 65)), (113, (2,)), (129, (2,))])
def test_wide_ladder_is_exact_on_integers(ctx, v, ms):
    rng = np.random.default_rng(7000 + v)
    npair = v * (v + 1) // 2
    Wp = np.full((npair, npair + PAD), np.nan)
    Wp[:, :npair] = _integers(rng, (npair, npair))
    d_W = ctx.to_device(Wp)
    for m in ms:
        tau, out0 = _integers(rng, (m, v, v)), _integers(rng, (m, v, v))
        ref = _exact_ladder(Wp, tau, v)
        assert np.abs(ref).max() < 2.0 ** 21 and np.array_equal(ref, np.rint(ref))
        d_tau = ctx.to_device(tau)
        for alpha, beta in ((1.0, 0.0), (-2.0, 1.0)):
            start = out0 if beta != 0.0 else np.full_like(out0, np.nan)   # beta = 0 never reads out
            got = _ladder(ctx, m, v, d_W, npair + PAD, d_tau, alpha, beta, start)
            want = alpha * ref + (beta * out0 if beta != 0.0 else 0.0)
            bad = got != want                                             # (NaN counts as different)
            print("m = %d, v = %d, alpha = %g, beta = %g: %d of %d elements differ, max |err| = %s, columns b of the differences: %s"
                  % (m, v, alpha, beta, bad.sum(), bad.size, np.abs(got - want).max(), np.unique(np.nonzero(bad)[2])[:8]))
            assert np.all(np.isfinite(got)) and not bad.any()
            assert np.array_equal((got + 0.0).view(np.uint64), (want + 0.0).view(np.uint64))      # the same bits (-0 + 0 = +0)


def test_ladder_refuses_bad_arguments(ctx):
    from libdmet_preview_amd._lib import lib
    m, v = 4, 3
    Wp, tau, out0, _, _ = _case(m, v)
    npair = v * (v + 1) // 2
    d_W, d_tau, d_out = ctx.to_device(Wp), ctx.to_device(tau), ctx.to_device(out0)
    call = lambda mm, vv, ld: lib.dmk_cc_ladder_s4(ctx.h, mm, vv, d_W.ptr, ld, d_tau.ptr, 1.0, 0.0, d_out.ptr)
    for mm, vv, ld in ((0, v, npair), (-1, v, npair), (m, 0, npair), (m, 513, 513 * 514 // 2), (m, v, npair - 1)):
        assert call(mm, vv, ld) == DMK_ERR_INVALID
    assert lib.dmk_cc_ladder_s4(ctx.h, m, v, None, npair, d_tau.ptr, 1.0, 0.0, d_out.ptr) == DMK_ERR_INVALID
    ctx.sync()
    assert np.array_equal(d_out.get(), out0)                          # nothing was launched
    assert call(m, v, npair + PAD) == 0
