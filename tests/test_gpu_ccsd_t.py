"""
The perturbative triples on the device (csrc/ccsd_t.hip) against formulation (b) of tests/ccsd_t_ref.py.

Shapes        through the C ABI alone: host orbitals of ccsd_ref.uneven_system, the blocks of ccsd_ref.restricted_blocks (the packed
              (vv|vv) block with a pitch of npair + 3 and NaN pad: (T) must not read it at all), dmk_rccsd_set of random symmetric
              amplitudes of scale 0.1.  (o, v) cover the vanishing cases o = 1 / v = 1, one, two and three 16-wide MFMA tiles along o
              (and both workgroup tiles: 32 up to o = 32, 64 above), K loops off every multiple of 4 in both parts, from 1 to 6545
              unique triples, and diagonal triples of every multiplicity.  Reference in longdouble up to (5, 17) / (17, 5), float64 above.
Tolerance     derived, not tuned:  |E_dev - E_ref| <= (2 (o + v) + 64) eps S,  S the same expression with the absolute value taken
              at every product.  Each of the two factors W of a term carries (o + v) eps of its own absolute sum (a K loop of v + o
              products, accumulated in any order); the 64 covers the six additions into W, r3, V, the division and the reductions.
Bits          repeats are bit-identical; a budget of fixed + exactly one triple (as many batches as unique triples) gives the bits of
              the default budget; a budget one byte below that is refused with DMK_ERR_NOMEM and nothing allocated.
Side effects  the amplitudes and the energy of the handle are what they were.
End to end    CCSolver.run then .ccsd_t() at n = 6 (4 electrons) and n = 17, against (b) at the device's orbitals and amplitudes;
              RCCSDLambda.ccsd_t gives the same number; ten rounds of solver.ccsd_t.kernel give the device memory back.
Measured      profiles/ccsd_t_notes.txt.
"""
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import ccsd_t_ref as TR
from tests import scf_ref as R
from tests.test_gpu_ccsd_shapes import Handle, PAD, T1, T2, _bits

pytestmark = pytest.mark.gpu

DMK_OK, DMK_ERR_NOMEM = 0, -3
EPS = np.finfo(np.float64).eps
SHAPES = [(1, 3), (3, 1), (2, 2), (2, 3), (3, 2), (4, 5), (5, 17), (17, 5), (33, 3), (3, 33), (16, 16)]
CASES = [(o, v, False) for o, v in SHAPES] + [(4, 5, True), (5, 17, True)]
LONG_LIMIT = 85          # o v up to which the reference runs in longdouble: (5, 17) and (17, 5)


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def bound(o, v, s):
    return (2 * (o + v) + 64) * EPS * s


@functools.lru_cache(maxsize=None)
def _case(o, v, rotated):
    """(fock, blocks, t1, t2, E_ref, S): shared by the tests, never modified."""
    sysm, Cm = CR.uneven_system(o, v)
    if rotated:
        Cm = CR.rotate_ov(Cm, o)
    f, blocks = CR.restricted_blocks(sysm, Cm, o, pad=PAD)
    t1, t2 = CR.random_amplitudes(np.random.default_rng(1000 * o + v), o, v)
    e, s = TR.t_closed_shell(f, blocks, t1, t2, np.longdouble if o * v <= LONG_LIMIT else np.float64)
    return f, blocks, t1, t2, e, s


def _triples(ctx, h, max_bytes=0):
    """-> (E_(T), batches) of dmk_rccsd_t on the Handle h"""
    from libdmet_preview_amd._lib import lib, c_dbl
    res = (c_dbl * 2)(np.nan, np.nan)
    ctx.check(lib.dmk_rccsd_t(h.h, int(max_bytes), res))
    return float(res[0]), int(res[1])


@pytest.mark.parametrize("o,v,rotated", CASES)
def test_triples_against_the_closed_shell_reference(ctx, o, v, rotated):
    f, blocks, t1, t2, e_ref, s = _case(o, v, rotated)
    if rotated:
        assert np.abs(f[:o, o:]).max() > 1e-3
    h = Handle(ctx, o, v, f, blocks)
    try:
        h.set(t1, t2)
        e0 = h.energy()
        e, batches = _triples(ctx, h)
        again, _ = _triples(ctx, h)
        g1, g2 = h.amps()
        e1 = h.energy()
    finally:
        h.close()
    frac = abs(e - e_ref) / bound(o, v, s)
    print("(o, v) = (%d, %d)%s: E_(T) = %.15e, reference %.15e, S = %.3e, |d| = %.3e = %.4f of the bound, %d batch(es)"
          % (o, v, " rotated" if rotated else "", e, e_ref, s, abs(e - e_ref), frac, batches))
    assert np.isfinite(e) and batches >= 1
    assert abs(e - e_ref) <= bound(o, v, s)
    if o == 1 or v == 1:
        assert abs(e) <= bound(o, v, s)                      # vanishes identically
    else:
        assert abs(e_ref) > 1e3 * bound(o, v, s)             # the comparison resolves the number
    assert np.array_equal(_bits(e), _bits(again))
    assert np.array_equal(_bits(g1), _bits(t1)) and np.array_equal(_bits(g2), _bits(t2)) and np.array_equal(_bits(e0), _bits(e1))


@pytest.mark.parametrize("o,v", [(4, 5), (5, 17)])
def test_budget_does_not_change_the_bits(ctx, o, v):
    from libdmet_preview_amd._lib import lib, c_dbl, c_i64
    f, blocks, t1, t2, e_ref, s = _case(o, v, False)
    plan = (c_i64 * 2)()
    assert lib.dmk_rccsd_t_plan(o, v, plan) == DMK_OK
    fixed, unit = int(plan[0]), int(plan[1])
    ntr = v * (v + 1) * (v + 2) // 6
    h = Handle(ctx, o, v, f, blocks)
    try:
        h.set(t1, t2)
        e, batches = _triples(ctx, h)
        e_one, batches_one = _triples(ctx, h, fixed + unit)
        e_few, batches_few = _triples(ctx, h, fixed + 7 * unit)
        ctx.sync()
        before = ctx.mem_info()[0]
        res = (c_dbl * 2)(np.nan, np.nan)
        rc = lib.dmk_rccsd_t(h.h, fixed + unit - 1, res)
        after = ctx.mem_info()[0]
        e_after, _ = _triples(ctx, h)
    finally:
        h.close()
    print("(o, v) = (%d, %d): %d / %d / %d batches for the default budget / one triple / seven triples in flight" % (o, v, batches, batches_one, batches_few))
    assert batches == 1 and batches_one == ntr and batches_few == (ntr + 6) // 7
    assert np.array_equal(_bits(e), _bits(e_one)) and np.array_equal(_bits(e), _bits(e_few)) and np.array_equal(_bits(e), _bits(e_after))
    assert rc == DMK_ERR_NOMEM and np.isnan(res[0]) and after == before


@functools.lru_cache(maxsize=None)
def _solved(n, o, seed):
    """(CCSolver after run, system, E): shared, never modified."""
    from libdmet_preview_amd.solver import cc_solver
    from libdmet_preview_amd.system import integral
    sysm = R.System(n, seed, [o])
    Ham = integral.Integral(n, True, False, 0.0, {"cd": sysm.h1[None].copy()}, {"ccdd": sysm.blocks_s4()[:1].copy()})
    solver = cc_solver.CCSolver(restricted=True, tol=1e-12, tol_normt=1e-10)
    _, E = solver.run(Ham, nelec=2 * o)
    return solver, sysm, E


@pytest.mark.parametrize("n,o,seed", [(6, 2, 2207), (17, 8, 17)])
def test_solver_end_to_end(ctx, n, o, seed):
    from libdmet_preview_amd.solver import cc_lambda, ccsd_t
    solver, sysm, E = _solved(n, o, seed)
    v = n - o
    obj = solver.cisolver
    assert isinstance(obj, cc_lambda.RCCSDLambda) and obj.converged
    e_t = solver.ccsd_t()
    f, blocks = CR.restricted_blocks(sysm, obj._mo(), o)
    e_ref, s = TR.t_closed_shell(f, blocks, obj.t1, obj.t2, np.longdouble)
    print("n = %d: E_CCSD = %.12f, E_(T) = %.15e, reference %.15e, |d| = %.3e = %.4f of the bound"
          % (n, E, e_t, e_ref, abs(e_t - e_ref), abs(e_t - e_ref) / bound(o, v, s)))
    assert e_t < 0.0 and abs(e_t - e_ref) <= bound(o, v, s) and abs(e_ref) > 1e3 * bound(o, v, s)
    assert obj.e_t == e_t
    assert np.array_equal(_bits(obj.ccsd_t()), _bits(e_t)) and np.array_equal(_bits(ccsd_t.kernel(obj)), _bits(e_t))
    assert np.array_equal(_bits(ccsd_t.kernel(obj, max_memory=0.0625)), _bits(e_t))   # 64 KiB: many batches, the same bits
    with pytest.raises(MemoryError, match="max_memory"):
        ccsd_t.kernel(obj, max_memory=1e-4)
    # (T) left the CCSD state alone: the density of the run is still what make_rdm1 gives
    c = obj._mo()
    assert np.abs(2.0 * solver.onepdm[0] - c @ obj.make_rdm1() @ c.T).max() <= 1e-13
    assert np.array_equal(_bits(obj.ccsd_t(obj.t1, obj.t2)), _bits(e_t))          # given amplitudes: the same ones


def test_triples_give_their_memory_back(ctx):
    """The mechanism of tests/test_gpu_ccsd.py: sync, trim, mem_info after every round; ten rounds end no more than 1 MiB below the
    mark taken after the first."""
    from libdmet_preview_amd.solver import ccsd_t
    solver, _, _ = _solved(17, 8, 17)
    mark = free = None
    for it in range(1 + 10):
        ccsd_t.kernel(solver.cisolver)
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == 0:
            mark = free
    assert mark - free < (1 << 20), (mark, free)
