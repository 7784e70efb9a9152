"""
The perturbative triples on the device (csrc/ccsd_t.hip) at the shapes and handle states tests/test_gpu_ccsd_t.py does
not reach: the wide workgroup tile cct_w_kernel<2> beyond its one shape (33, 3), more than one tile along i and k (o > 64), a second
particle K tile under the wide tile, full tiles, and (T) on handles that carry a DIIS ring, Lambda state or earlier amplitudes.

Everything goes through the C ABI alone (the last test excepted), on the host blocks of ccsd_ref.restricted_blocks with the
NaN-padded (vv|vv) pitch and the random amplitudes of ccsd_ref.random_amplitudes.  The reference is
ccsd_t_ref.t_closed_shell_streamed in float64 (O(o^3) memory; tests/test_host_ccsd_t.py holds it to t_closed_shell within 1e-13).
Tolerance: the derived bound of tests/test_gpu_ccsd_t.py, unchanged, |E_dev - E_ref| <= (2 (o + v) + 64) eps S.

Shapes (each the smallest that reaches its path; tile = the workgroup tile of cct_w_kernel, tiles = its count along i and along k)
    (32, 3)            <1>, 1 tile    the full 32-tile: no row or column masked
    (64, 3)            <2>, 1 tile    the full 64-tile, the production tile
    (48, 3)            <2>, 1 tile    the third MFMA block full, the fourth empty: a whole accumulator of a wave masked
    (65, 3)            <2>, 2 tiles   i0 / k0 = 64, a second tile with one valid row and column, five hole K tiles, one valid m in the last
    (129, 2)           <2>, 3 tiles   an odd tile count (% tiles against a power-of-two slip); four triples of 17 MB of W each
    (33, 17)           <2>, 1 tile    two particle K tiles with a masked tail f = 16, then three hole tiles: the staging switch at tt = 2
    (34, 17) rotated   <2>, 1 tile    the same with f_ov != 0
Fixtures: at every shape the host SCF converges, max(e_o - e_v) <= -1.28 (asserted <= -1) and |E_ref| is 5.7e9 .. 7.2e10 times the
bound (asserted > 1e3); no shape had to move.
Budgets at (65, 3) and (33, 17): the default, fixed + unit (one triple in flight), fixed + 3 unit: 1 / ntr / ceil(ntr / 3) batches, the
same bits; fixed + unit - 1 is refused with DMK_ERR_NOMEM, the result left NaN and nothing allocated.
State, at (4, 5) and (33, 3): (T) after init + four ringed iterations (unconverged, a ring of three wrapped) belongs to the amplitudes
the handle returns and leaves them and the energy alone; after lambda_init + lambda_update it gives the same bits and leaves Lambda
alone; set(A), T, set(B), T, set(A), T on one handle gives T(A), T(B) of a fresh handle, T(A), bit for bit.
Python: solver.ccsd_t.kernel with amplitudes other than the converged ones, then .ccsd_t() without arguments.

Measured (one MI355X, its host with 16 threads for the reference; profiles/ccsd_t_notes.txt)
    |E_dev - E_ref| as a fraction of the bound: (32, 3) 0, (64, 3) 7.5e-6, (48, 3) 5.4e-6, (65, 3) 0, (129, 2) 9.9e-7, (33, 17) 4.7e-5,
    (34, 17) rotated 0; after the ringed iterations 9.4e-5 at (4, 5) and 0 at (33, 3); through the Python module 8.4e-5.
    Streamed reference: 0.04 / 0.55 / 0.11 / 0.48 / 2.2 / 0.87 / 1.0 s in the order of the list (969 triples at v = 17: under the 10 s
    that would have traded (34, 17) for (34, 6)); building the blocks of (129, 2) takes 6.8 s on top (the (oo|oo) block the handle
    wants is 2.2 GB), which makes that case the slowest at 9.1 s; no other test takes more than 1.6 s.
    The 14 tests take 15.9 s together, references included (13.5 s in a second run).  These times belong to that host: the reference runs its chunks on up
    to 16 Python threads over a BLAS pool of the same size, and on 8 CPUs the v = 17 references take 6 .. 8 s (still under the 10 s).
Deliberate slips, each built once into a scratch library (never committed), every access still inside its arrays:
    i0 and k0 exchanged in the output store     red: (65, 3), (129, 2), the budgets at (65, 3); tests/test_gpu_ccsd_t.py stays green
    nkv = v / BK for the wide tile              drops the whole particle part below v = 16: red at every o > 32 here, and at (33, 3) of
                                                tests/test_gpu_ccsd_t.py as well
    nkv = max(v / BK, 1) for the wide tile      (only the tail chunk dropped) red: (33, 17), (34, 17) rotated, the budgets at (33, 17);
                                                tests/test_gpu_ccsd_t.py stays green
"""
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import ccsd_t_ref as TR
from tests.test_gpu_ccsd_shapes import Handle, PAD, _bits
from tests.test_gpu_ccsd_t import bound, _triples, _solved

pytestmark = pytest.mark.gpu

DMK_OK, DMK_ERR_NOMEM = 0, -3
CASES = [(32, 3, False), (64, 3, False), (48, 3, False), (65, 3, False), (129, 2, False), (33, 17, False), (34, 17, True)]
BUDGET_SHAPES = [(65, 3), (33, 17)]
STATE_SHAPES = [(4, 5), (33, 3)]
KEEP_BELOW = 100         # o from which a case is rebuilt instead of kept: the (oo|oo) block of (129, 2) alone is 2.2 GB of host memory


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _build(o, v, rotated):
    sysm, Cm = CR.uneven_system(o, v)                                 # asserts that the SCF converged
    if rotated:
        Cm = CR.rotate_ov(Cm, o)
    f, blocks = CR.restricted_blocks(sysm, Cm, o, pad=PAD)
    t1, t2 = CR.random_amplitudes(np.random.default_rng(1000 * o + v), o, v)
    e, s = TR.t_closed_shell_streamed(f, blocks, t1, t2)
    return f, blocks, t1, t2, e, s


_kept = functools.lru_cache(maxsize=None)(_build)


def _case(o, v, rotated):
    """(fock, blocks, t1, t2, E_ref, S): shared by the tests, never modified."""
    return _kept(o, v, rotated) if o < KEEP_BELOW else _build(o, v, rotated)


def _fixture_is_sound(o, v, f, e_ref, s):
    assert np.diag(f)[:o].max() - np.diag(f)[o:].min() <= -1.0        # no small denominator
    assert abs(e_ref) > 1e3 * bound(o, v, s)                          # the comparison resolves the number


@pytest.mark.parametrize("o,v,rotated", CASES)
def test_triples_at_the_wide_tile_shapes(ctx, o, v, rotated):
    f, blocks, t1, t2, e_ref, s = _case(o, v, rotated)
    _fixture_is_sound(o, v, f, e_ref, s)
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
    print("(o, v) = (%d, %d)%s: E_(T) = %.15e, reference %.15e, S = %.3e, |d| = %.3e = %.2e of the bound, %d batch(es)"
          % (o, v, " rotated" if rotated else "", e, e_ref, s, abs(e - e_ref), frac, batches))
    assert np.isfinite(e) and batches >= 1
    assert abs(e - e_ref) <= bound(o, v, s)
    assert np.array_equal(_bits(e), _bits(again))
    assert np.array_equal(_bits(g1), _bits(t1)) and np.array_equal(_bits(g2), _bits(t2)) and np.array_equal(_bits(e0), _bits(e1))


@pytest.mark.parametrize("o,v", BUDGET_SHAPES)
def test_budget_does_not_change_the_bits_at_the_wide_tile(ctx, o, v):
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
        e_few, batches_few = _triples(ctx, h, fixed + 3 * unit)
        ctx.sync()
        before = ctx.mem_info()[0]
        res = (c_dbl * 2)(np.nan, np.nan)
        rc = lib.dmk_rccsd_t(h.h, fixed + unit - 1, res)
        after = ctx.mem_info()[0]
    finally:
        h.close()
    print("(o, v) = (%d, %d): %d / %d / %d batches for the default budget / one triple / three triples in flight; |d| = %.2e of the bound"
          % (o, v, batches, batches_one, batches_few, abs(e - e_ref) / bound(o, v, s)))
    assert batches == 1 and batches_one == ntr and batches_few == (ntr + 2) // 3
    assert np.isfinite(e) and abs(e - e_ref) <= bound(o, v, s)
    assert np.array_equal(_bits(e), _bits(e_one)) and np.array_equal(_bits(e), _bits(e_few))
    assert rc == DMK_ERR_NOMEM and np.isnan(res[0]) and np.isnan(res[1]) and after == before


@pytest.mark.parametrize("o,v", STATE_SHAPES)
def test_triples_on_a_handle_with_a_ring_and_lambda_state(ctx, o, v):
    f, blocks = _case(o, v, False)[:2]
    h = Handle(ctx, o, v, f, blocks, diis=3)
    try:
        h.init()
        res = h.run(4)
        assert res[1] == 0.0 and res[2] == 4.0                        # unconverged, and four vectors went into a ring of three
        a1, a2 = h.amps()
        e0 = h.energy()
        e, _ = _triples(ctx, h)
        b1, b2 = h.amps()
        e1 = h.energy()
        h.lambda_init()
        h.lambda_update()
        l1, l2 = h.lams()
        e_l, _ = _triples(ctx, h)
        m1, m2 = h.lams()
        c1, c2 = h.amps()
    finally:
        h.close()
    e_ref, s = TR.t_closed_shell_streamed(f, blocks, a1, a2)
    print("(o, v) = (%d, %d), ring of 3 after 4 iterations: E_(T) = %.15e, reference %.15e, |d| = %.3e = %.2e of the bound"
          % (o, v, e, e_ref, abs(e - e_ref), abs(e - e_ref) / bound(o, v, s)))
    assert np.isfinite(e) and abs(e - e_ref) <= bound(o, v, s) and abs(e_ref) > 1e3 * bound(o, v, s)
    assert np.array_equal(_bits(a1), _bits(b1)) and np.array_equal(_bits(a2), _bits(b2)) and np.array_equal(_bits(e0), _bits(e1))
    assert np.array_equal(_bits(e_l), _bits(e))
    assert np.array_equal(_bits(l1), _bits(m1)) and np.array_equal(_bits(l2), _bits(m2))
    assert np.array_equal(_bits(a1), _bits(c1)) and np.array_equal(_bits(a2), _bits(c2))


@pytest.mark.parametrize("o,v", STATE_SHAPES)
def test_triples_follow_the_amplitudes_set_in_between(ctx, o, v):
    f, blocks, A1, A2, e_ref, s = _case(o, v, False)
    B1, B2 = CR.random_amplitudes(np.random.default_rng(7000 + 1000 * o + v), o, v)
    h, fresh = Handle(ctx, o, v, f, blocks), None
    try:
        h.set(A1, A2)
        e_a, _ = _triples(ctx, h)
        h.set(B1, B2)
        e_b, _ = _triples(ctx, h)
        h.set(A1, A2)
        e_a2, _ = _triples(ctx, h)
        fresh = Handle(ctx, o, v, f, blocks)
        fresh.set(B1, B2)
        e_b_fresh, _ = _triples(ctx, fresh)
    finally:
        h.close()
        if fresh is not None:
            fresh.close()
    print("(o, v) = (%d, %d): T(A) = %.15e, T(B) = %.15e, T(A) again = %.15e, T(B) on a fresh handle = %.15e" % (o, v, e_a, e_b, e_a2, e_b_fresh))
    assert abs(e_a - e_ref) <= bound(o, v, s)
    assert not np.array_equal(_bits(e_a), _bits(e_b))
    assert np.array_equal(_bits(e_a), _bits(e_a2)) and np.array_equal(_bits(e_b), _bits(e_b_fresh))


def test_given_amplitudes_become_current_through_the_python_module(ctx):
    from libdmet_preview_amd.solver import ccsd_t
    n, o = 6, 2
    solver, sysm, _ = _solved(n, o, 2207)
    obj = solver.cisolver
    t1c, t2c = obj.t1.copy(), obj.t2.copy()
    e_c = obj.ccsd_t()
    t1 = 1.1 * t1c
    t2 = 0.9 * t2c
    t2 = 0.5 * (t2 + t2.transpose(1, 0, 3, 2))
    assert np.abs(t2 - t2c).max() > 1e-4
    try:
        e = ccsd_t.kernel(obj, t1, t2)
        e_now = obj.ccsd_t()                                          # no arguments: the amplitudes given above are the current ones
    finally:
        e_back = obj.ccsd_t(t1c, t2c)                                 # the cached object as the other tests expect it
    f, blocks = CR.restricted_blocks(sysm, obj._mo(), o)
    e_ref, s = TR.t_closed_shell_streamed(f, blocks, t1, t2)
    print("n = %d, other amplitudes: E_(T) = %.15e, reference %.15e, |d| = %.3e = %.2e of the bound; converged amplitudes %.15e"
          % (n, e, e_ref, abs(e - e_ref), abs(e - e_ref) / bound(o, n - o, s), e_c))
    assert abs(e - e_ref) <= bound(o, n - o, s) and abs(e_ref) > 1e3 * bound(o, n - o, s)
    assert abs(e - e_c) > 1e3 * bound(o, n - o, s)                    # not the number of the converged amplitudes
    assert np.array_equal(_bits(e_now), _bits(e))
    assert np.array_equal(_bits(e_back), _bits(e_c)) and obj.e_t == e_c
    # ccsd_t.kernel hands the given amplitudes to the handle only; the object's own t1 / t2 were never touched by it (what puts
    # the handle back is the bit-equal e_back above)
    assert np.array_equal(_bits(obj.t1), _bits(t1c)) and np.array_equal(_bits(obj.t2), _bits(t2c))
