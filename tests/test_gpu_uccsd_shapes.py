"""
The dmk_uccsd handle through the C ABI at uneven shapes, over HOST blocks (no device SCF): the orbitals of the numpy
UHF of tests/scf_ref.py on System(n, 600 + 37 oa + ob, [oa, ob]) and tests/uccsd_ref.ints_u, against the spin-orbital reference of
tests/ccsd_ref.py (through tests/uccsd_ref.py).  The packed blocks have the pitch npair + 3 with a NaN pad: a read of the pad shows.

Shapes     (n, [oa, ob]): the smallest system, one extent of 1 on each side, strongly unequal extents in both directions, and extents
           past the 32-wide permute tile on one side only: (2,[1,1]), (3,[2,1]), (4,[1,3]), (6,[5,1]), (36,[33,3]), (42,[2,40]); each as
           it stands (canonical: f_ov = 0) and with rotated orbitals (ccsd_ref.rotate_ov, a different angle per spin).
Checks     the MP2 guess and its energy, the energy of random amplitudes and ONE update, all to 1e-10 max-abs; a second set + update
           returns the same bits; the state errors.
DIIS       at (7,[4,3]): a ring of one vector is plain iteration bit for bit; rings of 2 and 3 wrap and land on the DIIS-free
           reference within 10 delta + 1e-10 (delta: the reference's own convergence uncertainty, as in tests/test_gpu_ccsd.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import uccsd_ref as UR

pytestmark = pytest.mark.gpu

DMK_OK, DMK_ERR_INVALID, DMK_ERR_STATE = 0, -1, -5
TOL = 1e-10
PAD = 3
SHAPES = [(2, (1, 1)), (3, (2, 1)), (4, (1, 3)), (6, (5, 1)), (36, (33, 3)), (42, (2, 40))]
DIIS_SHAPE = (7, (4, 3))
TOL_E, TOL_NORMT = 1e-12, 1e-10
EMP2 = 5


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


class Handle(object):
    """One dmk_uccsd over host blocks uploaded here (the handle borrows them: they live as long as this object)."""

    def __init__(self, ctx, oa, va, ob, vb, fa, fb, blocks, diis=0):
        from libdmet_preview_amd._lib import lib, c_vp
        from libdmet_preview_amd.solver.uccsd import _Ints, _BLOCKS
        assert tuple(_BLOCKS) == tuple(UR.BLOCKS_U)
        self.ctx, self.lib, self.ext = ctx, lib, (oa, va, ob, vb)
        self.dev = {k: ctx.to_device(blocks[k]) for k in UR.BLOCKS_U}
        self.dev["fock_a"], self.dev["fock_b"] = ctx.to_device(fa), ctx.to_device(fb)
        self.ints = _Ints(ld_vvvv=blocks["vvvv"].shape[1], ld_VVVV=blocks["VVVV"].shape[1], ld_vvVV=blocks["vvVV"].shape[1],
                          **{k: d.ptr for k, d in self.dev.items()})
        self.h = c_vp()
        ctx.check(lib.dmk_uccsd_create(ctx.h, oa, va, ob, vb, C.byref(self.ints), diis, C.byref(self.h)))

    def shapes(self):
        oa, va, ob, vb = self.ext
        return (oa, va), (ob, vb), (oa, oa, va, va), (oa, ob, va, vb), (ob, ob, vb, vb), (1,)

    def close(self):
        h, self.h = self.h, None
        if h:
            self.ctx.check(self.lib.dmk_uccsd_free(h))

    def init(self):
        self.ctx.check(self.lib.dmk_uccsd_init(self.h))

    def set(self, amps):
        dev = [self.ctx.to_device(np.ascontiguousarray(a)) for a in amps]
        self.ctx.check(self.lib.dmk_uccsd_set(self.h, *[d.ptr for d in dev]))

    def get(self, what):
        d = self.ctx.empty(self.shapes()[what], np.float64)
        self.ctx.check(self.lib.dmk_uccsd_get(self.h, what, d.ptr))
        return d.get()

    def amps(self):
        return tuple(self.get(k) for k in range(5))

    def energy(self):
        d = self.ctx.empty((1,), np.float64)
        self.ctx.check(self.lib.dmk_uccsd_energy(self.h, d.ptr))
        return float(d.get()[0])

    def update(self):
        self.ctx.check(self.lib.dmk_uccsd_update(self.h))

    def run(self, max_iter, tol_e=TOL_E, tol_normt=TOL_NORMT):
        """-> (e_corr, converged, iterations, |dt|, dE)"""
        from libdmet_preview_amd._lib import c_dbl
        res = (c_dbl * 5)(*([np.nan] * 5))
        self.ctx.check(self.lib.dmk_uccsd_run(self.h, int(max_iter), tol_e, tol_normt, res))
        return tuple(float(x) for x in res)


@functools.lru_cache(maxsize=None)
def _host(n, nocc, rotated):
    """(spin-orbital Hamiltonian, Fock matrices, blocks with the padded NaN pitch) at the host orbitals of the case."""
    oa, ob = nocc
    sysm, Ca, Cb = UR.uneven_system_u(n, oa, ob)
    if rotated:
        Ca, Cb = CR.rotate_ov(Ca, oa, 0.05), CR.rotate_ov(Cb, ob, -0.08)
    so = UR.spin_orbital_u(sysm, Ca, Cb, oa, ob)
    fa, fb, blocks = UR.ints_u(sysm, Ca, Cb, oa, ob, pad=PAD)
    return so, fa, fb, blocks


def _maxerr(xs, ys):
    assert all(x.shape == y.shape for x, y in zip(xs, ys))
    return max(float(np.abs(x - y).max()) for x, y in zip(xs, ys))


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("n,nocc", SHAPES)
def test_guess_energy_and_one_update_at_uneven_shapes(ctx, n, nocc, rotated):
    so, fa, fb, blocks = _host(n, nocc, rotated)
    oa, ob = nocc
    va, vb = n - oa, n - ob
    for f, o in ((fa, oa), (fb, ob)):
        assert (np.diag(f)[:o, None] - np.diag(f)[None, o:]).max() <= -1.0                        # no denominator near zero
    if rotated:
        assert np.abs(fa[:oa, oa:]).max() > 1e-3 and np.abs(fb[:ob, ob:]).max() > 1e-3          # the initial t1 is not zero
    G1, G2 = CR.mp2_guess(so)
    guess = UR.from_so_u(G1, G2, oa, va)
    emp2_ref = CR.energy(so, 0.0 * G1, G2)
    amps = UR.random_amplitudes_u(np.random.default_rng(100 + n), oa, ob, va, vb)
    e_ref = UR.u_energy(so, amps)
    new = UR.u_update(so, amps)
    h = Handle(ctx, oa, va, ob, vb, fa, fb, blocks, diis=0)
    try:
        h.init()
        got_guess, emp2 = h.amps(), float(h.get(EMP2)[0])
        h.set(amps)
        e = h.energy()
        h.update()
        u = h.amps()
        h.set(amps)
        h.update()
        w = h.amps()
    finally:
        h.close()
    errs = (_maxerr(got_guess, guess), abs(emp2 - emp2_ref), abs(e - e_ref), _maxerr(u, new))
    print("n = %d, nocc = %s%s: guess max|dt| = %.3e |d emp2| = %.3e;  |de| = %.3e;  update max|dt| = %.3e  (max|t2ab new| = %.3f)"
          % ((n, nocc, " rotated" if rotated else "") + errs + (np.abs(new[3]).max(),)))
    for x in got_guess + u + (np.asarray([emp2, e]),):
        assert np.all(np.isfinite(x))
    assert max(errs) <= TOL
    assert _same_bits(u, w)                                           # two updates, the same bits


# ---- DIIS and the run loop -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diis_case():
    """The (7, [4, 3]) case, shared by the tests below and never modified: (so, fa, fb, blocks, converged DIIS-free reference)."""
    so, fa, fb, blocks = _host(DIIS_SHAPE[0], DIIS_SHAPE[1], False)
    return so, fa, fb, blocks, UR.converged_reference_u(so)


def _handle(ctx, diis):
    n, (oa, ob) = DIIS_SHAPE
    _, fa, fb, blocks, _ = _diis_case()
    return Handle(ctx, oa, n - oa, ob, n - ob, fa, fb, blocks, diis=diis)


def _solve(ctx, diis, max_iter=200):
    """init + run: (result, amplitudes, dmk_uccsd_energy of the amplitudes the handle holds after the run)."""
    h = _handle(ctx, diis)
    try:
        h.init()
        res = h.run(max_iter)
        return res, h.amps(), h.energy()
    finally:
        h.close()


def test_a_ring_of_one_vector_is_plain_iteration_bit_for_bit(ctx):
    (r0, a, _), (r1, b, _) = _solve(ctx, 0), _solve(ctx, 1)
    print("diis 0: e = %.15f, %d iterations;  diis 1: e = %.15f, %d iterations" % (r0[0], r0[2], r1[0], r1[2]))
    assert r0[1] == 1.0 and r1[1] == 1.0 and r0[2] == r1[2]
    assert np.array_equal(_bits(r0[0]), _bits(r1[0])) and _same_bits(a, b)


@pytest.mark.parametrize("diis", [2, 3])
def test_small_rings_wrap_and_converge_to_the_reference(ctx, diis):
    (e_ref, ref), de, dt = _diis_case()[4]
    res, amps, e = _solve(ctx, diis)
    errs = (abs(res[0] - e_ref), _maxerr(amps, ref))
    print("diis %d: reference delta_e = %.3e, delta_t = %.3e;  e_corr = %.12f, %d iterations, |de| = %.3e, max|dt| = %.3e"
          % ((diis, de, dt, res[0], res[2]) + errs))
    assert res[1] == 1.0 and res[2] > diis                            # more iterations than slots: the ring wrapped
    assert errs[0] <= 10.0 * de + 1e-10 and errs[1] <= 10.0 * dt + 1e-10
    assert np.array_equal(_bits(res[0]), _bits(e))                    # the energy returned belongs to the amplitudes returned


def test_handle_reports_state_errors_and_refuses_bad_arguments(ctx):
    from libdmet_preview_amd._lib import lib, c_vp, c_dbl
    n, (oa, ob) = DIIS_SHAPE
    va, vb = n - oa, n - ob
    h = _handle(ctx, 2)
    try:
        d = ctx.empty((oa, oa, va, va), np.float64)
        assert lib.dmk_uccsd_energy(h.h, d.ptr) == DMK_ERR_STATE                       # a fresh handle has no amplitudes
        assert lib.dmk_uccsd_update(h.h) == DMK_ERR_STATE
        for what in range(6):
            assert lib.dmk_uccsd_get(h.h, what, d.ptr) == DMK_ERR_STATE
        res = (c_dbl * 5)()
        assert lib.dmk_uccsd_run(h.h, -1, TOL_E, TOL_NORMT, res) == DMK_ERR_INVALID
        assert lib.dmk_uccsd_run(h.h, 5, TOL_E, TOL_NORMT, None) == DMK_ERR_INVALID
        assert lib.dmk_uccsd_update(h.h) == DMK_ERR_STATE                              # the refused runs made no guess
        assert lib.dmk_uccsd_set(h.h, d.ptr, d.ptr, None, d.ptr, d.ptr) == DMK_ERR_INVALID
        out = c_vp()

        def create(e=(oa, va, ob, vb), ints=h.ints, diis=2, res=C.byref(out)):
            return lib.dmk_uccsd_create(ctx.h, e[0], e[1], e[2], e[3], C.byref(ints) if ints is not None else None, diis, res)

        for k in range(4):
            for bad in (0, 513):
                e = [oa, va, ob, vb]
                e[k] = bad
                assert create(e=e) == DMK_ERR_INVALID and not out.value, (k, bad)
        for kw in (dict(diis=-1), dict(diis=13), dict(res=None), dict(ints=None)):
            assert create(**kw) == DMK_ERR_INVALID and not out.value, kw
        from libdmet_preview_amd.solver.uccsd import _Ints
        for name, _ in _Ints._fields_:
            bad = _Ints.from_buffer_copy(h.ints)
            setattr(bad, name, 0 if name.startswith("ld_") else None)                  # a pitch below npair, or a NULL block
            assert create(ints=bad) == DMK_ERR_INVALID and not out.value, name
        assert lib.dmk_uccsd_free(None) == DMK_OK
        assert create() == DMK_OK and out.value                                        # (the arguments themselves are good)
        assert lib.dmk_uccsd_free(out) == DMK_OK
    finally:
        h.close()
