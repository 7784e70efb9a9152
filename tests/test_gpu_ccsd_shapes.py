"""
The dmk_rccsd handle through the C ABI alone, at the shapes and settings the solver-level tests of
tests/test_gpu_ccsd.py never reach.  No device SCF and no dmk_ao2mo_s4: the Fock matrix and the seven blocks come from
ccsd_ref.restricted_blocks at the HOST orbitals of ccsd_ref.uneven_system, so only csrc/ccsd.hip is under test.

Uneven shapes   (o, v) with o != v, extents of 1 on either side, one side beyond a 32-tile of the permute and the other small: every
                case as it stands and with occupied-virtual rotated orbitals (f_ov != 0, so the initial t1 is non-zero).  The guess of
                dmk_rccsd_init (T1, T2, EMP2), the energy of random amplitudes and ONE update against the spin-orbital reference, to
                TOL = 1e-10 max-abs (the bound of tests/test_gpu_ccsd.py).  The packed (vv|vv) block has a pitch of npair + 3 whose pad
                is NaN: a handle that dropped the pitch, or read the pad, gives a non-finite or a wrong result.  A second set + update
                gives the same bits.
Refusals        DMK_ERR_STATE before init / set, the argument checks of create and run, free(NULL).
DIIS and run    at (o, v) = (3, 4), tol_e = 1e-12, tol_normt = 1e-10: a ring of one vector is plain iteration bit for bit (with m = 1
                dmk_diis_coeffs returns c / c = 1.0 exactly and the combination is fma(1, x, 0) = x); rings of 2 and 3 wrap many times
                and land on the DIIS-free reference within 10 delta + 1e-10 (delta: ccsd_ref.converged_reference); max_iter = 0
                returns the energy of the current amplitudes and leaves them alone; and after ANY run, converged or not, result[0] is
                bit for bit what dmk_rccsd_energy gives for the amplitudes the handle then holds (the same kernels in the same order)
                -- at the C ABI and through solver/cc.py.
Measured        uneven shapes: every error at most 1.1e-16 (largest: the t1 update at (3, 33) rotated; 9.0e-17 at (40, 2)); the ring of
                one vector and plain iteration take 14 iterations and agree in every bit; rings of 2 and 3 take 9 iterations and land
                within 1.6e-13 (energy) and 7.8e-13 (amplitudes) of the reference, whose delta is 7.8e-12 / 3.2e-11.

Out of reach: the M-chunk loop of Engine::gemm (more than 32 * 65535 rows of one product) needs o v^2 > 2.1e6; no test-sized shape
gets there, and there is no entry point to the engine other than the handle.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR

pytestmark = pytest.mark.gpu

DMK_OK, DMK_ERR_INVALID, DMK_ERR_STATE = 0, -1, -5          # include/libdmetk.h
T1, T2, EMP2, L1, L2 = 0, 1, 2, 3, 4
TOL = 1e-10
PAD = 3
SHAPES = [(1, 1), (2, 1), (1, 2), (5, 1), (1, 40), (40, 2), (33, 3), (3, 33), (2, 40)]
DIIS_SHAPE = (3, 4)
TOL_E, TOL_NORMT = 1e-12, 1e-10


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Handle(object):
    """One dmk_rccsd over host blocks uploaded here (the handle borrows them: they live as long as this object).  The Lambda entries
    are used by tests/test_gpu_cclambda_shapes.py."""

    def __init__(self, ctx, o, v, fock, blocks, diis=0):
        from libdmet_preview_amd._lib import lib, c_vp
        self.ctx, self.lib, self.o, self.v = ctx, lib, o, v
        self.dev = [ctx.to_device(fock)] + [ctx.to_device(blocks[k]) for k in CR.BLOCKS]
        self.h = c_vp()
        ctx.check(lib.dmk_rccsd_create(ctx.h, o, v, *([d.ptr for d in self.dev] + [blocks["vvvv"].shape[1], diis, C.byref(self.h)])))

    def close(self):
        h, self.h = self.h, None
        if h:
            self.ctx.check(self.lib.dmk_rccsd_free(h))

    def init(self):
        self.ctx.check(self.lib.dmk_rccsd_init(self.h))

    def set(self, t1, t2):
        d1, d2 = self.ctx.to_device(t1), self.ctx.to_device(t2)
        self.ctx.check(self.lib.dmk_rccsd_set(self.h, d1.ptr, d2.ptr))

    def get(self, what):
        o, v = self.o, self.v
        d = self.ctx.empty(((o, v), (o, o, v, v), (1,), (o, v), (o, o, v, v))[what], np.float64)
        self.ctx.check(self.lib.dmk_rccsd_get(self.h, what, d.ptr))
        return d.get()

    def amps(self):
        return self.get(T1), self.get(T2)

    def energy(self):
        d = self.ctx.empty((1,), np.float64)
        self.ctx.check(self.lib.dmk_rccsd_energy(self.h, d.ptr))
        return float(d.get()[0])

    def update(self):
        self.ctx.check(self.lib.dmk_rccsd_update(self.h))

    def run(self, max_iter, tol_e=TOL_E, tol_normt=TOL_NORMT):
        """-> (e_corr, converged, iterations, |dt|, dE)"""
        from libdmet_preview_amd._lib import c_dbl
        res = (c_dbl * 5)(*([np.nan] * 5))
        self.ctx.check(self.lib.dmk_rccsd_run(self.h, int(max_iter), tol_e, tol_normt, res))
        return tuple(float(x) for x in res)

    # ---- Lambda (tests/test_gpu_cclambda_shapes.py) ------------------------------------------------------------------------------
    def lambda_init(self):
        self.ctx.check(self.lib.dmk_rccsd_lambda_init(self.h))

    def lambda_set(self, l1, l2):
        d1, d2 = self.ctx.to_device(l1), self.ctx.to_device(l2)
        self.ctx.check(self.lib.dmk_rccsd_lambda_set(self.h, d1.ptr, d2.ptr))

    def lambda_update(self):
        self.ctx.check(self.lib.dmk_rccsd_lambda_update(self.h))

    def lambda_run(self, max_iter, tol_normt=TOL_NORMT):
        """-> (converged, iterations, |dl|)"""
        from libdmet_preview_amd._lib import c_dbl
        res = (c_dbl * 3)(*([np.nan] * 3))
        self.ctx.check(self.lib.dmk_rccsd_lambda_run(self.h, int(max_iter), tol_normt, res))
        return tuple(float(x) for x in res)

    def lams(self):
        return self.get(L1), self.get(L2)

    def rdm1(self):
        n = self.o + self.v
        d = self.ctx.empty((n, n), np.float64)
        self.ctx.check(self.lib.dmk_rccsd_rdm1(self.h, d.ptr))
        return d.get()

    def residual(self):
        o, v = self.o, self.v
        d1, d2 = self.ctx.empty((o, v), np.float64), self.ctx.empty((o, o, v, v), np.float64)
        self.ctx.check(self.lib.dmk_rccsd_residual(self.h, d1.ptr, d2.ptr))
        return d1.get(), d2.get()

    def lagrangian(self, l1, l2):
        d1, d2, d = self.ctx.to_device(l1), self.ctx.to_device(l2), self.ctx.empty((1,), np.float64)
        self.ctx.check(self.lib.dmk_rccsd_lagrangian(self.h, d1.ptr, d2.ptr, d.ptr))
        return float(d.get()[0])


def _host(o, v, rotated):
    """(spin-orbital Hamiltonian, Fock matrix, blocks with the padded NaN pitch) at the host orbitals of the case."""
    sysm, Cmo = CR.uneven_system(o, v)
    if rotated:
        Cmo = CR.rotate_ov(Cmo, o)
    so = CR.spin_orbital(sysm, Cmo, o)
    fock, blocks = CR.restricted_blocks(sysm, Cmo, o, pad=PAD)
    return so, fock, blocks


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("o,v", SHAPES)
def test_guess_energy_and_one_update_at_uneven_shapes(ctx, o, v, rotated):
    so, fock, blocks = _host(o, v, rotated)
    n = o + v
    d1 = so.eo[:o, None] - so.ev[None, :v]
    assert d1.max() <= -1.0                                           # no denominator near zero
    if rotated:
        assert np.abs(fock[:o, o:]).max() > 1e-3                      # the initial t1 is not zero
    G1, G2 = CR.mp2_guess(so)
    g1, g2 = CR.from_so(G1, G2)
    emp2_ref = CR.energy(so, 0.0 * G1, G2)
    t1, t2 = CR.random_amplitudes(np.random.default_rng(100 + n), o, v)
    e_ref = CR.r_energy(so, t1, t2)
    n1, n2 = CR.r_update(so, t1, t2)
    h = Handle(ctx, o, v, fock, blocks, diis=0)
    try:
        h.init()
        i1, i2, emp2 = h.get(T1), h.get(T2), float(h.get(EMP2)[0])
        h.set(t1, t2)
        e = h.energy()
        h.update()
        u1, u2 = h.amps()
        h.set(t1, t2)
        h.update()
        w1, w2 = h.amps()
    finally:
        h.close()
    errs = (np.abs(i1 - g1).max(), np.abs(i2 - g2).max(), abs(emp2 - emp2_ref), abs(e - e_ref), np.abs(u1 - n1).max(),
            np.abs(u2 - n2).max())
    print("(o, v) = (%d, %d)%s: guess max|d t1| = %.3e max|d t2| = %.3e |d emp2| = %.3e;  |de| = %.3e;  update max|d t1| = %.3e "
          "max|d t2| = %.3e  (max|t1 guess| = %.3f, max|t2new| = %.3f)"
          % ((o, v, " rotated" if rotated else "") + errs + (np.abs(g1).max(), np.abs(n2).max())))
    for x in (i1, i2, emp2, e, u1, u2):
        assert np.all(np.isfinite(x))
    assert u1.shape == n1.shape and u2.shape == n2.shape and max(errs) <= TOL
    assert np.array_equal(_bits(u1), _bits(w1)) and np.array_equal(_bits(u2), _bits(w2))          # two updates, the same bits


# ---- DIIS and the run loop -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diis_case():
    """The (3, 4) case, shared by the tests below and never modified: (so, fock, blocks, converged DIIS-free reference)."""
    so, fock, blocks = _host(DIIS_SHAPE[0], DIIS_SHAPE[1], False)
    return so, fock, blocks, CR.converged_reference(so)


def _handle(ctx, diis):
    _, fock, blocks, _ = _diis_case()
    return Handle(ctx, DIIS_SHAPE[0], DIIS_SHAPE[1], fock, blocks, diis=diis)


def _solve(ctx, diis, max_iter=200):
    """init + run: (result, t1, t2, dmk_rccsd_energy of the amplitudes the handle holds after the run)."""
    h = _handle(ctx, diis)
    try:
        h.init()
        res = h.run(max_iter)
        t1, t2 = h.amps()
        return res, t1, t2, h.energy()
    finally:
        h.close()


def test_a_ring_of_one_vector_is_plain_iteration_bit_for_bit(ctx):
    (r0, a1, a2, _), (r1, b1, b2, _) = _solve(ctx, 0), _solve(ctx, 1)
    print("diis 0: e = %.15f, %d iterations;  diis 1: e = %.15f, %d iterations" % (r0[0], r0[2], r1[0], r1[2]))
    assert r0[1] == 1.0 and r1[1] == 1.0 and r0[2] == r1[2]
    assert np.array_equal(_bits(r0[0]), _bits(r1[0])) and np.array_equal(_bits(a1), _bits(b1)) and np.array_equal(_bits(a2), _bits(b2))


@pytest.mark.parametrize("diis", [2, 3])
def test_small_rings_wrap_and_converge_to_the_reference(ctx, diis):
    (e_ref, t1_ref, t2_ref), de, dt = _diis_case()[3]
    res, t1, t2, _ = _solve(ctx, diis)
    errs = (abs(res[0] - e_ref), np.abs(t1 - t1_ref).max(), np.abs(t2 - t2_ref).max())
    print("diis %d: reference delta_e = %.3e, delta_t = %.3e;  e_corr = %.12f, %d iterations, |de| = %.3e, max|d t1| = %.3e, "
          "max|d t2| = %.3e" % ((diis, de, dt, res[0], res[2]) + errs))
    assert res[1] == 1.0 and res[2] > diis                            # more iterations than slots: the ring wrapped
    assert errs[0] <= 10.0 * de + 1e-10 and max(errs[1:]) <= 10.0 * dt + 1e-10


def test_no_iterations_returns_the_energy_of_the_guess_and_leaves_it(ctx):
    so = _diis_case()[0]
    g1, g2 = CR.from_so(*CR.mp2_guess(so))
    for diis in (0, 4):
        h = _handle(ctx, diis)
        try:
            h.init()
            t1, t2 = h.amps()
            e = h.energy()
            res = h.run(0)
            u1, u2 = h.amps()
        finally:
            h.close()
        assert np.array_equal(_bits(res[0]), _bits(e)) and res[1:] == (0.0, 0.0, 0.0, 0.0)
        assert abs(e - CR.r_energy(so, g1, g2)) <= TOL
        assert np.array_equal(_bits(t1), _bits(u1)) and np.array_equal(_bits(t2), _bits(u2))


@pytest.mark.parametrize("diis,max_iter", [(0, 1), (0, 3), (4, 1), (4, 3), (0, 200), (4, 200)])
def test_the_energy_returned_belongs_to_the_amplitudes_returned(ctx, diis, max_iter):
    res, t1, t2, e = _solve(ctx, diis, max_iter)
    print("diis %d, max_iter %d: result e = %.15f, energy of the handle's amplitudes = %.15f (difference %.3e), converged %d after %d"
          % (diis, max_iter, res[0], e, res[0] - e, res[1], res[2]))
    assert res[1] == (1.0 if max_iter == 200 else 0.0) and (res[1] == 1.0 or res[2] == max_iter)
    assert np.array_equal(_bits(res[0]), _bits(e))


def test_an_unconverged_kernel_returns_a_consistent_triple(ctx):
    from libdmet_preview_amd.solver import cc
    from tests.test_gpu_ccsd import _half_filled
    s, _ = _half_filled(6)
    obj = cc.RCCSD(s.mf)
    obj.conv_tol, obj.conv_tol_normt, obj.max_cycle = 1e-12, 1e-10, 3
    try:
        e_corr, t1, t2 = obj.kernel()
        assert not obj.converged and obj.cycles == 3 and obj.diis_space == 8 and e_corr == obj.e_corr
        e = obj.energy(obj.t1, obj.t2)
    finally:
        obj.close()
    print("max_cycle 3: e_corr = %.15f, energy(t1, t2) = %.15f" % (e_corr, e))
    assert e == obj.e_corr


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_handle_refuses_bad_states_and_arguments(ctx):
    from libdmet_preview_amd._lib import lib, c_vp, c_dbl
    o, v = DIIS_SHAPE
    _, fock, blocks, _ = _diis_case()
    npair = v * (v + 1) // 2
    h = Handle(ctx, o, v, fock, blocks, diis=2)
    try:
        d_e, d_t1 = ctx.empty((1,), np.float64), ctx.empty((o, v), np.float64)
        assert lib.dmk_rccsd_energy(h.h, d_e.ptr) == DMK_ERR_STATE                     # a fresh handle has no amplitudes
        assert lib.dmk_rccsd_update(h.h) == DMK_ERR_STATE
        for what in (T1, T2, EMP2):
            assert lib.dmk_rccsd_get(h.h, what, d_t1.ptr) == DMK_ERR_STATE
        res = (c_dbl * 5)()
        assert lib.dmk_rccsd_run(h.h, -1, TOL_E, TOL_NORMT, res) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_run(h.h, 5, TOL_E, TOL_NORMT, None) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_update(h.h) == DMK_ERR_STATE                              # the refused runs made no guess
        ptrs = [d.ptr for d in h.dev]
        out = c_vp()

        def create(nocc=o, nvir=v, p=ptrs, ld=npair + PAD, diis=2, res=C.byref(out)):
            return lib.dmk_rccsd_create(ctx.h, nocc, nvir, *(list(p) + [ld, diis, res]))

        for kw in (dict(nocc=0), dict(nocc=513), dict(nvir=0), dict(nvir=513), dict(diis=-1), dict(diis=13), dict(ld=npair - 1),
                   dict(res=None)):
            assert create(**kw) == DMK_ERR_INVALID and not out.value, kw
        for k in range(len(ptrs)):                                                     # the Fock matrix and each of the seven blocks
            assert create(p=ptrs[:k] + [None] + ptrs[k + 1:]) == DMK_ERR_INVALID and not out.value, k
        assert lib.dmk_rccsd_free(None) == DMK_OK
        assert create() == DMK_OK and out.value                                        # (the arguments themselves are good)
        assert lib.dmk_rccsd_free(out) == DMK_OK
    finally:
        h.close()
