"""
Restricted CCSD on the device over a converged device RHF: solver/cc.py (RCCSD, run_ccsd) against the spin-orbital
reference of tests/ccsd_ref.py evaluated at the DEVICE's own orbitals, so that only the CC code is measured (set up as
tests/test_gpu_mp2.py).

One step / energy   from random amplitudes of scale 0.1 with t_ij^ab = t_ji^ba (every term of the equations at full strength), at
                    n = 6, 17, 65 (o = 32, v = 33: off every tile) and at n = 17 with NON-CANONICAL orbitals (an occupied-virtual
                    rotation of angle 0.05: f_ov != 0, f_oo / f_vv not diagonal); 1e-10 max-abs, the TOL of the SCF / MP2 tests.
Converged           the two-electron systems of tests/test_host_ccsd.py against the exact singlet eigenvalue; n = 6 and n = 17 against
                    the converged reference.  The reference is run DIIS-free to |dt| < 1e-9 and on to 1e-11; the difference delta of
                    the two results is its convergence uncertainty, and the device (tol_e = 1e-12, tol_normt = 1e-10) must agree with
                    the tighter one within 10 delta + 1e-10 (the factor 10: DIIS lands on another iterate of the same fixed point).
                    Measured delta: n = 6: 9.2e-12 in the energy, 1.2e-10 in the largest amplitude difference; n = 17: 4.5e-12,
                    2.7e-11 (printed by the test; also in DESIGN.md K21).  The device lands within 2e-13 / 5e-12 of the tight reference.
emp2                equals mp.MP2(mf).kernel()[0] to 1e-12.  The two share their amplitudes only as far as the orbitals are canonical for
                    the Fock matrix of their OWN density (MP2 divides by the orbital energies, CCSD by the diagonal of that Fock
                    matrix), so the Hartree-Fock runs of this file are converged to an orbital gradient of 1e-10, not to the default
                    sqrt(tol) = 1e-6, at which the two energies differ by the SCF residual (measured 1.3e-12 at n = 6, 9.1e-12 at 17).
"""
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import scf_ref as R
from tests.test_gpu_mp2 import _dev_block
from tests.test_host_ccsd import TWO_ELECTRON

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCF_TOL = 1e-12
SCF_GRAD = 1e-10
SEED = {6: 11, 17: 17, 65: 12}          # n = 6 and 65: the listed cases of scf_ref.SEEDS


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@functools.lru_cache(maxsize=None)
def _converged(n, seed, nelec):
    """One converged device RHF per system, shared by the tests (never modified): (solver, system)."""
    from libdmet_preview_amd import _lib
    from libdmet_preview_amd.solver import scf
    ctx = _lib.get_ctx()
    sysm = R.System(n, seed, [nelec // 2])
    s = scf.SCF(newton_ah=False)
    s.set_system(nelec, 0, False, True)
    s.set_integral_dev(n, 0.0, ctx.to_device(sysm.h1[None]), None, [_dev_block(ctx, sysm, "aa")])
    s.HF(tol=SCF_TOL, MaxIter=100, conv_tol_grad=SCF_GRAD)
    assert s.mf.converged
    return s, sysm


def _half_filled(n):
    return _converged(n, SEED[n], R.nelec_of(n))


@functools.lru_cache(maxsize=None)
def _reference(n, rotated):
    """(spin-orbital Hamiltonian at the device's orbitals, orbitals, random amplitudes, their reference step and energy)."""
    s, sysm = _half_filled(n)
    o = n // 2
    C = np.asarray(s.mf.mo_coeff)
    if rotated:
        C = CR.rotate_ov(C, o)
    so = CR.spin_orbital(sysm, C, o)
    t1, t2 = CR.random_amplitudes(np.random.default_rng(100 + n), o, n - o)
    n1, n2 = CR.r_update(so, t1, t2)
    return so, C, (t1, t2), (n1, n2), CR.r_energy(so, t1, t2)


@functools.lru_cache(maxsize=None)
def _converged_reference(n):
    """DIIS-free reference at |dt| < 1e-9 and on to 1e-11: (tight result, delta_e, delta_t)."""
    return CR.converged_reference(_reference(n, False)[0])


@pytest.mark.parametrize("n,rotated", [(6, False), (17, False), (65, False), (17, True)])
def test_one_update_step_and_energy(ctx, n, rotated):
    from libdmet_preview_amd.solver import cc
    s, _ = _half_filled(n)
    so, C, (t1, t2), (n1, n2), e_ref = _reference(n, rotated)
    if rotated:
        assert np.abs(so.fov).max() > 1e-3 and np.abs(so.foo - np.diag(so.eo)).max() > 1e-4
    obj = cc.RCCSD(s.mf, mo_coeff=C if rotated else None)
    try:
        e = obj.energy(t1, t2)
        g1, g2 = obj.update_amps(t1, t2)
    finally:
        obj.close()
    errs = (abs(e - e_ref), np.abs(g1 - n1).max(), np.abs(g2 - n2).max())
    print("n = %d%s: |de| = %.3e  max|d t1| = %.3e  max|d t2| = %.3e  (max|t2new| = %.3f)"
          % ((n, " rotated" if rotated else "") + errs + (np.abs(n2).max(),)))
    assert g1.shape == n1.shape and g2.shape == n2.shape and max(errs) <= TOL


@pytest.mark.parametrize("n,seed", TWO_ELECTRON)
def test_two_electrons_are_exact(ctx, n, seed):
    from libdmet_preview_amd.solver import cc, mp
    s, sysm = _converged(n, seed, 2)
    exact = CR.exact_two_electron_singlet(sysm)
    obj = cc.RCCSD(s.mf)
    obj.conv_tol, obj.conv_tol_normt = 1e-12, 1e-10
    try:
        e_corr, t1, t2 = obj.kernel()
    finally:
        obj.close()
    print("n = %d: E_HF + E_corr = %.12f, exact = %.12f, %d iterations" % (n, s.mf.e_tot + e_corr, exact, obj.cycles))
    assert obj.converged and abs(s.mf.e_tot + e_corr - exact) <= 1e-9
    assert obj.e_tot == s.mf.e_tot + e_corr and t1.shape == (1, n - 1) and t2.shape == (1, 1, n - 1, n - 1)
    assert abs(obj.emp2 - mp.MP2(s.mf).kernel()[0]) <= 1e-12


@pytest.mark.parametrize("n", [6, 17])
def test_converged_against_the_reference_with_and_without_diis(ctx, n):
    from libdmet_preview_amd.solver import cc, mp
    s, _ = _half_filled(n)
    (e_ref, t1_ref, t2_ref), de, dt = _converged_reference(n)
    tol_e, tol_t = 10.0 * de + 1e-10, 10.0 * dt + 1e-10
    print("n = %d: reference delta_e = %.3e, delta_t = %.3e" % (n, de, dt))
    runs = {}
    for diis in (8, 0):
        obj = cc.RCCSD(s.mf)
        obj.conv_tol, obj.conv_tol_normt, obj.diis_space = 1e-12, 1e-10, diis
        try:
            e_corr, t1, t2 = obj.kernel()
            assert obj.converged and obj.e_corr == e_corr and obj.e_tot == s.mf.e_tot + e_corr
            errs = (abs(e_corr - e_ref), np.abs(t1 - t1_ref).max(), np.abs(t2 - t2_ref).max())
            print("n = %d diis %d: e_corr = %.12f, %d iterations, |de| = %.3e, max|d t1| = %.3e, max|d t2| = %.3e"
                  % ((n, diis, e_corr, obj.cycles) + errs))
            assert errs[0] <= tol_e and max(errs[1:]) <= tol_t
            assert np.array_equal(obj.t1, t1) and np.array_equal(obj.t2, t2)
            assert abs(obj.emp2 - mp.MP2(s.mf).kernel()[0]) <= 1e-12
            runs[diis] = (e_corr, obj.cycles)
            if diis:                                  # a restart from the converged amplitudes has nothing left to do
                e2, _, _ = obj.kernel(t1, t2)
                assert obj.converged and obj.cycles <= 2 and abs(e2 - e_corr) <= tol_e
        finally:
            obj.close()
    assert abs(runs[8][0] - runs[0][0]) <= tol_e and runs[8][1] < runs[0][1]


def test_run_ccsd_leaves_the_object_on_the_solver(ctx):
    from libdmet_preview_amd.solver import cc
    s, _ = _half_filled(6)
    (e_ref, _, _), de, _ = _converged_reference(6)
    e_corr, t1, t2 = cc.run_ccsd(s, conv_tol=1e-12, conv_tol_normt=1e-10)
    try:
        assert isinstance(s.cc, cc.RCCSD) and s.cc.converged and s.cc.e_corr == e_corr and s.cc.diis_space == 8
        assert abs(e_corr - e_ref) <= 10.0 * de + 1e-10 and t1.shape == (3, 3) and t2.shape == (3, 3, 3, 3)
        s.cc.max_memory = 1e-3                        # MB: the plan is compared before anything is allocated
        s.cc.close()
        with pytest.raises(MemoryError, match="max_memory"):
            s.cc.kernel()
        with pytest.raises(NotImplementedError, match="level shift"):
            cc.run_ccsd(s, level_shift=0.1)
    finally:
        s.cc.close()


def test_ccsd_runs_give_their_memory_back(ctx):
    """The mechanism of tests/test_gpu_handle_lifetime.py: sync, trim, mem_info after every round; ten rounds of create / run / free at
    n = 17 end no more than 1 MiB (that mechanism's bound) below the mark taken after the first."""
    from libdmet_preview_amd.solver import cc
    s, _ = _half_filled(17)
    mark = free = None
    for it in range(1 + 10):
        obj = cc.RCCSD(s.mf)
        obj.kernel()
        assert obj.converged
        obj.close()
        del obj
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == 0:
            mark = free
    assert mark - free < (1 << 20), (mark, free)
