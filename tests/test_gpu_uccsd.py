"""
Unrestricted CCSD on the device over a converged device UHF: solver/uccsd.py (UCCSD) and cc.run_ccsd against the
spin-orbital reference of tests/ccsd_ref.py, built from two sets of orbitals by tests/uccsd_ref.py and evaluated at the DEVICE's own
orbitals, so that only the CC code is measured (set up as tests/test_gpu_ccsd.py: SCF tolerance 1e-12, orbital gradient 1e-10).
System(n, seed, [oa, ob]) has different alpha and beta integral factors: a swapped or transposed block shows.

One step / energy   random amplitudes of scale 0.1 (t2aa / t2bb antisymmetric), 1e-10 max-abs (the project's TOL), at (n, Sz) = (6, 0),
                    (6, 2), (7, 1) (seven electrons), (17, 2), (65, 2) (oa, ob, va, vb = 33, 31, 32, 34: every permute tile edge with
                    unequal extents; its cost is the CPU reference) and at (17, 2) with NON-CANONICAL orbitals, each spin rotated by its
                    own angle (f_ov != 0, f_oo not diagonal: asserted first).
Two electrons       nocc [1, 1], n = 4 and 9: E_HF + E_corr is the lowest eigenvalue of h x 1 + 1 x h + (pr|qs)_ab within 1e-9.
Closed-shell limit  B = A, n = 6: UCCSD at the restricted orbitals equals cc.RCCSD (1e-10 in the energy, 1e-9 in t2ab = t2 and
                    t2aa = t2 - t2^T(ab)).
Converged           (6, 2) and (17, 2) with a ring of 8 and without, tol 1e-12 / 1e-10, within 10 delta + 1e-10 of the DIIS-free
                    reference (delta: its own convergence uncertainty; the factor 10 as in tests/test_gpu_ccsd.py); DIIS needs fewer
                    iterations; a restart from the result takes <= 2 cycles; emp2 is mp.UIMP2's to 1e-12; the energy returned is, bit
                    for bit, energy() of the amplitudes returned.
Dispatch, memory    cc.run_ccsd over an unrestricted solver; max_memory; ten create / run / free rounds give their memory back.
"""
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import scf_ref as R
from tests import uccsd_ref as UR
from tests.test_gpu_mp2 import _dev_block

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCF_TOL = 1e-12
SCF_GRAD = 1e-10
CASES = [(6, 0), (6, 2), (7, 1), (17, 2), (65, 2)]


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _nocc(n, Sz):
    ne = R.nelec_of(n) + (Sz % 2)                    # an odd Sz: one more electron
    return [(ne + Sz) // 2, (ne - Sz) // 2]


def _uhf(sysm, nocc, nblk=3):
    from libdmet_preview_amd import _lib
    from libdmet_preview_amd.solver import scf
    ctx = _lib.get_ctx()
    s = scf.SCF(newton_ah=False)
    s.set_system(nocc[0] + nocc[1], nocc[0] - nocc[1], False, False)
    s.set_integral_dev(sysm.n, 0.0, ctx.to_device(sysm.h1[None]), None, [_dev_block(ctx, sysm, w) for w in ("aa", "bb", "ab")[:nblk]])
    s.HF(tol=SCF_TOL, MaxIter=100, conv_tol_grad=SCF_GRAD)
    assert s.mf.converged
    return s


@functools.lru_cache(maxsize=None)
def _converged(n, Sz):
    """One converged device UHF per case, shared by the tests (never modified): (solver, system, nocc)."""
    nocc = _nocc(n, Sz)
    sysm = R.System(n, 700 + n + Sz, nocc)
    s = _uhf(sysm, nocc)
    occ = np.asarray(s.mf.mo_occ)
    assert [int(round(occ[k].sum())) for k in range(2)] == nocc
    return s, sysm, nocc


def _ordered(s, nocc):
    """The device's orbitals per spin, [occupied | virtual], and the matching occupations."""
    c, occ = np.asarray(s.mf.mo_coeff), np.asarray(s.mf.mo_occ)
    order = [np.concatenate([np.flatnonzero(occ[k] > 0), np.flatnonzero(occ[k] <= 0)]) for k in range(2)]
    n = c.shape[-1]
    return [c[k][:, order[k]] for k in range(2)], np.asarray([[1.0] * nocc[k] + [0.0] * (n - nocc[k]) for k in range(2)])


@functools.lru_cache(maxsize=None)
def _reference(n, Sz, rotated):
    """(spin-orbital Hamiltonian at the device's orbitals, orbitals, occupations, random amplitudes, their reference step and energy)."""
    s, sysm, nocc = _converged(n, Sz)
    (Ca, Cb), occ = _ordered(s, nocc)
    if rotated:
        Ca, Cb = CR.rotate_ov(Ca, nocc[0], 0.05), CR.rotate_ov(Cb, nocc[1], -0.08)
    so = UR.spin_orbital_u(sysm, Ca, Cb, nocc[0], nocc[1])
    amps = UR.random_amplitudes_u(np.random.default_rng(100 + n + Sz), nocc[0], nocc[1], n - nocc[0], n - nocc[1])
    return so, np.asarray([Ca, Cb]), occ, amps, UR.u_update(so, amps), UR.u_energy(so, amps)


@functools.lru_cache(maxsize=None)
def _converged_reference(n, Sz):
    return UR.converged_reference_u(_reference(n, Sz, False)[0])


def _maxerr(xs, ys):
    assert all(x.shape == y.shape for x, y in zip(xs, ys))
    return max(float(np.abs(x - y).max()) for x, y in zip(xs, ys))


def _flat(t1, t2):
    return tuple(t1) + tuple(t2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,Sz,rotated", [c + (False,) for c in CASES] + [(17, 2, True)])
def test_one_update_and_the_energy_against_the_spin_orbital_reference(ctx, n, Sz, rotated):
    from libdmet_preview_amd.solver import uccsd
    s, sysm, nocc = _converged(n, Sz)
    so, Cmo, occ, amps, new, e_ref = _reference(n, Sz, rotated)
    if rotated:
        fa, fb = so.f_mo
        for f, o in ((fa, nocc[0]), (fb, nocc[1])):
            assert np.abs(f[:o, o:]).max() > 1e-3 and np.abs(f[:o, :o] - np.diag(np.diag(f[:o, :o]))).max() > 1e-4
    obj = uccsd.UCCSD(s.mf, mo_coeff=Cmo, mo_occ=occ)
    try:
        assert obj.nocc == tuple(nocc)
        e = obj.energy(amps[:2], amps[2:])
        t1, t2 = obj.update_amps(amps[:2], amps[2:])
    finally:
        obj.close()
    errs = (abs(e - e_ref), _maxerr(_flat(t1, t2), new))
    print("n = %d, Sz = %d, nocc = %s%s: |de| = %.3e, update max|dt| = %.3e (max|t2ab new| = %.3f)"
          % ((n, Sz, nocc, " rotated" if rotated else "") + errs + (np.abs(new[3]).max(),)))
    assert max(errs) <= TOL


@pytest.mark.parametrize("n,seed", [(4, 71), (9, 72)])
def test_two_electrons_are_exact(ctx, n, seed):
    from libdmet_preview_amd.solver import uccsd
    sysm = R.System(n, seed, [1, 1])
    s = _uhf(sysm, [1, 1])
    obj = uccsd.UCCSD(s.mf)
    obj.conv_tol, obj.conv_tol_normt = 1e-12, 1e-10
    try:
        e_corr, t1, t2 = obj.kernel()
        assert obj.converged
    finally:
        obj.close()
    exact, gap = UR.exact_two_electron(sysm)
    print("n = %d: E_HF + E_corr = %.12f, exact = %.12f (gap %.2f), %d iterations" % (n, s.mf.e_tot + e_corr, exact, gap, obj.cycles))
    assert abs(s.mf.e_tot + e_corr - exact) <= 1e-9 and obj.e_tot == s.mf.e_tot + e_corr
    # one electron per spin: t_ii^ab is stored (the arrays are kept in full) and vanishes by antisymmetry, up to the rounding of terms
    # that cancel in pairs
    assert t2[1].shape == (1, 1, n - 1, n - 1) and np.abs(t2[0]).max() <= 1e-15 and np.abs(t2[2]).max() <= 1e-15


def test_closed_shell_limit_equals_rccsd(ctx):
    from libdmet_preview_amd.solver import cc, scf, uccsd
    n, o = 6, 3
    sysm = R.System(n, 11, [o])
    sysm.B = sysm.A
    r = scf.SCF(newton_ah=False)
    r.set_system(2 * o, 0, False, True)
    r.set_integral_dev(n, 0.0, ctx.to_device(sysm.h1[None]), None, [_dev_block(ctx, sysm, "aa")])
    r.HF(tol=SCF_TOL, MaxIter=100, conv_tol_grad=SCF_GRAD)
    u = _uhf(sysm, [o, o])
    robj = cc.RCCSD(r.mf)
    c, occ = np.asarray(r.mf.mo_coeff), np.asarray(r.mf.mo_occ)
    uobj = uccsd.UCCSD(u.mf, mo_coeff=np.asarray([c, c]), mo_occ=np.asarray([occ, occ]) * 0.5)
    for obj in (robj, uobj):
        obj.conv_tol, obj.conv_tol_normt = 1e-12, 1e-10
    try:
        e_r, t1, t2 = robj.kernel()
        e_u, (t1a, t1b), (t2aa, t2ab, t2bb) = uobj.kernel()
        assert robj.converged and uobj.converged
    finally:
        robj.close()
        uobj.close()
    same = t2 - t2.transpose(0, 1, 3, 2)
    errs = (abs(e_u - e_r), _maxerr((t1a, t1b, t2ab, t2aa, t2bb), (t1, t1, t2, same, same)))
    print("closed shell: e_r = %.12f, e_u = %.12f, |de| = %.3e, max|dt| = %.3e" % ((e_r, e_u) + errs))
    assert errs[0] <= 1e-10 and errs[1] <= 1e-9


@functools.lru_cache(maxsize=None)
def _solved(n, Sz, diis):
    """One converged device UCCSD per (case, ring), shared and never modified: (result dict of host values)."""
    from libdmet_preview_amd.solver import uccsd
    s, _, _ = _converged(n, Sz)
    obj = uccsd.UCCSD(s.mf)
    obj.conv_tol, obj.conv_tol_normt, obj.diis_space = 1e-12, 1e-10, diis
    try:
        e_corr, t1, t2 = obj.kernel()
        out = {"e": e_corr, "amps": _flat(t1, t2), "converged": obj.converged, "cycles": obj.cycles, "emp2": obj.emp2,
               "energy": obj.energy(t1, t2)}
        e2, _, _ = obj.kernel(t1=t1, t2=t2)
        out["restart"] = (e2, obj.cycles, obj.converged)
    finally:
        obj.close()
    return out


@pytest.mark.parametrize("diis", [8, 0])
@pytest.mark.parametrize("n,Sz", [(6, 2), (17, 2)])
def test_converged_amplitudes_against_the_reference(ctx, n, Sz, diis):
    from libdmet_preview_amd.solver import mp
    (e_ref, ref), de, dt = _converged_reference(n, Sz)
    got = _solved(n, Sz, diis)
    errs = (abs(got["e"] - e_ref), _maxerr(got["amps"], ref))
    print("n = %d, Sz = %d, diis %d: reference delta_e = %.3e, delta_t = %.3e;  e_corr = %.12f, %d iterations, |de| = %.3e, max|dt| = %.3e; "
          "restart %d cycle(s)" % ((n, Sz, diis, de, dt, got["e"], got["cycles"]) + errs + (got["restart"][1],)))
    assert got["converged"] and errs[0] <= 10.0 * de + 1e-10 and errs[1] <= 10.0 * dt + 1e-10
    assert np.array_equal(_bits(got["e"]), _bits(got["energy"]))      # the energy returned belongs to the amplitudes returned
    assert got["restart"][2] and got["restart"][1] <= 2 and abs(got["restart"][0] - got["e"]) <= 1e-11
    s, _, _ = _converged(n, Sz)
    emp2 = mp.UIMP2(s.mf).kernel(with_t2=False)[0]
    print("emp2 = %.15f, UIMP2 = %.15f" % (got["emp2"], emp2))
    assert abs(got["emp2"] - emp2) <= 1e-12


@pytest.mark.parametrize("n,Sz", [(6, 2), (17, 2)])
def test_diis_takes_fewer_iterations_than_plain_iteration(ctx, n, Sz):
    a, b = _solved(n, Sz, 8), _solved(n, Sz, 0)
    print("n = %d, Sz = %d: %d iterations with a ring of 8, %d without" % (n, Sz, a["cycles"], b["cycles"]))
    assert a["cycles"] < b["cycles"]


def test_run_ccsd_dispatches_and_memory_is_checked(ctx):
    from libdmet_preview_amd.solver import cc, uccsd
    n, Sz = 6, 2
    s, _, _ = _converged(n, Sz)
    want = _solved(n, Sz, 8)
    e_corr, t1, t2 = cc.run_ccsd(s, conv_tol=1e-12, conv_tol_normt=1e-10)
    try:
        assert isinstance(s.cc, uccsd.UCCSD) and s.cc.converged
        assert e_corr == want["e"] and all(np.array_equal(x, y) for x, y in zip(_flat(t1, t2), want["amps"]))
    finally:
        s.cc.close()
    obj = uccsd.UCCSD(s.mf)
    obj.max_memory = 1e-3
    plan = obj.memory_plan()
    assert set(plan) == {"handle", "workspace", "integrals", "transform"} and all(v > 0 for v in plan.values())
    with pytest.raises(MemoryError, match="max_memory"):
        obj.kernel()
    obj.close()


def test_uccsd_runs_give_their_memory_back(ctx):
    """The mechanism of tests/test_gpu_ccsd.py::test_ccsd_runs_give_their_memory_back: sync, trim, mem_info after every round; ten rounds
    of create / run / free at n = 17 end no more than 1 MiB below the mark taken after the first."""
    from libdmet_preview_amd.solver import uccsd
    s, _, _ = _converged(17, 2)
    mark = free = None
    for it in range(1 + 10):
        obj = uccsd.UCCSD(s.mf)
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
