"""
Host-side checks of the Lambda layer ("Lambda"), no GPU: the reference of tests/cclambda_ref.py validates itself (CCSD
with Lambda is exact for two electrons; the explicit density formulas are the derivative of the Lagrangian with respect to the Fock
matrix; that derivative is the response of the converged energy), the planner refuses what dmk_rccsd_plan refuses, and
solver/cc_lambda.py and solver/cc_solver.py import without a device and refuse by name what is not built.

Measured: two electrons, max|C gamma C^T - 2 X X^T| = 2e-15 (n = 5), 2e-14 (n = 6); formulas against the derivative <= 7e-18; central
difference of step 1e-4 against tr V gamma_corr 2e-9 .. 2e-8 (the bound 1e-6 covers the O(eps^2) term).

The REVERSE-MODE references (lambda_step_reverse, rdm1_reverse, grad_t_reverse: float64 CPU torch autograd through the one statement of
the amplitude equations in tests/ccsd_ref.py) are held here against the complex-step forms of the same file (the dense Jacobian, the loop
over Fock perturbations) where these can go, and against the closed-shell density formulas where they cannot, before
tests/test_gpu_cclambda_shapes.py holds the device against them.  Autograd and complex step share the equations and nothing else.
Bounds: 1e-13 between two exact derivatives of the same polynomial at random amplitudes of scale 0.1 (sums of at most a few thousand
terms of size <= 1: rounding, nothing else); 1e-12 against the formulas at (8, 9) and (3, 33), whose sums are ten times longer.
Measured: sweep against the Jacobian form 6.9e-17, density against complex step 5.6e-17, against the formulas 8.9e-16; the reference
sweep from l = t takes 21 sweeps to |dl|_2 < 1e-10 at (2, 3), coupling 2.0 (T: 38 plain iterations), and ends 2.7e-11 from the
solution of the Jacobian.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import cclambda_ref as LR
from tests import scf_ref as R
from tests.test_host_ccsd import TWO_ELECTRON, two_electron_hf

DMK_ERR_INVALID = -1
CASES = [(1, 4, 3.0, False), (2, 3, 2.0, True), (3, 4, 3.0, False)]          # (o, v, scale of the coupling, rotated orbitals)
JAC = [(1, 4, False), (2, 3, True), (3, 4, False)]                             # reverse mode against the dense Jacobian
RUN_SHAPE, RUN_SCALE = (2, 3), 2.0                                             # the run-loop system of tests/test_gpu_cclambda_shapes.py


@functools.lru_cache(maxsize=None)
def _solved(o, v, scale, rotated):
    """(spin-orbital Hamiltonian, t1, t2, l1, l2) of the converged DIIS-free reference and its Jacobian Lambda."""
    sysm = R.System(o + v, 500 + 37 * o + v, [o])
    sysm.lam *= scale
    ref = R.scf(sysm.h1[None], sysm.veff_rhf, [o], True)
    assert ref["converged"]
    Cmo = CR.rotate_ov(ref["mo_coeff"], o) if rotated else ref["mo_coeff"]
    so = CR.spin_orbital(sysm, Cmo, o)
    _, T1, T2, _ = CR.solve(so, 1e-12, max_iter=2000)
    l1, l2, _, _, L1, L2 = LR.lambda_by_jacobian(so, T1, T2, full=True)
    M1, M2 = CR.to_so(l1, l2)
    assert np.abs(M1 - L1).max() <= 1e-14 and np.abs(M2 - L2).max() <= 1e-14          # the spin-orbital Lambda is spin adapted
    return (so,) + CR.from_so(T1, T2) + (l1, l2)


@pytest.mark.parametrize("n,seed", TWO_ELECTRON)
def test_reference_density_is_exact_for_two_electrons(n, seed):
    sysm, ref = two_electron_hf(n, seed)
    Cmo = ref["mo_coeff"]
    so = CR.spin_orbital(sysm, Cmo, 1)
    _, T1, T2, _ = CR.solve(so, 1e-13, max_iter=2000)
    t1, t2 = CR.from_so(T1, T2)
    l1, l2 = LR.lambda_by_jacobian(so, T1, T2)
    e_fci, X = LR.fci_two_electron(sysm)
    gam = LR.rdm1_explicit(t1, t2, l1, l2)
    err = np.abs(Cmo @ gam @ Cmo.T - 2.0 * X @ X.T).max()
    e_l = ref["E"] + float(LR.lagrangian(so, t1, t2, l1, l2))
    print("n = %d: max|C gamma C^T - 2 X X^T| = %.3e, |E_HF + L - E_FCI| = %.3e" % (n, err, abs(e_l - e_fci)))
    assert err <= 1e-12 and abs(e_l - e_fci) <= 1e-9
    assert abs(LR.expval_ref(sysm, 0.0, Cmo, 1, t1, t2, l1, l2) - e_fci) <= 1e-9


@pytest.mark.parametrize("o,v,scale,rotated", CASES)
def test_formulas_are_the_derivative_and_the_response(o, v, scale, rotated):
    so, t1, t2, l1, l2 = _solved(o, v, scale, rotated)
    assert max(np.abs(l1 - t1).max(), np.abs(l2 - t2).max()) > 1e-5
    gam = LR.rdm1_explicit(t1, t2, l1, l2)
    err = np.abs(gam - LR.rdm1_by_derivative(so, t1, t2, l1, l2)).max()
    gam_corr = gam - np.diag([2.0] * o + [0.0] * v)
    V = np.random.default_rng(o + v).standard_normal((o + v, o + v))
    V = 0.5 * (V + V.T)
    e = [CR.solve(LR.with_fock(so, so.f_mo + s * 1e-4 * V), 1e-12, max_iter=2000)[0] for s in (1.0, -1.0)]
    fd, an = (e[0] - e[1]) / 2e-4, float(np.sum(V * gam_corr))
    d1, d2 = CR.random_amplitudes(np.random.default_rng(1), o, v, 1.0)
    st = LR.stationarity(so, t1, t2, l1, l2, d1, d2)
    print("(o, v) = (%d, %d): formulas against dL/df %.3e, |finite difference - tr V gamma_corr| = %.3e, trace %.3e, stationarity %.3e"
          % (o, v, err, abs(fd - an), np.trace(gam_corr), st))
    assert err <= 1e-12 and abs(fd - an) <= 1e-6 and abs(np.trace(gam_corr)) <= 1e-12 and abs(st) <= 1e-12
    assert abs(LR.stationarity(so, t1, t2, t1, t2, d1, d2)) > 1e-6


def test_lambda_plan_refuses_what_the_handle_plan_refuses():
    from libdmet_preview_amd._lib import lib
    from libdmet_preview_amd.solver import cc_lambda
    out = (C.c_int64 * 1)()
    assert lib.dmk_rccsd_lambda_plan(3, 4, 8, out) == 0 and int(out[0]) > 0 and int(out[0]) % 256 == 0
    small = int(out[0])
    assert cc_lambda.lambda_plan_bytes(3, 4, 8) == small and cc_lambda.lambda_plan_bytes(3, 4, 0) < small
    a = lambda count: (8 * max(int(count), 1) + 255) & ~255          # the formula of DESIGN.md K21 "Lambda"
    for o, v, diis in ((1, 1, 0), (3, 4, 8), (32, 33, 8)):
        nx = (o * v + 31) // 32 * 32 + o * o * v * v
        want = (2 + 2 * diis) * a(nx) + 5 * a(o * o * v * v) + a(o ** 4) + 2 * a(o ** 3 * v) + 10 * a(o * o) + 6 * a(v * v) + 6 * a(o * v)
        assert cc_lambda.lambda_plan_bytes(o, v, diis) == want, (o, v, diis)
    for o, v, diis in ((0, 3, 8), (3, 0, 8), (3, 3, 13), (-1, 3, 0), (513, 3, 0), (3, 513, 0), (3, 3, -1)):
        assert lib.dmk_rccsd_lambda_plan(o, v, diis, out) == DMK_ERR_INVALID
        with pytest.raises(ValueError):
            cc_lambda.lambda_plan_bytes(o, v, diis)
    assert lib.dmk_rccsd_lambda_plan(3, 3, 8, None) == DMK_ERR_INVALID


def test_modules_import_without_a_gpu_and_refuse_what_is_not_built():
    from libdmet_preview_amd.solver import cc, cc_lambda, cc_solver
    assert issubclass(cc_lambda.RCCSDLambda, cc.RCCSD) and cc.CCSD is cc.RCCSD
    with pytest.raises(NotImplementedError, match="DeviceHF"):
        cc_lambda.RCCSDLambda(object())
    with pytest.raises(NotImplementedError, match="frozen"):
        cc_lambda.RCCSDLambda(object(), frozen=1)
    obj = object.__new__(cc_lambda.RCCSDLambda)
    obj._h = obj._eris = None
    with pytest.raises(NotImplementedError, match="two-particle density"):
        obj.make_rdm2()
    with pytest.raises(NotImplementedError, match="unrestricted"):
        cc_solver.CCSolver()
    for key, val, name in (("ghf", True, "ghf"), ("bcs", True, "bcs"), ("linear", True, "linear"), ("tcc", True, "tcc"),
                           ("frozen", 2, "frozen"), ("use_mpi", True, "MPI"), ("nproc", 2, "MPI"), ("ring", True, "ring"), ("Sz", 2, "Sz")):
        with pytest.raises(NotImplementedError, match=name):
            cc_solver.CCSolver(restricted=True, **{key: val})
    s = cc_solver.CCSolver(restricted=True, approx_l=True)
    assert s.approx_l and s.restricted and s.make_rdm1() is None
    with pytest.raises(NotImplementedError, match="calc_rdm2"):
        s.run(None, nelec=2, calc_rdm2=True)
    for key in ("ccsdt", "bcc"):
        with pytest.raises(NotImplementedError, match=key):
            s.run(None, nelec=2, **{key: True})
    for key in ("save_dmet_ham", "use_calculated_twopdm", "ccsdt"):
        with pytest.raises(NotImplementedError, match=key):
            s.run_dmet_ham(None, **{key: True})
    with pytest.raises(NotImplementedError, match="two-particle density"):
        s.make_rdm2()


# ---- reverse mode -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(o, v, rotated):
    """(spin-orbital Hamiltonian, t1, t2, l1, l2): host orbitals, random symmetric amplitudes of scale 0.1; never modified."""
    sysm, C = CR.uneven_system(o, v)
    if rotated:
        C = CR.rotate_ov(C, o)
    rng = np.random.default_rng(11 * o + v)
    return (CR.spin_orbital(sysm, C, o),) + CR.random_amplitudes(rng, o, v) + CR.random_amplitudes(rng, o, v)


@pytest.mark.parametrize("o,v,rotated", JAC)
def test_reverse_sweep_is_the_jacobian_form(o, v, rotated):
    """d N = g + (J + diag d)^T Lam over the unique spin-orbital amplitudes: the relation tests/test_gpu_cclambda.py asserts of the
    device, here of lambda_step_reverse."""
    so, t1, t2, l1, l2 = _random(o, v, rotated)
    J, g = LR.jacobian(so, *CR.to_so(t1, t2))
    n1, n2 = LR.lambda_step_reverse(so, t1, t2, l1, l2)
    d1, d2 = CR._denoms(so)
    want = (g + (J + np.diag(LR._pack(d1, d2))).T @ LR._pack(*CR.to_so(l1, l2))) / LR._pack(d1, d2)
    W1, W2 = LR._unpack(want, 2 * o, 2 * v)
    w1, w2 = CR.from_so(W1, W2)
    err = max(np.abs(n1 - w1).max(), np.abs(n2 - w2).max())
    print("(o, v) = (%d, %d)%s: reverse sweep against the Jacobian form %.3e (max|l_new| = %.3f)"
          % (o, v, " rotated" if rotated else "", err, np.abs(w2).max()))
    assert n1.shape == (o, v) and n2.shape == (o, o, v, v) and err <= 1e-13
    assert np.abs(n2 - n2.transpose(1, 0, 3, 2)).max() <= 1e-14
    # the spin-orbital sweep keeps the spin adaptation: nothing is lost in from_so
    N1, N2 = CR.to_so(n1, n2)
    assert np.abs(LR._pack(N1, N2) - want).max() <= 1e-13
    # and its gradient is the one complex step gives along a direction
    L, G1, G2 = LR.grad_t_reverse(so, t1, t2, l1, l2)
    e1, e2 = CR.random_amplitudes(np.random.default_rng(3), o, v, 1.0)
    E1, E2 = CR.to_so(e1, e2)
    proj = float(np.sum(G1 * E1) + 0.25 * np.sum(G2 * E2))
    assert abs(L - float(LR.lagrangian(so, t1, t2, l1, l2))) <= 1e-13
    assert abs(proj - LR.stationarity(so, t1, t2, l1, l2, e1, e2)) <= 1e-13 * max(1.0, abs(proj))


@pytest.mark.parametrize("o,v,rotated", JAC)
def test_reverse_density_is_the_complex_step_density(o, v, rotated):
    so, t1, t2, l1, l2 = _random(o, v, rotated)
    gam = LR.rdm1_reverse(so, t1, t2, l1, l2)
    err = np.abs(gam - LR.rdm1_by_derivative(so, t1, t2, l1, l2)).max()
    print("(o, v) = (%d, %d)%s: reverse-mode density against complex step %.3e" % (o, v, " rotated" if rotated else "", err))
    assert gam.shape == (o + v, o + v) and np.array_equal(gam, gam.T) and err <= 1e-13


@pytest.mark.parametrize("o,v", [(8, 9), (3, 33)])
def test_reverse_density_is_the_formulas_where_complex_step_cannot_go(o, v):
    so, t1, t2, l1, l2 = _random(o, v, True)
    gam = LR.rdm1_reverse(so, t1, t2, l1, l2)
    err = np.abs(gam - LR.rdm1_explicit(t1, t2, l1, l2)).max()
    print("(o, v) = (%d, %d): reverse-mode density against the formulas %.3e, |trace - 2 o| = %.3e" % (o, v, err, abs(np.trace(gam) - 2 * o)))
    assert err <= 1e-12 and abs(np.trace(gam) - 2 * o) <= 1e-12


def test_reference_sweep_count_of_the_run_loop_system():
    """The GPU run-loop tests assert "more sweeps than slots" for rings up to 12: plain iteration must take more than 12 sweeps
    there, and not so many that a stalled loop would pass for a slow one."""
    o, v = RUN_SHAPE
    sysm, C = LR.coupled_system(o, v, RUN_SCALE)
    so = CR.spin_orbital(sysm, C, o)
    _, t1, t2, it_t = CR.r_solve(so, 1e-11)
    l1, l2 = t1, t2
    for sweeps in range(1, 201):
        n1, n2 = LR.lambda_step_reverse(so, t1, t2, l1, l2)
        dl = np.sqrt(np.sum((n1 - l1) ** 2) + np.sum((n2 - l2) ** 2))
        l1, l2 = n1, n2
        if dl < 1e-10:
            break
    r1, r2 = LR.solve_lambda_ref(so, t1, t2)
    err = max(np.abs(l1 - r1).max(), np.abs(l2 - r2).max())
    print("(2, 3), coupling 2.0: T in %d plain iterations, Lambda in %d sweeps (|dl| = %.3e), against the Jacobian solution %.3e, "
          "max|l - t| = %.3e" % (it_t, sweeps, dl, err, np.abs(l2 - t2).max()))
    assert dl < 1e-10 and 13 <= sweeps <= 100
    assert err <= 1e-8
    assert LR.lambda_run_ref(so, t1, t2, t1, t2, 0, 1e-10)[2] == sweeps          # the loop of the ring tests, without a ring
    # With DIIS the plain count says nothing about the ring: from l = t a ring of 12 is never full.  The ring tests therefore start
    # from run_loop_start, and "more sweeps than slots" must hold of the REFERENCE iteration there for every ring they use.
    short = LR.lambda_run_ref(so, t1, t2, t1, t2, 12, 1e-10)[2]
    start = LR.run_loop_start(o, v)
    counts = {}
    for ring in (2, 3, 12):
        a1, a2, counts[ring], _ = LR.lambda_run_ref(so, t1, t2, start[0], start[1], ring, 1e-10)
        assert max(np.abs(a1 - r1).max(), np.abs(a2 - r2).max()) <= 1e-8
    print("reference DIIS: ring of 12 from l = t %d sweeps;  from the random start, ring: sweeps = %s" % (short, counts))
    assert 0 < short <= 12
    assert all(ring < counts[ring] <= 100 for ring in counts)
