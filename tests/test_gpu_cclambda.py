"""
The Lambda equations, the one-particle density, the expectation value and the CCSD impurity solver on the device (DESIGN.md K21,
"Lambda"): solver/cc_lambda.py and solver/cc_solver.py against tests/cclambda_ref.py, which is built on the spin-orbital AMPLITUDE
equations of tests/ccsd_ref.py alone (derivatives by complex step), evaluated at the DEVICE's own orbitals and the device's own t.

Systems: R.System(o + v, 500 + 37 o + v, [o]) with the coupling `lam` multiplied by S[(o, v)] after construction, so that l differs
from t by 1e-4 .. 1e-3 (the stock coupling gives 1e-5).  T at tol_e = 1e-12, tol_normt = 1e-10, Lambda at 1e-10.
    (1, 4): 3   (2, 3): 2   (3, 4): 3   (the values at which the DIIS-free reference was seen to converge)
    (8, 9), (2, 17), (3, 33), (33, 3): 2   (the starting value for shapes nobody tried)

Bounds: amplitudes against the Jacobian reference 100 x the Lambda tolerance = 1e-8 (the last step norm bounds the error only up to
1 / (1 - rho)); one step and the explicit density 1e-10 (the project's one-step TOL); stationarity 1e-8, and > 1e-6 with l := t;
finite differences of step 1e-4 within 1e-6 (the O(eps^2) term); expval 1e-9, two electrons against FCI 1e-8.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import cclambda_ref as LR
from tests import scf_ref as R
from tests.test_gpu_mp2 import _dev_block
from tests.test_host_ccsd import TWO_ELECTRON

pytestmark = pytest.mark.gpu

S = {(1, 4): 3.0, (2, 3): 2.0, (3, 4): 3.0, (8, 9): 2.0, (2, 17): 2.0, (3, 33): 2.0, (33, 3): 2.0}
JAC = [(1, 4, False), (2, 3, True), (3, 4, False)]
BIG = [(8, 9), (2, 17), (3, 33), (33, 3)]
TOL = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _scf(sysm, o):
    from libdmet_preview_amd import _lib
    from libdmet_preview_amd.solver import scf
    ctx = _lib.get_ctx()
    s = scf.SCF(newton_ah=False)
    s.set_system(2 * o, 0, False, True)
    s.set_integral_dev(sysm.n, 0.0, ctx.to_device(sysm.h1[None]), None, [_dev_block(ctx, sysm, "aa")])
    s.HF(tol=1e-12, MaxIter=100, conv_tol_grad=1e-10)
    assert s.mf.converged
    return s


def _solved(s, C=None):
    from libdmet_preview_amd.solver import cc_lambda
    obj = cc_lambda.RCCSDLambda(s.mf, mo_coeff=C)
    obj.conv_tol, obj.conv_tol_normt = 1e-12, 1e-10
    obj.kernel()
    assert obj.converged
    obj.solve_lambda()
    assert obj.converged_lambda and obj.cycles_lambda > 1
    return obj


@functools.lru_cache(maxsize=None)
def _case(o, v, rotated=False, seed=None, scale=None):
    """(solver, system, orbitals [occ | vir], spin-orbital Hamiltonian there, solved RCCSDLambda): shared, never modified."""
    sysm = R.System(o + v, 500 + 37 * o + v if seed is None else seed, [o])
    sysm.lam *= S[(o, v)] if scale is None else scale
    s = _scf(sysm, o)
    C = np.asarray(s.mf.mo_coeff)
    if rotated:
        C = CR.rotate_ov(C, o)
    obj = _solved(s, C if rotated else None)
    return s, sysm, C, CR.spin_orbital(sysm, C, o), obj


@functools.lru_cache(maxsize=None)
def _jacobian(o, v, rotated):
    """The reference Lambda at the device's t: (l1, l2, J, g)."""
    so, obj = _case(o, v, rotated)[3:]
    return LR.lambda_by_jacobian(so, *CR.to_so(obj.t1, obj.t2), full=True)[:4]


@pytest.mark.parametrize("o,v,rotated", JAC)
def test_lambda_and_density_against_the_jacobian_reference(ctx, o, v, rotated):
    s, sysm, Cmo, so, obj = _case(o, v, rotated)
    if rotated:
        assert np.abs(so.fov).max() > 1e-3
    l1, l2 = _jacobian(o, v, rotated)[:2]
    err = max(np.abs(obj.l1 - l1).max(), np.abs(obj.l2 - l2).max())
    far = max(np.abs(obj.l1 - obj.t1).max(), np.abs(obj.l2 - obj.t2).max())
    gam = obj.make_rdm1()
    e_form = np.abs(gam - LR.rdm1_explicit(obj.t1, obj.t2, obj.l1, obj.l2)).max()
    e_der = np.abs(gam - LR.rdm1_by_derivative(so, obj.t1, obj.t2, l1, l2)).max()
    print("(o, v) = (%d, %d)%s: %d Lambda iterations, max|l - l_ref| = %.3e, max|l - t| = %.3e, density: formulas %.3e, derivative %.3e"
          % (o, v, " rotated" if rotated else "", obj.cycles_lambda, err, far, e_form, e_der))
    assert err <= 1e-8 and far > 1e-5
    assert np.abs(obj.l2 - obj.l2.transpose(1, 0, 3, 2)).max() <= 1e-12
    assert e_form <= TOL and e_der <= 1e-8
    assert np.array_equal(gam, gam.T) and abs(np.trace(gam) - 2 * o) <= TOL
    ao = obj.make_rdm1(ao_repr=True)
    assert np.abs(ao - Cmo @ gam @ Cmo.T).max() <= 1e-13


@pytest.mark.parametrize("o,v,rotated", JAC)
def test_one_update_lambda_step(ctx, o, v, rotated):
    """d l~_new - g = J^T l~ from random symmetric l of scale 0.1 (J over the unique spin-orbital amplitudes: the restricted l~ maps to
    spin orbitals as amplitudes do, through to_so of l)."""
    from libdmet_preview_amd.solver import cc_lambda
    s, sysm, Cmo, so, solved = _case(o, v, rotated)
    J = _jacobian(o, v, rotated)[2]
    l1, l2 = CR.random_amplitudes(np.random.default_rng(7 + o + v), o, v)
    obj = cc_lambda.RCCSDLambda(s.mf, mo_coeff=Cmo if rotated else None)
    try:
        n1, n2 = obj.update_lambda(l1, l2, solved.t1, solved.t2)
        m1, m2 = obj.update_lambda(l1, l2)
    finally:
        obj.close()
    assert np.array_equal(n1, m1) and np.array_equal(n2, m2)
    # in spin orbitals: d Lam_new + g = -(J + d)^T Lam, i.e. d (Lam_new) = -g - J^T Lam - d Lam  with J = dr/dx = dR_od/dx - d
    L1, L2 = CR.to_so(l1, l2)
    N1, N2 = CR.to_so(n1, n2)
    g = _jacobian(o, v, rotated)[3]
    d1 = so.eo[:, None] - so.ev[None, :]
    d2 = d1[:, None, :, None] + d1[None, :, None, :]
    lhs = LR._pack(d1 * N1, d2 * N2) - g
    rhs = (J + np.diag(LR._pack(d1, d2))).T @ LR._pack(L1, L2)
    err = np.abs(lhs - rhs).max()
    print("(o, v) = (%d, %d): one Lambda step, max|d l_new - g - Jod^T l| = %.3e (max|l_new| = %.3f)" % (o, v, err, np.abs(n2).max()))
    assert err <= TOL


@pytest.mark.parametrize("o,v", BIG)
def test_stationarity_and_density_where_the_jacobian_is_too_big(ctx, o, v):
    s, sysm, Cmo, so, obj = _case(o, v)
    rng = np.random.default_rng(3 * o + v)
    worst, vac = 0.0, 0.0
    for _ in range(2 if o + v < 30 else 1):          # the complex spin-orbital update at V = 66 takes seconds: one direction there
        d1, d2 = CR.random_amplitudes(rng, o, v, 1.0)
        nrm = np.sqrt(np.sum(d1 ** 2) + np.sum(d2 ** 2))
        d1, d2 = d1 / nrm, d2 / nrm
        worst = max(worst, abs(LR.stationarity(so, obj.t1, obj.t2, obj.l1, obj.l2, d1, d2)))
        vac = max(vac, abs(LR.stationarity(so, obj.t1, obj.t2, obj.t1, obj.t2, d1, d2)))
    gam = obj.make_rdm1()
    e_form = np.abs(gam - LR.rdm1_explicit(obj.t1, obj.t2, obj.l1, obj.l2)).max()
    print("(o, v) = (%d, %d): |dL/dt . delta| = %.3e (with l := t: %.3e), %d Lambda iterations, density against the formulas %.3e"
          % (o, v, worst, vac, obj.cycles_lambda, e_form))
    assert worst <= 1e-8 and vac > 1e-6
    assert e_form <= TOL and np.array_equal(gam, gam.T) and abs(np.trace(gam) - 2 * o) <= TOL


@pytest.mark.parametrize("n,seed", TWO_ELECTRON)
def test_two_electrons_density_and_expval_are_exact(ctx, n, seed):
    s, sysm, Cmo, so, obj = _case(1, n - 1, False, seed, 1.0)
    e_fci, X = LR.fci_two_electron(sysm)
    ao = obj.make_rdm1(ao_repr=True)
    other = R.System(n, seed + 100, [1])
    other.lam *= 0.5
    e2 = obj.expval(0.25, other.h1, other.block_s4("aa"))
    ref2 = 0.25 + float(X.reshape(-1) @ LR.two_electron_matrix(other) @ X.reshape(-1))
    print("n = %d: max|gamma_AO - 2 X X^T| = %.3e, |<H'> - X^T H' X| = %.3e" % (n, np.abs(ao - 2.0 * X @ X.T).max(), abs(e2 - ref2)))
    assert np.abs(ao - 2.0 * X @ X.T).max() <= 1e-8 and abs(e2 - ref2) <= 1e-8
    assert abs(s.mf.e_tot + obj.e_corr - e_fci) <= 1e-9


def test_density_is_the_derivative_of_the_device_energy(ctx):
    """Central difference of the DEVICE e_corr under f +- 1e-4 V (handles of dmk_rccsd_create over the same blocks) = tr V gamma_corr."""
    from tests.test_gpu_ccsd_shapes import Handle
    o, v = 2, 3
    s, sysm, Cmo, so, obj = _case(o, v, True)
    fock, blocks = CR.restricted_blocks(sysm, Cmo, o)
    rng = np.random.default_rng(4)
    V = rng.standard_normal((o + v, o + v))
    V = 0.5 * (V + V.T)
    e = {}
    for sign in (1.0, -1.0):
        h = Handle(ctx, o, v, fock + sign * 1e-4 * V, blocks, diis=8)
        try:
            res = h.run(100)
            assert res[1] == 1.0
            e[sign] = res[0]
        finally:
            h.close()
    gam = obj.make_rdm1()
    gam_corr = gam - np.diag([2.0] * o + [0.0] * v)
    fd, an = (e[1.0] - e[-1.0]) / 2e-4, float(np.sum(V * gam_corr))
    print("d e_corr / d f . V: finite difference %.10f, tr V gamma_corr %.10f, difference %.3e" % (fd, an, abs(fd - an)))
    assert abs(fd - an) <= 1e-6 and abs(np.trace(gam_corr)) <= TOL


def test_expval(ctx):
    o, v = 3, 4
    s, sysm, Cmo, so, obj = _case(o, v, False)
    n = o + v
    blk = sysm.block_s4("aa")
    e_same = obj.expval(0.0, sysm.h1, blk)
    other = R.System(n, 900, [o])
    other.lam *= 0.5
    e_other = obj.expval(0.5, other.h1, R.restore_s1(other.block_s4("aa"), n))          # the 1-fold format
    ref = LR.expval_ref(other, 0.5, Cmo, o, obj.t1, obj.t2, obj.l1, obj.l2)
    rng = np.random.default_rng(9)
    V = rng.standard_normal((n, n))
    V = 0.5 * (V + V.T)
    lin = obj.expval(0.0, sysm.h1 + V, blk) - e_same
    tr = float(np.sum(V * obj.make_rdm1(ao_repr=True)))
    print("expval: |<H> - (E_HF + E_corr)| = %.3e, other system %.3e, linearity %.3e"
          % (abs(e_same - s.mf.e_tot - obj.e_corr), abs(e_other - ref), abs(lin - tr)))
    assert abs(e_same - (s.mf.e_tot + obj.e_corr)) <= 1e-9
    assert abs(e_other - ref) <= 1e-9 and abs(lin - tr) <= 1e-9
    ctx.sync()
    before = ctx.mem_info()[0]
    obj.expval(0.0, sysm.h1, blk)
    ctx.sync()
    assert ctx.mem_info()[0] == before                    # the probe and its blocks were released


def test_solver_runs_the_reference_shape(ctx):
    from libdmet_preview_amd.solver import cc_solver
    from libdmet_preview_amd.system import integral
    o, v = 3, 4
    s, sysm, Cmo, so, ref = _case(o, v, False)
    n = o + v
    Ham = integral.Integral(n, True, False, 0.125, {"cd": sysm.h1[None].copy()}, {"ccdd": sysm.blocks_s4()[:1].copy()})
    solver = cc_solver.CCSolver(restricted=True, tol=1e-12, tol_normt=1e-10)
    onepdm, E = solver.run(Ham, nelec=2 * o)
    obj = solver.cisolver
    assert onepdm.shape == (1, n, n) and np.abs(2.0 * onepdm[0] - obj.make_rdm1(ao_repr=True)).max() <= 1e-13
    assert abs(E - (solver.mf.e_tot + obj.e_corr)) <= 1e-13 and abs(E - 0.125 - (s.mf.e_tot + ref.e_corr)) <= 1e-9
    assert np.abs(2.0 * onepdm[0] - ref.make_rdm1(ao_repr=True)).max() <= 1e-8 and solver.onepdm_mo.shape == (1, n, n)
    assert abs(solver.run_dmet_ham(Ham) - E) <= 1e-9
    first = (obj.l1.copy(), obj.l2.copy())
    obj.l1 = obj.l2 = None
    again = obj.solve_lambda()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])          # no atomics, fixed order
    # a restart has nothing left to do; approx_l returns the density of l = t
    onepdm2, E2 = solver.run(Ham, nelec=2 * o, restart=True)
    assert solver.cisolver.cycles <= 2 and solver.cisolver.cycles_lambda <= 2 and abs(E2 - E) <= 1e-10
    approx = cc_solver.CCSolver(restricted=True, tol=1e-12, tol_normt=1e-10, approx_l=True)
    pdm, _ = approx.run(Ham, nelec=2 * o, dm0=onepdm * 2.0)
    a = approx.cisolver
    assert np.array_equal(a.l1, a.t1) and np.array_equal(a.l2, a.t2)
    assert np.abs(a.make_rdm1() - LR.rdm1_explicit(a.t1, a.t2, a.t1, a.t2)).max() <= TOL
    assert np.abs(pdm - onepdm).max() > 1e-7
    for x in (solver.cisolver, a):
        x.close()


def test_lambda_allocation_is_what_the_planner_says(ctx):
    """o = v = 24, ring of 8: the plan is about 60 MB, far above any block the driver could hand out of memory it already holds; the
    drop of the free memory at the first Lambda call is the plan rounded up to the driver's granularity (at most 2 MiB)."""
    from libdmet_preview_amd._lib import lib, c_vp
    from libdmet_preview_amd.solver import cc_lambda
    from tests.test_gpu_ccsd_shapes import DMK_ERR_STATE
    o = v = 24
    plan = cc_lambda.lambda_plan_bytes(o, v, 8)
    npair = v * (v + 1) // 2
    rng = np.random.default_rng(0)
    sizes = [(o + v) ** 2, o ** 4, o ** 3 * v, o * o * v * v, o * o * v * v, o * o * v * v, o * v ** 3, npair * npair]
    dev = [ctx.to_device(0.01 * rng.standard_normal(k)) for k in sizes]
    h = c_vp()
    ctx.check(lib.dmk_rccsd_create(ctx.h, o, v, *([d.ptr for d in dev] + [npair, 8, C.byref(h)])))
    try:
        assert lib.dmk_rccsd_lambda_init(h) == DMK_ERR_STATE and lib.dmk_rccsd_lambda_update(h) == DMK_ERR_STATE
        ctx.sync()
        before = ctx.mem_info()[0]
        ctx.check(lib.dmk_rccsd_lambda_set(h, dev[3].ptr, dev[3].ptr))
        ctx.sync()
        used = before - ctx.mem_info()[0]
        print("Lambda state at o = v = 24, ring 8: plan %d bytes, the free memory dropped by %d" % (plan, used))
        assert plan <= used < plan + (2 << 20)
    finally:
        ctx.check(lib.dmk_rccsd_free(h))
