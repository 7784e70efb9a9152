"""
Host-side tests of the perturbative triples: the two references of tests/ccsd_t_ref.py against each other, the cases
in which (T) vanishes identically, the plan formula and the refusals of the C ABI, the import of solver.ccsd_t without a GPU, and the
normalisation of the references against exact diagonalisation.

Normalisation   CCSD is exact through third order of perturbation theory and (T) carries the whole fourth-order triples term, so with
                the two-body part scaled by lam,  rho(lam) = |E_FCI - E_CCSD - E_(T)| / |E_FCI - E_CCSD|  is O(lam): a (T) with a wrong
                prefactor (1/3 or 3 times, a missing multiplicity) leaves rho of order one at every lam.
Measured        the references agree within 7.6e-16 relative (bound 1e-12); at (1, 4) and (4, 1) the closed-shell form gives
                |E| <= 5.3e-19 (S = 0.04 ... 0.08); rho(1) = 0.0946, rho(1/2) = 0.0479 (and 0.0242 at 1/4: it halves with lam) on the 4-electron,
                n = 6 system of seed NORM_SEED; seeds 1, 2, 3 give 0.039 / 0.020, 0.130 / 0.064, 0.161 / 0.081
                (profiles/ccsd_t_notes.txt).  The streamed closed-shell form (the reference of tests/test_gpu_ccsd_t_shapes.py)
                agrees with the closed-shell form within 3.6e-16 relative in E and bit for bit in S (bound 1e-13) at (2, 2), (3, 4),
                (4, 3), (5, 17), canonical and rotated, and gives |E| <= 4.5e-19 at (1, 4) and (4, 1).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import ccsd_t_ref as TR
from tests import scf_ref as R

DMK_OK, DMK_ERR_INVALID = 0, -1
EPS = np.finfo(np.float64).eps
NORM_SEED = 2207


def _case(o, v, rotated, seed=0):
    sysm, Cm = CR.uneven_system(o, v)
    if rotated:
        Cm = CR.rotate_ov(Cm, o)
    t1, t2 = CR.random_amplitudes(np.random.default_rng(100 * o + v + seed), o, v)
    return sysm, Cm, t1, t2


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("o,v", [(2, 2), (3, 4), (4, 3)])
def test_the_two_references_agree(o, v, rotated):
    sysm, Cm, t1, t2 = _case(o, v, rotated)
    so = CR.spin_orbital(sysm, Cm, o)
    f, blocks = CR.restricted_blocks(sysm, Cm, o)
    ea = TR.t_spin_orbital(so, t1, t2)
    eb, s = TR.t_closed_shell(f, blocks, t1, t2)
    el, sl = TR.t_closed_shell(f, blocks, t1, t2, np.longdouble)
    print("(o, v) = (%d, %d)%s: spin-orbital %.15e, closed-shell %.15e, relative difference %.2e; longdouble against float64 %.2e; S = %.3e"
          % (o, v, " rotated" if rotated else "", ea, eb, abs(ea - eb) / abs(ea), abs(el - eb) / abs(ea), s))
    assert ea != 0.0 and abs(ea - eb) <= 1e-12 * abs(ea)
    assert abs(el - eb) <= 1e-12 * abs(ea) and abs(sl - s) <= 1e-12 * s and s >= abs(eb)
    if rotated:
        assert np.abs(f[:o, o:]).max() > 1e-3          # the f_ov term is exercised


@pytest.mark.parametrize("o,v", [(1, 4), (4, 1)])
def test_triples_vanish_with_one_occupied_or_one_virtual(o, v):
    """Three electrons (or three holes) in distinct spin orbitals do not exist there."""
    for rotated in (False, True):
        sysm, Cm, t1, t2 = _case(o, v, rotated)
        f, blocks = CR.restricted_blocks(sysm, Cm, o)
        e, s = TR.t_closed_shell(f, blocks, t1, t2)
        print("(o, v) = (%d, %d)%s: E_(T) = %.3e, S = %.3e, |E| / (64 eps S) = %.3f" % (o, v, " rotated" if rotated else "", e, s, abs(e) / (64 * EPS * s)))
        assert s > 0.0 and abs(e) <= 64 * EPS * s


STREAMED = [(2, 2, np.float64), (3, 4, np.float64), (4, 3, np.float64), (5, 17, np.float64),
            (2, 2, np.longdouble), (3, 4, np.longdouble), (4, 3, np.longdouble)]


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("o,v,dtype", STREAMED, ids=lambda x: x.__name__ if isinstance(x, type) else str(x))
def test_the_streamed_form_is_the_closed_shell_form(o, v, dtype, rotated):
    """t_closed_shell_streamed (matrix products, O(o^3) memory: the reference of tests/test_gpu_ccsd_t_shapes.py) against
    t_closed_shell, E relative to |E| and S relative to S.  The two differ in the order of the K sums only (einsum against a matrix
    product), which is a few eps of S spread over the elements; |E| / S is 3e-4 .. 9e-3 here.  With the c of a pair in chunks of two
    (the path the large shapes take) the numbers are the same within the same bound, and they do not depend on the thread count."""
    sysm, Cm, t1, t2 = _case(o, v, rotated)
    f, blocks = CR.restricted_blocks(sysm, Cm, o)
    e, s = TR.t_closed_shell(f, blocks, t1, t2, dtype)
    es, ss = TR.t_closed_shell_streamed(f, blocks, t1, t2, dtype)
    print("(o, v) = (%d, %d)%s %s: closed-shell %.16e, streamed %.16e, relative difference %.2e; S %.2e"
          % (o, v, " rotated" if rotated else "", dtype.__name__, e, es, abs(e - es) / abs(e), abs(s - ss) / s))
    assert e != 0.0 and abs(es - e) <= 1e-13 * abs(e) and abs(ss - s) <= 1e-13 * s
    assert TR.t_closed_shell_streamed(f, blocks, t1, t2, dtype, threads=1) == (es, ss)
    ec, sc = TR.t_closed_shell_streamed(f, blocks, t1, t2, dtype, chunk_elements=2 * o ** 3)
    assert abs(ec - e) <= 1e-13 * abs(e) and abs(sc - s) <= 1e-13 * s


@pytest.mark.parametrize("o,v", [(1, 4), (4, 1)])
def test_the_streamed_form_vanishes_with_one_occupied_or_one_virtual(o, v):
    for rotated in (False, True):
        sysm, Cm, t1, t2 = _case(o, v, rotated)
        f, blocks = CR.restricted_blocks(sysm, Cm, o)
        e, s = TR.t_closed_shell_streamed(f, blocks, t1, t2)
        print("(o, v) = (%d, %d)%s: streamed E_(T) = %.3e, S = %.3e, |E| / (64 eps S) = %.3f" % (o, v, " rotated" if rotated else "", e, s, abs(e) / (64 * EPS * s)))
        assert s > 0.0 and abs(e) <= 64 * EPS * s


def k22_bytes(o, v):
    """DESIGN.md K22, "Plan": the permuted t2, one double per unique triple, 1024 partial sums and the result record; one W."""
    a256 = lambda x: (x + 255) // 256 * 256
    return a256(8 * o * o * v * v) + a256(8 * (v * (v + 1) * (v + 2) // 6)) + a256(8 * 1024) + 256, a256(8 * o ** 3)


def test_plan_formula_and_refusals():
    from libdmet_preview_amd._lib import lib, c_i64
    from libdmet_preview_amd.solver import ccsd_t
    out = (c_i64 * 2)()
    for o, v in ((1, 1), (1, 3), (3, 1), (5, 17), (17, 5), (64, 192), (512, 512)):
        assert lib.dmk_rccsd_t_plan(o, v, out) == DMK_OK
        assert (int(out[0]), int(out[1])) == k22_bytes(o, v), (o, v)
        assert ccsd_t.plan_bytes(o, v) == k22_bytes(o, v)
    for o, v in ((0, 3), (3, 0), (-1, 3), (513, 3), (3, 513)):
        assert lib.dmk_rccsd_t_plan(o, v, out) == DMK_ERR_INVALID
        with pytest.raises(ValueError):
            ccsd_t.plan_bytes(o, v)
    assert lib.dmk_rccsd_t_plan(3, 3, None) == DMK_ERR_INVALID
    assert lib.dmk_rccsd_t(None, 0, (C.c_double * 2)()) == DMK_ERR_INVALID


def test_modules_import_without_a_gpu_and_the_front_doors():
    from libdmet_preview_amd.solver import cc, cc_lambda, cc_solver, ccsd_t
    assert callable(ccsd_t.kernel) and callable(cc_lambda.RCCSDLambda.ccsd_t)
    s = cc_solver.CCSolver(restricted=True)
    with pytest.raises(RuntimeError, match="run"):
        s.ccsd_t()
    # the (T) energy is built; the ccsdt=True path of the runs (Lambda and densities of (T)) is not, and says so
    with pytest.raises(NotImplementedError, match="densities"):
        s.run(None, nelec=2, ccsdt=True)
    with pytest.raises(NotImplementedError, match="densities"):
        cc.run_ccsd(None, ccsdt=True)
    obj = object.__new__(cc_lambda.RCCSDLambda)
    obj._h = obj._eris = None
    obj.t1 = obj.t2 = None
    with pytest.raises(RuntimeError, match="amplitudes"):
        ccsd_t.kernel(obj)
    with pytest.raises(ValueError):
        ccsd_t.kernel(obj, t1=np.zeros((1, 1)))
    # the memory check comes before any allocation and needs no device when max_memory is given
    obj._nocc, obj.max_memory = (64,), None
    obj._scf = type("S", (), {"_n": 256})()
    obj.t1 = obj.t2 = 0
    with pytest.raises(MemoryError, match="per triple in flight"):
        ccsd_t.kernel(obj, max_memory=1.0)


def _rho(scale):
    """(rho, E_FCI - E_HF, E_CCSD - E_HF, E_(T)) of the n = 6, 4-electron system with the two-body part scaled."""
    n, o = 6, 2
    sysm = R.System(n, NORM_SEED, [o])
    sysm.lam *= scale
    ref = R.scf(sysm.h1[None], sysm.veff_rhf, [o], True)
    assert ref["converged"]
    Cm = ref["mo_coeff"]
    Cm = Cm[0] if np.ndim(Cm) == 3 else Cm
    so = CR.spin_orbital(sysm, Cm, o)
    e_cc, T1, T2, _ = CR.solve(so, 1e-12)
    t1, t2 = CR.from_so(T1, T2)
    f, blocks = CR.restricted_blocks(sysm, Cm, o)
    e_t = TR.t_closed_shell(f, blocks, t1, t2)[0]
    assert abs(e_t - TR.t_spin_orbital(so, t1, t2)) <= 1e-12 * abs(e_t)
    h1, g = TR.mo_integrals(sysm, Cm)
    D = 2.0 * Cm[:, :o] @ Cm[:, :o].T
    e_hf = float(np.sum(D * (sysm.h1 + 0.5 * sysm.veff_rhf(D))))
    e_fci = TR.fci_energy(h1, g, o)
    return abs(e_fci - e_hf - e_cc - e_t) / abs(e_fci - e_hf - e_cc), e_fci - e_hf, e_cc, e_t


def test_normalisation_against_exact_diagonalisation():
    rho1, c1, cc1, t1 = _rho(1.0)
    rho2, c2, cc2, t2 = _rho(0.5)
    print("lam = 1  : E_FCI - E_HF = %.10f, E_CCSD = %.10f, E_(T) = %.3e, rho = %.4f" % (c1, cc1, t1, rho1))
    print("lam = 1/2: E_FCI - E_HF = %.10f, E_CCSD = %.10f, E_(T) = %.3e, rho = %.4f" % (c2, cc2, t2, rho2))
    assert c1 < cc1 < 0.0 and t1 < 0.0 and t2 < 0.0
    assert rho2 < rho1 and rho2 < 0.5
