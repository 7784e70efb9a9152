"""
MP2 on the device over the device Hartree-Fock solver: correlation energy, amplitudes and the unrelaxed density of
solver/mp.py (MP2, UIMP2, run_mp2) against the literal einsums of tests/mp2_ref.py evaluated at the DEVICE's own mo_coeff / mo_energy
-- so the comparison measures the transform and the MP2 kernels, not the SCF tolerance (that the orbitals are the Hartree-Fock
solution is the business of tests/test_gpu_scf.py).

Tolerance: 1e-10 max-abs (the TOL of tests/test_gpu_scf.py); amplitudes and density entries are O(0.1) and |e_corr| < 1 on these
systems.
"""
import functools

import numpy as np
import pytest

from tests import mp2_ref as M
from tests import scf_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCF_TOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _dev_block(ctx, sysm, which):
    from libdmet_preview_amd._lib import lib
    npair = sysm.n * (sysm.n + 1) // 2
    L = {"a": R.tril_pack(sysm.A), "b": R.tril_pack(sysm.B)}
    d_x, d_y = ctx.to_device(L[which[0]]), ctx.to_device(L[which[1]])
    d_E = ctx.zeros((npair, npair), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npair, npair, R.NAUX, sysm.lam, d_x.ptr, npair, d_y.ptr, npair, d_E.ptr, npair))
    return d_E


def _solver(ctx, kind, n, Sz, sysm, nblk=None):
    from libdmet_preview_amd.solver import scf
    s = scf.SCF(newton_ah=False)
    s.set_system(R.nelec_of(n), Sz, False, kind == "rhf")
    nblk = nblk or (1 if kind == "rhf" else 3)
    s.set_integral_dev(n, 0.0, ctx.to_device(sysm.h1[None]), None, [_dev_block(ctx, sysm, w) for w in ("aa", "bb", "ab")[:nblk]])
    return s


@functools.lru_cache(maxsize=None)
def _converged(kind, n, Sz):
    """One converged device Hartree-Fock per listed case, shared by the tests (never modified)."""
    from libdmet_preview_amd import _lib
    sysm = R.make_system(kind, n, Sz)
    s = _solver(_lib.get_ctx(), kind, n, Sz, sysm)
    s.HF(tol=SCF_TOL, MaxIter=50)
    assert s.mf.converged
    return s, sysm


def _reference(kind, n, Sz, sysm, mo_coeff, mo_energy):
    nocc = R.nocc_of(kind, n, Sz)
    if kind == "rhf":
        return M.rmp2(sysm, np.asarray(mo_coeff), np.asarray(mo_energy), nocc[0])
    return M.ump2(sysm, np.asarray(mo_coeff), np.asarray(mo_energy), nocc)


CASES = [("rhf", 6, 0), ("rhf", 65, 0), ("uhf", 6, 0), ("uhf", 6, 2), ("uhf", 65, 0), ("uhf", 65, 2)]


@pytest.mark.parametrize("kind,n,Sz", CASES)
def test_mp2_against_the_einsums_at_the_device_orbitals(ctx, kind, n, Sz):
    from libdmet_preview_amd.solver import mp
    s, sysm = _converged(kind, n, Sz)
    mf = s.mf
    ref = _reference(kind, n, Sz, sysm, mf.mo_coeff, mf.mo_energy)
    obj = (mp.MP2 if kind == "rhf" else mp.UIMP2)(mf)
    e_corr, t2 = obj.kernel(with_t2=(n == 6))
    d_mo, d_ao = obj.make_rdm1(), obj.make_rdm1(ao_repr=True)
    errs = (abs(e_corr - ref["e_corr"]), np.abs(d_mo - ref["rdm1_mo"]).max(), np.abs(d_ao - ref["rdm1_ao"]).max())
    print("%s n=%d Sz=%d: e_corr = %.12f  |de| = %.3e  max|d rdm1_mo| = %.3e  max|d rdm1_ao| = %.3e" % ((kind, n, Sz, e_corr) + errs))
    assert max(errs) <= TOL
    assert obj.e_corr == e_corr and obj.e_tot == mf.e_tot + e_corr and e_corr < 0.0
    nocc = R.nocc_of(kind, n, Sz)
    if kind == "rhf":
        assert obj.nocc == nocc[0] and obj.nmo == n and d_mo.shape == (n, n)
        assert abs(np.trace(d_mo) - 2 * nocc[0]) <= TOL and abs(np.trace(d_ao) - 2 * nocc[0]) <= TOL
    else:
        assert obj.nocc == tuple(nocc) and obj.nmo == (n, n) and d_mo.shape == (2, n, n)
        assert max(abs(np.trace(d_mo[k]) - nocc[k]) for k in range(2)) <= TOL
    if n == 6:
        if kind == "rhf":
            assert t2.shape == ref["t2"].shape and np.abs(t2 - ref["t2"]).max() <= TOL
        else:
            assert len(t2) == 3 and all(a.shape == b.shape and np.abs(a - b).max() <= TOL for a, b in zip(t2, ref["t2"]))
    else:
        assert t2 is None and obj.t2 is None
    e2, _ = obj.kernel(with_t2=False)                                        # the same call twice: the same bits
    assert e2 == e_corr and np.array_equal(obj.make_rdm1(), d_mo)
    eris = obj.ao2mo()                                                       # device arrays, rows (i, a), columns (j, b)
    o, v = nocc[0], n - nocc[0]
    assert eris.ovov.shape == (o * v, o * v) and (kind == "rhf" or eris.ovOV.shape == (o * v, nocc[1] * (n - nocc[1])))


@pytest.mark.parametrize("kind,n,Sz", [("rhf", 6, 0), ("rhf", 65, 0), ("uhf", 6, 2)])
def test_run_mp2_follows_the_reference_conventions(ctx, kind, n, Sz):
    from libdmet_preview_amd.solver import mp
    s, sysm = _converged(kind, n, Sz)
    ref = _reference(kind, n, Sz, sysm, s.mf.mo_coeff, s.mf.mo_energy)
    E, rdm1 = mp.run_mp2(s)
    assert abs(E - ref["e_corr"]) <= TOL and E == s.mp.e_corr                # the CORRELATION energy
    if kind == "rhf":
        assert rdm1.shape == (1, n, n) and np.abs(rdm1[0] - 0.5 * ref["rdm1_ao"]).max() <= TOL and isinstance(s.mp, mp.MP2)
    else:
        assert rdm1.shape == (2, n, n) and np.abs(rdm1 - ref["rdm1_ao"]).max() <= TOL and isinstance(s.mp, mp.UIMP2)


def test_uimp2_on_a_closed_shell_equals_mp2(ctx):
    """Equal spin blocks, the restricted orbitals handed to UIMP2 explicitly: energy, density and amplitudes of MP2."""
    from libdmet_preview_amd.solver import mp
    n = 6
    s, sysm = _converged("rhf", n, 0)
    r = mp.MP2(s.mf)
    e_r, t_r = r.kernel()
    su = _solver(ctx, "uhf", n, 0, sysm, nblk=1)                             # one block serves aa, bb and ab
    su.HF(tol=SCF_TOL)
    c, e, occ = s.mf.mo_coeff, s.mf.mo_energy, s.mf.mo_occ
    u = mp.UIMP2(su.mf, mo_coeff=np.asarray([c, c]), mo_occ=np.asarray([occ, occ]) * 0.5)
    e_u, t_u = u.kernel(mo_energy=np.asarray([e, e]), mo_coeff=np.asarray([c, c]))
    assert abs(e_u - e_r) <= TOL
    assert np.abs(u.make_rdm1().sum(axis=0) - r.make_rdm1()).max() <= TOL
    assert np.abs(t_u[1] - t_r).max() <= TOL and np.abs(t_u[0] - (t_r - t_r.transpose(0, 1, 3, 2))).max() <= TOL


def test_explicit_orbitals_and_energies_are_honoured(ctx):
    from libdmet_preview_amd.solver import mp
    kind, n, Sz = "rhf", 6, 0
    s, sysm = _converged(kind, n, Sz)
    mf = s.mf
    o = R.nocc_of(kind, n, Sz)[0]
    e_shift = np.array(mf.mo_energy)
    e_shift[o:] += 0.25
    want = M.rmp2(sysm, mf.mo_coeff, e_shift, o)
    obj = mp.MP2(mf)
    e_corr, t2 = obj.kernel(mo_energy=e_shift)
    assert abs(e_corr - want["e_corr"]) <= TOL and np.abs(t2 - want["t2"]).max() <= TOL
    assert abs(e_corr - _reference(kind, n, Sz, sysm, mf.mo_coeff, mf.mo_energy)["e_corr"]) > 1e-6
    # other orbitals (a rotation inside the occupied and inside the virtual space, listed in a shuffled order with their mo_occ)
    rng = np.random.default_rng(5)
    qo, _ = np.linalg.qr(rng.standard_normal((o, o)))
    qv, _ = np.linalg.qr(rng.standard_normal((n - o, n - o)))
    c_rot = np.hstack([mf.mo_coeff[:, :o] @ qo, mf.mo_coeff[:, o:] @ qv])
    e_rot = np.concatenate([np.linspace(-1.0, -0.5, o), np.linspace(0.5, 1.0, n - o)])
    want = M.rmp2(sysm, c_rot, e_rot, o)
    perm = rng.permutation(n)
    obj = mp.MP2(mf, mo_coeff=c_rot[:, perm], mo_occ=np.asarray(mf.mo_occ)[perm])
    e_corr, _ = obj.kernel(mo_energy=e_rot[perm], mo_coeff=c_rot[:, perm], with_t2=False)
    assert abs(e_corr - want["e_corr"]) <= TOL
    assert np.abs(obj.make_rdm1() - want["rdm1_mo"][np.ix_(perm, perm)]).max() <= TOL
    assert np.abs(obj.make_rdm1(ao_repr=True) - want["rdm1_ao"]).max() <= TOL
    with pytest.raises(NotImplementedError):
        mp.MP2(mf, mo_coeff=c_rot).kernel()                                  # other orbitals without their energies


def test_refusals(ctx):
    from libdmet_preview_amd.solver import mp, scf
    n = 6
    s, sysm = _converged("rhf", n, 0)
    for frozen in (1, [0], [0, 1]):
        with pytest.raises(NotImplementedError):
            mp.MP2(s.mf, frozen=frozen)
    assert mp.MP2(s.mf, frozen=0).frozen == 0 and mp.MP2(s.mf, frozen=None).frozen is None
    with pytest.raises(NotImplementedError):
        mp.UIMP2(s.mf)                                                       # a restricted object
    short = _solver(ctx, "rhf", n, 0, sysm)
    short.HF(tol=SCF_TOL, MaxIter=1)
    assert short.mf.converged is False
    with pytest.raises(NotImplementedError):
        mp.MP2(short.mf).kernel()                                            # PySCF would iterate the amplitudes
    e_corr, _ = mp.MP2(short.mf).kernel(mo_energy=short.mf.mo_energy)        # with explicit energies it is a plain evaluation
    want = M.rmp2(sysm, short.mf.mo_coeff, short.mf.mo_energy, R.nocc_of("rhf", n, 0)[0])
    assert abs(e_corr - want["e_corr"]) <= TOL
    for name in ("MP2", "GMP2"):                                             # SCF itself is not wired
        with pytest.raises(NotImplementedError):
            getattr(scf.SCF(), name)()


def test_mp2_runs_give_their_memory_back(ctx):
    """The pattern of tests/test_gpu_scf.py::test_hf_runs_give_their_memory_back: sync, trim, mem_info after every round; twenty
    rounds (a transform, a restricted and an unrestricted MP2 with amplitudes) end no more than 1 MiB below the mark taken after the
    warm-up rounds."""
    from libdmet_preview_amd.solver import mp, scf
    n = 33
    sr, su = R.System(n, 1, [16]), R.System(n, 2, [16])
    rhf, uhf = _solver(ctx, "rhf", n, 0, sr), _solver(ctx, "uhf", n, 0, su)
    rhf.HF(tol=1e-10)
    uhf.HF(tol=1e-10)
    d_E, d_C = _dev_block(ctx, sr, "aa"), ctx.to_device(np.asarray(rhf.mf.mo_coeff))

    def one_round():
        scf.ao2mo_block_dev(ctx, n, d_E, [d_C] * 4, compact=True, ws_bytes=1 << 22)      # several slabs
        mp.MP2(rhf.mf).kernel()
        mp.UIMP2(uhf.mf).kernel()
        mp.run_mp2(rhf)
    mark = free = None
    for it in range(3 + 20):
        one_round()
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == 2:
            mark = free
    assert mark - free < (1 << 20), (mark, free)
