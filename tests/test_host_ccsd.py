"""
Host-side checks of the CCSD layer, no GPU: the spin-orbital reference of tests/ccsd_ref.py validates itself against
exact diagonalisation (CCSD is exact for two electrons), the restricted blocks and energy that tests/test_gpu_ccsd_shapes.py hands to
the C ABI agree with it (so that a mistake in that helper is not blamed on the device), the planner dmk_rccsd_plan returns the byte counts of K21's formula, and
solver/cc.py imports without a GPU and refuses by name what is not built.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import scf_ref as R

DMK_ERR_INVALID = -1
TWO_ELECTRON = [(5, 31), (6, 32)]          # (n, seed) of System(n, seed, cuts=[1]); shared with tests/test_gpu_ccsd.py


def two_electron_hf(n, seed):
    sysm = R.System(n, seed, [1])
    ref = R.scf(sysm.h1[None], lambda D: sysm.veff_rhf(D), [1], True)
    assert ref["converged"]
    return sysm, ref


@pytest.mark.parametrize("n,seed", TWO_ELECTRON)
def test_reference_is_exact_for_two_electrons(n, seed):
    sysm, ref = two_electron_hf(n, seed)
    so = CR.spin_orbital(sysm, ref["mo_coeff"], 1)
    e_corr, t1, t2, it = CR.r_solve(so, 1e-12)
    exact = CR.exact_two_electron_singlet(sysm)
    print("n = %d: E_HF + E_corr = %.12f, exact singlet = %.12f, %d iterations" % (n, ref["E"] + e_corr, exact, it))
    assert abs(ref["E"] + e_corr - exact) <= 1e-9
    assert e_corr < 0.0 and t1.shape == (1, n - 1) and t2.shape == (1, 1, n - 1, n - 1)


def test_reference_maps_and_symmetry():
    n, o = 7, 3
    ref = R.run_case("rhf", n, 0, seed=41)
    so = CR.spin_orbital(ref["system"], CR.rotate_ov(ref["mo_coeff"], o), o)
    assert np.abs(so.fov).max() > 1e-3 and np.abs(so.foo - np.diag(so.eo)).max() > 1e-4          # non-canonical
    t1, t2 = CR.random_amplitudes(np.random.default_rng(2), o, n - o)
    T1, T2 = CR.to_so(t1, t2)
    assert np.abs(T2 + T2.transpose(1, 0, 2, 3)).max() == 0.0 and np.abs(T2 + T2.transpose(0, 1, 3, 2)).max() == 0.0
    b1, b2 = CR.from_so(T1, T2)
    assert np.array_equal(b1, t1) and np.array_equal(b2, t2)
    N1, N2 = CR.update(so, T1, T2)                    # the step keeps the spin adaptation: the maps close on it
    n1, n2 = CR.from_so(N1, N2)
    M1, M2 = CR.to_so(n1, n2)
    assert np.abs(M1 - N1).max() <= 1e-14 and np.abs(M2 - N2).max() <= 1e-14
    assert np.abs(n2 - n2.transpose(1, 0, 3, 2)).max() <= 1e-14


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("o,v", [(2, 5), (5, 2)])
def test_restricted_blocks_and_energy_agree_with_the_spin_orbital_reference(o, v, rotated):
    sysm, C = CR.uneven_system(o, v)
    if rotated:
        C = CR.rotate_ov(C, o)
    so = CR.spin_orbital(sysm, C, o)
    fock, blocks = CR.restricted_blocks(sysm, C, o, pad=3)
    n, npair = o + v, v * (v + 1) // 2
    assert np.array_equal(fock, so.f_mo) and fock.shape == (n, n)
    assert [blocks[k].shape for k in CR.BLOCKS[:-1]] == [tuple({"o": o, "v": v}[x] for x in k) for k in CR.BLOCKS[:-1]]
    g = sysm.lam * np.einsum("Ppq,Prs->pqrs", sysm.A, sysm.A)                             # the AO (pq|rs), literally
    for name in CR.BLOCKS[:-1]:
        c = [C[:, :o] if x == "o" else C[:, o:] for x in name]
        assert np.abs(blocks[name] - np.einsum("pqrs,pi,qj,rk,sl->ijkl", g, *c)).max() <= 1e-13, name
    vvvv = np.einsum("pqrs,pi,qj,rk,sl->ijkl", g, *([C[:, o:]] * 4))
    packed = blocks["vvvv"]
    assert packed.shape == (npair, npair + 3) and np.all(np.isnan(packed[:, npair:]))
    assert np.abs(R.restore_s1(packed[:, :npair], v) - vvvv).max() <= 1e-13
    for t1, t2 in (CR.random_amplitudes(np.random.default_rng(100 + n), o, v), CR.from_so(*CR.mp2_guess(so))):
        e, e_so = CR.restricted_energy(fock, blocks, t1, t2), CR.r_energy(so, t1, t2)
        print("(o, v) = (%d, %d)%s: restricted %.15f, spin-orbital %.15f" % (o, v, " rotated" if rotated else "", e, e_so))
        assert abs(e - e_so) <= 1e-12
    if rotated:
        assert np.abs(fock[:o, o:]).max() > 1e-3


def _a256(count):
    return (8 * max(int(count), 1) + 255) & ~255


def k21_bytes(o, v, diis):
    """The formula of DESIGN.md K21: every array 256-byte aligned."""
    nx = (o * v + 31) // 32 * 32 + o * o * v * v
    handle = (2 + 2 * diis) * _a256(nx) + 8 * _a256(o * o * v * v) + _a256(o ** 4) + 2 * _a256(o ** 3 * v) + 5 * _a256(o * o) \
        + 3 * _a256(v * v) + 3 * _a256(o * v) + _a256(o) + _a256(v) + _a256(2048) + _a256(16)
    big = max(o ** 4, o ** 3 * v, o * o * v * v, o * v ** 3)
    return handle, 3 * _a256(big)


def test_plan_returns_the_bytes_of_the_formula():
    from libdmet_preview_amd._lib import lib
    from libdmet_preview_amd.solver import cc
    out = (C.c_int64 * 2)()
    for o, v, diis in ((1, 1, 0), (3, 3, 8), (32, 33, 8)):
        assert lib.dmk_rccsd_plan(o, v, diis, out) == 0
        assert (int(out[0]), int(out[1])) == k21_bytes(o, v, diis), (o, v, diis)
        assert cc.plan_bytes(o, v, diis) == k21_bytes(o, v, diis)
    for o, v, diis in ((0, 3, 8), (3, 0, 8), (3, 3, 13), (-1, 3, 0)):
        assert lib.dmk_rccsd_plan(o, v, diis, out) == DMK_ERR_INVALID
    assert lib.dmk_rccsd_plan(3, 3, 8, None) == DMK_ERR_INVALID


def test_module_imports_without_a_gpu_and_refuses_what_is_not_built():
    from libdmet_preview_amd.solver import cc, mp
    from libdmet_preview_amd.solver._posthf import PostHFBase
    assert callable(cc.RCCSD) and callable(cc.run_ccsd) and cc.CCSD is cc.RCCSD
    assert issubclass(cc.RCCSD, PostHFBase) and issubclass(mp.MP2, PostHFBase)          # one copy of the argument checks
    for frozen in (1, [0], [0, 1]):
        with pytest.raises(NotImplementedError, match="frozen"):
            cc.RCCSD(object(), frozen=frozen)
    with pytest.raises(NotImplementedError, match="DeviceHF"):
        cc.RCCSD(object())
    obj = object.__new__(cc.RCCSD)                    # the option checks need no device
    obj.level_shift, obj.iterative_damping, obj.diis_space = 0.0, 1.0, 8
    obj._check_options()
    obj.level_shift = 0.1
    with pytest.raises(NotImplementedError, match="level shift"):
        obj._check_options()
    obj.level_shift, obj.iterative_damping = 0.0, 0.8
    with pytest.raises(NotImplementedError, match="damping"):
        obj._check_options()
    for call, name in ((obj.solve_lambda, "Lambda"), (obj.make_rdm1, "density"), (obj.make_rdm2, "density"), (obj.ccsd_t, r"\(T\)"),
                       (cc.UCCSD, "UCCSD"), (cc.GCCSD, "GCCSD"), (cc.run, "CCSD.run"), (cc.run_dmet_ham, "run_dmet_ham")):
        with pytest.raises(NotImplementedError, match=name):
            call()
    for key, name in (("ccsdt", r"\(T\)"), ("bcc", "Brueckner"), ("tcc", "Tailored"), ("calc_rdm2", "density"), ("restart", "Restart")):
        with pytest.raises(NotImplementedError, match=name):
            cc.run_ccsd(None, **{key: True})
    with pytest.raises(TypeError):
        cc.run_ccsd(None, no_such_option=1)
    obj._h = obj._eris = None                         # (so that the destructor of the bare object has nothing to do)
