"""
Host-side checks of unrestricted CCSD, no GPU: the plan formula, the refusals of solver/uccsd.py, and the numpy
reference of tests/uccsd_ref.py itself -- its closed-shell limit against tests/ccsd_ref.spin_orbital, its maps, and exactness for two
electrons (one alpha, one beta: CCSD is exact) against the diagonalisation in the n^2 space of (alpha, beta) determinants.  The
contraction lines of csrc/uccsd.hip (uc_rod) are also read from the source and evaluated in numpy against the spin-orbital step: the
spin-blocked equations are checked before any device runs them.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import scf_ref as R
from tests import uccsd_ref as UR

DMK_ERR_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_ELECTRON = ((4, 71), (9, 72))          # (n, seed): System(n, seed, [1, 1])


def _a256(count):
    return (8 * max(int(count), 1) + 255) & ~255


# DESIGN.md K24, "Memory": how many arrays of each shape the handle carves (o, v alpha; O, V beta)
K24_ARRAYS = {"oovv": 5, "oOvV": 5, "OOVV": 5, "vv": 3, "VV": 3, "oo": 3, "OO": 3, "ov": 3, "OV": 3, "oooo": 1, "oOoO": 1, "OOOO": 1,
              "ovvo": 1, "oVvO": 1, "oVVo": 1, "OvvO": 1, "OvVo": 1, "OVVO": 1, "ovoo": 2, "oVoO": 2, "OvoO": 2, "OVOO": 2, "oVOo": 1, "OvOo": 1,
              "o": 1, "O": 1, "v": 1, "V": 1}


def k24_bytes(oa, va, ob, vb, diis):
    """The formula of DESIGN.md K24: every array 256-byte aligned."""
    e = {"o": oa, "v": va, "O": ob, "V": vb}
    count = lambda t: int(np.prod([e[c] for c in t], dtype=np.int64))
    pad32 = lambda k: (k + 31) // 32 * 32
    nx = sum(pad32(count(t)) for t in ("ov", "OV", "oovv", "oOvV", "OOVV"))
    handle = (2 + 2 * diis) * _a256(nx) + sum(k * _a256(count(t)) for t, k in K24_ARRAYS.items()) + _a256(2048) + _a256(16)
    big = 0
    for (o, v), (p, q) in (((oa, va), (oa, va)), ((ob, vb), (ob, vb)), ((oa, va), (ob, vb))):
        first, second = (o * o, o * v, v * v), (p * p, p * q, q * q)
        big = max([big] + [first[x] * second[y] for x in range(3) for y in range(3) if x + y < 4])
    return handle, 3 * _a256(big)


def test_plan_returns_the_bytes_of_the_formula():
    from libdmet_preview_amd._lib import lib
    from libdmet_preview_amd.solver import uccsd
    out = (C.c_int64 * 2)()
    for ext in ((1, 1, 1, 1), (4, 2, 2, 4), (33, 32, 31, 34)):
        for diis in (0, 8):
            assert lib.dmk_uccsd_plan(*(ext + (diis, out))) == 0
            assert (int(out[0]), int(out[1])) == k24_bytes(*(ext + (diis,))), (ext, diis)
            assert uccsd.plan_bytes(*(ext + (diis,))) == k24_bytes(*(ext + (diis,)))
    # with equal extents the contraction workspace is the restricted one
    from tests.test_host_ccsd import k21_bytes
    assert k24_bytes(5, 7, 5, 7, 8)[1] == k21_bytes(5, 7, 8)[1]
    for k in range(4):
        for bad in (0, 513, -1):
            ext = [3, 3, 3, 3]
            ext[k] = bad
            assert lib.dmk_uccsd_plan(*(ext + [8, out])) == DMK_ERR_INVALID
    assert lib.dmk_uccsd_plan(3, 3, 3, 3, 13, out) == DMK_ERR_INVALID and lib.dmk_uccsd_plan(3, 3, 3, 3, -1, out) == DMK_ERR_INVALID
    assert lib.dmk_uccsd_plan(3, 3, 3, 3, 8, None) == DMK_ERR_INVALID
    with pytest.raises(ValueError, match="dmk_uccsd_plan"):
        uccsd.plan_bytes(3, 0, 3, 3, 8)


def test_module_imports_without_a_gpu_and_refuses_what_is_not_built():
    from libdmet_preview_amd.solver import cc, scf, uccsd
    from libdmet_preview_amd.solver._posthf import PostHFBase
    assert issubclass(uccsd.UCCSD, PostHFBase) and uccsd.UCCSD._restricted is False
    for frozen in (1, [0], [0, 1]):
        with pytest.raises(NotImplementedError, match="frozen"):
            uccsd.UCCSD(object(), frozen=frozen)
    with pytest.raises(NotImplementedError, match="DeviceHF"):
        uccsd.UCCSD(object())
    mf = object.__new__(scf.DeviceHF)                 # a bare restricted object: the check needs no device
    mf._restricted = True
    with pytest.raises(NotImplementedError, match="a restricted"):
        uccsd.UCCSD(mf)
    mf._ctx = None
    obj = object.__new__(uccsd.UCCSD)                 # the option checks need no device
    obj.level_shift, obj.iterative_damping, obj.diis_space = 0.0, 1.0, 8
    obj._check_options()
    obj.level_shift = 0.1
    with pytest.raises(NotImplementedError, match="level shift"):
        obj._check_options()
    obj.level_shift, obj.iterative_damping = 0.0, 0.8
    with pytest.raises(NotImplementedError, match="damping"):
        obj._check_options()
    obj.iterative_damping, obj.diis_space = 1.0, 13
    with pytest.raises(ValueError, match="diis_space"):
        obj._check_options()
    for call, name in ((obj.solve_lambda, "Lambda"), (obj.make_rdm1, "density"), (obj.make_rdm2, "density"), (obj.ccsd_t, r"\(T\)")):
        with pytest.raises(NotImplementedError, match=name):
            call()
    with pytest.raises(NotImplementedError, match=r"solver\.uccsd\.UCCSD"):          # the stub of solver/cc.py says where it is
        cc.UCCSD()
    obj._h = obj._eris = None                         # (so that the destructor of the bare object has nothing to do)
    # the struct of pointers is the header's: 2 Fock matrices, 21 blocks, 3 pitches
    assert [f[0] for f in uccsd._Ints._fields_] == ["fock_a", "fock_b"] + list(UR.BLOCKS_U) + ["ld_vvvv", "ld_VVVV", "ld_vvVV"]
    assert C.sizeof(uccsd._Ints) == 8 * 26


def test_closed_shell_limit_of_the_reference():
    """With B = A and [3, 3] occupied of 6 the two-orbital-set builder gives the Hamiltonian of ccsd_ref.spin_orbital exactly."""
    n, o = 6, 3
    sysm = R.System(n, 11, [o])
    sysm.B = sysm.A
    ref = R.scf(sysm.h1[None], sysm.veff_rhf, [o], True)
    Cmo = CR.rotate_ov(ref["mo_coeff"], o)
    so, su = CR.spin_orbital(sysm, Cmo, o), UR.spin_orbital_u(sysm, Cmo, Cmo, o, o)
    for name in ("foo", "fov", "fvv", "oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv"):
        assert np.abs(getattr(so, name) - getattr(su, name)).max() <= 1e-14, name
    t1, t2 = CR.random_amplitudes(np.random.default_rng(5), o, n - o)
    amps = (t1, t1, t2 - t2.transpose(0, 1, 3, 2), t2, t2 - t2.transpose(0, 1, 3, 2))
    T, Tu = CR.to_so(t1, t2), UR.to_so_u(*amps)
    assert np.array_equal(T[0], Tu[0]) and np.array_equal(T[1], Tu[1])
    assert CR.energy(so, *T) == CR.energy(su, *Tu)                    # the energy is the same number
    assert abs(UR.u_energy(su, amps) - CR.r_energy(so, t1, t2)) <= 1e-14


def test_maps_close_and_keep_the_antisymmetry():
    n, oa, ob = 6, 4, 2
    sysm = R.System(n, 31, [oa, ob])
    Ca, Cb, _ = UR.uhf_orbitals(sysm, [oa, ob])
    so = UR.spin_orbital_u(sysm, CR.rotate_ov(Ca, oa, 0.05), CR.rotate_ov(Cb, ob, -0.08), oa, ob)
    assert np.abs(so.fov).max() > 1e-3
    amps = UR.random_amplitudes_u(np.random.default_rng(3), oa, ob, n - oa, n - ob)
    for t in (amps[2], amps[4]):
        assert np.abs(t + t.transpose(1, 0, 2, 3)).max() == 0.0 and np.abs(t + t.transpose(0, 1, 3, 2)).max() == 0.0
    T1, T2 = UR.to_so_u(*amps)
    assert np.abs(T2 + T2.transpose(1, 0, 2, 3)).max() == 0.0 and np.abs(T2 + T2.transpose(0, 1, 3, 2)).max() == 0.0
    back = UR.from_so_u(T1, T2, oa, n - oa)
    assert all(np.array_equal(x, y) for x, y in zip(back, amps))
    N1, N2 = CR.update(so, T1, T2)                    # the step keeps the spin structure: the maps close on it
    M1, M2 = UR.to_so_u(*UR.from_so_u(N1, N2, oa, n - oa))
    assert np.abs(M1 - N1).max() <= 1e-14 and np.abs(M2 - N2).max() <= 1e-14
    # the blocks handed to the device are the reference's own integrals
    fa, fb, blocks = UR.ints_u(sysm, Ca, Cb, oa, ob, pad=3)
    assert set(blocks) == set(UR.BLOCKS_U)
    gab = sysm.lam * np.einsum("Ppq,Prs->pqrs", sysm.A, sysm.B)                           # the AO (pq|rs) of the ab block, literally
    got = np.einsum("pqrs,pi,qj,rk,sl->ijkl", gab, Ca[:, :oa], Ca[:, oa:], Cb[:, :ob], Cb[:, ob:])
    assert np.abs(blocks["ovOV"] - got).max() <= 1e-13
    assert np.abs(blocks["OVoo"] - np.einsum("pqrs,pi,qj,rk,sl->klij", gab, Ca[:, :oa], Ca[:, :oa], Cb[:, :ob], Cb[:, ob:])).max() <= 1e-13
    va, vb = n - oa, n - ob
    packed = blocks["vvVV"]
    assert packed.shape == (va * (va + 1) // 2, vb * (vb + 1) // 2 + 3) and np.all(np.isnan(packed[:, -3:]))


@pytest.mark.parametrize("n,seed", TWO_ELECTRON)
def test_reference_is_exact_for_two_electrons(n, seed):
    sysm = R.System(n, seed, [1, 1])
    Ca, Cb, ref = UR.uhf_orbitals(sysm, [1, 1])
    so = UR.spin_orbital_u(sysm, Ca, Cb, 1, 1)
    e_corr, amps, it = UR.u_solve(so, 1e-12)
    exact, gap = UR.exact_two_electron(sysm)
    print("n = %d: E_HF + E_corr = %.12f, exact = %.12f (gap %.2f), %d iterations" % (n, ref["E"] + e_corr, exact, gap, it))
    assert gap > 1.0 and abs(ref["E"] + e_corr - exact) <= 1e-9
    assert e_corr < 0.0 and amps[3].shape == (1, 1, n - 1, n - 1) and np.abs(amps[2]).max() == 0.0 and np.abs(amps[4]).max() == 0.0


# ---- the equations of csrc/uccsd.hip, read from the source and evaluated in numpy -----------------------------------------------------
_CT = re.compile(r'CT\(([-\d.]+), (\w+), "(\w+)", (\w+), "(\w+)", ([\d.]+), (\w+), "(\w+)"\);')
_PM = re.compile(r'PM\(([-\d.]+), (\w+), "(\w+)", ([\d.]+), (\w+), "(\w+)"\);')
_TAU = re.compile(r'TAU\(([\d.]+), ([\d.]+), (\d), (\d), (\w+)\);')
_LAD = re.compile(r'LADDER\([^;]*I\.(\w+), I\.ld_\w+, (\w+), (\w+)\);')


def _uc_rod_lines():
    src = open(os.path.join(ROOT, "libdmet_preview_amd", "csrc", "uccsd.hip")).read()
    body = src[src.index("int uc_rod(dmk_uccsd *h, const double *src) {"):]
    body = body[body.index("int rc;"):body.index("return DMK_OK;")]
    lines = [ln.strip() for ln in body.splitlines()[1:] if ln.strip() and not ln.strip().startswith("//")]
    return lines


def _run_uc_rod(lines, env, full):
    """The CT / PM / TAU / LADDER lines as einsums over `env` (name -> array); `full`: the three vvvv-type blocks as [a, c, b, d]."""
    t1, t2 = ("t1a", "t1b"), ("t2aa", "t2ab", "t2bb")
    for ln in lines:
        m = _CT.fullmatch(ln)
        if m:
            c, A, sa, B, sb, beta, Cn, sc = m.groups()
            val = float(c) * np.einsum("%s,%s->%s" % (sa, sb, sc), env[A], env[B], optimize=True)
            env[Cn] = val + (env[Cn] if float(beta) else 0.0)
            continue
        m = _PM.fullmatch(ln)
        if m:
            c, A, sa, beta, Cn, sc = m.groups()
            val = float(c) * np.einsum("%s->%s" % (sa, sc), env[A])
            env[Cn] = val + (env[Cn] if float(beta) else 0.0)
            continue
        m = _TAU.fullmatch(ln)
        if m:
            c2, c1, si, sj, out = m.groups()
            si, sj = int(si), int(sj)
            env[out] = float(c2) * env[t2[si + sj]] + float(c1) * np.einsum("ia,jb->ijab", env[t1[si]], env[t1[sj]])
            continue
        m = _LAD.fullmatch(ln)
        assert m, "a line of uc_rod that is neither CT, PM, TAU nor LADDER: %r" % ln
        W, tau, dst = m.groups()
        env[dst] = env[dst] + np.einsum("ijcd,acbd->ijab", env[tau], full[W])
    return env


@pytest.mark.parametrize("n,nocc,rotated", [(5, (3, 1), True), (5, (1, 3), True), (4, (2, 2), False), (6, (3, 2), True), (2, (1, 1), True)])
def test_the_lines_of_uc_rod_are_the_spin_orbital_step(n, nocc, rotated):
    """What csrc/uccsd.hip computes, without a device: its contraction lines read from the source, evaluated by numpy over the blocks
    of ints_u and divided by the Fock-diagonal denominators, equal ccsd_ref.update at random amplitudes (every term at full
    strength, non-canonical orbitals).  Bound 1e-14: both sides are float64 sums of a few hundred terms of size <= 0.1 (eps 1.1e-16)
    in different orders."""
    oa, ob = nocc
    va, vb = n - oa, n - ob
    sysm = R.System(n, 80 + n + oa, [oa, ob])
    Ca, Cb, _ = UR.uhf_orbitals(sysm, [oa, ob])
    if rotated:
        Ca, Cb = CR.rotate_ov(Ca, oa, 0.05), CR.rotate_ov(Cb, ob, -0.08)
    so = UR.spin_orbital_u(sysm, Ca, Cb, oa, ob)
    amps = UR.random_amplitudes_u(np.random.default_rng(n), oa, ob, va, vb)
    fa, fb, blocks = UR.ints_u(sysm, Ca, Cb, oa, ob, pad=0)
    env = {k: v for k, v in blocks.items() if k not in UR.PACKED}
    part = UR._parts(Ca, Cb, oa, ob)
    full = {k: UR.chem_block(sysm, k, part) for k in UR.PACKED}
    off = lambda f: f - np.diag(np.diag(f))
    for s, f, o in (("a", fa, oa), ("b", fb, ob)):
        env["fov" + s], env["foo" + s], env["fvv" + s] = f[:o, o:], off(f[:o, :o]), off(f[o:, o:])
    env.update(zip(("t1a", "t1b", "t2aa", "t2ab", "t2bb"), amps))
    lines = _uc_rod_lines()
    assert len(lines) > 200 and sum(ln.startswith("LADDER") for ln in lines) == 3
    _run_uc_rod(lines, env, full)
    ea, eb = np.diag(fa), np.diag(fb)
    d2 = lambda e1, o1, e2, o2: (e1[:o1, None, None, None] + e2[None, :o2, None, None] - e1[None, None, o1:, None] - e2[None, None, None, o2:])
    got = (env["n1a"] / (ea[:oa, None] - ea[None, oa:]), env["n1b"] / (eb[:ob, None] - eb[None, ob:]), env["Raa"] / d2(ea, oa, ea, oa),
           env["Rab"] / d2(ea, oa, eb, ob), env["Rbb"] / d2(eb, ob, eb, ob))
    want = UR.u_update(so, amps)
    err = max(float(np.abs(x - y).max()) for x, y in zip(got, want))
    print("n = %d, nocc = %s: %d lines, max|dt| = %.3e" % (n, nocc, len(lines), err))
    assert err <= 1e-14
