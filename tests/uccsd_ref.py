"""
Numpy reference of UNRESTRICTED CCSD for the tests of DESIGN.md K24 (tests/test_host_uccsd.py, tests/test_gpu_uccsd*.py): the
spin-orbital equations of tests/ccsd_ref.py (update, energy, solve are used as they stand) over a spin-orbital Hamiltonian built from
TWO sets of orbitals and the three integral blocks 'aa', 'bb', 'ab' of a tests/scf_ref.System, whose alpha and beta factors differ --
a swapped block shows.  Nothing here shares a formula with the device code, which works on spin blocks over chemists' integrals.

Spin orbitals are ordered [occupied alpha, occupied beta | virtual alpha, virtual beta].

    spin_orbital_u(sysm, Ca, Cb, oa, ob)   -> ccsd_ref.SO at the orbitals Ca, Cb (columns, the occupied first); every <pq||rs> block is
                                           assembled one spin block at a time from mp2_ref.transform ('aa', 'bb', 'ab', and the
                                           transpose of 'ab' for a beta bra with an alpha ket); no (2n)^4 tensor is held
    to_so_u / from_so_u                    (t1a, t1b, t2aa, t2ab, t2bb) <-> spin-orbital (T1, T2)
    random_amplitudes_u                    scale 0.1, t2aa / t2bb antisymmetric in ij and in ab
    ints_u                                 the two MO Fock matrices and the blocks of dmk_uccsd_ints (BLOCKS_U), the three packed ones
                                           with pitch npair + pad and a NaN pad
    u_update / u_energy / u_solve / converged_reference_u     ccsd_ref's through the maps
    uhf_orbitals(sysm, nocc)               orbitals of the numpy UHF of tests/scf_ref.py, [occupied | virtual]
    exact_two_electron(sysm)               lowest eigenvalue of h x 1 + 1 x h + (pr|qs)_ab in the n^2 space |p alpha, q beta>
"""
import numpy as np

from tests import ccsd_ref as CC
from tests import mp2_ref as M
from tests import scf_ref as R

# what csrc/uccsd.hip reads; lower case alpha, upper case beta, (pq|rs) row-major in the order of the letters
BLOCKS_U = ("oooo", "ovoo", "ovov", "oovv", "ovvv", "vvvv", "OOOO", "OVOO", "OVOV", "OOVV", "OVVV", "VVVV",
            "ooOO", "ovOO", "ovOV", "ooVV", "ovVV", "vvVV", "OVoo", "OOvv", "OVvv")
PACKED = ("vvvv", "VVVV", "vvVV")


def _parts(Ca, Cb, oa, ob):
    Ca, Cb = np.asarray(Ca, dtype=np.float64), np.asarray(Cb, dtype=np.float64)
    return {"o": Ca[:, :oa], "v": Ca[:, oa:], "O": Cb[:, :ob], "V": Cb[:, ob:]}


def chem_block(sysm, name, part):
    """(pq|rs) for the four ranges named by `name` (case = spin), as a 4-index array."""
    c = [part[x] for x in name]
    bra, ket = "ab"[name[0].isupper()], "ab"[name[2].isupper()]
    shape = [x.shape[1] for x in c]
    if bra + ket == "ba":                                               # no block of its own: the transpose of its alpha-beta twin
        g = M.transform(sysm, "ab", c[2], c[3], c[0], c[1]).T
    else:
        g = M.transform(sysm, bra + ket, *c)
    return g.reshape(shape)


def _phys(sysm, part, sl):
    """<pq|rs> = (pr|qs) delta(spin p, spin r) delta(spin q, spin s) over spin orbitals, for the block types sl of 'o' / 'v'."""
    dim = lambda c, s: part[c.upper() if s else c].shape[1]
    tot = [dim(c, 0) + dim(c, 1) for c in sl]
    out = np.zeros(tot)
    rng = lambda c, s: slice(0, dim(c, 0)) if s == 0 else slice(dim(c, 0), dim(c, 0) + dim(c, 1))
    case = lambda c, s: c.upper() if s else c
    for s1 in range(2):
        for s2 in range(2):
            name = case(sl[0], s1) + case(sl[2], s1) + case(sl[1], s2) + case(sl[3], s2)       # (p r | q s)
            g = chem_block(sysm, name, part)
            out[rng(sl[0], s1), rng(sl[1], s2), rng(sl[2], s1), rng(sl[3], s2)] = g.transpose(0, 2, 1, 3)
    return out


def _anti(sysm, part, sl):
    return _phys(sysm, part, sl) - _phys(sysm, part, sl[0] + sl[1] + sl[3] + sl[2]).transpose(0, 1, 3, 2)


def fock_u(sysm, Ca, Cb, oa, ob):
    """The two MO Fock matrices C_s^T (h1 + veff_uhf(D))_s C_s of the density of the occupied columns."""
    Ca, Cb = np.asarray(Ca, dtype=np.float64), np.asarray(Cb, dtype=np.float64)
    D = np.asarray([Ca[:, :oa] @ Ca[:, :oa].T, Cb[:, :ob] @ Cb[:, :ob].T])
    F = sysm.h1[None] + sysm.veff_uhf(D)
    return Ca.T @ F[0] @ Ca, Cb.T @ F[1] @ Cb


def _bd(a, b):
    out = np.zeros((a.shape[0] + b.shape[0], a.shape[1] + b.shape[1]))
    out[:a.shape[0], :a.shape[1]] = a
    out[a.shape[0]:, a.shape[1]:] = b
    return out


def spin_orbital_u(sysm, Ca, Cb, oa, ob):
    part = _parts(Ca, Cb, oa, ob)
    fa, fb = fock_u(sysm, Ca, Cb, oa, ob)
    so = CC.SO()
    so.oa, so.ob, so.va, so.vb = oa, ob, sysm.n - oa, sysm.n - ob
    so.foo, so.fov, so.fvv = _bd(fa[:oa, :oa], fb[:ob, :ob]), _bd(fa[:oa, oa:], fb[:ob, ob:]), _bd(fa[oa:, oa:], fb[ob:, ob:])
    for name in ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv"):
        setattr(so, name, _anti(sysm, part, name))
    so.eo, so.ev = np.diag(so.foo).copy(), np.diag(so.fvv).copy()
    so.f_mo = (fa, fb)
    return so


def to_so_u(t1a, t1b, t2aa, t2ab, t2bb):
    (oa, va), (ob, vb) = t1a.shape, t1b.shape
    T1 = _bd(t1a, t1b)
    T2 = np.zeros((oa + ob, oa + ob, va + vb, va + vb))
    a, b, A, B = slice(0, oa), slice(oa, oa + ob), slice(0, va), slice(va, va + vb)
    T2[a, a, A, A], T2[b, b, B, B] = t2aa, t2bb
    T2[a, b, A, B] = t2ab
    T2[b, a, B, A] = t2ab.transpose(1, 0, 3, 2)
    T2[a, b, B, A] = -t2ab.transpose(0, 1, 3, 2)
    T2[b, a, A, B] = -t2ab.transpose(1, 0, 2, 3)
    return T1, T2


def from_so_u(T1, T2, oa, va):
    a, b, A, B = slice(0, oa), slice(oa, None), slice(0, va), slice(va, None)
    return T1[a, A].copy(), T1[b, B].copy(), T2[a, a, A, A].copy(), T2[a, b, A, B].copy(), T2[b, b, B, B].copy()


def random_amplitudes_u(rng, oa, ob, va, vb, scale=0.1):
    def anti(t):                                   # two differences in a row: antisymmetric to the bit
        x = t - t.transpose(1, 0, 2, 3)
        return 0.5 * (x - x.transpose(0, 1, 3, 2))
    g = lambda *s: scale * rng.standard_normal(s)
    return g(oa, va), g(ob, vb), anti(g(oa, oa, va, va)), g(oa, ob, va, vb), anti(g(ob, ob, vb, vb))


def u_update(so, amps):
    return from_so_u(*CC.update(so, *to_so_u(*amps)), so.oa, so.va)


def u_energy(so, amps):
    return CC.energy(so, *to_so_u(*amps))


def u_solve(so, tol, max_iter=500, amps=None):
    T = (None, None) if amps is None else to_so_u(*amps)
    e, T1, T2, it = CC.solve(so, tol, max_iter, T1=T[0], T2=T[1])
    return e, from_so_u(T1, T2, so.oa, so.va), it


def converged_reference_u(so):
    """As ccsd_ref.converged_reference: ((e, amps) at |dt| < 1e-11, delta_e, delta_t against the run at 1e-9)."""
    e9, a9, _ = u_solve(so, 1e-9)
    e11, a11, _ = u_solve(so, 1e-11, amps=a9)
    return (e11, a11), abs(e9 - e11), max(np.abs(x - y).max() for x, y in zip(a9, a11))


def ints_u(sysm, Ca, Cb, oa, ob, pad=3):
    """(fock_a, fock_b, blocks): blocks[name] for BLOCKS_U; the packed ones (rows pair over the bra's virtuals, columns pair over the
    ket's) have the row pitch npair_ket + pad with a NaN pad."""
    part = _parts(Ca, Cb, oa, ob)
    fa, fb = fock_u(sysm, Ca, Cb, oa, ob)
    blocks = {}
    for name in BLOCKS_U:
        if name in PACKED:
            c = [part[x] for x in name]
            v1, v2 = c[0].shape[1], c[2].shape[1]
            g = M.pack_cols(M.pack_rows(chem_block(sysm, name, part).reshape(v1 * v1, v2 * v2), v1), v2)
            blocks[name] = np.full((g.shape[0], g.shape[1] + pad), np.nan)
            blocks[name][:, :g.shape[1]] = g
        else:
            blocks[name] = np.ascontiguousarray(chem_block(sysm, name, part))
    return fa, fb, blocks


def uhf_orbitals(sysm, nocc):
    ref = R.scf(np.asarray([sysm.h1, sysm.h1]), sysm.veff_uhf, list(nocc), False)
    assert ref["converged"], nocc
    return ref["mo_coeff"][0], ref["mo_coeff"][1], ref


def uneven_system_u(n, oa, ob):
    """(system, Ca, Cb) of the cases of tests/test_gpu_uccsd_shapes.py: System(n, 600 + 37 oa + ob, [oa, ob]), numpy UHF orbitals."""
    sysm = R.System(n, 600 + 37 * oa + ob, [oa, ob])
    Ca, Cb, ref = uhf_orbitals(sysm, [oa, ob])
    assert ref["gap"] > 1.0, (n, oa, ob, ref["gap"])
    return sysm, Ca, Cb


def exact_two_electron(sysm):
    """Lowest eigenvalue of H = h(1) + h(2) + (pr|qs)_ab in the n^2 space |p alpha, q beta> (AO basis, orthonormal); gap to the next."""
    n = sysm.n
    eye = np.eye(n)
    g = M.transform(sysm, "ab", eye, eye, eye, eye).reshape(n, n, n, n)          # (pr|qs) at g[p, r, q, s]
    H = np.einsum("pr,qs->pqrs", sysm.h1, eye) + np.einsum("pr,qs->pqrs", eye, sysm.h1) + g.transpose(0, 2, 1, 3)
    w = np.linalg.eigvalsh(H.reshape(n * n, n * n))
    return float(w[0]), float(w[1] - w[0])
