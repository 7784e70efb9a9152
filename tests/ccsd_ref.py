"""
Numpy restatement of closed-shell CCSD for the tests of DESIGN.md K21 (tests/test_host_ccsd.py, tests/test_gpu_ccsd.py), in a
formulation that shares nothing with the device code: SPIN-ORBITAL CCSD with antisymmetrised integrals <pq||rs> and literal einsums
for the textbook T1 / T2 equations with a general (non-canonical) Fock matrix (Stanton, Gauss, Watts, Bartlett, J. Chem. Phys. 94,
4334 (1991), equations 1-13), on the factored Hamiltonians of tests/scf_ref.py through mp2_ref.transform.

Spin orbitals are ordered [occupied alpha, occupied beta | virtual alpha, virtual beta].  A restricted (t1 (o, v), t2 (o, o, v, v),
t_ij^ab = t_ji^ba) maps to spin-orbital amplitudes as   aa = t - t^T(ab),   ab = t   (and the blocks that antisymmetry fixes).

    spin_orbital(sysm, C, nocc)   -> SO: the Fock blocks and the <pq||rs> blocks at the orbitals C (columns, occupied first)
    update(so, T1, T2)            one application of the amplitude equations (Jacobi step with the Fock diagonal)
    energy(so, T1, T2)            f_ia t_ia + 1/4 <ij||ab> t_ijab + 1/2 <ij||ab> t_ia t_jb
    NP / torch_namespace()        update and energy_of are stated ONCE, over an array namespace (einsum, diag, axis permutation): numpy
                                  by default, torch tensors for the reverse-mode derivatives of tests/cclambda_ref.py
    solve(so, tol)                DIIS-free iteration from the MP2 guess until the amplitudes move by less than tol
    to_so / from_so               the maps between restricted and spin-orbital amplitudes
    r_update / r_energy / r_solve the same through the maps, on restricted amplitudes
    converged_reference(so)       DIIS-free solution at |dt| < 1e-11 with its own convergence uncertainty (against |dt| < 1e-9)
    uneven_system(o, v)           the host system and orbitals of the uneven-shape tests (no device SCF)
    restricted_blocks / restricted_energy   the Fock matrix and the seven SPATIAL blocks in the layout of dmk_rccsd_create, and the
                                  closed-shell energy over them: what a test hands to the C ABI without a device SCF or transform
    exact_two_electron_singlet    lowest singlet eigenvalue of H in the n^2 space of (alpha, beta) determinants
"""
import numpy as np

from tests import mp2_ref as M

ES = lambda *a: np.einsum(*a, optimize=True)


class NP(object):
    """The array namespace of the equations below for numpy arrays (real or complex)."""
    es = staticmethod(ES)
    diag = staticmethod(np.diag)
    tr = staticmethod(lambda x, *axes: x.transpose(*axes))


def torch_namespace():
    """The same three operations for torch tensors (imported here: the module imports without torch), so that autograd can go
    through update / energy_of: tests/cclambda_ref.py, the reverse-mode references."""
    import torch

    class TORCH(object):
        es = staticmethod(torch.einsum)
        diag = staticmethod(torch.diag)
        tr = staticmethod(lambda x, *axes: x.permute(*axes))
    return TORCH


class SO(object):
    pass


def _phys(g, sl, o):
    """<pq|rs> = (pr|qs) over spin orbitals for the block types sl = (X, Y, Z, W) of 'o' / 'v'; g the spatial (pq|rs), n^4."""
    n = g.shape[0]
    rng = {"o": slice(0, o), "v": slice(o, n)}
    X, Y, Z, W = (rng[c] for c in sl)
    sp = g[X, Z, Y, W].transpose(0, 2, 1, 3)                    # spatial <pq|rs>
    d = sp.shape
    out = np.zeros(tuple(2 * x for x in d))
    for s1 in range(2):
        for s2 in range(2):                                      # spin(p) = spin(r) = s1, spin(q) = spin(s) = s2
            out[s1 * d[0]:(s1 + 1) * d[0], s2 * d[1]:(s2 + 1) * d[1], s1 * d[2]:(s1 + 1) * d[2], s2 * d[3]:(s2 + 1) * d[3]] = sp
    return out


def _anti(g, sl, o):
    return _phys(g, sl, o) - _phys(g, sl[0] + sl[1] + sl[3] + sl[2], o).transpose(0, 1, 3, 2)


def spin_orbital(sysm, C, nocc, fock_ao=None):
    """The spin-orbital Hamiltonian at the orbitals C (n x n, the nocc occupied columns first).  fock_ao: the AO Fock matrix (default:
    the closed-shell one of the density of the occupied columns)."""
    n, o = sysm.n, nocc
    C = np.asarray(C, dtype=np.float64)
    if fock_ao is None:
        D = 2.0 * C[:, :o] @ C[:, :o].T
        fock_ao = sysm.h1 + sysm.veff_rhf(D)
    f = C.T @ fock_ao @ C
    g = M.transform(sysm, "aa", C, C, C, C).reshape(n, n, n, n)
    so = SO()
    so.o, so.v = o, n - o
    two = lambda a: np.kron(np.eye(2), a)
    so.foo, so.fov, so.fvv = two(f[:o, :o]), two(f[:o, o:]), two(f[o:, o:])
    for name in ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv"):
        setattr(so, name, _anti(g, name, o))
    so.eo, so.ev = np.diag(so.foo).copy(), np.diag(so.fvv).copy()
    so.f_mo = f
    return so


def _denoms(so):
    d1 = so.eo[:, None] - so.ev[None, :]
    return d1, d1[:, None, :, None] + d1[None, :, None, :]


def update(so, T1, T2, xp=NP):
    """One step of Stanton et al. eqs. 1-13; T1 (O, V), T2 (O, O, V, V) over spin orbitals.  xp: the array namespace of `so` and the
    amplitudes (NP, or torch_namespace() for tensors)."""
    ES, diag, tr = xp.es, xp.diag, xp.tr
    oooo, ooov, oovv, ovov, ovvv, vvvv = so.oooo, so.ooov, so.oovv, so.ovov, so.ovvv, so.vvvv
    fov = so.fov
    foo_od, fvv_od = so.foo - diag(so.eo), so.fvv - diag(so.ev)
    tt = ES("ia,jb->ijab", T1, T1)
    tau_t = T2 + 0.5 * (tt - tr(tt, 0, 1, 3, 2))
    tau = T2 + tt - tr(tt, 0, 1, 3, 2)
    # <am||ef> = -<ma||ef>;  <mb||ej> = -<mb||je>;  <mn||ej> = -<mn||je>
    Fae = fvv_od - 0.5 * ES("me,ma->ae", fov, T1) + ES("mf,mafe->ae", T1, ovvv) - 0.5 * ES("mnaf,mnef->ae", tau_t, oovv)
    Fmi = foo_od + 0.5 * ES("ie,me->mi", T1, fov) + ES("ne,mnie->mi", T1, ooov) + 0.5 * ES("inef,mnef->mi", tau_t, oovv)
    Fme = fov + ES("nf,mnef->me", T1, oovv)
    Wmnij = oooo + ES("je,mnie->mnij", T1, ooov) - ES("ie,mnje->mnij", T1, ooov) + 0.25 * ES("ijef,mnef->mnij", tau, oovv)
    Wabef = vvvv + ES("mb,maef->abef", T1, ovvv) - ES("ma,mbef->abef", T1, ovvv) + 0.25 * ES("mnab,mnef->abef", tau, oovv)
    Wmbej = -tr(ovov, 0, 1, 3, 2) + ES("jf,mbef->mbej", T1, ovvv) + ES("nb,mnje->mbej", T1, ooov) \
        - ES("jnfb,mnef->mbej", 0.5 * T2 + ES("jf,nb->jnfb", T1, T1), oovv)
    # T1
    r1 = fov + ES("ie,ae->ia", T1, Fae) - ES("ma,mi->ia", T1, Fmi) + ES("imae,me->ia", T2, Fme) - ES("nf,naif->ia", T1, ovov) \
        - 0.5 * ES("imef,maef->ia", T2, ovvv) + 0.5 * ES("mnae,nmie->ia", T2, ooov)
    # T2
    Fbe = Fae - 0.5 * ES("mb,me->be", T1, Fme)
    x = ES("ijae,be->ijab", T2, Fbe)
    r2 = oovv + x - tr(x, 0, 1, 3, 2)
    Fmj = Fmi + 0.5 * ES("je,me->mj", T1, Fme)
    x = ES("imab,mj->ijab", T2, Fmj)
    r2 = r2 - (x - tr(x, 1, 0, 2, 3))
    r2 = r2 + 0.5 * ES("mnab,mnij->ijab", tau, Wmnij) + 0.5 * ES("ijef,abef->ijab", tau, Wabef)
    x = ES("imae,mbej->ijab", T2, Wmbej) + ES("ie,ma,mbje->ijab", T1, T1, ovov)          # - t t <mb||ej> = + t t <mb||je>
    r2 = r2 + x - tr(x, 1, 0, 2, 3) - tr(x, 0, 1, 3, 2) + tr(x, 1, 0, 3, 2)
    x = -ES("ie,jeab->ijab", T1, ovvv)                                                    # <ab||ej> = -<je||ab>
    r2 = r2 + x - tr(x, 1, 0, 2, 3)
    x = ES("ma,ijmb->ijab", T1, ooov)                                                     # <mb||ij> = <ij||mb>
    r2 = r2 - (x - tr(x, 0, 1, 3, 2))
    d1, d2 = _denoms(so)
    return r1 / d1, r2 / d2


def energy_of(so, T1, T2, xp=NP):
    """The correlation energy as a 0-d array of the namespace (complex amplitudes and tensors keep their type)."""
    ES = xp.es
    return ES("ia,ia", so.fov, T1) + 0.25 * ES("ijab,ijab", so.oovv, T2) + 0.5 * ES("ijab,ia,jb", so.oovv, T1, T1)


def energy(so, T1, T2):
    return float(energy_of(so, T1, T2))


def mp2_guess(so):
    d1, d2 = _denoms(so)
    return so.fov / d1, so.oovv / d2


def solve(so, tol, max_iter=500, T1=None, T2=None):
    """DIIS-free: -> (e_corr, T1, T2, iterations); stops when sqrt(|dT1|^2 + |dT2|^2) < tol."""
    if T1 is None:
        T1, T2 = mp2_guess(so)
    for it in range(1, max_iter + 1):
        N1, N2 = update(so, T1, T2)
        dt = np.sqrt(np.sum((N1 - T1) ** 2) + np.sum((N2 - T2) ** 2))
        T1, T2 = N1, N2
        if dt < tol:
            return energy(so, T1, T2), T1, T2, it
    raise RuntimeError("the reference CCSD did not converge in %d iterations (|dT| = %.3e)" % (max_iter, dt))


def to_so(t1, t2):
    o, v = t1.shape
    T1 = np.kron(np.eye(2), t1)
    T2 = np.zeros((2 * o, 2 * o, 2 * v, 2 * v))
    a, b = slice(0, o), slice(o, 2 * o)
    A, B = slice(0, v), slice(v, 2 * v)
    same = t2 - t2.transpose(0, 1, 3, 2)
    T2[a, a, A, A] = T2[b, b, B, B] = same
    T2[a, b, A, B] = T2[b, a, B, A] = t2
    T2[a, b, B, A] = T2[b, a, A, B] = -t2.transpose(0, 1, 3, 2)
    return T1, T2


def from_so(T1, T2):
    o, v = T1.shape[0] // 2, T1.shape[1] // 2
    return T1[:o, :v].copy(), T2[:o, o:, :v, v:].copy()


def r_update(so, t1, t2):
    return from_so(*update(so, *to_so(t1, t2)))


def r_energy(so, t1, t2):
    return energy(so, *to_so(t1, t2))


def r_solve(so, tol, max_iter=500):
    e, T1, T2, it = solve(so, tol, max_iter)
    return (e,) + from_so(T1, T2) + (it,)


def converged_reference(so):
    """DIIS-free reference at |dt| < 1e-9 and on to 1e-11: ((e, t1, t2) of the tighter run, delta_e, delta_t), the deltas between the
    two runs being the reference's own convergence uncertainty."""
    e9, T1, T2, _ = solve(so, 1e-9)
    e11, U1, U2, _ = solve(so, 1e-11, T1=T1, T2=T2)
    a9, a11 = from_so(T1, T2), from_so(U1, U2)
    dt = max(np.abs(a9[0] - a11[0]).max(), np.abs(a9[1] - a11[1]).max())
    return (e11,) + a11, abs(e9 - e11), dt


BLOCKS = ("oooo", "ovoo", "ovov", "oovv", "ovvo", "ovvv", "vvvv")


def restricted_blocks(sysm, C, o, pad=0):
    """(fock_mo, blocks) as dmk_rccsd_create takes them, at the orbitals C (columns, the o occupied first): fock_mo = C^T F C (n, n)
    with F the closed-shell Fock matrix of the density of the occupied columns; blocks[name] for oooo, ovoo, ovov, oovv, ovvo, ovvv the
    spatial (pq|rs) row-major in the order of the letters, and vvvv packed on both sides (rows pair(a, c), columns pair(b, d)) with a
    row pitch of npair + pad whose pad columns are NaN (never to be read)."""
    n, v = sysm.n, sysm.n - o
    C = np.asarray(C, dtype=np.float64)
    D = 2.0 * C[:, :o] @ C[:, :o].T
    f = C.T @ (sysm.h1 + sysm.veff_rhf(D)) @ C
    part = {"o": C[:, :o], "v": C[:, o:]}
    blocks = {}
    for name in BLOCKS[:-1]:
        c = [part[x] for x in name]
        blocks[name] = M.transform(sysm, "aa", *c).reshape([x.shape[1] for x in c])
    g = M.pack_cols(M.pack_rows(M.transform(sysm, "aa", *([part["v"]] * 4)), v), v)
    npair = v * (v + 1) // 2
    blocks["vvvv"] = np.full((npair, npair + pad), np.nan)
    blocks["vvvv"][:, :npair] = g
    return f, blocks


def uneven_system(o, v):
    """(system, canonical host orbitals) of the o-occupied, v-virtual case of tests/test_gpu_ccsd_shapes.py: System(o + v, 500 + 37 o
    + v, [o]) and the orbitals of the numpy SCF of tests/scf_ref.py on it."""
    from tests import scf_ref as R
    sysm = R.System(o + v, 500 + 37 * o + v, [o])
    ref = R.scf(sysm.h1[None], sysm.veff_rhf, [o], True)
    assert ref["converged"], (o, v)
    return sysm, ref["mo_coeff"]


def restricted_energy(fock_mo, blocks, t1, t2):
    """2 f_ia t_ia + sum (2 (ia|jb) - (ib|ja)) (t_ij^ab + t_i^a t_j^b) over the blocks of restricted_blocks, plain numpy."""
    o = t1.shape[0]
    g = blocks["ovov"]                                                   # g[i, a, j, b] = (ia|jb)
    tau = t2 + np.einsum("ia,jb->ijab", t1, t1)
    return float(2.0 * np.sum(fock_mo[:o, o:] * t1) + np.einsum("iajb,ijab", 2.0 * g - g.transpose(0, 3, 2, 1), tau))


def random_amplitudes(rng, o, v, scale=0.1):
    """Random restricted amplitudes of the given scale with t_ij^ab = t_ji^ba."""
    t1 = scale * rng.standard_normal((o, v))
    t2 = scale * rng.standard_normal((o, o, v, v))
    return t1, 0.5 * (t2 + t2.transpose(1, 0, 3, 2))


def rotate_ov(C, o, angle=0.05):
    """C with a fixed orthogonal rotation of the given angle that mixes occupied column k with virtual column k (every k that has
    both): non-canonical orbitals with f_ov != 0 and non-diagonal f_oo / f_vv."""
    C = np.array(C, dtype=np.float64)
    n = C.shape[1]
    c, s = np.cos(angle), np.sin(angle)
    for k in range(min(o, n - o)):
        i, a = k, o + k
        ci, ca = C[:, i].copy(), C[:, a].copy()
        C[:, i], C[:, a] = c * ci + s * ca, -s * ci + c * ca
    # a second rotation inside the occupied and inside the virtual space makes f_oo / f_vv non-diagonal where o, v >= 2
    for lo, hi in ((0, o), (o, n)):
        for k in range(lo, hi - 1, 2):
            ci, cj = C[:, k].copy(), C[:, k + 1].copy()
            C[:, k], C[:, k + 1] = c * ci + s * cj, -s * ci + c * cj
    return C


def exact_two_electron_singlet(sysm):
    """Lowest singlet eigenvalue of H = h(1) + h(2) + (pr|qs) in the n^2 space |p alpha, q beta> (AO basis, orthonormal)."""
    n = sysm.n
    eye = np.eye(n)
    g = M.transform(sysm, "aa", eye, eye, eye, eye).reshape(n, n, n, n)          # (pr|qs) at g[p, r, q, s]
    H = np.einsum("pr,qs->pqrs", sysm.h1, eye) + np.einsum("pr,qs->pqrs", eye, sysm.h1) + g.transpose(0, 2, 1, 3)
    w, c = np.linalg.eigh(H.reshape(n * n, n * n))
    for k in range(n * n):
        x = c[:, k].reshape(n, n)
        if np.abs(x - x.T).max() < 1e-8:          # spatially symmetric = singlet
            return float(w[k])
    raise RuntimeError("no singlet state found")
