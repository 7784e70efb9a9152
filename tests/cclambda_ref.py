"""
Reference for the Lambda equations, the one-particle density and the expectation value of restricted CCSD (the Lambda
subsection), built ONLY on the spin-orbital amplitude equations of tests/ccsd_ref.py: there are no hand-written Lambda equations here.

The spin-orbital Lagrangian is  L = E(T) + sum_ia L1_ia r1_ia + 1/4 sum_ijab L2_ijab r2_ijab  with the projected residual
r = d (update(T) - T) (d the Fock-diagonal denominators: r is the residual without any division).  Everything is a derivative of L,
taken by COMPLEX STEP: the equations are polynomial in T and linear in the Hamiltonian, so f(x + i h).imag / h is exact to rounding
for h = 1e-30.

    lambda_by_jacobian(so, T1, T2)   J = dr/dx and g = dE/dx over x = (T1, the unique T2: i < j, a < b); solves J^T lam = -g and
                                     returns the restricted (l1, l2) = from_so(lam)
    lagrangian(so, t1, t2, l1, l2)   E_corr + 2 l1 . r1 + (2 l2 - l2^T(ab)) . r2 on restricted amplitudes (complex-capable)
    stationarity(...)                d/d eps of that along a symmetric direction (delta1, delta2), complex step
    rdm1_by_derivative(so, t, l)     dL/df_pq over symmetric unit perturbations of the Fock matrix, plus 2 on the occupied diagonal
    rdm1_explicit(t1, t2, l1, l2)    the closed-shell formulas of the density (the ones the device evaluates), plain numpy
    expval_ref(...)                  H0' + E_HF' + L(t, l; f', g') of another Hamiltonian over the same orbitals
    fci_two_electron(sysm)           (E, X): the singlet ground vector of the n^2 problem; gamma_AO = 2 X X^T, <H'> = X^T H' X
    two_electron_matrix(sysm)        the n^2 x n^2 Hamiltonian of fci_two_electron
"""
import copy

import numpy as np

from tests import ccsd_ref as CR
from tests import mp2_ref as M

ES = CR.ES
STEP = 1e-30


def to_so_c(t1, t2):
    """ccsd_ref.to_so for real or complex amplitudes (that one allocates a real array)."""
    o, v = t1.shape
    T1 = np.kron(np.eye(2), t1)
    T2 = np.zeros((2 * o, 2 * o, 2 * v, 2 * v), dtype=np.result_type(t1, t2))
    a, b = slice(0, o), slice(o, 2 * o)
    A, B = slice(0, v), slice(v, 2 * v)
    same = t2 - t2.transpose(0, 1, 3, 2)
    T2[a, a, A, A] = T2[b, b, B, B] = same
    T2[a, b, A, B] = T2[b, a, B, A] = t2
    T2[a, b, B, A] = T2[b, a, A, B] = -t2.transpose(0, 1, 3, 2)
    return T1, T2


def energy_c(so, T1, T2):
    """ccsd_ref.energy without the cast to float."""
    return ES("ia,ia", so.fov, T1) + 0.25 * ES("ijab,ijab", so.oovv, T2) + 0.5 * ES("ijab,ia,jb", so.oovv, T1, T1)


def residual(so, T1, T2):
    """r = d (update(T) - T): the projected residual, zero at convergence."""
    N1, N2 = CR.update(so, T1, T2)
    d1 = so.eo[:, None] - so.ev[None, :]
    d2 = d1[:, None, :, None] + d1[None, :, None, :]
    return d1 * (N1 - T1), d2 * (N2 - T2)


def _pairs(n):
    return np.triu_indices(n, 1)


def _pack(T1, T2):
    O, V = T1.shape
    i, j = _pairs(O)
    a, b = _pairs(V)
    return np.concatenate([T1.ravel(), T2[i[:, None], j[:, None], a[None, :], b[None, :]].ravel()])


def _unpack(x, O, V):
    i, j = _pairs(O)
    a, b = _pairs(V)
    T1 = x[:O * V].reshape(O, V)
    u = x[O * V:].reshape(len(i), len(a))
    T2 = np.zeros((O, O, V, V), dtype=x.dtype)
    T2[i[:, None], j[:, None], a[None, :], b[None, :]] = u
    T2[j[:, None], i[:, None], a[None, :], b[None, :]] = -u
    T2[i[:, None], j[:, None], b[None, :], a[None, :]] = -u
    T2[j[:, None], i[:, None], b[None, :], a[None, :]] = u
    return T1, T2


def jacobian(so, T1, T2):
    """(J, g): J[m, k] = d r_m / d x_k and g[k] = dE / dx_k over the unique spin-orbital amplitudes x, by complex step."""
    O, V = T1.shape
    x0 = _pack(T1, T2).astype(np.complex128)
    nx = x0.size
    J, g = np.empty((nx, nx)), np.empty(nx)
    for k in range(nx):
        x = x0.copy()
        x[k] += 1j * STEP
        U1, U2 = _unpack(x, O, V)
        J[:, k] = _pack(*residual(so, U1, U2)).imag / STEP
        g[k] = energy_c(so, U1, U2).imag / STEP
    return J, g


def lambda_by_jacobian(so, T1, T2, full=False):
    """The restricted (l1, l2) that make L stationary at the spin-orbital amplitudes (T1, T2); full=True: also (J, g, Lam1, Lam2)."""
    O, V = T1.shape
    J, g = jacobian(so, T1, T2)
    lam = np.linalg.solve(J.T, -g)
    L1, L2 = _unpack(lam, O, V)
    l1, l2 = CR.from_so(L1, L2)
    return (l1, l2, J, g, L1, L2) if full else (l1, l2)


def tilde(l1, l2):
    """The weights of the restricted Lagrangian: (2 l1, 2 l2 - l2^T(ab))."""
    return 2.0 * l1, 2.0 * l2 - l2.transpose(0, 1, 3, 2)


def untilde(w1, w2):
    return 0.5 * w1, (2.0 * w2 + w2.transpose(0, 1, 3, 2)) / 3.0


def r_residual(so, t1, t2):
    return CR.from_so(*residual(so, *to_so_c(t1, t2)))


def lagrangian(so, t1, t2, l1, l2):
    """E_corr(t) + 2 l1 . r1(t) + (2 l2 - l2^T(ab)) . r2(t) of restricted amplitudes (real or complex t)."""
    T1, T2 = to_so_c(t1, t2)
    r1, r2 = CR.from_so(*residual(so, T1, T2))
    w1, w2 = tilde(l1, l2)
    return energy_c(so, T1, T2) + np.sum(w1 * r1) + np.sum(w2 * r2)


def stationarity(so, t1, t2, l1, l2, delta1, delta2):
    """d/d eps L(t + eps delta, l) at eps = 0 for a direction with delta2_ijab = delta2_jiba."""
    assert np.abs(delta2 - delta2.transpose(1, 0, 3, 2)).max() <= 1e-14
    return float(lagrangian(so, t1 + 1j * STEP * delta1, t2 + 1j * STEP * delta2, l1, l2).imag / STEP)


def with_fock(so, f_mo):
    """A copy of the spin-orbital Hamiltonian `so` whose Fock matrix is f_mo (n, n; real or complex), the integrals shared."""
    o = so.o
    s2 = copy.copy(so)
    two = lambda a: np.kron(np.eye(2), a)
    s2.foo, s2.fov, s2.fvv = two(f_mo[:o, :o]), two(f_mo[:o, o:]), two(f_mo[o:, o:])
    s2.eo, s2.ev = np.diag(s2.foo).copy(), np.diag(s2.fvv).copy()
    s2.f_mo = f_mo
    return s2


def rdm1_by_derivative(so, t1, t2, l1, l2):
    """gamma_pq = dL/df_pq (MO basis, [occ | vir], spin-summed, symmetric) + 2 on the occupied diagonal.  For p != q the
    perturbation is the symmetric unit E_pq + E_qp, whose derivative is gamma_pq + gamma_qp = 2 gamma_pq."""
    n, o = so.o + so.v, so.o
    gam = np.zeros((n, n))
    for p in range(n):
        for q in range(p, n):
            V = np.zeros((n, n), dtype=np.complex128)
            V[p, q] = V[q, p] = 1j * STEP
            d = lagrangian(with_fock(so, so.f_mo + V), t1, t2, l1, l2).imag / STEP
            gam[p, q] = gam[q, p] = d if p == q else 0.5 * d
    gam[:o, :o] += 2.0 * np.eye(o)
    return gam


def rdm1_explicit(t1, t2, l1, l2):
    """The closed-shell CCSD one-particle density in the MO basis ([occ | vir], spin-summed), from the amplitudes."""
    o, v = t1.shape
    th = 2.0 * t2 - t2.transpose(0, 1, 3, 2)
    doo = -ES("ja,ia->ij", t1, l1) - ES("jkab,ikab->ij", th, l2)
    dvv = ES("ia,ib->ab", t1, l1) + ES("jica,jicb->ab", th, l2)
    xt1 = ES("mnef,inef->mi", l2, th)
    xt2 = ES("mnaf,mnef->ea", l2, th)
    dvo = t1.T - ES("ie,me,ma->ai", t1, l1, t1) + ES("imae,me->ai", th, l1) - ES("mi,ma->ai", xt1, t1) - ES("ie,ae->ai", t1, xt2)
    dov = l1
    gam = np.zeros((o + v, o + v))
    gam[:o, :o] = doo + doo.T + 2.0 * np.eye(o)
    gam[:o, o:] = dov + dvo.T
    gam[o:, :o] = gam[:o, o:].T
    gam[o:, o:] = dvv + dvv.T
    return gam


def expval_ref(sysm2, H0, C, o, t1, t2, l1, l2):
    """H0 + E_HF' + E_corr(t; f', g') + <l~, r(t; f', g')> of the Hamiltonian of `sysm2` at the orbitals C (o occupied columns first)
    of ANOTHER system's Hartree-Fock state: f' = C^T (h1' + veff'[D_HF]) C."""
    C = np.asarray(C, dtype=np.float64)
    D = 2.0 * C[:, :o] @ C[:, :o].T
    veff = sysm2.veff_rhf(D)
    so2 = CR.spin_orbital(sysm2, C, o, fock_ao=sysm2.h1 + veff)
    e_hf = float(np.sum(D * (sysm2.h1 + 0.5 * veff)))
    return H0 + e_hf + float(lagrangian(so2, t1, t2, l1, l2))


def two_electron_matrix(sysm):
    """H = h(1) + h(2) + (pr|qs) in the n^2 space |p alpha, q beta> (AO basis, orthonormal), as an (n^2, n^2) matrix."""
    n = sysm.n
    eye = np.eye(n)
    g = M.transform(sysm, "aa", eye, eye, eye, eye).reshape(n, n, n, n)
    H = np.einsum("pr,qs->pqrs", sysm.h1, eye) + np.einsum("pr,qs->pqrs", eye, sysm.h1) + g.transpose(0, 2, 1, 3)
    return H.reshape(n * n, n * n)


def fci_two_electron(sysm):
    """(E, X): the lowest singlet of the two-electron problem, X (n, n) symmetric with |X|_F = 1."""
    n = sysm.n
    w, c = np.linalg.eigh(two_electron_matrix(sysm))
    for k in range(n * n):
        x = c[:, k].reshape(n, n)
        if np.abs(x - x.T).max() < 1e-8:
            return float(w[k]), x
    raise RuntimeError("no singlet state found")


def solve_lambda_ref(so, t1, t2):
    """(l1, l2) of the restricted amplitudes (t1, t2) through the Jacobian."""
    return lambda_by_jacobian(so, *CR.to_so(t1, t2))
