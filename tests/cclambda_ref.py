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
    lambda_step_reverse / rdm1_reverse / grad_t_reverse   the same derivatives in REVERSE MODE: one backward pass of float64 CPU torch
                                     autograd through the same update (ccsd_ref.torch_namespace) gives a whole gradient at any shape
    lambda_run_ref / diis_coeffs_ref the iteration of dmk_rccsd_lambda_run (ring, DIIS weights as the header documents them) over the
                                     reference sweep: how many sweeps a ring needs; run_loop_start / coupled_system: its test system
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


energy_c = CR.energy_of          # ccsd_ref.energy without the cast to float


def residual(so, T1, T2, xp=CR.NP):
    """r = d (update(T) - T): the projected residual, zero at convergence."""
    N1, N2 = CR.update(so, T1, T2, xp)
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


# ---- reverse mode ----------------------------------------------------------------------------------------------------------------
_SO_ARRAYS = ("foo", "fov", "fvv", "eo", "ev", "oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv")


def _torch_so(so, f_mo=None):
    """(torch, namespace, copy of `so` over float64 CPU tensors).  f_mo: a tensor that replaces the Fock matrix as with_fock does,
    every Fock block derived from it inside the graph."""
    import torch
    s2 = copy.copy(so)
    for name in _SO_ARRAYS:
        setattr(s2, name, torch.from_numpy(np.ascontiguousarray(getattr(so, name), dtype=np.float64)))
    if f_mo is not None:
        o = so.o
        two = lambda a: torch.kron(torch.eye(2, dtype=torch.float64), a)
        s2.foo, s2.fov, s2.fvv = two(f_mo[:o, :o]), two(f_mo[:o, o:]), two(f_mo[o:, o:])
        s2.eo, s2.ev = torch.diag(s2.foo), torch.diag(s2.fvv)
        s2.f_mo = f_mo
    return torch, CR.torch_namespace(), s2


def _lagrangian_t(torch, xp, st, T1, T2, l1, l2):
    """The spin-orbital L = E(T) + sum Lam1 r1 + 1/4 sum Lam2 r2 with Lam = to_so(l) as a 0-d tensor, and the denominators."""
    Lam1, Lam2 = (torch.from_numpy(x) for x in CR.to_so(np.asarray(l1, dtype=np.float64), np.asarray(l2, dtype=np.float64)))
    r1, r2 = residual(st, T1, T2, xp)
    d1 = st.eo[:, None] - st.ev[None, :]
    d2 = d1[:, None, :, None] + d1[None, :, None, :]
    return CR.energy_of(st, T1, T2, xp) + torch.sum(Lam1 * r1) + 0.25 * torch.sum(Lam2 * r2), Lam1, Lam2, d1, d2


def _grad_t(so, t1, t2, l1, l2):
    """dL/dT over the FULL spin-orbital tensors (every element an independent leaf), the doubles part antisymmetrised onto the
    unique amplitudes:  -> (L, G1, G2a, Lam1, Lam2, d1, d2) as numpy."""
    torch, xp, st = _torch_so(so)
    T1, T2 = (torch.from_numpy(x).requires_grad_(True) for x in CR.to_so(np.asarray(t1, dtype=np.float64), np.asarray(t2, dtype=np.float64)))
    L, Lam1, Lam2, d1, d2 = _lagrangian_t(torch, xp, st, T1, T2, l1, l2)
    L.backward()
    G1, G2 = T1.grad.numpy(), T2.grad.numpy()
    G2a = G2 - G2.transpose(1, 0, 2, 3) - G2.transpose(0, 1, 3, 2) + G2.transpose(1, 0, 3, 2)
    return float(L.detach()), G1, G2a, Lam1.numpy(), Lam2.numpy(), d1.numpy(), d2.numpy()


def lambda_step_reverse(so, t1, t2, l1, l2):
    """ONE sweep of the Lambda equations on restricted amplitudes, (l1new, l2new) = from_so(Lam + (dL/dT) / d): the Jacobi step on
    the stationarity condition dL/dT = 0 with the Fock-diagonal denominators (d Lam_new = g + (J + diag d)^T Lam in the notation of
    lambda_by_jacobian, since dL/dx = g + J^T Lam)."""
    _, G1, G2a, Lam1, Lam2, d1, d2 = _grad_t(so, t1, t2, l1, l2)
    return CR.from_so(Lam1 + G1 / d1, Lam2 + G2a / d2)


def grad_t_reverse(so, t1, t2, l1, l2):
    """(L, dL/dT1 (O, V), dL/dT2 over the unique amplitudes spread antisymmetrically (O, O, V, V)) in spin orbitals: zero at the
    solution of the Lambda equations."""
    return _grad_t(so, t1, t2, l1, l2)[:3]


def rdm1_reverse(so, t1, t2, l1, l2):
    """gamma (n, n) = sym(dL/df) + 2 on the occupied diagonal for ANY (t, l): the Fock matrix is the leaf, its blocks and the
    denominators derived from it as with_fock does."""
    import torch
    f = torch.from_numpy(np.array(so.f_mo, dtype=np.float64)).requires_grad_(True)
    torch, xp, st = _torch_so(so, f)
    T1, T2 = (torch.from_numpy(x) for x in CR.to_so(np.asarray(t1, dtype=np.float64), np.asarray(t2, dtype=np.float64)))
    _lagrangian_t(torch, xp, st, T1, T2, l1, l2)[0].backward()
    G = f.grad.numpy()
    gam = 0.5 * (G + G.T)
    gam[:so.o, :so.o] += 2.0 * np.eye(so.o)
    return gam


def diis_coeffs_ref(B):
    """The DIIS weights as include/libdmetk.h documents them for dmk_diis_coeffs, in numpy: the Gram matrix scaled to a unit largest
    diagonal, bordered with ones, pseudo-inverted on (0, ..., 0, 1) with the directions of |w| <= 1e-13 dropped, normalised."""
    m = B.shape[0]
    A = np.zeros((m + 1, m + 1))
    A[:m, :m] = 0.5 * (B + B.T) / np.abs(np.diag(B)).max()
    A[m, :m] = A[:m, m] = 1.0
    w, V = np.linalg.eigh(A)
    keep = np.abs(w) > 1e-13
    c = (V[:m, keep] * (V[m, keep] / w[keep])).sum(axis=1)
    return c / c.sum()


def lambda_run_ref(so, t1, t2, l1, l2, ring, tol, max_iter=200):
    """The iteration of dmk_rccsd_lambda_run over the REFERENCE sweep (lambda_step_reverse): a ring of `ring` (sweep, step) pairs,
    the newest overwriting the oldest, the next l their DIIS combination; ring = 0: plain sweeping.  Converged when the 2-norm of a
    step is below tol; the l kept is then that sweep's.  -> (l1, l2, sweeps, |dl|), sweeps = -1 when max_iter did not suffice."""
    o, v = t1.shape
    split = lambda x: (x[:o * v].reshape(o, v), x[o * v:].reshape(o, o, v, v))
    x = np.concatenate([np.ravel(l1), np.ravel(l2)])
    X, E, dl = [], [], np.inf
    for it in range(1, max_iter + 1):
        new = np.concatenate([np.ravel(a) for a in lambda_step_reverse(so, t1, t2, *split(x))])
        step = new - x
        dl = float(np.sqrt(np.sum(step ** 2)))
        if dl < tol or not ring:
            x = new
            if dl < tol:
                return split(x) + (it, dl)
            continue
        if len(X) < ring:
            X.append(new)
            E.append(step)
        else:
            X[(it - 1) % ring], E[(it - 1) % ring] = new, step
        x = diis_coeffs_ref(np.array(E) @ np.array(E).T) @ np.array(X)
    return split(x) + (-1, dl)


def run_loop_start(o, v):
    """The l the ring tests of tests/test_gpu_cclambda_shapes.py start from: random, symmetric, of scale 0.1 like every other l of
    that file.  (From l = t the run-loop system is 2.5e-4 from its solution and a ring of 12 converges in 9 sweeps, before it is
    full; tests/test_host_cclambda.py pins both counts over the reference sweep.)"""
    return CR.random_amplitudes(np.random.default_rng(21), o, v)


def coupled_system(o, v, scale):
    """(system, canonical host orbitals) of ccsd_ref.uneven_system with the coupling `lam` multiplied by `scale` BEFORE the numpy
    SCF: the system of the run-loop tests of tests/test_gpu_cclambda_shapes.py at (2, 3), scale 2.0 (l differs from t by 1e-4)."""
    from tests import scf_ref as R
    sysm = R.System(o + v, 500 + 37 * o + v, [o])
    sysm.lam *= scale
    ref = R.scf(sysm.h1[None], sysm.veff_rhf, [o], True)
    assert ref["converged"], (o, v, scale)
    return sysm, ref["mo_coeff"]


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
