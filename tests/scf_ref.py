"""
Numpy restatement of embedded Hartree-Fock for the tests of the device solver (tests/test_host_scf.py, tests/test_gpu_scf.py).

Test Hamiltonians are FACTORED, so that the reference J / K never touch the packed 4-fold layout and never need n^4 memory:

    h1           symmetric with a prescribed spectrum: evenly spaced levels of width 1 with a step of 1.5 (a HOMO-LUMO gap >= 1 of
                 the core Hamiltonian) after each filling in `cuts`
    (ij|kl)_aa = lam sum_P A_P[i,j] A_P[k,l]     (ij|kl)_bb = lam sum_P B_P[i,j] B_P[k,l]     (ij|kl)_ab = lam sum_P A_P[i,j] B_P[k,l]
                 A_P, B_P: NAUX = 12 random symmetric n x n matrices, lam = 0.05 / n: a valid 4-fold symmetric, positive ERI
    J[D]       = lam sum_P A_P tr(A_P D)         K[D] = lam sum_P A_P D A_P

SEEDS lists the (kind, n, Sz) cases of the GPU tests with the seed of each; test_host_scf.py asserts for every one of them that the
reference SCF reaches the same energy (<= 1e-12) from the core guess and from a perturbed one and that its converged gap is >= 0.5.
"""
import numpy as np

NAUX = 12

# (kind, n, Sz) -> seed
SEEDS = {
    ("rhf", 6, 0): 11, ("rhf", 65, 0): 12, ("rhf", 129, 0): 13,
    ("uhf", 6, 0): 21, ("uhf", 6, 2): 22, ("uhf", 65, 0): 23, ("uhf", 65, 2): 24,
}


def nelec_of(n):
    """Half filling, rounded down to an even number."""
    return 2 * (n // 2)


def nocc_of(kind, n, Sz):
    ne = nelec_of(n)
    return [ne // 2] if kind == "rhf" else [(ne + Sz) // 2, (ne - Sz) // 2]


def tril_pack(M):
    n = M.shape[-1]
    i, j = np.tril_indices(n)
    return M[..., i, j]


class System(object):
    """One factored test Hamiltonian."""

    def __init__(self, n, seed, cuts):
        rng = np.random.default_rng(seed)
        self.n, self.lam = n, 0.05 / n
        levels = np.linspace(0.0, 1.0, n)
        for c in sorted(set(cuts)):
            levels[c:] += 1.5
        levels -= levels.mean()
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        self.h1 = (q * levels) @ q.T
        self.h1 = 0.5 * (self.h1 + self.h1.T)
        sym = lambda a: 0.5 * (a + a.transpose(0, 2, 1))
        self.A = sym(rng.standard_normal((NAUX, n, n)))
        self.B = sym(rng.standard_normal((NAUX, n, n)))

    def block_s4(self, which):
        """The packed npair x npair block: 'aa', 'bb' or 'ab'."""
        L = {"a": tril_pack(self.A), "b": tril_pack(self.B)}
        return self.lam * (L[which[0]].T @ L[which[1]])

    def blocks_s4(self):
        return np.asarray([self.block_s4(w) for w in ("aa", "bb", "ab")])

    def J(self, which, D):
        """J of block `which` = 'xy': acts on spin x, from a density of spin y."""
        L = {"a": self.A, "b": self.B}
        return self.lam * np.einsum("Pij,P->ij", L[which[0]], np.einsum("Pkl,kl->P", L[which[1]], D))

    def K(self, which, D):
        L = {"a": self.A, "b": self.B}[which[0]]
        Lt = L.transpose(0, 2, 1)
        return self.lam * np.matmul(np.matmul(Lt, D), Lt).sum(axis=0)          # sum_P "ij,il,kl->jk" as two matrix products

    def veff_rhf(self, D, alpha=1.0):
        return self.J("aa", D) - 0.5 * alpha * self.K("aa", D)

    def veff_uhf(self, D, alpha=1.0):
        return np.asarray([self.J("aa", D[0]) + self.J("ab", D[1]) - alpha * self.K("aa", D[0]),
                           self.J("bb", D[1]) + self.J("ba", D[0]) - alpha * self.K("bb", D[1])])


def make_system(kind, n, Sz, seed=None):
    seed = SEEDS[(kind, n, Sz)] if seed is None else seed
    return System(n, seed, nocc_of(kind, n, Sz))


def restore_s1(block, n):
    """4-fold packed block -> (n, n, n, n)."""
    idx = np.zeros((n, n), dtype=np.int64)
    i, j = np.tril_indices(n)
    idx[i, j] = idx[j, i] = np.arange(len(i))
    return block[idx.reshape(-1)][:, idx.reshape(-1)].reshape(n, n, n, n)


def pack_s8(block):
    i, j = np.tril_indices(block.shape[0])
    return block[i, j]


def einsum_jk(eri1, dm):
    """The literal contractions (n <= 6)."""
    return np.einsum("ijkl,kl->ij", eri1, dm), np.einsum("ijkl,il->jk", eri1, dm)


def veff_s1(eri1, D, restricted, alpha=1.0):
    """veff from 1-fold blocks (aa[, bb, ab]): the literal formulas of RHF / UIHF."""
    if restricted:
        j, k = einsum_jk(eri1[0], D)
        return j - 0.5 * alpha * k
    jaa, kaa = einsum_jk(eri1[0], D[0])
    jbb, kbb = einsum_jk(eri1[1], D[1])
    jab = np.einsum("ijkl,kl->ij", eri1[2], D[1])
    jba = np.einsum("ijkl,ij->kl", eri1[2], D[0])
    return np.asarray([jaa + jab - alpha * kaa, jbb + jba - alpha * kbb])


def diis_coeffs_lstsq(errs):
    """Literal statement: minimise |sum_i c_i e_i|_2 under sum_i c_i = 1 (c_last eliminated, least squares for the rest)."""
    e = np.asarray([np.ravel(x) for x in errs])
    m = e.shape[0]
    if m == 1:
        return np.ones(1)
    A = (e[:-1] - e[-1]).T
    z = np.linalg.lstsq(A, -e[-1], rcond=None)[0]
    return np.concatenate([z, [1.0 - z.sum()]])


def _orth(S, n):
    if S is None:
        return np.eye(n)
    w, v = np.linalg.eigh(S)
    return (v / np.sqrt(w)) @ v.T


def scf(h1, veff, nocc, restricted, S=None, dm0=None, H0=0.0, h1_energy=None, tol=1e-13, max_iter=300, diis_dim=8):
    """Plain commutator-DIIS Hartree-Fock.  h1 (ns, n, n); veff(D) with D (n, n) spin-traced for restricted, (2, n, n) else; S None,
    (n, n) or (ns, n, n).  Converged when the energy changes by < tol and max |X^T (F D S - S D F) X| < 1e-11."""
    h1 = np.asarray(h1)
    ns, n = h1.shape[0], h1.shape[-1]
    Ss = [None] * ns if S is None else ([S] * ns if np.ndim(S) == 2 else list(S))
    Xs = [_orth(s, n) for s in Ss]
    occ = 2.0 if restricted else 1.0
    h1_energy = h1 if h1_energy is None else np.asarray(h1_energy)
    shape = (lambda a: a[0]) if restricted else (lambda a: a)

    def eig(F):
        out = []
        for s in range(ns):
            w, c = np.linalg.eigh(Xs[s].T @ F[s] @ Xs[s])
            out.append((w, Xs[s] @ c))
        return out

    def density(wc):
        return np.asarray([occ * wc[s][1][:, :nocc[s]] @ wc[s][1][:, :nocc[s]].T for s in range(ns)])

    def evaluate(D):
        V = np.asarray(veff(shape(D))).reshape(ns, n, n)
        return V, float(np.sum(h1_energy * D) + 0.5 * np.sum(V * D) + H0)

    D = density(eig(h1)) if dm0 is None else np.asarray(dm0, dtype=float).reshape(ns, n, n)
    V, E = evaluate(D)
    Fs, es, converged, it = [], [], False, 0
    for it in range(max_iter):
        F = h1 + V
        err = []
        for s in range(ns):
            fds = F[s] @ D[s] @ (np.eye(n) if Ss[s] is None else Ss[s])
            err.append(Xs[s].T @ (fds - fds.T) @ Xs[s])
        err = np.asarray(err)
        if it > 0 and abs(E - E_prev) < tol and np.abs(err).max() < 1e-11:
            converged = True
            break
        Fs, es = (Fs + [F])[-diis_dim:], (es + [err])[-diis_dim:]
        c = diis_coeffs_lstsq(es)
        D = density(eig(sum(ci * Fi for ci, Fi in zip(c, Fs))))
        E_prev = E
        V, E = evaluate(D)
    F = h1 + V
    wc = eig(F)
    gap = min(wc[s][0][nocc[s]] - wc[s][0][nocc[s] - 1] for s in range(ns) if 0 < nocc[s] < n)
    return {"E": E, "D": shape(D), "F": shape(F), "V": shape(V), "mo_energy": shape(np.asarray([x[0] for x in wc])),
            "mo_coeff": shape(np.asarray([x[1] for x in wc])), "gap": float(gap), "converged": converged, "iterations": it}


def run_case(kind, n, Sz, dm0=None, alpha=1.0, S=None, seed=None, **kw):
    """The reference solution of one listed case."""
    sysm = make_system(kind, n, Sz, seed)
    nocc = nocc_of(kind, n, Sz)
    if kind == "rhf":
        out = scf(sysm.h1[None], lambda D: sysm.veff_rhf(D, alpha), nocc, True, S=S, dm0=dm0, **kw)
    else:
        out = scf(np.asarray([sysm.h1, sysm.h1]), lambda D: sysm.veff_uhf(D, alpha), nocc, False, S=S, dm0=dm0, **kw)
    out["system"], out["nocc"] = sysm, nocc
    return out


def core_guess(kind, n, Sz, seed=None):
    sysm = make_system(kind, n, Sz, seed)
    w, c = np.linalg.eigh(sysm.h1)
    occ = 2.0 if kind == "rhf" else 1.0
    D = np.asarray([occ * c[:, :k] @ c[:, :k].T for k in nocc_of(kind, n, Sz)])
    return D[0] if kind == "rhf" else D
