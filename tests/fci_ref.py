"""
Numpy reference of full configuration interaction for the tests of the device solver (tests/test_host_fci.py, tests/test_gpu_fci.py,
tests/test_gpu_fci_edges.py).

No link tables: creation and annihilation operators act on bit masks over ONE spin-orbital order (alpha orbitals 0 .. n-1, then beta
orbitals n .. 2n-1) with Jordan-Wigner signs; the basis state of a mask is prod_{i in mask, ascending} a+_i |0>, which is the device's
|Ia Ib> = prod_{p in Ia} a+_p,alpha prod_{q in Ib} a+_q,beta |0>.  Determinant index = index(Ia) * Nb + index(Ib), strings ordered by
integer value.

    H = sum_PQ k_PQ a+_P a_Q + 1/2 sum_PQRS G_PQRS a+_P a_Q a+_R a_S       (P, Q of one spin; R, S of one spin)
    k^s_pq = h^s_pq - 1/2 sum_r g^ss_prrq,      G = g^{spin(P) spin(R)}_pqrs,   g^ba_pqrs = g^ab_rspq

`Space.matvec` evaluates H c by applying a+_R a_S to the whole vector for every pair, contracting with G, and applying a+_P a_Q;
with absolute=True the same routine runs with |k|, |G|, |c| and every sign +, which gives the |terms| sum of every element: the scale
of the rounding-error bounds of the GPU tests.  Densities: gamma^s_pq = <p+ q>, dm2[p, q, r, s] = <p+ r+ s q>.

`Solvable`: a Hamiltonian of commuting terms with a closed-form spectrum and ground vector, for spaces too large for a reference
eigen-solve.  `davidson`: the device's Davidson loop restated step by step, for iteration counts and flags.
"""
import functools
import itertools

import numpy as np

from tests import scf_ref as R


class Space(object):
    def __init__(self, n, na, nb):
        self.n, self.na, self.nb = n, na, nb
        self.sa = np.array(sorted(sum(1 << i for i in s) for s in itertools.combinations(range(n), na)), dtype=np.int64)
        self.sb = np.array(sorted(sum(1 << i for i in s) for s in itertools.combinations(range(n), nb)), dtype=np.int64)
        self.Na, self.Nb = len(self.sa), len(self.sb)
        self.ndet = self.Na * self.Nb
        # spin-orbital masks of all determinants in the order of the vector
        self.masks = (self.sa[:, None] | (self.sb[None, :] << n)).reshape(-1)
        self.order = np.argsort(self.masks, kind="stable")
        self.sorted_masks = self.masks[self.order]
        self._memo = {}

    # ---- operators on bit masks ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _below(masks, i):
        """parity of the occupied spin orbitals below i"""
        x = masks & ((1 << i) - 1)
        par = np.zeros_like(x)
        while np.any(x):
            par ^= x & 1
            x = x >> 1
        return par

    def annihilate(self, masks, sign, i):
        ok = (masks >> i) & 1 == 1
        s = np.where(self._below(masks, i) == 1, -sign, sign)
        return np.where(ok, masks & ~(1 << i), masks), np.where(ok, s, 0)

    def create(self, masks, sign, i):
        ok = (masks >> i) & 1 == 0
        s = np.where(self._below(masks, i) == 1, -sign, sign)
        return np.where(ok, masks | (1 << i), masks), np.where(ok, s, 0)

    def apply(self, ops, vec, absolute=False):
        """(prod ops) vec, ops = [('c' | 'a', spin orbital), ...] applied right to left, on a vector over this space; the image must
        lie in the space again (particle numbers per spin conserved) or vanish."""
        key = tuple(ops)
        if key not in self._memo:          # the image of every basis state under this product: computed once, by the bit operations
            m, s = self.masks.copy(), np.ones(self.ndet, dtype=np.int64)
            for kind, i in reversed(ops):
                m, s = (self.create if kind == "c" else self.annihilate)(m, s, i)
            live = np.nonzero(s)[0]
            pos = np.searchsorted(self.sorted_masks, m[live])
            assert np.array_equal(self.sorted_masks[pos], m[live]), "operator product leaves the space"
            if len(self._memo) > 4096:
                self._memo.clear()
            self._memo[key] = (live, self.order[pos], s[live].astype(np.float64))
        live, tgt, sgn = self._memo[key]
        vec = np.asarray(vec, dtype=np.float64)
        out = np.zeros(vec.shape)
        if len(live):                      # a product of operators maps distinct basis states to distinct basis states
            w = np.ones_like(sgn) if absolute else sgn
            out[tgt] = vec[live] * (w if vec.ndim == 1 else w[:, None])
        return out

    def pairs(self):
        """the spin-conserving pairs (P, Q) in the order (spin, p, q)"""
        n = self.n
        return [(s * n + p, s * n + q) for s in range(2) for p in range(n) for q in range(n)]

    def excited(self, vec, absolute=False):
        """X[(s, p, q)] = a+_P a_Q vec, (2 n^2, ndet)"""
        return np.asarray([self.apply([("c", P), ("a", Q)], vec, absolute) for P, Q in self.pairs()])

    # ---- Hamiltonian ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def supermatrix(h1, eri):
        """(k (2 n^2), G (2 n^2, 2 n^2)) of h1 (2, n, n) and eri = (aa, ab, bb)."""
        n = h1.shape[-1]
        gaa, gab, gbb = [np.asarray(g).reshape(n * n, n * n) for g in eri]
        k = np.concatenate([(h1[0] - 0.5 * np.einsum("prrq->pq", eri[0])).reshape(-1), (h1[1] - 0.5 * np.einsum("prrq->pq", eri[2])).reshape(-1)])
        G = np.block([[gaa, gab], [gab.T, gbb]])
        return k, G

    def matvec(self, h1, eri, vec, absolute=False):
        """H vec (without H0); vec (ndet) or (ndet, k) columns"""
        vec = np.asarray(vec, dtype=np.float64)
        k, G = self.supermatrix(h1, eri)
        if absolute:
            k, G, vec = np.abs(k), np.abs(G), np.abs(vec)
        X = self.excited(vec, absolute)
        Y = k.reshape((-1,) + (1,) * vec.ndim) * vec[None] + 0.5 * np.tensordot(G, X, 1)
        out = np.zeros(vec.shape)
        for (P, Q), y in zip(self.pairs(), Y):
            out += self.apply([("c", P), ("a", Q)], y, absolute)
        return out

    def dense(self, h1, eri):
        H = self.matvec(h1, eri, np.eye(self.ndet))
        assert np.abs(H - H.T).max() <= 1e-12 * max(1.0, np.abs(H).max())
        return 0.5 * (H + H.T)

    def hdiag(self, h1, eri):
        """H_II by the occupation-number formula."""
        n = self.n
        occ = lambda strs: np.asarray([[(s >> p) & 1 for p in range(n)] for s in strs], dtype=np.float64)
        oa, ob = occ(self.sa), occ(self.sb)
        J = lambda g: np.einsum("ppqq->pq", g)
        K = lambda g: np.einsum("pqqp->pq", g)
        ea = oa @ np.diag(h1[0]) + 0.5 * np.einsum("ip,pq,iq->i", oa, J(eri[0]) - K(eri[0]), oa)
        eb = ob @ np.diag(h1[1]) + 0.5 * np.einsum("ip,pq,iq->i", ob, J(eri[2]) - K(eri[2]), ob)
        return (ea[:, None] + eb[None, :] + oa @ J(eri[1]) @ ob.T).reshape(-1)

    # ---- densities -----------------------------------------------------------------------------------------------------------------
    def rdm1(self, vec, absolute=False):
        """gamma (2, n, n), gamma^s_pq = <p+_s q_s>"""
        n = self.n
        v = np.abs(vec) if absolute else vec
        return (self.excited(v, absolute) @ v).reshape(2, n, n)

    def rdm2(self, vec, absolute=False):
        """(aa, ab, bb), each dm2[p, q, r, s] = <p+ r+ s q> = <E_pq E_rs> - delta_qr delta_spin <E_ps>; <E_pq E_rs> = (E_qp c) . (E_rs c).
        absolute: the sum of the absolute values of all terms (the delta term added)."""
        n = self.n
        v = np.abs(vec) if absolute else vec
        X = self.excited(v, absolute).reshape(2, n, n, self.ndet)
        g1 = (X.reshape(2 * n * n, -1) @ v).reshape(2, n, n)
        out = []
        for s, t in ((0, 0), (0, 1), (1, 1)):
            # sum_I X^s[q, p, I] X^t[r, s, I] as ONE matrix product [(q p), I] [I, (r s)] (the same sums as the einsum over I, at the
            # speed of a product: 9 s -> 0.2 s at 75075 determinants), then q <-> p
            d = (X[s].reshape(n * n, -1) @ X[t].reshape(n * n, -1).T).reshape(n, n, n, n).transpose(1, 0, 2, 3)
            if s == t:
                corr = np.einsum("qr,ps->pqrs", np.eye(n), g1[s])
                d = d + corr if absolute else d - corr
            out.append(d)
        return np.asarray(out)

    def rdm2_direct(self, vec):
        """the same three blocks by applying the four operators one after the other (small n only)."""
        n = self.n
        out = np.zeros((3, n, n, n, n))
        for b, (s, t) in enumerate(((0, 0), (0, 1), (1, 1))):
            for p, q, r, u in itertools.product(range(n), repeat=4):
                ops = [("c", s * n + p), ("c", t * n + r), ("a", t * n + u), ("a", s * n + q)]
                out[b, p, q, r, u] = vec @ self.apply(ops, vec)
        return out


def spin_summed(dm2):
    """aa + ab + ba + bb of the three blocks aa, ab, bb: ba[p, q, r, s] = ab[r, s, p, q]"""
    return dm2[0] + dm2[1] + dm2[1].transpose(2, 3, 0, 1) + dm2[2]


def energy_from_rdm(h1, eri, g1, dm2, h0=0.0):
    """H0 + sum h g + 1/2 sum_st g^st_pqrs dm2^st_pqrs"""
    e = h0 + np.sum(h1[0] * g1[0]) + np.sum(h1[1] * g1[1])
    return float(e + 0.5 * np.sum(eri[0] * dm2[0]) + np.sum(eri[1] * dm2[1]) + 0.5 * np.sum(eri[2] * dm2[2]))


# ---- test Hamiltonians ----------------------------------------------------------------------------------------------------------------
def hubbard_ring(n, U, field=0.0):
    """(h1 (2, n, n), (aa, ab, bb)) of the periodic Hubbard ring with hopping 1; `field`: a staggered, spin-dependent site energy
    +-field (-1)^i that breaks the translational and spin symmetry (lifts degeneracies)."""
    t = np.zeros((n, n))
    for i in range(n):
        t[i, (i + 1) % n] -= 1.0
        t[(i + 1) % n, i] -= 1.0
    if n == 2:
        t *= 0.5
    st = np.diag(field * (-1.0) ** np.arange(n))
    g = np.zeros((n, n, n, n))
    for i in range(n):
        g[i, i, i, i] = U
    return np.asarray([t + st, t - st]), (g, g.copy(), g.copy())


def factored(n, seed, unrestricted, scale=4.0):
    """(h1 (2, n, n), (aa, ab, bb)) of scf_ref.System (the factored test Hamiltonian) in its own orthonormal basis, the two-electron part
    made `scale` times stronger (correlation that a mean field misses); restricted: the A factors serve both spins."""
    sysm = R.System(n, seed, [n // 2])
    lam = sysm.lam * scale
    A, B = sysm.A, (sysm.B if unrestricted else sysm.A)
    gaa = lam * np.einsum("Pij,Pkl->ijkl", A, A)
    gab = lam * np.einsum("Pij,Pkl->ijkl", A, B)
    gbb = lam * np.einsum("Pij,Pkl->ijkl", B, B)
    h1b = sysm.h1 + (0.1 * B[0] if unrestricted else 0.0)
    return np.asarray([sysm.h1, h1b]), (gaa, gab, gbb)


def to_basis(h1, eri, C):
    """the integrals in the orthonormal orbitals C (columns), the same for both spins"""
    t4 = lambda g: np.einsum("ijkl,ip,jq,kr,ls->pqrs", g, C, C, C, C, optimize=True)
    return np.asarray([C.T @ h1[0] @ C, C.T @ h1[1] @ C]), tuple(t4(g) for g in eri)


# name -> (kind, n, na, nb, spin, parameter): the converged-solver cases of tests/test_gpu_fci.py.  All in the eigenbasis of the alpha
# one-body matrix (the device solver is used behind a mean field: a diagonally dominant H, a single-determinant start).
# tests/test_host_fci.py asserts for every one that the gap above the ground state is >= 1e-2.
SOLVER_CASES = {
    "sys4": ("factored", 4, 2, 2, 1, 31), "sys6": ("factored", 6, 3, 3, 1, 32), "sys6u": ("factored", 6, 4, 2, 2, 33),
    "sys8": ("factored", 8, 4, 4, 1, 34),
    "ring6": ("ring", 6, 3, 3, 1, 4.0), "ring6u": ("ring", 6, 3, 3, 2, 8.0), "ring8": ("ring", 8, 4, 4, 1, 4.0), "ring8u": ("ring", 8, 4, 4, 2, 8.0),
}
RING_FIELD = 0.25          # the symmetry-breaking staggered field of the unrestricted rings


@functools.lru_cache(maxsize=None)
def solver_case(name):
    """(Space, h1 (2, n, n), (aa, ab, bb), H0, E0, gap, c0): the reference ground state, by dense eigh up to 400 determinants and by
    scipy's eigsh over `matvec` above.  Shared by the tests, never modified."""
    kind, n, na, nb, spin, par = SOLVER_CASES[name]
    if kind == "factored":
        h1, eri = factored(n, par, spin == 2)
    else:
        h1, eri = hubbard_ring(n, par, RING_FIELD if spin == 2 else 0.0)
    h1, eri = to_basis(h1, eri, np.linalg.eigh(h1[0])[1])
    sp = Space(n, na, nb)
    if sp.ndet <= 400:
        w, v = np.linalg.eigh(sp.dense(h1, eri))
    else:
        from scipy.sparse.linalg import LinearOperator, eigsh
        op = LinearOperator((sp.ndet, sp.ndet), matvec=lambda x: sp.matvec(h1, eri, np.asarray(x).reshape(-1)), dtype=np.float64)
        w, v = eigsh(op, k=3, which="SA", tol=1e-13, ncv=40, v0=np.random.default_rng(5).standard_normal(sp.ndet))
        o = np.argsort(w)
        w, v = w[o], v[:, o]
    return sp, h1, eri, 0.25 * n, float(w[0]), float(w[1] - w[0]), v[:, 0]


# ---- an exactly solvable Hamiltonian (spaces too large for a reference eigen-solve) ---------------------------------------------------
class Solvable(object):
    """h_s = U_s diag(eps_s) U_s^T with U_s = expm(antisymmetric), g^st_pqrs = lam (h_s)_pq (h_t)_rs.  Then

        H = H1 + lam / 2 H1^2 - lam / 2 sum_s (h_s^2)^,        H1 = sum_s sum_pq (h_s)_pq Es_pq,

    and every term commutes: in the orbitals U_s the eigenstates are occupation patterns, of energy e + lam / 2 e^2 - lam / 2 sum eps_i^2
    with e = sum eps_i over the occupied spin orbitals.  The ground vector in the string basis is the outer product of two Slater
    determinants (the minors of U_s over the occupied columns), its one-particle density U_s occ U_s^T."""

    def __init__(self, n, na, nb, unrestricted, seed=11, rot=0.08, lam=0.1, spread=0.05, split=0.04):
        from scipy.linalg import expm
        rng = np.random.default_rng(seed)
        self.n, self.na, self.nb, self.lam, self._memo_ob = n, na, nb, lam, {}
        ea = np.arange(n) - n // 2 + spread * rng.uniform(-1.0, 1.0, n)
        Ka = rng.uniform(-1.0, 1.0, (n, n))
        eb, Kb = ea, Ka
        if unrestricted:
            eb = ea + split * rng.uniform(-1.0, 1.0, n)
            Kb = rng.uniform(-1.0, 1.0, (n, n))
        self.eps = np.asarray([ea, eb])
        self.U = np.asarray([expm(rot * (K - K.T)) for K in (Ka, Kb)])
        self.h1 = np.asarray([U @ np.diag(e) @ U.T for U, e in zip(self.U, self.eps)])
        self.h1 = 0.5 * (self.h1 + self.h1.transpose(0, 2, 1))
        g = lambda s, t: lam * np.einsum("pq,rs->pqrs", self.h1[s], self.h1[t])
        self.eri = (g(0, 0), g(0, 1), g(1, 1))
        # the occupation patterns of each spin, in the order of itertools.combinations
        self.pat = [list(itertools.combinations(range(n), k)) for k in (na, nb)]
        e1 = [np.asarray([sum(self.eps[s][i] for i in p) for p in self.pat[s]]) for s in range(2)]
        e2 = [np.asarray([sum(self.eps[s][i] ** 2 for i in p) for p in self.pat[s]]) for s in range(2)]
        e = e1[0][:, None] + e1[1][None, :]
        self.levels = e + 0.5 * lam * e * e - 0.5 * lam * (e2[0][:, None] + e2[1][None, :])          # (patterns a, patterns b)
        flat = np.sort(self.levels.reshape(-1))
        self.e0 = float(flat[0])
        self.gap = float(flat[1] - flat[0]) if flat.size > 1 else np.inf
        ia, ib = np.unravel_index(int(np.argmin(self.levels)), self.levels.shape)
        self.occ = (self.pat[0][ia], self.pat[1][ib])

    def spectrum(self):
        return np.sort(self.levels.reshape(-1))

    def slater(self, s, occ):
        """the determinant of the orbitals U_s[:, occ] over the strings of spin s in the order of Space: the minors U_s[I, occ]"""
        k = len(occ)
        if k == 0:
            return np.ones(1)
        rows = np.asarray(sorted(itertools.combinations(range(self.n), k), key=lambda c: sum(1 << i for i in c)))
        return np.linalg.det(self.U[s][rows[:, :, None], np.asarray(occ)[None, None, :]])

    def ground_vector(self):
        return np.multiply.outer(self.slater(0, self.occ[0]), self.slater(1, self.occ[1])).reshape(-1)

    def ground_rdm1(self):
        out = []
        for s in range(2):
            o = np.zeros(self.n)
            o[list(self.occ[s])] = 1.0
            out.append(self.U[s] @ np.diag(o) @ self.U[s].T)
        return np.asarray(out)

    def one_body(self, s, h):
        """O_s(h): sum_pq h_pq E_pq in the string basis of spin s (operators on bit masks, no ERIs)"""
        key = (s, h.tobytes())
        if key not in self._memo_ob:
            sp = Space(self.n, (self.na, self.nb)[s], 0)
            eye, O = np.eye(sp.ndet), np.zeros((sp.ndet, sp.ndet))
            for p in range(self.n):
                for q in range(self.n):
                    O += h[p, q] * sp.apply([("c", p), ("a", q)], eye)
            self._memo_ob[key] = O
        return self._memo_ob[key]

    def matvec(self, c):
        """H c in matrix form: M(h) C = O_a(h_a) C + C O_b(h_b)^T on C (Na, Nb);  H C = M C + lam / 2 M (M C) - lam / 2 M(h^2) C"""
        Oa, Ob = self.one_body(0, self.h1[0]), self.one_body(1, self.h1[1])
        Qa, Qb = self.one_body(0, self.h1[0] @ self.h1[0]), self.one_body(1, self.h1[1] @ self.h1[1])
        Cm = np.asarray(c, dtype=np.float64).reshape(Oa.shape[0], Ob.shape[0])
        M = lambda X: Oa @ X + X @ Ob.T
        MC = M(Cm)
        return (MC + 0.5 * self.lam * M(MC) - 0.5 * self.lam * (Qa @ Cm + Cm @ Qb.T)).reshape(-1)


@functools.lru_cache(maxsize=None)
def solvable(n, na, nb, unrestricted, seed=11, rot=0.08, lam=0.1):
    """shared by the tests, never modified"""
    return Solvable(n, na, nb, unrestricted, seed, rot, lam)


# ---- the device's Davidson loop, restated ---------------------------------------------------------------------------------------------
def davidson(H, hdiag, c0=None, max_iter=200, tol_e=1e-12, tol_r=1e-10, max_space=12):
    """dmk_fci_run of csrc/fci.hip step by step in numpy (H: a dense matrix or a function c -> H c, without H0): the same order of
    tests, the same collapse, the same 1e-14 exhaustion exit (there the residual alone decides `converged`).  A reference for iteration
    counts and flags, never for tolerances.  c0 None: the unit vector on the lowest-diagonal determinant."""
    mv = H if callable(H) else (lambda x: H @ x)
    hdiag = np.asarray(hdiag, dtype=np.float64)
    if c0 is None:
        c0 = np.zeros(hdiag.size)
        c0[int(np.argmin(hdiag))] = 1.0
    c = np.asarray(c0, dtype=np.float64).copy()
    theta = rnorm = dE = e_prev = np.nan
    V, HV, Hs = [], [], np.zeros((16, 16))
    it, conv = 0, 0
    if max_iter > 0:
        V.append(c / np.linalg.norm(c))
    while it < max_iter:
        m = len(HV)
        HV.append(mv(V[m]))
        for k in range(m + 1):
            Hs[k, m] = Hs[m, k] = HV[m] @ V[k]
        m += 1
        it += 1
        w, y = np.linalg.eigh(Hs[:m, :m])
        theta, y = w[0], y[:, 0]
        y = y * (-1.0 if y[int(np.argmax(np.abs(y)))] < 0.0 else 1.0) / np.linalg.norm(y)
        if it == 1:
            e_prev = theta
        c = sum(yk * v for yk, v in zip(y, V))
        hc = sum(yk * v for yk, v in zip(y, HV))
        if m == max_space:
            V, HV, m = [c], [hc], 1
            Hs[0, 0] = theta
        r = hc - theta * c
        t = r / np.maximum(np.abs(hdiag - theta), 1e-8)
        rnorm = float(np.linalg.norm(r))
        dE, e_prev = theta - e_prev, theta
        if abs(dE) < tol_e and rnorm < tol_r:
            conv = 1
            break
        if it == max_iter:
            break
        for _ in range(2):
            for v in V:
                t = t - (t @ v) * v
        nrm = float(np.linalg.norm(t))
        if not nrm > 1e-14:          # no new direction: the Ritz pair cannot improve, the residual alone decides
            conv = int(rnorm < tol_r)
            break
        V.append(t / nrm)
    return dict(e=float(theta), converged=conv, iterations=it, r=rnorm, de=float(dE), c=c)


# iterations of `davidson` (tol_e = 1e-12, tol_r = 1e-10, start: the lowest-diagonal determinant) by max_space; tests/test_host_fci.py
# asserts them, tests/test_gpu_fci_edges.py gives the device twice as many
COLLAPSE_COUNTS = {"sys6": {2: 51, 3: 35, 5: 28, 12: 23}, "sys6u": {2: 146, 3: 76, 5: 51, 12: 40}, "ring6": {2: 68, 3: 46, 5: 34, 12: 28}}

# name -> (kind, n, na, nb, spin, parameter): spaces of at most max_space determinants (the Davidson basis exhausts them), in the
# eigenbasis of the alpha one-body matrix like SOLVER_CASES.
TINY_CASES = {
    "one1": ("factored", 1, 1, 0, 1, 61), "one4": ("factored", 4, 4, 0, 1, 62),
    "two": ("factored", 2, 1, 1, 1, 63), "two_u": ("factored", 2, 1, 1, 2, 64),
    "dimer": ("ring", 2, 1, 1, 1, (4.0, 0.0)), "dimer_field": ("ring", 2, 1, 1, 2, (4.0, 0.25)),
    "three_u": ("factored", 3, 2, 1, 2, 65), "three": ("factored", 3, 1, 1, 1, 66),
}


@functools.lru_cache(maxsize=None)
def tiny_case(name, scale=1.0):
    """(Space, h1, eri, H0, eigenvalues, eigenvectors) of TINY_CASES[name], the whole Hamiltonian multiplied by `scale`."""
    kind, n, na, nb, spin, par = TINY_CASES[name]
    h1, eri = factored(n, par, spin == 2) if kind == "factored" else hubbard_ring(n, par[0], par[1])
    h1, eri = to_basis(h1, eri, np.linalg.eigh(h1[0])[1])
    h1, eri = scale * h1, tuple(scale * g for g in eri)
    sp = Space(n, na, nb)
    w, v = np.linalg.eigh(sp.dense(h1, eri))
    return sp, h1, eri, 0.25 * n * scale, w, v
