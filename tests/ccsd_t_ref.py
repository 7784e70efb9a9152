"""
Numpy restatements of the perturbative triples (T) for the tests of DESIGN.md K22 (tests/test_host_ccsd_t.py,
tests/test_gpu_ccsd_t.py, tests/test_gpu_ccsd_t_shapes.py), in two formulations that share nothing with the device code (csrc/ccsd_t.hip) and little with each other.

  t_spin_orbital(so, t1, t2)      (a) the spin-orbital formula on ccsd_ref.spin_orbital / to_so, with 6-index arrays (small shapes only):
                                      E_(T) = 1/36 sum c (c + d) / D,
                                      c = P(i/jk) P(a/bc) [ sum_e T_jk^ae <ei||bc> - sum_m T_im^bc <ma||jk> ],
                                      d = P(i/jk) P(a/bc) [ T_i^a <jk||bc> + f_ia T_jk^bc ],
                                      D = e_i + e_j + e_k - e_a - e_b - e_c  (the Fock diagonal),  P(i/jk) X = X - X(i<->j) - X(i<->k)
  t_closed_shell(f, blocks, t1, t2, dtype)
                                  (b) the closed-shell formula of DESIGN.md K22 over the blocks of ccsd_ref.restricted_blocks, evaluated
                                      triple by triple over a >= b >= c, in float64 or np.longdouble: -> (E_(T), S), S the same expression
                                      with the absolute value taken at every product (the scale rounding errors are measured against)
  t_closed_shell_streamed(f, blocks, t1, t2, dtype)
                                  (b) again with the six w of one unique triple at a time from matrix products: O(o^3) memory where
                                      t_closed_shell holds v^3 o^3 numbers twice (tests/test_gpu_ccsd_t_shapes.py: o up to 129, v up to 17)
  fci_energy(sysm, nelec_pair)    the exact ground-state energy of a small closed-shell system (all determinants, plain numpy)

Notation of (b): i j k m occupied, a b c f virtual, integrals in chemists' order, t2[i, j, a, b] = t_ij^ab.
    w_ijk^abc = sum_f (ia|bf) t_kj^cf - sum_m (ia|jm) t_mk^bc
    W = the six simultaneous permutations of the pairs (i, a), (j, b), (k, c) of w
    V = W + 1/2 P6[ (ia|jb) t_kc + t_ij^ab f_kc ]
    r3(X)_ijk = 4 X_ijk + X_jki + X_kij - 2 X_kji - 2 X_ikj - 2 X_jik
    Y^abc = sum_ijk W_ijk r3(V)_ijk / D_ijk,     E_(T) = sum_{a >= b >= c} mult(abc) Y^abc,  mult = 2 / 1 / 1/3
"""
import concurrent.futures
import itertools
import os

import numpy as np

from tests import ccsd_ref as CR
from tests import mp2_ref as M


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def _p_i_jk(x):
    """P(i/jk) on the first three axes."""
    return x - x.transpose(1, 0, 2, 3, 4, 5) - x.transpose(2, 1, 0, 3, 4, 5)


def _p_a_bc(x):
    return x - x.transpose(0, 1, 2, 4, 3, 5) - x.transpose(0, 1, 2, 5, 4, 3)


def t_spin_orbital(so, t1, t2):
    T1, T2 = CR.to_so(t1, t2)
    # <ei||bc> = -<ie||bc> = -ovvv[i, e, b, c];  <ma||jk> = <jk||ma> = ooov[j, k, m, a]
    c = -np.einsum("jkae,iebc->ijkabc", T2, so.ovvv) - np.einsum("imbc,jkma->ijkabc", T2, so.ooov)
    d = np.einsum("ia,jkbc->ijkabc", T1, so.oovv) + np.einsum("ia,jkbc->ijkabc", so.fov, T2)
    c, d = _p_a_bc(_p_i_jk(c)), _p_a_bc(_p_i_jk(d))
    eo, ev = so.eo, so.ev
    D = (eo[:, None, None, None, None, None] + eo[None, :, None, None, None, None] + eo[None, None, :, None, None, None]
         - ev[None, None, None, :, None, None] - ev[None, None, None, None, :, None] - ev[None, None, None, None, None, :])
    return float(np.sum(c * (c + d) / D) / 36.0)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
_PERMS = list(itertools.permutations(range(3)))


def _r3(x, sign):
    """r3 with the factors -2 (sign = -1), or all factors taken positive (sign = +1: the absolute-value sum)."""
    return (4 * x + x.transpose(1, 2, 0) + x.transpose(2, 0, 1)
            + sign * 2 * (x.transpose(2, 1, 0) + x.transpose(0, 2, 1) + x.transpose(1, 0, 2)))


def t_closed_shell(fock_mo, blocks, t1, t2, dtype=np.float64):
    """-> (E_(T), S) as Python floats.  All of the arithmetic runs in `dtype`."""
    o, v = t1.shape
    cast = lambda x: np.asarray(x, dtype=dtype)
    f = cast(fock_mo)
    ovvv, ovoo, ovov = cast(blocks["ovvv"]), cast(blocks["ovoo"]), cast(blocks["ovov"])
    t1, t2 = cast(t1), cast(t2)
    fov, eo, ev = f[:o, o:], np.diag(f)[:o], np.diag(f)[o:]
    # every w at once (v^3 o^3 numbers: the shapes of the tests only), then the unique triples one by one
    w_all = np.einsum("iabf,kjcf->abcijk", ovvv, t2) - np.einsum("iajm,mkbc->abcijk", ovoo, t2)
    wabs_all = np.einsum("iabf,kjcf->abcijk", abs(ovvv), abs(t2)) + np.einsum("iajm,mkbc->abcijk", abs(ovoo), abs(t2))
    eijk = eo[:, None, None] + eo[None, :, None] + eo[None, None, :]
    third = dtype(1) / dtype(3)
    e_t = s_t = dtype(0)
    for a in range(v):
        for b in range(a + 1):
            for c in range(b + 1):
                x = (a, b, c)
                W = np.zeros((o, o, o), dtype=dtype)
                Wa = np.zeros((o, o, o), dtype=dtype)
                X = np.zeros((o, o, o), dtype=dtype)
                Xa = np.zeros((o, o, o), dtype=dtype)
                for p in _PERMS:
                    # the pairs in the order p: w^{x_p0 x_p1 x_p2} carries the occupied indices in that order too
                    inv = np.argsort(p)
                    W += w_all[x[p[0]], x[p[1]], x[p[2]]].transpose(*inv)
                    Wa += wabs_all[x[p[0]], x[p[1]], x[p[2]]].transpose(*inv)
                    g = ovov[:, x[p[0]], :, x[p[1]]]                    # (first occupied, second occupied)
                    t = t2[:, :, x[p[0]], x[p[1]]]
                    term = g[:, :, None] * t1[None, None, :, x[p[2]]] + t[:, :, None] * fov[None, None, :, x[p[2]]]
                    terma = abs(g)[:, :, None] * abs(t1)[None, None, :, x[p[2]]] + abs(t)[:, :, None] * abs(fov)[None, None, :, x[p[2]]]
                    X += term.transpose(*inv)
                    Xa += terma.transpose(*inv)
                D = eijk - (ev[a] + ev[b] + ev[c])
                mult = third if a == c else (dtype(1) if (a == b or b == c) else dtype(2))
                e_t += mult * np.sum(W * _r3(W + X / 2, -1) / D)
                s_t += mult * np.sum(Wa * _r3(Wa + Xa / 2, +1) / abs(D))
    return float(e_t), float(s_t)


def t_closed_shell_streamed(fock_mo, blocks, t1, t2, dtype=np.float64, threads=None, chunk_elements=1 << 21):
    """(b) again -> (E_(T), S), for the shapes at which v^3 o^3 numbers do not fit: the six w of a unique triple from matrix products,

        particle part of w^{xyz}   ovvv[:, x, y, :] @ t2[:, :, z, :].reshape(o o, v).T     viewed as (i, k, j)
        hole part of w^{xyz}       ovoo[:, x, :, :].reshape(o o, o) @ t2[:, :, y, z]       viewed as (i, j, k)

    and nothing kept between triples.  The elementwise work of a pair (a, b) runs over a chunk of its c <= b at once (a leading axis
    of at most chunk_elements / o^3 triples, so the memory stays O(o^3)), and the triples are added up one by one in the order of
    t_closed_shell.  The chunks run on `threads` Python threads (default: the CPUs of the process, 16 at the most); the result does
    not depend on their number."""
    o, v = t1.shape
    cast = lambda x: np.asarray(x, dtype=dtype)
    f = cast(fock_mo)
    ovvv, ovoo, ovov = cast(blocks["ovvv"]), cast(blocks["ovoo"]), cast(blocks["ovov"])
    t1, t2 = cast(t1), cast(t2)
    fov, eo, ev = f[:o, o:], np.diag(f)[:o], np.diag(f)[o:]
    sets = ((ovvv, ovoo, ovov, t1, t2, fov, -1), (abs(ovvv), abs(ovoo), abs(ovov), abs(t1), abs(t2), abs(fov), +1))
    eijk = eo[:, None, None] + eo[None, :, None] + eo[None, None, :]
    third = dtype(1) / dtype(3)
    step = max(1, int(chunk_elements) // o ** 3)

    def six(arrays, a, b, cs):
        """(W, X) of the triples (a, b, c), c in the slice cs, as (c, i, j, k), from one set of arrays: the signed one, or the
        absolute values with every term added.  All three virtual indices are index VECTORS of the chunk's length (a and b
        repeated), so every array below has the same shape whichever place c takes in the permutation."""
        vvv, voo, vov, s1, s2, sf, sign = arrays
        nc = cs.stop - cs.start
        W = np.zeros((nc, o, o, o), dtype=dtype)
        X = np.zeros((nc, o, o, o), dtype=dtype)
        x = (np.full(nc, a), np.full(nc, b), np.arange(cs.start, cs.stop))
        for p in _PERMS:
            X0, X1, X2 = x[p[0]], x[p[1]], x[p[2]]                       # the pairs of this w, in its own order (first, second, third)
            # particle: sum_f (first X0 | X1 f) t_{third second}^{X2 f}
            A = vvv[:, X0, X1, :].transpose(1, 0, 2)                     # (c, first, f)
            B = s2[:, :, X2, :].transpose(2, 0, 1, 3).reshape(nc, o * o, v)          # (c, (third second), f)
            part = np.matmul(A, B.transpose(0, 2, 1)).reshape(nc, o, o, o).transpose(0, 1, 3, 2)     # (c, first, second, third)
            # hole: sum_m (first X0 | second m) t_{m third}^{X1 X2}
            A = voo[:, X0, :, :].transpose(1, 0, 2, 3).reshape(nc, o * o, o)         # (c, (first second), m)
            B = s2[:, :, X1, X2].transpose(2, 0, 1)                      # (c, m, third)
            hole = np.matmul(A, B).reshape(nc, o, o, o)                  # (c, first, second, third)
            w = part + sign * hole
            # (first X0 | second X1) t1[third, X2] + t2[first, second, X0, X1] f_ov[third, X2]
            g = vov[:, X0, :, X1]                                        # (c, first, second): index vectors around a slice lead
            t = s2[:, :, X0, X1].transpose(2, 0, 1)                      # (c, first, second)
            u, h = s1[:, X2].T, sf[:, X2].T                              # (c, third)
            term = g[:, :, :, None] * u[:, None, None, :] + t[:, :, :, None] * h[:, None, None, :]
            # the occupied axes from the order of this w to (i, j, k) of the triple (a, b, c): t_closed_shell's transposition
            inv = [0] + [1 + q for q in np.argsort(p)]
            W += w.transpose(*inv)
            X += term.transpose(*inv)
        return W, X

    def r3(xx, sign):
        return (4 * xx + xx.transpose(0, 2, 3, 1) + xx.transpose(0, 3, 1, 2)
                + sign * 2 * (xx.transpose(0, 3, 2, 1) + xx.transpose(0, 1, 3, 2) + xx.transpose(0, 2, 1, 3)))

    def chunk(item):
        """The sums over i j k of the triples (a, b, c in cs): one (signed, absolute) pair of numbers per c."""
        a, b, cs = item
        W, X = six(sets[0], a, b, cs)
        Wa, Xa = six(sets[1], a, b, cs)
        D = eijk[None] - (ev[a] + ev[b] + ev[cs])[:, None, None, None]
        ye = W * r3(W + X / 2, -1) / D
        ys = Wa * r3(Wa + Xa / 2, +1) / abs(D)
        return [(np.sum(ye[n]), np.sum(ys[n])) for n in range(cs.stop - cs.start)]

    # the chunks share nothing, so they may run side by side (numpy drops the interpreter lock in its loops); the sum over the
    # triples below is taken in the fixed order of the list whatever the number of threads
    items = [(a, b, slice(c0, min(b + 1, c0 + step))) for a in range(v) for b in range(a + 1) for c0 in range(0, b + 1, step)]
    if threads is None:
        threads = min(16, len(os.sched_getaffinity(0)))
    threads = max(1, min(int(threads), len(items)))
    if threads == 1:
        sums = [chunk(item) for item in items]
    else:
        with concurrent.futures.ThreadPoolExecutor(threads) as pool:
            sums = list(pool.map(chunk, items))
    e_t = s_t = dtype(0)
    for (a, b, cs), per_c in zip(items, sums):
        for c, (ye, ys) in zip(range(cs.start, cs.stop), per_c):
            mult = third if a == c else (dtype(1) if (a == b or b == c) else dtype(2))
            e_t += mult * ye
            s_t += mult * ys
    return float(e_t), float(s_t)


# ---- exact diagonalisation ---------------------------------------------------------------------------------------------------------
def fci_energy(h1, g, npair):
    """The lowest eigenvalue of H = sum h_pq a+_p a_q + 1/2 sum (pq|rs) a+_p a+_r a_s a_q in the space of npair alpha and npair beta
    electrons over the n orthonormal orbitals of h1 (n, n) and g (n, n, n, n), all determinants, dense."""
    n = h1.shape[0]
    strings = [s for s in itertools.combinations(range(n), npair)]
    index = {s: k for k, s in enumerate(strings)}
    ns = len(strings)

    def excite(s, p, q):
        """a+_p a_q |s> -> (sign, string) or None"""
        if q not in s or (p in s and p != q):
            return None
        lst = list(s)
        sign = (-1) ** lst.index(q)
        lst.remove(q)
        pos = sum(1 for r in lst if r < p)
        sign *= (-1) ** pos
        lst.insert(pos, p)
        return sign, tuple(lst)

    # E_pq for one spin as a dense (ns, ns) matrix
    E = np.zeros((n, n, ns, ns))
    for k, s in enumerate(strings):
        for p in range(n):
            for q in range(n):
                r = excite(s, p, q)
                if r is not None:
                    E[p, q, index[r[1]], k] += r[0]
    eye = np.eye(ns)
    # H = sum h_pq E_pq + 1/2 sum (pq|rs) (E_pq E_rs - delta_qr E_ps), E = E^alpha + E^beta
    k1 = h1 - 0.5 * np.einsum("prrq->pq", g)
    Ea = E.reshape(n * n, ns, ns)
    H = np.zeros((ns * ns, ns * ns))
    one = np.einsum("x,xuv->uv", k1.reshape(-1), Ea)
    H += np.kron(one, eye) + np.kron(eye, one)
    G = g.reshape(n * n, n * n)
    same = 0.5 * np.einsum("xy,xuw,ywv->uv", G, Ea, Ea, optimize=True)
    H += np.kron(same, eye) + np.kron(eye, same)
    lw, lv = np.linalg.eigh(G)
    for val, vec in zip(lw, lv.T):
        if abs(val) > 1e-14:
            A = np.einsum("x,xuv->uv", vec, Ea)
            H += val * np.kron(A, A)                           # 1/2 (E^a E^b + E^b E^a) = E^a (x) E^b
    return float(np.linalg.eigvalsh(H)[0])


def mo_integrals(sysm, C):
    """(h1, g) of the system at the orbitals C: g[p, q, r, s] = (pq|rs)."""
    n = sysm.n
    C = np.asarray(C, dtype=np.float64)
    return C.T @ sysm.h1 @ C, M.transform(sysm, "aa", C, C, C, C).reshape(n, n, n, n)
