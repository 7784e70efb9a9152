"""
Numpy restatement of the MO integral transform and of MP2 for the tests of DESIGN.md K19 / K20 (tests/test_host_mp2.py,
tests/test_gpu_ao2mo.py, tests/test_gpu_mp2.py), on the FACTORED Hamiltonians of tests/scf_ref.py:

    (ij|kl)_xy = lam sum_P X_P[i,j] Y_P[k,l]            X, Y in {A, B}: the symmetric factor matrices of the system

The transform never touches the packed layout:   out[(i,j),(k,l)] = lam sum_P (C1^T X_P C2)[i,j] (C3^T Y_P C4)[k,l]
and (ia|jb) comes from the same factors.  The MP2 formulas are literal einsums (PySCF's mp2.make_rdm1 / ump2 conventions):

  restricted    D_ij^ab = e_i + e_j - e_a - e_b,  t = (ia|jb) / D,  t~ = 2 t_ij^ab - t_ij^ba,  e = sum t~ (ia|jb),
                X_ij = sum_kab t_ik^ab t~_jk^ab,  Y_ab = sum_ijc t_ij^ac t~_ij^bc,  doo = 2 - (X + X^T),  dvv = Y + Y^T
  unrestricted  t_aa = [(ia|jb) - (ib|ja)] / D (t_bb likewise),  t_ab = (ia|JB) / D,
                e = 1/4 sum t_aa <ij||ab> + 1/4 sum t_bb <IJ||AB> + sum t_ab (ia|JB),
                doo_a = 1 - 1/2 sum_kab t_aa t_aa - sum_KaB t_ab t_ab,  dvv_a = 1/2 sum t_aa t_aa + sum t_ab t_ab,
                the beta blocks with t_ab contracted over its alpha indices
"""
import numpy as np

from tests import scf_ref as R


def factors(sysm, which):
    """(X, Y) factor stacks of block `which` = 'aa' | 'bb' | 'ab'."""
    L = {"a": sysm.A, "b": sysm.B}
    return L[which[0]], L[which[1]]


def transform(sysm, which, c1, c2, c3, c4):
    """out[(i,j),(k,l)] of block `which`, (n1 n2, n3 n4)."""
    X, Y = factors(sysm, which)
    bra = np.einsum("pi,Ppq,qj->Pij", c1, X, c2).reshape(X.shape[0], -1)
    ket = np.einsum("rk,Prs,sl->Pkl", c3, Y, c4).reshape(Y.shape[0], -1)
    return sysm.lam * (bra.T @ ket)


def transform_einsum(eri1, c1, c2, c3, c4):
    """The literal n^4 contraction of a 1-fold block (n <= 6)."""
    n1, n2, n3, n4 = c1.shape[1], c2.shape[1], c3.shape[1], c4.shape[1]
    return np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri1, c1, c2, c3, c4).reshape(n1 * n2, n3 * n4)


def pack_rows(M, n):
    """Rows (i, j) of an (n n, .) matrix -> rows pair(i, j), i >= j."""
    i, j = np.tril_indices(n)
    return M.reshape(n, n, -1)[i, j]


def pack_cols(M, n):
    i, j = np.tril_indices(n)
    return M.reshape(M.shape[0], n, n)[:, i, j]


def ovov(sysm, which, co1, cv1, co2, cv2):
    """(ia|jb) as (o1, v1, o2, v2)."""
    return transform(sysm, which, co1, cv1, co2, cv2).reshape(co1.shape[1], cv1.shape[1], co2.shape[1], cv2.shape[1])


def _denominator(eo1, ev1, eo2, ev2):
    return eo1[:, None, None, None] + eo2[None, :, None, None] - ev1[None, None, :, None] - ev2[None, None, None, :]


def rmp2(sysm, mo_coeff, mo_energy, nocc):
    """Restricted MP2: {"e_corr", "t2" (i, j, a, b), "rdm1_mo" (spin-traced), "rdm1_ao"}."""
    n = mo_coeff.shape[0]
    co, cv, eo, ev = mo_coeff[:, :nocc], mo_coeff[:, nocc:], mo_energy[:nocc], mo_energy[nocc:]
    g = ovov(sysm, "aa", co, cv, co, cv).transpose(0, 2, 1, 3)                       # g[i, j, a, b] = (ia|jb)
    t = g / _denominator(eo, ev, eo, ev)
    tt = 2.0 * t - t.transpose(0, 1, 3, 2)
    e = np.einsum("ijab,ijab", tt, g)
    X = np.einsum("ikab,jkab->ij", t, tt)
    Y = np.einsum("ijac,ijbc->ab", t, tt)
    D = np.zeros((n, n))
    D[:nocc, :nocc] = 2.0 * np.eye(nocc) - (X + X.T)
    D[nocc:, nocc:] = Y + Y.T
    return {"e_corr": float(e), "t2": t, "rdm1_mo": D, "rdm1_ao": mo_coeff @ D @ mo_coeff.T}


def ump2(sysm, mo_coeff, mo_energy, nocc):
    """Unrestricted MP2 (mo_coeff (2, n, n), mo_energy (2, n), nocc (na, nb)): t2 = (aa, ab, bb), rdm1 (2, n, n)."""
    n = mo_coeff.shape[-1]
    (ca, cb), (ea, eb), (oa, ob) = mo_coeff, mo_energy, nocc
    gaa = ovov(sysm, "aa", ca[:, :oa], ca[:, oa:], ca[:, :oa], ca[:, oa:]).transpose(0, 2, 1, 3)
    gbb = ovov(sysm, "bb", cb[:, :ob], cb[:, ob:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
    gab = ovov(sysm, "ab", ca[:, :oa], ca[:, oa:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
    aaa, abb = gaa - gaa.transpose(0, 1, 3, 2), gbb - gbb.transpose(0, 1, 3, 2)                # <ij||ab>
    taa = aaa / _denominator(ea[:oa], ea[oa:], ea[:oa], ea[oa:])
    tbb = abb / _denominator(eb[:ob], eb[ob:], eb[:ob], eb[ob:])
    tab = gab / _denominator(ea[:oa], ea[oa:], eb[:ob], eb[ob:])
    e = 0.25 * np.einsum("ijab,ijab", taa, aaa) + 0.25 * np.einsum("ijab,ijab", tbb, abb) + np.einsum("ijab,ijab", tab, gab)
    D = np.zeros((2, n, n))
    D[0, :oa, :oa] = np.eye(oa) - 0.5 * np.einsum("ikab,jkab->ij", taa, taa) - np.einsum("ikab,jkab->ij", tab, tab)
    D[0, oa:, oa:] = 0.5 * np.einsum("ijac,ijbc->ab", taa, taa) + np.einsum("ijac,ijbc->ab", tab, tab)
    D[1, :ob, :ob] = np.eye(ob) - 0.5 * np.einsum("ikab,jkab->ij", tbb, tbb) - np.einsum("kiab,kjab->ij", tab, tab)
    D[1, ob:, ob:] = 0.5 * np.einsum("ijac,ijbc->ab", tbb, tbb) + np.einsum("ijca,ijcb->ab", tab, tab)
    return {"e_corr": float(e), "t2": (taa, tab, tbb), "rdm1_mo": D,
            "rdm1_ao": np.asarray([mo_coeff[s] @ D[s] @ mo_coeff[s].T for s in range(2)])}


def mp2_of_case(kind, n, Sz, mo_coeff=None, mo_energy=None):
    """MP2 of a listed case of scf_ref.SEEDS at the given orbitals (default: the numpy SCF's own)."""
    sysm = R.make_system(kind, n, Sz)
    nocc = R.nocc_of(kind, n, Sz)
    if mo_coeff is None:
        ref = R.run_case(kind, n, Sz)
        mo_coeff, mo_energy = ref["mo_coeff"], ref["mo_energy"]
    if kind == "rhf":
        return rmp2(sysm, np.asarray(mo_coeff), np.asarray(mo_energy), nocc[0])
    return ump2(sysm, np.asarray(mo_coeff), np.asarray(mo_energy), nocc)
