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

The formulas stand once, in rmp2_from_g / ump2_from_g, which work in the dtype of their arguments: rmp2 / ump2 feed them the float64
integrals of a factored system, tests/test_gpu_mp2_kernel.py synthetic integrals (synthetic_g, synthetic_levels) at np.longdouble
together with the forward error bounds of rmp2_bounds / ump2_bounds.
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


def rmp2_from_g(g, eo, ev):
    """Restricted MP2 from g[i, j, a, b] = (ia|jb) and the orbital energies, in the dtype of the arguments (float64 or
    np.longdouble): {"e_corr", "t2" (i, j, a, b), "doo", "dvv"} (spin-traced blocks)."""
    o = g.shape[0]
    t = g / _denominator(eo, ev, eo, ev)
    tt = 2.0 * t - t.transpose(0, 1, 3, 2)
    e = np.einsum("ijab,ijab", tt, g)
    X = np.einsum("ikab,jkab->ij", t, tt)
    Y = np.einsum("ijac,ijbc->ab", t, tt)
    return {"e_corr": e, "t2": t, "doo": 2.0 * np.eye(o, dtype=g.dtype) - (X + X.T), "dvv": Y + Y.T}


def ump2_from_g(gaa, gab, gbb, ea_o, ea_v, eb_o, eb_v):
    """Unrestricted MP2 from g[i, j, a, b] = (ia|jb) of the three spin blocks, in the dtype of the arguments:
    {"e_corr", "t2" = (aa, ab, bb), "doo_a", "dvv_a", "doo_b", "dvv_b"}."""
    oa, ob = gaa.shape[0], gbb.shape[0]
    aaa, abb = gaa - gaa.transpose(0, 1, 3, 2), gbb - gbb.transpose(0, 1, 3, 2)                # <ij||ab>
    taa = aaa / _denominator(ea_o, ea_v, ea_o, ea_v)
    tbb = abb / _denominator(eb_o, eb_v, eb_o, eb_v)
    tab = gab / _denominator(ea_o, ea_v, eb_o, eb_v)
    e = 0.25 * np.einsum("ijab,ijab", taa, aaa) + 0.25 * np.einsum("ijab,ijab", tbb, abb) + np.einsum("ijab,ijab", tab, gab)
    return {"e_corr": e, "t2": (taa, tab, tbb),
            "doo_a": np.eye(oa, dtype=gaa.dtype) - 0.5 * np.einsum("ikab,jkab->ij", taa, taa) - np.einsum("ikab,jkab->ij", tab, tab),
            "dvv_a": 0.5 * np.einsum("ijac,ijbc->ab", taa, taa) + np.einsum("ijac,ijbc->ab", tab, tab),
            "doo_b": np.eye(ob, dtype=gbb.dtype) - 0.5 * np.einsum("ikab,jkab->ij", tbb, tbb) - np.einsum("kiab,kjab->ij", tab, tab),
            "dvv_b": 0.5 * np.einsum("ijac,ijbc->ab", tbb, tbb) + np.einsum("ijca,ijcb->ab", tab, tab)}


EPS = 2.0 ** -52


def _diag(d):
    return 2.0 * EPS * np.eye(d, dtype=np.longdouble)


def rmp2_bounds(g, ref):
    """Per-element forward bounds of a float64 evaluation against `ref` = rmp2_from_g at np.longdouble (tests/test_gpu_mp2_kernel.py,
    tests/test_host_mp2.py), themselves evaluated in np.longdouble:
      amplitudes  16 eps |t|: three additions in the denominator (|D| >= 2, operands <= 1.5 each) and one correctly rounded division
      energy      (N + 64) eps sum |t~ g|, N the number of amplitudes
      densities   (L + 64) eps S + 2 eps on the diagonal; L the contraction length (o v^2, o^2 v), S the contraction over absolute
                  values plus its transpose (the blocks are symmetrised); the 64 covers the propagated amplitude error."""
    ld = np.longdouble
    o, v = g.shape[0], g.shape[2]
    t = np.abs(ref["t2"].astype(ld))
    tt = np.abs(2.0 * ref["t2"].astype(ld) - ref["t2"].astype(ld).transpose(0, 1, 3, 2))
    X, Y = np.einsum("ikab,jkab->ij", t, tt), np.einsum("ijac,ijbc->ab", t, tt)
    return {"t2": 16.0 * EPS * t, "e_corr": (t.size + 64) * EPS * np.einsum("ijab,ijab", tt, np.abs(g.astype(ld))),
            "doo": (o * v * v + 64) * EPS * (X + X.T) + _diag(o), "dvv": (o * o * v + 64) * EPS * (Y + Y.T) + _diag(v)}


def ump2_bounds(gaa, gab, gbb, ref):
    """rmp2_bounds for ump2_from_g.  A density block is a sum of two contractions: each contributes (L + 64) eps S with its own
    length and its own sum over absolute values (the same-spin one carries its factor 1/2)."""
    ld = np.longdouble
    (oa, _, va, _), (ob, _, vb, _) = gaa.shape, gbb.shape
    taa, tab, tbb = (np.abs(x.astype(ld)) for x in ref["t2"])
    anti = lambda x: np.abs(x.astype(ld) - x.astype(ld).transpose(0, 1, 3, 2))
    e = 0.25 * np.einsum("ijab,ijab", taa, anti(gaa)) + 0.25 * np.einsum("ijab,ijab", tbb, anti(gbb)) + \
        np.einsum("ijab,ijab", tab, np.abs(gab.astype(ld)))
    term = lambda L, S: (L + 64) * EPS * S
    return {"t2": tuple(16.0 * EPS * x for x in (taa, tab, tbb)),
            "e_corr": (taa.size + tab.size + tbb.size + 64) * EPS * e,
            "doo_a": term(oa * va * va, 0.5 * np.einsum("ikab,jkab->ij", taa, taa)) +
                     term(ob * va * vb, np.einsum("ikab,jkab->ij", tab, tab)) + _diag(oa),
            "dvv_a": term(oa * oa * va, 0.5 * np.einsum("ijac,ijbc->ab", taa, taa)) +
                     term(oa * ob * vb, np.einsum("ijac,ijbc->ab", tab, tab)) + _diag(va),
            "doo_b": term(ob * vb * vb, 0.5 * np.einsum("ikab,jkab->ij", tbb, tbb)) +
                     term(oa * va * vb, np.einsum("kiab,kjab->ij", tab, tab)) + _diag(ob),
            "dvv_b": term(ob * ob * vb, 0.5 * np.einsum("ijac,ijbc->ab", tbb, tbb)) +
                     term(oa * ob * va, np.einsum("ijca,ijcb->ab", tab, tab)) + _diag(vb)}


def ratio(got, ref, bound):
    """Largest |got - ref| / bound over the elements, in np.longdouble; an exact zero of the bound (the same-spin amplitudes with
    i = j or a = b) admits only an exact result: 0 / 0 counts 0, anything else inf."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    bound = np.asarray(bound, dtype=np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


def ratios(got, ref, bound):
    """ratio per key of the dictionaries of *_from_g / *_bounds (t2 an array or a tuple of three)."""
    out = {}
    for key, b in bound.items():
        if isinstance(b, tuple):
            out[key] = max(ratio(x, y, z) for x, y, z in zip(got[key], ref[key], b))
        else:
            out[key] = ratio(got[key], ref[key], b)
    return out


def synthetic_g(rng, n1, n2=None, naux=12):
    """A synthetic (ia|jb) matrix, rows (i, a), columns (j, b): L^T L / naux, exactly symmetric (one compound index, n2 None), or
    La^T Lb / naux for two different ones."""
    La = rng.standard_normal((naux, n1))
    if n2 is None:
        V = La.T @ La / naux
        return 0.5 * (V + V.T)
    return La.T @ rng.standard_normal((naux, n2)) / naux


def synthetic_levels(rng, o, v):
    """Occupied levels in [-1.5, -0.5] and virtual levels in [0.5, 1.5] in one array (every denominator <= -2), one exactly
    repeated level in each group that has at least two."""
    eo, ev = rng.uniform(-1.5, -0.5, o), rng.uniform(0.5, 1.5, v)
    if o >= 2:
        eo[-1] = eo[0]
    if v >= 2:
        ev[v // 2] = ev[0]
    return np.concatenate([eo, ev])


def rmp2(sysm, mo_coeff, mo_energy, nocc):
    """Restricted MP2: {"e_corr", "t2" (i, j, a, b), "rdm1_mo" (spin-traced), "rdm1_ao"}."""
    n = mo_coeff.shape[0]
    co, cv, eo, ev = mo_coeff[:, :nocc], mo_coeff[:, nocc:], mo_energy[:nocc], mo_energy[nocc:]
    g = ovov(sysm, "aa", co, cv, co, cv).transpose(0, 2, 1, 3)                       # g[i, j, a, b] = (ia|jb)
    out = rmp2_from_g(g, eo, ev)
    D = np.zeros((n, n))
    D[:nocc, :nocc] = out["doo"]
    D[nocc:, nocc:] = out["dvv"]
    return {"e_corr": float(out["e_corr"]), "t2": out["t2"], "rdm1_mo": D, "rdm1_ao": mo_coeff @ D @ mo_coeff.T}


def ump2(sysm, mo_coeff, mo_energy, nocc):
    """Unrestricted MP2 (mo_coeff (2, n, n), mo_energy (2, n), nocc (na, nb)): t2 = (aa, ab, bb), rdm1 (2, n, n)."""
    n = mo_coeff.shape[-1]
    (ca, cb), (ea, eb), (oa, ob) = mo_coeff, mo_energy, nocc
    gaa = ovov(sysm, "aa", ca[:, :oa], ca[:, oa:], ca[:, :oa], ca[:, oa:]).transpose(0, 2, 1, 3)
    gbb = ovov(sysm, "bb", cb[:, :ob], cb[:, ob:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
    gab = ovov(sysm, "ab", ca[:, :oa], ca[:, oa:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
    out = ump2_from_g(gaa, gab, gbb, ea[:oa], ea[oa:], eb[:ob], eb[ob:])
    D = np.zeros((2, n, n))
    D[0, :oa, :oa], D[0, oa:, oa:] = out["doo_a"], out["dvv_a"]
    D[1, :ob, :ob], D[1, ob:, ob:] = out["doo_b"], out["dvv_b"]
    return {"e_corr": float(out["e_corr"]), "t2": out["t2"], "rdm1_mo": D,
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
