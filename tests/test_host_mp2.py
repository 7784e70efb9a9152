"""
Host-side checks of the MO transform and MP2 layer, no GPU: the numpy reference of tests/mp2_ref.py against
literal n^4 einsums and against itself (restricted = unrestricted with equal spins, traces), the host-only pieces of solver/scf.py and
solver/mp.py (regularize_coeff, argument checks that raise before a device context exists, the planner of the transform) and the
rows of the rebinding table.
"""
import numpy as np
import pytest

from tests import mp2_ref as M
from tests import scf_ref as R


def test_modules_import_without_a_gpu():
    from libdmet_preview_amd.solver import mp, scf
    assert callable(scf.incore_transform) and callable(scf.ao2mo_Ham) and callable(scf.regularize_coeff)
    assert callable(mp.MP2) and callable(mp.UIMP2) and callable(mp.run_mp2)


@pytest.mark.parametrize("which", ["aa", "ab"])
def test_factored_transform_equals_the_einsum(which):
    n = 6
    sysm = R.System(n, 5, [3])
    rng = np.random.default_rng(8)
    cs = [rng.standard_normal((n, w)) for w in (3, 2, 4, 5)]
    e1 = R.restore_s1(sysm.block_s4(which), n)
    assert np.abs(M.transform(sysm, which, *cs) - M.transform_einsum(e1, *cs)).max() <= 1e-13
    full = M.transform(sysm, which, cs[0], cs[0], cs[2], cs[2])
    assert M.pack_rows(full, 3).shape == (6, 16) and M.pack_cols(full, 4).shape == (9, 10)
    assert np.array_equal(M.pack_cols(M.pack_rows(full, 3), 4)[1], full.reshape(3, 3, 4, 4)[1, 0][np.tril_indices(4)])


@pytest.mark.parametrize("n", [6, 9])
def test_restricted_equals_unrestricted_with_equal_spins(n):
    ref = R.run_case("rhf", n, 0, seed=70 + n)
    sysm, nocc = ref["system"], ref["nocc"][0]
    sysm.B = sysm.A                                    # equal spins: bb and ab are the aa block
    c, e = ref["mo_coeff"], ref["mo_energy"]
    r = M.rmp2(sysm, c, e, nocc)
    u = M.ump2(sysm, np.asarray([c, c]), np.asarray([e, e]), (nocc, nocc))
    assert abs(r["e_corr"] - u["e_corr"]) <= 1e-14 and r["e_corr"] < 0.0
    assert np.abs(r["rdm1_mo"] - u["rdm1_mo"].sum(axis=0)).max() <= 1e-14
    assert np.abs(u["rdm1_mo"][0] - u["rdm1_mo"][1]).max() <= 1e-14
    assert np.abs(r["t2"] - u["t2"][1]).max() <= 1e-14
    assert np.abs(u["t2"][0] - (r["t2"] - r["t2"].transpose(0, 1, 3, 2))).max() <= 1e-14


@pytest.mark.parametrize("kind,n,Sz", [("rhf", 6, 0), ("uhf", 6, 0), ("uhf", 6, 2), ("rhf", 9, 0)])
def test_density_trace_is_the_electron_count(kind, n, Sz):
    if (kind, n, Sz) in R.SEEDS:
        out = M.mp2_of_case(kind, n, Sz)
    else:
        ref = R.run_case(kind, n, Sz, seed=77)
        out = M.rmp2(ref["system"], ref["mo_coeff"], ref["mo_energy"], ref["nocc"][0])
    nocc = R.nocc_of(kind, n, Sz)
    D = out["rdm1_mo"]
    if kind == "rhf":
        assert abs(np.trace(D) - 2 * nocc[0]) <= 1e-13 and abs(np.trace(out["rdm1_ao"]) - 2 * nocc[0]) <= 1e-12
        assert np.abs(D - D.T).max() <= 1e-15
    else:
        assert abs(np.trace(D[0]) - nocc[0]) <= 1e-13 and abs(np.trace(D[1]) - nocc[1]) <= 1e-13
    assert out["e_corr"] < 0.0 and abs(out["e_corr"]) < 1.0


@pytest.mark.parametrize("kind,n,Sz", [("rhf", 6, 0), ("uhf", 6, 2)])
def test_longdouble_reference_equals_the_float64_one_on_a_listed_system(kind, n, Sz):
    """The formulas of rmp2_from_g / ump2_from_g at np.longdouble (the reference of tests/test_gpu_mp2_kernel.py) against the
    float64 evaluation that rmp2 / ump2 return, on listed cases of scf_ref.SEEDS: within 1e-12, and within the forward bounds."""
    ld = np.longdouble
    ref = R.run_case(kind, n, Sz)
    sysm, c, e, nocc = ref["system"], np.asarray(ref["mo_coeff"]), np.asarray(ref["mo_energy"]), ref["nocc"]
    if kind == "rhf":
        o = nocc[0]
        g = M.ovov(sysm, "aa", c[:, :o], c[:, o:], c[:, :o], c[:, o:]).transpose(0, 2, 1, 3)
        lo, hi = M.rmp2_from_g(g, e[:o], e[o:]), M.rmp2_from_g(g.astype(ld), e[:o].astype(ld), e[o:].astype(ld))
        bound = M.rmp2_bounds(g, hi)
        assert lo["t2"].dtype == np.float64 and hi["t2"].dtype == ld and hi["doo"].dtype == ld and hi["dvv"].dtype == ld
        assert np.array_equal(lo["t2"], M.rmp2(sysm, c, e, o)["t2"])
    else:
        (ca, cb), (ea, eb), (oa, ob) = c, e, nocc
        gaa = M.ovov(sysm, "aa", ca[:, :oa], ca[:, oa:], ca[:, :oa], ca[:, oa:]).transpose(0, 2, 1, 3)
        gbb = M.ovov(sysm, "bb", cb[:, :ob], cb[:, ob:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
        gab = M.ovov(sysm, "ab", ca[:, :oa], ca[:, oa:], cb[:, :ob], cb[:, ob:]).transpose(0, 2, 1, 3)
        es = (ea[:oa], ea[oa:], eb[:ob], eb[ob:])
        lo = M.ump2_from_g(gaa, gab, gbb, *es)
        hi = M.ump2_from_g(gaa.astype(ld), gab.astype(ld), gbb.astype(ld), *(x.astype(ld) for x in es))
        bound = M.ump2_bounds(gaa, gab, gbb, hi)
        assert all(x.dtype == ld for x in hi["t2"]) and hi["doo_b"].dtype == ld
        assert all(np.array_equal(x, y) for x, y in zip(lo["t2"], M.ump2(sysm, c, e, nocc)["t2"]))
    for key in bound:
        a, b = (lo[key], hi[key]) if isinstance(bound[key], tuple) else ((lo[key],), (hi[key],))
        assert max(float(np.abs(x.astype(ld) - y).max()) for x, y in zip(a, b)) <= 1e-12, key
    ratios = M.ratios(lo, hi, bound)
    print("%s n=%d Sz=%d float64 against longdouble, err / bound: %s" % (kind, n, Sz, {k: "%.3f" % r for k, r in ratios.items()}))
    assert max(ratios.values()) <= 1.0


def test_float64_formulas_hold_the_bounds_on_synthetic_integrals():
    """The inputs of tests/test_gpu_mp2_kernel.py (synthetic_g, synthetic_levels) at two of its shapes: numpy's float64 evaluation
    of the formulas stays within the bounds the device result is held to, denominators are <= -2 and the repeated levels are there."""
    ld = np.longdouble
    rng = np.random.default_rng(20)
    for o, v in [(1, 1), (2, 3), (7, 16)]:
        V, e = M.synthetic_g(rng, o * v), M.synthetic_levels(rng, o, v)
        assert np.array_equal(V, V.T) and e[:o].max() <= -0.5 and e[o:].min() >= 0.5
        assert (o < 2 or e[o - 1] == e[0]) and (v < 2 or e[o + v // 2] == e[o])
        g = V.reshape(o, v, o, v).transpose(0, 2, 1, 3)
        lo, hi = M.rmp2_from_g(g, e[:o], e[o:]), M.rmp2_from_g(g.astype(ld), e[:o].astype(ld), e[o:].astype(ld))
        assert max(M.ratios(lo, hi, M.rmp2_bounds(g, hi)).values()) <= 1.0
        assert abs(float(np.trace(hi["doo"]) + np.trace(hi["dvv"])) - 2 * o) <= 1e-15 * o * o * v * v
    oa, va, ob, vb = 5, 9, 2, 12
    gaa = M.synthetic_g(rng, oa * va).reshape(oa, va, oa, va).transpose(0, 2, 1, 3)
    gbb = M.synthetic_g(rng, ob * vb).reshape(ob, vb, ob, vb).transpose(0, 2, 1, 3)
    gab = M.synthetic_g(rng, oa * va, ob * vb).reshape(oa, va, ob, vb).transpose(0, 2, 1, 3)
    ea, eb = M.synthetic_levels(rng, oa, va), M.synthetic_levels(rng, ob, vb)
    es = (ea[:oa], ea[oa:], eb[:ob], eb[ob:])
    lo = M.ump2_from_g(gaa, gab, gbb, *es)
    hi = M.ump2_from_g(gaa.astype(ld), gab.astype(ld), gbb.astype(ld), *(x.astype(ld) for x in es))
    assert max(M.ratios(lo, hi, M.ump2_bounds(gaa, gab, gbb, hi)).values()) <= 1.0
    assert abs(float(np.trace(hi["doo_a"]) + np.trace(hi["dvv_a"])) - oa) <= 1e-15 and \
        abs(float(np.trace(hi["doo_b"]) + np.trace(hi["dvv_b"])) - ob) <= 1e-15


def test_restricted_energy_against_the_spin_orbital_formula():
    """e = 1/4 sum |<ij||ab>|^2 / D over spin orbitals, from the 1-fold block -- a third statement of the energy."""
    n = 6
    ref = R.run_case("rhf", n, 0)
    sysm, o = ref["system"], ref["nocc"][0]
    c, e = ref["mo_coeff"], ref["mo_energy"]
    mo = np.einsum("pqrs,pi,qj,rk,sl->ijkl", R.restore_s1(sysm.block_s4("aa"), n), c, c, c, c)
    so = np.zeros((2 * n,) * 4)
    for s in range(2):
        for t in range(2):
            so[s::2, s::2, t::2, t::2] = mo                                   # (pq|rs) with spin(p) = spin(q), spin(r) = spin(s)
    eso = np.repeat(e, 2)
    occ, vir = np.arange(2 * o), np.arange(2 * o, 2 * n)
    g = so[np.ix_(occ, vir, occ, vir)].transpose(0, 2, 1, 3)
    anti = g - g.transpose(0, 1, 3, 2)
    D = eso[occ][:, None, None, None] + eso[occ][None, :, None, None] - eso[vir][None, None, :, None] - eso[vir][None, None, None, :]
    assert abs(0.25 * np.sum(anti ** 2 / D) - M.rmp2(sysm, c, e, o)["e_corr"]) <= 1e-14


def test_regularize_coeff():
    from libdmet_preview_amd.solver.scf import regularize_coeff
    a, b = np.zeros((4, 2)), np.ones((4, 3))
    lst, spin = regularize_coeff((a, b, a, b))
    assert spin == 1 and lst[0] is a and lst[1] is b
    lst, spin = regularize_coeff(([a], [b], [a], [b]))
    assert spin == 1 and lst[0] is a and lst[3] is b
    lst, spin = regularize_coeff(([a, b], [a, b], [a, b], [a, b]))
    assert spin == 2 and lst[2][0] is a and lst[2][1] is b
    lst, spin = regularize_coeff((np.zeros((2, 4, 2)),) * 4)                   # a 3-d array is a pair of spin channels
    assert spin == 2 and lst[0].shape == (2, 4, 2)


def test_argument_checks_raise_before_a_context_exists():
    from libdmet_preview_amd.solver import mp, scf
    from libdmet_preview_amd.system import integral
    with pytest.raises(Exception):
        scf.incore_transform(np.zeros((10, 10)), (np.eye(4),) * 3)                       # three coefficient sets
    with pytest.raises(ValueError):
        scf.incore_transform(np.zeros((3, 10, 10)), (np.eye(4),) * 4)                    # spinless coefficients, three blocks
    with pytest.raises(ValueError):
        scf.incore_transform(np.zeros((10, 10)), ([np.eye(4)] * 3,) * 4)                 # three spin channels
    bogo = integral.Integral(4, False, True, 0.0, {"cd": np.zeros((2, 4, 4))}, {"ccdd": np.zeros((3, 10, 10))})
    with pytest.raises(NotImplementedError):
        scf.ao2mo_Ham(bogo, np.eye(4))
    with pytest.raises(NotImplementedError):
        mp.MP2(object(), frozen=2)
    with pytest.raises(NotImplementedError):
        mp.MP2(object(), frozen=[0, 1])
    with pytest.raises(NotImplementedError):
        mp.UIMP2(object())                                                               # not a device Hartree-Fock object
    s = scf.SCF()
    for name in ("MP2", "GMP2"):
        with pytest.raises(NotImplementedError, match="run_mp2"):
            getattr(s, name)()


def test_transform_planner():
    """dmk_ao2mo_plan (host): one slab under the default workspace for the shapes of the tests, at least three under a quarter of
    that, the workspace within the budget given, and the refusals."""
    import ctypes as C
    from libdmet_preview_amd._lib import lib
    plan = (C.c_int64 * 3)()
    assert lib.dmk_ao2mo_plan(65, 65, 65, 65, 65, 3, 0, plan) == 0
    npair = 65 * 66 // 2
    assert plan[0] == 1 and plan[2] == npair * npair
    one = plan[1]
    assert lib.dmk_ao2mo_plan(65, 65, 65, 65, 65, 3, one // 4, plan) == 0
    assert plan[0] >= 3 and plan[1] <= one // 4
    assert lib.dmk_ao2mo_plan(65, 17, 48, 33, 65, 0, 0, plan) == 0 and plan[0] == 1 and plan[2] == 17 * 48 * 33 * 65
    assert lib.dmk_ao2mo_plan(256, 128, 128, 128, 128, 0, 0, plan) == 0 and plan[1] <= 12 << 30
    assert lib.dmk_ao2mo_plan(65, 65, 65, 65, 65, 3, 1 << 16, plan) == -1 and plan[1] > (1 << 16)      # cannot hold one k
    assert lib.dmk_ao2mo_plan(65, 17, 48, 33, 65, 1, 0, plan) == -1                                   # PACK_BRA with n1 != n2
    assert lib.dmk_ao2mo_plan(513, 5, 5, 5, 5, 0, 0, plan) == -1 and lib.dmk_ao2mo_plan(65, 0, 5, 5, 5, 0, 0, plan) == -1
    assert lib.dmk_ao2mo_plan(65, 66, 5, 5, 5, 0, 0, plan) == -1


def test_patch_rows_for_the_transform():
    from libdmet_preview_amd import patch
    from libdmet_preview_amd.solver import scf
    rows = [(o, r, n) for o, r, n in patch.binding_table() if n in ("incore_transform", "ao2mo_Ham")]
    assert sorted(rows) == [("solver.scf", "solver.scf", "ao2mo_Ham"), ("solver.scf", "solver.scf", "incore_transform")]
    assert all(callable(getattr(scf, n)) for _, _, n in rows)
