"""
CPU-only checks of the FCI layer: the numpy reference of tests/fci_ref.py against independent exact
diagonalisations, identities of the exact densities, the conditions the GPU tests rely on, the plan formula of dmk_fci_plan and the
refusals of solver/fci.py.
"""
import ctypes as C
from math import comb

import numpy as np
import pytest

from tests import ccsd_t_ref as TR
from tests import cclambda_ref as LR
from tests import fci_ref as F
from tests import scf_ref as R


@pytest.mark.parametrize("n,npair,seed", [(4, 2, 5), (5, 2, 6), (5, 3, 7)])
def test_reference_against_the_kron_built_hamiltonian(n, npair, seed):
    """ccsd_t_ref.fci_energy builds H from dense E_pq matrices and Kronecker products: another route to the same spectrum."""
    h1, eri = F.factored(n, seed, False, 1.0)
    sp = F.Space(n, npair, npair)
    H = sp.dense(h1, eri)
    assert abs(np.linalg.eigvalsh(H)[0] - TR.fci_energy(h1[0], eri[0], npair)) <= 1e-12
    assert np.abs(np.diag(H) - sp.hdiag(h1, eri)).max() <= 1e-13


@pytest.mark.parametrize("n,seed", [(3, 1), (5, 2)])
def test_reference_against_the_two_electron_problem(n, seed):
    """one alpha and one beta electron: the string index is the orbital, c[Ia][Ib] the spatial wave function"""
    sysm = R.System(n, seed, [1])
    e_ref, x_ref = LR.fci_two_electron(sysm)
    g = sysm.lam * np.einsum("Pij,Pkl->ijkl", sysm.A, sysm.A)
    sp = F.Space(n, 1, 1)
    w, v = np.linalg.eigh(sp.dense(np.asarray([sysm.h1, sysm.h1]), (g, g, g)))
    k = [i for i in range(n * n) if np.abs(v[:, i].reshape(n, n) - v[:, i].reshape(n, n).T).max() < 1e-8][0]
    assert abs(w[k] - e_ref) <= 1e-12
    assert min(np.abs(v[:, k].reshape(n, n) - s * x_ref).max() for s in (1, -1)) <= 1e-8
    g1 = sp.rdm1(v[:, k])
    assert np.abs(g1[0] - x_ref @ x_ref.T).max() <= 1e-8 and np.abs(g1[1] - x_ref.T @ x_ref).max() <= 1e-8


@pytest.mark.parametrize("n,na,nb,unrestricted", [(4, 2, 2, False), (4, 2, 1, True), (5, 3, 1, True), (4, 4, 0, False)])
def test_densities_of_the_reference(n, na, nb, unrestricted):
    """the Gram form of dm2 against the four operators applied one after the other; energy from the densities; sum rules"""
    h1, eri = F.factored(n, 40 + n + na, unrestricted)
    sp = F.Space(n, na, nb)
    w, v = np.linalg.eigh(sp.dense(h1, eri))
    rng = np.random.default_rng(n)
    for c in (v[:, 0], rng.standard_normal(sp.ndet)):
        c = c / np.linalg.norm(c)
        g1, g2 = sp.rdm1(c), sp.rdm2(c)
        assert np.abs(g2 - sp.rdm2_direct(c)).max() <= 1e-13
        assert abs(F.energy_from_rdm(h1, eri, g1, g2) - c @ sp.matvec(h1, eri, c)) <= 1e-12
        N, G, g = na + nb, F.spin_summed(g2), g1[0] + g1[1]
        assert np.abs(np.einsum("pqrr->pq", G) - (N - 1) * g).max() <= 1e-13
        assert np.abs(np.einsum("pqrr->pq", g2[0]) - (na - 1) * g1[0]).max() <= 1e-13
        assert np.abs(np.einsum("pqrr->pq", g2[1]) - nb * g1[0]).max() <= 1e-13
        assert np.all(sp.rdm1(c, True) >= np.abs(g1) - 1e-15) and np.all(sp.rdm2(c, True) >= np.abs(g2) - 1e-15)
        assert np.all(sp.matvec(h1, eri, c, True) >= np.abs(sp.matvec(h1, eri, c)) - 1e-15)


@pytest.mark.parametrize("name", ["sys4", "sys6", "ring6"])
def test_closed_shell_ground_states_are_singlets(name):
    """<S^2> = -N (N - 4) / 4 - 1/2 sum_pq Gamma_pqqp = 0 for the spin-summed Gamma of a closed-shell ground state"""
    sp, h1, eri, h0, e0, gap, c0 = F.solver_case(name)
    N = sp.na + sp.nb
    G = F.spin_summed(sp.rdm2(c0))
    assert abs(-N * (N - 4) / 4.0 - 0.5 * np.einsum("pqqp->", G)) <= 1e-12
    assert np.abs(np.einsum("pqrr->pq", G) - (N - 1) * (sp.rdm1(c0)[0] + sp.rdm1(c0)[1])).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(F.SOLVER_CASES))
def test_solver_cases_have_a_gap_and_a_reachable_start(name):
    """what tests/test_gpu_fci.py relies on: gap >= 1e-2, and the lowest-diagonal determinant overlaps with the ground state"""
    sp, h1, eri, h0, e0, gap, c0 = F.solver_case(name)
    assert gap >= 1e-2
    assert np.linalg.norm(sp.matvec(h1, eri, c0) - e0 * c0) <= 1e-9
    hd = sp.hdiag(h1, eri)
    assert abs(c0[int(np.argmin(hd))]) >= 1e-3


def _plan(n, na, nb, spin, ms):
    from libdmet_preview_amd._lib import lib
    b = (C.c_int64 * 3)()
    return lib.dmk_fci_plan(n, na, nb, spin, ms, b), [int(x) for x in b]


@pytest.mark.parametrize("n,na,nb", [(1, 1, 0), (6, 3, 3), (10, 5, 3), (14, 7, 7), (16, 8, 8), (32, 2, 1)])
@pytest.mark.parametrize("spin", [1, 2])
def test_plan_formula(n, na, nb, spin):
    a256 = lambda x: (x + 255) // 256 * 256
    for ms in (2, 12, 16):
        rc, (fixed, per_row, ndet) = _plan(n, na, nb, spin, ms)
        Na, Nb, n2 = comb(n, na), comb(n, nb), n * n
        assert rc == 0 and ndet == Na * Nb
        assert per_row == ((2 * n2 + 1) + spin * n2) * Nb * 8                 # the columns of D and of G of one alpha row
        la, lb = max(na * (n - na + 1), 1), max(nb * (n - nb + 1), 1)
        want = (3 + 2 * ms) * a256(ndet * 8)
        want += a256(n2 * Na * 4) + 2 * a256(la * Na * 4) + a256(Na * 4) + a256(n2 * Nb * 4) + 2 * a256(lb * Nb * 4) + a256(Nb * 4)
        want += a256(spin * n2 * (spin * n2 + 1) * 8) + a256((2 * n2 + 1) ** 2 * 8) + a256((2 * n + 3 * n2) * 8) + a256(512 * 17 * 16) + 4096
        assert fixed == want
    if (n, na, nb) == (14, 7, 7):
        assert abs(per_row * Na / 1e9 - (55.5 if spin == 1 else 74.0)) < 0.1          # D and G of the whole space: slabs are not optional


def test_plan_refusals():
    for bad in ((0, 0, 0, 1, 12), (33, 1, 1, 1, 12), (6, 7, 1, 1, 12), (6, -1, 1, 1, 12), (6, 3, 3, 0, 12), (6, 3, 3, 3, 12), (6, 3, 3, 1, 1),
                (6, 3, 3, 1, 17), (32, 16, 16, 1, 12)):
        assert _plan(*bad)[0] == -1, bad
    from libdmet_preview_amd._lib import lib
    assert lib.dmk_fci_plan(6, 3, 3, 1, 12, None) == -1


def test_solver_refusals_and_import_without_a_gpu():
    from libdmet_preview_amd.solver import fci
    from libdmet_preview_amd.system import integral
    for kw in (dict(ghf=True), dict(bcs=True), dict(nproc=2), dict(nnode=2), dict(compact_rdm2=True), dict(something_else=1)):
        with pytest.raises(NotImplementedError):
            fci.FCI(**kw)
    with pytest.raises(NotImplementedError):
        fci.FCI_AO()
    s = fci.FCI()
    assert s.restricted is False and s.Sz == 0 and s.conv_tol == 1e-10 and s.cisolver.max_cycle == 200
    n = 4
    Ham = integral.Integral(n, True, False, 0.0, {"cd": np.zeros((1, n, n))}, {"ccdd": np.zeros((1, 10, 10))})
    for kw in (dict(Mu=0.1), dict(pspace_size=400), dict(mo_coeff_custom=np.eye(n)), dict(mo_energy_custom=np.zeros(n)),
               dict(mo_occ_custom=np.zeros(n))):
        with pytest.raises(NotImplementedError):
            s.run(Ham, nelec=4, **kw)
    with pytest.raises(ValueError):
        s.run(Ham)
    with pytest.raises(RuntimeError):
        s.run_dmet_ham(Ham)
    with pytest.raises(RuntimeError):
        s.cisolver.make_rdm1()
    with pytest.raises(NotImplementedError):
        fci.DeviceFCI().kernel(np.zeros((n, n)), np.zeros((n, n, n, n)), n, 4, pspace_size=10)
    assert fci.plan_bytes(6, 6, 1, 12) == fci.plan_bytes(6, (3, 3), 1, 12) and fci.plan_bytes(5, 5, 2, 12)[2] == comb(5, 3) * comb(5, 2)
    with pytest.raises(ValueError):
        fci.plan_bytes(40, 2, 1, 12)
    s.cleanup()


def test_molecular_density_transforms():
    from libdmet_preview_amd.basis_transform import make_basis as mb
    rng = np.random.default_rng(3)
    n = 4
    C = rng.standard_normal((2, n, n))
    g1 = rng.standard_normal((2, n, n))
    g2 = rng.standard_normal((3, n, n, n, n))
    assert np.abs(mb.transform_rdm1_to_ao_mol(g1, C)[1] - C[1] @ g1[1] @ C[1].T).max() <= 1e-13
    assert np.abs(mb.transform_rdm1_to_ao_mol(g1[0], C[0]) - C[0] @ g1[0] @ C[0].T).max() <= 1e-13
    assert mb.transform_rdm1_to_ao_mol(g1[:1], C[0]).shape == (1, n, n) and mb.transform_rdm1_to_ao_mol(g1, C[0]).shape == (2, n, n)
    out = mb.transform_rdm2_to_ao_mol(g2, C)
    h = rng.standard_normal((n, n, n, n))
    # sum_pqrs h_pqrs G^AO_pqrs = sum_ijkl (h transformed to the MO basis)_ijkl G^MO_ijkl
    for b, (x, y) in enumerate(((0, 0), (0, 1), (1, 1))):
        hmo = np.einsum("pqrs,pi,qj,rk,sl->ijkl", h, C[x], C[x], C[y], C[y], optimize=True)
        assert abs(np.sum(h * out[b]) - np.sum(hmo * g2[b])) <= 1e-10
    assert np.abs(mb.transform_rdm2_to_ao_mol(g2[:1], C[0])[0] - mb.transform_rdm2_to_ao_mol(g2[0], C[0])).max() == 0.0
    with pytest.raises(ValueError):
        mb.transform_rdm2_to_ao_mol(g2[:2], C)


# ---- the references of tests/test_gpu_fci_edges.py ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("unrestricted", [False, True])
def test_solvable_hamiltonian_against_dense(unrestricted):
    """the occupation-pattern spectrum against eigvalsh of the operator-built H; the product of minors is the ground vector"""
    S = F.solvable(5, 2, 3, unrestricted)
    sp = F.Space(5, 2, 3)
    H = sp.dense(S.h1, S.eri)
    assert np.abs(np.linalg.eigvalsh(H) - S.spectrum()).max() <= 1e-12
    c = S.ground_vector()
    assert abs(np.linalg.norm(c) - 1.0) <= 1e-13 and np.linalg.norm(H @ c - S.e0 * c) <= 1e-12
    assert np.abs(sp.rdm1(c) - S.ground_rdm1()).max() <= 1e-13
    assert (not unrestricted and np.array_equal(S.h1[0], S.h1[1])) or (unrestricted and np.abs(S.h1[0] - S.h1[1]).max() > 1e-3)


@pytest.mark.parametrize("na,nb,unrestricted", [(3, 2, False), (2, 4, True), (6, 1, True)])
def test_solvable_matrix_form_product(na, nb, unrestricted):
    S = F.solvable(6, na, nb, unrestricted)
    sp = F.Space(6, na, nb)
    x = np.random.default_rng(na).standard_normal(sp.ndet)
    ref = sp.matvec(S.h1, S.eri, x)
    assert np.abs(S.matvec(x) - ref).max() <= 1e-12 * np.abs(sp.matvec(S.h1, S.eri, x, True)).max()
    c = S.ground_vector()
    assert np.linalg.norm(S.matvec(c) - S.e0 * c) <= 1e-12


@pytest.mark.parametrize("unrestricted", [False, True])
def test_solvable_case_of_the_gpu_test(unrestricted):
    """(11, 4, 5), 152460 determinants: what the device test relies on -- a gap, a start that overlaps, an eigenvector in closed form"""
    S = F.solvable(11, 4, 5, unrestricted)
    sp = F.Space(11, 4, 5)
    c = S.ground_vector()
    assert sp.ndet == 152460 and S.gap >= 1e-2
    assert abs(c[int(np.argmin(sp.hdiag(S.h1, S.eri)))]) >= 1e-3
    assert abs(np.linalg.norm(c) - 1.0) <= 1e-13 and np.linalg.norm(S.matvec(c) - S.e0 * c) <= 1e-11
    res = F.davidson(S.matvec, sp.hdiag(S.h1, S.eri))
    assert res["converged"] == 1 and abs(res["e"] - S.e0) <= 1e-10 and res["iterations"] <= 100


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("name", sorted(F.TINY_CASES))
def test_restated_davidson_on_tiny_spaces(name, scale):
    """the restatement of the device loop where the basis exhausts the space: converged, and the conditions of the device test"""
    sp, h1, eri, h0, w, v = F.tiny_case(name, scale)
    assert sp.ndet <= 12 and (sp.ndet == 1 or w[1] - w[0] >= 1e-2 * scale)
    H, hd = sp.dense(h1, eri), sp.hdiag(h1, eri)
    assert abs(v[int(np.argmin(hd)), 0]) >= 1e-3
    for ms in (12, 2):
        res = F.davidson(H, hd, max_space=ms, tol_e=1e-12 * scale, tol_r=1e-10 * scale)
        assert res["converged"] == 1 and res["r"] < 1e-10 * scale and abs(res["e"] - w[0]) <= 1e-10 * scale
        assert ms == 2 or res["iterations"] <= sp.ndet + 1


@pytest.mark.parametrize("name", sorted(F.COLLAPSE_COUNTS))
def test_restated_davidson_counts(name):
    """the iteration counts the device tests take their max_iter from (twice these); rounding may move one by a step or two"""
    sp, h1, eri, h0, e0, gap, c0 = F.solver_case(name)
    H, hd = sp.dense(h1, eri), sp.hdiag(h1, eri)
    for ms, want in F.COLLAPSE_COUNTS[name].items():
        res = F.davidson(H, hd, max_space=ms, max_iter=400)
        assert res["converged"] == 1 and abs(res["e"] - e0) <= 1e-10
        assert abs(res["iterations"] - want) <= 2, (ms, res["iterations"], want)
    assert F.davidson(H, hd, max_iter=5)["converged"] == 0 and F.davidson(H, hd, max_iter=0)["iterations"] == 0
