"""
FCI on the device (csrc/fci.hip) at the shapes where its kernels change behaviour, and on state left behind.  The
constants of fci.hip: NT = 256 threads, RED_GRID = 512 workgroups of a reduction, LDS_NB = 4096 staged beta strings, at most 8
y-blocks.  Bounds, handle and checker are those of tests/test_gpu_fci.py; references are tests/fci_ref.py.

1 Wide        sigma, diagonal, gamma, Gamma of a GIVEN random vector, element by element within (2 K + 64) eps S, repeats bit-identical:
              (11,2,5) Nb = 462: two y-blocks, the second partial;  (14,1,6) Nb = 3003: eight y-blocks, a second stride pass with a
              partial tail, the row still staged in LDS;  (15,1,6) Nb = 5005: the unstaged gather, three stride passes, 75075 > 65536
              determinants, whole and in slabs of 4 alpha rows (4, 4, 4, 3);  (15,6,1): 5005 workgroups in x, alpha link lists of 60,
              slabs of 2048 rows.  One Davidson step from the given vector at 75075 determinants (reduction grid 294: the second pass
              of fci_dotsum_kernel) against the reference's Rayleigh quotient and residual norm.
              Reference (matvec twice, densities twice, on the CPU, once per case): 0.9 / 0.7 s at (11,2,5), 2.3 s at (14,1,6), 5.0 s
              at (15,1,6) for each spin form, 5.2 s at (15,6,1).
2 Solvable    152460 determinants (11,4,5), reduction grids at their cap of 512 with a grid-stride pass: fci_ref.Solvable, a
              Hamiltonian of commuting terms whose ground state is a product of two Slater determinants (gap 0.275 / 0.268): diagonal,
              argmin, converged Davidson, E within 1e-10, residual by the matrix-form product, gamma against U occ U^T, sum rules and
              energy of Gamma, second run bit-identical.
3 Tiny        1, 4 and 9 determinants, max_space 12 (the basis exhausts the space) and 2 (collapse), H and 1000 H: converged, exact
              energy and densities, at most Ndet + 1 iterations; FCI.run on two orbitals.
4 Collapse    run(max_space = 2, 3, 5) on a handle of 12: the same ground state, bit-identical repeats; max_space 12 from there: <= 2.
5 Stale       outputs pre-filled with NaN; the two layouts of the workspace D (n^2 + 1 rows for spin-1 sigma, 2 n^2 + 1 for the Gram
              product) one after the other on one handle: every result carries the bits of a fresh handle.
Measured      on one MI355X (profiles/fci_notes.txt, section 5).  Largest fraction of the bound over all elements:
                  (n, na, nb)  spin  Na x Nb     slabs   hdiag    sigma    rdm1     rdm2
                  (11, 2, 5)    1    55 x 462      1     0.0025   0.0013   0.0007   0.0004
                  (11, 2, 5)    2    55 x 462      1     0.0042   0.0012   0.0007   0.0005
                  (14, 1, 6)    2    14 x 3003     1     0.0025   0.0010   0.0004   0.0004
                  (15, 1, 6)    1    15 x 5005     1     0.0020   0.0008   0.0002   0.0002
                  (15, 1, 6)    2    15 x 5005     4     0.0019   0.0008   0.0001   0.0001
                  (15, 6, 1)    2    5005 x 15     3     0.0026   0.0008   0.0001   0.0001
              One step at 75075: theta 2.2e-16 from the reference (bound 1.8e-9), |r| 4.4e-16 (bound 1.0e-10), the vector unchanged.
              Iterations, the device and fci_ref.davidson (the numpy restatement of the device loop) alike; max_iter of every run
              here is twice the restatement's count:
                  solvable (11,4,5): 46 restricted, 41 unrestricted; |E - E_exact| = 1.4e-13 / 1.1e-13, |r| = 5.8e-11 / 7.2e-11
                  tiny, max_space 12 / 2: dimer 2 / 2, dimer_field 4 / 53, two 3 / 9, two_u 4 / 12, three 6 / 22, three_u 9 / 27,
                      one determinant 1 / 1; the same for 1000 H.  Before the exit on an exhausted space took the residual as its
                      test, dimer, dimer_field, two, two_u and three reported converged = 0 at |r| <= 1e-15 (the device and the
                      restatement alike), and FCI.run on two orbitals logged "converged: False" at the exact energy.
                  collapse, max_space 2 / 3 / 5: sys6 51 / 35 / 28, sys6u 146 / 76 / 51, ring6 68 / 46 / 34; then 1 at max_space 12
"""
import functools

import numpy as np
import pytest

from tests import fci_ref as F
from tests.test_gpu_fci import DMK_OK, EPS, TOL_E, TOL_R, Handle, _case, _check_kernels, _dm2_of, _frac, _hdiag_scale, bound, ctx, plan  # noqa: F401

pytestmark = pytest.mark.gpu


def _budget(n, na, nb, spin, rows, max_space=2):
    fixed, per_row, ndet = plan(n, na, nb, spin, max_space)
    return fixed + rows * per_row


# ---- 1. wide strings ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,na,nb,spin,rows", [(11, 2, 5, 1, None), (11, 2, 5, 2, None), (14, 1, 6, 2, None), (15, 1, 6, 1, None), (15, 1, 6, 2, 4),
                                                (15, 6, 1, 2, 2048)])
def test_wide_strings_on_a_given_vector(ctx, n, na, nb, spin, rows):
    if rows is None:
        _check_kernels(ctx, n, na, nb, spin)
    else:
        _check_kernels(ctx, n, na, nb, spin, max_bytes=_budget(n, na, nb, spin, rows), want_rows=rows)


def test_one_davidson_step_at_75075_determinants(ctx):
    """run(max_iter = 1) from the given vector: normalise (fci_dot + fci_dotsum over 294 partial sums), H c, theta = c . H c, |H c - theta c|."""
    n, na, nb, spin = 15, 1, 6, 1
    sp, h1, eri, c, ref = _case(n, na, nb, spin)
    assert sp.ndet == 75075 and -(-sp.ndet // 256) == 294
    h = Handle(ctx, n, na, nb, spin, h1, eri)
    assert h.rc == DMK_OK
    try:
        h.set(c)
        res = h.run(max_iter=1, max_space=2)
        back = h.get(0)
    finally:
        h.close()
    sig, S = ref["sigma"], ref["sigma_s"]
    theta = float(c @ sig)
    b_theta = bound(sp.ndet, float(np.abs(c) @ S))
    rvec = sig - theta * c
    rn = float(np.linalg.norm(rvec))
    delta = bound(2 * n * n, S) + np.abs(c) * abs(res["e"] - theta)
    b_r = float(np.linalg.norm(delta)) + (2 * sp.ndet + 64) * EPS * rn
    print("one step at %d determinants: theta %.15f (reference %.15f, |d| = %.2e of %.2e), |r| %.15f (reference %.15f, |d| = %.2e of %.2e), "
          "vector |d| / (eps |c|) <= %.2f" % (sp.ndet, res["e"], theta, abs(res["e"] - theta), b_theta, res["r"], rn, abs(res["r"] - rn), b_r,
                                             float(np.max(np.abs(back - c) / (EPS * np.abs(c))))))
    assert res["converged"] == 0 and res["iterations"] == 1 and res["de"] == 0.0
    assert abs(res["e"] - theta) <= b_theta
    assert abs(res["r"] - rn) <= b_r
    assert np.all(np.abs(back - c) <= 4 * EPS * np.abs(c))


# ---- 2. an exactly solvable Hamiltonian at 152460 determinants -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solvable_case(unrestricted):
    S = F.solvable(11, 4, 5, unrestricted)
    sp = F.Space(11, 4, 5)
    hd = sp.hdiag(S.h1, S.eri)
    return S, sp, hd, _hdiag_scale(sp, S.h1, S.eri), F.davidson(S.matvec, hd)["iterations"]


@pytest.mark.parametrize("spin", [1, 2])
def test_solvable_hamiltonian_at_152460_determinants(ctx, spin):
    S, sp, hd, hd_s, count = _solvable_case(spin == 2)
    n, N = sp.n, sp.na + sp.nb
    assert sp.ndet == 152460 and sp.ndet > 512 * 256 and S.gap >= 1e-2
    h = Handle(ctx, n, sp.na, sp.nb, spin, S.h1, S.eri, max_space=12)
    assert h.rc == DMK_OK
    try:
        hd_dev, start = h.get(1), h.get(0)
        res = h.run(max_iter=2 * count)
        c = h.get(0)
        g1, dm2 = h.rdm1(), h.rdm2()
        h.set(start)
        res2 = h.run(max_iter=2 * count)
        c2 = h.get(0)
    finally:
        h.close()
    fr = _frac(hd_dev, hd, hd_s, 2 * n * n + n)
    two = np.partition(hd, 1)[:2]
    at = int(np.argmin(hd))
    assert two[1] - two[0] > 2 * bound(2 * n * n + n, hd_s.max())          # the index of the minimum does not depend on rounding
    resid = float(np.linalg.norm(S.matvec(c) - res["e"] * c))
    tol_d = 4.0 * res["r"] / S.gap + 1e-12
    d1 = float(np.abs(g1 - S.ground_rdm1()).max())
    ga, gb = g1
    if spin == 1:
        rules = [np.einsum("pqrr->pq", dm2[0]) - (N - 1) * (ga + gb)]
        e_rdm = float(np.sum(S.h1[0] * (ga + gb)) + 0.5 * np.sum(S.eri[0] * dm2[0]))
    else:
        rules = [np.einsum("pqrr->pq", dm2[0]) - (sp.na - 1) * ga, np.einsum("pqrr->pq", dm2[1]) - sp.nb * ga,
                 np.einsum("rrpq->pq", dm2[1]) - sp.na * gb, np.einsum("pqrr->pq", dm2[2]) - (sp.nb - 1) * gb]
        e_rdm = F.energy_from_rdm(S.h1, S.eri, g1, dm2)
    d_rule = max(float(np.abs(x).max()) for x in rules)
    # |dE| <= sum |coefficient| |d density|: the density tolerance times the sum of the |integrals| that multiply the densities
    weight = float(np.abs(S.h1).sum() + 0.5 * np.abs(S.eri[0]).sum() + np.abs(S.eri[1]).sum() + 0.5 * np.abs(S.eri[2]).sum())
    print("solvable (11, 4, 5) spin %d: hdiag %.4f of the bound, %d iterations (restatement %d), E = %.13f (exact %.13f, |d| = %.2e), |r| = %.2e "
          "(matrix form: %.2e), gap %.3f, rdm1 %.2e of %.2e, sum rules %.2e of %.2e, E(rdm) - E = %.2e of %.2e"
          % (spin, fr, res["iterations"], count, res["e"], S.e0, abs(res["e"] - S.e0), res["r"], resid, S.gap, d1, tol_d, d_rule, n * tol_d,
             abs(e_rdm - res["e"]), weight * tol_d))
    assert fr <= 1.0
    assert start[at] == 1.0 and np.count_nonzero(start) == 1
    assert res["converged"] == 1 and res["r"] < TOL_R and abs(res["de"]) < TOL_E
    assert abs(res["e"] - S.e0) <= 1e-10
    assert resid <= 2 * TOL_R
    assert abs(np.linalg.norm(c) - 1.0) <= 1e-13
    assert d1 <= tol_d
    assert d_rule <= n * tol_d
    assert abs(e_rdm - res["e"]) <= weight * tol_d
    assert res2 == res and np.array_equal(c, c2)


# ---- 3. tiny spaces --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("name", sorted(F.TINY_CASES))
def test_tiny_spaces_converge(ctx, name, scale):
    """Ndet <= max_space: the basis exhausts the space (or the symmetry sector of the start), the residual vanishes on that step while
    dE is still the last real change.  `scale`: the whole Hamiltonian and both tolerances times 1000 -- the exhaustion test of the
    loop is an absolute 1e-14 on the correction, which does not scale with H."""
    sp, h1, eri, h0, w, v = F.tiny_case(name, scale)
    spin = F.TINY_CASES[name][4]
    tol_e, tol_r = TOL_E * scale, TOL_R * scale
    gap = float(w[1] - w[0]) if sp.ndet > 1 else np.inf
    assert gap >= 1e-2 * scale
    c0 = v[:, 0]
    g1_ref, dm2_ref = sp.rdm1(c0), _dm2_of(spin, sp.rdm2(c0))
    H, hd = sp.dense(h1, eri), sp.hdiag(h1, eri)
    h = Handle(ctx, sp.n, sp.na, sp.nb, spin, h1, eri, h0=h0, max_space=12)
    assert h.rc == DMK_OK
    out = []
    try:
        start = h.get(0)
        for ms in (12, 2):
            count = F.davidson(H, hd, max_space=ms, tol_e=tol_e, tol_r=tol_r)["iterations"]
            h.set(start)
            res = h.run(max_iter=2 * count, tol_e=tol_e, tol_r=tol_r, max_space=ms)
            out.append((ms, count, res, h.get(0), h.rdm1(), h.rdm2()))
    finally:
        h.close()
    for ms, count, res, c, g1, dm2 in out:
        tol_d = 4.0 * res["r"] / gap + 1e-12
        d1, d2 = float(np.abs(g1 - g1_ref).max()), float(np.abs(dm2 - dm2_ref).max())
        print("%s x %g, %d determinants, max_space %d: converged %d in %d iterations (restatement %d), E - E_ref = %.2e, |r| = %.2e, dE = %.2e, "
              "density errors %.2e / %.2e of %.2e" % (name, scale, sp.ndet, ms, res["converged"], res["iterations"], count,
                                                      res["e"] - w[0] - h0, res["r"], res["de"], d1, d2, tol_d))
        assert res["converged"] == 1
        assert res["r"] < tol_r
        assert abs(res["e"] - (w[0] + h0)) <= 1e-10 * scale
        if ms == 12:
            assert res["iterations"] <= sp.ndet + 1
        assert abs(np.linalg.norm(c) - 1.0) <= 1e-13
        assert d1 <= tol_d and d2 <= tol_d


def test_fci_solver_on_two_orbitals(ctx):
    """the single-site DMET impurity: two orbitals, two electrons, four determinants"""
    from libdmet_preview_amd.solver import fci
    from libdmet_preview_amd.system import integral
    n = 2
    h1, eri = F.hubbard_ring(n, 4.0)
    h = h1[0] + np.diag([0.1, -0.1])
    i, j = np.tril_indices(n)
    g4 = eri[0][i, j][:, i, j]
    Ham = integral.Integral(n, True, False, 0.375, {"cd": h[None].copy()}, {"ccdd": g4[None].copy()})
    e_ref = 0.375 + np.linalg.eigvalsh(F.Space(n, 1, 1).dense(np.asarray([h, h]), eri))[0]
    solver = fci.FCI(restricted=True, tol=TOL_E, tol_residual=TOL_R)
    try:
        onepdm, E = solver.run(Ham, nelec=2)
        print("two orbitals: E = %.13f (reference %.13f), converged %s in %d iterations, |r| = %.2e"
              % (E, e_ref, solver.cisolver.converged, solver.cisolver.iterations, solver.cisolver.residual))
        assert solver.cisolver.converged is True
        assert abs(E - e_ref) <= 1e-10
    finally:
        solver.cleanup()


# ---- 4. small subspaces and collapse ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 5])
@pytest.mark.parametrize("name", sorted(F.COLLAPSE_COUNTS))
def test_small_subspaces_collapse_to_the_same_state(ctx, name, m):
    sp, h1, eri, h0, e0, gap, c0 = F.solver_case(name)
    spin = F.SOLVER_CASES[name][4]
    count = F.COLLAPSE_COUNTS[name][m]
    h = Handle(ctx, sp.n, sp.na, sp.nb, spin, h1, eri, h0=h0, max_space=12)
    assert h.rc == DMK_OK
    try:
        start = h.get(0)
        res = h.run(max_iter=2 * count, max_space=m)
        c = h.get(0)
        h.set(start)
        res2 = h.run(max_iter=2 * count, max_space=m)
        c2 = h.get(0)
        more = h.run(max_space=12)
    finally:
        h.close()
    resid = float(np.linalg.norm(sp.matvec(h1, eri, c) - (res["e"] - h0) * c))
    print("%s, max_space %d of 12: %d iterations (restatement %d), |E - E_ref| = %.2e, |r| = %.2e (reference matvec: %.2e); max_space 12 from "
          "there: %d iteration(s)" % (name, m, res["iterations"], count, abs(res["e"] - e0 - h0), res["r"], resid, more["iterations"]))
    assert res["converged"] == 1 and res["r"] < TOL_R and abs(res["de"]) < TOL_E
    assert abs(res["e"] - (e0 + h0)) <= 1e-10
    assert resid <= 2 * TOL_R
    assert abs(np.linalg.norm(c) - 1.0) <= 1e-13
    assert res2 == res and np.array_equal(c, c2)
    assert more["converged"] == 1 and more["iterations"] <= 2 and abs(more["e"] - (e0 + h0)) <= 1e-10


# ---- 5. stale workspace and poisoned outputs ---------------------------------------------------------------------------------------------
class PoisonedHandle(Handle):
    """every output buffer holds NaN before the call that fills it"""

    def _nan(self, shape):
        return self.ctx.to_device(np.full(shape, np.nan))

    def get(self, what=0):
        d = self._nan((self.ndet,))
        self.ctx.check(self.lib.dmk_fci_get(self.h, what, d.ptr))
        out = d.get()
        d.free()
        return out

    def sigma(self, c):
        dc, ds = self.ctx.to_device(c), self._nan((self.ndet,))
        self.ctx.check(self.lib.dmk_fci_sigma(self.h, dc.ptr, ds.ptr))
        out = ds.get()
        dc.free(), ds.free()
        return out

    def rdm1(self):
        d = self._nan((2, self.n, self.n))
        self.ctx.check(self.lib.dmk_fci_rdm1(self.h, d.ptr))
        out = d.get()
        d.free()
        return out

    def rdm2(self):
        n = self.n
        d = self._nan((1 if self.spin == 1 else 3, n, n, n, n))
        self.ctx.check(self.lib.dmk_fci_rdm2(self.h, d.ptr))
        out = d.get()
        d.free()
        return out


@pytest.mark.parametrize("rows", [None, 7])
@pytest.mark.parametrize("spin", [1, 2])
@pytest.mark.parametrize("n,na,nb", [(6, 3, 3), (6, 5, 1)])
def test_outputs_that_hold_nan_are_overwritten(ctx, n, na, nb, spin, rows):
    sp, h1, eri, c, ref = _case(n, na, nb, spin)
    h = PoisonedHandle(ctx, n, na, nb, spin, h1, eri, max_bytes=0 if rows is None else _budget(n, na, nb, spin, rows))
    assert h.rc == DMK_OK
    try:
        assert (h.rows, h.slabs) == ((sp.Na, 1) if rows is None else (min(rows, sp.Na), -(-sp.Na // min(rows, sp.Na))))
        hd, sig = h.get(1), h.sigma(c)
        h.set(c)
        back, g1, dm2 = h.get(0), h.rdm1(), h.rdm2()
    finally:
        h.close()
    for x in (hd, sig, back, g1, dm2):
        assert np.all(np.isfinite(x))
    assert np.array_equal(back, c)
    assert _frac(hd, ref["hdiag"], _hdiag_scale(sp, h1, eri), 2 * n * n + n) <= 1.0
    assert _frac(sig, ref["sigma"], ref["sigma_s"], 2 * n * n) <= 1.0
    assert _frac(g1, ref["g1"], ref["g1_s"], sp.ndet) <= 1.0
    assert _frac(dm2, _dm2_of(spin, ref["dm2"]), _dm2_of(spin, ref["dm2_s"]), sp.ndet) <= 1.0


@pytest.mark.parametrize("spin", [1, 2])
def test_one_workspace_in_two_layouts(ctx, spin):
    """sigma (D of n^2 + 1 rows on one spin block), the Gram product (2 n^2 + 1 rows) and the Davidson loop one after the other on one
    handle, three slabs: nothing of an earlier call shows in a later one."""
    n, na, nb = 6, 3, 3
    sp, h1, eri, c1, ref = _case(n, na, nb, spin)
    c2 = np.random.default_rng(99).standard_normal(sp.ndet)
    c2 /= np.linalg.norm(c2)
    mb = _budget(n, na, nb, spin, 7)
    fresh = Handle(ctx, n, na, nb, spin, h1, eri, max_bytes=mb)
    assert fresh.rc == DMK_OK
    try:
        assert fresh.rows == 7 and fresh.slabs == 3
        want_sig = fresh.sigma(c2)
        fresh.set(c2)
        want_g1, want_dm2 = fresh.rdm1(), fresh.rdm2()
    finally:
        fresh.close()
    h = Handle(ctx, n, na, nb, spin, h1, eri, max_bytes=mb)
    assert h.rc == DMK_OK
    try:
        own = h.get(0)
        h.sigma(c1)
        assert np.array_equal(h.get(0), own)          # sigma of a given vector leaves the handle's own alone
        h.set(c1)
        h.rdm2()
        s_a = h.sigma(c2)
        assert np.array_equal(h.get(0), c1)
        h.run(max_iter=3, max_space=2)
        s_b = h.sigma(c2)
        h.set(c2)
        g1, dm2 = h.rdm1(), h.rdm2()
    finally:
        h.close()
    assert np.array_equal(s_a, want_sig) and np.array_equal(s_b, want_sig)
    assert np.array_equal(g1, want_g1) and np.array_equal(dm2, want_dm2)
    assert _frac(want_sig, sp.matvec(h1, eri, c2), sp.matvec(h1, eri, c2, True), 2 * n * n) <= 1.0
