"""
The FCI impurity solver (libdmet/solver/fci.py :41-314 of the reference) on the device Hartree-Fock of solver/scf.py and the device
FCI of csrc/fci.hip, laid out like solver/cc_solver.py.

  DeviceFCI      the handle wrapper, shaped like PySCF's direct_spin1 / direct_uhf objects:
                   kernel(h1, eri, norb, nelec, ci0=None, ecore=0) -> (E, fcivec)     Davidson for the lowest root
                   sigma(c)                                       (H - ecore) c of the last kernel's Hamiltonian (contract_2e's role)
                   make_rdm1 / make_rdm1s / make_rdm2 / make_rdm12s                   densities of a vector (default: the last one)
                   converged, memory_plan(), close()
                 h1 (n, n) and eri (n, n, n, n) [or 4-fold packed]: one spin block; h1 (2, n, n) and eri = (aa, ab, bb): three.
                 dm2[p, q, r, s] = <p+ r+ s q> (PySCF's convention).
  FCI            run            :78-204    HF, the transformation to the HF orbitals, FCI, make_rdm1 -> (onepdm, E)
                 make_rdm2      :281-303   twopdm_mo (and twopdm with ao_repr): restricted (1, n, n, n, n) spin-summed; unrestricted
                                           aa, bb, ab
                 run_dmet_ham   :206-259   the energy of a scaled Hamiltonian from onepdm_mo / twopdm_mo (numpy on the host: n is small)

ghf, bcs, Mu, mo_*_custom, a pspace_size other than the default, FCI_AO and MPI are not built: each raises NotImplementedError by
name.  Convergence: |dE| < conv_tol and |r|_2 < conv_tol_residual (default sqrt(conv_tol), PySCF's rule); where the Davidson basis
exhausts the space (a handful of determinants) the residual alone decides.  The module imports without a GPU; the device context is
created by the first call that computes.
"""
import ctypes as C

import numpy as np

from libdmet_preview_amd.basis_transform.make_basis import transform_rdm1_to_ao_mol, transform_rdm2_to_ao_mol
from libdmet_preview_amd.solver import scf
from libdmet_preview_amd.system import integral
from libdmet_preview_amd.utils import logger as log

PSPACE_DEFAULT = 800


def _refuse(what):
    raise NotImplementedError("FCI: %s is not built (restricted and unrestricted FCI with the one- and two-particle densities only)" % what)


def _unpack_nelec(nelec):
    if isinstance(nelec, (int, np.integer)):
        nelec = int(nelec)
        return nelec - nelec // 2, nelec // 2
    na, nb = nelec
    return int(na), int(nb)


def plan_bytes(norb, nelec, spin, max_space):
    """(fixed bytes of a handle, bytes per alpha row in flight, determinants): dmk_fci_plan, host arithmetic."""
    from libdmet_preview_amd._lib import lib
    na, nb = _unpack_nelec(nelec)
    out = (C.c_int64 * 3)()
    if lib.dmk_fci_plan(int(norb), na, nb, int(spin), int(max_space), out) != 0:
        raise ValueError("dmk_fci_plan refuses norb = %d, nelec = (%d, %d), spin = %d, max_space = %d" % (norb, na, nb, spin, max_space))
    return int(out[0]), int(out[1]), int(out[2])


def _full_eri(g, n):
    """(n, n, n, n) of a 1-fold or 4-fold block"""
    g = np.asarray(g, dtype=np.float64)
    if g.shape == (n, n, n, n):
        return g
    npair = n * (n + 1) // 2
    if g.shape == (npair, npair):
        idx = np.zeros((n, n), dtype=np.int64)
        i, j = np.tril_indices(n)
        idx[i, j] = idx[j, i] = np.arange(npair)
        return g[idx.reshape(-1)][:, idx.reshape(-1)].reshape(n, n, n, n)
    raise ValueError("an ERI block of shape %s for %d orbitals (1-fold or 4-fold)" % (g.shape, n))


class DeviceFCI(object):
    def __init__(self, ctx=None):
        self._ctx, self._h, self._key = ctx, None, None
        self.max_cycle, self.conv_tol, self.conv_tol_residual, self.max_space = 200, 1e-10, None, 12
        self.max_memory = None          # MB of device memory for the handle; None: three quarters of what is free
        self.converged, self.eci, self.ci, self.iterations, self.residual = False, None, None, 0, None

    # ---- the handle ------------------------------------------------------------------------------------------------------------------
    def _context(self):
        if self._ctx is None:
            from libdmet_preview_amd._lib import get_ctx
            self._ctx = get_ctx()
        return self._ctx

    def memory_plan(self, norb, nelec, spin=1):
        """The figures of a handle for this problem and the budget it would get: fixed bytes, bytes per alpha row in flight,
        determinants, budget, alpha rows in flight and slabs per product H c.  MemoryError when fixed + one row exceed the budget."""
        fixed, per_row, ndet = plan_bytes(norb, nelec, spin, self.max_space)
        if self.max_memory is None:
            have, what = self._context().mem_info()[0] // 4 * 3, "three quarters of what is free on the device"
        else:
            have, what = int(float(self.max_memory) * (1 << 20)), "allowed by max_memory"
        na, nb = _unpack_nelec(nelec)
        if fixed + per_row > have:
            raise MemoryError("FCI with norb = %d, nelec = (%d, %d): %d determinants plan %d bytes of device memory (vector, diagonal, "
                              "%d Davidson vectors, link tables, integrals) and %d bytes per alpha row in flight; %d bytes are %s"
                              % (norb, na, nb, ndet, fixed, 2 * self.max_space, per_row, have, what))
        nrow = ndet // max(1, _nstr(norb, nb))
        rows = min(nrow, (have - fixed) // per_row)
        return dict(fixed=fixed, per_row=per_row, ndet=ndet, budget=have, rows=rows, slabs=-(-nrow // rows))

    def _create(self, h1, eri, norb, nelec, ecore):
        from libdmet_preview_amd._lib import lib, c_vp
        self.close()
        h1 = np.asarray(h1, dtype=np.float64)
        spin = 1 if h1.ndim == 2 else 2
        if h1.shape != ((norb, norb) if spin == 1 else (2, norb, norb)):
            raise ValueError("h1 of shape %s for %d orbitals" % (h1.shape, norb))
        blocks = [_full_eri(eri, norb)] if spin == 1 else [_full_eri(g, norb) for g in eri]
        if spin == 2 and len(blocks) != 3:
            raise ValueError("three ERI blocks (aa, ab, bb) go with h1 (2, n, n)")
        na, nb = _unpack_nelec(nelec)
        plan = self.memory_plan(norb, (na, nb), spin)          # MemoryError before anything is allocated
        ctx = self._context()
        d = [ctx.to_device(h1)] + [ctx.to_device(g) for g in blocks]
        h = c_vp()
        try:
            ctx.check(lib.dmk_fci_create(ctx.h, int(norb), na, nb, spin, d[0].ptr, d[1].ptr, d[2].ptr if spin == 2 else None,
                                         d[3].ptr if spin == 2 else None, float(ecore), int(self.max_space), int(plan["budget"]), C.byref(h)))
        finally:
            for x in d:
                x.free()
        self._h, self._key = h, (int(norb), na, nb, spin)
        self._shape = (_nstr(norb, na), _nstr(norb, nb))
        log.debug(0, "FCI: %d x %d determinants, %d alpha rows in flight (%d slabs)", self._shape[0], self._shape[1], plan["rows"], plan["slabs"])

    def close(self):
        if self._h is not None:
            from libdmet_preview_amd._lib import lib
            lib.dmk_fci_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self, norb=None, nelec=None):
        if self._h is None:
            raise RuntimeError("DeviceFCI: no Hamiltonian yet (kernel() first)")
        if norb is not None and nelec is not None and (int(norb),) + _unpack_nelec(nelec) != self._key[:3]:
            raise ValueError("DeviceFCI: (norb, nelec) = (%s, %s) is not the problem of the last kernel() %s" % (norb, nelec, self._key[:3]))
        return self._h

    def _set(self, c):
        from libdmet_preview_amd._lib import lib
        c = np.ascontiguousarray(c, dtype=np.float64)
        if c.size != self._shape[0] * self._shape[1]:
            raise ValueError("a vector of %d elements for %d x %d determinants" % (c.size, self._shape[0], self._shape[1]))
        ctx = self._context()
        d = ctx.to_device(c.reshape(-1))
        ctx.check(lib.dmk_fci_set(self._h, d.ptr))
        d.free()

    def _get(self, what=0):
        from libdmet_preview_amd._lib import lib
        ctx = self._context()
        d = ctx.empty((self._shape[0] * self._shape[1],), np.float64)
        ctx.check(lib.dmk_fci_get(self._h, what, d.ptr))
        out = d.get().reshape(self._shape)
        d.free()
        return out

    # ---- PySCF's interface -----------------------------------------------------------------------------------------------------------
    def kernel(self, h1, eri, norb, nelec, ci0=None, ecore=0, pspace_size=PSPACE_DEFAULT, **kwargs):
        """The lowest root of H = ecore + h1 + eri in the space of nelec = n | (na, nb) electrons -> (E, fcivec (Na, Nb)).  ci0: the
        start (default: the lowest-diagonal determinant)."""
        from libdmet_preview_amd._lib import lib
        if pspace_size != PSPACE_DEFAULT:
            _refuse("pspace_size = %r (the start is one determinant or ci0; only the default is accepted, and ignored)" % (pspace_size,))
        for name, val in kwargs.items():
            if val is not None:
                _refuse("%s=%r in DeviceFCI.kernel" % (name, val))
        self._create(h1, eri, norb, nelec, ecore)
        if ci0 is not None:
            self._set(ci0)
        tol_r = self.conv_tol_residual if self.conv_tol_residual is not None else np.sqrt(self.conv_tol)
        res = (C.c_double * 5)()
        self._context().check(lib.dmk_fci_run(self._h, int(self.max_cycle), float(self.conv_tol), float(tol_r), int(self.max_space), res))
        self.eci, self.converged, self.iterations, self.residual = float(res[0]), bool(res[1]), int(res[2]), float(res[3])
        self.ci = self._get()
        log.debug(0, "FCI: E = %.12f, converged %s in %d iterations, |r| = %.2e, dE = %.2e", self.eci, self.converged, self.iterations,
                  self.residual, res[4])
        return self.eci, self.ci

    def sigma(self, c, norb=None, nelec=None):
        """(H - ecore) c with the Hamiltonian of the last kernel(), shape of c."""
        from libdmet_preview_amd._lib import lib
        self._handle(norb, nelec)
        ctx = self._context()
        c = np.ascontiguousarray(c, dtype=np.float64)
        if c.size != self._shape[0] * self._shape[1]:
            raise ValueError("a vector of %d elements for %d x %d determinants" % (c.size, self._shape[0], self._shape[1]))
        dc, ds = ctx.to_device(c.reshape(-1)), ctx.empty((c.size,), np.float64)
        ctx.check(lib.dmk_fci_sigma(self._h, dc.ptr, ds.ptr))
        out = ds.get().reshape(c.shape)
        dc.free(), ds.free()
        return out

    def hdiag(self):
        return self._get(1)

    def _densities(self, fcivec, norb, nelec, two):
        from libdmet_preview_amd._lib import lib
        self._handle(norb, nelec)
        if fcivec is not None:
            self._set(fcivec)
        ctx, (n, _, _, spin) = self._context(), self._key
        d1 = ctx.empty((2, n, n), np.float64)
        ctx.check(lib.dmk_fci_rdm1(self._h, d1.ptr))
        g1 = d1.get()
        d1.free()
        if not two:
            return g1, None
        d2 = ctx.empty((1 if spin == 1 else 3, n, n, n, n), np.float64)
        ctx.check(lib.dmk_fci_rdm2(self._h, d2.ptr))
        g2 = d2.get()
        d2.free()
        return g1, g2

    def make_rdm1s(self, fcivec=None, norb=None, nelec=None):
        """(gamma_alpha, gamma_beta), gamma_pq = <p+ q>"""
        g1, _ = self._densities(fcivec, norb, nelec, False)
        return g1[0], g1[1]

    def make_rdm1(self, fcivec=None, norb=None, nelec=None):
        """the spin-traced one-particle density"""
        g1, _ = self._densities(fcivec, norb, nelec, False)
        return g1[0] + g1[1]

    def make_rdm2(self, fcivec=None, norb=None, nelec=None):
        """the spin-summed dm2[p, q, r, s] = <p+ r+ s q> (one spin block), or aa + ab + ba + bb of the three"""
        _, g2 = self._densities(fcivec, norb, nelec, True)
        return g2[0] if len(g2) == 1 else g2[0] + g2[1] + g2[1].transpose(2, 3, 0, 1) + g2[2]

    def make_rdm12s(self, fcivec=None, norb=None, nelec=None):
        """((gamma_a, gamma_b), (aa, ab, bb)): needs the three-block form (h1 (2, n, n))"""
        g1, g2 = self._densities(fcivec, norb, nelec, True)
        if len(g2) != 3:
            raise RuntimeError("make_rdm12s: the spin-resolved two-particle density needs a handle of three spin blocks (h1 of shape (2, n, n))")
        return (g1[0], g1[1]), (g2[0], g2[1], g2[2])


def _nstr(n, k):
    from math import comb
    return comb(int(n), int(k))


class FCI(object):
    def __init__(self, nproc=1, nnode=1, TmpDir="./tmp", SharedDir=None, restricted=False, Sz=0, bcs=False, tol=1e-10, max_cycle=200,
                 max_memory=None, compact_rdm2=False, scf_newton=True, ghf=False, alpha=None, beta=np.inf, tol_residual=None,
                 max_space=12, **kwargs):
        """max_memory: MB of DEVICE memory for the FCI handle (None: three quarters of what is free)."""
        for name, on in (("ghf", ghf), ("bcs", bcs), ("compact_rdm2", compact_rdm2)):
            if on:
                _refuse("%s=%r" % (name, on))
        if nproc * nnode > 1:
            _refuse("MPI (nproc * nnode > 1)")
        for name, on in kwargs.items():
            if on:
                _refuse("%s=%r" % (name, on))
        self.restricted, self.Sz, self.bcs, self.ghf = restricted, Sz, False, False
        self.alpha, self.beta, self.conv_tol, self.max_memory = alpha, beta, tol, max_memory
        self.cisolver = DeviceFCI()
        self.cisolver.max_memory, self.cisolver.max_cycle, self.cisolver.conv_tol = max_memory, max_cycle, tol
        self.cisolver.conv_tol_residual, self.cisolver.max_space = tol_residual, max_space
        self.scfsolver = scf.SCF(newton_ah=scf_newton)
        self.fcivec = self.onepdm = self.twopdm = self.onepdm_mo = self.twopdm_mo = None
        self.optimized = False

    def _unrestricted_ham(self, Ham):
        """a spin-independent Hamiltonian for the unrestricted solver: H1 doubled, the one ERI block serves aa, bb and ab"""
        if not Ham.restricted:
            return Ham
        H1 = np.asarray(Ham.H1["cd"], dtype=np.float64)
        return integral.Integral(Ham.norb, False, False, Ham.H0, {"cd": np.asarray([H1[0], H1[0]])}, {"ccdd": Ham.H2["ccdd"]},
                                 getattr(Ham, "ovlp", None))

    def _mo_ham(self, Ham):
        """Ham at the orbitals of the last mean field: (h1, h2) as the device FCI takes them (h2: one block, or aa, ab, bb)"""
        mo = np.asarray(self.scfsolver.mf.mo_coeff)
        if self.restricted:
            H = scf.ao2mo_Ham(Ham, mo, compact=False)
            return H, np.asarray(H.H1["cd"])[0], np.asarray(H.H2["ccdd"])[0]
        H = scf.ao2mo_Ham(self._unrestricted_ham(Ham), mo, compact=False)
        h2 = np.asarray(H.H2["ccdd"])          # aa, bb, ab
        return H, np.asarray(H.H1["cd"]), (h2[0], h2[2], h2[1])

    def run(self, Ham, nelec=None, guess=None, calc_rdm2=False, pspace_size=PSPACE_DEFAULT, Mu=None, **kwargs):
        """HF, FCI at the HF orbitals and the density -> (onepdm, E): onepdm (1, n, n) = half the spin-traced density (restricted) or
        (2, n, n) (unrestricted), in the basis of Ham.  guess: None, "random" or a vector (Na, Nb) in the HF orbitals of this run.
        kwargs: dm0, scf_max_cycle (200)."""
        log.info("FCI solver Run")
        if Mu is not None:
            _refuse("a chemical potential (Mu)")
        if pspace_size != PSPACE_DEFAULT:
            _refuse("pspace_size = %r (only the default is accepted, and ignored)" % (pspace_size,))
        for name in ("mo_energy_custom", "mo_occ_custom", "mo_coeff_custom"):
            if kwargs.get(name, None) is not None:
                _refuse(name)
        if Ham.bogoliubov:
            _refuse("a Bogoliubov Hamiltonian")
        spin = np.asarray(Ham.H1["cd"]).shape[0]
        if spin > 1:
            log.eassert(not self.restricted, "a spin-dependent Hamiltonian needs restricted=False")
        if nelec is None:
            raise ValueError("FCI solver: nelec cannot be None")
        nelec_a, nelec_b = (nelec + self.Sz) // 2, (nelec - self.Sz) // 2
        log.eassert(nelec_a >= 0 and nelec_b >= 0 and nelec_a + nelec_b == nelec, "nelec = %s and Sz = %s do not fit", nelec, self.Sz)
        self.nelec = (nelec_a, nelec_b)
        self.scfsolver.set_system(nelec, self.Sz, False, self.restricted)
        self.scfsolver.set_integral(Ham)
        E_HF, _ = self.scfsolver.HF(tol=min(1e-10, self.conv_tol * 0.1), MaxIter=kwargs.get("scf_max_cycle", 200),
                                    InitGuess=kwargs.get("dm0", None), alpha=self.alpha, beta=self.beta)
        log.debug(1, "FCI solver: mean-field converged: %s", self.scfsolver.mf.converged)
        HamMO, h1, h2 = self._mo_ham(Ham)
        if isinstance(guess, str):
            if guess != "random":
                raise ValueError("guess: None, 'random' or a vector")
            ci0 = np.random.random((_nstr(Ham.norb, nelec_a), _nstr(Ham.norb, nelec_b))) - 0.5
            ci0 /= np.linalg.norm(ci0)
        else:
            ci0 = guess
        E, self.fcivec = self.cisolver.kernel(h1, h2, Ham.norb, self.nelec, ci0=ci0, ecore=Ham.H0)
        self.make_rdm1(Ham)
        if calc_rdm2:
            self.make_rdm2(Ham)
        self.optimized, self.E = True, E
        log.info("FCI solver converged: %s", self.cisolver.converged)
        log.info("FCI total energy: %s (E_HF = %s)", E, E_HF)
        return self.onepdm, E

    def make_rdm1(self, Ham=None):
        if self.restricted:
            self.onepdm_mo = (self.cisolver.make_rdm1() * 0.5)[np.newaxis]
        else:
            self.onepdm_mo = np.asarray(self.cisolver.make_rdm1s())
        self.onepdm = transform_rdm1_to_ao_mol(self.onepdm_mo, self.scfsolver.mf.mo_coeff)
        return self.onepdm

    def make_rdm2(self, Ham=None, ao_repr=False):
        """twopdm_mo in the HF orbitals -- restricted: (1, n, n, n, n) spin-summed; unrestricted: aa, bb, ab -- and, with ao_repr,
        twopdm in the basis of the Hamiltonian."""
        if self.restricted:
            pdm = self.cisolver.make_rdm2()[np.newaxis]
        else:
            pdm = np.asarray(self.cisolver.make_rdm12s()[1])          # aa, ab, bb
        ao = transform_rdm2_to_ao_mol(pdm, self.scfsolver.mf.mo_coeff) if ao_repr else None
        if not self.restricted:
            pdm = pdm[[0, 2, 1]]
            ao = None if ao is None else ao[[0, 2, 1]]
        self.twopdm_mo, self.twopdm = pdm, ao
        return self.twopdm_mo

    def run_dmet_ham(self, Ham, last_aabb=True, **kwargs):
        """<Ham> in the FCI state of the last run (Ham in the embedding basis of that run; it is not modified)."""
        log.info("FCI solver Run DMET Hamiltonian.")
        if not self.optimized:
            raise RuntimeError("FCI.run_dmet_ham: run() first")
        H, _, _ = self._mo_ham(Ham)
        h1, h2 = np.asarray(H.H1["cd"]), np.asarray(H.H2["ccdd"])
        self.make_rdm2(Ham)
        r1, r2 = self.onepdm_mo, self.twopdm_mo
        log.eassert(h1.shape == r1.shape and h2.shape == r2.shape, "run_dmet_ham: shapes of the Hamiltonian and the densities differ")
        if self.restricted:
            E1 = 2.0 * np.einsum("pq,qp", h1[0], r1[0])
            E2 = 0.5 * np.einsum("pqrs,pqrs", h2[0], r2[0])
        else:          # both in the order aa, bb, ab
            E1 = np.einsum("spq,sqp", h1, r1)
            E2 = 0.5 * np.einsum("pqrs,pqrs", h2[0], r2[0]) + 0.5 * np.einsum("pqrs,pqrs", h2[1], r2[1]) + np.einsum("pqrs,pqrs", h2[2], r2[2])
        E = E1 + E2 + Ham.H0
        log.debug(0, "run DMET Hamiltonian:\nE0 = %20.12f, E1 = %20.12f, E2 = %20.12f, E = %20.12f", Ham.H0, E1, E2, E)
        return float(E)

    def cleanup(self):
        self.cisolver.close()
        if self.scfsolver.mf is not None:
            self.scfsolver.mf.close()


class FCI_AO(object):
    def __init__(self, *args, **kwargs):
        _refuse("FCI_AO (FCI without a mean field first; FCI does the same after Hartree-Fock)")
