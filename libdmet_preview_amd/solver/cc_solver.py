"""
The CCSD impurity solver: the restricted branch of the reference's CCSD class (libdmet/solver/cc.py :567-1211) on the device
Hartree-Fock of solver/scf.py and the device CCSD of solver/cc.py + solver/cc_lambda.py, laid out like
solver/scf_solver.py.

  run            :618-1153   HF, T, solve_lambda, make_rdm1 -> (onepdm, E)
  run_dmet_ham   :1169-1211  the energy of the CCSD state on a scaled DMET Hamiltonian: RCCSDLambda.expval in place of exp_val_rccsd
  make_rdm1      the density of the last run
  ccsd_t         :1073-1076  E_(T) of the last run's amplitudes (solver/ccsd_t.py): E_CCSD(T) = E + ccsd_t()

Unrestricted and generalised references, the ccsdt=True path of run / run_dmet_ham (it needs the (T) Lambda equations and the (T)
densities, _get_ccsdt_drv), Brueckner / tailored / linear CC, frozen orbitals, the two-particle density, HDF5 output and MPI are not
built: each raises NotImplementedError by name.  A restart (restart=True) starts T and Lambda from the amplitudes of
the previous run, held in memory only.  The module imports without a GPU; the device context is created by the first call that computes.
"""
import numpy as np

from libdmet_preview_amd.solver import scf
from libdmet_preview_amd.solver._posthf import check_frozen
from libdmet_preview_amd.system import integral
from libdmet_preview_amd.utils import logger as log


def _refuse(what):
    raise NotImplementedError("CCSolver: %s is not built (restricted CCSD with Lambda, the one-particle density and expval only)" % what)


class CCSolver(object):
    def __init__(self, nproc=1, nnode=1, nthread=1, TmpDir="./tmp", SharedDir=None, restricted=False, Sz=0, bcs=False, ghf=False,
                 tol=1e-7, tol_normt=1e-5, max_cycle=200, level_shift=0.0, frozen=0, max_memory=40000, compact_rdm2=False,
                 scf_newton=True, diis_space=8, diis_start_cycle=None, iterative_damping=1.0, linear=False, approx_l=False, alpha=None,
                 beta=np.inf, tcc=False, ite=None, ite_rk=None, use_mpi=False, **kwargs):
        if not restricted:
            _refuse("unrestricted CCSD (restricted=False)")
        for name, on in (("ghf", ghf), ("bcs", bcs), ("linear", linear), ("tcc", tcc), ("ite", ite), ("ite_rk", ite_rk)):
            if on:
                _refuse("%s=%r" % (name, on))
        if use_mpi or nproc * nnode > 1:
            _refuse("MPI (use_mpi, nproc * nnode > 1)")
        for name, on in kwargs.items():
            if on:
                _refuse("%s=%r" % (name, on))
        check_frozen(frozen, "CCSD")
        if Sz != 0:
            _refuse("an open shell (Sz = %r) in restricted CCSD" % (Sz,))
        self.restricted, self.Sz, self.frozen = True, 0, frozen
        self.conv_tol, self.conv_tol_normt, self.max_cycle, self.max_memory = tol, tol_normt, max_cycle, max_memory
        self.level_shift, self.iterative_damping, self.diis_space = level_shift, iterative_damping, diis_space
        self.approx_l, self.alpha, self.beta = approx_l, alpha, beta
        self.bcs = self.ghf = self.linear = self.tcc = False
        self.scfsolver = scf.SCF(newton_ah=scf_newton)
        self.cisolver = None
        self.onepdm = self.twopdm = self.onepdm_mo = None
        self.optimized = False
        self._amps = None          # (t1, t2, l1, l2) of the last run: the restart

    @property
    def mf(self):
        return self.scfsolver.mf

    def run(self, Ham=None, nelec=None, guess=None, restart=False, calc_rdm2=False, Mu=None, **kwargs):
        """HF, T, Lambda and the density on Ham (restricted: one spin block) -> (onepdm, E): onepdm (1, n, n), per spin
        (C gamma C^T / 2), E = E_HF + E_corr.  kwargs: dm0, scf_max_cycle (200)."""
        from libdmet_preview_amd.solver import cc_lambda
        log.info("CC solver: start")
        if calc_rdm2:
            _refuse("the two-particle density (calc_rdm2)")
        if Mu is not None:
            _refuse("a chemical potential (Mu) in restricted CCSD")
        for name in ("ccsdt", "ccsdt_energy"):
            if kwargs.get(name, None) not in (None, False):
                _refuse("%s=%r (the (T) Lambda equations and the (T) densities; the (T) energy alone is ccsd_t() after run())"
                        % (name, kwargs[name]))
        for name in ("bcc", "ccd", "dump_tl", "fcc_name_save", "remove_h2", "mo_energy_custom", "mo_occ_custom",
                     "mo_coeff_custom"):
            if kwargs.get(name, None) not in (None, False):
                _refuse("%s=%r" % (name, kwargs[name]))
        spin = Ham.H1["cd"].shape[0]
        if spin > 1 or not Ham.restricted:
            _refuse("a spin-dependent Hamiltonian")
        if nelec is None:
            raise ValueError("CC solver: nelec cannot be None for RCC or UCC.")
        if nelec % 2 or nelec < 2:
            _refuse("an odd number of electrons (nelec = %r)" % (nelec,))
        self.scfsolver.set_system(nelec, 0, False, True, max_memory=self.max_memory)
        self.scfsolver.set_integral(Ham)
        E_HF, _ = self.scfsolver.HF(tol=min(self.conv_tol * 0.1, 1e-10), MaxIter=kwargs.get("scf_max_cycle", 200),
                                    InitGuess=kwargs.get("dm0", None), alpha=self.alpha, beta=self.beta)
        mf = self.scfsolver.mf
        log.debug(1, "CC solver: mean-field converged: %s", mf.converged)
        if self.cisolver is not None:
            self.cisolver.close()
        obj = cc_lambda.RCCSDLambda(mf)
        obj.conv_tol, obj.conv_tol_normt, obj.max_cycle, obj.diis_space = self.conv_tol, self.conv_tol_normt, self.max_cycle, self.diis_space
        obj.level_shift, obj.iterative_damping = self.level_shift, self.iterative_damping
        self.cisolver = obj
        t1 = t2 = l1 = l2 = None
        if guess is not None:
            t1, t2 = guess[:2]
            if len(guess) == 4:
                l1, l2 = guess[2:]
        elif restart and self.optimized and self._amps is not None and self._amps[0].shape == obj._shapes()[0]:
            t1, t2, l1, l2 = self._amps
        e_corr, t1, t2 = obj.kernel(t1=t1, t2=t2)
        log.eassert(obj.converged or self.max_cycle < 2, "CC solver: the amplitude equations did not converge")
        l1, l2 = obj.solve_lambda(l1=l1, l2=l2, approx_l=self.approx_l)
        gam = obj.make_rdm1()
        c = obj._mo()
        self.onepdm_mo = gam[None] * 0.5
        self.onepdm = (c @ gam @ c.T)[None] * 0.5
        self._amps, self.optimized = (t1, t2, l1, l2), True
        E = E_HF + e_corr
        log.info("CC solver: E_HF = %20.12f, E_corr = %20.12f", E_HF, e_corr)
        return self.onepdm, E

    def run_dmet_ham(self, Ham, last_aabb=True, save_dmet_ham=False, dmet_ham_fname="dmet_ham.h5", use_calculated_twopdm=False, **kwargs):
        """<Ham> in the CCSD state of the last run: expval(Ham.H0, Ham.H1["cd"][0], Ham.H2["ccdd"][0]) (Ham in the embedding basis)."""
        log.info("CC solver Run DMET Hamiltonian.")
        if save_dmet_ham:
            _refuse("save_dmet_ham (HDF5 output)")
        if use_calculated_twopdm:
            _refuse("use_calculated_twopdm (the two-particle density)")
        if kwargs.get("ccsdt", False):
            _refuse("ccsdt (the (T) densities)")
        if self.cisolver is None:
            raise RuntimeError("CCSolver.run_dmet_ham: run() first")
        eri = np.asarray(Ham.H2["ccdd"])
        if integral.get_eri_format(eri, Ham.norb)[1]:
            eri = eri[0]
        return self.cisolver.expval(Ham.H0, np.asarray(Ham.H1["cd"])[0], eri)

    def make_rdm1(self, Ham=None):
        return self.onepdm

    def ccsd_t(self):
        """E_(T) of the amplitudes of the last run (PySCF's closed-shell ccsd_t on the device): E_CCSD(T) = E + ccsd_t()."""
        if self.cisolver is None or not self.optimized:
            raise RuntimeError("CCSolver.ccsd_t: run() first")
        return self.cisolver.ccsd_t()

    def make_rdm2(self, *args, **kwargs):
        _refuse("the two-particle density (make_rdm2)")
