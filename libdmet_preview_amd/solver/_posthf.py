"""
What the post-Hartree-Fock objects over solver.scf.DeviceHF share (solver/mp.py, solver/cc.py): the argument checks of their
constructors and the [occupied | virtual] ordering of the orbitals that the MO transform is fed with.  Imports without a GPU.
"""
import numpy as np

from libdmet_preview_amd.solver import scf


def check_frozen(frozen, method):
    if not (frozen is None or (np.isscalar(frozen) and frozen == 0)):
        raise NotImplementedError("%s with frozen orbitals (frozen = %r) is not built" % (method, frozen))


class PostHFBase(object):
    _restricted = True
    _method = "post-HF"          # the name the messages use

    def __init__(self, mf, frozen=None, mo_coeff=None, mo_occ=None):
        check_frozen(frozen, self._method)
        if not isinstance(mf, scf.DeviceHF):
            raise NotImplementedError("%s needs the device Hartree-Fock object (solver.scf.DeviceHF), got %s; generalised and "
                                      "Bogoliubov references are not built" % (type(self).__name__, type(mf).__name__))
        if mf._restricted != self._restricted:
            raise NotImplementedError("%s over %s Hartree-Fock object" % (type(self).__name__,
                                                                          "a restricted" if mf._restricted else "an unrestricted"))
        self._scf, self.frozen = mf, frozen
        self.mo_coeff = mf.mo_coeff if mo_coeff is None else mo_coeff
        self.mo_occ = mf.mo_occ if mo_occ is None else mo_occ
        if self.mo_coeff is None or self.mo_occ is None:
            raise ValueError("%s: the Hartree-Fock object has no orbitals yet (run its kernel first)" % type(self).__name__)
        self.e_corr = None
        self._set_orbitals(self.mo_coeff)

    def _spins(self, a):
        a = np.asarray(a, dtype=np.float64)
        return a[None] if self._restricted else a

    def _set_orbitals(self, mo_coeff):
        n = self._scf._n
        c, occ = self._spins(mo_coeff), self._spins(self.mo_occ)
        ns = 1 if self._restricted else 2
        if c.shape != (ns, n, n) or occ.shape != (ns, n):
            raise ValueError("mo_coeff %s / mo_occ %s do not fit %d spin channel(s) of %d orbitals" % (c.shape, occ.shape, ns, n))
        # [occupied | virtual] column order of every spin: the blocks of the transform are column ranges of one matrix
        self._order = [np.concatenate([np.flatnonzero(occ[s] > 0), np.flatnonzero(occ[s] <= 0)]) for s in range(ns)]
        self._nocc = [int(np.count_nonzero(occ[s] > 0)) for s in range(ns)]
        if any(o < 1 or o >= n for o in self._nocc):
            raise ValueError("%s needs occupied and virtual orbitals in every spin channel (nocc = %s of %d)"
                             % (self._method, self._nocc, n))
        self._c = c

    @property
    def nmo(self):
        return self._scf._n if self._restricted else (self._scf._n, self._scf._n)

    @property
    def nocc(self):
        return self._nocc[0] if self._restricted else tuple(self._nocc)

    @property
    def e_tot(self):
        return self._scf.e_tot + (self.e_corr or 0.0)

    def _dev_coeff(self):
        ctx = self._scf._ctx
        return [ctx.to_device(self._c[s][:, self._order[s]]) for s in range(len(self._c))]
