"""
Unrestricted CCSD on the device, over the unrestricted Hartree-Fock object of solver/scf.py (DeviceHF): DESIGN.md K24.

  UCCSD   the T1 / T2 amplitude equations with general (non-canonical) Fock matrices and the correlation energy over two sets of
          orbitals: what UICCSD(mf).kernel() does behind the reference's CCSD.run with its default restricted=False
          (solver/cc.py:227, :912).  solver.cc.run_ccsd dispatches here for an unrestricted solver.

The MO blocks come from dmk_ao2mo_s4 applied to the three ERI blocks the DeviceHF already holds (mf._blocks = [aa, bb, ab]; the ERI is
not uploaded again; (vv|vv), (VV|VV) and (vv|VV) stay 4-fold packed and are never unpacked).  A block with a beta bra and an alpha ket
has no AO block of its own: it is the transpose of its alpha-beta twin, made on the device.  The iteration is dmk_uccsd_run.  Amplitudes
in PySCF's layout: t1 = (t1a, t1b), t2 = (t2aa, t2ab, t2bb), t2aa / t2bb stored in full.  Not built, each refusing by name: the Lambda
equations, the densities, the perturbative triples, frozen orbitals, a level shift other than 0 and a damping other than 1
(solver.cc_solver.CCSolver(restricted=False) keeps refusing: it needs the first two).  The module imports without a GPU.
"""
import ctypes as C

import numpy as np

from libdmet_preview_amd._lib import lib, c_vp, c_i64
from libdmet_preview_amd.solver import scf
from libdmet_preview_amd.solver.cc import _CCSDBase

_PACK_BOTH = 3          # DMK_AO2MO_PACK_BRA | DMK_AO2MO_PACK_KET

# what csrc/uccsd.hip reads, in the order of dmk_uccsd_ints: lower case alpha, upper case beta
_BLOCKS = ("oooo", "ovoo", "ovov", "oovv", "ovvv", "vvvv", "OOOO", "OVOO", "OVOV", "OOVV", "OVVV", "VVVV",
           "ooOO", "ovOO", "ovOV", "ooVV", "ovVV", "vvVV", "OVoo", "OOvv", "OVvv")
_PACKED = ("vvvv", "VVVV", "vvVV")


class _Ints(C.Structure):
    """dmk_uccsd_ints of include/libdmetk.h."""
    _fields_ = ([("fock_a", c_vp), ("fock_b", c_vp)] + [(name, c_vp) for name in _BLOCKS]
                + [("ld_vvvv", c_i64), ("ld_VVVV", c_i64), ("ld_vvVV", c_i64)])


def _not_built(what):
    raise NotImplementedError("%s is not built (solver.uccsd has the unrestricted T equations and the correlation energy only)" % what)


def plan_bytes(nocc_a, nvir_a, nocc_b, nvir_b, diis_space):
    """(bytes of the dmk_uccsd handle, bytes of its contraction workspace): dmk_uccsd_plan, host arithmetic."""
    out = (c_i64 * 2)()
    rc = lib.dmk_uccsd_plan(int(nocc_a), int(nvir_a), int(nocc_b), int(nvir_b), int(diis_space), out)
    if rc != 0:
        raise ValueError("dmk_uccsd_plan refuses (nocc_a, nvir_a, nocc_b, nvir_b, diis_space) = (%d, %d, %d, %d, %d)"
                         % (nocc_a, nvir_a, nocc_b, nvir_b, diis_space))
    return int(out[0]), int(out[1])


class _ERIS(object):
    """What ao2mo() hands back: the MO blocks as device arrays ((pq|rs) at row (p, q), column (r, s); the three vvvv-type blocks packed
    on both sides) and the two MO Fock matrices (host)."""
    fock = None


class UCCSD(_CCSDBase):
    _restricted = False
    _method = "UCCSD"
    _name, _prefix, _memory_title = "UCCSD", "dmk_uccsd_", "UCCSD with"
    _not_built = staticmethod(_not_built)

    # ---- what is not built -------------------------------------------------------------------------------------------------------
    def solve_lambda(self, *args, **kwargs):
        _not_built("The unrestricted Lambda equations (solve_lambda)")

    def make_rdm1(self, *args, **kwargs):
        _not_built("The UCCSD one-particle density (make_rdm1, it needs the Lambda equations)")

    def make_rdm2(self, *args, **kwargs):
        _not_built("The UCCSD two-particle density (make_rdm2, it needs the Lambda equations)")

    def ccsd_t(self, *args, **kwargs):
        _not_built("The unrestricted perturbative triples (T) (ccsd_t)")

    # ---- memory ------------------------------------------------------------------------------------------------------------------
    def _extents(self):
        n = self._scf._n
        oa, ob = self._nocc
        return {"o": oa, "v": n - oa, "O": ob, "V": n - ob}

    def memory_plan(self):
        """Bytes the solver will hold on the device, from host arithmetic alone: {"handle", "workspace", "integrals", "transform"}
        (the transform's workspace is released before the handle is made; a block with a beta bra is counted twice while its twin is
        transposed)."""
        n, e = self._scf._n, self._extents()
        handle, ws = plan_bytes(e["o"], e["v"], e["O"], e["V"], self.diis_space)
        pair = lambda k: k * (k + 1) // 2
        count = lambda name: (pair(e[name[0]]) * pair(e[name[2]]) if name in _PACKED
                              else e[name[0]] * e[name[1]] * e[name[2]] * e[name[3]])
        integrals = 8 * (sum(count(name) for name in _BLOCKS) + max(count(name) for name in _BLOCKS[-3:]) + 2 * n * n)
        transform = 0
        for w, flags in ((("o", "v", "v", "v"), 0), (("O", "V", "V", "V"), 0), (("o", "v", "V", "V"), 0), (("v", "v", "O", "V"), 0),
                         (("v", "v", "v", "v"), _PACK_BOTH), (("V", "V", "V", "V"), _PACK_BOTH), (("v", "v", "V", "V"), _PACK_BOTH)):
            p = (c_i64 * 3)()
            lib.dmk_ao2mo_plan(n, e[w[0]], e[w[1]], e[w[2]], e[w[3]], flags, 0, p)
            transform = max(transform, int(p[1]))
        return {"handle": handle, "workspace": ws, "integrals": integrals, "transform": transform}

    def _extents_text(self):
        e = self._extents()
        return "nocc = (%d, %d), nvir = (%d, %d)" % (e["o"], e["O"], e["v"], e["V"])

    # ---- the integrals -----------------------------------------------------------------------------------------------------------
    def ao2mo(self, mo_coeff=None):
        """The MO blocks (device) and the Fock matrices C_s^T F_s C_s of the density of these orbitals (host, [occupied | virtual])."""
        if mo_coeff is not None:
            self.mo_coeff = mo_coeff
            self._set_orbitals(mo_coeff)
        mf = self._scf
        ctx, n, ld, e = mf._ctx, mf._n, mf._ld, self._extents()
        d_c = self._dev_coeff()
        rng = {"o": (d_c[0], 0, e["o"]), "v": (d_c[0], e["o"], e["v"]), "O": (d_c[1], 0, e["O"]), "V": (d_c[1], e["O"], e["V"])}
        eris = _ERIS()
        for name in _BLOCKS:
            bra, ket = name[0].isupper(), name[2].isupper()
            if bra and not ket:
                # (PQ|rs) = (rs|PQ)^T: the transform of the ab block with the ranges swapped, then a device transpose
                twin = scf.ao2mo_block_dev(ctx, n, mf._blocks[2], [rng[x] for x in name[2:] + name[:2]], ld=ld)
                blk = ctx.empty((twin.shape[1], twin.shape[0]), np.float64)
                ctx.check(lib.dmk_transpose_f64(ctx.h, twin.shape[0], twin.shape[1], twin.ptr, blk.ptr))
                ctx.sync()
            else:
                eri = mf._blocks[2 if ket and not bra else 1 if bra else 0]
                blk = scf.ao2mo_block_dev(ctx, n, eri, [rng[x] for x in name], compact=name in _PACKED, ld=ld)
            setattr(eris, name, blk)
        dm = mf.make_rdm1(self.mo_coeff, self.mo_occ)
        fock = np.asarray(mf.get_fock(dm=dm), dtype=np.float64).reshape(2, n, n)
        cs = [self._c[s][:, self._order[s]] for s in range(2)]
        eris.fock = [cs[s].T @ fock[s] @ cs[s] for s in range(2)]
        return eris

    def _create(self, eris, diis_space):
        ctx, e = self._scf._ctx, self._extents()
        eris.d_fock = [ctx.to_device(f) for f in eris.fock]
        pair = lambda k: k * (k + 1) // 2
        ints = _Ints(fock_a=eris.d_fock[0].ptr, fock_b=eris.d_fock[1].ptr, ld_vvvv=pair(e["v"]), ld_VVVV=pair(e["V"]), ld_vvVV=pair(e["V"]),
                     **{name: getattr(eris, name).ptr for name in _BLOCKS})
        h = c_vp()
        ctx.check(lib.dmk_uccsd_create(ctx.h, e["o"], e["v"], e["O"], e["V"], C.byref(ints), int(diis_space), C.byref(h)))
        return h

    # ---- amplitudes --------------------------------------------------------------------------------------------------------------
    def _shapes(self):
        e = self._extents()
        oa, va, ob, vb = e["o"], e["v"], e["O"], e["V"]
        return (oa, va), (ob, vb), (oa, oa, va, va), (oa, ob, va, vb), (ob, ob, vb, vb)

    def _flatten(self, t1, t2):
        if t1 is None or t2 is None or len(t1) != 2 or len(t2) != 3:
            raise ValueError("unrestricted amplitudes are t1 = (t1a, t1b) and t2 = (t2aa, t2ab, t2bb)")
        amps = [np.ascontiguousarray(a, dtype=np.float64) for a in tuple(t1) + tuple(t2)]
        shapes = self._shapes()
        if any(a.shape != s for a, s in zip(amps, shapes)):
            raise ValueError("amplitudes of shapes %s; expected %s" % ([a.shape for a in amps], list(shapes)))
        return amps

    def _rebuild(self, parts):
        return tuple(parts[:2]), tuple(parts[2:])
