"""
The perturbative triples (T) of restricted CCSD on the device (csrc/ccsd_t.hip), over a solver.cc.RCCSD object: what
self.cisolver.ccsd_t(eris=eris) does behind the reference's CCSD.run (solver/cc.py:1073-1076).

  kernel(mycc, t1=None, t2=None, max_memory=None) -> e_t     E_(T) of the object's current amplitudes, or of the ones given

The arithmetic is that of PySCF's closed-shell ccsd_t: denominators from the Fock DIAGONAL, the f_ov term kept.  At the device
Hartree-Fock's canonical orbitals that is the usual (T); at rotated (non-canonical) orbitals it is PySCF's number, NOT an
orbital-invariant one.  E_CCSD(T) = E_HF + e_corr + e_t.

W of a batch of unique triples a >= b >= c lives in a workspace that dmk_rccsd_t allocates and frees; max_memory (MB; default: the
object's max_memory, else what is free) bounds it.  The result does not depend on that bound, bit for bit.  solver.cc.RCCSD.ccsd_t
keeps refusing (its tests pin that); solver.cc_lambda.RCCSDLambda.ccsd_t and solver.cc_solver.CCSolver.ccsd_t call this module.  The
(T) Lambda equations and the (T) densities (the reference's ccsdt=True path, _get_ccsdt_drv) are not built.  The module imports
without a GPU.
"""
from libdmet_preview_amd._lib import lib, c_dbl, c_i64
from libdmet_preview_amd.utils import logger as log


def plan_bytes(nocc, nvir):
    """(fixed bytes of the workspace of dmk_rccsd_t, bytes per triple in flight): dmk_rccsd_t_plan, host arithmetic."""
    out = (c_i64 * 2)()
    rc = lib.dmk_rccsd_t_plan(int(nocc), int(nvir), out)
    if rc != 0:
        raise ValueError("dmk_rccsd_t_plan refuses (nocc, nvir) = (%d, %d)" % (nocc, nvir))
    return int(out[0]), int(out[1])


def _budget(mycc, max_memory):
    """Bytes the workspace may take, checked against fixed + one triple BEFORE anything is allocated."""
    o = mycc._nocc[0]
    v = mycc._scf._n - o
    fixed, unit = plan_bytes(o, v)
    if max_memory is None:
        max_memory = mycc.max_memory
    if max_memory is None:
        have, what = mycc._scf._ctx.mem_info()[0] // 4 * 3, "three quarters of what is free on the device"
    else:
        have, what = int(float(max_memory) * (1 << 20)), "allowed by max_memory"
    if fixed + unit > have:
        raise MemoryError("(T) with nocc = %d, nvir = %d plans %d bytes of device memory (permuted t2, one double per unique triple and "
                          "the partial sums) and %d bytes per triple in flight; %d bytes are %s" % (o, v, fixed, unit, have, what))
    return have


def kernel(mycc, t1=None, t2=None, max_memory=None):
    """E_(T) of the amplitudes of `mycc` (a solver.cc.RCCSD whose kernel() has run), or of t1, t2 when both are given (they become
    the object's current amplitudes).  max_memory: MB of device memory for W."""
    if (t1 is None) != (t2 is None):
        raise ValueError("amplitudes: both t1 and t2, or neither")
    if t1 is None and mycc.t1 is None:
        raise RuntimeError("(T): no amplitudes (run kernel() first, or pass t1 and t2)")
    have = _budget(mycc, max_memory)
    if t1 is not None:
        mycc._set(t1, t2)
    res = (c_dbl * 2)()
    mycc._scf._ctx.check(lib.dmk_rccsd_t(mycc._handle(), have, res))
    log.debug(0, "RCCSD(T): e_t = %.12f in %d batches of triples", res[0], int(res[1]))
    return float(res[0])
