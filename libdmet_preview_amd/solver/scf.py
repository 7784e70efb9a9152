"""
The ERI x density piece of libdmet/solver/scf.py on the MI355X:

  _get_jk     solver/scf.py:255-335   (RHF / UHF / UIHF; pyscf hf.dot_eri_dm -> dmk_jk_s4)
  _get_veff   solver/scf.py:337-352
  SCF         solver/scf.py:883-1304  (the Hartree-Fock part: HF, get_mo, get_mo_energy; `.mf` = DeviceHF)
  regularize_coeff, incore_transform, ao2mo_Ham   solver/scf.py:51-189  (pyscf ao2mo -> dmk_ao2mo_s4)

MP2 on top of a finished SCF is solver.mp.run_mp2(scfsolver) (solver/mp.py); SCF.MP2 itself still raises.

The embedding ERI is streamed from HBM in its 4-fold packed form, once for J (both directions of the
alpha-beta block in the same pass) and once for K; 1-fold / 8-fold inputs are gathered into the 4-fold
form on the device first (dmk_eri_to_s4).  `jk_blocks_dev` is the device-resident form used by the
pipeline: it takes the three spin blocks by pointer, so the (aa, ab, bb) order of the transform and the
(aa, bb, ab) order of the Hamiltonian (routine/slater.py:461-462) need no 26 GB shuffle.
"""
import ctypes as C

import numpy as np

from libdmet_preview_amd._lib import lib, get_ctx, c_vp, c_int, c_dbl
from libdmet_preview_amd.system import integral
from libdmet_preview_amd.utils import logger as log


def _rows_call(ctx, outs, whole, rows, row_ranges):
    """The `row_ranges` convention of jk_dev / fock_dev: None runs `whole()`, an empty list leaves zero partial results in `outs`,
    anything else goes to `rows(nranges, pointer)` as an int64 (nranges, 2) array."""
    if row_ranges is None:
        ctx.check(whole())
    elif len(row_ranges) == 0:
        for o in outs:
            if o is not None:
                o.zero_()
    else:
        rr = np.ascontiguousarray(row_ranges, dtype=np.int64).reshape(-1, 2)
        ctx.check(rows(len(rr), rr.ctypes.data))


def jk_dev(ctx, n, d_eri, d_dm_row=None, d_dm_col=None, d_dm_k=None, ld=None, row_ranges=None):
    """One 4-fold block: returns device (vj_row, vj_col, vk), None where the density was not given.  `row_ranges`
    ([(lo, hi)] of packed pair rows, lo a multiple of 32): the PARTIAL results of those rows of a row-sharded ERI -- the
    caller sums them over ranks."""
    npair = n * (n + 1) // 2
    out = [ctx.empty((n, n), np.float64) if d is not None else None for d in (d_dm_row, d_dm_col, d_dm_k)]
    p = lambda a: a.ptr if a is not None else None
    head = (ctx.h, int(n), d_eri.ptr, int(ld or npair))
    tail = (p(d_dm_row), p(d_dm_col), p(d_dm_k), p(out[0]), p(out[1]), p(out[2]))
    _rows_call(ctx, out, lambda: lib.dmk_jk_s4(*head, *tail), lambda nr, rr: lib.dmk_jk_s4_rows(*head, nr, rr, *tail), row_ranges)
    return tuple(out)


def jk_blocks_dev(ctx, n, d_aa, d_bb, d_ab, d_dm, with_j=True, with_k=True, row_ranges=None):
    """UIHF J/K from the three device blocks and d_dm (2, n, n): ((vj00, vj11), (vj01, vj10)), (vk00, vk11)."""
    dma, dmb = d_dm.offset(0, (n, n)), d_dm.offset(n * n, (n, n))
    vj00, _, vk00 = jk_dev(ctx, n, d_aa, dma if with_j else None, None, dma if with_k else None, row_ranges=row_ranges)
    vj11, _, vk11 = jk_dev(ctx, n, d_bb, dmb if with_j else None, None, dmb if with_k else None, row_ranges=row_ranges)
    vj01 = vj10 = None
    if with_j:
        vj01, vj10, _ = jk_dev(ctx, n, d_ab, dmb, dma, None, row_ranges=row_ranges)     # J a from b (rows), J b from a (columns)
    return ((vj00, vj11), (vj01, vj10)), (vk00, vk11)


def _block_to_dev_s4(ctx, blk, fmt, n):
    npair = n * (n + 1) // 2
    d = ctx.to_device(np.ascontiguousarray(blk, dtype=np.float64).reshape(-1))
    if fmt == 's4':
        return d
    out = ctx.empty((npair, npair), np.float64)
    ctx.check(lib.dmk_eri_to_s4(ctx.h, int(n), 1 if fmt == 's1' else 8, d.ptr, out.ptr))
    return out


def _get_jk(dm, eri, with_j=True, with_k=True):
    """
    J and K from rdm1 and ERI (RHF, UHF, UIHF).  J: ijkl,kl->ij   K: ijkl,il->jk.

    dm ((spin,) nao, nao); eri with or without spin dimension, s1 / s4 / s8.
    Returns vj (spin, nao, nao) [(2, 2, nao, nao) for UIHF] and vk (spin, nao, nao).
    """
    dm = np.asarray(dm, dtype=np.double)
    if dm.ndim == 2:
        dm = dm[np.newaxis]
    spin, nao = dm.shape[0], dm.shape[-1]
    eri = np.asarray(eri, dtype=np.double)
    eri_format, spin_dim = integral.get_eri_format(eri, nao)
    if spin_dim == 0:
        eri = eri[None]
        spin_dim = 1
    ctx = get_ctx()
    d_dm = ctx.to_device(dm)
    get = lambda a: a.get() if a is not None else None
    if spin == 1 or spin_dim == 1:
        d_E = _block_to_dev_s4(ctx, eri[0], eri_format, nao)
        vj, vk = [], []
        for s in range(spin):
            d = d_dm.offset(s * nao * nao, (nao, nao))
            j, _, k = jk_dev(ctx, nao, d_E, d if with_j else None, None, d if with_k else None)
            vj.append(get(j))
            vk.append(get(k))
        return (np.asarray(vj) if with_j else None), (np.asarray(vk) if with_k else None)
    elif spin_dim == 3:      # UIHF
        assert dm.shape[0] == 2
        blocks = [_block_to_dev_s4(ctx, eri[b], eri_format, nao) for b in range(3)]
        ((j00, j11), (j01, j10)), (k00, k11) = jk_blocks_dev(ctx, nao, blocks[0], blocks[1], blocks[2], d_dm,
                                                              with_j, with_k)
        # NOTE explicit write down vj, without broadcast (solver/scf.py:330-332)
        vj = np.asarray(((get(j00), get(j11)), (get(j01), get(j10)))) if with_j else None
        vk = np.asarray((get(k00), get(k11))) if with_k else None
        return vj, vk
    raise ValueError


def _get_veff(dm, eri):
    """HF effective potential (RHF: vj - vk/2 with a spin-traced dm; UHF: vj_a + vj_b - vk), (spin, nao, nao)."""
    dm = np.asarray(dm, dtype=np.double)
    if dm.ndim == 2:
        dm = dm[np.newaxis]
    spin = dm.shape[0]
    vj, vk = _get_jk(dm, eri)
    if spin == 1:
        veff = vj - vk * 0.5
    else:
        veff = vj[0] + vj[1] - vk
    return veff


def _get_veff_ghf(dm, eri):
    """HF effective potential of a generalised (spin-orbital) density against a spinless ERI, vj - vk (solver/scf.py:732-740)."""
    dm = np.asarray(dm, dtype=np.double)
    vj, vk = _get_jk(dm, eri)
    return vj[0] - vk[0]


# *********************************************************************
# MO integral transform on the device: DESIGN.md K19
# *********************************************************************

_AO2MO_PACK_BRA, _AO2MO_PACK_KET = 1, 2


def regularize_coeff(mo_coeffs):
    """Four sets of MO coefficients -> ([c0, c1, c2, c3], spin): every entry a 2-d array (spin 1; a one-element list is unwrapped)
    or a pair of them [c_alpha, c_beta] (spin 2); `spin` is that of the last entry, as in the reference (solver/scf.py:51-69)."""
    out, spin = [], 1
    for mo in mo_coeffs:
        if isinstance(mo, np.ndarray) and mo.ndim == 2:
            out.append(mo)
            spin = 1
        else:
            spin = len(mo)
            out.append(mo[0] if spin == 1 else mo)
    return out, spin


def _col_range(c):
    """(DevArray of a row-major (n, ncols) matrix, first column, width) from that triple or from a bare DevArray (all columns)."""
    if isinstance(c, tuple):
        d, c0, w = c
        return d, int(c0), int(w)
    return c, 0, int(c.shape[-1])


def ao2mo_block_dev(ctx, n, d_eri, coeffs, compact=False, ld=None, ws_bytes=0):
    """One 4-fold device block through dmk_ao2mo_s4: `coeffs` are four column ranges (DevArray (n, ncols), first column, width) or
    bare DevArrays.  compact=True packs a pair index whose two ranges are the same range of the same array.  Returns the DevArray
    (rows (i, j), columns (k, l)); nothing crosses to the host."""
    npair = n * (n + 1) // 2
    cs = [_col_range(c) for c in coeffs]
    for d, c0, w in cs:
        if d.shape[-2] != n or c0 < 0 or w < 1 or c0 + w > d.shape[-1]:
            raise ValueError("ao2mo: a coefficient range [%d, %d) of a %s matrix for n = %d" % (c0, c0 + w, d.shape, n))
    same = lambda a, b: a[0].address == b[0].address and a[0].shape[-1] == b[0].shape[-1] and a[1:] == b[1:]
    flags = 0
    if compact and same(cs[0], cs[1]):
        flags |= _AO2MO_PACK_BRA
    if compact and same(cs[2], cs[3]):
        flags |= _AO2MO_PACK_KET
    w = [c[2] for c in cs]
    rows = w[0] * (w[0] + 1) // 2 if flags & _AO2MO_PACK_BRA else w[0] * w[1]
    cols = w[2] * (w[2] + 1) // 2 if flags & _AO2MO_PACK_KET else w[2] * w[3]
    out = ctx.empty((rows, cols), np.float64)
    args = []
    for d, c0, wd in cs:
        args += [c_vp(d.address + 8 * c0), int(d.shape[-1]), wd]
    ctx.check(lib.dmk_ao2mo_s4(ctx.h, int(n), d_eri.ptr, int(ld or npair), *(args + [flags, int(ws_bytes), out.ptr])))
    return out


def _same_coeff(a, b):
    return a is b or (a.shape == b.shape and np.array_equal(a, b))


def _upload_coeffs(ctx, cs):
    """Host coefficient matrices -> DevArrays; matrices that are the same array (or equal) share one upload, and with it one pointer."""
    seen, out = [], []
    for c in cs:
        c = np.ascontiguousarray(c, dtype=np.float64)
        for h, d in seen:
            if _same_coeff(h, c):
                out.append(d)
                break
        else:
            d = ctx.to_device(c)
            seen.append((c, d))
            out.append(d)
    return out


def _spin_blocks_to_dev(ctx, eri, nao):
    """ERI (s1 / s4 / s8, with or without a spin axis) -> list of 4-fold device blocks (one per entry of the spin axis)."""
    eri = np.asarray(eri, dtype=np.double)
    fmt, spin_dim = integral.get_eri_format(eri, nao)
    if spin_dim == 0:
        eri = eri[None]
    return [_block_to_dev_s4(ctx, blk, fmt, nao) for blk in eri]


def incore_transform_dev(ctx, n, blocks, c, compact=False, ld=None, ws_bytes=0):
    """incore_transform over device arrays: `blocks` the 4-fold DevArrays (one, or aa, bb, ab), `c` four DevArrays / column ranges or
    four [alpha, beta] pairs of them.  Returns the list of transformed DevArrays (one, or aa, bb, ab)."""
    log.eassert(len(c) == 4, "Need 4 coefficents for transformation.")
    spin_resolved = isinstance(c[-1], (list,)) and len(c[-1]) == 2
    if not spin_resolved:
        c = [x[0] if isinstance(x, list) else x for x in c]
        log.eassert(len(blocks) == 1, "a spin-independent transform takes one ERI block, got %d", len(blocks))
        return [ao2mo_block_dev(ctx, n, blocks[0], c, compact, ld, ws_bytes)]
    log.eassert(len(blocks) in (1, 3), "spin-resolved coefficients take one ERI block or (aa, bb, ab), got %d", len(blocks))
    b = list(blocks) * 3 if len(blocks) == 1 else blocks
    pick = lambda spins: [c[m][s] for m, s in enumerate(spins)]
    return [ao2mo_block_dev(ctx, n, b[0], pick((0, 0, 0, 0)), compact, ld, ws_bytes),
            ao2mo_block_dev(ctx, n, b[1], pick((1, 1, 1, 1)), compact, ld, ws_bytes),
            ao2mo_block_dev(ctx, n, b[2], pick((0, 0, 1, 1)), compact, ld, ws_bytes)]


def incore_transform(eri, c, compact=False):
    """Two-electron integral transformation (solver/scf.py:71-119) on the device: c is a tuple of four coefficient sets, each a
    2-d array or [alpha, beta]; eri s1 / s4 / s8 with or without a spin axis.  The result always has a spin axis: (1, ., .) or
    (aa, bb, ab) with the ab block transformed by (C_a, C_a, C_b, C_b).  compact=True packs a pair index whose two coefficient
    matrices are the same array."""
    log.eassert(len(c) == 4, "Need 4 coefficents for transformation.")
    c, spin = regularize_coeff(c)
    if spin == 1:
        nao = c[0].shape[-2]
        _, spin_dim = integral.get_eri_format(np.asarray(eri), nao)
        if spin_dim > 1 or spin_dim < 0:
            raise ValueError("a spin-independent transform of an ERI with a spin axis of %d" % spin_dim)
        ctx = get_ctx()
        out = incore_transform_dev(ctx, nao, _spin_blocks_to_dev(ctx, eri, nao), _upload_coeffs(ctx, c), compact)
        return out[0].get()[np.newaxis]
    elif spin == 2:
        nao = c[0][0].shape[-2]
        _, spin_dim = integral.get_eri_format(np.asarray(eri), nao)
        if spin_dim not in (0, 1, 3):
            raise ValueError("a spin-resolved transform of an ERI with a spin axis of %d" % spin_dim)
        ctx = get_ctx()
        flat = _upload_coeffs(ctx, [c[m][s] for m in range(4) for s in range(2)])
        d_c = [[flat[2 * m], flat[2 * m + 1]] for m in range(4)]
        out = incore_transform_dev(ctx, nao, _spin_blocks_to_dev(ctx, eri, nao), d_c, compact)
        return np.asarray([o.get() for o in out])
    raise ValueError("Incorrect spin dimension (%s) of mo_coeff." % spin)


def ao2mo_Ham_dev(ctx, norb, d_h1, blocks, d_C, compact=True, ld=None, ws_bytes=0):
    """ao2mo_Ham over device arrays, in the spirit of set_integral_dev: d_h1 (s1, norb, norb), `blocks` the 4-fold DevArrays (one, or
    aa, bb, ab), d_C (s, norb, norb) with s = 1 (restricted) or 2.  Returns (d_h1_mo (s, norb, norb), [transformed blocks]): one block
    for s = 1, (aa, bb, ab) for s = 2; nothing crosses to the host."""
    ns, nn = int(d_C.shape[0]), norb * norb
    d_t, d_out = ctx.empty((ns, norb, norb), np.float64), ctx.empty((ns, norb, norb), np.float64)
    sh = nn if d_h1.shape[0] == ns and ns > 1 else 0
    ctx.check(lib.dmk_dgemm_batched(ctx.h, 0, 0, norb, norb, norb, ns, 1.0, d_h1.ptr, norb, sh, d_C.ptr, norb, nn, 0.0, d_t.ptr, norb, nn))
    ctx.check(lib.dmk_dgemm_batched(ctx.h, 1, 0, norb, norb, norb, ns, 1.0, d_C.ptr, norb, nn, d_t.ptr, norb, nn, 0.0, d_out.ptr, norb, nn))
    cs = [d_C.offset(s * nn, (norb, norb)) for s in range(ns)]
    if ns == 1:
        return d_out, [ao2mo_block_dev(ctx, norb, blocks[0], [cs[0]] * 4, compact, ld, ws_bytes)]
    return d_out, incore_transform_dev(ctx, norb, blocks, [[cs[0], cs[1]]] * 4, compact, ld, ws_bytes)


def ao2mo_Ham(Ham, C, compact=True, in_place=False):
    """The Hamiltonian in the MO basis C (solver/scf.py:121-189): H1 -> C^T H1 C, the ERI through dmk_ao2mo_s4 -- 4-fold (compact) or
    (spin, norb, norb, norb, norb).  Restricted: C (norb, norb) or (1, norb, norb); unrestricted: C (2, norb, norb), an ERI of one
    spin block serves aa, bb and ab."""
    norb = Ham.norb
    if Ham.bogoliubov:
        raise NotImplementedError("ao2mo_Ham: Bogoliubov Hamiltonians are not built")
    C_ = np.asarray(C, dtype=np.float64)
    if C_.ndim == 2:
        C_ = C_[np.newaxis]
    H1 = np.asarray(Ham.H1["cd"], dtype=np.float64)
    ctx = get_ctx()
    blocks = _spin_blocks_to_dev(ctx, Ham.H2["ccdd"], norb)
    if Ham.restricted:
        C_ = C_[:1]
        blocks = blocks[:1]
    else:
        log.eassert(C_.ndim == 3 and C_.shape[0] == 2, "unrestricted ao2mo_Ham needs C of shape (2, norb, norb)")
        if len(blocks) not in (1, 3):
            raise ValueError("ao2mo_Ham: an ERI with a spin axis of %d" % len(blocks))
    d_h1, d_eri = ao2mo_Ham_dev(ctx, norb, ctx.to_device(H1), blocks, ctx.to_device(C_), compact)
    h1e = d_h1.get()
    eri = np.asarray([b.get() for b in d_eri])
    if not compact:
        eri = eri.reshape((-1, norb, norb, norb, norb))
    if in_place:
        Ham.H1["cd"] = h1e
        Ham.H2["ccdd"] = eri
        return Ham
    return integral.Integral(norb, Ham.restricted, Ham.bogoliubov, Ham.H0, {"cd": h1e}, {"ccdd": eri})


# *********************************************************************
# Hartree-Fock on the device (RHF, UHF, UIHF): DESIGN.md K18
# *********************************************************************

def fock_dev(ctx, n, d_eri, d_dm_j, d_dm_k, ld=None, row_ranges=None):
    """J[dm_j] and K[dm_k] of one 4-fold block from ONE pass over it (dmk_fock_s4): device (vj, vk).  `row_ranges` as in jk_dev."""
    npair = n * (n + 1) // 2
    vj, vk = ctx.empty((n, n), np.float64), ctx.empty((n, n), np.float64)
    head = (ctx.h, int(n), d_eri.ptr, int(ld or npair))
    tail = (d_dm_j.ptr, d_dm_k.ptr, vj.ptr, vk.ptr)
    _rows_call(ctx, (vj, vk), lambda: lib.dmk_fock_s4(*head, *tail), lambda nr, rr: lib.dmk_fock_s4_rows(*head, nr, rr, *tail), row_ranges)
    return vj, vk


def diis_coeffs(B):
    """DIIS coefficients of the Gram matrix B of the error vectors (dmk_diis_coeffs, host arithmetic of the library)."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    m = B.shape[0]
    c = np.empty(m)
    rc = lib.dmk_diis_coeffs(int(m), B.ctypes.data, c.ctypes.data)
    if rc != 0:
        raise ValueError("dmk_diis_coeffs failed with %d for a %s matrix" % (rc, B.shape))
    return c


_SCF_DM, _SCF_FOCK, _SCF_VEFF, _SCF_MO_COEFF, _SCF_MO_ENERGY = range(5)
_SCF_TWO_PASS = 1
# the Fock build of the driver: dmk_fock_s4 (one pass per block) unless this is set (two dmk_jk_s4 passes; tools/fock_pass_lab.py)
TWO_PASS_FOCK = False


class DeviceHF(object):
    """The `.mf` of SCF: the attributes and methods of a PySCF RHF / UHF object that the callers of the reference read
    (solver/scf.py RIHF :231-253, UIHF :354-460), over a dmk_scf handle.  Restricted: 2-d arrays, spin-traced density;
    unrestricted: a leading spin axis of 2."""

    def __init__(self, ctx, norb, restricted, h1e, ovlp, blocks, ld, nocc, H0=0.0, alpha=None, Mu=None, h1e_no_mu=None, DiisDim=12,
                 MaxIter=50, tol=1e-10, conv_tol_grad=None, do_diis=True):
        self._ctx, self._n, self._restricted = ctx, int(norb), bool(restricted)
        self._ns = 1 if restricted else 2
        self.h1e = np.array(h1e, dtype=np.float64).reshape(self._ns, norb, norb)
        self.ovlp = None if ovlp is None else np.asarray(ovlp, dtype=np.float64)
        self.Mu, self.alpha = Mu, alpha
        self.diis_space, self.max_cycle, self.conv_tol, self.conv_tol_grad = int(DiisDim), int(MaxIter), float(tol), conv_tol_grad
        self.diis = True if do_diis else None
        self._H0, self._nocc = float(H0), [int(x) for x in nocc]
        self.mo_coeff = self.mo_energy = self.mo_occ = None
        self.converged, self.e_tot, self.cycles = False, 0.0, 0
        self._blocks = blocks                       # borrowed DevArrays: kept alive here, never freed by the handle
        self._ld = int(ld)                          # their row pitch (solver/mp.py reads the blocks in place)
        self._run = (None, None, None)
        n, ns = self._n, self._ns
        novlp, d_S, d_X = 0, None, None
        if self.ovlp is not None and not all(np.array_equal(s, np.eye(n)) for s in self.ovlp.reshape(-1, n, n)):
            from libdmet_preview_amd.lo import lowdin
            S = self.ovlp.reshape(-1, n, n)
            log.eassert(S.shape[0] in (1, ns), "overlap: one matrix or one per spin, got %s", self.ovlp.shape)
            novlp = S.shape[0]
            d_S = ctx.to_device(S)
            d_X = ctx.to_device(np.asarray([lowdin._lowdin(s) for s in S]))
        d_h1 = ctx.to_device(self.h1e)
        d_h1n = None if h1e_no_mu is None else ctx.to_device(np.asarray(h1e_no_mu, dtype=np.float64).reshape(ns, n, n))
        p = lambda a: a.ptr if a is not None else None
        b = list(blocks) + [None] * (3 - len(blocks))
        h = c_vp()
        ctx.check(lib.dmk_scf_create(ctx.h, n, ns, d_h1.ptr, p(d_h1n), p(d_S), p(d_X), novlp, b[0].ptr, p(b[1]), p(b[2]),
                                     int(ld), min(max(self.diis_space, 1), 12), _SCF_TWO_PASS if TWO_PASS_FOCK else 0, C.byref(h)))
        self._h = h
        ctx.sync()                                  # the inputs were copied in stream order: the uploads above may go now

    # ---- life time ---------------------------------------------------------------------------------------------------------------
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and self._ctx.h:
            lib.dmk_scf_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the run -----------------------------------------------------------------------------------------------------------------
    def _shape(self, a):
        return a[0] if self._restricted else a

    def _fetch(self, what, shape):
        d = self._ctx.empty(shape, np.float64)
        self._ctx.check(lib.dmk_scf_get(self._h, what, d.ptr))
        return d.get()

    def kernel(self, dm0=None):
        ctx, n, ns = self._ctx, self._n, self._ns
        d_dm0 = None
        if dm0 is not None:
            d_dm0 = ctx.to_device(np.asarray(dm0, dtype=np.float64).reshape(ns, n, n))
        tol_grad = self.conv_tol_grad if self.conv_tol_grad is not None else np.sqrt(self.conv_tol)
        nocc = (c_int * 2)(*(self._nocc + [0])[:2])
        res = (c_dbl * 5)()
        ctx.check(lib.dmk_scf_run(self._h, C.cast(nocc, c_vp), d_dm0.ptr if d_dm0 is not None else None,
                                  1.0 if self.alpha is None else float(self.alpha), self._H0, self.max_cycle, self.conv_tol,
                                  float(tol_grad), 1 if self.diis else 0, C.cast(res, c_vp)))
        self.e_tot, self.converged, self.cycles = float(res[0]), bool(res[1]), int(res[2])
        Vt = self._fetch(_SCF_MO_COEFF, (ns, n, n))
        self.mo_coeff = self._shape(np.ascontiguousarray(Vt.transpose(0, 2, 1)))       # columns = orbitals, as PySCF
        self.mo_energy = self._shape(self._fetch(_SCF_MO_ENERGY, (ns, n)))
        occ = np.zeros((ns, n))
        for s in range(ns):
            occ[s, :self._nocc[s]] = 2.0 if self._restricted else 1.0
        self.mo_occ = self._shape(occ)
        self._run = (self.mo_coeff, self.mo_occ, self._shape(self._fetch(_SCF_DM, (ns, n, n))))
        return self.e_tot

    # ---- what the callers read ------------------------------------------------------------------------------------------------------
    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        """(C occ) C^T: the device's own density of the run while mo_coeff / mo_occ are the run's, else built from the orbitals
        given (or assigned to the object: mo_coeff_custom of SCFSolver.run)."""
        mo_coeff = self.mo_coeff if mo_coeff is None else mo_coeff
        mo_occ = self.mo_occ if mo_occ is None else mo_occ
        if mo_coeff is self._run[0] and mo_occ is self._run[1]:
            return self._run[2].copy()
        c, f = np.asarray(mo_coeff, dtype=np.float64), np.asarray(mo_occ, dtype=np.float64)
        if self._restricted:
            return np.dot(c * f, c.T)
        return np.asarray([np.dot(c[s] * f[s], c[s].T) for s in range(2)])

    def get_hcore(self, *args):
        return self._shape(self.h1e)

    def get_ovlp(self, *args):
        return np.eye(self._n) if self.ovlp is None else self.ovlp

    def get_veff(self, mol=None, dm=None, *args, **kwargs):
        """RHF: vj - alpha vk / 2 of the spin-traced density; UHF: vj_a + vj_b - alpha vk_s (one pass per aa / bb block, the ab
        block J-only)."""
        if dm is None and isinstance(mol, np.ndarray):
            mol, dm = None, mol
        dm = self.make_rdm1() if dm is None else dm
        ctx, n, ns = self._ctx, self._n, self._ns
        d_dm = ctx.to_device(np.asarray(dm, dtype=np.float64).reshape(ns, n, n))
        d_v = ctx.empty((ns, n, n), np.float64)
        ctx.check(lib.dmk_scf_veff(self._h, d_dm.ptr, 1.0 if self.alpha is None else float(self.alpha), d_v.ptr))
        return self._shape(d_v.get())

    def get_fock(self, h1e=None, s1e=None, vhf=None, dm=None, *args, **kwargs):
        h1e = self.get_hcore() if h1e is None else h1e
        vhf = self.get_veff(dm=dm) if vhf is None else vhf
        return np.asarray(h1e) + np.asarray(vhf)

    def energy_elec(self, dm=None, h1e=None, vhf=None):
        """sum h1 D + 1/2 sum veff D without the contribution of Mu (UIHF.energy_elec, solver/scf.py:404-421)."""
        dm = self.make_rdm1() if dm is None else dm
        h1e = self.get_hcore() if h1e is None else h1e
        vhf = self.get_veff(dm=dm) if vhf is None else vhf
        h = np.array(h1e, dtype=np.float64)
        if self.Mu is not None and not self._restricted:
            S = self.get_ovlp()
            S = S if S.ndim == 2 else S[0]
            nao = self._n // 2
            h[0, :nao, :nao] += S[:nao, :nao] * self.Mu
            h[0, nao:, nao:] -= S[nao:, nao:] * self.Mu
        e_coul = 0.5 * float(np.sum(np.asarray(vhf) * np.asarray(dm)))
        return float(np.sum(h * np.asarray(dm))) + e_coul, e_coul

    def energy_nuc(self, *args):
        return self._H0

    def energy_tot(self, dm=None, h1e=None, vhf=None):
        return self.energy_elec(dm, h1e, vhf)[0] + self._H0


class SCF(object):
    """SCF of the reference (solver/scf.py:883-1304), Hartree-Fock part, without PySCF: the iteration runs in the library
    (csrc/scf.hip) on the 4-fold ERI resident in HBM."""

    def __init__(self, tmp="/tmp", newton_ah=True, no_kernel=False, verbose=None, chkname=None):
        if chkname is not None:
            raise NotImplementedError("chkname: checkpoint files are a PySCF facility, not built here")
        self.mf = None
        self.sys_initialized = self.integral_initialized = self.doneHF = False
        self.newton_ah, self.no_kernel, self.verbose, self.chkname = newton_ah, no_kernel, verbose, chkname
        self._newton_logged = False
        self._dev = None                # (ctx, [blocks], ld): the ERI on the device

    def set_system(self, nelec, spin, bogoliubov, spinRestricted, max_memory=120000):
        if bogoliubov:
            log.eassert(nelec is None, "nelec cannot be specified when doing BCS calculations")
        self.nelec, self.spin, self.bogoliubov, self.spinRestricted = nelec, spin, bogoliubov, spinRestricted
        self.max_memory = max_memory
        self.sys_initialized = True

    def set_integral(self, *args):
        log.eassert(self.sys_initialized, "set_integral() should be used after initializing set_system()")
        if len(args) == 1:
            log.eassert(self.bogoliubov == args[0].bogoliubov, "Integral is not consistent with system type")
            self.integral = args[0]
        elif len(args) == 4:
            self.integral = integral.Integral(args[0], self.spinRestricted, self.bogoliubov, *args[1:])
        else:
            log.error("input either an integral object, or (norb, H0, H1, H2)")
            raise ValueError("set_integral: an Integral object or (norb, H0, H1, H2)")
        self._dev = None
        self.integral_initialized = True

    def set_integral_dev(self, norb, H0, d_h1, d_ovlp, blocks, eri_format="s4", ld=None):
        """The Hamiltonian by device arrays (DevArray): d_h1 (spin, norb, norb), d_ovlp (norb, norb) or None, `blocks` the spin
        blocks of the ERI in the Hamiltonian's order (aa, bb, ab; one block for a spin-independent ERI) -- read in place when
        4-fold (row pitch ld), gathered into 4-fold copies on the device when 1- or 8-fold.  The ERI makes no host trip; the two
        small matrices are read back once."""
        log.eassert(self.sys_initialized, "set_integral_dev() should be used after initializing set_system()")
        log.eassert(eri_format in ("s1", "s4", "s8"), "eri_format must be s1, s4 or s8")
        ctx = d_h1.ctx
        npair = norb * (norb + 1) // 2
        H1 = d_h1.get().reshape(-1, norb, norb)
        ovlp = None if d_ovlp is None else d_ovlp.get()
        self.integral = integral.Integral(norb, self.spinRestricted, False, H0, {"cd": H1}, {"ccdd": None}, ovlp)
        own = []
        for b in blocks:
            if eri_format == "s4":
                own.append(b)
            else:
                out = ctx.empty((npair, npair), np.float64)
                ctx.check(lib.dmk_eri_to_s4(ctx.h, int(norb), 1 if eri_format == "s1" else 8, b.ptr, out.ptr))
                own.append(out)
        self._dev = (ctx, own, int(ld) if (ld and eri_format == "s4") else npair)
        self.integral_initialized = True

    def _device_eri(self):
        if self._dev is None:
            ctx = get_ctx()
            n = self.integral.norb
            eri = np.asarray(self.integral.H2["ccdd"], dtype=np.double)
            fmt, spin_dim = integral.get_eri_format(eri, n)
            if spin_dim == 0:
                eri = eri[None]
            self._dev = (ctx, [_block_to_dev_s4(ctx, blk, fmt, n) for blk in eri], n * (n + 1) // 2)
        return self._dev

    def HF(self, DiisDim=12, MaxIter=50, InitGuess=None, tol=1e-10, Mu=None, do_diis=True, alpha=None, beta=np.inf, fit_spin=True,
           conv_tol_grad=None):
        """R / U(I)HF (solver/scf.py:954-1043) -> (E, rho).  RHF: rho = make_rdm1()[None] / 2; UHF: (2, n, n); a one-spin H1 is
        duplicated for UHF; Mu (UHF) is a -/+ shift on the two halves of h1e[0] that the energy leaves out again."""
        log.eassert(self.sys_initialized and self.integral_initialized,
                    "components for Hartree-Fock (Bogoliubov) calculation are not ready\nsys_init = %s\nint_init = %s",
                    self.sys_initialized, self.integral_initialized)
        if self.bogoliubov:
            return self.HFB(0.0, DiisDim, MaxIter, InitGuess, tol)
        if beta < np.inf:
            raise NotImplementedError("finite temperature (PySCF's smearing_) is not built: the device driver fills by aufbau")
        if self.newton_ah and not self._newton_logged:
            log.info("newton_ah: the DIIS iteration is run; it reaches the same fixed point as the second-order solver")
            self._newton_logged = True
        n = self.integral.norb
        ovlp = self.integral.ovlp
        H1 = np.asarray(self.integral.H1["cd"], dtype=np.float64)
        nelec_a = (self.nelec + self.spin) // 2
        nelec_b = self.nelec - nelec_a
        log.eassert(0 <= nelec_b <= n and 0 <= nelec_a <= n, "nelec = %s, spin = %s do not fit %d orbitals", self.nelec, self.spin, n)
        h1e_no_mu = None
        if not self.spinRestricted:
            log.result("Unrestricted Hartree-Fock on the device")
            h1e = np.array(H1, copy=True)
            if len(h1e) == 1:
                h1e = np.asarray((h1e[0], h1e[0]))
            if Mu is not None:
                h1e_no_mu = h1e.copy()
                S = np.asarray(ovlp)
                S = S if S.ndim == 2 else S[0]
                nao = n // 2
                h1e[0, :nao, :nao] -= S[:nao, :nao] * Mu
                h1e[0, nao:, nao:] += S[nao:, nao:] * Mu
            nocc = [nelec_a, nelec_b]
        else:
            log.result("Restricted Hartree-Fock on the device")
            if nelec_a != nelec_b:
                raise NotImplementedError("restricted open-shell Hartree-Fock is not built (nelec = %s, spin = %s)" % (self.nelec, self.spin))
            h1e = H1[:1]
            nocc = [nelec_a]
            if InitGuess is not None and np.ndim(InitGuess) == 3:
                InitGuess = InitGuess[0]
        ctx, blocks, ld = self._device_eri()
        ns = 1 if self.spinRestricted else 2
        if ns == 2 and len(blocks) == 1:
            blocks = [blocks[0]] * 3
        log.eassert(len(blocks) >= (1 if ns == 1 else 3), "UHF needs the aa, bb and ab blocks of the ERI")
        if self.mf is not None:
            self.mf.close()
        self.mf = DeviceHF(ctx, n, self.spinRestricted, h1e, ovlp, blocks[:1] if ns == 1 else blocks[:3], ld, nocc, H0=self.integral.H0,
                           alpha=alpha, Mu=Mu if ns == 2 else None, h1e_no_mu=h1e_no_mu, DiisDim=DiisDim, MaxIter=MaxIter, tol=tol,
                           conv_tol_grad=conv_tol_grad, do_diis=do_diis)
        if self.no_kernel:
            E = rho = 0.0
        else:
            E = self.mf.kernel(dm0=InitGuess)
            rho = np.asarray(self.mf.make_rdm1())
            if self.spinRestricted:
                rho = rho[None] * 0.5          # NOTE the 0.5 factor and additional dim (solver/scf.py:1037-1038)
        log.result("Hartree-Fock convergence: %s", self.mf.converged)
        log.result("Hartree-Fock energy = %20.12f", E)
        self.doneHF = True
        return E, rho

    def HFB(self, *args, **kwargs):
        raise NotImplementedError("HFB: the Bogoliubov mean field of the solver layer is not built")

    def GHF(self, *args, **kwargs):
        raise NotImplementedError("GHF: the generalised mean field of the solver layer is not built")

    def GGHF(self, *args, **kwargs):
        raise NotImplementedError("GGHF: the generalised mean field of the solver layer is not built")

    def MP2(self, *args, **kwargs):
        raise NotImplementedError("MP2 is not wired into SCF: call solver.mp.run_mp2(scfsolver) (DESIGN.md K19, K20)")

    def GMP2(self, *args, **kwargs):
        raise NotImplementedError("GMP2: generalised references are not built (restricted / unrestricted MP2: solver.mp.run_mp2)")

    def get_mo(self):
        log.eassert(self.doneHF, "Hartree-Fock calculation is not done")
        c = np.asarray(self.mf.mo_coeff)
        return c[None] if c.ndim == 2 else c

    def get_mo_energy(self):
        log.eassert(self.doneHF, "Hartree-Fock calculation is not done")
        e = np.asarray(self.mf.mo_energy)
        return e[None] if np.asarray(self.mf.mo_coeff).ndim == 2 else e
