"""
Basis algebra with the reference's signatures (libdmet/basis_transform/make_basis.py),
every product running through the batched complex MFMA GEMM of libdmetk:

  multiply_basis         make_basis.py:923-962   (utils/misc.py:49-59 kdot)
  transform_h1_to_lo     make_basis.py:524-558
  transform_rdm1_to_lo   make_basis.py:590-618
  transform_rdm1_to_ao   make_basis.py:620-644
  transform_rdm1_to_ao_mol, transform_rdm2_to_ao_mol   make_basis.py:812-917 (no k-points, impurity-sized: numpy on the host)
"""
import numpy as np

from libdmet_preview_amd._lib import lib, get_ctx
from libdmet_preview_amd.utils.misc import add_spin_dim, get_spin_dim

_OP = {"N": 0, "T": 1, "C": 2}


def bgemm_dev(ctx, opA, opB, M, N, K, batch, A, strideA, B, strideB, C=None, strideC=None, alpha=1.0):
    """C[b] = alpha op(A[b]) op(B[b]) on device arrays (c128)."""
    if C is None:
        C = ctx.empty((batch, M, N), np.complex128)
    if strideC is None:
        strideC = M * N
    ctx.check(lib.dmk_zgemm_batched(ctx.h, _OP[opA], _OP[opB], int(M), int(N), int(K), int(batch), float(alpha),
                                    A.ptr, int(strideA), B.ptr, int(strideB), C.ptr, int(strideC)))
    return C


def _bgemm(opA, opB, a, b):
    """Host convenience: batched op(a[k]) @ op(b[k]) for (nk, r, c) stacks -> numpy c128."""
    ctx = get_ctx()
    a = np.ascontiguousarray(a, dtype=np.complex128)
    b = np.ascontiguousarray(b, dtype=np.complex128)
    nk = a.shape[0]
    M, K = (a.shape[1], a.shape[2]) if opA == "N" else (a.shape[2], a.shape[1])
    K2, N = (b.shape[1], b.shape[2]) if opB == "N" else (b.shape[2], b.shape[1])
    assert K == K2 and b.shape[0] == nk
    da, db = ctx.to_device(a), ctx.to_device(b)
    return bgemm_dev(ctx, opA, opB, M, N, K, nk, da, a.shape[1] * a.shape[2], db, b.shape[1] * b.shape[2]).get()


def _result(x, *inputs):
    """Reference dtype rule: np.result_type of the inputs (real only if everything is real)."""
    rt = np.result_type(*[np.asarray(i).dtype for i in inputs])
    if rt.kind != "c":
        return np.ascontiguousarray(x.real)
    return x


def _spin_stacks(*stacks):
    """Bring (nk, ., .) / (spin, nk, ., .) stacks to a common leading spin axis (a single channel is repeated).
    Returns the flattened (spin * nk, ., .) views, the spin count and whether ANY input carried a spin axis."""
    stacks = [np.asarray(x) for x in stacks]
    if any(x.ndim not in (3, 4) for x in stacks):
        raise ValueError("expected (nkpts, n, m) or (spin, nkpts, n, m) arrays, got shapes %s" % ([x.shape for x in stacks],))
    spin = get_spin_dim(stacks)
    flat = []
    for x in stacks:
        x = add_spin_dim(x, spin)
        flat.append(x.reshape((spin * x.shape[1],) + x.shape[2:]))
    return flat, spin, any(x.ndim == 4 for x in stacks)


def _unflatten(out, spin, keep_spin):
    return out.reshape((spin, out.shape[0] // spin) + out.shape[1:]) if keep_spin else out


def multiply_basis(C_ao_lo, C_lo_eo):
    """C_ao_eo[s, k] = C_ao_lo[s, k] C_lo_eo[s, k] (make_basis.py:923-962); either factor may omit the spin axis."""
    try:
        (A, B), spin, keep = _spin_stacks(C_ao_lo, C_lo_eo)
    except ValueError:
        raise ValueError("invalid shape for multiply_basis: C_ao_lo shape %s, C_lo_eo shape: %s"
                         % (np.shape(C_ao_lo), np.shape(C_lo_eo)))
    return _result(_unflatten(_bgemm("N", "N", A, B), spin, keep), C_ao_lo, C_lo_eo)


def _triple(opL, L, Mid, opR, Rt):
    """op(L[k]) @ Mid[k] @ op(R[k]) for flat (nk, ., .) stacks, intermediates stay on the device."""
    ctx = get_ctx()
    L = np.ascontiguousarray(L, dtype=np.complex128)
    Mid = np.ascontiguousarray(Mid, dtype=np.complex128)
    Rt = np.ascontiguousarray(Rt, dtype=np.complex128)
    nk = L.shape[0]
    dL, dM, dR = ctx.to_device(L), ctx.to_device(Mid), ctx.to_device(Rt)
    m1, k1 = (L.shape[1], L.shape[2]) if opL == "N" else (L.shape[2], L.shape[1])
    n1 = Mid.shape[2]
    assert Mid.shape[1] == k1
    T = bgemm_dev(ctx, opL, "N", m1, n1, k1, nk, dL, L.shape[1] * L.shape[2], dM, Mid.shape[1] * Mid.shape[2])
    k2, n2 = (Rt.shape[1], Rt.shape[2]) if opR == "N" else (Rt.shape[2], Rt.shape[1])
    assert k2 == n1
    out = bgemm_dev(ctx, "N", opR, m1, n2, k2, nk, T, m1 * n1, dR, Rt.shape[1] * Rt.shape[2])
    return out.get()


def transform_h1_to_lo(h_ao_ao, C_ao_lo):
    r"""h^{LO}[s, k] = C^{\dagger} h^{AO} C (make_basis.py:524-558).  A scalar (or one scalar per spin) stands for that
    multiple of the all-ones matrix and is only broadcast."""
    h_ao_ao = np.asarray(h_ao_ao)
    C_ao_lo = np.asarray(C_ao_lo)
    nkpts, nlo = C_ao_lo.shape[-3], C_ao_lo.shape[-1]
    if h_ao_ao.ndim <= 1:
        ones = np.ones((nkpts, nlo, nlo), dtype=np.result_type(h_ao_ao.dtype, C_ao_lo.dtype))
        return ones * h_ao_ao if h_ao_ao.ndim == 0 else np.asarray([ones * x for x in h_ao_ao])
    (H, Cf), spin, keep = _spin_stacks(h_ao_ao, C_ao_lo)
    return _result(_unflatten(_triple("C", Cf, H, "N", Cf), spin, keep), h_ao_ao, C_ao_lo)


def transform_rdm1_to_lo(dm_ao_ao, C_ao_lo, S_ao_ao):
    r"""\gamma^{LO} = C^{-1} \gamma^{AO} (C^{-1})^{\dagger} with C^{-1} = C^{\dagger} S (make_basis.py:590-618); the overlap has
    no spin axis."""
    (D, Cf, Sf), spin, _ = _spin_stacks(dm_ao_ao, C_ao_lo, S_ao_ao)
    keep = np.ndim(dm_ao_ao) == 4 or np.ndim(C_ao_lo) == 4
    Cinv = _bgemm("C", "N", Cf, Sf)
    return _result(_unflatten(_triple("N", Cinv, D, "C", Cinv), spin, keep), dm_ao_ao, C_ao_lo, S_ao_ao)


def transform_rdm1_to_ao(dm_lo_lo, C_ao_lo):
    r"""\gamma^{AO} = C \gamma^{LO} C^{\dagger} (make_basis.py:620-644)."""
    (D, Cf), spin, keep = _spin_stacks(dm_lo_lo, C_ao_lo)
    return _result(_unflatten(_triple("N", Cf, D, "C", Cf), spin, keep), dm_lo_lo, C_ao_lo)



# ---- molecular (no k-points) densities of an impurity solver: a few dozen orbitals, numpy on the host -----------------------------

def _mol_spin(C_ao_mo, nspin):
    """C with a leading spin axis of nspin (one set of orbitals is repeated)"""
    C = np.asarray(C_ao_mo)
    if C.ndim == 2:
        C = C[np.newaxis]
    if C.shape[0] not in (1, nspin):
        raise ValueError("orbitals of %d spin channels for a density of %d" % (C.shape[0], nspin))
    return C if C.shape[0] == nspin else np.asarray([C[0]] * nspin)


def transform_rdm1_to_ao_mol(dm_mo_mo, C_ao_mo):
    r"""\gamma^{AO} = C \gamma^{MO} C^{\dagger} without k-points (make_basis.py:812-834).  The spin axis comes from the orbitals; a
    density without one is shared by their spin channels, orbitals without one serve every spin channel of the density."""
    dm, C = np.asarray(dm_mo_mo), np.asarray(C_ao_mo)
    if dm.ndim == 2 and C.ndim == 2:
        return C @ dm @ C.conj().T
    nspin = max(dm.shape[0] if dm.ndim == 3 else 1, C.shape[0] if C.ndim == 3 else 1)
    C = _mol_spin(C, nspin)
    dm = _mol_spin(dm, nspin)
    return np.asarray([C[s] @ dm[s] @ C[s].conj().T for s in range(nspin)])


def transform_rdm2_to_ao_mol(rdm2_mo, C_ao_mo):
    r"""\Gamma^{AO}_{pqrs} = \sum C_{pi} C^*_{qj} C_{rk} C^*_{sl} \Gamma^{MO}_{ijkl} without k-points (make_basis.py:866-917): one
    block (4-d, or a spin axis of 1) with one set of orbitals, or the blocks aa, ab, bb (spin axis of 3) with the orbitals of the
    first pair of indices from the first and of the second pair from the second spin of the block."""
    g, C = np.asarray(rdm2_mo), np.asarray(C_ao_mo)
    one = lambda x, Ca, Cb: np.einsum("pi,qj,rk,sl,ijkl->pqrs", Ca, Ca.conj(), Cb, Cb.conj(), x, optimize=True)
    if g.ndim == 4:
        if C.ndim != 2:
            raise ValueError("a two-particle density without a spin axis needs one set of orbitals")
        return one(g, C, C)
    if g.shape[0] == 1:
        C = _mol_spin(C, 1) if C.ndim == 2 or C.shape[0] == 1 else C
        return one(g[0], C[0], C[0])[np.newaxis]
    if g.shape[0] != 3:
        raise ValueError("a two-particle density with a spin axis of %d (1, or 3: aa, ab, bb)" % g.shape[0])
    C = _mol_spin(C, 2)
    return np.asarray([one(g[0], C[0], C[0]), one(g[1], C[0], C[1]), one(g[2], C[1], C[1])])
