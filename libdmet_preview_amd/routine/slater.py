"""
Schmidt-decomposition bath with the reference's entry point
(libdmet/routine/slater.py:98-318: get_emb_basis / embBasis, SVD and eig flavours).

The SVD flavour never materialises `lattice.expand(rdm1)` (slater.py:167-171): the env x imp block is
gathered on the device from the stripe by index arithmetic, factorised (Householder QR + Jacobi SVD,
dmk_bath_svd), thresholded on the host (`(sigma >= tol_bath).sum()`, slater.py:181-185) and
orthogonalised / scattered by dmk_bath_assemble (slater.py:200-213, lo/lowdin.py:83-101).

get_emb_Ham (slater.py:320-704) completes the exit of the path: H2 from the DF transform (or the cell-local
4-index transform for models), H1 = basis^H (hcore + vhf) basis - JK_emb with JK_emb from dmk_jk_s4.
"""
import ctypes as C
from math import sqrt
try:
    from collections.abc import Iterable
except ImportError:  # pragma: no cover
    from collections import Iterable

import numpy as np

from libdmet_preview_amd._lib import lib, mesh3, get_ctx
from libdmet_preview_amd.routine import ftsystem
from libdmet_preview_amd.routine.fit import minimize
from libdmet_preview_amd.routine.mfd import check_nelec as mfd_check_nelec
from libdmet_preview_amd.settings import IMAG_DISCARD_TOL
from libdmet_preview_amd.utils.misc import max_abs
from libdmet_preview_amd.basis_transform.eri_transform import get_emb_eri, get_unit_eri
from libdmet_preview_amd.routine.slater_helper import *       # noqa: F401,F403  (reference: slater.py:35)
from libdmet_preview_amd.routine.slater_helper import (transform_trans_inv, transform_trans_inv_k, transform_local,
                                                       transform_imp, transform_eri_local, unit2emb)
from libdmet_preview_amd.solver.scf import _get_jk, _get_veff, _get_veff_ghf
from libdmet_preview_amd.system import integral
from libdmet_preview_amd.utils import logger as log
from libdmet_preview_amd.utils.misc import add_spin_dim


def _index_sets(lattice, imp_idx, val_idx, valence_bath):
    ncells, nlo = lattice.ncells, lattice.nscsites
    imp_idx_bath = list(val_idx) if valence_bath else list(imp_idx)
    bath_set, imp_set = set(imp_idx_bath), set(imp_idx)
    env_idx = [i for i in range(ncells * nlo) if i not in bath_set]
    virt_mask = [i in imp_set for i in env_idx]
    return imp_idx_bath, np.asarray(env_idx, dtype=np.int32), np.asarray(virt_mask, dtype=np.int32)


def get_emb_basis(lattice, rho=None, local=True, kind='svd', **kwargs):
    """Embedding basis C_lo_eo for a Slater determinant, shape (spin, ncells, nlo, nemb)."""
    if rho is None:
        rho = lattice.rdm1_lo_R
    if not local:
        # the reference calls `__embBasis_phsymm` here (slater.py:105-106), a name its module never defines: the branch raises
        # NameError there; nothing to mirror
        raise NotImplementedError("non-local (particle-hole symmetric) Slater bath: the reference's own branch calls an undefined "
                                  "function (routine/slater.py:106); use routine.bcs.embBasis(local=False) for the quasiparticle bath")
    rho = np.asarray(rho).real
    if kind == 'svd':
        return _get_emb_basis_svd(lattice, rho, **kwargs)
    elif kind == 'eig':
        return _get_emb_basis_eig(lattice, rho, **kwargs)
    raise ValueError("get_emb_basis: Unknown kind %s" % kind)


embBasis = get_emb_basis


def bath_svd_dev(ctx, kmesh, nlo, d_rdm1_s, d_env, nenv, d_col, nb):
    d_sigma = ctx.empty((nb,), np.float64)
    d_U = ctx.empty((nenv, nb), np.float64)
    ctx.check(lib.dmk_bath_svd(ctx.h, mesh3(kmesh), int(nlo), d_rdm1_s.ptr, d_env.ptr, int(nenv), d_col.ptr,
                               int(nb), d_sigma.ptr, d_U.ptr))
    return d_sigma, d_U


def orthonormal_completion(U, keep, null):
    """Overwrite the columns `null` of U (nenv, nb) in place with unit vectors orthogonal to the columns `keep` and to each other
    (host numpy; see complete_null_columns)."""
    nenv = U.shape[0]
    Q = U[:, keep].copy()
    if Q.shape[1] + len(null) > nenv:
        raise ValueError("complete_null_columns: %d kept + %d null columns do not fit %d environment rows"
                         % (Q.shape[1], len(null), nenv))
    for j in null:
        # the unit vector that is furthest from span(Q): its residual norm^2 is 1 - |Q^T e_i|^2 = 1 - sum_c Q[i, c]^2, and the
        # largest of them is >= (nenv - rank Q) / nenv > 0 -- no threshold to miss, no index to run past
        resid = 1.0 - (Q * Q).sum(axis=1)
        i = int(np.argmax(resid))
        e = np.zeros(nenv)
        e[i] = 1.0
        for _ in range(2):
            e -= Q @ (Q.T @ e)
        nrm = float(np.linalg.norm(e))
        if not nrm > 1e-8:
            raise ValueError("complete_null_columns: no direction left outside the kept columns (residual %.1e)" % nrm)
        U[:, j] = e / nrm
        Q = np.concatenate([Q, U[:, j:j + 1]], axis=1)
    return U


def complete_null_columns(ctx, sigma, d_U, nenv, nb, ncheck=None):
    """Where the reference keeps left singular vectors whatever their singular value -- every column in routine/bcs.py:46, 84, the first
    `nbath` columns when the caller fixes `nbath` (routine/slater.py:177-186, with its "Zero singular value exists" warning) --
    LAPACK returns an orthonormal completion for the singular values that vanish (an impurity that is not entangled with part of the
    environment; a band that is full or empty at every k gives A = 0).  The device factorisation forms u_j = A v_j / sigma_j, which has
    no direction there: such columns are replaced by an orthonormal completion (unit vectors orthogonalised against the columns kept,
    twice), so that the embedding basis stays orthonormal.  Which completion is a matter of convention in the reference as well.
    Rare and small: done on the host."""
    sigma = np.asarray(sigma, dtype=float).reshape(-1)[:nb]
    smax = float(sigma.max()) if nb else 0.0
    ncheck = nb if ncheck is None else min(int(ncheck), nb)             # only the first `ncheck` columns are used by the caller
    null = [j for j in range(ncheck) if not sigma[j] > 4.0 * nenv * np.finfo(float).eps * smax]
    if not null or nenv < nb:
        return
    U = d_U.get().reshape(nenv, nb)
    orthonormal_completion(U, [j for j in range(ncheck) if j not in null], null)
    ctx.check(lib.dmk_memcpy_h2d(ctx.h, d_U.ptr, np.ascontiguousarray(U).ctypes.data, U.nbytes))


def bath_svd_batched_dev(ctx, kmesh, nlo, d_rdm1, spin, d_env, nenv, d_col, nb):
    """All spin channels in one chain of launches: d_rdm1 (spin, ncells, nlo, nlo) -> sigma (spin, nb), U (spin, nenv, nb)."""
    d_sigma = ctx.empty((spin, nb), np.float64)
    d_U = ctx.empty((spin, nenv, nb), np.float64)
    ctx.check(lib.dmk_bath_svd_batched(ctx.h, mesh3(kmesh), int(nlo), int(spin), d_rdm1.ptr, int(d_rdm1.size // spin), d_env.ptr,
                                       int(nenv), d_col.ptr, int(nb), d_sigma.ptr, d_U.ptr))
    return d_sigma, d_U


def bath_assemble_dev(ctx, d_U, nenv, nb, nbath, d_virt, orth, d_env, d_imp, nimp, nsites, ncol, d_basis):
    ctx.check(lib.dmk_bath_assemble(ctx.h, d_U.ptr, int(nenv), int(nb), int(nbath), d_virt.ptr, 1 if orth else 0,
                                    d_env.ptr, d_imp.ptr, int(nimp), int(nsites), int(ncol), d_basis.ptr))
    return d_basis


# environment / lattice dimension above which the eigenvalue-flavoured baths use the many-workgroup eigensolver
# (csrc/eigh_large.hip); up to it, one workgroup per matrix (csrc/eigh.hip, whose limit this is)
EIGH_LARGE_MIN = 2000


def stripe_gather_dev(ctx, kmesh, nlo, d_stripe, d_rows, d_cols, d_out):
    """d_out (nrow, ncol) = expand(stripe)[rows][:, cols] by index arithmetic on the device (dmk_stripe_gather)."""
    ctx.check(lib.dmk_stripe_gather(ctx.h, mesh3(kmesh), int(nlo), d_stripe.ptr, int(d_rows.size), d_rows.ptr, int(d_cols.size),
                                    d_cols.ptr, d_out.ptr))
    return d_out


def eigh_large_selected(ctx, d_A, n, select):
    """Selected eigenpairs of the real symmetric device matrix d_A (n x n, lower triangle referenced, left unchanged): every
    eigenvalue `ew` (host, ascending), then the eigenvectors of the indices `select(ew)` returns (ascending) as the ROWS of a device
    array (max(m, 1), n).  The host applies its comparisons to the very doubles the device computed -- the reference's
    `abs(e) > tol and abs(1 - e) > tol` (slater.py:283-287) or `ev[:, -nemb:]` (spinless.py:306) -- and the device computes
    exactly those vectors.  Returns (ew, idx, d_Vt)."""
    h = C.c_void_p()
    d_w = ctx.empty((n,), np.float64)
    ctx.check(lib.dmk_eighl_factor(ctx.h, int(n), d_A.ptr, int(n), d_w.ptr, C.byref(h)))
    try:
        ew = d_w.get()
        idx = np.ascontiguousarray(select(ew), dtype=np.int32)
        d_Vt = ctx.empty((max(len(idx), 1), n), np.float64)
        ctx.check(lib.dmk_eighl_vectors(h, int(len(idx)), idx.ctypes.data_as(C.c_void_p), d_Vt.ptr))
    finally:
        lib.dmk_eighl_free(h)
    return ew, idx, d_Vt


def _get_emb_basis_svd(lattice, rdm1, **kwargs):
    imp_idx = kwargs.get("imp_idx", lattice.imp_idx)
    val_idx = kwargs.get("val_idx", lattice.val_idx)
    valence_bath = kwargs.get("valence_bath", True)
    orth = kwargs.get("orth", True)
    tol_bath = kwargs.get("tol_bath", 1e-9)
    nbath = kwargs.get("nbath", None)
    loc_method = kwargs.get("localize_bath", None)

    ncells, nlo = lattice.ncells, lattice.nscsites
    imp_idx = list(imp_idx)
    imp_idx_bath, env_idx, virt_mask = _index_sets(lattice, imp_idx, val_idx, valence_bath)
    nimp = len(imp_idx)
    rdm1 = np.asarray(rdm1)
    if rdm1.ndim == 3:
        rdm1 = rdm1[np.newaxis]
    assert rdm1.shape[-3:] == (ncells, nlo, nlo)
    spin = rdm1.shape[0]
    # same nbath_final seeds as the two branches of slater.py:167-175
    nbath_final = len(imp_idx_bath) if np.max(imp_idx_bath) >= nlo - 1 else nlo
    nb, nenv = len(imp_idx_bath), len(env_idx)
    nsites, ncol = ncells * nlo, nimp * 2

    ctx = get_ctx()
    d_env = ctx.to_device(env_idx, np.int32)
    d_col = ctx.to_device(np.asarray(imp_idx_bath), np.int32)
    d_virt = ctx.to_device(virt_mask, np.int32)
    d_imp = ctx.to_device(np.asarray(imp_idx), np.int32)
    d_rdm1 = ctx.to_device(rdm1, np.float64)
    basis = np.zeros((spin, nsites, ncol))
    d_sigma_all, d_U_all = bath_svd_batched_dev(ctx, lattice.kmesh, nlo, d_rdm1, spin, d_env, nenv, d_col, nb)
    sigma_all = d_sigma_all.get()
    for s in range(spin):
        d_U = d_U_all.offset(s * nenv * nb, (nenv, nb))
        sigma = sigma_all[s]
        nbath_s = int((sigma >= tol_bath).sum()) if nbath is None else int(nbath)
        nzero = int(np.sum(np.abs(sigma[:nbath_s]) < tol_bath))
        log.debug(0, "Zero singular values number: %s", nzero)
        if nzero > 0:
            log.warn("Zero singular value exists, \nthis may cause numerical instability.")
            complete_null_columns(ctx, sigma, d_U, nenv, nb, ncheck=nbath_s)
        d_basis = ctx.empty((nsites, ncol), np.float64)
        bath_assemble_dev(ctx, d_U, nenv, nb, nbath_s, d_virt, orth, d_env, d_imp, nimp, nsites, ncol, d_basis)
        basis[s] = d_basis.get()
        if loc_method is not None and nbath_s > 0:
            # localisation of the (orthonormalised) bath columns (slater.py:204-210, routine/localizer.py)
            from libdmet_preview_amd.routine import localizer
            if not lattice.is_model:
                log.warn("Only model is currently supported for localization of bath.")
            cols = np.arange(nimp, nimp + nbath_s)
            basis[s][np.ix_(env_idx, cols)] = localizer.localize_bath(basis[s][np.ix_(env_idx, cols)], method=loc_method)
        nbath_final = min(nbath_final, nbath_s)
    log.debug(0, "nimp : %d", nimp)
    log.debug(0, "nbath: %d", nbath_final)
    return np.ascontiguousarray(basis[:, :, :nimp + nbath_final]).reshape(spin, ncells, nlo, nimp + nbath_final)


def _get_emb_basis_eig(lattice, rdm1, **kwargs):
    """Eigen-decomposition of the env-env block (slater.py:224-318).  Up to EIGH_LARGE_MIN environment orbitals the block is cut
    from the expanded matrix on the host and goes through the one-workgroup solver; above, it is gathered on the device from
    the stripe (dmk_stripe_gather) and only the eigenvectors the reference's comparison keeps are computed (eigh_large_selected)."""
    imp_idx = kwargs.get("imp_idx", lattice.imp_idx)
    val_idx = kwargs.get("val_idx", lattice.val_idx)
    valence_bath = kwargs.get("valence_bath", True)
    orth = kwargs.get("orth", True)
    tol_bath = kwargs.get("tol_bath", 1e-9)
    ncells, nlo = lattice.ncells, lattice.nscsites
    imp_idx = list(imp_idx)
    imp_idx_bath, env_idx, virt_mask = _index_sets(lattice, imp_idx, val_idx, valence_bath)
    nimp, nenv = len(imp_idx), len(env_idx)
    rdm1 = np.asarray(rdm1)
    if rdm1.ndim == 3:
        rdm1 = rdm1[np.newaxis]
    spin = rdm1.shape[0]
    ctx = get_ctx()
    select = lambda ew: [i for i, e in enumerate(ew) if abs(e) > tol_bath and abs(1 - e) > tol_bath]       # noqa: E731
    if nenv > EIGH_LARGE_MIN:
        d_rdm1 = ctx.to_device(rdm1, np.float64)
        d_env = ctx.to_device(env_idx, np.int32)
        d_A = ctx.empty((nenv, nenv), np.float64)
        kept = []
        for s in range(spin):
            stripe_gather_dev(ctx, lattice.kmesh, nlo, d_rdm1.offset(s * ncells * nlo * nlo, (ncells, nlo, nlo)), d_env, d_env, d_A)
            _, idx, d_sel = eigh_large_selected(ctx, d_A, nenv, select)
            kept.append(d_sel.get()[:len(idx)])
    else:
        env_env = lattice.expand(rdm1)[:, env_idx][:, :, env_idx]
        d_A = ctx.to_device(env_env, np.float64)
        d_w = ctx.empty((spin, nenv), np.float64)
        d_Vt = ctx.empty((spin, nenv, nenv), np.float64)
        ctx.check(lib.dmk_eigh_batched_real(ctx.h, nenv, spin, d_A.ptr, d_w.ptr, d_Vt.ptr))
        ew, Vt = d_w.get(), d_Vt.get()
        kept = [Vt[s][select(ew[s])] for s in range(spin)]
    nb = len(kept[0])
    if any(len(k) != nb for k in kept):
        raise ValueError("eig bath: spin sectors give different numbers of bath orbitals")
    nsites = ncells * nlo
    basis = np.zeros((spin, nsites, nimp + nb))
    d_env = ctx.to_device(env_idx, np.int32)
    d_virt = ctx.to_device(virt_mask, np.int32)
    d_imp = ctx.to_device(np.asarray(imp_idx), np.int32)
    for s in range(spin):
        if nb == 0:
            basis[s, imp_idx, :nimp] = np.eye(nimp)
            continue
        U = np.ascontiguousarray(kept[s].T)                 # (nenv, nb) columns = kept eigenvectors
        d_U = ctx.to_device(U, np.float64)
        d_basis = ctx.empty((nsites, nimp + nb), np.float64)
        bath_assemble_dev(ctx, d_U, nenv, nb, nb, d_virt, orth, d_env, d_imp, nimp, nsites, nimp + nb, d_basis)
        basis[s] = d_basis.get()
    return basis.reshape(spin, ncells, nlo, nimp + nb)


# ---------------------------------------------------------------------------------------------
# embedding Hamiltonian (routine/slater.py:320-704)
# ---------------------------------------------------------------------------------------------

def transform_h1(H1_k, basis_k):
    """(spin, nbasis, nbasis) = per spin (1/nk) Re sum_k basis_k^H H1_k basis_k   (slater.py:682-689)."""
    basis_k = np.asarray(basis_k)
    spin, nbasis = basis_k.shape[0], basis_k.shape[-1]
    H1_k = add_spin_dim(H1_k, spin, non_spin_dim=3)
    H1 = np.empty((spin, nbasis, nbasis))
    for s in range(spin):
        H1[s] = transform_trans_inv_k(basis_k[s], H1_k[s])
    return H1


foldRho_k = transform_h1


def foldRho(rho, lattice, basis):
    """Density matrix into the embedding space from the real-space stripe (slater.py:691-701)."""
    spin, nbasis = rho.shape[0], basis.shape[-1]
    rdm1_emb = np.empty((spin, nbasis, nbasis))
    for s in range(spin):
        rdm1_emb[s] = transform_trans_inv(basis[s], lattice, rho[s])
    return rdm1_emb


def get_veff(rdm1, eri, hyb=1.0, ghf=False, hyb_j=1.0):
    """Effective potential of the embedding Hamiltonian (slater.py:477-523); rdm1 is spin traced if restricted."""
    rdm1 = np.asarray(rdm1)
    if ghf:
        # ONE spin-orbital density against a spinless ERI (slater.py:489-506): J - hyb K, J scaled by hyb_j in the DFT branches
        assert rdm1.ndim == 2
        if hyb == 1.0:
            return _get_veff_ghf(rdm1, eri)
        vj, vk = _get_jk(rdm1, eri, with_j=True, with_k=hyb != 0.0)
        vj0 = vj[0] if hyb_j == 1.0 else vj[0] * hyb_j
        return vj0 if hyb == 0.0 else vj0 - (vk[0] * hyb)
    if rdm1.ndim == 2:
        rdm1 = rdm1[None]
    spin = rdm1.shape[0]
    if hyb == 1.0:      # HF
        veff = _get_veff(rdm1, eri)
    elif hyb == 0.0:    # pure DFT, J only
        vj = _get_jk(rdm1, eri, with_j=True, with_k=False)[0]
        veff = vj if spin == 1 else vj[0] + vj[1]
    else:               # hybrid DFT
        vj, vk = _get_jk(rdm1, eri, with_j=True, with_k=True)
        veff = vj - vk * (hyb * 0.5) if spin == 1 else vj[0] + vj[1] - vk * hyb
    return veff


def _embHam2e(lattice, basis, vcor, local, int_bath=True, last_aabb=True, **kwargs):
    """H2_emb (slater.py:372-475): DF transform for ab-initio lattices, cell-local 4-index transform for models."""
    nbasis, spin = basis.shape[-1], basis.shape[0]
    if lattice.is_model:
        LatH2 = lattice.getH2(compact=False, kspace=False)
        log.eassert(local, "non local bath is outside the HIP path")
        if lattice.H2_format == 'local':
            if int_bath:
                H2 = transform_eri_local(basis, lattice, LatH2)
            else:
                H2 = unit2emb(np.asarray((LatH2,) * (spin * (spin + 1) // 2)), nbasis)
        elif lattice.H2_format in ("nearest", "full", "spin local"):
            # bare bath only (slater.py:407-426): the impurity block of the lattice ERI -- LatH2[0] of a neighbour list,
            # LatH2[0, 0, 0] of a full cell-resolved tensor, LatH2[i] per spin block -- zero-padded to the embedding size
            if int_bath:
                raise NotImplementedError
            nblk = spin * (spin + 1) // 2
            LatH2 = np.asarray(LatH2)
            if lattice.H2_format == "nearest":
                blocks = np.asarray((LatH2[0],) * nblk)
            elif lattice.H2_format == "full":
                blocks = np.asarray((LatH2[0, 0, 0],) * nblk)
            else:
                blocks = LatH2[:nblk]
            H2 = unit2emb(np.ascontiguousarray(blocks), nbasis)
        else:
            raise ValueError("unknown H2_format %s" % lattice.H2_format)
    else:
        opts = dict(kscaled_center=kwargs.get("kscaled_center", None), symmetry=lattice.eri_symmetry,
                    max_memory=kwargs.get("max_memory", None), swap_idx=kwargs.get("swap_idx", None),
                    t_reversal_symm=kwargs.get("t_reversal_symm", True), incore=kwargs.get("incore", True),
                    fout=kwargs.get("fout", "H2.h5"), use_mpi=kwargs.get("use_mpi", False))
        if int_bath:
            H2 = get_emb_eri(lattice.cell, lattice.df, C_ao_lo=lattice.C_ao_lo, basis=basis, **opts)
            if last_aabb and isinstance(H2, np.ndarray) and H2.shape[0] == 3:
                H2 = H2[[0, 2, 1]]
        else:
            H2 = get_unit_eri(lattice.cell, lattice.df, C_ao_lo=lattice.C_ao_lo, **opts)
            if last_aabb and isinstance(H2, np.ndarray) and H2.shape[0] == 3:
                H2 = H2[[0, 2, 1]]
            H2 = unit2emb(H2, nbasis)
    if isinstance(H2, np.ndarray):
        log.info("H2 memory allocated size = %d MB", H2.size * 8. / 1024 / 1024)
    return H2


def _embHam1e(lattice, basis, vcor, H2_emb, int_bath=True, add_vcor=False, **kwargs):
    """One-body part of the embedding Hamiltonian and the embedding overlap for Hartree-Fock mean fields
    (reference behaviour: routine/slater.py:525-680); also leaves `lattice.JK_core` behind, like the reference.

    Three regimes decide what the bare fold B^H fock B is corrected by:
      interacting bath      -- the mean-field potential of the EMBEDDED density with the embedding ERI is taken out
                               (it is double counted by the impurity solver), JK_core = H1 - hcore_emb;
      bare bath, hcore      -- `use_hcore_as_emb_ham`: nothing to correct, no JK_core;
      bare bath, Fock       -- the impurity-local JK (given as `JK_imp`, else rebuilt from the embedded density) is
                               taken out.
    A bare bath always carries the correlation potential; with `add_vcor` an interacting one does too (on the
    environment only unless `fitting`).  Every fold (1/nk) Re sum_k B_k^H O_k B_k runs on the device."""
    unsupported = [k for k in ("dft", "qsgw", "vxc_dc") if kwargs.get(k, False)]
    if unsupported:
        raise NotImplementedError("%s embedding Hamiltonian is outside the HIP path" % unsupported[0])
    spin = basis.shape[0]
    basis_k = lattice.R2k_basis(basis)
    fold = lambda op_k: transform_h1(op_k, basis_k)
    eri = H2_emb if isinstance(H2_emb, np.ndarray) else np.asarray(H2_emb["ccdd"])
    embedded_density = lambda: foldRho_k(lattice.rdm1_lo_k, basis_k)

    hcore_emb = fold(lattice.getH1(kspace=True))
    ovlp_emb = fold(lattice.get_ovlp(kspace=True))
    if ovlp_emb.ndim == 3 and len(ovlp_emb) == 1:
        ovlp_emb = ovlp_emb[0]
    fock_k = lattice.getFock(kspace=True)
    JK_imp = lattice.get_JK_imp()                      # read before any branch: the reference queries it up front

    if int_bath:
        if not lattice.is_model:
            fock_k = lattice.hcore_lo_k + lattice.vhf_lo_k
        H1 = fold(fock_k) - get_veff(embedded_density(), eri)
        lattice.JK_core = H1 - hcore_emb
        with_vcor = add_vcor
    elif lattice.use_hcore_as_emb_ham:
        H1, lattice.JK_core, with_vcor = hcore_emb, None, True
    else:
        if JK_imp is None:
            local_jk = get_veff(embedded_density(), eri)
        else:
            JK_imp = np.asarray(JK_imp)
            per_spin = (lambda s: JK_imp) if JK_imp.ndim == 2 else (lambda s: JK_imp[s])
            local_jk = np.asarray([transform_imp(basis[s], lattice, per_spin(s)) for s in range(spin)])
        H1 = fold(fock_k) - local_jk
        lattice.JK_core = H1 - hcore_emb
        with_vcor = True

    if with_vcor:
        log.eassert(vcor.islocal(), "nonlocal correlation potential cannot be treated in this routine")
        on_impurity_too = bool(kwargs.get("fitting", False))
        v = vcor.get()
        for s in range(spin):
            H1[s] += transform_local(basis[s], lattice, v[s])
            if not on_impurity_too:
                H1[s] -= transform_imp(basis[s], lattice, v[s])
    return H1, ovlp_emb


def get_emb_Ham(lattice, basis, vcor, local=True, **kwargs):
    """
    Embedding Hamiltonian (slater.py:320-370): two-body part first (JK_emb needs it), then the one-body part.

    Kwargs: incore, H2_given (ndarray), int_bath, add_vcor, fitting, and the ERI-transform options.
    Returns (ImpHam, None) with ImpHam an integral.Integral.
    """
    basis = np.asarray(basis)
    spin, nbasis = basis.shape[0], basis.shape[-1]
    log.info("Two-body part")
    H2_given = kwargs.get("H2_given", None)
    if H2_given is None:
        if kwargs.get("H2_fname", None) is not None:
            raise NotImplementedError("H2_fname (HDF5) is not available; pass H2_given")
        H2 = _embHam2e(lattice, basis, vcor, local, **kwargs)
    else:
        log.debug(1, "Using specified H2 array.")
        H2 = H2_given
    log.info("One-body part")
    H1, ovlp_emb = _embHam1e(lattice, basis, vcor, H2, **kwargs)
    H0 = lattice.getH0()
    if isinstance(H2, np.ndarray):
        H2 = {"ccdd": H2}
    ImpHam = integral.Integral(nbasis, spin == 1, False, H0, {"cd": H1}, H2, ovlp=ovlp_emb)
    return ImpHam, None


embHam = get_emb_Ham


# ---------------------------------------------------------------------------------------------
# correlation-potential fit in the embedding space (routine/slater.py:851-1329)
# ---------------------------------------------------------------------------------------------

def get_dV_dparam_dev(ctx, vcor, basis, thr=1e-7, rows=None, lattice=None):
    """Device dV_dparam (nparam, spin, npair) f64, tril packed (slater.py:851-877 with transform_local_sparseH,
    slater_helper.py:91-100): gathered from the cell Gram matrix of the basis rows that any parameter touches.
    `rows` = (p_lo, p_hi): only that range of parameters (a rank's shard of the table), shape (p_hi - p_lo, spin, npair).
    A potential that is not local (vcor.VcorNonLocal, or the reference's own object of that kind) goes to _dV_dparam_cells_dev;
    `lattice` supplies the cell arithmetic when the potential does not carry one."""
    basis = np.asarray(basis, dtype=np.float64)
    spin, ncells, nlo, nb = basis.shape
    npair = nb * (nb + 1) // 2
    nparam = vcor.length()
    if not vcor.is_local():
        return _dV_dparam_cells_dev(ctx, vcor, basis, lattice if lattice is not None else getattr(vcor, "lattice", None), rows=rows)
    if hasattr(vcor, "grad_entries"):                                # sparse description, same order as np.nonzero below
        gp, gb, gi, gj, gv = vcor.grad_entries()
        keep = (gb < spin) & (np.abs(gv) > thr)
        nz, vals = (gp[keep], gb[keep], gi[keep], gj[keep]), gv[keep]
    else:
        g = np.asarray(vcor.gradient())[:, :spin]                   # (nparam, spin, nlo, nlo)
        nz = np.nonzero(np.abs(g) > thr)                             # entries in (param, spin, row, col) order
        vals = g[nz]
    used = np.unique(np.concatenate([nz[2], nz[3]])) if len(nz[0]) else np.zeros(0, dtype=int)
    pos = -np.ones(nlo, dtype=np.int64)
    pos[used] = np.arange(len(used))
    p_lo, p_hi = (0, nparam) if rows is None else (int(rows[0]), int(rows[1]))
    d_dV = ctx.zeros((max(p_hi - p_lo, 1), spin, npair), np.float64)
    if len(used) == 0 or p_hi <= p_lo:
        return d_dV
    m = len(used) * nb
    for s in range(spin):
        sel = (nz[1] == s) & (nz[0] >= p_lo) & (nz[0] < p_hi)
        ip, zi, zj, zv = nz[0][sel], pos[nz[2][sel]], pos[nz[3][sel]], vals[sel]
        if len(ip) == 0:
            continue
        ents = np.unique(ip)                                          # parameters with entries in this spin block
        ptr = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(ents, ip), minlength=len(ents)))])
        d_X = ctx.to_device(np.ascontiguousarray(basis[s][:, used, :]).reshape(ncells, m))
        d_G = ctx.zeros((m, m), np.float64)
        ctx.check(lib.dmk_dgemm_tn_acc(ctx.h, m, ncells, 1.0, d_X.ptr, d_X.ptr, m, d_G.ptr, m))
        off = ((ents.astype(np.int64) - p_lo) * spin + s) * npair
        _gather_dV(ctx, d_G, m, nb, ptr, zi, zj, zv, off, d_dV)
    return d_dV


def _gather_dV(ctx, d_G, ldg, nb, ptr, zi, zj, zv, off, d_dV):
    """dV[off[e] + pair(p, q)] = sum over the entries ptr[e]:ptr[e+1] of zv * G[(zi, p), (zj, q)], 32768 parameters per launch."""
    for e0 in range(0, len(off), 32768):
        e1 = min(len(off), e0 + 32768)
        sl = slice(ptr[e0], ptr[e1])
        args = [ctx.to_device((ptr[e0:e1 + 1] - ptr[e0]).astype(np.int32)), ctx.to_device(zi[sl].astype(np.int32)),
                ctx.to_device(zj[sl].astype(np.int32)), ctx.to_device(zv[sl].astype(np.float64)),
                ctx.to_device(np.ascontiguousarray(off[e0:e1], dtype=np.int64))]
        ctx.check(lib.dmk_vcor_dV_dparam(ctx.h, e1 - e0, nb, d_G.ptr, ldg, args[0].ptr, args[1].ptr, args[2].ptr,
                                         args[3].ptr, args[4].ptr, d_dV.ptr))
        ctx.sync()                               # the index arrays die with this iteration


CELL_GRAM_DOUBLES = 1 << 28                      # 2 GiB of shifted Gram matrices per pass of _dV_dparam_cells_dev


def _dV_dparam_cells_dev(ctx, vcor, basis, lat, rows=None):
    """dV/dparam of a cell-resolved potential (vcor.VcorNonLocal), the `else` branch of slater.py:893-902.  The reference sends every
    parameter's gradient to k space and through transform_trans_inv_k, (1/nk) Re sum_k B_k^H g_k B_k; a unit entry g[R0, i, j] of
    it is the cell CORRELATION of two basis rows,  sum_R B[R, i, :]^T B[R - R0, j, :],  so the whole table is gathered from shifted
    Gram matrices  G_R0 = X^T X(. - R0)  of the touched rows X (one rectangular real GEMM for a group of cells R0), with the
    kernel of the local branch reading column block R0.  A parameter's entries sit on a cell and its inverse only
    (vcor.py:128-137), and such pairs are never split across passes."""
    spin, ncells, nlo, nb = basis.shape
    npair = nb * (nb + 1) // 2
    nparam = vcor.length()
    log.eassert(lat is not None, "dV_dparam of a non-local potential needs the lattice (cell arithmetic)")
    if hasattr(vcor, "cell_entries"):
        P, B, CELL, I, J = vcor.cell_entries()
        W = np.ones(len(P))
    else:                                                  # the reference's own object: dense (nparam, nblk, ncells, nlo, nlo) gradient
        g = np.asarray(vcor.gradient())
        P, B, CELL, I, J = np.nonzero(g)
        W = g[P, B, CELL, I, J]
    keep = B < spin
    P, B, CELL, I, J, W = P[keep], B[keep], CELL[keep], I[keep], J[keep], W[keep]
    p_lo, p_hi = (0, nparam) if rows is None else (int(rows[0]), int(rows[1]))
    d_dV = ctx.zeros((max(p_hi - p_lo, 1), spin, npair), np.float64)
    if len(P) == 0 or p_hi <= p_lo:
        return d_dV
    used = np.unique(np.concatenate([I, J]))
    pos = -np.ones(nlo, dtype=np.int64)
    pos[used] = np.arange(len(used))
    nu = len(used)
    m = nu * nb
    size = np.asarray(lat.csize, dtype=np.int64)
    where = np.asarray([lat.cell_idx2pos(R) for R in range(ncells)], dtype=np.int64) % size
    index_of = np.empty(ncells, dtype=np.int64)
    index_of[np.ravel_multi_index(tuple(where.T), tuple(size))] = np.arange(ncells)
    shift = index_of[np.ravel_multi_index(tuple(((where[:, None, :] - where[None, :, :]) % size).transpose(2, 0, 1)), tuple(size))]  # [R, R0] = R - R0
    mate = index_of[np.ravel_multi_index(tuple(((-where) % size).T), tuple(size))]                                            # -R
    present = set(int(R) for R in np.unique(CELL))
    groups = [[R] if mate[R] == R else [R, int(mate[R])] for R in sorted(present) if mate[R] >= R or int(mate[R]) not in present]
    per_pass = max(2, CELL_GRAM_DOUBLES // max(m * m, 1))
    passes, cur = [], []
    for grp in groups:
        if cur and len(cur) + len(grp) > per_pass:
            passes.append(cur)
            cur = []
        cur = cur + grp
    passes.append(cur)
    for cells in passes:
        cells = np.asarray(cells, dtype=np.int64)
        slot = -np.ones(ncells, dtype=np.int64)
        slot[cells] = np.arange(len(cells))
        width = len(cells) * m
        for s in range(spin):
            sel = (B == s) & (slot[CELL] >= 0) & (P >= p_lo) & (P < p_hi)
            if not sel.any():
                continue
            ip = P[sel]
            ents = np.unique(ip)
            ptr = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(ents, ip), minlength=len(ents)))])
            X = np.ascontiguousarray(basis[s][:, used, :]).reshape(ncells, m)
            d_X = ctx.to_device(X)
            d_Y = ctx.to_device(np.ascontiguousarray(X[shift[:, cells]]).reshape(ncells, width))
            d_G = ctx.zeros((m, width), np.float64)
            ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, m, width, ncells, 1.0, d_X.ptr, m, d_Y.ptr, width, d_G.ptr, width))
            off = ((ents.astype(np.int64) - p_lo) * spin + s) * npair
            _gather_dV(ctx, d_G, width, nb, ptr, pos[I[sel]], slot[CELL[sel]] * nu + pos[J[sel]], W[sel], off, d_dV)
    return d_dV


def get_active_projector_full(P_act, ovlp):
    """Projector from the full LO space onto an active space and back, P (P^H S P) P^H per spin and k point (slater.py:2195-2219).
    P_act: a list (spin, nkpts, nlo, nact); ovlp ((spin,) nkpts, nlo, nlo).  Returns (spin, nkpts, nlo, nlo)."""
    from libdmet_preview_amd.basis_transform.make_basis import _triple
    ovlp = np.asarray(ovlp)
    if ovlp.ndim == 3:
        ovlp = ovlp[None]
    spin, nkpts, nlo, _ = ovlp.shape
    assert len(P_act) == spin
    P_full = np.empty((spin, nkpts, nlo, nlo), dtype=ovlp.dtype)
    for s in range(spin):
        P = np.asarray(P_act[s])
        ovlp_act = _triple("C", P, ovlp[s], "N", P)
        out = _triple("N", P, ovlp_act, "C", P)
        P_full[s] = out if np.iscomplexobj(P_full) else out.real
    return P_full


def _projected_basis_rows(P_full, basis_k):
    """The rows the cell Gram matrix of get_dV_dparam_dev is built from when the basis is projected in k space (slater.py:878-892):
    C(k) = P_full(k) basis_k(k), and for a k-INDEPENDENT matrix g  Re (1/nk) sum_k C(k)^H g C(k) = sum_rows X^T g X with the
    real row stack X = [Re C(k); Im C(k)] / sqrt(nk) -- (spin, 2 nk, nlo, nb): the same shape of problem as the R-space basis."""
    from libdmet_preview_amd.basis_transform.make_basis import multiply_basis
    C_lo_eo = np.asarray(multiply_basis(np.asarray(P_full), np.asarray(basis_k)))
    nk = C_lo_eo.shape[-3]
    return np.ascontiguousarray(np.concatenate([C_lo_eo.real, C_lo_eo.imag], axis=-3) / sqrt(nk))


def get_dV_dparam(vcor, basis, basis_k, lattice, P_act=None, compact=True):
    """dV / dparam: (nparam, spin, npair) if compact else (nparam, spin, nbasis, nbasis).  `P_act`: the FULL projector
    (spin, nkpts, nlo, nlo) of get_active_projector_full, applied to basis_k (slater.py:878-892)."""
    if getattr(vcor, "is_vcor_kpts", False):
        raise NotImplementedError("get_dV_dparam: VcorKpoints has no gradient in the reference either (routine/vcor.py gradient())")
    ctx = get_ctx()
    spin, _, _, nbasis = np.asarray(basis).shape
    if not vcor.is_local():
        d = get_dV_dparam_dev(ctx, vcor, basis, lattice=lattice)   # the reference's non-local branch does not read P_act (slater.py:893-902)
    elif P_act is not None:
        if basis_k is None:
            basis_k = lattice.R2k_basis(np.asarray(basis))
        d = get_dV_dparam_dev(ctx, vcor, _projected_basis_rows(P_act, basis_k), thr=0.0)
    else:
        d = get_dV_dparam_dev(ctx, vcor, basis)
    if not compact:
        full = ctx.empty((vcor.length() * spin, nbasis, nbasis), np.float64)
        ctx.check(lib.dmk_sym_unpack(ctx.h, nbasis, vcor.length() * spin, d.ptr, None, full.ptr))
        d = full.reshape(vcor.length(), spin, nbasis, nbasis)
    vcor.grad = None           # release the gradient memory like the reference (slater.py:903-905)
    vcor.grad_k = None
    return d.get()


class EmbFitDevice(object):
    """errfunc / gradfunc of FitVcorEmb (slater.py:1059-1197) with every array resident in HBM.

    Per evaluation: V_emb = param . dV_dparam (dmk_dgemv2, one pass over dV), eigh of embH1 + V_emb (dmk_eigh_batched_real;
    a non-identity embedding overlap is folded in through X = S^-1/2), host occupations (mfd.assignocc), density,
    |drho|; the gradient adds ev [(C^T 2 drho C) o K] ev^T, its tril fold and the second pass over dV.  K is the
    divided-difference matrix of the occupations: the T = 0 branch (slater.py:1126-1141) and the finite-T branch
    (ftsystem.py:151-213) are the same expression with different K."""

    def __init__(self, ctx, rho, lattice, basis, vcor, beta, nelec, imp_idx, det_idx, fock_k, ovlp_k, mu0=None,
                 fix_mu=False, tol_deg=1e-3, remove_diag_grad=False, eigh="jacobi", shard=False, C_act=None, P_act=None,
                 operators=None, dV_table=None, norm=None):
        """`C_act` (spin, nidx, nact): the residual is projected on active orbitals, C^T drho C, before the norm (slater.py:1083-1088);
        `P_act`: FULL active-space projector (spin, nkpts, nlo, nlo) applied to the basis inside dV_dparam (slater.py:878-892).
        A twin of the fit hands over its own ingredients: `operators` = (embH1, ovlp_emb) as (spin, nb, nb) arrays in place of the
        folds of fock_k / ovlp_k, `dV_table` = the device table (nparam, spin, npair), `norm` = the divisor of |drho| (default
        sqrt(spin); the GSO fit divides by sqrt(2) with one block, routine/spinless.py:1259)."""
        from libdmet_preview_amd.routine import mfd
        self._mfd = mfd
        self.ctx, self.vcor = ctx, vcor
        if operators is not None:                            # the embedded operators say how many blocks of which size there are
            log.eassert(dV_table is not None or basis is not None, "EmbFitDevice: handed-over operators need the dV table or the basis")
            embH1_given = np.asarray(operators[0], dtype=np.float64)
            self.spin, self.nb = (1, embH1_given.shape[-1]) if embH1_given.ndim == 2 else (embH1_given.shape[0], embH1_given.shape[-1])
        else:
            basis = np.asarray(basis, dtype=np.float64)
            self.spin, self.nb = basis.shape[0], basis.shape[-1]
        spin, nb = self.spin, self.nb
        self.npair = nb * (nb + 1) // 2
        self.beta, self.nelec, self.mu0, self.fix_mu, self.tol_deg = beta, nelec, mu0, fix_mu, tol_deg
        self.remove_diag_grad = remove_diag_grad
        self.nparam = vcor.length()
        self.norm = sqrt(spin) if norm is None else float(norm)
        if operators is None:
            basis_k = lattice.R2k_basis(basis)
            embH1 = transform_h1(fock_k, basis_k)
            ovlp = transform_h1(ovlp_k, basis_k)
        else:
            basis_k = None
            embH1, ovlp = (np.asarray(x, dtype=np.float64).reshape(spin, nb, nb) for x in operators)
        tl = np.tril_indices(nb)
        self.d_H1 = ctx.to_device(np.asarray([h[tl] for h in embH1]))
        # generalised problem: X = S^-1/2 (symmetric), skipped for an orthonormal embedding basis
        self.d_X = None
        if max_abs(ovlp - np.eye(nb)) > 1e-13:
            self.d_X = ctx.empty((spin, nb, nb), np.float64)
            for s in range(spin):
                d_w = ctx.empty((1, nb), np.float64)
                d_V = ctx.empty((1, nb, nb), np.float64)
                d_S = ctx.to_device(ovlp[s])
                ctx.check(lib.dmk_eigh_batched_real(ctx.h, nb, 1, d_S.ptr, d_w.ptr, d_V.ptr))
                w = d_w.get()[0]
                log.eassert(w[0] > 0, "embedding overlap is not positive definite")
                d_sc = ctx.to_device(1.0 / np.sqrt(w))
                d_T = ctx.empty((nb, nb), np.float64)
                ctx.check(lib.dmk_ewise_mul(ctx.h, 1, nb, nb, d_V.ptr, d_sc.ptr, d_T.ptr))          # rows v_m / sqrt(w_m)
                ctx.check(lib.dmk_dgemm_batched(ctx.h, 1, 0, nb, nb, nb, 1, 1.0, d_V.ptr, nb, nb * nb, d_T.ptr, nb, nb * nb,
                                                0.0, self.d_X.offset(s * nb * nb, (nb, nb)).ptr, nb, nb * nb))
        # Rank-sharded table, OPT-IN (`shard=True`; the reference's FitVcorEmb is purely local and so is the default here: a
        # driver that fits on one rank and broadcasts the result must not find a collective inside).  With `shard=True` every
        # evaluation is a COLLECTIVE -- all ranks of the process group have to run the same fit.
        # Rank r holds the rows [p_lo, p_hi) of dV_dparam (1.68 GB / N at C5), contracts its slice in both
        # table passes and the small results are summed over ranks -- V_emb (spin x npair) after the column pass, the
        # gradient slices after the row pass.  Everything else (eigh of nemb x nemb, densities) is replicated and, being
        # deterministic on identical inputs, stays bit-identical across ranks.  The reference shards the gradient of its lattice
        # fit over ranks the same way (routine/mfd_mpi.py:117-162 get_dw_dparam: local slice, then mpi reduce).
        from libdmet_preview_amd.parallel import dist as _dist
        self._dist = _dist if (shard and _dist.is_initialized() and _dist.world_size() > 1) else None
        if self._dist is not None:
            cuts = np.linspace(0, self.nparam, self._dist.world_size() + 1).astype(np.int64)
            self.p_lo, self.p_hi = int(cuts[self._dist.rank()]), int(cuts[self._dist.rank() + 1])
        else:
            self.p_lo, self.p_hi = 0, self.nparam
        self.nloc = self.p_hi - self.p_lo
        if dV_table is not None:
            log.eassert(self._dist is None and tuple(dV_table.shape) == (self.nparam, spin, self.npair),
                        "EmbFitDevice: a handed-over dV table is (nparam, spin, npair) and not sharded")
            self.d_dV = dV_table
        elif P_act is not None and vcor.is_local():          # the non-local branch of get_dV_dparam does not read P_act (slater.py:893-902)
            self.d_dV = get_dV_dparam_dev(ctx, vcor, _projected_basis_rows(P_act, basis_k), thr=0.0, rows=(self.p_lo, self.p_hi))
        else:
            self.d_dV = get_dV_dparam_dev(ctx, vcor, basis, rows=(self.p_lo, self.p_hi), lattice=lattice)
        # fitted entries: the imp x imp block and the det diagonal of rho[fit_idx, fit_idx] (slater.py:1012-1017)
        self.fit_idx = list(imp_idx) + list(det_idx)
        nimp, nidx = len(imp_idx), len(self.fit_idx)
        self.nidx = nidx
        W = np.zeros((nidx, nidx))
        W[:nimp, :nimp] = 1.0
        W[range(nimp, nidx), range(nimp, nidx)] = 1.0
        target = np.zeros((spin, nidx, nidx))
        for s in range(spin):
            target[s][:nimp, :nimp] = rho[s][np.ix_(imp_idx, imp_idx)]
            target[s][range(nimp, nidx), range(nimp, nidx)] = rho[s][det_idx, det_idx]
        self.d_W = ctx.to_device(np.asarray([W] * spin))
        self.d_target = ctx.to_device(target)
        self.d_fit = ctx.to_device(np.asarray(self.fit_idx, dtype=np.int32))
        # work arrays
        e = lambda *shape: ctx.empty(shape, np.float64)
        self.d_param, self.d_vemb, self.d_H = e(max(self.nloc, 1)), e(spin, self.npair), e(spin, nb, nb)
        self.d_T, self.d_T2, self.d_w, self.d_Vp, self.d_Vt = e(spin, nb, nb), e(spin, nb, nb), e(spin, nb), e(spin, nb, nb), e(spin, nb, nb)
        self.d_occ, self.d_sc, self.d_rho = e(spin, nb), e(spin, nb, nb), e(spin, nb, nb)
        self.d_rfit, self.d_drho, self.d_ss = e(spin, nidx, nidx), e(spin, nidx, nidx), e(1)
        self.d_C, self.d_M1, self.d_K = e(spin, nb, nidx), e(spin, nb, nidx), e(spin, nb, nb)
        self.d_dw, self.d_grad = e(spin, self.npair), e(max(self.nloc, 1))
        # residual projected on active orbitals (C_act): two small products after the residual, two more in front of the gradient
        self.d_Cact = None
        if C_act is not None:
            C_act = np.ascontiguousarray(np.asarray(C_act, dtype=np.float64))
            if C_act.shape[:2] != (spin, nidx):
                raise ValueError("C_act of shape %s for %d spin blocks of %d fitted indices" % (C_act.shape, spin, nidx))
            self.nact = C_act.shape[-1]
            self.d_Cact = ctx.to_device(C_act)
            self.d_act, self.d_actT, self.d_zero = e(spin, self.nact, self.nact), e(spin, nidx, self.nact), ctx.zeros((spin, self.nact, self.nact), np.float64)
        if self._dist is not None:
            # lock-step by construction: the optimiser's decisions depend on f and the gradient only, which are deterministic
            # functions of (embH1, X, target, summed V_emb) -- so rank 0's copies of those inputs replace every rank's own (a
            # density that differs in the last bits between ranks could otherwise end a line search one evaluation apart and
            # leave a rank waiting in an all-reduce)
            for d in (self.d_H1, self.d_target) + ((self.d_X,) if self.d_X is not None else ()):
                self._dist.broadcast_dev(d, src=0)
        self._key, self._state = None, None
        self.nfev = self.ngev = 0
        # eigensolver: "jacobi" (multi-CU, warm started: latency) or "ql" (batched Householder + QL); DMK_FIT_EIGH overrides
        import os
        choice = os.environ.get("DMK_FIT_EIGH", eigh)
        self.use_jacobi = (choice == "jacobi") and nb <= 576 and spin * ((nb + 31) // 32) <= 256
        self._have_prev, self.sweeps = False, 0
        self._ray, self._ray_host, self._ray_serial = None, None, 0
        self.table_passes_saved = 0
        self.on_ray_hits = [0, 0]                      # table passes saved at a gradient's forward pass / at the start of a ray
        # fused native objective (dmk_fit_objective): T = 0, orthonormal embedding basis, warm eigensolver.  DMK_FIT_FUSED=0 keeps
        # the chain of separate calls (which stays the path of the first evaluation, of finite T and of every fallback)
        self._fused = None
        self.fused_calls = self.fused_fallbacks = 0
        self.settle_hist = {}                          # measurement pass that settled the refinement -> evaluations
        if (self.beta == np.inf and self.d_X is None and self.use_jacobi and os.environ.get("DMK_FIT_FUSED", "1") != "0"
                and self.d_Cact is None and ((nidx + 15) // 16) ** 2 * spin <= 2048):
            self._fused_setup()

    # -- fused native objective ----------------------------------------------------------------------
    def _fused_setup(self):
        from libdmet_preview_amd._lib import FitArgs, PinnedArray
        ctx, spin, nb = self.ctx, self.spin, self.nb
        ne = [self.nelec] if spin == 1 else list(self.nelec)
        ne = [float(self._mfd.check_nelec(x, None)[0]) for x in ne]
        self._f_nelec = (C.c_double * spin)(*ne)
        mu = [0.0] * spin
        if self.fix_mu:
            mu = [float(self.mu0)] * spin if np.ndim(self.mu0) == 0 else [float(x) for x in self.mu0]
        self._f_mu0 = (C.c_double * spin)(*mu)
        self._f_work = ctx.zeros((4096,), np.float64)
        self._f_slot = PinnedArray(ctx, (64,), np.float64)
        self._f_slot.a[:] = 0.0
        a = FitArgs()
        a.nb, a.spin, a.nidx, a.npass, a.has_mu0 = nb, spin, self.nidx, 3, 1 if self.fix_mu else 0
        a.tol_deg = float(self.tol_deg)
        a.H1, a.H, a.Vp, a.w, a.occ = self.d_H1.ptr, self.d_H.ptr, self.d_Vp.ptr, self.d_w.ptr, self.d_occ.ptr
        a.nelec, a.mu0 = C.cast(self._f_nelec, C.c_void_p), C.cast(self._f_mu0, C.c_void_p)
        a.fit_idx, a.W, a.target = self.d_fit.ptr, self.d_W.ptr, self.d_target.ptr
        a.drho, a.work, a.slot = self.d_drho.ptr, self._f_work.ptr, self._f_slot.ptr
        self._fused = a
        self._ray_norm = None
        self._f_out = (C.c_double(), C.c_int(), C.c_int())

    def _forward_fused(self, d_v0, d_v1, t):
        """The whole objective in one library call (csrc/fit.hip dmk_fit_objective); None when the enqueued refinement did not
        verify its basis (the caller then runs the chain of separate, synchronous calls)."""
        a = self._fused
        a.v0, a.v1, a.t = d_v0.ptr, (None if d_v1 is None else d_v1.ptr), float(t)
        a.ray_norm = None
        if d_v1 is not None and self._ray is not None and self._ray_norm is not None:
            for slot in (0, 1):                            # the bounds belong to the ray buffers they were computed from
                if self._ray[slot][0] is d_v0 and self._ray[slot][1] is d_v1:
                    a.ray_norm = self._ray_norm[slot].ptr
        f2, st, sp = self._f_out
        self.ctx.check(lib.dmk_fit_objective(self.ctx.h, C.byref(a), C.byref(f2), C.byref(st), C.byref(sp)))
        self.fused_calls += 1
        if st.value == 2:
            raise FloatingPointError("FitVcorEmb: non-finite embedding levels in the T = 0 forward pass")
        if st.value != 0:
            self.fused_fallbacks += 1
            a.npass = min(a.npass + 2, 8)
            return None
        self.settle_hist[sp.value] = self.settle_hist.get(sp.value, 0) + 1
        a.npass = min(max(sp.value + 2, 2), 8)           # settled at measurement pass sp (0-based): one spare pass next time
        return float(np.sqrt(f2.value))

    # -- forward pass ------------------------------------------------------------------------------
    def _gemm(self, opA, opB, M, N, K, A, lda, B, ldb, C, ldc, alpha=1.0):
        ctx, sp = self.ctx, self.spin
        ctx.check(lib.dmk_dgemm_batched(ctx.h, opA, opB, M, N, K, sp, alpha, A.ptr, lda, A.size // sp, B.ptr, ldb,
                                        B.size // sp, 0.0, C.ptr, ldc, C.size // sp))

    def _vemb_into(self, param, d_out):
        """d_out (spin, npair) = param . dV_dparam: one pass over the 1.7 GB (C5) table."""
        ctx, spin = self.ctx, self.spin
        param = np.ascontiguousarray(np.asarray(param, dtype=np.float64)[self.p_lo:self.p_hi])
        if self.nloc > 0:
            ctx.check(lib.dmk_memcpy_h2d(ctx.h, self.d_param.ptr, param.ctypes.data, param.nbytes))
            ctx.check(lib.dmk_dgemv2(ctx.h, self.nloc, spin * self.npair, self.d_dV.ptr, spin * self.npair, None,
                                     self.d_param.ptr, None, d_out.ptr))
        else:
            d_out.zero_()
        if self._dist is not None:
            self._dist.all_reduce_sum_dev(d_out)                  # spin x npair doubles (0.5 MB at C5)

    def _forward(self, param, ray=None):
        if ray is not None and param is None:
            key = ("ray", id(ray[0]), self._ray_serial, ray[2])     # a trial step of the current ray: no host vector is formed
        else:
            param = np.ascontiguousarray(param, dtype=np.float64)
            key = param.tobytes()
        if key == self._key:
            return self._state
        ctx, spin, nb, nidx = self.ctx, self.spin, self.nb, self.nidx
        if ray is None:
            # a point of the current line-search ray (the gradient at the accepted step): V_emb from the ray, no table pass
            t_on = self._on_ray(param)
            if t_on is not None:
                ray = self._ray[self._ray_cur] + (t_on,)
                key = ("ray", id(ray[0]), self._ray_serial, t_on)
                if key == self._key:                                    # the accepted step was the last one evaluated
                    return self._state
                self.table_passes_saved += 1
                self.on_ray_hits[0] += 1
            else:
                self._vemb_into(param, self.d_vemb)
        if self._fused is not None and self._have_prev:
            val = self._forward_fused(*((self.d_vemb, None, 0.0) if ray is None else ray))
            if val is not None:
                self._key, self._state = key, (None, None, None, val, self.d_Vp)
                return self._state
        if ray is not None:
            d_v0, d_v1, t = ray                                   # V_emb(x + t p) = V_emb(x) + t V_emb(p)
            ctx.check(lib.dmk_memcpy_d2d(ctx.h, self.d_vemb.ptr, d_v0.ptr, self.d_vemb.nbytes))
            ctx.check(lib.dmk_axpy_f64(ctx.h, spin * self.npair, float(t), d_v1.ptr, self.d_vemb.ptr))
        ctx.check(lib.dmk_sym_unpack(ctx.h, nb, spin, self.d_vemb.ptr, self.d_H1.ptr, self.d_H.ptr))
        d_A = self.d_H
        if self.d_X is not None:
            self._gemm(0, 0, nb, nb, nb, self.d_H, nb, self.d_X, nb, self.d_T, nb)          # H X
            self._gemm(0, 0, nb, nb, nb, self.d_X, nb, self.d_T, nb, self.d_T2, nb)         # X H X  (X symmetric)
            d_A = self.d_T2
        if self.use_jacobi:
            # low-latency multi-CU Jacobi, warm-started from the eigenvectors of the previous evaluation
            sw = C.c_int()
            ctx.check(lib.dmk_eigh_jacobi_real(ctx.h, nb, spin, d_A.ptr, self.d_Vp.ptr if self._have_prev else None,
                                               self.d_w.ptr, self.d_Vp.ptr, C.byref(sw)))
            self._have_prev = True
            self.sweeps += sw.value
        else:
            ctx.check(lib.dmk_eigh_batched_real(ctx.h, nb, spin, d_A.ptr, self.d_w.ptr, self.d_Vp.ptr))
        if self.d_X is not None:
            self._gemm(0, 0, nb, nb, nb, self.d_Vp, nb, self.d_X, nb, self.d_Vt, nb)        # rows: (X v_m)^T
            d_Vt = self.d_Vt
        else:
            d_Vt = self.d_Vp
        if self.beta == np.inf:
            # T = 0: occupations straight from the device eigenvalues, one particle-number sector per spin (the frontier
            # mid-point the reference passes as mu0 is what dmk_assign_occ picks on its own); ew / occ stay in HBM and are
            # only fetched when the gradient asks for them
            ne = [self.nelec] if spin == 1 else list(self.nelec)
            for s in range(spin):
                guess = None if not self.fix_mu else (self.mu0 if np.ndim(self.mu0) == 0 else self.mu0[s])
                # the eigensolver returns each spin's levels ascending; nothing is read back (mu is not needed at T = 0 and the
                # eigensolver has already rejected non-finite input)
                self._mfd.assignocc_dev(ctx, self.d_w.offset(s * nb, (nb,)), ne[s], self.beta, mu0=guess, thr_deg=self.tol_deg,
                                        d_occ=self.d_occ.offset(s * nb, (nb,)), ascending=True, sync=False)
            mu = None
            ew = occ = None
        else:
            ew = self.d_w.get()
            if not self.fix_mu:
                ne = self.nelec
                mu = (0.5 * (ew[0][ne - 1] + ew[0][ne]) if spin == 1 else
                      [0.5 * (ew[0][ne[0] - 1] + ew[0][ne[0]]), 0.5 * (ew[1][ne[1] - 1] + ew[1][ne[1]])])
            else:
                mu = self.mu0
            occ, mu, _ = self._mfd.assignocc(ew, self.nelec, self.beta, mu, fix_mu=self.fix_mu, thr_deg=self.tol_deg)
            occ = np.ascontiguousarray(occ, dtype=np.float64)
            ctx.check(lib.dmk_memcpy_h2d(ctx.h, self.d_occ.ptr, occ.ctypes.data, occ.nbytes))
        ctx.check(lib.dmk_ewise_mul(ctx.h, 1, spin * nb, nb, d_Vt.ptr, self.d_occ.ptr, self.d_sc.ptr))
        self._gemm(1, 0, nb, nb, nb, d_Vt, nb, self.d_sc, nb, self.d_rho, nb)               # ev occ ev^T
        for s in range(spin):
            ctx.check(lib.dmk_gather2d_f64(ctx.h, nidx, nidx, self.d_fit.ptr, self.d_fit.ptr,
                                           self.d_rho.offset(s * nb * nb, (nb, nb)).ptr, nb,
                                           self.d_rfit.offset(s * nidx * nidx, (nidx, nidx)).ptr))
        ctx.check(lib.dmk_ewise_mul(ctx.h, 0, spin * nidx, nidx, self.d_rfit.ptr, self.d_W.ptr, self.d_rfit.ptr))
        ctx.check(lib.dmk_sub_sumsq(ctx.h, spin * nidx * nidx, self.d_rfit.ptr, self.d_target.ptr, self.d_drho.ptr,
                                    self.d_ss.ptr))
        if self.d_Cact is not None:
            # act = C^T drho C is what the norm is taken of; the gradient sees C act C^T (slater.py:1083-1088, 1112-1124)
            na = self.nact
            self._gemm(0, 0, nidx, na, nidx, self.d_drho, nidx, self.d_Cact, na, self.d_actT, na)      # drho C
            self._gemm(1, 0, na, na, nidx, self.d_Cact, na, self.d_actT, na, self.d_act, na)           # C^T (drho C)
            ctx.check(lib.dmk_sub_sumsq(ctx.h, spin * na * na, self.d_act.ptr, self.d_zero.ptr, None, self.d_ss.ptr))
            self._gemm(0, 0, nidx, na, na, self.d_Cact, na, self.d_act, na, self.d_actT, na)           # C act
            self._gemm(0, 1, nidx, nidx, na, self.d_actT, na, self.d_Cact, na, self.d_drho, nidx)      # (C act) C^T
        val = float(np.sqrt(self.d_ss.get()[0]))
        self._key, self._state = key, (ew, occ, mu, val, d_Vt)
        return self._state

    def errfunc(self, param):
        self.nfev += 1
        return self._forward(param)[3] / self.norm

    def _on_ray(self, param):
        """t with param == x + t p BITWISE for the current line-search ray and a step t that was evaluated on it (the optimiser
        forms its next point as xk + alpha_k pk from the arrays it handed to errfunc_ray and a step the search returned), else
        None.  One vector operation: the candidate is the evaluated step closest to the quotient of the largest component."""
        r = self._ray_host
        if r is None or not r["ts"] or param.shape != r["x"].shape:
            return None
        i = r["imax"]
        if r["p"][i] == 0.0:
            return None
        guess = (param[i] - r["x"][i]) / r["p"][i]
        t = min(r["ts"], key=lambda u: abs(u - guess))
        return t if np.array_equal(r["x"] + t * r["p"], param) else None

    def errfunc_ray(self, x, p):
        """phi(t) = errfunc(x + t p) for a line search: the embedding potential is LINEAR in the parameters, so the two
        table passes V_emb(x), V_emb(p) are made once and every trial step is an axpy of spin * npair numbers (the pass over
        dV_dparam was half of an objective evaluation at C5).  Round 5: when x itself lies on the PREVIOUS ray (x = x' + t p':
        the CG / BFGS drivers step exactly that way), V_emb(x) = V_emb(x') + t V_emb(p') is an axpy too and only V_emb(p) costs
        a table pass; every 16th ray takes the real pass so that the recursion cannot drift."""
        x, p = np.array(x, dtype=np.float64), np.array(p, dtype=np.float64)
        if self._ray is None:
            e = lambda: self.ctx.empty((self.spin, self.npair), np.float64)
            self._ray = [(e(), e()), (e(), e())]
            self._ray_cur, self._ray_age = 0, 0
        t_prev = self._on_ray(x) if self._ray_age < 16 else None
        old_v0, old_v1 = self._ray[self._ray_cur]
        self._ray_cur ^= 1
        d_v0, d_v1 = self._ray[self._ray_cur]
        if t_prev is not None:
            ctx = self.ctx
            ctx.check(lib.dmk_memcpy_d2d(ctx.h, d_v0.ptr, old_v0.ptr, d_v0.nbytes))
            ctx.check(lib.dmk_axpy_f64(ctx.h, self.spin * self.npair, float(t_prev), old_v1.ptr, d_v0.ptr))
            self._ray_age += 1
            self.table_passes_saved += 1
            self.on_ray_hits[1] += 1
        else:
            self._vemb_into(x, d_v0)
            self._ray_age = 0
        self._vemb_into(p, d_v1)
        if self._fused is not None:
            # the refinement's bound on |H| along this ray from TWO bounds computed once: |H0 + t V1| <= |H0| + |t| |V1|
            # (dmk_sym_norm_bound of the unpacked matrices; it measured the bound from H in a launch of its own per trial step)
            ctx = self.ctx
            if self._ray_norm is None:
                self._ray_norm = [ctx.empty((2, self.spin), np.float64), ctx.empty((2, self.spin), np.float64)]
            d_rn = self._ray_norm[self._ray_cur]
            ctx.check(lib.dmk_sym_unpack(ctx.h, self.nb, self.spin, d_v0.ptr, self.d_H1.ptr, self.d_H.ptr))
            ctx.check(lib.dmk_sym_norm_bound(ctx.h, self.nb, self.spin, self.d_H.ptr, d_rn.ptr))
            ctx.check(lib.dmk_sym_unpack(ctx.h, self.nb, self.spin, d_v1.ptr, None, self.d_H.ptr))
            ctx.check(lib.dmk_sym_norm_bound(ctx.h, self.nb, self.spin, self.d_H.ptr, d_rn.offset(self.spin, (self.spin,)).ptr))
        self._ray_host = {"x": x, "p": p, "ts": [], "imax": int(np.argmax(np.abs(p))) if p.size else 0}
        self._ray_serial += 1
        ts = self._ray_host["ts"]
        inv = 1.0 / self.norm

        def phi(t):
            t = float(np.asarray(t).ravel()[0])                   # the Nelder-Mead fallback passes a 1-vector
            self.nfev += 1
            ts.append(t)
            return self._forward(None, ray=(d_v0, d_v1, t))[3] * inv
        return phi

    # -- gradient ----------------------------------------------------------------------------------
    def _kmat_dev(self, occ, mu):
        """Divided differences of the occupations on the device (dmk_fit_kmat); returns f (1 - f) at finite T."""
        ctx, spin, nb = self.ctx, self.spin, self.nb
        if self.beta == np.inf:
            nocc = int(np.round(np.sum(occ) / spin))                      # slater.py:1126
            ctx.check(lib.dmk_fit_kmat(ctx.h, nb, spin, self.d_w.ptr, None, -1.0, nocc, self.d_K.ptr))
            return None
        f = np.ascontiguousarray(ftsystem.fermi_smearing_occ(mu, self._ew, self.beta), dtype=np.float64)
        ctx.check(lib.dmk_memcpy_h2d(ctx.h, self.d_occ.ptr, f.ctypes.data, f.nbytes))
        ctx.check(lib.dmk_fit_kmat(ctx.h, nb, spin, self.d_w.ptr, self.d_occ.ptr, float(self.beta), 0, self.d_K.ptr))
        return f * (1.0 - f)

    def gradfunc(self, param):
        self.ngev += 1
        ctx, spin, nb, nidx = self.ctx, self.spin, self.nb, self.nidx
        ew, occ, mu, val, d_Vt = self._forward(param)
        if ew is None:                                                     # T = 0 forward pass: levels and occupations are in HBM
            ew, occ = self.d_w.get(), self.d_occ.get()
            # the forward pass enqueued dmk_assign_occ without reading its status back (flags bit 2: levels taken as sorted);
            # here, where the levels are on the host anyway, the assumptions it ran on are checked once per gradient
            lv = ew.reshape(spin, nb)
            if not np.all(np.isfinite(lv)):
                raise FloatingPointError("FitVcorEmb: non-finite embedding levels in the T = 0 forward pass")
            if np.any(np.diff(lv, axis=1) < 0.0):
                raise AssertionError("FitVcorEmb: the eigensolver returned unsorted levels; the T = 0 occupations assumed ascending order")
            ne = [self.nelec] if spin == 1 else list(self.nelec)
            for s in range(spin):
                if 0 < ne[s] < nb and lv[s, ne[s]] - lv[s, ne[s] - 1] < self.tol_deg and not getattr(self, "_warned_deg", False):
                    self._warned_deg = True                                # once per fit, like a summary of the reference's per-call warning
                    log.warn("degenerate HOMO-LUMO in the embedding fit (spin %d): gap %g < %g", s,
                             lv[s, ne[s]] - lv[s, ne[s] - 1], self.tol_deg)
        self._ew = ew
        ff = self._kmat_dev(occ, mu)
        for s in range(spin):                                              # C = ev[fit_idx]^T : (orbital m, fitted index a)
            ctx.check(lib.dmk_gather2d_f64(ctx.h, nb, nidx, None, self.d_fit.ptr, d_Vt.offset(s * nb * nb, (nb, nb)).ptr, nb,
                                           self.d_C.offset(s * nb * nidx, (nb, nidx)).ptr))
        self._gemm(0, 0, nb, nidx, nidx, self.d_C, nidx, self.d_drho, nidx, self.d_M1, nidx, alpha=2.0)   # C (2 drho)
        self._gemm(0, 1, nb, nb, nidx, self.d_M1, nidx, self.d_C, nidx, self.d_T, nb)                      # . C^T
        ctx.check(lib.dmk_ewise_mul(ctx.h, 0, spin * nb, nb, self.d_T.ptr, self.d_K.ptr, self.d_T.ptr))
        self._gemm(0, 0, nb, nb, nb, self.d_T, nb, d_Vt, nb, self.d_T2, nb)                                # tmp ev^T
        self._gemm(1, 0, nb, nb, nb, d_Vt, nb, self.d_T2, nb, self.d_sc, nb)                               # ev tmp ev^T
        if ff is not None and not self.fix_mu:
            # response of the chemical potential (ftsystem.py:189-204): dw_dv += drho_dmu (dw_dmu / sum f(1-f)), per spin
            ffd = np.ascontiguousarray(ff)
            ctx.check(lib.dmk_memcpy_h2d(ctx.h, self.d_occ.ptr, ffd.ctypes.data, ffd.nbytes))
            ctx.check(lib.dmk_ewise_mul(ctx.h, 1, spin * nb, nb, d_Vt.ptr, self.d_occ.ptr, self.d_T.ptr))
            self._gemm(1, 0, nb, nb, nb, d_Vt, nb, self.d_T, nb, self.d_T2, nb)                            # drho_dmu
            for s in range(spin):
                fsum = float(np.sum(ff[s]))
                if abs(fsum) <= ftsystem.ZERO_TOL:
                    continue
                d_dm = self.d_T2.offset(s * nb * nb, (nb, nb))
                d_sub = self.d_rfit.offset(s * nidx * nidx, (nidx, nidx))                                   # scratch: drho_dmu[fit, fit]
                ctx.check(lib.dmk_gather2d_f64(ctx.h, nidx, nidx, self.d_fit.ptr, self.d_fit.ptr, d_dm.ptr, nb, d_sub.ptr))
                ctx.check(lib.dmk_dgemv2(ctx.h, 1, nidx * nidx, self.d_drho.offset(s * nidx * nidx, (nidx * nidx,)).ptr,
                                         nidx * nidx, d_sub.ptr, None, self.d_ss.ptr, None))                 # <drho, drho_dmu[fit,fit]>
                dw_dmu = float(self.d_ss.get()[0]) * 2.0 * self.beta
                ctx.check(lib.dmk_axpy_f64(ctx.h, nb * nb, dw_dmu / fsum, d_dm.ptr, self.d_sc.offset(s * nb * nb, (nb, nb)).ptr))
        ctx.check(lib.dmk_sym_fold(ctx.h, nb, spin, self.d_sc.ptr, self.d_dw.ptr))
        if self.nloc > 0:
            ctx.check(lib.dmk_dgemv2(ctx.h, self.nloc, spin * self.npair, self.d_dV.ptr, spin * self.npair, self.d_dw.ptr,
                                     None, self.d_grad.ptr, None))
        if self._dist is not None:
            full = np.zeros(self.nparam)                           # every rank fills its slice; the sum is the whole gradient
            if self.nloc > 0:
                full[self.p_lo:self.p_hi] = self.d_grad.get()[:self.nloc]
            res = self._dist.all_reduce_sum_numpy(full) / (2.0 * val * self.norm)
        else:
            res = self.d_grad.get()[:self.nloc] / (2.0 * val * self.norm)
        if self.remove_diag_grad:
            for s in range(spin):
                d = self.vcor.diag_indices()[s]
                res[d] -= np.average(res[d])
        return res

    def drho_dparam(self, param, chunk=256):
        """Response of the tril-packed embedding density to every parameter at finite temperature, (spin, nparam, npair)
        (slater.py:1227-1261 over ftsystem.get_rho_grad, ftsystem.py:147-221).  The reference forms the npair x npair response
        matrix d rho / d v and contracts it with dV_dparam; contracted with a SYMMETRIC V_p that is the directional derivative
            D rho[V_p] = ev [(ev^T V_p ev) o K] ev^T  +  (sum_i ff_i (ev^T V_p ev)_ii / sum ff) beta ev diag(ff) ev^T     (fix_mu: first term only)
        with K the divided differences of the occupations (dmk_fit_kmat) and ff = f (1 - f): four nb^3 products per parameter,
        batched over chunks of parameters (dmk_dgemm_batched with the eigenvectors as the shared operand)."""
        if not self.beta < np.inf:
            raise AssertionError("drho_dparam needs a finite temperature (slater.py:1231)")
        if self._dist is not None:
            raise NotImplementedError("drho_dparam with a rank-sharded table")
        ctx, spin, nb, npair = self.ctx, self.spin, self.nb, self.npair
        ew, occ, mu, val, d_Vt = self._forward(param)
        self._ew = ew
        ff = self._kmat_dev(occ, mu)                                       # K in self.d_K, f in self.d_occ
        nparam = self.nparam
        out = np.empty((spin, nparam, npair))
        chunk = max(1, min(int(chunk), nparam))
        e = lambda *shape: ctx.empty(shape, np.float64)
        d_V, d_T, d_M, d_Kt, d_tr = e(chunk, nb, nb), e(chunk, nb, nb), e(chunk, nb, nb), e(chunk, nb, nb), e(chunk, npair)
        d_c, d_diag, d_dm, d_sc = e(chunk), ctx.zeros((nb * nb,), np.float64), e(nb, nb), e(nb, nb)
        tl = np.tril_indices(nb)
        off = tl[0] != tl[1]
        for s in range(spin):
            d_ev_t = d_Vt.offset(s * nb * nb, (nb, nb))                    # rows = eigenvectors
            d_K = self.d_K.offset(s * nb * nb, (nb, nb))
            for c in range(chunk):                                         # K tiled over the chunk: one Hadamard per chunk
                ctx.check(lib.dmk_memcpy_d2d(ctx.h, d_Kt.offset(c * nb * nb, (nb, nb)).ptr, d_K.ptr, nb * nb * 8))
            fsum = 0.0
            if ff is not None and not self.fix_mu:
                fsum = float(np.sum(ff[s]))
                if abs(fsum) > ftsystem.ZERO_TOL:
                    dg = np.zeros(nb * nb)
                    dg[::nb + 1] = ff[s]
                    ctx.check(lib.dmk_memcpy_h2d(ctx.h, d_diag.ptr, dg.ctypes.data, dg.nbytes))
                    ffd = np.ascontiguousarray(ff[s])
                    d_ff = ctx.to_device(ffd)
                    ctx.check(lib.dmk_ewise_mul(ctx.h, 1, nb, nb, d_ev_t.ptr, d_ff.ptr, d_sc.ptr))                 # rows v_m ff_m
                    ctx.check(lib.dmk_dgemm_batched(ctx.h, 1, 0, nb, nb, nb, 1, float(self.beta), d_ev_t.ptr, nb, 0, d_sc.ptr, nb, 0,
                                                    0.0, d_dm.ptr, nb, 0))                                         # drho_dmu
            for p0 in range(0, nparam, chunk):
                n = min(chunk, nparam - p0)
                for c in range(n):                                         # V_p of this spin, tril -> full symmetric
                    ctx.check(lib.dmk_sym_unpack(ctx.h, nb, 1, self.d_dV.offset(((p0 + c) * spin + s) * npair, (npair,)).ptr, None,
                                                 d_V.offset(c * nb * nb, (nb, nb)).ptr))
                bg = lambda opA, opB, A, sA, B, sB, Cm, beta=0.0: ctx.check(lib.dmk_dgemm_batched(
                    ctx.h, opA, opB, nb, nb, nb, n, 1.0, A.ptr, nb, sA, B.ptr, nb, sB, beta, Cm.ptr, nb, nb * nb))
                bg(0, 1, d_V, nb * nb, d_ev_t, 0, d_T)                     # V ev            (ev = Vt^T)
                bg(0, 0, d_ev_t, 0, d_T, nb * nb, d_M)                     # ev^T V ev
                if fsum and abs(fsum) > ftsystem.ZERO_TOL:
                    ctx.check(lib.dmk_dgemv2(ctx.h, n, nb * nb, d_M.ptr, nb * nb, d_diag.ptr, None, d_c.ptr, None))   # sum_i ff_i M_ii
                ctx.check(lib.dmk_ewise_mul(ctx.h, 0, n * nb, nb, d_M.ptr, d_Kt.ptr, d_M.ptr))
                bg(0, 0, d_M, nb * nb, d_ev_t, 0, d_T)                     # (M o K) ev^T
                bg(1, 0, d_ev_t, 0, d_T, nb * nb, d_V)                     # ev (M o K) ev^T
                if fsum and abs(fsum) > ftsystem.ZERO_TOL:
                    ctx.check(lib.dmk_dgemm_batched(ctx.h, 0, 0, n, nb * nb, 1, 1, 1.0 / fsum, d_c.ptr, 1, 0, d_dm.ptr, nb * nb, 0,
                                                    1.0, d_V.ptr, nb * nb, 0))                                     # + c_p drho_dmu / fsum
                ctx.check(lib.dmk_sym_fold(ctx.h, nb, n, d_V.ptr, d_tr.ptr))
                blk = d_tr.get()[:n]
                blk[:, off] *= 0.5                                         # the fold doubled the off-diagonal pairs of a symmetric matrix
                out[s, p0:p0 + n] = blk
        return out


def addDiag(v, val, idx_range=None):
    """Add `val` (a number, or one per spin block) to the diagonal of the normal blocks of a potential on `idx_range` and re-project
    it on its parameters (slater.py:757-778; the pairing block of a BCS / GSO potential is left alone)."""
    rep = np.array(v.get(), copy=True)
    nblk = rep.shape[0]
    shifts = list(val) if isinstance(val, Iterable) else [val] * nblk
    if idx_range is None:
        idx_range = getattr(v, "idx_range", range(rep.shape[-1]))
    idx = list(idx_range)
    for s in range(min(nblk, 2)):
        rep[s, idx, idx] += shifts[s]
    v.assign(rep)
    return v


def vcor_diag_average(v, idx_range=None):
    """Mean diagonal element of every block of a potential on `idx_range` (slater.py:780-795)."""
    rep = np.asarray(v.get())
    if idx_range is None:
        idx_range = getattr(v, "idx_range", range(rep.shape[-1]))
    idx = list(idx_range)
    return np.average(rep[:, idx, idx], axis=1)


def make_vcor_trace_unchanged(v_new, v_old, idx_range=None):
    """Shift the diagonal of `v_new` so that its trace on `idx_range` equals that of `v_old`, block by block (slater.py:797-818)."""
    new, old = np.asarray(v_new.get()), np.asarray(v_old.get())
    if idx_range is None:
        idx_range = getattr(v_new, "idx_range", range(new.shape[-1]))
    idx = list(idx_range)
    drift = np.average((new - old)[:, idx, idx], axis=1)
    return addDiag(v_new, -drift, idx_range=idx_range)


def test_grad(vcor, errfunc, gradfunc, dx=1e-5):
    """Analytic gradient against central differences of the objective, logged (slater.py:820-849); returns the two vectors."""
    param0 = vcor if isinstance(vcor, np.ndarray) else vcor.param.copy()
    grad_ana = gradfunc(param0)
    grad_num = np.zeros_like(param0)
    for i in range(len(grad_num)):
        lo, hi = param0.copy(), param0.copy()
        lo[i] -= dx
        hi[i] += dx
        grad_num[i] = (errfunc(hi) - errfunc(lo)) / dx / 2
    log.info("Test gradients in fitting, finite difference dx = %s", dx)
    log.info("Analytical gradient:\n%s", grad_ana)
    log.info("Numerical gradient:\n%s", grad_num)
    log.info("grad diff (abs): %s", max_abs(grad_ana - grad_num))
    return grad_ana, grad_num


test_grad.__test__ = False          # (not a pytest case: the reference's name)


def FitVcorEmb(rho, lattice, basis, vcor, beta, MaxIter=300, imp_fit=False, imp_idx=None, det=False, det_idx=None,
               CG_check=False, BFGS=False, diff_criterion=None, **kwargs):
    """
    Fit the correlation potential in the embedding space (slater.py:909-1329): minimise
    |rho_emb[vcor] - rho|_F / sqrt(spin) over the vcor parameters with an analytic gradient.

    Kwargs: ytol, gtol, dx_tol, method, mu0, fix_mu, num_grad, remove_diag_grad, nelec, tol_deg, vcor_mat, idem_fit (fit the
    idempotent part of rho, get_rdm1_idem), P_act (active-space projector columns (spin, nkpts, nlo, nact) for the potential),
    C_act (active orbitals (spin, nidx, nact) the residual is projected on), return_drho_dparam / use_drho_dparam (finite T: the
    response of the embedding density to the parameters; `return_` hands it back instead of fitting), test_grad.
    `shard=True` (default False: local, like the reference) shards the dV_dparam table over the ranks of an initialised
    torch.distributed group and makes the call COLLECTIVE: every rank must call it; rank 0's inputs (embedded Hamiltonian,
    target density, starting parameters) are broadcast so that all ranks take identical optimiser decisions.
    Returns (vcor, err_begin, err_end).
    """
    idem_fit, P_act, C_act = kwargs.get("idem_fit", False), kwargs.get("P_act", None), kwargs.get("C_act", None)
    basis = np.asarray(basis)
    param_begin = vcor.param.copy()
    spin, nbasis = basis.shape[0], basis.shape[-1]
    nelec = kwargs.get("nelec", None)
    if nelec is None:
        nelec = lattice.ncore + lattice.nval if spin == 1 else [lattice.ncore + lattice.nval] * 2
    if idem_fit:
        log.info("idempotent fitting? %s", idem_fit)
        rho = get_rdm1_idem(rho, nelec, beta)                      # slater.py:975-978
    fock_k = lattice.getH1(kspace=True) if lattice.use_hcore_as_emb_ham else lattice.getFock(kspace=True)
    fock_k = np.array(fock_k, copy=True)
    if fock_k.ndim == 3:
        fock_k = fock_k[np.newaxis]
    vcor_mat = kwargs.get("vcor_mat", None)
    if vcor_mat is not None:
        for s in range(spin):
            fock_k[s] += vcor_mat[s]
    if P_act is not None:
        log.info("active space fitting? True.")
        ovlp_lo_k = getattr(lattice, "ovlp_lo_k", None)
        if ovlp_lo_k is None:                                           # (an orthonormal LO basis that never installed an overlap)
            ovlp_lo_k = lattice.get_ovlp(kspace=True)
        ovlp_lo_k = np.asarray(ovlp_lo_k)
        if ovlp_lo_k.ndim == 3 and len(P_act) > 1:                      # one overlap for both spin channels
            ovlp_lo_k = np.asarray([ovlp_lo_k] * len(P_act))
        P_act = get_active_projector_full(P_act, ovlp_lo_k)             # slater.py:1021-1023
    # fitted index sets (slater.py:985-1005)
    if imp_fit:
        imp_idx, det_idx = list(range(lattice.nimp)), []
    elif det:
        imp_idx, det_idx = [], list(range(lattice.nimp))
    elif imp_idx is None:
        if det_idx is None:
            imp_idx, det_idx = list(range(nbasis)), []
        else:
            imp_idx = []
    elif det_idx is None:
        det_idx = []
    imp_idx, det_idx = list(imp_idx), list(det_idx)
    log.info("impurity fitting? %s", imp_fit)
    log.info("det (diagonal fitting)? %s", det)
    if len(np.unique(imp_idx + det_idx)) != len(imp_idx + det_idx):
        log.warn("fit_idx has repeated indices: %s", imp_idx + det_idx)

    ctx = get_ctx()
    fit = EmbFitDevice(ctx, np.asarray(rho), lattice, basis, vcor, beta, nelec, imp_idx, det_idx, fock_k,
                       lattice.get_ovlp(kspace=True), mu0=kwargs.get("mu0", None), fix_mu=kwargs.get("fix_mu", False),
                       tol_deg=kwargs.get("tol_deg", 1e-3), remove_diag_grad=kwargs.get("remove_diag_grad", False),
                       eigh=kwargs.get("eigh", "jacobi"), shard=bool(kwargs.pop("shard", False)), C_act=C_act, P_act=P_act)
    return drive_emb_fit(fit, vcor, param_begin, beta, MaxIter, CG_check, BFGS, diff_criterion, kwargs, FitVcorEmb)


def drive_emb_fit(fit, vcor, param_begin, beta, MaxIter, CG_check, BFGS, diff_criterion, kwargs, owner, grad_check_steps=(1e-4, 1e-6)):
    """Everything of FitVcorEmb after the objective exists (slater.py:1199-1329; shared with the GSO twin, spinless.py:1347-1430):
    the optional gradient test and density response, the minimiser on the device objective, the SciPy cross-check.  `owner` is the
    public function whose `last_fit` attribute keeps the device state of the most recent fit."""
    if fit._dist is not None:
        vcor.update(fit._dist.broadcast_numpy(np.asarray(vcor.param, dtype=np.float64), src=0))
    errfunc, gradfunc = fit.errfunc, fit.gradfunc
    err_begin = errfunc(vcor.param)
    if beta == np.inf:
        log.info("Using analytic gradient for 0 T")
    else:
        log.info("Using analytic gradient for finite T, beta = %s", beta)
    if kwargs.get("test_grad", False):
        # analytic against central-difference gradients at a random point, logged (slater.py:820-849, 1215-1225)
        param_rand = kwargs.get("param_rand", None)
        if param_rand is None:
            np.random.seed(10086)
            param_rand = (np.random.random(vcor.param.shape) - 0.5) * 0.1
        for dx in grad_check_steps:
            test_grad(param_rand.copy(), errfunc, gradfunc, dx=dx)
    if kwargs.get("use_drho_dparam", False) or kwargs.get("return_drho_dparam", False):
        log.info("compute drho_dparam")
        drho_dparam = fit.drho_dparam(vcor.param)
        log.info("norm: %s", np.linalg.norm(drho_dparam, axis=1))
        if kwargs.get("return_drho_dparam", False):
            owner.last_fit = fit
            return drho_dparam
    if kwargs.get("num_grad", False):
        log.warn("You are using numerical gradient...")
        gradfunc = None
    if kwargs.get("ray_objective", True):
        kwargs = dict(kwargs, ray_fn=fit.errfunc_ray)
    param, err_end, pattern, gnorm_res = minimize(errfunc, vcor.param, MaxIter, gradfunc, **kwargs)
    vcor.update(param)
    log.info("Minimizer converge pattern: %d ", pattern)
    log.info("Current function value: %15.8f", err_end)
    log.info("Norm of gradients: %s", gnorm_res)
    log.info("Norm diff of x: %15.8f", max_abs(param - param_begin))

    if CG_check and (pattern == 0 or gnorm_res > 1.0e-4):
        # cross-check with SciPy's own CG / BFGS driving the same device objective (slater.py:1283-1322)
        from scipy import optimize as opt
        param_new = param.copy()
        gtol = min(max(5.0e-5, gnorm_res * 0.1), 1.0e-2)
        method = 'BFGS' if BFGS else 'CG'
        res = opt.minimize(errfunc, param_new, method=method, jac=gradfunc,
                           options={'maxiter': min(len(param_new) * 10, MaxIter), 'disp': False, 'gtol': gtol})
        gnorm_new = max_abs(res.jac)
        diff_old = max_abs(res.x - param_new)
        if diff_criterion is None:
            diff_criterion = 2.0 if pattern == 0 else 1.0
        if (gnorm_new < gnorm_res * 0.9) and (res.fun < err_end) and (diff_old < diff_criterion):
            log.info("New result used")
            vcor.update(res.x)
            err_end = res.fun
        else:
            log.info("Old result used")
            vcor.update(param_new)
    owner.last_fit = fit               # evaluation counters / device state of the most recent fit (bench, tests)
    return vcor, err_begin, err_end


class FullFitDevice(object):
    """errfunc of FitVcorFull (slater.py:1448-1478): the whole lattice is re-diagonalised for every parameter vector
    (dmk_eigh_batched over all k and spins with the trial vcor as the shared shift, Fock_k resident in HBM),
    occupations on the host, density on the device and either its fold into the embedding space (imp + bath fit)
    or its cell-0 block (impurity / diagonal fit)."""

    def __init__(self, ctx, rho, lattice, basis, vcor, beta, nelec, imp_idx, det_idx, imp_bath_fit, fix_mu=False,
                 fock_k=None, shift_of=None, dV=None, norm=None, mask=None):
        """A twin of the fit hands over its own ingredients (the GSO lattice stage, routine/spinless.py:1464-1769): `fock_k`
        (spin, nk, n, n) in place of lattice.getFock, `shift_of(vcor)` -> the real (spin, n, n) matrix the trial potential adds to
        every k, `dV` the tril-packed parameter gradient (nparam, spin, npair), `norm` the divisor of |drho| (default sqrt(spin)),
        `mask` (nidx, nidx) zeroing entries of the fitted block that are not to be fitted."""
        from libdmet_preview_amd.routine import mfd
        from libdmet_preview_amd.system import fourier
        from libdmet_preview_amd.basis_transform.make_basis import bgemm_dev
        self._mfd, self._fourier, self._bgemm = mfd, fourier, bgemm_dev
        self.ctx, self.vcor, self.lattice = ctx, vcor, lattice
        basis = np.asarray(basis, dtype=np.float64)
        spin, nk, n, nb = basis.shape
        self.spin, self.nk, self.n, self.nb = spin, nk, n, nb
        self.beta, self.nelec, self.fix_mu, self.imp_bath_fit = beta, nelec, fix_mu, imp_bath_fit
        Fock = np.asarray(lattice.getFock(kspace=True) if fock_k is None else fock_k)
        if Fock.ndim == 3:
            Fock = Fock[np.newaxis]
        if Fock.shape[0] < spin:
            Fock = np.asarray((Fock[0],) * spin)
        self.norm = sqrt(spin) if norm is None else float(norm)
        self._shift_of = shift_of if shift_of is not None else (lambda v: np.asarray(v.get(0, True))[:spin].real)
        self.extra_shift, self.last_dens = None, None       # a second k-independent shift a caller may vary (a chemical potential searched
                                                            # inside every evaluation, spinless.FitVcorFull_mu); the cell-0 density of the last evaluation
        self.kpts = bool(getattr(vcor, "is_vcor_kpts", False))
        if self.kpts:
            self.F_host = np.array(Fock[:spin], dtype=np.complex128)       # the potential differs from k to k: added before the upload
        else:
            self.d_F = ctx.to_device(Fock[:spin].reshape(spin * nk, n, n), np.complex128)
        if imp_bath_fit:
            self.d_bk = fourier.fold_R2k_dev(ctx.to_device(basis.reshape(spin, nk, n * nb)), lattice.kmesh, spin, n * nb)
        self.fit_idx = list(imp_idx) + list(det_idx)
        nimp, nidx = len(imp_idx), len(self.fit_idx)
        self.nidx = nidx
        W = np.zeros((nidx, nidx))
        W[:nimp, :nimp] = 1.0
        W[range(nimp, nidx), range(nimp, nidx)] = 1.0
        if mask is not None:
            W = W * np.asarray(mask, dtype=np.float64)
        target = np.zeros((spin, nidx, nidx))
        for s in range(spin):
            target[s][:nimp, :nimp] = rho[s][np.ix_(imp_idx, imp_idx)]
            target[s][range(nimp, nidx), range(nimp, nidx)] = rho[s][det_idx, det_idx]
            target[s] *= W if mask is not None else 1.0
        self.d_W = ctx.to_device(np.asarray([W] * spin))
        self.d_target = ctx.to_device(target)
        self.d_fit = ctx.to_device(np.asarray(self.fit_idx, dtype=np.int32))
        self.d_rfit = ctx.empty((spin, nidx, nidx), np.float64)
        self.d_drho = ctx.empty((spin, nidx, nidx), np.float64)
        self.d_ss = ctx.empty((1,), np.float64)
        self.nfev = self.ngev = 0
        self._key, self._state = None, None
        self.npair = n * (n + 1) // 2
        if dV is not None:
            dV = np.ascontiguousarray(dV, dtype=np.float64)
            log.eassert(dV.ndim == 3 and dV.shape[1:] == (spin, self.npair), "FullFitDevice: dV is (nparam, spin, npair)")
            self.nparam, self.d_dV = dV.shape[0], ctx.to_device(dV)
            self.d_even = ctx.to_device(np.arange(0, 2 * n, 2, dtype=np.int32))
            return
        if self.kpts:
            self.nparam = vcor.length()                       # slater.py:1439-1440: no dV_dparam, the gradient is assembled per k group
            return
        # dV_dparam of the lattice problem: tril-packed vcor.gradient() (get_dV_dparam_full, slater.py:1331-1350)
        g = np.asarray(vcor.gradient())
        self.nparam = g.shape[0]
        tl = np.tril_indices(n)
        self.d_dV = ctx.to_device(np.ascontiguousarray(g[:, :spin][:, :, tl[0], tl[1]], dtype=np.float64))
        self.d_even = ctx.to_device(np.arange(0, 2 * n, 2, dtype=np.int32))

    def _forward(self, param):
        param = np.ascontiguousarray(param, dtype=np.float64)
        key = param.tobytes() + (b"" if self.extra_shift is None else np.ascontiguousarray(self.extra_shift, dtype=np.float64).tobytes())
        if key == self._key:
            return self._state
        ctx, spin, nk, n, nb, nidx = self.ctx, self.spin, self.nk, self.n, self.nb, self.nidx
        mfd = self._mfd
        self.vcor.update(param)
        if self.kpts:
            per_k = np.asarray(self.vcor.value)[:, :spin].transpose(1, 0, 2, 3)                # (spin, nk, n, n) complex
            d_w, d_Vt = mfd.eigh_dev(ctx, ctx.to_device((self.F_host + per_k).reshape(spin * nk, n, n), np.complex128), n, spin * nk)
        else:
            v = np.ascontiguousarray(self._shift_of(self.vcor), dtype=np.float64)
            if self.extra_shift is not None:
                v = v + np.asarray(self.extra_shift, dtype=np.float64)
            d_add = ctx.to_device(v)
            d_w, d_Vt = mfd.eigh_dev(ctx, self.d_F, n, spin * nk, d_add, nk)
        ew = d_w.get().reshape(spin, nk, n)
        occ, mu, nerr = mfd.assignocc(ew, self.nelec, self.beta, mu0=0.0, fix_mu=self.fix_mu)
        d_occ = ctx.to_device(np.ascontiguousarray(occ).reshape(spin * nk, n), np.float64)
        d_rho = mfd.density_dev(ctx, d_Vt, d_occ, n, spin * nk)                   # (spin*nk, n, n) c128
        if self.imp_bath_fit:
            d_T = self._bgemm(ctx, "N", "N", n, nb, n, spin * nk, d_rho, n * n, self.d_bk, n * nb)
            d_R = self._bgemm(ctx, "C", "N", nb, nb, nk * n, spin, self.d_bk, nk * n * nb, d_T, nk * n * nb, alpha=1.0 / nk)
            dens = np.ascontiguousarray(d_R.get().reshape(spin, nb, nb).real)
            m = nb
        else:
            imax = ctx.zeros((1,), np.float64)
            d_rhoR = self._fourier.fold_k2R_dev(d_rho.reshape(spin, nk, n * n), self.lattice.kmesh, spin, n * n, imag_max=imax)
            dens = np.ascontiguousarray(d_rhoR.get().reshape(spin, nk, n, n)[:, 0])      # (1/nk) sum_k rho_k, real part
            self.last_dens = dens
            if float(imax.get()[0]) > IMAG_DISCARD_TOL:
                log.warn("rhoT has imag part %s", float(imax.get()[0]))
            m = n
        d_dens = ctx.to_device(dens)
        for s in range(spin):
            ctx.check(lib.dmk_gather2d_f64(ctx.h, nidx, nidx, self.d_fit.ptr, self.d_fit.ptr, d_dens.offset(s * m * m, (m, m)).ptr,
                                           m, self.d_rfit.offset(s * nidx * nidx, (nidx, nidx)).ptr))
        ctx.check(lib.dmk_ewise_mul(ctx.h, 0, spin * nidx, nidx, self.d_rfit.ptr, self.d_W.ptr, self.d_rfit.ptr))
        ctx.check(lib.dmk_sub_sumsq(ctx.h, spin * nidx * nidx, self.d_rfit.ptr, self.d_target.ptr, self.d_drho.ptr, self.d_ss.ptr))
        val = float(np.sqrt(self.d_ss.get()[0]))
        ctx.sync()
        self._key, self._state = key, (ew, mu, val, d_w, d_Vt)
        return self._state

    def errfunc(self, param):
        self.nfev += 1
        return self._forward(param)[2] / self.norm

    def gradfunc(self, param):
        """Analytic finite-T gradient (slater.py:1480-1640, local vcor): for every k
            dw_dv_k = ev_k^* [(ev_k[fit]^T 2 drho ev_k[fit]^*) o K_k] ev_k^T  (+ the per-k chemical-potential response),
        all k and spins in batched complex GEMMs on the resident eigenvectors; the k sum, real part, "x2 tril" packing
        and the contraction with dV_dparam are streaming kernels.  Row m of Vt is eigenvector m, so
        ev[fit]^T D' ev[fit]^* = Vt D Vt^H with D = drho scattered to the fitted indices, and ev^* X ev^T = Vt^H X Vt."""
        if self.imp_bath_fit:
            raise NotImplementedError("imp + bath fit has no analytic gradient (slater.py:1510-1512)")
        if self.beta == np.inf:
            raise NotImplementedError("no analytic T = 0 lattice gradient (slater.py:1642-1645)")
        self.ngev += 1
        ctx, spin, nk, n, nidx, beta = self.ctx, self.spin, self.nk, self.n, self.nidx, self.beta
        B, n2 = spin * nk, n * n
        bg = self._bgemm
        ew, mu, val, d_w, d_Vt = self._forward(param)
        f = np.empty((spin, nk, n))
        for k in range(nk):
            f[:, k] = ftsystem.fermi_smearing_occ(mu, ew[:, k], beta)
        d_f = ctx.to_device(np.ascontiguousarray(f).reshape(B, n))
        d_K = ctx.empty((B, n, n), np.float64)
        ctx.check(lib.dmk_fit_kmat(ctx.h, n, B, d_w.ptr, d_f.ptr, float(beta), 0, d_K.ptr))
        d_D = ctx.zeros((spin, n, n), np.complex128)
        for s in range(spin):
            ctx.check(lib.dmk_scatter2d_add_f64(ctx.h, nidx, self.d_fit.ptr, self.d_drho.offset(s * nidx * nidx, (nidx, nidx)).ptr,
                                                2.0, d_D.offset(s * n2, (n, n)).ptr, n, 2))
        d_T1 = ctx.empty((B, n, n), np.complex128)
        for s in range(spin):
            bg(ctx, "N", "N", n, n, n, nk, d_Vt.offset(s * nk * n2, (nk, n, n)), n2, d_D.offset(s * n2, (n, n)), 0,
               C=d_T1.offset(s * nk * n2, (nk, n, n)))
        d_tmp = bg(ctx, "N", "C", n, n, n, B, d_T1, n2, d_Vt, n2)
        ctx.check(lib.dmk_ewise_mul(ctx.h, 2, B * n, 2 * n, d_tmp.ptr, d_K.ptr, d_tmp.ptr))
        bg(ctx, "C", "N", n, n, n, B, d_Vt, n2, d_tmp, n2, C=d_T1)
        d_G = bg(ctx, "N", "N", n, n, n, B, d_T1, n2, d_Vt, n2, C=d_tmp)
        if self.kpts:
            return self._grad_per_k_group(d_G, d_Vt, d_D, f, val)
        d_sum = ctx.empty((spin, n, n), np.complex128)
        d_one = ctx.to_device(np.ones(nk))
        for s in range(spin):
            ctx.check(lib.dmk_dgemv2(ctx.h, nk, 2 * n2, d_G.offset(s * nk * n2, (nk, n, n)).ptr, 2 * n2, None, d_one.ptr, None,
                                     d_sum.offset(s * n2, (n, n)).ptr))
        if not self.fix_mu:
            d_rmu, coef = self._mu_response(d_Vt, d_D, f)                           # per (spin, k): ftsystem.py:265-279
            d_c = ctx.to_device(np.ascontiguousarray(coef).reshape(B))
            d_mu = ctx.empty((spin, n, n), np.complex128)
            for s in range(spin):
                ctx.check(lib.dmk_dgemv2(ctx.h, nk, 2 * n2, d_rmu.offset(s * nk * n2, (nk, n, n)).ptr, 2 * n2, None,
                                         d_c.offset(s * nk, (nk,)).ptr, None, d_mu.offset(s * n2, (n, n)).ptr))
            ctx.check(lib.dmk_axpy_f64(ctx.h, 2 * spin * n2, 1.0, d_mu.ptr, d_sum.ptr))
        d_re = ctx.empty((spin, n, n), np.float64)
        for s in range(spin):
            ctx.check(lib.dmk_gather2d_f64(ctx.h, n, n, None, self.d_even.ptr, d_sum.offset(s * n2, (n, n)).ptr, 2 * n,
                                           d_re.offset(s * n2, (n, n)).ptr))
        d_dw = ctx.empty((spin, self.npair), np.float64)
        ctx.check(lib.dmk_sym_fold(ctx.h, n, spin, d_re.ptr, d_dw.ptr))
        d_grad = ctx.empty((self.nparam,), np.float64)
        ctx.check(lib.dmk_dgemv2(ctx.h, self.nparam, spin * self.npair, self.d_dV.ptr, spin * self.npair, d_dw.ptr, None,
                                 d_grad.ptr, None))
        return d_grad.get() / (2.0 * val * self.norm * nk)


    def _mu_response(self, d_Vt, d_D, f):
        """Per (spin, k): drho_dmu / beta on the device and the coefficient of ftsystem.py:265-279 (zero where sum f (1 - f) vanishes)."""
        ctx, spin, nk, n, beta = self.ctx, self.spin, self.nk, self.n, self.beta
        B, n2 = spin * nk, n * n
        ff = f * (1.0 - f)
        fsum = ff.sum(axis=2)
        d_ff = ctx.to_device(np.ascontiguousarray(ff).reshape(B, n))
        d_rmu = self._mfd.density_dev(ctx, d_Vt, d_ff, n, B)
        d_y = ctx.empty((B,), np.float64)
        for s in range(spin):
            ctx.check(lib.dmk_dgemv2(ctx.h, nk, 2 * n2, d_rmu.offset(s * nk * n2, (nk, n, n)).ptr, 2 * n2,
                                     d_D.offset(s * n2, (n, n)).ptr, None, d_y.offset(s * nk, (nk,)).ptr, None))
        y = d_y.get().reshape(spin, nk)
        coef = np.where(np.abs(fsum) > ftsystem.ZERO_TOL, beta * y / np.where(fsum == 0.0, 1.0, fsum), 0.0)
        return d_rmu, coef

    def _grad_per_k_group(self, d_G, d_Vt, d_D, f, val):
        """slater.py:1519-1628 for vcor.VcorKpoints: the response matrix dw_dv of the FIRST k point of every inversion group
        answers for the group's parameters -- its real part (lower triangle, off-diagonal doubled) for the real parameters,
        -2 Im (strict lower triangle, doubled) for the imaginary ones of a +-k pair whose second member sees the conjugate.
        The matrices come from the batched device products of gradfunc; this is index bookkeeping on nparam numbers."""
        spin, nk, n, v = self.spin, self.nk, self.n, self.vcor
        dw = d_G.get().reshape(spin, nk, n, n)
        if not self.fix_mu:
            d_rmu, coef = self._mu_response(d_Vt, d_D, f)
            dw = dw + coef[:, :, None, None] * d_rmu.get().reshape(spin, nk, n, n)
        lo, so = np.tril_indices(n), np.tril_indices(n, -1)
        n_re = n * (n + 1) // 2
        res = np.zeros(self.nparam)
        for grp, ks in enumerate(v.kpts_map):
            step = v.param_k_slices[grp]
            for s in range(1 if v.restricted else spin):      # a restricted potential reads spin block 0 only (slater.py:1539-1552)
                sl = step if v.restricted else step[1 + s]
                m = dw[s, ks[0]]
                paired = len(ks) == 2
                re = (2.0 if paired else 1.0) * m.real
                re[so] *= 2.0
                res[sl.start:sl.start + n_re] = re[lo]
                if paired:
                    res[sl.start + n_re:sl.stop] = -4.0 * m.imag[so]
        return res / (2.0 * val * self.norm * nk)


def FitVcorFull(rho, lattice, basis, vcor, beta, filling, MaxIter=20, imp_fit=False, imp_idx=None, det=False, det_idx=None,
                CG_check=False, BFGS=False, diff_criterion=None, scf=False, **kwargs):
    """
    Fit the correlation potential in the full lattice space (slater.py:1352-1682).  The objective runs on the device
    (FullFitDevice); the gradient is the reference's analytic finite-T lattice gradient (FullFitDevice.gradfunc,
    slater.py:1480-1640) or, with `num_grad=True` (required at T = 0 as in the reference), central differences inside
    the minimiser.  A vcor.VcorKpoints potential (one matrix per k point) takes the per-k-group gradient of slater.py:1519-1628
    (FullFitDevice._grad_per_k_group).  The SCF variant is outside the HIP path.
    """
    if scf:
        raise NotImplementedError("the SCF variant of FitVcorFull is outside the HIP path")
    if not vcor.is_local() and not getattr(vcor, "is_vcor_kpts", False):
        raise NotImplementedError("FitVcorFull: a cell-resolved potential has no lattice-stage gradient (get_dV_dparam_full asserts a local "
                                  "one, slater.py:1341); fit it in the embedding space (FitVcorEmb)")
    if not kwargs.get("num_grad", False) and beta == np.inf:
        raise NotImplementedError("FitVcorFull: no analytic T = 0 gradient, pass num_grad=True (slater.py:1642-1645)")
    basis = np.asarray(basis)
    param_begin = vcor.param.copy()
    spin, nkpts, nao, nbasis = basis.shape
    assert len(rho) == spin
    imp_bath_fit = False
    if imp_fit:
        if imp_idx is None:
            imp_idx = list(range(lattice.nimp))
        det_idx = []
    elif det:
        imp_idx = []
        if det_idx is None:
            det_idx = list(range(lattice.nimp))
    elif imp_idx is None:
        if det_idx is None:
            imp_idx, det_idx = list(range(nbasis)), []
            imp_bath_fit = True
        else:
            imp_idx = []
    elif det_idx is None:
        det_idx = []
    imp_idx, det_idx = list(imp_idx), list(det_idx)
    if np.asarray(rho).shape[-1] != nao:
        log.warn("FitVcorFull: target rho should has shape (%s, %s, %s) , now has shape %s ...", spin, nao, nao,
                 np.asarray(rho).shape)
    if isinstance(filling, Iterable):
        nelec = [nkpts * nao * filling[0], nkpts * nao * filling[1]]
        nelec[0], nelec[1] = mfd_check_nelec(nelec[0])[0], mfd_check_nelec(nelec[1])[0]
    else:
        nelec = mfd_check_nelec(spin * nkpts * nao * filling)[0]
    ctx = get_ctx()
    fit = FullFitDevice(ctx, np.asarray(rho), lattice, basis, vcor, beta, nelec, imp_idx, det_idx, imp_bath_fit,
                        fix_mu=kwargs.get("fix_mu", False))
    if kwargs.get("num_grad", False):
        log.warn("You are using numerical gradient...")
        gradfunc = None
    else:
        log.info("Using analytic gradient for finite T, beta = %s", beta)
        gradfunc = fit.gradfunc
    err_begin = fit.errfunc(param_begin)
    param, err_end, pattern, gnorm_res = minimize(fit.errfunc, param_begin.copy(), MaxIter, gradfunc, **kwargs)
    vcor.update(param)
    log.info("Minimizer converge pattern: %d ", pattern)
    log.info("Current function value: %15.8f", err_end)
    log.info("Norm of gradients: %s", gnorm_res)
    log.info("Norm diff of x: %6.3e", max_abs(param - param_begin))
    FitVcorFull.last_fit = fit
    return vcor, err_begin, err_end


def FitVcorTwoStep(rho, lattice, basis, vcor, beta, filling, MaxIter1=300, MaxIter2=0, **kwargs):
    """Main wrapper for correlation potential fitting (slater.py:1684-1714): embedding-space stage, then lattice stage."""
    import copy
    vcor_new = copy.deepcopy(vcor)
    log.result("Using two-step vcor fitting")
    err_begin = None
    if MaxIter1 > 0:
        log.info("Impurity model stage  max %d steps", MaxIter1)
        vcor_new, err_begin, err_end = FitVcorEmb(rho, lattice, basis, vcor_new, beta, MaxIter=MaxIter1, **kwargs)
        log.result("residue (begin) = %20.12f", err_begin)
        log.info("residue (end)   = %20.12f", err_end)
    if MaxIter2 > 0:
        log.info("Full lattice stage  max %d steps", MaxIter2)
        vcor_new, err_begin2, err_end = FitVcorFull(rho, lattice, basis, vcor_new, beta, filling, MaxIter=MaxIter2, **kwargs)
        if err_begin is None:
            err_begin = err_begin2
    log.result("residue (begin) = %20.12f", err_begin)
    log.result("residue (end)   = %20.12f", err_end)
    return vcor_new, err_end


# ---------------------------------------------------------------------------------------------
# behind the solver (slater.py:1716-2119): scaled Hamiltonians, results, the veff rebuild, the DMET energy Hamiltonian
# ---------------------------------------------------------------------------------------------

def _env_of(nbasis, imp_idx):
    return np.asarray([idx for idx in range(nbasis) if idx not in imp_idx], dtype=int)


def get_H1_scaled(H1, imp_idx, env_idx=None):
    """Scale H1 by the number of impurity indices, in place (slater.py:1716-1732): imp-env blocks halved, env-env zeroed."""
    assert H1.ndim == 3
    if env_idx is None:
        env_idx = _env_of(H1.shape[-1], imp_idx)
    imp_env, env_imp, env_env = np.ix_(imp_idx, env_idx), np.ix_(env_idx, imp_idx), np.ix_(env_idx, env_idx)
    for s in range(H1.shape[0]):
        H1[s][imp_env] *= 0.5
        H1[s][env_imp] *= 0.5
        H1[s][env_env] = 0.0
    return H1


def h2_scaled_dev(ctx, n, imp_idx, d_in, in_symmetry, d_out, out_symmetry, ld_in=None, ld_out=None):
    """dmk_dmet_h2_scaled on device blocks: d_out = the ERI block d_in weighted by (m_i + m_j + m_k + m_l) / 4, m the indicator
    of imp_idx; symmetries (in, out) in (4, 4), (1, 4), (8, 4), (4, 1), (1, 1); d_out may be d_in where they agree."""
    row = {1: n * n, 4: n * (n + 1) // 2, 8: 0}
    imp = np.ascontiguousarray(np.asarray(imp_idx).ravel(), dtype=np.int32)
    ctx.check(lib.dmk_dmet_h2_scaled(ctx.h, int(n), imp.ctypes.data if imp.size else None, int(imp.size), int(in_symmetry), d_in.ptr,
                                     int(row[in_symmetry] if ld_in is None else ld_in), int(out_symmetry), d_out.ptr,
                                     int(row[out_symmetry] if ld_out is None else ld_out)))
    return d_out


def get_H2_scaled(H2, imp_idx, env_idx=None):
    """Scale H2 by the number of impurity indices, in place on the array passed (slater.py:1734-1778): (nblk, npair, npair)
    4-fold or (nblk, n, n, n, n) 1-fold.  Each spin block goes through the device once (dmk_dmet_h2_scaled), bit-identical to
    the reference's mask loops."""
    if H2.ndim == 3:
        n, sym = int(np.sqrt(H2.shape[-1] * 2)), 4
    elif H2.ndim == 5:
        n, sym = H2.shape[-1], 1
        if env_idx is not None and sorted(np.asarray(env_idx).tolist()) != _env_of(n, imp_idx).tolist():
            raise NotImplementedError("get_H2_scaled: env_idx must be the complement of imp_idx")
    else:
        raise ValueError("Unknown H2 shape to scale: %s" % (str(H2.shape)))
    ctx = get_ctx()
    for s in range(H2.shape[0]):
        d = ctx.to_device(H2[s], np.float64)
        H2[s] = h2_scaled_dev(ctx, n, imp_idx, d, sym, d, sym).get()
    return H2


def transformResults(rhoEmb, E, basis, ImpHam, H1e=None, **kwargs):
    """Density matrix of the impurity, DMET energy (non-interacting bath) and electron number (slater.py:1780-1840)."""
    spin = rhoEmb.shape[0]
    nscsites = basis.shape[2]
    nbasis = basis.shape[-1]
    if "lattice" in kwargs:
        imp_idx = np.asarray(kwargs.get("imp_idx", range(kwargs["lattice"].nimp)))
    else:
        imp_idx = np.asarray(kwargs.get("imp_idx", np.arange(nscsites)))
    if any(imp_idx >= nscsites):
        log.warn("imp_idx is out of the first cell... imp_idx:\n%s", imp_idx)
    nelec = 0.0
    for s in range(spin):
        nelec += np.sum(rhoEmb[s, imp_idx, imp_idx])
    nelec *= (2.0 / spin)
    rhoImp = rhoEmb[np.ix_(range(spin), imp_idx, imp_idx)]

    if E is None:
        return rhoImp, None, nelec
    lattice = kwargs["lattice"]
    last_dmu = kwargs["last_dmu"]
    imp_idx = np.asarray(kwargs.get("imp_idx", list(range(lattice.nimp))))
    dmu_idx = kwargs.get("dmu_idx", None)
    if dmu_idx is None:
        dmu_idx = list(range(nscsites))
    env_idx = _env_of(nbasis, imp_idx)

    E2 = E - np.einsum('spq, sqp', ImpHam.H1["cd"], rhoEmb) * (2.0 / spin) - ImpHam.H0
    H1_scaled = np.array(ImpHam.H1["cd"], copy=True)
    dmu_mat = np.zeros((nscsites, nscsites))
    dmu_mat[dmu_idx, dmu_idx] = -last_dmu
    for s in range(spin):
        H1_scaled[s] -= transform_imp(basis[s], lattice, dmu_mat)      # remove the contribution of last_dmu
        if lattice.JK_core is not None:                                # and the JK_core
            H1_scaled[s] -= 0.5 * lattice.JK_core[s]
    H1_scaled = get_H1_scaled(H1_scaled, imp_idx, env_idx)
    E1 = np.einsum('spq, sqp', H1_scaled, rhoEmb) * (2.0 / spin)
    Efrag = E1 + E2 + lattice.getH0()
    log.debug(0, "E0 = %20.12f, E1 = %20.12f, E2 = %20.12f, E = %20.12f", lattice.getH0(), E1, E2, Efrag)
    return rhoImp, Efrag, nelec


def get_veff_from_rdm1_emb(lattice, rdm1_emb, basis, kmf=None, C_ao_lo=None, return_update=False, sign=None):
    """veff in the LO basis from the global density of the embedding rdm1 (per spin), slater.py:1842-1903: democratic global
    density x 2 / spin -> AO -> J, K -> LO.  J and K come from
      a model lattice with H2_format "local": the cell-0 density against the local ERI on the device (as LatticeModel.update_Ham;
          "nearest" / "full" raise NotImplementedError as there);
      ab initio: kmf.get_jk(dm_kpts=.) when kmf offers it, else the device DF build pbc_helper.get_jk_gdf(lattice.cell, lattice.df, .).
    return_update=True: (veff, veff_ao, lattice.k2R(rdm1_glob)), what lattice.update_Ham takes.
    The reference also writes rdm1_glob_lo_k.npy into the working directory; that side effect is NOT mirrored."""
    from libdmet_preview_amd.basis_transform import make_basis
    if not isinstance(lattice, Iterable):
        lattice, rdm1_emb, basis = [lattice], [rdm1_emb], [basis]
    lat0 = lattice[0]
    if kmf is None:
        kmf = getattr(lat0, "kmf", None)
    if C_ao_lo is None:
        if lat0.is_model:
            spin, nkpts, nlo, neo = np.asarray(basis[0]).shape
            C_ao_lo = np.zeros((spin, nkpts, nlo, nlo))
            C_ao_lo[:, :, range(nlo), range(nlo)] = 1.0
        else:
            C_ao_lo = lat0.C_ao_lo
    spin = np.asarray(basis[0]).shape[-4]

    rdm1_glob = get_rho_glob_k(basis, lattice, rdm1_emb, sign=sign) * (2.0 / spin)
    rdm1_veff = make_basis.transform_rdm1_to_ao(rdm1_glob, C_ao_lo)

    if lat0.is_model:
        if lat0.H2_format == "local":
            dm = np.asarray(rdm1_veff)
            dm_ave = dm.sum(axis=-3) / float(dm.shape[-3])
            if max_abs(dm_ave.imag) >= IMAG_DISCARD_TOL:
                log.warn("get_veff_from_rdm1_emb: a local ERI assumes a real cell-0 density, now imag = %s", max_abs(dm_ave.imag))
            vj0, vk0 = _get_jk(np.ascontiguousarray(dm_ave.real), np.asarray(lat0.getH2(compact=False, kspace=False)))
            vj, vk = (np.repeat(np.asarray(v)[:, None], dm.shape[-3], axis=1) for v in (vj0, vk0))
        elif lat0.H2_format in ("nearest", "full"):
            raise NotImplementedError("get_veff_from_rdm1_emb with a %s lattice ERI (cell-resolved J / K) is not built"
                                      % lat0.H2_format)
        else:
            raise ValueError
        veff_ao = vj - (vk * 0.5) if spin == 1 else vj[0] + vj[1] - vk
    elif getattr(lat0.cell, 'pbc_intor', None) or not hasattr(kmf, "get_jk"):
        if kmf is not None and hasattr(kmf, "get_jk"):
            vj, vk = kmf.get_jk(dm_kpts=rdm1_veff)
        else:
            from libdmet_preview_amd.routine import pbc_helper
            vj, vk = pbc_helper.get_jk_gdf(lat0.cell, lat0.df, rdm1_veff)
        vj, vk = np.asarray(vj), np.asarray(vk)
        veff_ao = vj - (vk * 0.5) if spin == 1 else vj[0] + vj[1] - vk
    else:       # a molecular mean-field object: one density per spin
        if spin == 1:
            vj, vk = kmf.get_jk(dm=rdm1_veff[0, 0])
            veff_ao = (vj - (vk * 0.5))[None, None]
        else:
            vj, vk = kmf.get_jk(dm=rdm1_veff[:, 0])
            veff_ao = (vj[0] + vj[1] - vk)[:, None]

    veff = make_basis.transform_h1_to_lo(veff_ao, C_ao_lo)
    if return_update:
        return veff, veff_ao, lat0.k2R(rdm1_glob)
    return veff


def _h2_dmet_blocks(H2, nbasis, imp_idx, nblk, compact):
    """The scaled two-body part of get_H_dmet: blocks H2[s] (any storage) -> 4-fold (compact) or 1-fold, one device pass each;
    a 4-fold input goes to the scaled 1-fold output directly (no scaled 4-fold intermediate)."""
    ctx = get_ctx()
    npair = nbasis * (nbasis + 1) // 2
    out = np.empty((nblk, npair, npair) if compact else (nblk,) + (nbasis,) * 4)
    everything = np.arange(nbasis)
    for s in range(nblk):
        blk = np.asarray(H2[s], dtype=np.float64)
        sym = {"s1": 1, "s4": 4, "s8": 8}[integral.get_eri_format(blk, nbasis)[0]]
        d = ctx.to_device(blk.reshape(-1))
        if sym != 4:
            d = h2_scaled_dev(ctx, nbasis, imp_idx, d, sym, ctx.empty((npair, npair), np.float64), 4)
        elif compact:
            d = h2_scaled_dev(ctx, nbasis, imp_idx, d, 4, d, 4)
        if not compact:     # (a block that was gathered above is already scaled: the plain restore is the all-impurity case)
            d = h2_scaled_dev(ctx, nbasis, imp_idx if sym == 4 else everything, d, 4, ctx.empty((nbasis,) * 4, np.float64), 1)
        out[s] = d.get().reshape(out.shape[1:])
    return out


def get_H_dmet(basis, lattice, ImpHam, last_dmu, imp_idx=None, dmu_idx=None, add_vcor_to_E=False, vcor=None, compact=True,
               rdm1_emb=None, veff=None, rebuild_veff=False, E1=None, **kwargs):
    """The DMET Hamiltonian, scaled by the number of impurity indices, whose expectation value is the DMET energy
    (slater.py:1957-2032).  rdm1_emb: embedding rdm1 per spin; veff: used as JK_core if given; rebuild_veff: JK_core from the
    global density; E1: taken as the one-body energy (hcore, J and K).  The aabb order of an unrestricted Hamiltonian is kept.
    compact=False returns the 1-fold ERI, written by the scaling kernel itself."""
    log.debug(0, "Construct Heff for DMET.")
    spin = basis.shape[0]
    nbasis = basis.shape[-1]
    if imp_idx is None:
        imp_idx = list(range(lattice.nimp))
    imp_idx = np.asarray(imp_idx)
    env_idx = _env_of(nbasis, imp_idx)
    basis_k = lattice.R2k_basis(basis)

    if E1 is None:
        H1_scaled = transform_h1(lattice.getH1(kspace=True), basis_k)
        # note the double counting from JK_core cf. HF energy
        if (veff is not None) or rebuild_veff:
            if veff is None:
                veff = get_veff_from_rdm1_emb(lattice, rdm1_emb, basis)
            JK_core = transform_h1(veff, basis_k)
            JK_core -= get_veff(rdm1_emb * (2.0 / spin), ImpHam.H2["ccdd"], hyb=1.0)
            if lattice.JK_core is not None:
                log.debug(1, "difference between JK_glob and JK_HF: %15.8g", max_abs(JK_core - lattice.JK_core))
        elif lattice.JK_core is not None:
            JK_core = lattice.JK_core
        else:
            JK_core = [0.0 for s in range(spin)]
        for s in range(spin):
            H1_scaled[s] += 0.5 * JK_core[s]
            if add_vcor_to_E:
                log.debug(0, "Add Vcor to energy expression")
                H1_scaled[s] += transform_local(basis[s], lattice, vcor.get()[s] * 0.5)
                H1_scaled[s] -= transform_imp(basis[s], lattice, vcor.get()[s] * 0.5)
        H1_scaled = get_H1_scaled(H1_scaled, imp_idx, env_idx)
        H0 = lattice.getH0()
    else:
        # manually specify E1 (contribution from hcore and J, K)
        H1_scaled = (-1.0 / spin) * get_veff(rdm1_emb, ImpHam.H2["ccdd"], hyb=1.0)
        H1_scaled = get_H1_scaled(H1_scaled, imp_idx, env_idx)
        H0 = (E1 + lattice.getH0()).real

    if not compact:
        log.warn("Restoring 1-fold symmetry in dmet Hamiltonian...")
    H2_scaled = _h2_dmet_blocks(ImpHam.H2["ccdd"], nbasis, imp_idx, spin * (spin + 1) // 2, compact)
    return integral.Integral(nbasis, spin == 1, False, H0, {"cd": H1_scaled}, {"ccdd": H2_scaled})


def get_E_dmet(basis, lattice, ImpHam, last_dmu, solver, solver_args={}, **kwargs):
    ImpHam_scaled = get_H_dmet(basis, lattice, ImpHam, last_dmu, **kwargs)
    return solver.run_dmet_ham(ImpHam_scaled, **solver_args)


def get_E_dmet_HF(basis, lattice, ImpHam, last_dmu, solver, **kwargs):
    """DMET energy of a mean-field solver (slater.py:2039-2085); `solver.mf` (or `solver.scfsolver.mf`) is asked for
    make_rdm1, get_hcore and get_fock."""
    log.debug(0, "Construct Heff for DMET (HF).")
    spin = basis.shape[0]
    nbasis = basis.shape[-1]
    nscsites = lattice.nscsites
    mf = solver.mf if hasattr(solver, "mf") else solver.scfsolver.mf
    imp_idx = kwargs.get("imp_idx", list(range(lattice.nimp)))
    env_idx = _env_of(nbasis, imp_idx)
    dmu_mat = np.zeros((nscsites, nscsites))
    dmu_mat[imp_idx, imp_idx] = (-last_dmu)

    rdm1 = np.asarray(mf.make_rdm1())
    h1e = np.asarray(mf.get_hcore())
    fock = np.asarray(mf.get_fock(h1e=h1e, dm=rdm1))
    if rdm1.ndim == 2:
        rdm1, h1e, fock = rdm1[np.newaxis], h1e[np.newaxis], fock[np.newaxis]
    heff = (h1e + fock) * 0.5
    for s in range(spin):
        if lattice.JK_core is not None:        # remove the double counting from JK_core cf. HF energy
            heff[s] -= 0.5 * lattice.JK_core[s]
        heff[s] -= transform_imp(basis[s], lattice, dmu_mat)
    heff = get_H1_scaled(heff, imp_idx, env_idx)
    E = np.sum(heff * rdm1) + lattice.getH0()
    if lattice.JK_core is not None:
        JK_core_scaled = get_H1_scaled(np.asarray(lattice.JK_core) * 0.5, imp_idx, env_idx)
        log.debug(0, "JK_core contribution in DMET HF energy: %20.10f", np.sum(JK_core_scaled * rdm1))
    return E


def get_H1_dmet(lattice, basis, hcore_lo_k, fock_lo_k, JK_imp, imp_idx=None):
    """The scaled one-body DMET Hamiltonian from hcore_lo_k, fock_lo_k and JK_imp alone (slater.py:2091-2119)."""
    log.debug(0, "Construct Heff_1 for DMET.")
    spin, nkpts, nlo, nbasis = basis.shape
    basis_k = lattice.R2k_basis(basis)
    hcore_emb = transform_h1(hcore_lo_k, basis_k)
    fock_emb = transform_h1(fock_lo_k, basis_k)
    JK_imp = add_spin_dim(JK_imp, spin, non_spin_dim=2)
    JK_emb = np.asarray([transform_imp(basis[s], lattice, JK_imp[s]) for s in range(spin)])
    H1 = hcore_emb + (fock_emb - hcore_emb - JK_emb) * 0.5
    if imp_idx is None:
        imp_idx = list(range(lattice.nimp))
    imp_idx = np.asarray(imp_idx)
    return get_H1_scaled(H1, imp_idx, _env_of(nbasis, imp_idx))
