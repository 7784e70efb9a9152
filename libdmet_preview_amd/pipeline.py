"""
Device-resident embedding-construction iteration on synthetic k-sampled tensors:

    Fock_k + vcor --eigh--> (ew, ev) --occupations--> rho_k --k2R--> rho_R   (routine/mfd.py:235-360)
    rho_R --Schmidt bath--> basis = C_lo_eo                                   (routine/slater.py:98-220)
    basis --R2k, C_ao_lo--> C_ao_emb --DF half transform + contraction--> ERI (eri_transform.py:235-399)
    basis, ERI, rho --one-body folds + ERI x density--> H1_emb = fock_emb - JK_emb      (routine/slater.py:525-680)

Inputs live in HBM before the iteration starts; only scalars and O(nk*nlo) vectors (eigenvalues,
occupations, singular values) cross PCIe.  Multi-GPU (one process per GPU):
k-points are sharded for the diag/density stage (+-k kept together) with ONE all-reduce of the
eigenvalue table and ONE of the partial rho_R; irreducible kL are sharded for the ERI stage, whose planes stay resident
(K-stacked contraction) so that the final contraction can be finished band by band of the pair index with every finished
band reduced to its owner rank underneath the remaining GEMMs; the summed ERI stays row-sharded and only the n x n J / K
matrices of the embedding Hamiltonian are all-reduced.
"""
import os
import time
import numpy as np

from libdmet_preview_amd import synth
from libdmet_preview_amd._lib import lib, mesh3
from libdmet_preview_amd.basis_transform import eri_transform as et
from libdmet_preview_amd.basis_transform.make_basis import bgemm_dev
from libdmet_preview_amd.parallel import dist
from libdmet_preview_amd.routine import mfd, slater
from libdmet_preview_amd.solver import scf
from libdmet_preview_amd.system import fourier
from libdmet_preview_amd.system.lattice import _UnitCell


class SyntheticSystem(object):
    """Seeded synthetic lattice problem of a BASELINE.json config, resident in HBM."""

    def __init__(self, ctx, mesh, nlo, naux, nval, spin, seed=synth.DEFAULT_SEED, filling=0.5, name="custom"):
        self.ctx = ctx
        self.name = name
        self.mesh = [int(x) for x in mesh] + [1] * (3 - len(mesh))
        self.nk = int(np.prod(self.mesh))
        self.nlo = self.nao = int(nlo)
        self.naux, self.nval, self.spin = int(naux), int(nval), int(spin)
        self.filling = filling
        self.seed = int(seed)
        self.restricted = (spin == 1)
        FR = synth.make_fock_R(self.mesh, nlo, spin=spin, seed=seed)
        self.Fock_R = FR
        self.d_Fock_k = ctx.to_device(synth.fold_R2k(FR, self.mesh), np.complex128)       # (spin, nk, n, n)
        self.hcore_scale = 0.5                        # synthetic hcore = 0.5 Fock (vhf = the other half), as in G3
        v = np.zeros((2, nlo, nlo))
        self.vcor = v
        self.d_vcor = ctx.to_device(v[:spin])
        C = synth.make_C_ao_lo(self.mesh, nlo, nlo, spin=spin, seed=seed + 1)
        self.C_ao_lo = C
        self.d_C_ao_lo = ctx.to_device(C, np.complex128)
        self.cell = _UnitCell(nlo)
        ks = fourier.make_kpts_scaled(self.mesh)
        self.kpts = self.cell.get_abs_kpts(ks)
        self.df = et.GDFPhilox(self.kpts, naux, nlo, seed=seed + 2) if naux > 0 else None
        self.df_resident = None                 # et.GDFResident of a kL shard (make_df_resident): the blocks kept in HBM
        self.eri_inv_cache = None               # et.EriInvariantCache of eri_stage: invariant step-2 planes kept across iterations
        # orbital index sets: impurity = cell 0, valence = first nval orbitals (ncore = 0)
        self.imp_idx = list(range(nlo))
        self.val_idx = list(range(nval))
        bath_set = set(self.val_idx)
        env = [i for i in range(self.nk * nlo) if i not in bath_set]
        self.env_idx = np.asarray(env, dtype=np.int32)
        self.virt_mask = np.asarray([i < nlo for i in env], dtype=np.int32)
        self.d_env = ctx.to_device(self.env_idx)
        self.d_virt = ctx.to_device(self.virt_mask)
        self.d_col = ctx.to_device(np.asarray(self.val_idx, dtype=np.int32))
        self.d_imp = ctx.to_device(np.asarray(self.imp_idx, dtype=np.int32))
        _, self.neg, _ = fourier.kmesh_tables(self.mesh)

    @classmethod
    def from_workload(cls, ctx, name, seed=synth.DEFAULT_SEED, **over):
        w = dict(synth.WORKLOADS[name])
        w.update(over)
        return cls(ctx, w["mesh"], w["nlo"], w["naux"], w["nval"], w["spin"], seed=seed, name=name)

    def make_df_resident(self, kL_list=None, max_fraction_of_free=0.45):
        """Keep the AO DF blocks of `kL_list` (default: every irreducible kL) resident in HBM when they fit in
        `max_fraction_of_free` of the free device memory; later ERI transforms of those kL read them in place instead of
        regenerating / re-reading them (et.GDFResident).  Returns the bytes held (0: does not fit, nothing changed)."""
        if self.df is None:
            return 0
        need = et.GDFResident.bytes_needed(self.mesh, self.nao, self.naux, kL_list)
        free, _ = self.ctx.mem_info()
        if need == 0 or need > max_fraction_of_free * free:
            return 0
        if self.df_resident is not None:
            self.df_resident.free()
        self.df_resident = et.GDFResident(self.ctx, self.df, self.mesh, self.nao, self.naux, kL_list)
        return need

    def k_shard(self, rank, world):
        """k-points owned by `rank`: +-k pairs stay together."""
        if world == 1:
            return list(range(self.nk))
        groups = [sorted({k, int(self.neg[k])}) for k in range(self.nk) if k <= int(self.neg[k])]
        mine = []
        for g_i, grp in enumerate(groups):
            if g_i % world == rank:
                mine.extend(grp)
        return sorted(mine)


_STAGE_SYNC = os.environ.get("DMK_STAGE_SYNC", "1") != "0"


def _stage(ctx, timers, key, t0):
    """Close a stage's timer.  The device is drained first so that the seconds belong to the stage (DMK_STAGE_SYNC=0: no drain --
    the stage timers then only hold host time, the step is a few synchronisations shorter: for latency-bound tiny systems)."""
    if _STAGE_SYNC:
        ctx.sync()
    t1 = time.perf_counter()
    timers[key] = timers.get(key, 0.0) + (t1 - t0)
    return t1


def mean_field_stage(ctx, sysm, timers=None, tol_bath=1e-9):
    """diag + occupations + density + fold (+ all-reduce): returns device rho_R (spin, nk, n*n) f64 and info."""
    timers = {} if timers is None else timers
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    rank, world = dist.rank(), dist.world_size()
    t = time.perf_counter()
    kmine = sysm.k_shard(rank, world)
    if world == 1:
        d_F = sysm.d_Fock_k.reshape(spin * nk, n, n)
        nloc = nk
    else:
        # this rank's (spin, k) rows of the resident Fock batch: ONE gather launch (mfd_mpi.py:64-74 scatters them over MPI)
        nloc = len(kmine)
        if nloc == 0:
            # more ranks than +-k groups (a 2-point mesh on three ranks): this rank diagonalises nothing and only takes part in the
            # sums (the reference's scatter hands such a rank an empty list as well, mfd_mpi.py:64-74)
            return _mean_field_stage_idle(ctx, sysm, timers, t)
        rows = np.asarray([s * nk + k for s in range(spin) for k in kmine], dtype=np.int32)
        d_rows = ctx.to_device(rows)
        d_F = ctx.empty((spin * nloc, n, n), np.complex128)
        ctx.check(lib.dmk_copy_rows_f64(ctx.h, len(rows), 2 * n * n, d_rows.ptr, sysm.d_Fock_k.ptr, d_F.ptr, 0))
    d_w, d_Vt = mfd.eigh_dev(ctx, d_F, n, spin * nloc, sysm.d_vcor, nloc)
    t = _stage(ctx, timers, "diag", t)
    if world == 1:
        # occupations without leaving the device: no D2H of the eigenvalues, no host sort (csrc/occ.hip)
        d_w_all = d_w
        d_occ, mu, nerr = mfd.assignocc_dev(ctx, d_w, spin * nk * n * sysm.filling, np.inf)
        d_occ_all = d_occ
    else:
        # every rank needs ALL eigenvalues for the Fermi level: the shards are scattered into a zeroed all-k table and summed
        # over ranks on the device (mfd_mpi.py:93-94 gathers them through pickled MPI messages); the occupation kernel then
        # runs replicated (one workgroup, 1.9 ms at C5) and the rank keeps its own rows -- nothing crosses PCIe
        d_w_all = ctx.zeros((spin * nk, n), np.float64)
        ctx.check(lib.dmk_copy_rows_f64(ctx.h, len(rows), n, d_rows.ptr, d_w.ptr, d_w_all.ptr, 1))
        dist.all_reduce_sum_dev(d_w_all)
        d_occ_all, mu, nerr = mfd.assignocc_dev(ctx, d_w_all, spin * nk * n * sysm.filling, np.inf)
        d_occ = ctx.empty((spin * nloc, n), np.float64)
        ctx.check(lib.dmk_copy_rows_f64(ctx.h, len(rows), n, d_rows.ptr, d_occ_all.ptr, d_occ.ptr, 0))
    t = _stage(ctx, timers, "occupations", t)
    d_rho = mfd.density_dev(ctx, d_Vt, d_occ, n, spin * nloc)
    t = _stage(ctx, timers, "density", t)
    d_rhoR = fourier.fold_k2R_dev(d_rho.reshape(spin, nloc, n * n), sysm.mesh, spin, n * n,
                                  k_subset=None if world == 1 else kmine)
    t = _stage(ctx, timers, "fold_k2R", t)
    if dist.is_initialized():
        dist.all_reduce_sum_dev(d_rhoR)
        t = _stage(ctx, timers, "allreduce_rho", t)
    return d_rhoR, {"mu": mu, "ew": d_w_all, "occ": d_occ_all, "nerr": nerr}


def _mean_field_stage_idle(ctx, sysm, timers, t):
    """mean_field_stage of a rank that owns no k-point: zeros into the two sums, the replicated occupation kernel, nothing else."""
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    t = _stage(ctx, timers, "diag", t)
    d_w_all = ctx.zeros((spin * nk, n), np.float64)
    dist.all_reduce_sum_dev(d_w_all)
    d_occ_all, mu, nerr = mfd.assignocc_dev(ctx, d_w_all, spin * nk * n * sysm.filling, np.inf)
    t = _stage(ctx, timers, "occupations", t)
    t = _stage(ctx, timers, "density", t)
    d_rhoR = ctx.zeros((spin, nk, n * n), np.float64)
    t = _stage(ctx, timers, "fold_k2R", t)
    dist.all_reduce_sum_dev(d_rhoR)
    _stage(ctx, timers, "allreduce_rho", t)
    return d_rhoR, {"mu": mu, "ew": d_w_all, "occ": d_occ_all, "nerr": nerr}


def bath_stage(ctx, sysm, d_rhoR, timers=None, tol_bath=1e-9):
    """Schmidt bath on the device: returns device basis (spin, nk, nlo, nemb) f64, nemb and sigma."""
    timers = {} if timers is None else timers
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    nb, nenv, nimp = sysm.nval, len(sysm.env_idx), n
    t = time.perf_counter()
    svd, sigmas, nbaths = [], [], []
    # both spin channels through ONE chain of launches (TSQR tree, Jacobi SVD of the two root R factors side by side)
    d_sigma, d_U_all = slater.bath_svd_batched_dev(ctx, sysm.mesh, n, d_rhoR, spin, sysm.d_env, nenv, sysm.d_col, nb)
    sig_all = d_sigma.get()
    for s in range(spin):
        svd.append(d_U_all.offset(s * nenv * nb, (nenv, nb)))
        sigmas.append(sig_all[s])
        nbaths.append(int((sig_all[s] >= tol_bath).sum()))
    nbath_final = min([nb] + nbaths)          # nbath_final seed: len(imp_idx_bath) or nlo (slater.py:171,175)
    nemb = nimp + nbath_final
    d_basis = ctx.empty((spin, nk * n, nemb), np.float64)
    for s in range(spin):
        slater.bath_assemble_dev(ctx, svd[s], nenv, nb, nbaths[s], sysm.d_virt, True, sysm.d_env, sysm.d_imp, nimp,
                                 nk * n, nemb, d_basis.offset(s * nk * n * nemb, (nk * n, nemb)))
    _stage(ctx, timers, "bath", t)
    return d_basis, nemb, sigmas


def small_lattice_stages(ctx, sysm, timers=None, tol_bath=1e-9):
    """Mean field + Schmidt bath of a SMALL model lattice (<= 8 orbitals per cell, spin * nk <= 256) as two launches and ONE
    read-back (csrc/small.hip: dmk_small_meanfield, dmk_small_bath): the same products as mean_field_stage + bath_stage, or None
    when the shape is outside the limits of the fused kernels (or DMK_SMALL=0).  reference: routine/mfd.py:235-360,
    routine/slater.py:117-220."""
    import ctypes as C
    import os
    if os.environ.get("DMK_SMALL", "1") == "0" or dist.world_size() > 1:
        return None
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    nb, nenv, nimp = sysm.nval, len(sysm.env_idx), n
    if n > 8 or nb > 8 or spin * nk > 128 or nk > 128:
        return None
    timers = {} if timers is None else timers
    t = time.perf_counter()
    # Everything that does not change from step to step lives with the system: the device arrays of the step (seven hipMalloc /
    # hipFree pairs cost more than the two kernels), the mesh / electron count / views of the result record.  The products
    # returned below are therefore valid until the next small-lattice step on the same system.
    ws = sysm.__dict__.get("_small_ws")
    if ws is None:
        from libdmet_preview_amd._lib import mesh3
        nrec = 12 + spin * nb + 2                   # one result record: info[12] | sigma[spin][nb] | (ncol, nbath_s.., flag) as int32
        d_rec = ctx.empty((nrec,), np.float64)
        ws = {"w": ctx.empty((spin * nk, n), np.float64), "occ": ctx.empty((spin * nk, n), np.float64),
              "Vt": ctx.empty((spin * nk, n, n), np.complex128), "rho": ctx.empty((spin * nk, n, n), np.complex128),
              "rhoR": ctx.empty((spin, nk, n * n), np.float64), "rec": d_rec,
              "basis": ctx.empty((spin, nk * n, nimp + nb), np.float64), "sigma": d_rec.offset(12, (spin, nb)),
              "iout": d_rec.offset(12 + spin * nb, (2,)), "mesh": mesh3(sysm.mesh),
              "nelec": float(mfd.check_nelec(spin * nk * n * sysm.filling, None)[0]), "views": {}}
        sysm.__dict__["_small_ws"] = ws
    d_w, d_occ, d_rhoR, d_rec, d_basis_buf = ws["w"], ws["occ"], ws["rhoR"], ws["rec"], ws["basis"]
    handled = C.c_int(0)
    ctx.check(lib.dmk_small_meanfield(ctx.h, ws["mesh"], n, spin, sysm.d_Fock_k.ptr, sysm.d_vcor.ptr if sysm.d_vcor is not None else None,
                                      nk, ws["nelec"], float("inf"), 0.0, 0, 1e-6, 1e-12, d_w.ptr, d_occ.ptr, ws["Vt"].ptr, ws["rho"].ptr,
                                      d_rhoR.ptr, d_rec.ptr, C.byref(handled)))
    if not handled.value:
        return None
    ctx.check(lib.dmk_small_bath(ctx.h, ws["mesh"], n, spin, d_rhoR.ptr, nk * n * n, sysm.d_env.ptr, nenv, sysm.d_col.ptr, nb,
                                 sysm.d_virt.ptr, 1, sysm.d_imp.ptr, nimp, nk * n, float(tol_bath), ws["sigma"].ptr, None, d_basis_buf.ptr,
                                 ws["iout"].ptr, C.byref(handled)))
    if not handled.value:
        return None
    rec = d_rec.get()                                   # the ONE synchronising read-back of the step
    info, sig = rec[:12], rec[12:12 + spin * nb].reshape(spin, nb)
    iout = rec[12 + spin * nb:].view(np.int32)
    if info[4] != 0.0 or info[6] != 0.0 or iout[1 + spin] != 0:
        raise RuntimeError("small-lattice step failed: occupation status %g, eigensolver flag %g, SVD flag %d"
                           % (info[4], info[6], int(iout[1 + spin])))
    nemb = int(iout[0])
    d_basis = ws["views"].get(nemb)
    if d_basis is None:
        d_basis = ws["views"][nemb] = ctx.wrap(d_basis_buf.address, (spin, nk * n, nemb), np.float64, keepalive=d_basis_buf)
    timers["small_step"] = timers.get("small_step", 0.0) + (time.perf_counter() - t)
    mf = {"mu": float(info[0]), "ew": d_w, "occ": d_occ, "nerr": float(info[1]), "imag_max": float(info[5]), "jacobi_sweeps": int(info[7]),
          "phase_us": [float(x) for x in info[8:12]]}
    return d_rhoR, mf, d_basis, nemb, [sig[s] for s in range(spin)]


def c_ao_emb_stage(ctx, sysm, d_basis, nemb, timers=None, return_basis_k=False):
    timers = {} if timers is None else timers
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    t = time.perf_counter()
    d_bk = fourier.fold_R2k_dev(d_basis.reshape(spin, nk, n * nemb), sysm.mesh, spin, n * nemb)
    d_C = bgemm_dev(ctx, "N", "N", n, nemb, n, spin * nk, sysm.d_C_ao_lo, n * n, d_bk, n * nemb,
                    alpha=1.0 / (nk ** 0.75)).reshape(spin, nk, n, nemb)
    _stage(ctx, timers, "c_ao_emb", t)
    return (d_C, d_bk) if return_basis_k else d_C     # the embedding-Hamiltonian stage folds with the same basis_k


def emb_ham_stage(ctx, sysm, d_basis, nemb, d_rhoR, eri_dev, timers=None, d_bk=None, eri_rows=None):
    """One-body part of the embedding Hamiltonian (slater.py:525-606, interacting bath, HF):
    H1 = basis^H fock basis - JK_emb(rdm1_emb, ERI), JK_core = H1 - hcore_emb.  The one-body folds are replicated (every
    rank holds rho_R and the basis).  `eri_rows` = ownership table of a ROW-SHARDED ERI (dist.reduce_eri_bands): every rank
    streams only the pair rows it owns and the n x n partial J / K are summed over ranks; None = the whole ERI is local.
    Returns host (spin, nemb, nemb) arrays."""
    timers = {} if timers is None else timers
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    t = time.perf_counter()
    if d_bk is None:
        d_bk = fourier.fold_R2k_dev(d_basis.reshape(spin, nk, n * nemb), sysm.mesh, spin, n * nemb)
    d_rho_k = fourier.fold_R2k_dev(d_rhoR.reshape(spin, nk, n * n), sysm.mesh, spin, n * n)

    def fold(d_op_k):
        """(spin, nemb, nemb) real:  (1/nk) Re sum_k B_k^H op_k B_k."""
        d_T = bgemm_dev(ctx, "N", "N", n, nemb, n, spin * nk, d_op_k, n * n, d_bk, n * nemb)
        d_R = bgemm_dev(ctx, "C", "N", nemb, nemb, nk * n, spin, d_bk, nk * n * nemb, d_T, nk * n * nemb, alpha=1.0 / nk)
        return np.ascontiguousarray(d_R.get().reshape(spin, nemb, nemb).real)

    fock_emb = fold(sysm.d_Fock_k)
    rdm1_emb = fold(d_rho_k)
    hcore_emb = sysm.hcore_scale * fock_emb
    t = _stage(ctx, timers, "emb_h1", t)
    npair = nemb * (nemb + 1) // 2
    blk = lambda b: eri_dev.offset(b * npair * npair, (npair, npair))
    mine = None if eri_rows is None else dist.owned_ranges(eri_rows)
    if spin == 1:
        d_dm = ctx.to_device(2.0 * rdm1_emb[0])                         # restricted: spin-traced density (slater.py:481)
        vj, _, vk = scf.jk_dev(ctx, nemb, blk(0), d_dm, None, d_dm, row_ranges=mine)
        veff = (vj.get() - 0.5 * vk.get())[None]
    else:
        d_dm = ctx.to_device(rdm1_emb)
        # the transform leaves the blocks in (aa, ab, bb) order (eri_transform.py:465-467)
        (vj_s, vj_x), vk = scf.jk_blocks_dev(ctx, nemb, blk(0), blk(2), blk(1), d_dm, row_ranges=mine)
        vj = np.asarray([vj_s[0].get() + vj_x[0].get(), vj_s[1].get() + vj_x[1].get()])
        veff = vj - np.asarray([vk[0].get(), vk[1].get()])
    if mine is not None:
        veff = dist.all_reduce_sum_numpy(veff)                          # (spin, nemb, nemb): the only J / K data on the wire
    H1 = fock_emb - veff
    _stage(ctx, timers, "emb_jk", t)
    return {"H1": H1, "JK_core": H1 - hcore_emb, "rdm1_emb": rdm1_emb, "veff": veff, "fock_emb": fock_emb}


def vcor_fit_stage(ctx, sysm, d_basis, nemb, rdm1_emb, MaxIter=5, beta=np.inf, scale=0.02, seed=77, gtol=1e-6, ytol=1e-10,
                   dx_tol=1e-9, shard=None):
    """Correlation-potential fit in the embedding space (routine/slater.py:909-1329) on the synthetic system.
    The potential is VcorLocal on the valence orbitals (C5: 56 -> 3192 parameters).  The target density is the
    embedded mean-field density of a hidden, seeded parameter vector p_true (it stands in for the impurity solver's
    density and makes the fit a round trip: the error must fall towards zero and the parameters towards p_true).
    The stopping tolerances are TIGHTER than the reference's defaults (gtol 1e-3, ytol 1e-7, dx_tol 1e-7, fit.py:59): at
    those the synthetic problem stops after 5 gradient evaluations with the error barely changed, which measures the cost
    of 5 iterations and not of a fit; with these the CG runs until the density error has dropped by orders of magnitude
    (the returned dict says how far).  Returns timings per evaluation.  Collective over the ranks of an initialised process
    group: the dV_dparam table is sharded row-wise (slater.EmbFitDevice), the nemb x nemb algebra is replicated."""
    from libdmet_preview_amd.dmet import Hubbard
    from libdmet_preview_amd.system.lattice import Lattice
    n, nk, spin = sysm.nlo, sysm.nk, sysm.spin
    L = Lattice(n, sysm.mesh)
    L.val_idx, L.virt_idx, L.core_idx = list(sysm.val_idx), [i for i in range(n) if i not in sysm.val_idx], []
    Fk = sysm.d_Fock_k.get().reshape(spin, nk, n, n)
    L.fock_lo_k = L.hcore_lo_k = Fk if spin == 2 else Fk[0]
    basis = d_basis.get().reshape(spin, nk, n, nemb)
    # the embedded electron number of the synthetic system is whatever the mean field put there
    ne = [int(round(np.trace(rdm1_emb[s]))) for s in range(spin)]
    nelec = ne[0] if spin == 1 else ne
    v = Hubbard.VcorLocal(spin == 1, False, n, idx_range=sysm.val_idx)
    rng = np.random.default_rng(seed)
    p_true = scale * rng.standard_normal(v.length())
    gen = slater.EmbFitDevice(ctx, np.zeros((spin, nemb, nemb)), L, basis, v, beta, nelec, list(range(nemb)), [],
                              Fk, L.get_ovlp(kspace=True))
    gen.errfunc(p_true)
    target = gen.d_rho.get().reshape(spin, nemb, nemb)
    del gen
    # (1) the reference's own stopping rules (fit.py:59: gtol 1e-3, ytol 1e-7, dx_tol 1e-7): what a DMET iteration would pay
    ctx.sync()
    t0 = time.perf_counter()
    v_ref = Hubbard.VcorLocal(spin == 1, False, n, idx_range=sysm.val_idx)
    # every rank of the bench runs this stage: the table is sharded over them (FitVcorEmb(shard=True) is a collective)
    from libdmet_preview_amd.parallel import dist as _dist
    if shard is None:
        shard = _dist.is_initialized() and _dist.world_size() > 1
    v_ref, e0_ref, e1_ref = slater.FitVcorEmb(target, L, basis, v_ref, beta, MaxIter=MaxIter, nelec=nelec, shard=shard)
    ctx.sync()
    t_ref = time.perf_counter() - t0
    fit_ref = slater.FitVcorEmb.last_fit
    ref_counts = (int(fit_ref.nfev), int(fit_ref.ngev))
    p_ref = v_ref.param.copy()
    del fit_ref
    # (2) run to convergence
    ctx.sync()
    t0 = time.perf_counter()
    v, e0, e1 = slater.FitVcorEmb(target, L, basis, v, beta, MaxIter=MaxIter, nelec=nelec, gtol=gtol, ytol=ytol, dx_tol=dx_tol,
                                  shard=shard)
    ctx.sync()
    t_total = time.perf_counter() - t0
    fit = slater.FitVcorEmb.last_fit
    p = v.param.copy()
    reps = 3
    ctx.sync()
    t = time.perf_counter()
    for r in range(reps):
        fit.errfunc(p + 1e-9 * (r + 1))
    ctx.sync()
    t_err = (time.perf_counter() - t) / reps
    t = time.perf_counter()
    for r in range(reps):
        fit.gradfunc(p + 1e-9 * (r + 11))
    ctx.sync()
    t_grad = (time.perf_counter() - t) / reps
    return {"nparam": int(v.length()), "nemb": int(nemb), "MaxIter": int(MaxIter), "err_begin": float(e0), "err_end": float(e1),
            "param_err_begin": float(np.abs(p_true).max()), "param_err_end": float(np.abs(p - p_true).max()),
            "seconds_total": t_total, "objective_evals": int(fit.nfev), "gradient_evals": int(fit.ngev),
            "fused_objective_calls": int(getattr(fit, "fused_calls", 0)), "fused_objective_fallbacks": int(getattr(fit, "fused_fallbacks", 0)),
            "table_passes_saved": int(getattr(fit, "table_passes_saved", 0)), "on_ray_hits": list(getattr(fit, "on_ray_hits", [])),
            "refinement_settle_pass_histogram": {str(k): int(n) for k, n in sorted(getattr(fit, "settle_hist", {}).items())},
            "reference_tolerances": {"seconds_total": t_ref, "objective_evals": ref_counts[0], "gradient_evals": ref_counts[1],
                                     "err_end": float(e1_ref), "param_err_end": float(np.abs(p_ref - p_true).max()),
                                     "note": "UNCONVERGED: at the reference's default stopping rules this synthetic problem stops after "
                                             "%d gradient evaluations with the error barely moved; it measures the cost of that many "
                                             "evaluations, not of a fit, and is not part of any headline key" % ref_counts[1]},
            "table_rows_per_rank": int(fit.nloc), "ranks": int(dist.world_size()),
            "ms_per_objective": 1e3 * t_err, "ms_per_objective_plus_gradient": 1e3 * t_grad,
            "dV_dparam_bytes": int(fit.d_dV.nbytes), "vcor": v,
            "err_reduction": float(e0 / max(e1, 1e-300)),
            "param_err_reduction": float(np.abs(p_true).max() / max(np.abs(p - p_true).max(), 1e-300)),
            "tolerances": {"gtol": gtol, "ytol": ytol, "dx_tol": dx_tol, "reference_defaults": {"gtol": 1e-3, "ytol": 1e-7, "dx_tol": 1e-7}},
            "note": "FitVcorEmb, VcorLocal on the valence orbitals, CG with analytic gradient; one objective = one pass over dV_dparam "
                    "+ one eigh(nemb) per spin + nemb^3 algebra; objective + gradient = two passes"}


def eri_stage(ctx, sysm, d_C, nemb, eri_dev, kL_list=None, timers=None, max_blocks_per_kL=None, exchange=None, probe=None):
    """DF half transform + contraction over this rank's kL shard.  The planes of the shard stay resident (as many kL as the
    DMK_ERI_STACK_GB budget holds) and are contracted together.  `exchange`: None (local result), "allreduce" (every rank gets
    the whole sum) or "row_sharded" (finished bands of pair rows are reduced to their owners underneath the remaining
    contraction, dist.reduce_eri_bands).  `probe` = (d_x, d_yref): Freivalds probe of the contraction (EriEngine.set_probe).  Returns (nblocks, flops_half, flops_contract, ownership table or None)."""
    timers = {} if timers is None else timers
    t = time.perf_counter()
    # iteration-invariant step-2 planes: the impurity columns of C_ao_emb come first and do not change between iterations.  The
    # tests below only avoid a cache that could never hit; what makes a hit legal is the library's bitwise compare of the columns
    # (DMK_ERI_INV=0: the dense step 2 of every call, the A/B switch; DMK_ERI_INV_BLOCK=0: the planes are cached, but the
    # contraction computes every tile of the result on every call)
    inv = None
    if os.environ.get("DMK_ERI_INV", "1") != "0":
        inv = getattr(sysm, "eri_inv_cache", None)
        nimp = len(sysm.imp_idx)
        if inv is None and ((nemb == 256 and nimp >= 192) or (nemb != 256 and nimp >= 16)):
            inv = sysm.eri_inv_cache = et.EriInvariantCache(ctx)
    # split step 1: asked for exactly where the cache above could exist -- a provider with a token and 192 impurity
    # columns -- with or without DMK_ERI_INV, so the uncached A/B run sums in the order of the cached ones; a caller that can never
    # go warm never pays the dense surcharge.  DMK_ERI_SPLIT1=0: the old order.  The strip order (K6m) rides on the same rule;
    # DMK_ERI_STRIP=0 keeps K6l's
    srcs = [p for p in (sysm.df, getattr(sysm, "df_resident", None)) if p is not None]
    split1 = et.split_step1_wanted(nemb, any(getattr(p, "df_token", None) is not None for p in srcs), len(sysm.imp_idx))
    eng = et.EriEngine(ctx, sysm.mesh, sysm.nao, sysm.naux, nemb, sysm.spin, d_C, eri_dev, True, inv_cache=inv,
                       inv_cols=len(sysm.imp_idx), inv_block=os.environ.get("DMK_ERI_INV_BLOCK", "1") != "0", split_step1=split1,
                       strip_step1=et.strip_step1_wanted(split1))
    rows = None
    try:
        todo = eng.irreducible_kL() if kL_list is None else list(kL_list)
        eng.set_stack(n_kL=len(todo))
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        nblk = 0
        res = getattr(sysm, "df_resident", None)
        for kL in todo:
            src = res if (res is not None and int(kL) in res.offset) else sysm.df
            nblk += eng.run_kL(kL, src, max_blocks=max_blocks_per_kL)
        fh, fc = eng.flops()
        if exchange == "row_sharded" and dist.is_initialized():
            npair = nemb * (nemb + 1) // 2
            rows = dist.reduce_eri_bands(eng, eri_dev, sysm.spin * (sysm.spin + 1) // 2, npair)
            _stage(ctx, timers, "eri", t)
        else:
            eng.contract()
            t = _stage(ctx, timers, "eri", t)
            if exchange == "allreduce" and dist.is_initialized():
                dist.all_reduce_sum_dev(eri_dev)
                _stage(ctx, timers, "allreduce_eri", t)
    finally:
        eng.close()
    return nblk, fh, fc, rows


def iteration(ctx, sysm, eri_dev=None, kL_list=None, timers=None, max_blocks_per_kL=None, allreduce_eri=True,
              emb_ham=True, eri_exchange=None, eri_probe=None):
    """One embedding-construction pass.  Returns a dict with the products and per-stage seconds.  `eri_exchange`: how the
    kL-sharded ERI is summed over ranks -- "allreduce" (default when `allreduce_eri`), "row_sharded" or "none"."""
    if eri_exchange is None:
        eri_exchange = "allreduce" if allreduce_eri else "none"
    timers = {} if timers is None else timers
    small = small_lattice_stages(ctx, sysm, timers)
    if small is not None:
        d_rhoR, mf, d_basis, nemb, sigmas = small
    else:
        d_rhoR, mf = mean_field_stage(ctx, sysm, timers)
        d_basis, nemb, sigmas = bath_stage(ctx, sysm, d_rhoR, timers)
    out = {"rho_R": d_rhoR, "basis": d_basis, "nemb": nemb, "sigma": sigmas, "mu": mf["mu"], "ew": mf["ew"], "occ": mf["occ"],
           "timers": timers, "jacobi_sweeps": mf.get("jacobi_sweeps"), "small_phase_us": mf.get("phase_us")}
    if sysm.naux > 0:
        d_C, d_bk = c_ao_emb_stage(ctx, sysm, d_basis, nemb, timers, return_basis_k=True)
        npair = nemb * (nemb + 1) // 2
        spin_pair = sysm.spin * (sysm.spin + 1) // 2
        if eri_dev is None:
            eri_dev = ctx.zeros((spin_pair, npair, npair), np.float64)
        nblk, fh, fc, rows = eri_stage(ctx, sysm, d_C, nemb, eri_dev, kL_list, timers, max_blocks_per_kL,
                                       exchange=None if eri_exchange == "none" else eri_exchange, probe=eri_probe)
        out.update({"C_ao_emb": d_C, "eri": eri_dev, "nblocks": nblk, "flops_half": fh, "flops_contract": fc, "eri_rows": rows})
        if emb_ham:
            out["emb_ham"] = emb_ham_stage(ctx, sysm, d_basis, nemb, d_rhoR, eri_dev, timers, d_bk=d_bk, eri_rows=rows)
    return out
