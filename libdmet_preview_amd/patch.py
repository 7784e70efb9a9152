"""
Rebinding of the reference's entry points to this package.

The reference has no plugin interface: its hot-path callables are plain module attributes, and several callers bind
them BY NAME at import time (`from ...eri_transform import get_emb_eri` in routine/slater.py:32-33,
`from libdmet.routine.mfd import HF` in dmet/HubPhSymm.py:22, the star import of `fourier` in system/lattice.py:23),
so the defining module AND every importing module's copy have to be replaced.  `install()` does exactly that from
the table below and returns a handle `uninstall()` undoes; nothing here computes anything.

    import libdmet_preview_amd.patch as hip
    handle = hip.install()            # after `import libdmet`, before building Lattice objects
    ...
    hip.uninstall(handle)

`install` raises if the HIP library cannot be loaded (there is no CPU fallback to bind) and, with `strict=True`
(default), if a name of the table is missing on the reference side -- a renamed entry point must not be skipped
silently.
"""
import importlib

# (our module, [reference modules that hold a copy], [names])  -- reference file:line of every import-time binding
_FUNCTIONS = [
    # Lattice.k2R / R2k / FFTtoK / FFTtoT resolve these from the module globals (system/lattice.py:23 star import)
    ("system.fourier", ["system.fourier", "system.lattice"], ["FFTtoK", "FFTtoT", "k2R", "R2k"]),
    # HF() looks the diagonalisers up in its own module globals (routine/mfd.py:283-298)
    ("routine.mfd", ["routine.mfd"],
     ["DiagRHF", "DiagUHF", "DiagRHF_symm", "DiagUHF_symm", "DiagGHF", "DiagGHF_symm", "DiagBdG", "DiagBdGsymm",
      "assignocc"]),
    # AO -> LO -> EO basis products (basis_transform/__init__.py star import; eri_transform.py:27)
    ("basis_transform.make_basis", ["basis_transform.make_basis", "basis_transform"],
     ["multiply_basis", "transform_h1_to_lo", "transform_rdm1_to_lo", "transform_rdm1_to_ao"]),
    ("basis_transform.make_basis", ["basis_transform.eri_transform"], ["multiply_basis"]),
    # Schmidt bath; called as slater.embBasis (dmet/HubPhSymm.py:77)
    ("routine.slater", ["routine.slater"],
     ["get_emb_basis", "embBasis", "get_emb_Ham", "embHam", "transform_h1", "foldRho", "foldRho_k", "get_veff",
      "get_dV_dparam", "FitVcorEmb", "FitVcorFull", "FitVcorTwoStep"]),
    # the ERI transform; routine/slater.py:32-33 holds its own copy.  The rebound functions take the reference's own
    # argument -- a pyscf.pbc.df.GDF object (`_cderi` path / container, `kpts`, `cell`) -- and adapt it themselves
    # (eri_transform.resolve_df); `use_mpi=True` goes to this package's eri_transform_mpi twin with the reference's
    # (cell, cderi, kpts=...) hand-over (eri_transform.py:76-87), so libdmet.basis_transform.eri_transform_mpi (which needs
    # mpi4pyscf to import at all) is never touched
    ("basis_transform.eri_transform", ["basis_transform.eri_transform", "basis_transform", "routine.slater"],
     ["get_emb_eri", "get_unit_eri"]),
    # spinless.py:518-538 imports get_emb_eri_gso lazily from the module; cderi layout helpers
    ("basis_transform.eri_transform", ["basis_transform.eri_transform"],
     ["get_emb_eri_gso", "get_mask_kptij_lst", "transform_gdf_to_lo", "convert_eri_to_gdf", "eri_restore", "get_emb_eri_fast_gdf",
      "transform_ao_to_emb", "_Lij_s4_to_eri", "get_basis_k", "get_weights_t_reversal"]),
    # J / K on the resident ERI (routine/slater.py:30 imports them by name)
    ("solver.scf", ["solver.scf", "routine.slater"], ["_get_jk", "_get_veff"]),
    ("solver.scf", ["solver.scf", "routine.spinless"], ["_get_veff_ghf"]),          # routine/spinless.py:28 imports it by name
    # Hartree-Fock without PySCF (solver/scf_solver.py builds its scfsolver as scf.SCF(...), an attribute lookup at call time)
    ("solver.scf", ["solver.scf"], ["SCF"]),
    # the MO integral transform: the correlated solvers of the reference call these as scf.incore_transform /
    # scf.ao2mo_Ham, attribute lookups at call time
    ("solver.scf", ["solver.scf"], ["incore_transform", "ao2mo_Ham"]),
    # one-body folds (routine/slater.py:35 star-imports slater_helper)
    ("routine.slater_helper", ["routine.slater_helper", "routine.slater"],
     ["transform_trans_inv", "transform_trans_inv_k", "transform_local", "transform_imp", "transform_imp_env",
      "transform_4idx", "transform_eri_local", "unit2emb"]),
    # round 6: the idempotent projection and the active-space projector of the fit, the finite-T single-matrix mean field and its
    # response formulas, the Cholesky vectors behind convert_eri_to_gdf
    ("routine.slater_helper", ["routine.slater_helper", "routine.slater"], ["get_rdm1_idem"]),
    ("routine.slater", ["routine.slater"], ["get_active_projector_full"]),
    # behind the solver: results, the democratic global density, the veff rebuild and the DMET energy Hamiltonian
    # (dmet/Hubbard.py:43-71 calls them as slater.*; routine/spinless.py:23 keeps its own copies of the two scalers: the GSO twin
    # is not built)
    ("routine.slater", ["routine.slater"],
     ["get_H1_scaled", "get_H2_scaled", "transformResults", "get_veff_from_rdm1_emb", "get_H_dmet", "get_E_dmet", "get_E_dmet_HF",
      "get_H1_dmet"]),
    ("routine.slater_helper", ["routine.slater_helper", "routine.slater"],
     ["get_emb_basis_other_cell", "get_rho_glob_R", "get_rho_glob_k", "get_rho_glob_full"]),
    ("routine.ftsystem", ["routine.ftsystem"], ["kernel", "make_rdm1", "get_rho_grad", "get_dw_dv"]),
    ("utils.cholesky", ["utils.cholesky"], ["modified_cholesky", "modified_cholesky_uhf", "get_cderi_rhf", "get_cderi_uhf"]),
    ("routine.localizer", ["routine.localizer"], ["localize_bath", "localize_bath_scdm"]),
    # the cell-resolved and the k-point-resolved potentials (dmet/Hubbard.py:1495-1497 re-exports them): the index-table classes the
    # device dV/dparam builder and the lattice-stage fit read without a dense (nparam, nblk, ncells, nlo, nlo) gradient
    ("routine.vcor", ["routine.vcor", "dmet.Hubbard"], ["VcorNonLocal", "VcorKpoints"]),
    ("dmet.Hubbard", ["dmet.Hubbard"], ["VcorRestricted", "VcorSymm", "VcorSymmSpin", "VcorSymmBogo"]),
    ("routine.vcor", ["routine.vcor"], ["get_kpts_map"]),
    # BCS twin (routine/bcs.py:13 star-imports bcs_helper)
    ("routine.bcs_helper", ["routine.bcs_helper", "routine.bcs"],
     ["contract_trans_inv", "transform_trans_inv", "contract_local", "transform_local", "transform_imp",
      "contract_imp_env", "transform_imp_env", "transform_local_grad", "get_dV_dparam"]),
    ("routine.bcs", ["routine.bcs"], ["embBasis", "get_emb_basis", "embHam", "get_emb_Ham", "FitVcorEmb", "FitVcorFull", "FitVcorFullK", "FitVcorTwoStep", "foldRho", "foldRho_k"]),
    # optimiser of the vcor fit (routine/slater.py:27 imports minimize by name)
    ("routine.fit", ["routine.fit", "routine.slater"], ["minimize"]),
    ("routine.spinless", ["routine.spinless"], ["get_emb_basis", "embBasis", "get_emb_basis_opt", "get_emb_Ham", "embHam", "foldRho_k", "get_dV_dparam", "FitVcorEmb", "get_dV_dparam_full", "FitVcorFull"]),
    # (FitVcorFull_mu and FitVcorTwoStep of the GSO twin stay the reference's: its convex `use_cvx_frac` branch is not built here)
    # the GSO one-body folds and ERI containers (routine/spinless.py:32 star-imports the helper module)
    ("routine.spinless_helper", ["routine.spinless_helper", "routine.spinless"],
     ["unit2emb", "transform_eri_local", "transform_trans_inv_k", "transform_local", "transform_imp", "get_H2_mask"]),
    ("dmet.HubPhSymm", ["dmet.HubPhSymm"], ["basisMatching", "VcorLocalPhSymm", "VcorDCAPhSymm", "InitGuess", "HartreeFock", "FitVcor"]),
    # driver layer: dmet/Hubbard.py:8 star-imports HubPhSymm, so it holds its own ConstructImpHam; it defines the RHF / UHF
    # HartreeFock wrapper (:14-41) and FitVcor (:1503) itself
    ("dmet.HubPhSymm", ["dmet.HubPhSymm", "dmet.Hubbard"], ["ConstructImpHam"]),
    # (apply_dmu is NOT rebound: dmet/HubbardBCS.py:104 and HubbardGSO.py:134 overwrite Hubbard.apply_dmu at import; the
    # reference's versions reach the device through the rebound transform_imp helpers)
    ("dmet.Hubbard", ["dmet.Hubbard"], ["HartreeFock", "RHartreeFock", "FitVcor"]),
    # the BCS driver layer (dmet/HubbardBCS.py:9-112) and the root search under its chemical-potential fit
    ("dmet.HubbardBCS", ["dmet.HubbardBCS"], ["HartreeFockBogoliubov", "ConstructImpHam"]),
    ("routine.bcs_helper", ["routine.bcs_helper", "routine.bcs", "dmet.HubbardBCS"], ["mono_fit"]),
    # the GSO driver layer (dmet/HubbardGSO.py:16-134); mono_fit / mono_fit_2 reach it through spinless_helper's star import
    ("dmet.HubbardGSO", ["dmet.HubbardGSO"], ["GHartreeFock", "ConstructImpHam"]),
    ("routine.bcs_helper", ["routine.bcs_helper", "routine.spinless_helper", "dmet.HubbardGSO"], ["mono_fit_2"]),
    # Loewdin orthogonalisation (routine/slater.py imports lo.lowdin's vec_lowdin by name)
    ("lo.lowdin", ["lo.lowdin"], ["_lowdin", "_vec_lowdin", "vec_lowdin", "vec_lowdin_k"]),
    ("lo.lowdin", ["routine.slater"], ["vec_lowdin"]),
]
# methods of the reference's Lattice replaced by ours (they only touch duck-typed attributes; system/lattice.py:416-673)
_LATTICE_METHODS = ["set_Ham", "setHam", "set_Ham_model", "setHam_model", "update_Ham", "transform_obj_to_lo"]
# HF itself: dmet/HubPhSymm.py:22 binds it by name, dmet/Hubbard.py:9 star-imports that module
_HF_HOLDERS = ["routine.mfd", "dmet.HubPhSymm", "dmet.Hubbard"]
# HFB: routine/bcs.py:15 and dmet/HubbardBCS.py:6 import it by name
_HFB_HOLDERS = ["routine.mfd", "routine.bcs", "dmet.HubbardBCS"]
# GHF: dmet/HubbardGSO.py imports it by name
_GHF_HOLDERS = ["routine.mfd", "dmet.HubbardGSO"]


def binding_table():
    """The rebinding plan as (our dotted module, reference dotted module, attribute) triples."""
    out = []
    for ours, refs, names in _FUNCTIONS:
        for r in refs:
            for n in names:
                out.append((ours, r, n))
    for r in _HF_HOLDERS:
        out.append(("routine.mfd", r, "HF"))
    for r in _HFB_HOLDERS:
        out.append(("routine.mfd", r, "HFB"))
    for r in _GHF_HOLDERS:
        out.append(("routine.mfd", r, "GHF"))
    return out


def install(reference_package="libdmet", replace_hf=True, strict=True, resident_df=None, invariant_planes=None):
    """Rebind the reference's hot-path entry points to the HIP implementations; returns the undo handle.
    `resident_df=True`: the DF tensor behind `lattice.df` is loaded into HBM by the first get_emb_eri of a run and read in place by
    every later one (eri_transform.RESIDENT_DF; as many kL as fit, the rest streamed as before) -- no change to the DMET script.
    `invariant_planes=True` (with `resident_df`): the impurity-only part of the step-2 planes is kept next to the resident tensor and
    reused by every later transform whose leading C_ao_emb columns are bit-identical (eri_transform.INVARIANT_PLANES): at
    nemb = 256 the region of the specialised kernel (192 columns), at any other embedding dimension the pairs below
    A = 16 floor(nimp / 16), where nimp is read off a `basis=` of the form [I_imp | bath] (the `C_ao_eo=` entry stays dense).
    With the planes the invariant block of the RESULT follows (EriEngine(inv_block=True)): the stacked contraction leaves the tiles
    of the impurity-only pair prefix out and copies their kept sum back."""
    from libdmet_preview_amd import _lib          # noqa: F401 -- loading libdmetk.so fails loudly here if it is missing
    undo = []

    def bind(ref_mod, name, value):
        if not hasattr(ref_mod, name):
            if strict:
                raise AttributeError("%s has no attribute %s to rebind" % (ref_mod.__name__, name))
            return
        undo.append((ref_mod, name, getattr(ref_mod, name)))
        setattr(ref_mod, name, value)

    for ours, ref, name in binding_table():
        if name in ("HF", "HFB", "GHF") and not replace_hf:
            continue
        mine = importlib.import_module("libdmet_preview_amd." + ours)
        bind(importlib.import_module(reference_package + "." + ref), name, getattr(mine, name))
    ref_lat = importlib.import_module(reference_package + ".system.lattice")
    from libdmet_preview_amd.system import lattice as my_lat
    for name in _LATTICE_METHODS:
        bind(ref_lat.Lattice, name, getattr(my_lat.Lattice, name))
    if resident_df is not None:
        from libdmet_preview_amd.basis_transform import eri_transform as my_et
        undo.append((my_et, "RESIDENT_DF", my_et.RESIDENT_DF))
        my_et.RESIDENT_DF = bool(resident_df)
    if invariant_planes is not None:
        from libdmet_preview_amd.basis_transform import eri_transform as my_et
        undo.append((my_et, "INVARIANT_PLANES", my_et.INVARIANT_PLANES))
        my_et.INVARIANT_PLANES = bool(invariant_planes)
    return undo


def uninstall(handle):
    for obj, name, old in reversed(handle):
        setattr(obj, name, old)
    del handle[:]
