"""
Density-fitted k-point J/K build on the device (routine/pbc_helper.py get_jk_gdf / DeviceJK, the dmk_dfjk_* ABI, the
Lattice.set_Ham fallback) against the numpy restatement tests/dfjk_ref.py and, for G39, the reference's own results.

Gate: max |x - ref| <= 1e-10 max |ref| on vj and vk -- the project's standing bound for FP64 stages.  The sums here are shorter
than 1e4 terms, so correct code sits orders of magnitude below it.  The shapes are the smallest at which the kernels take another
path: off every tile (nao 19, naux 11), one past the 64 / 128 output tiles (nao 129), a single auxiliary row, and a split-K
launch with several chunks and a remainder (naux 7 -> chunks of 2, 2, 3 rows).
"""
import ctypes as C
import functools
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dfjk_ref
from tests.test_dfjk_oracle import load_g39

TOL = 1e-10
SHAPES = {"off_tile": ((2, 2, 1), 19, 11), "past_tile": ((2, 1, 1), 129, 3), "naux1": ((2, 1, 1), 16, 1), "split_k": ((5, 1, 1), 24, 7)}


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _cell_kpts(mesh, nao):
    from libdmet_preview_amd.system import fourier, lattice
    cell = lattice._UnitCell(nao)
    return cell, cell.get_abs_kpts(fourier.make_kpts_scaled(list(mesh)))


def _close(name, got, ref):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print("%s: max |x - ref| / max |ref| = %.3e" % (name, err / scale))
    assert got.shape == ref.shape
    assert err <= TOL * scale, (name, err / scale)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs with the pair relation and time-reversal symmetry, and the restatement's J / K of them (computed once)."""
    from libdmet_preview_amd.system import fourier
    mesh, nao, naux = SHAPES[name]
    ks, blocks = dfjk_ref.stripe_blocks(mesh, nao, naux, seed=len(name))
    assert np.abs(ks - fourier.make_kpts_scaled(list(mesh))).max() < 1e-14
    dm = dfjk_ref.stripe_density(mesh, nao, 2, seed=7 + len(name))
    vj, vk = dfjk_ref.get_jk(lambda i, j: blocks[(i, j)], dm)
    for a in (dm, vj, vk):
        a.setflags(write=False)
    return mesh, nao, naux, blocks, dm, vj, vk


def _mem(name):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    mesh, nao, naux, blocks, dm, vj, vk = _case(name)
    cell, kpts = _cell_kpts(mesh, nao)
    return cell, et.GDFMemory(kpts, blocks, naux=naux), dm, vj, vk


@pytest.mark.parametrize("tag", ["rhf", "uhf"])
def test_g39_matches_reference(ctx, golden, tag):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    from libdmet_preview_amd.routine import pbc_helper
    g = golden("G39_dfjk.npz")
    nk, blocks = load_g39(g)
    cell, kpts = _cell_kpts(tuple(g["mesh"]), int(g["nao"]))
    df = et.GDFMemory(kpts, blocks, naux=int(g["naux"]))
    dm, rj, rk = g["dm_" + tag], g["vj_" + tag], g["vk_" + tag]
    vj, vk = pbc_helper.get_jk_gdf(cell, df, dm)
    _close("G39 %s vj" % tag, vj, rj)
    _close("G39 %s vk" % tag, vk, rk)
    vj1, none = pbc_helper.get_jk_gdf(cell, df, dm, with_k=False)
    assert none is None
    _close("G39 %s vj only" % tag, vj1, rj)
    none, vk1 = pbc_helper.get_jk_gdf(cell, df, dm, with_j=False)
    assert none is None
    _close("G39 %s vk only" % tag, vk1, rk)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_full_time_reversal_determinism(ctx, name):
    from libdmet_preview_amd.routine import pbc_helper
    from libdmet_preview_amd.system import fourier
    cell, df, dm, rj, rk = _mem(name)
    vj, vk = pbc_helper.get_jk_gdf(cell, df, dm)
    _close(name + " vj", vj, rj)
    _close(name + " vk", vk, rk)
    vj2, vk2 = pbc_helper.get_jk_gdf(cell, df, dm)
    assert np.array_equal(vj, vj2) and np.array_equal(vk, vk2)            # same call, same bits
    tj, tk = pbc_helper.get_jk_gdf(cell, df, dm, t_reversal_symm=True)
    _close(name + " vj (time reversal)", tj, rj)
    _close(name + " vk (time reversal)", tk, rk)
    _close(name + " vj (time reversal vs full)", tj, vj)
    _close(name + " vk (time reversal vs full)", tk, vk)
    neg = fourier.kmesh_tables(list(SHAPES[name][0]))[1]
    assert np.array_equal(tk[:, neg], tk.conj()) and np.array_equal(tj[:, neg], tj.conj())
    # a single spin channel of the same density, 3-index in and out
    sj, sk = pbc_helper.get_jk_gdf(cell, df, dm[0])
    assert sj.shape == dm[0].shape
    _close(name + " vj (3-index)", sj, dfjk_ref.get_jk(df.get_block, dm[0], with_k=False)[0])
    _close(name + " vk (3-index)", sk, rk[0])


def test_providers(ctx):
    """A tensor generated on the device (ring, no host copy), the same blocks fed from the host, and the blocks resident in HBM."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    from libdmet_preview_amd.routine import pbc_helper
    mesh, nao, naux = (3, 1, 1), 24, 5
    cell, kpts = _cell_kpts(mesh, nao)
    nk = len(kpts)
    phil = et.GDFPhilox(kpts, naux, nao, seed=39)
    buf = ctx.empty((naux, nao, nao), np.complex128)
    blocks = {}
    for i in range(nk):
        for j in range(nk):
            phil.load_block(ctx, i, j, buf)
            blocks[(i, j)] = buf.get()
    dm = dfjk_ref.stripe_density(mesh, nao, 2, seed=3)
    rj, rk = dfjk_ref.get_jk(lambda i, j: blocks[(i, j)], dm)
    pj, pk = pbc_helper.get_jk_gdf(cell, phil, dm)
    _close("philox vj", pj, rj)
    _close("philox vk", pk, rk)
    mj, mk = pbc_helper.get_jk_gdf(cell, et.GDFMemory(kpts, blocks, naux=naux), dm)
    _close("host-fed vs philox vj", mj, pj)
    _close("host-fed vs philox vk", mk, pk)
    res = et.GDFResident(ctx, phil, list(mesh), nao, naux, t_reversal_symm=False)
    try:
        assert res.nblocks == nk * nk
        qj, qk = pbc_helper.get_jk_gdf(cell, res, dm)
    finally:
        res.free()
    assert np.array_equal(qj, pj) and np.array_equal(qk, pk)


def test_ewald(ctx):
    from libdmet_preview_amd.routine import pbc_helper
    cell, df, dm, rj, rk = _mem("off_tile")
    mesh, nao, naux = SHAPES["off_tile"]
    S = dfjk_ref.stripe_density(mesh, nao, 1, seed=11)[0]
    S = np.einsum("kpq,krq->kpr", S, S.conj()) + np.eye(nao)[None]          # Hermitian positive
    mad = 0.37
    ej, ek = dfjk_ref.get_jk(df.get_block, dm, madelung=mad, ovlp=S)
    assert np.abs(ek - rk).max() > 1e-3 * np.abs(rk).max()                   # the term is not negligible here
    vj, vk = pbc_helper.get_jk_gdf(cell, df, dm, exxdiv="ewald", madelung=mad, ovlp=S)
    _close("ewald vj", vj, ej)
    _close("ewald vk", vk, ek)
    tj, tk = pbc_helper.get_jk_gdf(cell, df, dm, exxdiv="ewald", madelung=mad, ovlp=S, t_reversal_symm=True)
    _close("ewald vk (time reversal)", tk, ek)
    with pytest.raises(ValueError):
        pbc_helper.get_jk_gdf(cell, df, dm, exxdiv="ewald", ovlp=S)
    with pytest.raises(NotImplementedError):
        pbc_helper.get_jk_gdf(cell, df, dm, exxdiv="vcut_sph")


def test_lattice_fallback_and_adapter(ctx):
    """Lattice.set_Ham / update_Ham without a mean-field object: J and K come from the DF tensor on the device."""
    from libdmet_preview_amd.routine import pbc_helper
    from libdmet_preview_amd.system.lattice import Lattice
    name = "off_tile"
    cell, df, dm2, _, _ = _mem(name)
    mesh, nao, naux = SHAPES[name]
    dm = np.ascontiguousarray(dm2[0])
    hcore = dfjk_ref.stripe_density(mesh, nao, 1, seed=21)[0]
    S = np.eye(nao)[None] + 0.05 * dfjk_ref.stripe_density(mesh, nao, 1, seed=22)[0]
    Cmat = np.eye(nao)[None] + 0.1 * dfjk_ref.stripe_density(mesh, nao, 1, seed=23)[0]
    rj, rk = dfjk_ref.get_jk(df.get_block, dm)

    def same(a, b):
        for k in ("fock_lo_k", "vhf_lo_k", "fock_lo_R"):
            _close(k, np.asarray(getattr(a, k)), np.asarray(getattr(b, k)))

    ref = Lattice(nao, mesh)
    ref.set_Ham(None, None, Cmat, ovlp=S, hcore=hcore, rdm1=dm, vj=rj, vk=rk)
    dev = Lattice(nao, mesh)
    dev.set_Ham(None, df, Cmat, ovlp=S, hcore=hcore, rdm1=dm)
    same(dev, ref)
    ada = Lattice(nao, mesh)
    ada.set_Ham(pbc_helper.DeviceJK(cell, df), None, Cmat, ovlp=S, hcore=hcore, rdm1=dm)
    same(ada, ref)
    with pytest.raises(ValueError):
        Lattice(nao, mesh).set_Ham(None, None, Cmat, ovlp=S, hcore=hcore, rdm1=dm)

    stripe = dev.k2R(dfjk_ref.stripe_density(mesh, nao, 1, seed=24)[0])
    dev.update_Ham(stripe)
    ada.update_Ham(stripe)
    new_dm = np.asarray(dev.rdm1_ao_k)
    assert new_dm.ndim == 3
    uj, uk = dfjk_ref.get_jk(df.get_block, new_dm)
    ref.update_Ham(stripe, vhf=uj - 0.5 * uk)
    same(dev, ref)
    same(ada, ref)

    jk = pbc_helper.DeviceJK(cell, df)
    with pytest.raises(NotImplementedError):
        jk.get_jk(dm_kpts=dm, kpts_band=jk.kpts[:1])
    with pytest.raises(NotImplementedError):
        jk.get_jk(dm_kpts=dm, kpts=jk.kpts + 0.01)
    vj, vk = jk.get_jk(dm_kpts=dm, kpts=jk.kpts, with_k=False)
    assert vk is None
    _close("adapter vj", vj, rj)


def test_abi_misuse(ctx):
    """Calls out of order and indices out of range are refused before anything is launched: the outputs keep the zeros of begin."""
    from libdmet_preview_amd._lib import lib
    nk, nao, naux = 2, 16, 2
    rng = np.random.default_rng(5)
    dm = ctx.to_device(rng.standard_normal((1, nk, nao, nao)) + 0j)
    blk = ctx.to_device(rng.standard_normal((naux, nao, nao)) + 0j)
    vj, vk = ctx.empty((1, nk, nao, nao), np.complex128), ctx.empty((1, nk, nao, nao), np.complex128)
    h = C.c_void_p()
    assert lib.dmk_dfjk_begin(ctx.h, nk, nao, naux, 1, 3, dm.ptr, vj.ptr, vk.ptr, C.byref(h)) == 0
    try:
        assert lib.dmk_dfjk_push_block(h, nk, 0, 0, blk.ptr) == -1             # DMK_ERR_INVALID: index outside [0, nk)
        assert lib.dmk_dfjk_push_block(h, 0, -1, 0, blk.ptr) == -1
        assert lib.dmk_dfjk_push_block(h, 0, 1, 1, blk.ptr) == -1              # Coulomb passes take diagonal blocks
        assert lib.dmk_dfjk_push_block(h, 0, 0, 7, blk.ptr) == -1
        assert lib.dmk_dfjk_push_block(h, 0, 0, 2, blk.ptr) == -5              # DMK_ERR_STATE: pass 2 before pass 1
        assert lib.dmk_dfjk_finish(h) == -5
        for k in range(nk):
            assert lib.dmk_dfjk_push_block(h, k, k, 1, blk.ptr) == 0
        assert lib.dmk_dfjk_finish(h) == -5                                     # finish before Coulomb pass 2
        assert lib.dmk_dfjk_push_block(h, 0, 0, 1, blk.ptr) == -5              # pass 1 twice
        ctx.sync()
        assert not vj.get().any() and not vk.get().any()
        for k in range(nk):
            assert lib.dmk_dfjk_push_block(h, k, k, 2, blk.ptr) == 0
        assert lib.dmk_dfjk_push_block(h, 0, 0, 0, blk.ptr) == 0
        assert lib.dmk_dfjk_finish(h) == -5                                     # row 0 has one of its two exchange blocks
        assert lib.dmk_dfjk_push_block(h, 0, 1, 0, blk.ptr) == 0
        assert lib.dmk_dfjk_finish(h) == 0
        assert lib.dmk_dfjk_finish(h) == -5
        assert lib.dmk_dfjk_push_block(h, 1, 0, 0, blk.ptr) == -5
        f = (C.c_double * 2)()
        assert lib.dmk_dfjk_flops(h, f) == 0 and f[0] > 0 and f[1] > 0
    finally:
        assert lib.dmk_dfjk_free(h) == 0
    big = C.c_void_p()
    assert lib.dmk_dfjk_begin(ctx.h, 1, 4096, 16, 1, 3, dm.ptr, vj.ptr, vk.ptr, C.byref(big)) == -1    # a 4 GiB block: refused
    assert not big.value
