"""
Device code behind the solver, run with -m gpu on an MI355X:

  dmk_dmet_h2_scaled   against the mask loops of tests/dmet_ham_ref.py, bit for bit (NaN compared as NaN only in the 1-fold form,
                       the one form whose rule lets a NaN without impurity index survive), its argument checks, and two cases with
                       more than 2^31 output elements
  dmk_rho_glob         and get_rho_glob_R / k / full against golden G41 (the reference) and the literal loop over cells
  the host layer       every G41 output of routine/slater.py's new functions, and the rebinding through a stand-in libdmet tree
  memory               twenty calls of each new entry point leave the free device memory where it was

Tolerances: 1e-10 max-abs for densities, one-body quantities and energies; the scaled ERIs are compared
with array_equal.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dfjk_ref, dmet_ham_ref as ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("uhf_231", (2, 3, 1)), ("rhf_411", (4, 1, 1)), ("uhf_222", (2, 2, 2))]
SYM_PAIRS = [(4, 4), (1, 4), (8, 4), (4, 1), (1, 1)]
DMK_ERR_INVALID = -1
TOL = 1e-10
SENTINEL = 777.0


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@pytest.fixture(scope="module")
def g41():
    return np.load(os.path.join(GOLD, "G41_dmet_ham.npz"))


@pytest.fixture(scope="module")
def g8():
    return np.load(os.path.join(GOLD, "G8_embham.npz"))


# ---- the scaling kernel ---------------------------------------------------------------------------------------------------------

def _rows(n, sym):
    return {1: n * n, 4: n * (n + 1) // 2}[sym]


def _planted_block(n, imp, seed):
    """A symmetric 4-fold block with a NaN in an element without impurity index and an Inf in one with two (where they exist)."""
    npair = _rows(n, 4)
    rng = np.random.default_rng(seed)
    e4 = rng.standard_normal((npair, npair))
    e4 = e4 + e4.T
    cls = ref.pair_classes(n, imp)
    c0, c1, c2 = (np.where(cls == c)[0] for c in range(3))
    if len(c0):
        e4[c0[-1], c0[-1]] = np.nan
    if len(c1):
        e4[c1[0], c1[0]] = np.inf
    elif len(c0) and len(c2):
        e4[c0[0], c2[0]] = e4[c2[0], c0[0]] = np.inf
    return e4


def _layout(e4, n, sym, ld):
    """The flat host buffer of the block in storage `sym` with pitch ld (padding = SENTINEL)."""
    if sym == 8:
        return ref.pack_s8(e4)
    body = e4 if sym == 4 else ref.restore_1(e4, n).reshape(n * n, n * n)
    buf = np.full((body.shape[0], ld), SENTINEL)
    buf[:, :body.shape[1]] = body
    return buf.reshape(-1)


def _call(ctx, n, imp, d_in, in_sym, ld_in, d_out, out_sym, ld_out):
    from libdmet_preview_amd._lib import lib
    imp = np.ascontiguousarray(imp, dtype=np.int32)
    return lib.dmk_dmet_h2_scaled(ctx.h, n, imp.ctypes.data if imp.size else None, int(imp.size), in_sym, d_in.ptr, ld_in, out_sym,
                                  d_out.ptr, ld_out)


def _same_bits(got, want, nan_survives):
    if not nan_survives:
        assert not np.isnan(want).any()
        return np.array_equal(got.view(np.int64), want.view(np.int64))           # (the sign of an assigned zero included)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.parametrize("n", [5, 16, 33])
@pytest.mark.parametrize("in_sym,out_sym", SYM_PAIRS)
def test_h2_scaled_matches_the_mask_loops(ctx, n, in_sym, out_sym):
    for imp in ([], list(range(n)), [0, 1, 2], [0, 2, n - 1]):
        e4 = _planted_block(n, imp, seed=100 * n + len(imp))
        for pad in (0, 3):
            ld_in = 0 if in_sym == 8 else _rows(n, in_sym) + pad
            ld_out = _rows(n, out_sym) + pad
            host_in = _layout(e4, n, in_sym, ld_in)
            want = ref.h2_scaled(host_in, n, imp, in_sym, out_sym, ld_in=ld_in or None, ld_out=ld_out, out_fill=SENTINEL)
            want = np.concatenate([want, np.full(_rows(n, out_sym) * ld_out - want.size, SENTINEL)])
            for in_place in ((False, True) if in_sym == out_sym else (False,)):
                d_in = ctx.to_device(host_in)
                d_out = d_in if in_place else ctx.to_device(np.full(want.size, SENTINEL))
                assert _call(ctx, n, imp, d_in, in_sym, ld_in, d_out, out_sym, ld_out) == 0
                got = d_out.get()
                assert _same_bits(got, want, nan_survives=(in_sym, out_sym) == (1, 1)), (n, imp, pad, in_place)
                if not in_place:
                    assert np.array_equal(d_in.get(), host_in, equal_nan=True)      # the input is only read


@pytest.mark.parametrize("n", [64, 70])
def test_h2_scaled_4_to_1_tiles(ctx, n):
    """The tiled 4 -> 1 kernel of even n: tiles above, below and on the diagonal and on the edge (n = 70 is no multiple of the
    32-wide tile), and an odd pitch of the input; pitch n^2 + 3 of the output takes the element-wise kernel instead."""
    imp = [0, 2, n - 1]
    e4 = _planted_block(n, imp, seed=n)
    npair, nn = _rows(n, 4), _rows(n, 1)
    for pad_in, pad_out in ((0, 0), (3, 2), (0, 3)):
        host_in = _layout(e4, n, 4, npair + pad_in)
        want = ref.h2_scaled(host_in, n, imp, 4, 1, ld_in=npair + pad_in, ld_out=nn + pad_out, out_fill=SENTINEL)
        want = np.concatenate([want, np.full(nn * (nn + pad_out) - want.size, SENTINEL)])
        d_in, d_out = ctx.to_device(host_in), ctx.to_device(np.full(want.size, SENTINEL))
        assert _call(ctx, n, imp, d_in, 4, npair + pad_in, d_out, 1, nn + pad_out) == 0
        assert _same_bits(d_out.get(), want, nan_survives=False), (n, pad_in, pad_out)
        d_in.free(), d_out.free()


def test_h2_scaled_refuses_bad_indices_and_overlap(ctx):
    n = 6
    npair, nn = _rows(n, 4), _rows(n, 1)
    d_a, d_b = ctx.zeros((nn * nn + 64,), np.float64), ctx.zeros((nn * nn,), np.float64)
    for bad in ([0, 6], [-1, 2], [1, 3, 1], [0, 1, 2, 3, 4, 5, 5]):
        assert _call(ctx, n, bad, d_a, 4, npair, d_b, 4, npair) == DMK_ERR_INVALID, bad
    shifted = d_a.offset(8, (npair * npair,))
    assert _call(ctx, n, [0, 1], d_a, 4, npair, shifted, 4, npair) == DMK_ERR_INVALID            # partial overlap
    assert _call(ctx, n, [0, 1], d_a, 4, npair, d_a, 1, nn) == DMK_ERR_INVALID                   # same base, other storage
    assert _call(ctx, n, [0, 1], d_a, 4, npair + 1, d_a, 4, npair) == DMK_ERR_INVALID            # same base, other pitch
    assert _call(ctx, n, [0, 1], d_a, 4, npair - 1, d_b, 4, npair) == DMK_ERR_INVALID            # pitch shorter than a row
    assert _call(ctx, n, [0, 1], d_a, 8, 0, d_b, 1, nn) == DMK_ERR_INVALID                       # no 8 -> 1 form
    assert np.all(d_a.get() == 0.0) and np.all(d_b.get() == 0.0)                                 # nothing was launched
    assert _call(ctx, n, [0, 1], d_a, 4, npair, d_a, 4, npair) == 0


PERIOD = 1048573


def _pattern(idx):
    """Closed form of the element index: exact in binary, and exact after the scaling by a multiple of 1/4."""
    return ((idx % PERIOD) + 1) * 0.125


def _device_pattern(ctx, nelem):
    """_pattern(0 .. nelem) built on the device: one period uploaded, then doubled by device-to-device copies."""
    from libdmet_preview_amd._lib import lib
    d = ctx.empty((nelem,), np.float64)
    d.offset(0, (PERIOD,)).set(_pattern(np.arange(PERIOD)))
    have = PERIOD
    while have < nelem:
        m = min(have, nelem - have)
        ctx.check(lib.dmk_memcpy_d2d(ctx.h, d.offset(have, (m,)).ptr, d.ptr, m * 8))
        have += m
    return d


@pytest.mark.parametrize("n,out_sym", [(216, 1), (304, 4)])
def test_h2_scaled_beyond_2_to_31_elements(ctx, n, out_sym):
    ctx.trim()
    if ctx.mem_info()[0] < 48 * (1 << 30):
        pytest.skip("needs 48 GB of free device memory")
    npair = _rows(n, 4)
    nrow = _rows(n, out_sym)
    n_in, n_out = npair * npair, nrow * nrow
    assert n_out > 2 ** 31
    imp = [0, 2, n - 1]
    d_in = _device_pattern(ctx, n_in)
    d_out = ctx.empty((n_out,), np.float64)
    assert _call(ctx, n, imp, d_in, 4, npair, d_out, out_sym, nrow) == 0

    # sampled elements: random ones, the last row of every row class at its last column and at a column without impurity
    # index, the very last element
    rng = np.random.default_rng(n)
    rows, cols = rng.integers(0, nrow, 3000), rng.integers(0, nrow, 3000)
    cls = ref.pair_classes(n, imp)
    k, l = ref.tril_pairs(n)
    pair = np.zeros((n, n), dtype=np.int64)
    pair[k, l] = pair[l, k] = np.arange(npair)
    if out_sym == 4:
        row_cls = cls
        to_pair = lambda r: r
    else:
        row_cls = cls[pair.reshape(-1)]
        to_pair = lambda r: pair.reshape(-1)[r]
    last_rows = [int(np.where(row_cls == c)[0][-1]) for c in range(3)]
    col_env = int(pair[1, 1]) if out_sym == 4 else n + 1
    rows = np.concatenate([rows, last_rows, last_rows, [nrow - 1]])
    cols = np.concatenate([cols, [nrow - 1] * 3, [col_env] * 3, [nrow - 1]])
    p, q = to_pair(rows), to_pair(cols)
    csum = cls[p] + cls[q]
    src = _pattern(p.astype(np.int64) * npair + q)
    want = np.where(csum == 4, src, np.where(csum == 0, 0.0, src * (csum * 0.25)))
    flat = rows.astype(np.int64) * nrow + cols
    assert flat.max() == n_out - 1 and flat.max() > 2 ** 31 and set(csum.tolist()) == {0, 1, 2, 3, 4}
    got = np.asarray([d_out.offset(int(f), (1,)).get()[0] for f in flat])
    assert np.array_equal(got, want)
    d_in.free()
    d_out.free()
    ctx.trim()


# ---- the global density ---------------------------------------------------------------------------------------------------------

def _lattice(mesh, nlo, imp):
    from libdmet_preview_amd.system.lattice import Lattice
    L = Lattice(nlo, mesh)
    L.set_val_virt_core(list(imp), [], [i for i in range(nlo) if i not in imp])
    return L


@pytest.mark.parametrize("name,mesh", CASES)
def test_rho_glob_matches_the_reference(ctx, g41, name, mesh):
    from libdmet_preview_amd.routine import slater_helper as sh
    g = lambda key: g41[name + "/" + key]
    basis, rho = g("basis"), g("rdm1_emb")
    nlo = basis.shape[2]
    L, L2 = _lattice(mesh, nlo, g("lo_imp_idx")), _lattice(mesh, nlo, g("frag2_imp_idx"))
    assert np.abs(sh.get_rho_glob_R(basis, L, rho) - g("rho_glob_R")).max() < TOL
    assert np.abs(sh.get_rho_glob_R(basis, L, rho, compact=False) - g("rho_glob_R_full")).max() < TOL
    assert np.abs(sh.get_rho_glob_full(basis, L, rho) - g("rho_glob_full")).max() < TOL
    assert np.abs(sh.get_rho_glob_k(basis, L, rho) - g("rho_glob_k")).max() < TOL
    two = sh.get_rho_glob_R([basis, basis], [L, L2], [rho, g("rdm1_emb2")], sign=[1, -1])
    assert two.shape == g("rho_glob_2frag").shape and np.abs(two - g("rho_glob_2frag")).max() < TOL
    two_k = sh.get_rho_glob_k([basis, basis], [L, L2], [rho, g("rdm1_emb2")], sign=[1, -1])
    assert np.abs(two_k - g("rho_glob_2frag_k")).max() < TOL
    other = sh.get_emb_basis_other_cell(L, basis, 1)
    assert np.array_equal(other, basis[:, [L.subtract(I, 1) for I in range(basis.shape[1])]])


def test_rho_glob_against_the_loop_over_cells(ctx):
    from libdmet_preview_amd.routine import slater_helper as sh
    mesh, nlo, neo, imp = (3, 2, 1), 5, 7, [0, 2, 3]
    rng = np.random.default_rng(321)
    sub = ref.mesh_subtract(mesh)
    for spin in (1, 2):
        basis = rng.standard_normal((spin, 6, nlo, neo))
        rho = rng.standard_normal((spin, neo, neo))
        rho = 0.5 * (rho + rho.transpose(0, 2, 1))
        L = _lattice(mesh, nlo, imp)
        want = ref.rho_glob_R(basis, sub, imp, rho)
        assert np.abs(sh.get_rho_glob_R(basis, L, rho) - want).max() < TOL
        assert np.abs(sh.get_rho_glob_R(basis, L, rho, sign=[1]) - ref.rho_glob_R(basis, sub, imp, rho, compact=False)).max() < TOL
        assert np.abs(sh.get_rho_glob_R(basis[0], L, rho[0]) - want[:1]).max() < TOL        # no spin axis: one is added
    with pytest.raises(NotImplementedError):
        sh.get_rho_glob_R(basis, _outside(mesh, nlo), rho)


def _outside(mesh, nlo):
    L = _lattice(mesh, nlo, [0, 2])
    L.val_idx = [0, nlo + 2]          # an impurity orbital in the second cell
    return L


# ---- the host layer -------------------------------------------------------------------------------------------------------------

class _Vcor(object):
    def __init__(self, value):
        self.value = value

    def get(self, i=0, kspace=True):
        return self.value


def _setup(g41, g8, name, mesh):
    """This package's Lattice and Integral in the state the fixture generator gave the reference's."""
    from libdmet_preview_amd.system import integral
    g = lambda key: g41[name + "/" + key]
    basis = g("basis")
    spin, nk, nlo, nb = basis.shape
    val = [int(x) for x in g8[name + "/val"]]
    from libdmet_preview_amd.system.lattice import Lattice
    L = Lattice(nlo, mesh)
    L.set_val_virt_core(val, [i for i in range(nlo) if i > max(val)], [i for i in range(nlo) if i < min(val)])
    sq = (lambda x: x[0]) if spin == 1 else (lambda x: x)
    L.hcore_lo_R, L.fock_lo_R = sq(g8[name + "/H1_R"]), sq(g8[name + "/Fock_R"])
    L.hcore_lo_k, L.fock_lo_k = L.R2k(L.hcore_lo_R), L.R2k(L.fock_lo_R)
    L.JK_core, L.H0 = np.array(g("JK_core")), float(g("lattice_H0"))
    L.cell.pbc_intor = True
    stored = {}
    for i in range(nk):
        for j in range(i, nk):
            stored[(i, j)] = g("B_%d_%d" % (i, j))
    blocks = dfjk_ref.expand_pairs(stored, nk)

    class Kmf(object):
        def get_jk(self, dm_kpts=None):
            return dfjk_ref.get_jk(lambda a, b: blocks[(a, b)], dm_kpts)
    L.kmf, L.C_ao_lo = Kmf(), g("C_ao_lo")
    ImpHam = integral.Integral(nb, spin == 1, False, float(g("H0")), {"cd": np.array(g("H1"))}, {"ccdd": np.array(g8[name + "/H2"])})
    return g, L, ImpHam, basis, spin, nb


@pytest.mark.parametrize("name,mesh", CASES)
def test_scalers_and_results_match_the_reference(ctx, g41, g8, name, mesh):
    from libdmet_preview_amd.routine import slater
    g, L, ImpHam, basis, spin, nb = _setup(g41, g8, name, mesh)
    imp, rho = g("imp_idx"), g("rdm1_emb")
    H2 = np.array(ImpHam.H2["ccdd"])
    out = slater.get_H2_scaled(H2, imp)
    assert out is H2 and np.array_equal(H2, g("H2_scaled_s4"))
    H2_s1 = np.asarray([ref.restore_1(h, nb) for h in ImpHam.H2["ccdd"]])
    want_s1 = g("H2_scaled_s1") if name + "/H2_scaled_s1" in g41.files else np.asarray([ref.restore_1(h, nb) for h in g("H2_scaled_s4")])
    assert np.array_equal(slater.get_H2_scaled(H2_s1, imp), want_s1)
    with pytest.raises(ValueError):
        slater.get_H2_scaled(np.zeros((1, 3, 3, 3)), [0])

    rhoImp, Efrag, nelec = slater.transformResults(rho, None, basis, ImpHam)
    assert Efrag is None and np.array_equal(rhoImp, g("tr_rhoImp")) and abs(nelec - g("tr_nelec")) < TOL
    rhoImp, Efrag, nelec = slater.transformResults(rho, float(g("E_solver")), basis, ImpHam, lattice=L, last_dmu=float(g("last_dmu")))
    assert np.array_equal(rhoImp, g("tr_lat_rhoImp")) and abs(Efrag - g("tr_lat_Efrag")) < TOL and abs(nelec - g("tr_lat_nelec")) < TOL
    L.JK_core = None
    rhoImp, Efrag, nelec = slater.transformResults(rho, float(g("E_solver")), basis, ImpHam, lattice=L, last_dmu=float(g("last_dmu")),
                                                   imp_idx=g("tr_sub_imp_idx"), dmu_idx=list(g("tr_sub_dmu_idx")))
    assert np.array_equal(rhoImp, g("tr_sub_rhoImp")) and abs(Efrag - g("tr_sub_Efrag")) < TOL and abs(nelec - g("tr_sub_nelec")) < TOL


@pytest.mark.parametrize("name,mesh", CASES)
def test_veff_and_dmet_hamiltonian_match_the_reference(ctx, g41, g8, name, mesh, tmp_path, monkeypatch):
    from libdmet_preview_amd.routine import slater
    monkeypatch.chdir(tmp_path)
    g, L, ImpHam, basis, spin, nb = _setup(g41, g8, name, mesh)
    rho, last_dmu = g("rdm1_emb"), float(g("last_dmu"))
    veff, veff_ao, rdm1_R = slater.get_veff_from_rdm1_emb(L, rho, basis, return_update=True)
    assert np.abs(veff - g("veff")).max() < TOL and np.abs(veff_ao - g("veff_ao")).max() < TOL
    assert np.abs(rdm1_R - g("veff_rdm1_glob_R")).max() < TOL
    assert np.abs(slater.get_veff_from_rdm1_emb(L, rho, basis) - g("veff")).max() < TOL
    assert os.listdir(str(tmp_path)) == []                  # the reference's rdm1_glob_lo_k.npy is not written

    want_s4 = g("H2_scaled_s4")
    want_s1 = g("H2_scaled_s1") if name + "/H2_scaled_s1" in g41.files else np.asarray([ref.restore_1(h, nb) for h in want_s4])

    def check(tag, H, compact=True):
        assert np.abs(H.H1["cd"] - g("hd_%s_H1" % tag)).max() < TOL and abs(H.H0 - g("hd_%s_H0" % tag)) < TOL, tag
        assert H.norb == nb and H.restricted == (spin == 1) and not H.bogoliubov
        assert np.array_equal(H.H2["ccdd"], want_s4 if compact else want_s1), tag
    check("jkcore", slater.get_H_dmet(basis, L, ImpHam, last_dmu))
    check("jkcore_s1", slater.get_H_dmet(basis, L, ImpHam, last_dmu, compact=False), compact=False)
    keep, L.JK_core = L.JK_core, None
    check("nojk", slater.get_H_dmet(basis, L, ImpHam, last_dmu))
    L.JK_core = keep
    check("veff", slater.get_H_dmet(basis, L, ImpHam, last_dmu, rdm1_emb=rho, veff=g("veff")))
    check("rebuild", slater.get_H_dmet(basis, L, ImpHam, last_dmu, rdm1_emb=rho, rebuild_veff=True))
    check("E1", slater.get_H_dmet(basis, L, ImpHam, last_dmu, rdm1_emb=rho, E1=float(g("E1_given"))))
    check("vcor", slater.get_H_dmet(basis, L, ImpHam, last_dmu, add_vcor_to_E=True, vcor=_Vcor(g("vcor"))))
    # the ERI handed in 1-fold storage gives the same scaled blocks
    Ham1 = type(ImpHam)(nb, spin == 1, False, ImpHam.H0, {"cd": ImpHam.H1["cd"]},
                        {"ccdd": np.asarray([ref.restore_1(h, nb) for h in ImpHam.H2["ccdd"]])})
    check("jkcore", slater.get_H_dmet(basis, L, Ham1, last_dmu))
    check("jkcore_s1", slater.get_H_dmet(basis, L, Ham1, last_dmu, compact=False), compact=False)

    class Solver(object):
        def run_dmet_ham(self, H, scale=1.0):
            return scale * (H.H0 + np.sum(H.H1["cd"] * rho) + 1e-2 * np.sum(H.H2["ccdd"][0]))
    assert abs(slater.get_E_dmet(basis, L, ImpHam, last_dmu, Solver(), solver_args={"scale": 0.5}) - g("E_dmet")) < TOL
    fock_add = g("mf_fock_add")

    class Mf(object):
        def make_rdm1(self):
            return rho if spin == 2 else rho[0] * 2.0

        def get_hcore(self):
            return ImpHam.H1["cd"] if spin == 2 else ImpHam.H1["cd"][0]

        def get_fock(self, h1e=None, dm=None):
            return h1e + (fock_add if spin == 2 else fock_add[0])

    class HfSolver(object):
        mf = Mf()
    assert abs(slater.get_E_dmet_HF(basis, L, ImpHam, last_dmu, HfSolver()) - g("E_dmet_HF")) < TOL
    assert np.abs(slater.get_H1_dmet(L, basis, L.hcore_lo_k, L.fock_lo_k, g("JK_imp2")) - g("H1_dmet")).max() < TOL


def test_veff_of_a_model_lattice_uses_the_local_eri(ctx):
    """The "local" branch: J and K of the cell-0 density against the cell-local ERI, the same at every k; other formats raise."""
    from libdmet_preview_amd.routine import slater
    mesh, nlo, neo = (3, 2, 1), 4, 6
    rng = np.random.default_rng(77)
    L = _lattice(mesh, nlo, [0, 1, 2, 3])
    L.is_model = True
    eri = rng.standard_normal((nlo,) * 4)
    eri = eri + eri.transpose(1, 0, 2, 3)
    eri = eri + eri.transpose(0, 1, 3, 2)
    eri = eri + eri.transpose(2, 3, 0, 1)
    L.set_H2_local(eri)
    basis = rng.standard_normal((1, 6, nlo, neo))
    rho = rng.standard_normal((1, neo, neo))
    rho = 0.5 * (rho + rho.transpose(0, 2, 1))
    veff, veff_ao, rdm1_R = slater.get_veff_from_rdm1_emb(L, rho, basis, return_update=True)
    dm0 = 2.0 * ref.rho_glob_R(basis, ref.mesh_subtract(mesh), [0, 1, 2, 3], rho)[0, 0]
    want = np.einsum("ijkl,kl->ij", eri, dm0) - 0.5 * np.einsum("ijkl,il->jk", eri, dm0)
    assert veff.shape == (1, 6, nlo, nlo) and np.abs(veff - want[None, None]).max() < TOL * max(1.0, np.abs(want).max())
    assert np.abs(veff_ao - veff).max() < TOL and np.abs(rdm1_R[0, 0] - dm0).max() < TOL
    L.H2_format = "nearest"
    with pytest.raises(NotImplementedError):
        slater.get_veff_from_rdm1_emb(L, rho, basis)


def test_rebound_get_H_dmet_is_this_package(ctx, g41, g8):
    from tests import df_duck
    from libdmet_preview_amd.routine import slater
    name, mesh = CASES[1]
    g, L, ImpHam, basis, spin, nb = _setup(g41, g8, name, mesh)
    with df_duck.patched_reference() as rs:
        assert rs.get_H_dmet is slater.get_H_dmet and rs.get_rho_glob_R is slater.get_rho_glob_R
        assert rs.transformResults is slater.transformResults and rs.get_H2_scaled is slater.get_H2_scaled
        H = rs.get_H_dmet(basis, L, ImpHam, float(g("last_dmu")))
    assert np.abs(H.H1["cd"] - g("hd_jkcore_H1")).max() < TOL and np.array_equal(H.H2["ccdd"], g("H2_scaled_s4"))


# ---- memory ---------------------------------------------------------------------------------------------------------------------

def test_entry_points_give_their_memory_back(ctx):
    """The method of tests/test_gpu_handle_lifetime.py: sync, trim, mem_info after every call; twenty calls of each new entry point
    end no more than 1 MiB below the mark taken after the warm-up calls."""
    from libdmet_preview_amd._lib import lib, mesh3
    n, imp = 33, np.asarray([0, 2, 32], dtype=np.int32)
    npair = _rows(n, 4)
    d4, d1 = ctx.zeros((npair * npair,), np.float64), ctx.zeros((n ** 4,), np.float64)
    mesh, nlo, neo, spin = (3, 2, 1), 5, 7, 2
    rng = np.random.default_rng(1)
    d_b, d_r = ctx.to_device(rng.standard_normal((spin, 6, nlo, neo))), ctx.to_device(rng.standard_normal((spin, neo, neo)))
    d_o = ctx.empty((spin, 6, nlo, nlo), np.float64)
    imp_lo = np.asarray([0, 2, 3], dtype=np.int32)

    def one_call():
        ctx.check(lib.dmk_dmet_h2_scaled(ctx.h, n, imp.ctypes.data, 3, 4, d4.ptr, npair, 1, d1.ptr, n * n))
        ctx.check(lib.dmk_dmet_h2_scaled(ctx.h, n, imp.ctypes.data, 3, 1, d1.ptr, n * n, 4, d4.ptr, npair))
        ctx.check(lib.dmk_rho_glob(ctx.h, mesh3(mesh), nlo, neo, spin, d_b.ptr, d_r.ptr, imp_lo.ctypes.data, 3, d_o.ptr))
    mark = free = None
    for it in range(3 + 20):
        one_call()
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == 2:
            mark = free
    assert mark - free < (1 << 20), (mark, free)
