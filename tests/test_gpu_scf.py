"""
The embedded Hartree-Fock solver on the device: the one-pass Fock build dmk_fock_s4 against the factored reference
of tests/scf_ref.py and against literal einsums, the SCF driver (solver/scf.py SCF.HF) against the numpy SCF of the same file, the
SCFSolver layer and the DMET energies built on it.

Tolerances: 1e-10 max-abs for one-body quantities whose entries are O(1); converged densities within the
first-order rotation bound 4 sqrt(tol) / gap of the gradient threshold sqrt(tol).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import scf_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCF_TOL = 1e-12
DMK_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _npair(n):
    return n * (n + 1) // 2


def _sym(rng, shape):
    a = rng.standard_normal(shape)
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _dev_block(ctx, sysm, which, ld=None):
    """lam L_x^T L_y as a device block of pitch ld, built by the library's own contraction from the 12 packed factor rows (a
    562 MB block at n = 129 is never formed on the host)."""
    from libdmet_preview_amd._lib import lib
    npair = _npair(sysm.n)
    ld = ld or npair
    L = {"a": R.tril_pack(sysm.A), "b": R.tril_pack(sysm.B)}
    d_x, d_y = ctx.to_device(L[which[0]]), ctx.to_device(L[which[1]])
    d_E = ctx.zeros((npair, ld), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npair, npair, R.NAUX, sysm.lam, d_x.ptr, npair, d_y.ptr, npair, d_E.ptr, ld))
    return d_E


@functools.lru_cache(maxsize=None)
def _ref(kind, n, Sz, alpha=1.0):
    return R.run_case(kind, n, Sz, alpha=alpha)


# ---- 1. the one-pass Fock build --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [5, 64, 65, 129])
def test_fock_s4_against_the_factored_reference(ctx, n, pad):
    from libdmet_preview_amd.solver import scf
    sysm = R.System(n, 100 + n, [n // 2])
    npair = _npair(n)
    rng = np.random.default_rng(n)
    d_E = _dev_block(ctx, sysm, "aa", npair + pad)
    dj, dk = _sym(rng, (n, n)), _sym(rng, (n, n)) / np.sqrt(n)          # two DIFFERENT densities: J[dm_j], K[dm_k]
    vj, vk = scf.fock_dev(ctx, n, d_E, ctx.to_device(dj), ctx.to_device(dk), ld=npair + pad)
    ej, ek = np.abs(vj.get() - sysm.J("aa", dj)).max(), np.abs(vk.get() - sysm.K("aa", dk)).max()
    print("fock_s4 n=%d pad=%d: max|dJ| = %.3e  max|dK| = %.3e  (|J| %.2f |K| %.2f)" % (
        n, pad, ej, ek, np.abs(sysm.J("aa", dj)).max(), np.abs(sysm.K("aa", dk)).max()))
    assert ej <= TOL and ek <= TOL
    # the two passes it replaces: J to rounding (jk_j_kernel sums in another order), K bit for bit (both families of the row kernel
    # share one body), and the pass is bit-reproducible
    j2, _, _ = scf.jk_dev(ctx, n, d_E, ctx.to_device(dj), None, None, ld=npair + pad)
    _, _, k2 = scf.jk_dev(ctx, n, d_E, None, None, ctx.to_device(dk), ld=npair + pad)
    assert np.abs(vj.get() - j2.get()).max() <= TOL
    assert np.array_equal(vk.get(), k2.get())
    vj3, vk3 = scf.fock_dev(ctx, n, d_E, ctx.to_device(dj), ctx.to_device(dk), ld=npair + pad)
    assert np.array_equal(vj.get(), vj3.get()) and np.array_equal(vk.get(), vk3.get())


@pytest.mark.parametrize("pad", [0, 3])
def test_fock_s4_nonsymmetric_density_against_the_einsum(ctx, pad):
    from libdmet_preview_amd.solver import scf
    n = 5
    npair = _npair(n)
    sysm = R.System(n, 7, [2])
    rng = np.random.default_rng(17)
    dj, dk = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    blk = np.zeros((npair, npair + pad))
    blk[:, :npair] = sysm.block_s4("aa")
    e1 = R.restore_s1(sysm.block_s4("aa"), n)
    vj, vk = scf.fock_dev(ctx, n, ctx.to_device(blk), ctx.to_device(dj), ctx.to_device(dk), ld=npair + pad)
    assert np.abs(vj.get() - np.einsum("ijkl,kl->ij", e1, dj)).max() <= TOL
    assert np.abs(vk.get() - np.einsum("ijkl,il->jk", e1, dk)).max() <= TOL


# ---- 2. the NM = 8 instantiation through a row range ---------------------------------------------------------------------------------

def test_fock_s4_rows_at_n_257(ctx):
    from libdmet_preview_amd.solver import scf
    n, nrows = 257, 64
    npair = _npair(n)
    rng = np.random.default_rng(257)
    rows = rng.standard_normal((nrows, npair)) / n          # the first 64 packed rows of a block: all the call may touch
    dj, dk = _sym(rng, (n, n)), rng.standard_normal((n, n))
    vj, vk = scf.fock_dev(ctx, n, ctx.to_device(rows), ctx.to_device(dj), ctx.to_device(dk), row_ranges=[(0, nrows)])
    ti, tj = np.tril_indices(n)
    xt = np.where(ti == tj, dj[ti, tj], dj[ti, tj] + dj[tj, ti])
    want_j, want_k = np.zeros((n, n)), np.zeros((n, n))
    for r in range(nrows):
        i, j = ti[r], tj[r]
        M = np.zeros((n, n))
        M[ti, tj] = rows[r]
        M[tj, ti] = rows[r]
        want_j[i, j] = want_j[j, i] = rows[r] @ xt
        want_k[j, :] += M @ dk[i, :]
        if i != j:
            want_k[i, :] += M @ dk[j, :]
    ej, ek = np.abs(vj.get() - want_j).max(), np.abs(vk.get() - want_k).max()
    print("fock_s4_rows n=257 rows [0, 64): max|dJ| = %.3e  max|dK| = %.3e" % (ej, ek))
    assert ej <= TOL and ek <= TOL
    _, _, k2 = scf.jk_dev(ctx, n, ctx.to_device(rows), None, None, ctx.to_device(dk), row_ranges=[(0, nrows)])
    assert np.array_equal(vk.get(), k2.get())          # the K-only family of the row kernel: the same arithmetic in the same order


def test_fock_s4_row_ranges_add_up(ctx):
    """The fused pass over row ranges at n = 65 (NM = 2, npair = 2145): the range rule, the clearing of the rows a call does not
    touch and the fused kernel together.  The partial results of [0, 96) and [96, npair) sum to the whole-block result within
    1e-12 (entries are O(1); the fixed-order gathers add the same terms with zeros in other places), and each partial K equals
    the K-only pass over the same range bit for bit."""
    from libdmet_preview_amd.solver import scf
    n = 65
    npair = _npair(n)
    sysm = R.System(n, 100 + n, [n // 2])
    rng = np.random.default_rng(6500)
    d_E = _dev_block(ctx, sysm, "aa")
    d_dj, d_dk = ctx.to_device(_sym(rng, (n, n))), ctx.to_device(_sym(rng, (n, n)) / np.sqrt(n))
    vj, vk = (a.get() for a in scf.fock_dev(ctx, n, d_E, d_dj, d_dk))
    sum_j, sum_k = np.zeros((n, n)), np.zeros((n, n))
    for rr in ([(0, 96)], [(96, npair)]):
        pj, pk = (a.get() for a in scf.fock_dev(ctx, n, d_E, d_dj, d_dk, row_ranges=rr))
        _, _, k2 = scf.jk_dev(ctx, n, d_E, None, None, d_dk, row_ranges=rr)
        assert np.array_equal(pk, k2.get())
        sum_j += pj
        sum_k += pk
    ej, ek = np.abs(sum_j - vj).max(), np.abs(sum_k - vk).max()
    print("fock_s4_rows n=65 [0, 96) + [96, %d): max|dJ| = %.3e  max|dK| = %.3e" % (npair, ej, ek))
    assert ej <= 1e-12 and ek <= 1e-12


# ---- 2b. the fused pass at its extremes, through the C ABI ---------------------------------------------------------------------------
#
# n < 8 (fewer row pairs than waves: some waves own none), n = 128 / 256 (every lane of every m live in NM = 2 / 4) and n = 512 (the
# documented maximum: 48 KiB of dynamic LDS plus the static jred).  References in np.longdouble; TOL as above, and err / bound printed
# against the forward bounds  J: (npair + 8) eps sum |E| |x~|   K: (2 n + 8) eps sum |M| |d|   (eps = 2^-52).

LD = np.longdouble
EPS = 2.0 ** -52


def _abi_pass(ctx, fused, n, d_E, ld, d_dj, d_dk, ranges=None):
    """dmk_fock_s4[_rows] (fused) or the K-only dmk_jk_s4[_rows] over NaN-filled outputs: host (vj, vk), vj None for K-only."""
    from libdmet_preview_amd._lib import lib
    vj, vk = ctx.to_device(np.full((n, n), np.nan)), ctx.to_device(np.full((n, n), np.nan))
    rr = None if ranges is None else np.asarray(ranges, dtype=np.int64).ravel()
    if fused and ranges is None:
        rc = lib.dmk_fock_s4(ctx.h, n, d_E.ptr, ld, d_dj.ptr, d_dk.ptr, vj.ptr, vk.ptr)
    elif fused:
        rc = lib.dmk_fock_s4_rows(ctx.h, n, d_E.ptr, ld, len(ranges), rr.ctypes.data, d_dj.ptr, d_dk.ptr, vj.ptr, vk.ptr)
    elif ranges is None:
        rc = lib.dmk_jk_s4(ctx.h, n, d_E.ptr, ld, None, None, d_dk.ptr, None, None, vk.ptr)
    else:
        rc = lib.dmk_jk_s4_rows(ctx.h, n, d_E.ptr, ld, len(ranges), rr.ctypes.data, None, None, d_dk.ptr, None, None, vk.ptr)
    ctx.check(rc)
    return (vj.get() if fused else None), vk.get()


def _ratio(got, want, bound):
    return float((np.abs(got.astype(LD) - want) / bound).max())


def test_fock_s4_whole_blocks_below_eight(ctx):
    """Random blocks WITHOUT pair-exchange symmetry (E[p][q] != E[q][p]), non-symmetric dm_j and dm_k, pitch npair + 3 with NaN in
    the padding, against the einsum over the unpacked block."""
    pad = 3
    for n in (1, 2, 3, 4, 7, 8):
        npair = _npair(n)
        rng = np.random.default_rng(800 + n)
        blk = np.full((npair, npair + pad), np.nan)
        blk[:, :npair] = rng.standard_normal((npair, npair))
        dj, dk = rng.standard_normal((n, n)), rng.standard_normal((n, n))
        ti, tj = np.tril_indices(n)
        half = np.zeros((npair, n, n), dtype=LD)
        half[:, ti, tj] = blk[:, :npair]
        half[:, tj, ti] = blk[:, :npair]
        e1 = np.zeros((n, n, n, n), dtype=LD)
        e1[ti, tj], e1[tj, ti] = half, half
        want_j, want_k = np.einsum("ijkl,kl->ij", e1, dj.astype(LD)), np.einsum("ijkl,il->jk", e1, dk.astype(LD))
        # J is computed on the folded density x~ = dj[k,l] + dj[l,k]: the bound sums |E| |x~|
        xt = np.abs(dj + dj.T - np.diag(np.diag(dj))).astype(LD)
        bound_j = (npair + 8) * LD(EPS) * 0.5 * np.einsum("ijkl,kl->ij", np.abs(e1), xt + np.diag(np.diag(xt)))
        bound_k = (2 * n + 8) * LD(EPS) * np.einsum("ijkl,il->jk", np.abs(e1), np.abs(dk).astype(LD))
        d_E, d_dj, d_dk = ctx.to_device(blk), ctx.to_device(dj), ctx.to_device(dk)
        vj, vk = _abi_pass(ctx, True, n, d_E, npair + pad, d_dj, d_dk)
        ej, ek = np.abs(vj - want_j).max(), np.abs(vk - want_k).max()
        print("fock_s4 n=%d pad=%d: max|dJ| = %.3e  max|dK| = %.3e  err / bound J %.4f K %.4f" % (
            n, pad, ej, ek, _ratio(vj, want_j, bound_j), _ratio(vk, want_k, bound_k)))
        assert np.isfinite(vj).all() and np.isfinite(vk).all() and ej <= TOL and ek <= TOL
        _, k2 = _abi_pass(ctx, False, n, d_E, npair + pad, d_dj, d_dk)
        assert np.array_equal(vk, k2)                      # the K-only family: bit for bit
        vj3, vk3 = _abi_pass(ctx, True, n, d_E, npair + pad, d_dj, d_dk)
        assert np.array_equal(vj, vj3) and np.array_equal(vk, vk3)


@pytest.mark.parametrize("n", [128, 256, 512])
def test_fock_s4_rows_with_every_lane_live(ctx, n):
    """Rows [0, 64) as in test_fock_s4_rows_at_n_257: only those rows are allocated, the reference is the same per-row loop, in
    np.longdouble.  At n = 512 the two ranges [0, 32), [32, 64) of ONE call give the bits of the single range."""
    nrows = 64
    npair = _npair(n)
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((nrows, npair)) / n
    dj, dk = _sym(rng, (n, n)), rng.standard_normal((n, n))
    d_rows, d_dj, d_dk = ctx.to_device(rows), ctx.to_device(dj), ctx.to_device(dk)
    vj, vk = _abi_pass(ctx, True, n, d_rows, npair, d_dj, d_dk, [(0, nrows)])
    ti, tj = np.tril_indices(n)
    xt = np.where(ti == tj, dj[ti, tj], dj[ti, tj] + dj[tj, ti]).astype(LD)
    dkl = dk.astype(LD)
    want_j, want_k, abs_j, abs_k = (np.zeros((n, n), dtype=LD) for _ in range(4))
    M = np.zeros((n, n), dtype=LD)
    for r in range(nrows):
        i, j = ti[r], tj[r]
        row = rows[r].astype(LD)
        M[ti, tj] = row
        M[tj, ti] = row
        want_j[i, j] = want_j[j, i] = row @ xt
        abs_j[i, j] = abs_j[j, i] = np.abs(row) @ np.abs(xt)
        want_k[j, :] += M @ dkl[i, :]
        abs_k[j, :] += np.abs(M) @ np.abs(dkl[i, :])
        if i != j:
            want_k[i, :] += M @ dkl[j, :]
            abs_k[i, :] += np.abs(M) @ np.abs(dkl[j, :])
    ej, ek = np.abs(vj - want_j).max(), np.abs(vk - want_k).max()
    live_j, live_k = abs_j > 0, abs_k > 0                  # rows of J / K that the 64 packed rows reach; the rest are exact zeros
    rj = _ratio(vj[live_j], want_j[live_j], (npair + 8) * LD(EPS) * abs_j[live_j])
    rk = _ratio(vk[live_k], want_k[live_k], (2 * n + 8) * LD(EPS) * abs_k[live_k])
    print("fock_s4_rows n=%d rows [0, 64): max|dJ| = %.3e  max|dK| = %.3e  err / bound J %.4f K %.4f" % (n, ej, ek, rj, rk))
    assert ej <= TOL and ek <= TOL
    assert not vj[~live_j].any() and not vk[~live_k].any()
    _, k2 = _abi_pass(ctx, False, n, d_rows, npair, d_dj, d_dk, [(0, nrows)])
    assert np.array_equal(vk, k2)                          # the K-only family of the row kernel: the same arithmetic in the same order
    if n == 512:
        vj2, vk2 = _abi_pass(ctx, True, n, d_rows, npair, d_dj, d_dk, [(0, 32), (32, 64)])
        assert np.array_equal(vj, vj2) and np.array_equal(vk, vk2)


# ---- 3. argument checks --------------------------------------------------------------------------------------------------------------

def test_fock_s4_refuses_bad_arguments(ctx):
    from libdmet_preview_amd._lib import lib
    n = 8
    npair = _npair(n)
    d_E, d_d, d_j, d_k = ctx.zeros((npair, npair), np.float64), ctx.zeros((n, n), np.float64), ctx.zeros((n, n), np.float64), \
        ctx.zeros((n, n), np.float64)
    call = lambda nn, ld, dj, dk, vj, vk: lib.dmk_fock_s4(ctx.h, nn, d_E.ptr, ld, dj, dk, vj, vk)
    assert call(n, npair, d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == 0
    assert call(513, _npair(513), d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == DMK_ERR_INVALID          # n > 512
    assert call(n, npair - 1, d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == DMK_ERR_INVALID              # ld < npair
    assert call(n, npair, d_d.ptr, d_d.ptr, None, d_k.ptr) == DMK_ERR_INVALID                     # a density without its output
    assert call(n, npair, d_d.ptr, d_d.ptr, d_j.ptr, None) == DMK_ERR_INVALID
    for rng_ in ([3, npair], [0, 33], [0, npair + 32]):                                            # misaligned / outside
        rr = np.asarray(rng_, dtype=np.int64)
        assert lib.dmk_fock_s4_rows(ctx.h, n, d_E.ptr, npair, 1, rr.ctypes.data, d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == DMK_ERR_INVALID
    assert lib.dmk_fock_s4_rows(ctx.h, n, d_E.ptr, npair, 0, None, d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == DMK_ERR_INVALID
    rr = np.asarray([0, 32, 32, npair], dtype=np.int64)
    assert lib.dmk_fock_s4_rows(ctx.h, n, d_E.ptr, npair, 2, rr.ctypes.data, d_d.ptr, d_d.ptr, d_j.ptr, d_k.ptr) == 0
    ctx.sync()


# ---- 4. converged SCF against the numpy SCF ----------------------------------------------------------------------------------------------

def _solver(ctx, kind, n, Sz, sysm, ovlp=None):
    """SCF over the device blocks of `sysm` (set_integral_dev: the ERI makes no host trip)."""
    from libdmet_preview_amd.solver import scf
    s = scf.SCF(newton_ah=False)
    s.set_system(R.nelec_of(n), Sz, False, kind == "rhf")
    blocks = [_dev_block(ctx, sysm, w) for w in (("aa",) if kind == "rhf" else ("aa", "bb", "ab"))]
    s.set_integral_dev(n, 0.0, ctx.to_device(sysm.h1[None]), None if ovlp is None else ctx.to_device(ovlp), blocks)
    if ovlp is not None and np.ndim(ovlp) == 3:
        s.integral.ovlp = ovlp
    return s


def _commutator(mf, S=None):
    D, F = np.asarray(mf.make_rdm1()), np.asarray(mf.get_fock(dm=mf.make_rdm1()))
    n = D.shape[-1]
    D, F = D.reshape(-1, n, n), F.reshape(-1, n, n)
    out = 0.0
    for s in range(D.shape[0]):
        Ss = np.eye(D.shape[-1]) if S is None else (S if np.ndim(S) == 2 else S[s])
        fds = F[s] @ D[s] @ Ss
        out = max(out, np.abs(fds - fds.T).max())
    return out


@pytest.mark.parametrize("kind,n,Sz", [("rhf", 6, 0), ("rhf", 65, 0), ("rhf", 129, 0), ("uhf", 6, 0), ("uhf", 6, 2), ("uhf", 65, 0),
                                       ("uhf", 65, 2)])
def test_converged_scf_matches_the_reference(ctx, kind, n, Sz):
    ref = _ref(kind, n, Sz)
    s = _solver(ctx, kind, n, Sz, ref["system"])
    E, rho = s.HF(tol=SCF_TOL, MaxIter=50)
    mf = s.mf
    D = np.asarray(mf.make_rdm1())
    dD, comm = np.abs(D - ref["D"]).max(), _commutator(mf)
    print("%s n=%d Sz=%d: E = %.12f  |dE| = %.3e  cycles %d  max|dD| = %.3e (bound %.3e)  max|FD-DF| = %.3e  gap_ref %.3f" % (
        kind, n, Sz, E, abs(E - ref["E"]), mf.cycles, dD, 4.0 * np.sqrt(SCF_TOL) / ref["gap"], comm, ref["gap"]))
    assert mf.converged is True
    assert abs(E - ref["E"]) <= TOL
    assert dD <= 4.0 * np.sqrt(SCF_TOL) / ref["gap"]
    assert comm <= np.sqrt(SCF_TOL)
    # the reference's conventions for what HF returns and what .mf holds
    if kind == "rhf":
        assert rho.shape == (1, n, n) and np.array_equal(rho[0], D * 0.5)
        assert mf.mo_coeff.shape == (n, n) and mf.mo_energy.shape == (n,) and mf.mo_occ.sum() == R.nelec_of(n)
        assert s.get_mo().shape == (1, n, n) and s.get_mo_energy().shape == (1, n)
    else:
        assert rho.shape == (2, n, n) and np.array_equal(rho, D)
        assert mf.mo_coeff.shape == (2, n, n) and [int(x) for x in mf.mo_occ.sum(axis=1)] == ref["nocc"]
        assert s.get_mo().shape == (2, n, n) and s.get_mo_energy().shape == (2, n)
    assert np.abs(np.asarray(mf.mo_energy) - ref["mo_energy"]).max() <= 4.0 * np.sqrt(SCF_TOL)
    assert abs(mf.e_tot - E) == 0.0 and abs(mf.energy_tot() - E) <= TOL and abs(mf.energy_elec()[0] - E) <= TOL
    assert np.abs(np.asarray(mf.get_veff(dm=ref["D"])) - ref["V"]).max() <= TOL
    assert np.array_equal(np.asarray(mf.get_hcore()), ref["system"].h1 if kind == "rhf" else np.asarray([ref["system"].h1] * 2))


# ---- 5. option variants (n = 6) -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,spin_resolved", [("rhf", False), ("uhf", False), ("uhf", True)])
def test_scf_with_an_overlap(ctx, kind, spin_resolved):
    n, Sz = 6, 0
    sysm = R.make_system(kind, n, Sz)
    rng = np.random.default_rng(31)
    S = np.eye(n) + 0.05 * _sym(rng, (n, n))
    if spin_resolved:
        S = np.asarray([S, np.eye(n) + 0.05 * _sym(rng, (n, n))])
    ref = R.run_case(kind, n, Sz, S=S)
    assert ref["converged"] and ref["gap"] >= 0.5
    s = _solver(ctx, kind, n, Sz, sysm, ovlp=S)
    E, _ = s.HF(tol=SCF_TOL)
    assert s.mf.converged and abs(E - ref["E"]) <= TOL
    assert np.abs(np.asarray(s.mf.make_rdm1()) - ref["D"]).max() <= 4.0 * np.sqrt(SCF_TOL) / ref["gap"]
    assert _commutator(s.mf, S) <= np.sqrt(SCF_TOL)
    C_ = np.asarray(s.mf.mo_coeff).reshape(-1, n, n)
    for k in range(C_.shape[0]):               # orbitals are orthonormal in the metric of their spin
        Sk = S if np.ndim(S) == 2 else S[k]
        assert np.abs(C_[k].T @ Sk @ C_[k] - np.eye(n)).max() <= TOL


def test_uhf_with_mu(ctx):
    kind, n, Sz, Mu = "uhf", 6, 0, 0.3
    sysm = R.make_system(kind, n, Sz)
    h = np.asarray([sysm.h1, sysm.h1])
    h_mu = h.copy()
    h_mu[0, :n // 2, :n // 2] -= np.eye(n // 2) * Mu
    h_mu[0, n // 2:, n // 2:] += np.eye(n - n // 2) * Mu
    ref = R.scf(h_mu, sysm.veff_uhf, R.nocc_of(kind, n, Sz), False, h1_energy=h)
    assert ref["converged"] and ref["gap"] >= 0.5
    s = _solver(ctx, kind, n, Sz, sysm)
    E, rho = s.HF(tol=SCF_TOL, Mu=Mu)
    assert s.mf.converged and abs(E - ref["E"]) <= TOL and np.abs(rho - ref["D"]).max() <= 4.0 * np.sqrt(SCF_TOL) / ref["gap"]
    assert np.array_equal(s.mf.get_hcore(), h_mu) and abs(s.mf.energy_tot() - E) <= TOL
    E0, _ = s.HF(tol=SCF_TOL)
    assert abs(E0 - _ref(kind, n, Sz)["E"]) <= TOL and abs(E0 - E) > 1e-6          # the shift did change the state


@pytest.mark.parametrize("kind", ["rhf", "uhf"])
def test_scf_options(ctx, kind):
    n, Sz = 6, 0
    ref, half = _ref(kind, n, Sz), _ref(kind, n, Sz, 0.5)
    s = _solver(ctx, kind, n, Sz, ref["system"])
    E_half, _ = s.HF(tol=SCF_TOL, alpha=0.5)
    assert s.mf.converged and abs(E_half - half["E"]) <= TOL and abs(E_half - ref["E"]) > 1e-6
    # a guess given (3-d is accepted for RHF too) and the core guess land on the same energy
    g = R.core_guess(kind, n, Sz) + 1e-2 * _sym(np.random.default_rng(3), (n, n))
    E_guess, _ = s.HF(tol=SCF_TOL, InitGuess=g[None] if kind == "rhf" else g)
    E_core, _ = s.HF(tol=SCF_TOL, InitGuess=None)
    assert abs(E_guess - ref["E"]) <= TOL and abs(E_core - ref["E"]) <= TOL
    E_plain, _ = s.HF(tol=SCF_TOL, do_diis=False)
    assert s.mf.converged and abs(E_plain - ref["E"]) <= TOL
    E_short, rho = s.HF(tol=SCF_TOL, MaxIter=2)
    assert s.mf.converged is False and s.mf.cycles == 2 and np.isfinite(E_short) and np.isfinite(rho).all()
    s2 = _solver(ctx, kind, n, Sz, ref["system"])
    s2.no_kernel = True
    assert s2.HF() == (0.0, 0.0)
    s3 = _solver(ctx, kind, n, Sz, ref["system"])
    s3.newton_ah = True                                                  # accepted: runs the DIIS iteration
    assert abs(s3.HF(tol=SCF_TOL)[0] - ref["E"]) <= TOL


# ---- 6. ERI input forms -----------------------------------------------------------------------------------------------------------------

def _energy_of_form(kind, n, Sz, h1, eri):
    from libdmet_preview_amd.solver import scf
    s = scf.SCF(newton_ah=False)
    s.set_system(R.nelec_of(n), Sz, False, kind == "rhf")
    s.set_integral(n, 0.125, {"cd": h1[None]}, {"ccdd": eri})          # a one-spin H1: duplicated for UHF
    E, _ = s.HF(tol=SCF_TOL)
    assert s.mf.converged
    return E


@pytest.mark.parametrize("kind", ["rhf", "uhf"])
def test_eri_forms_give_the_same_energy(ctx, kind):
    """1-, 4- and 8-fold input.  (An 8-fold array carries one spin block -- with a spin axis of three it has the shape of a bare
    4-fold one, system/integral.py get_eri_format -- so the unrestricted 8-fold case is the spin-independent ERI.)"""
    n, Sz = 6, 0
    ref = _ref(kind, n, Sz)
    sysm = ref["system"]
    one = sysm.blocks_s4()[:1]
    forms = lambda blocks: {"s4": blocks, "s1": np.asarray([R.restore_s1(b, n) for b in blocks]),
                            "s8": np.asarray([R.pack_s8(b) for b in blocks])}
    E = {name: _energy_of_form(kind, n, Sz, sysm.h1, eri) for name, eri in forms(one).items()}
    assert abs(E["s1"] - E["s4"]) <= 1e-12 and abs(E["s8"] - E["s4"]) <= 1e-12
    if kind == "rhf":
        assert abs(E["s4"] - 0.125 - ref["E"]) <= TOL
    else:
        three = forms(sysm.blocks_s4())
        E3 = {name: _energy_of_form(kind, n, Sz, sysm.h1, three[name]) for name in ("s4", "s1")}
        assert abs(E3["s4"] - 0.125 - ref["E"]) <= TOL and abs(E3["s1"] - E3["s4"]) <= 1e-12


# ---- 7. SCFSolver and the DMET energies ---------------------------------------------------------------------------------------------------

def _ham(kind, n, sysm, H0=0.0):
    from libdmet_preview_amd.system import integral
    restricted = kind == "rhf"
    h1 = sysm.h1[None] if restricted else np.asarray([sysm.h1, sysm.h1])
    return integral.Integral(n, restricted, False, H0, {"cd": h1}, {"ccdd": sysm.blocks_s4()[:1 if restricted else 3]})


@pytest.mark.parametrize("kind,Sz", [("rhf", 0), ("uhf", 0), ("uhf", 2)])
def test_scfsolver_run_and_dmet_hamiltonian_energy(ctx, kind, Sz):
    from libdmet_preview_amd.solver import scf, scf_solver
    from libdmet_preview_amd.routine import slater
    from libdmet_preview_amd.system import integral
    n = 6
    ref = _ref(kind, n, Sz)
    sysm, restricted = ref["system"], kind == "rhf"
    Ham = _ham(kind, n, sysm)
    solver = scf_solver.SCFSolver(restricted=restricted, Sz=Sz, tol=SCF_TOL)
    rho, E = solver.run(Ham, nelec=R.nelec_of(n))
    s = scf.SCF(newton_ah=True)
    s.set_system(R.nelec_of(n), Sz, False, restricted)
    s.set_integral(Ham)
    E2, rho2 = s.HF(tol=SCF_TOL, MaxIter=200)
    assert E == E2 and np.array_equal(rho, rho2) and abs(E - ref["E"]) <= TOL and solver.make_rdm1() is rho
    assert solver.mf is solver.scfsolver.mf and solver.mf.converged

    # the energy of the state on a scaled DMET Hamiltonian: against h1 . r1 + 1/2 r2 . h2 with the literal r2
    imp = np.asarray([0, 1, 3])
    rng = np.random.default_rng(9)
    H1s = _sym(rng, Ham.H1["cd"].shape)
    H2s = slater.get_H2_scaled(np.array(Ham.H2["ccdd"]), imp)
    Hs = integral.Integral(n, restricted, False, 0.75, {"cd": H1s}, {"ccdd": H2s})
    h2 = [R.restore_s1(b, n) for b in H2s]
    r2 = solver.make_rdm2(ao_repr=True)
    if restricted:
        want = 2.0 * np.einsum("pq,qp", H1s[0], rho[0]) + 0.5 * np.einsum("pqrs,pqrs", h2[0], r2[0])
    else:
        want = (np.einsum("spq,sqp", H1s, rho) + 0.5 * np.einsum("pqrs,pqrs", r2[0], h2[0]) + 0.5 * np.einsum("pqrs,pqrs", r2[1], h2[1])
                + np.einsum("pqrs,pqrs", r2[2], h2[2]))
    want += 0.75
    got_mo, got_ao = solver.run_dmet_ham(Hs), solver.run_dmet_ham(Hs, ao_repr=True)
    print("run_dmet_ham %s Sz=%d: %.12f  want %.12f" % (kind, Sz, got_mo, want))
    assert abs(got_mo - want) <= TOL and got_ao == got_mo

    # customised orbitals: the density and the energy follow them
    c = np.asarray(ref["mo_coeff"])
    rho3, E3 = solver.run(Ham, nelec=R.nelec_of(n), mo_coeff_custom=c)
    assert np.abs(rho3 - (ref["D"][None] * 0.5 if restricted else ref["D"])).max() <= TOL and abs(E3 - ref["E"]) <= TOL


@pytest.mark.parametrize("name,nelec", [("rhf_411", 4), ("uhf_222", 6)])
def test_dmet_hf_energy_with_the_new_solver(ctx, name, nelec):
    """slater.get_E_dmet_HF on the Hubbard stand-in of tests/test_gpu_dmet_ham.py with the device solver, against the same formula
    fed with the numpy SCF's density and Fock matrix.  The formula is linear in D at fixed Fock matrix and F is linear in D, so with
    |dD|_max <= 4 sqrt(tol) / gap the energies differ by at most (sum |h1 + F| / 2 + sum |D| max |dF / dD|) |dD|_max; the bound
    below takes the cruder n^2 (max |h1| + 2 max |F|) |dD|_max."""
    from tests.test_gpu_dmet_ham import _setup, CASES
    from libdmet_preview_amd.routine import slater
    from libdmet_preview_amd.solver import scf_solver
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g41, g8 = np.load(os.path.join(gold, "G41_dmet_ham.npz")), np.load(os.path.join(gold, "G8_embham.npz"))
    g, L, ImpHam, basis, spin, nb = _setup(g41, g8, name, dict(CASES)[name])
    restricted = spin == 1
    e1 = [R.restore_s1(b, nb) for b in ImpHam.H2["ccdd"]]
    nocc = [nelec // 2] * spin
    ref = R.scf(ImpHam.H1["cd"], lambda D: R.veff_s1(e1, D, restricted), nocc, restricted, H0=ImpHam.H0)
    assert ref["converged"] and ref["gap"] >= 0.5
    solver = scf_solver.SCFSolver(restricted=restricted, Sz=0, tol=SCF_TOL)
    solver.run(ImpHam, nelec=nelec, dm0=ref["D"])                  # (the stand-in has several SCF solutions: start at the reference's)
    assert solver.mf.converged and abs(solver.mf.e_tot - ref["E"]) <= TOL
    last_dmu = float(g("last_dmu"))
    got = slater.get_E_dmet_HF(basis, L, ImpHam, last_dmu, solver)

    class RefMf(object):
        def make_rdm1(self):
            return ref["D"]

        def get_hcore(self):
            return ImpHam.H1["cd"][0] if restricted else ImpHam.H1["cd"]

        def get_fock(self, h1e=None, dm=None):
            return ref["F"]
    want = slater.get_E_dmet_HF(basis, L, ImpHam, last_dmu, type("S", (), {"mf": RefMf()})())
    bound = nb * nb * (np.abs(ImpHam.H1["cd"]).max() + 2.0 * np.abs(ref["F"]).max()) * 4.0 * np.sqrt(SCF_TOL) / ref["gap"]
    print("get_E_dmet_HF %s: %.12f  reference %.12f  |d| = %.3e  bound %.3e" % (name, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound


# ---- 8. memory --------------------------------------------------------------------------------------------------------------------------

def test_hf_runs_give_their_memory_back(ctx):
    """The pattern of tests/test_gpu_dmet_ham.py: sync, trim, mem_info after every round; twenty rounds (a restricted and an
    unrestricted run, each creating and destroying its handle, and a bare create / free) end no more than 1 MiB below the mark
    taken after the warm-up rounds."""
    from libdmet_preview_amd._lib import lib
    n = 33
    sr, su = R.System(n, 1, [16]), R.System(n, 2, [16])
    rhf, uhf = _solver(ctx, "rhf", n, 0, sr), _solver(ctx, "uhf", n, 0, su)
    d_h, d_E = ctx.to_device(sr.h1[None]), _dev_block(ctx, sr, "aa")

    def one_round():
        rhf.HF(tol=1e-8)
        uhf.HF(tol=1e-8)
        h = C.c_void_p()
        ctx.check(lib.dmk_scf_create(ctx.h, n, 1, d_h.ptr, None, None, None, 0, d_E.ptr, None, None, _npair(n), 12, 0, C.byref(h)))
        ctx.check(lib.dmk_scf_free(h))
    mark = free = None
    for it in range(3 + 20):
        one_round()
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == 2:
            mark = free
    assert mark - free < (1 << 20), (mark, free)
