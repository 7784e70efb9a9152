"""
GPU tests (-m gpu) of the many-workgroup real symmetric eigensolver (csrc/eigh_large.hip: dmk_eighl_factor / _vectors / _free),
the device gather of a block of the expanded density (dmk_stripe_gather) and the eigenvalue-flavoured baths / bath_opt above the
one-workgroup limit (routine/slater.py, routine/spinless.py: EIGH_LARGE_MIN).

Bounds of the kernel tests are those of tests/test_gpu_parity.py::test_eigh_above_1024 (n = 1100), each times max(1, n / 1100).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import restate as R
from oracle import restate_gso as G
from tests.test_oracle_gso import BATH
from tests.test_gpu_parity import _wilkinson, _glued, _lattice, _proj

NB = 32           # reflectors per compact-WY panel of csrc/eigh_large.hip; an n x n matrix has n - 1 reflectors


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _factor(ctx, A, lda=None):
    """(handle, w, device copy of A, host image of what was uploaded)."""
    from libdmet_preview_amd._lib import lib
    n = A.shape[0]
    lda = n if lda is None else lda
    buf = np.full((n, lda), 7.5)                   # the padding columns must never be read
    buf[:, :n] = A
    dA = ctx.to_device(buf)
    dw = ctx.empty((n,), np.float64)
    h = C.c_void_p()
    ctx.check(lib.dmk_eighl_factor(ctx.h, n, dA.ptr, lda, dw.ptr, C.byref(h)))
    return h, dw.get(), dA, buf


def _vectors(ctx, h, n, idx):
    from libdmet_preview_amd._lib import lib
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    dV = ctx.empty((max(len(idx), 1), n), np.float64)
    ctx.check(lib.dmk_eighl_vectors(h, len(idx), idx.ctypes.data_as(C.c_void_p), dV.ptr))
    return dV.get()[:len(idx)]


def _solve(ctx, A, idx=None, lda=None):
    from libdmet_preview_amd._lib import lib
    n = A.shape[0]
    h, w, dA, buf = _factor(ctx, A, lda)
    try:
        Vt = _vectors(ctx, h, n, np.arange(n) if idx is None else idx)
    finally:
        lib.dmk_eighl_free(h)
    assert np.array_equal(dA.get(), buf)            # A is not modified
    return w, Vt


def _check(A, w, Vt, idx=None):
    """eigenvalues, orthonormality and residual with the bounds of test_eigh_above_1024 scaled by max(1, n / 1100)."""
    n = A.shape[0]
    f = max(1.0, n / 1100.0)
    wr = np.linalg.eigvalsh(A)
    scale = np.abs(wr).max()
    errs = (np.abs(w - wr).max() / scale, 0.0, 0.0)
    if Vt.shape[0]:
        sel = np.arange(n) if idx is None else np.asarray(idx)
        V = Vt.T
        errs = (errs[0], np.abs(V.T @ V - np.eye(V.shape[1])).max(), np.abs(A @ V - V * w[sel]).max() / scale)
    print("n = %d, m = %d: eigenvalues %.2e, orthonormality %.2e, residual %.2e" % ((n, Vt.shape[0]) + errs))
    assert errs[0] < 1e-11 * f
    assert errs[1] < 1e-11 * f
    assert errs[2] < 1e-10 * f


def _rand_sym(n, seed=None):
    g = np.random.default_rng(n if seed is None else seed).standard_normal((n, n))
    return g + g.T


# 2, 3: the smallest (one reflector with tau = 0; one active reflector).  n - 1 reflectors against NB = 32: 31 and 32 below one panel,
# 33 exactly one, 34 one and a ragged second; 64 / 65 / 66 the same around two panels; 129 four panels exactly; 300 nine full panels
# and a ragged tenth.  Odd n also exercises the padding column of the working copy, n = 300 several row groups per workgroup.
@pytest.mark.parametrize("n,lda", [(2, None), (3, None), (31, None), (32, None), (33, None), (34, None), (64, None), (65, 72),
                                   (66, None), (129, None), (300, None)])
def test_eighl_parity(ctx, n, lda):
    A = _rand_sym(n)
    w, Vt = _solve(ctx, A, lda=lda)
    _check(A, w, Vt)
    w2, Vt2 = _solve(ctx, A, lda=lda)
    assert np.array_equal(w, w2) and np.array_equal(Vt, Vt2)          # no atomics: bit-identical


def test_eighl_selection(ctx):
    """Subsets of the vectors: the rows must be those of the all-vectors call up to sign.  Both calls deliver vectors whose residual
    |A v - w v|_2 is below r = sqrt(n) 1e-10 max|w| (asserted in max-norm by _check); an approximate eigenvector with residual r lies
    within r / gap of the true one (sin theta theorem, gap = distance of its eigenvalue to the rest of the spectrum), two of them
    within 2 r / gap of each other -- that is the bound, nothing fitted."""
    from libdmet_preview_amd._lib import lib
    n = 300
    A = _rand_sym(n)
    h, w, dA, buf = _factor(ctx, A)
    try:
        full = _vectors(ctx, h, n, np.arange(n))
        _check(A, w, full)
        gap = np.minimum(np.diff(w, prepend=-np.inf), np.diff(w, append=np.inf))
        r = np.sqrt(n) * 1e-10 * np.abs(w).max()
        rng = np.random.default_rng(5)
        for idx in (np.sort(rng.choice(n, 23, replace=False)), np.asarray([137]), np.arange(n - 17, n), np.asarray([], dtype=np.int32)):
            Vt = _vectors(ctx, h, n, idx)
            assert Vt.shape == (len(idx), n)
            _check(A, w, Vt, idx)
            for q, j in enumerate(idx):
                dev = min(np.abs(Vt[q] - full[j]).max(), np.abs(Vt[q] + full[j]).max())
                assert dev <= 2.0 * r / gap[j], (j, dev, gap[j])
    finally:
        lib.dmk_eighl_free(h)
    assert np.array_equal(dA.get(), buf)


@pytest.mark.parametrize("copies,glue", [(9, 1e-9), (4, 1e-13)])
def test_eighl_glued_wilkinson(ctx, copies, glue):
    """Clusters of `copies` eigenvalues within `glue` inside ONE unreduced block (tests/test_gpu_parity.py), dressed by a fixed
    random orthogonal similarity so that the tridiagonalisation has work to do."""
    T = _glued([_wilkinson(10)] * copies, glue)
    n = T.shape[0]
    Q, _ = np.linalg.qr(np.random.default_rng(11).standard_normal((n, n)))
    A = Q @ T @ Q.T
    A = 0.5 * (A + A.T)
    w, Vt = _solve(ctx, A)
    _check(A, w, Vt)


def test_eighl_projector(ctx):
    """An exact projector: the 40 selected vectors are ONE cluster (eigenvalue 1, 40-fold); what must come back is its range."""
    n, k = 200, 40
    Q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((n, k)))
    P = Q @ Q.T
    P = 0.5 * (P + P.T)
    w, Vt = _solve(ctx, P, idx=np.arange(n - k, n))
    print("projector: |Vt^T Vt - P| %.2e, orthonormality %.2e, top eigenvalues in [%.16f, %.16f]"
          % (np.abs(Vt.T @ Vt - P).max(), np.abs(Vt @ Vt.T - np.eye(k)).max(), w[n - k], w[-1]))
    assert np.abs(Vt.T @ Vt - P).max() < 1e-11
    assert np.abs(Vt @ Vt.T - np.eye(k)).max() < 1e-11


def test_eighl_refusals(ctx):
    from libdmet_preview_amd._lib import lib, DmkError
    A = _rand_sym(40)
    bad = A.copy()
    bad[7, 3] = np.nan                                # lower triangle: it is referenced
    with pytest.raises(DmkError, match="error -4"):   # DMK_ERR_NOCONV
        _factor(ctx, bad)
    h, w, _, _ = _factor(ctx, A)
    try:
        for idx in ([3, 3], [5, 2], [0, 40], [-1, 4]):
            with pytest.raises(DmkError, match="error -1"):      # DMK_ERR_INVALID
                _vectors(ctx, h, 40, idx)
        _check(A, w, _vectors(ctx, h, 40, [2, 5]), [2, 5])        # the handle is still good
    finally:
        lib.dmk_eighl_free(h)


def test_stripe_gather(ctx):
    from libdmet_preview_amd.routine.slater import stripe_gather_dev
    mesh, nlo = (3, 2, 2), 5
    stripe = np.random.default_rng(2).standard_normal((12, nlo, nlo))
    big = R.CellArith(mesh).expand(stripe[None])[0]
    imp = np.asarray([1, 2, 3], dtype=np.int32)
    env = np.asarray([i for i in range(12 * nlo) if i not in set(imp.tolist())], dtype=np.int32)
    d_stripe = ctx.to_device(stripe)
    for rows, cols in ((env, env), (env, imp)):
        out = stripe_gather_dev(ctx, mesh, nlo, d_stripe, ctx.to_device(rows), ctx.to_device(cols),
                                ctx.empty((len(rows), len(cols)), np.float64)).get()
        assert np.array_equal(out, big[rows][:, cols])


# ---- golden cases through the new path (EIGH_LARGE_MIN lowered to 0) -----------------------------------------------------

@pytest.fixture
def large_everywhere(monkeypatch):
    from libdmet_preview_amd.routine import slater, spinless
    monkeypatch.setattr(slater, "EIGH_LARGE_MIN", 0)
    monkeypatch.setattr(spinless, "EIGH_LARGE_MIN", 0)


def test_G4_eig_bath_large_path(ctx, golden, large_everywhere):
    from libdmet_preview_amd.routine import slater
    g = golden("G4_bath.npz")
    for name in ("C1", "C2"):
        mesh = tuple(int(x) for x in g[name + "/mesh"])
        rho = g[name + "/rhoT"]
        nlo = rho.shape[-1]
        Lm = _lattice(mesh, nlo, val=list(range(nlo)))
        bb = slater.get_emb_basis(Lm, rho, kind="eig")
        ref = g[name + "/basis_eig"]
        assert bb.shape == ref.shape
        assert np.linalg.norm(_proj(bb) - _proj(ref)) < 1e-10


def _span(a, r):
    a, r = a.reshape(-1, a.shape[-1]), r.reshape(-1, r.shape[-1])
    return np.abs(a @ a.T - r @ r.T).max()


def _gso_lattice(golden, name, n, val):
    from libdmet_preview_amd.system.lattice import Lattice
    g7 = golden("G7_bcs.npz")
    mesh = tuple(int(x) for x in g7[name + "/mesh"])
    L = Lattice(n, mesh)
    L.val_idx = list(val)
    L.virt_idx = [i for i in range(n) if i > max(val)]
    L.core_idx = [i for i in range(n) if i < min(val)]
    return L, mesh, g7[name + "/GRho"]


@pytest.mark.parametrize("name,n,val", BATH)
def test_gso_eig_bath_large_path(ctx, golden, large_everywhere, name, n, val):
    from libdmet_preview_amd.routine import spinless
    L, mesh, GRho = _gso_lattice(golden, name, n, val)
    nimp = 2 * (len(L.val_idx) + len(L.virt_idx))
    g18 = golden("G18_branches.npz")
    for vb, tag in ((True, "val"), (False, "full")):
        be = spinless.get_emb_basis(L, GRho, kind="eig", valence_bath=vb)
        ref = g18["%s/gso_eig_%s" % (name, tag)]
        assert be.shape == ref.shape and np.array_equal(be[..., :nimp], ref[..., :nimp])
        assert _span(be[..., nimp:], ref[..., nimp:]) < 1e-10


@pytest.mark.parametrize("name,n,val", BATH)
def test_bath_opt_large_path(ctx, golden, large_everywhere, name, n, val):
    from libdmet_preview_amd.routine import spinless
    L, mesh, _ = _gso_lattice(golden, name, n, val)
    g19 = golden("G19_bath_opt.npz")
    for tag in ("a", "b"):
        GT = g19["%s/%s/GRho" % (name, tag)]
        D = R.CellArith(mesh).expand(GT[None])[0]
        for vb, vtag in ((True, "val"), (False, "full")):
            key = "%s/%s/%s" % (name, tag, vtag)
            bo = spinless.get_emb_basis(L, GT, kind="svd", valence_bath=vb, bath_opt=True)
            ref = g19[key + "/basis_opt"]
            assert bo.shape == ref.shape and _span(bo, ref) < 1e-8
            Bm = bo.reshape(-1, bo.shape[-1])
            ne = np.trace(Bm.T @ D @ Bm)
            assert abs(ne - round(ne)) < 1e-5 and np.abs(Bm.T @ Bm - np.eye(Bm.shape[-1])).max() < 1e-10


# ---- the public path above 2000 ---------------------------------------------------------------------------------------

NCELL = 288


def _chain_density(nlo, beta=None):
    """Density of a gapped chain of NCELL cells: real nearest-neighbour hopping block 0.5 N(0, 1), symmetrised random on-site block
    plus a +-2 staggering, nlo / 2 bands occupied at every k (Fermi function at `beta` around the mid-gap level otherwise), folded
    k -> R.  Returns (mesh, stripe (NCELL, nlo, nlo), band gap)."""
    mesh = (1, 1, NCELL)
    rng = np.random.default_rng(1)
    T = 0.5 * rng.standard_normal((nlo, nlo))
    S = rng.standard_normal((nlo, nlo))
    H0 = 0.5 * (S + S.T) + np.diag([2.0 if i % 2 == 0 else -2.0 for i in range(nlo)])
    HR = np.zeros((NCELL, nlo, nlo))
    HR[0], HR[1], HR[NCELL - 1] = H0, T, T.T
    ew, ev = np.linalg.eigh(R.R2k(HR, mesh))
    nocc = nlo // 2
    lo, hi = ew[:, nocc - 1].max(), ew[:, nocc].min()
    if beta is None:
        occ = np.zeros_like(ew)
        occ[:, :nocc] = 1.0
    else:
        occ = 1.0 / (np.exp(beta * (ew - 0.5 * (lo + hi))) + 1.0)
    return mesh, R.k2R(np.einsum("kpi,ki,kqi->kpq", ev, occ, ev.conj()), mesh), hi - lo


def _env_eigenvalues(mesh, stripe, imp):
    big = R.CellArith(mesh).expand(stripe[None])[0]
    env = [i for i in range(big.shape[0]) if i not in set(imp)]
    return np.linalg.eigvalsh(big[env][:, env])


def _no_hair_splitting(ew):
    """No eigenvalue whose distance to {0, 1} lies in [1e-12, 1e-6]: the default tol_bath = 1e-9 then selects the same set whether it
    is applied to the oracle's eigenvalues or to the device's (which agree to ~1e-13)."""
    dist = np.minimum(np.abs(ew), np.abs(1.0 - ew))
    assert not np.any((dist >= 1e-12) & (dist <= 1e-6)), np.sort(dist[(dist >= 1e-12) & (dist <= 1e-6)])
    return dist


@pytest.fixture(scope="module")
def chain_zero_t():
    """Zero-temperature model (env 2296) and the oracle's eig bath, computed once."""
    mesh, rho, gap = _chain_density(8)
    dist = _no_hair_splitting(_env_eigenvalues(mesh, rho, range(8)))
    ref = R.get_emb_basis(mesh, 8, rho, imp_idx=list(range(8)), val_idx=list(range(8)), kind="eig")
    print("chain: gap %.3f, %d env eigenvalues off {0, 1} by more than 1e-6" % (gap, int((dist > 1e-6).sum())))
    return mesh, rho, ref


def test_eig_bath_above_2000_zero_t(ctx, chain_zero_t):
    from libdmet_preview_amd.routine import slater
    mesh, rho, ref = chain_zero_t
    L = _lattice(mesh, 8, val=list(range(8)))
    assert L.ncells * 8 - 8 > slater.EIGH_LARGE_MIN == 2000
    b = slater.get_emb_basis(L, rho, kind="eig")
    assert b.shape == ref.shape
    assert np.array_equal(b[..., :8], ref[..., :8])
    assert np.linalg.norm(_proj(b[..., 8:]) - _proj(ref[..., 8:])) < 1e-10
    b2 = slater.get_emb_basis(L, np.asarray((rho, rho)), kind="eig")
    assert b2.shape == (2,) + ref.shape[1:]
    for s in range(2):
        assert np.array_equal(b2[s, ..., :8], ref[0, ..., :8])
        assert np.linalg.norm(_proj(b2[s:s + 1, ..., 8:]) - _proj(ref[..., 8:])) < 1e-10


def test_eig_bath_above_2000_fractional(ctx):
    """Fermi occupations at beta = 3: every env eigenvalue is kept and they are heavily clustered, so the span is the whole
    environment and the content of the test is the orthonormality of 2296 re-orthogonalised vectors."""
    from libdmet_preview_amd.routine import slater
    mesh, rho, _ = _chain_density(8, beta=3.0)
    ref, info = R.get_emb_basis(mesh, 8, rho, imp_idx=list(range(8)), val_idx=list(range(8)), kind="eig", return_info=True)
    L = _lattice(mesh, 8, val=list(range(8)))
    b = slater.get_emb_basis(L, rho, kind="eig")
    assert b.shape == ref.shape == (1, NCELL, 8, 8 + 2296)
    assert b.shape[-1] - 8 == info["nbath_s"][0]
    B = b.reshape(-1, b.shape[-1])
    err = np.abs(B.T @ B - np.eye(B.shape[1])).max()
    print("beta = 3: |B^T B - I| = %.2e" % err)
    assert err < 1e-10


def test_gso_eig_bath_above_2000(ctx):
    from libdmet_preview_amd.routine import spinless
    from libdmet_preview_amd.system.lattice import Lattice
    mesh, rho, gap = _chain_density(4)
    GRho = np.zeros((NCELL, 8, 8))
    GRho[:, :4, :4] = rho
    GRho[:, 4:, 4:] = -rho
    GRho[0, 4:, 4:] += np.eye(4)
    _no_hair_splitting(_env_eigenvalues(mesh, GRho, range(8)))
    L = Lattice(4, mesh)
    L.val_idx = list(range(4))
    assert NCELL * 8 - 8 > spinless.EIGH_LARGE_MIN == 2000
    ref, _ = G.get_emb_basis_gso_eig(mesh, GRho, 4, list(range(4)), list(range(4)))
    b = spinless.get_emb_basis(L, GRho, kind="eig")
    assert b.shape == ref.shape and np.array_equal(b[..., :8], ref[..., :8])
    assert _span(b[..., 8:], ref[..., 8:]) < 1e-10


def test_eighl_c4_size(ctx):
    """The env dimension of BASELINE config 4 with the spectrum of a density matrix: 3000 zeros, 3540 ones and 12 values inside,
    A = H diag(lam) H^T with H a product of three Householder reflectors (O(n^2) host work, no host eigensolver)."""
    n = 6552
    f = n / 1100.0
    rng = np.random.default_rng(6552)
    inner = np.sort(rng.uniform(0.05, 0.95, 12))
    lam = np.concatenate([np.zeros(3000), inner, np.ones(3540)])       # ascending: the 12 are indices 3000 .. 3011
    A = np.diag(lam)
    for _ in range(3):
        u = rng.standard_normal(n)
        u /= np.linalg.norm(u)
        A -= 2.0 * np.outer(u, u @ A)
        A -= 2.0 * np.outer(A @ u, u)
    A = 0.5 * (A + A.T)
    idx = np.arange(3000, 3012)
    w, Vt = _solve(ctx, A, idx=idx)
    V = Vt.T
    errs = (np.abs(w[idx] - inner).max(), np.abs(A @ V - V * w[idx]).max(), np.abs(V.T @ V - np.eye(12)).max())
    print("n = 6552: interior eigenvalues %.2e, residual %.2e, orthonormality %.2e" % errs)
    assert errs[0] < 1e-11 * f
    assert errs[1] < 1e-10 * f
    assert errs[2] < 1e-11 * f
