"""
The invariant block of the ERI contraction (dmk_eri_attach_cache_block / EriEngine(inv_block=True), run with -m gpu on an MI355X).

With `ninv` invariant leading columns of C_ao_emb the pairs b <= a < ninv are the prefix [0, P) of the packed pair index,
P = ninv (ninv + 1) / 2, and the corner [0, S 128)^2, S = floor(P / 128), of every spin block of the result is the same in every
call that contracts the same kL in the same order into a zeroed ERI.  A warm stacked contraction leaves the corner's tiles out of
every launch (dmk_dgemm_tile_table with skip = S) and copies the kept corner back.

Reference of every comparison: the same engine WITHOUT a cache (the dense path of the same build) on the same inputs, with the same
plane stack.  Dense against dense is bit-identical (one writer per element per launch, stream-ordered launches), and so must be
everything else: every ERI comparison here is exact.
Shapes: mesh 3 x 2 x 1 (two weight-1 and two weight-2 kL), naux 24, nao 24, nemb 48 (npair 1176 = 10 tiles, the last one ragged),
two spins, a stack over all kL; ninv 32 (plane region A = 32, S = 4) and ninv 40 (A = 32, S = 6: columns [32, 40) belong to the
block alone).  The bare product: M = N = 680 (6 tiles, ragged), K = 24.
"""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MESH, NK, NAUX, NAO, NEMB, SPIN = (3, 2, 1), 6, 24, 24, 48, 2
NPAIR = NEMB * (NEMB + 1) // 2
NBLK = SPIN * (SPIN + 1) // 2
TILES = (NPAIR + 127) // 128
CASES = {32: 4, 40: 6}                       # ninv -> S


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@pytest.fixture(scope="module")
def bufs(ctx):
    b = [ctx.zeros((NBLK, NPAIR, NPAIR), np.float64) for _ in range(3)]
    yield b
    for x in b:
        x.free()


def _C(seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((SPIN, NK, NAO, NEMB)) + 1j * rng.standard_normal((SPIN, NK, NAO, NEMB))) / np.sqrt(NAO)


def _df(seed=5):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((NK, 3)), NAUX, NAO, seed=seed)


def _count(symm, skip, tiles=TILES):
    from libdmet_preview_amd._lib import lib
    n = C.c_int64(-1)
    assert lib.dmk_dgemm_tile_table(tiles, tiles, int(symm), -1, -1, skip, None, 0, C.byref(n)) == 0
    return int(n.value)


def _run(ctx, Ce, df, eri_dev, cache=None, inv_cols=None, prefill=None, nslots=None, max_blocks=None, probe=None, bands=False):
    """One whole transform into `eri_dev` (zeroed first, or set to `prefill`).  Returns the engine's flags and the executed dgemm
    flop of the call."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    if prefill is None:
        eri_dev.zero_()
    else:
        eri_dev.set(prefill)
    C_dev = ctx.to_device(Ce)
    eng = et.EriEngine(ctx, MESH, NAO, NAUX, NEMB, SPIN, C_dev, eri_dev, inv_cache=cache, inv_cols=inv_cols)
    out = {"attached": eng.inv_attached, "cols_used": eng.inv_cols_used, "tiles": eng.inv_block_tiles, "weights": eng.weights,
           "kL": eng.irreducible_kL()}
    try:
        if nslots is None:
            eng.set_stack(n_kL=len(eng.irreducible_kL()))
        else:
            assert eng.set_stack(nslots=nslots) == nslots
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        ctx.profile_read_flops(reset=True)
        for kL in eng.irreducible_kL():
            eng.run_kL(kL, df, max_blocks=max_blocks)
        if bands:
            nb, _ = eng.nbands()
            for b in range(nb):
                eng.contract(b, b + 1, done=(b == nb - 1))
        else:
            eng.contract()
        ctx.sync()
        out["dgemm_flops"] = ctx.profile_read_flops(reset=True)["dgemm"]
    finally:
        eng.close()
    return out


def _flops(run, skip):
    """Executed flop of one stacked contraction over all kL as launch_dgemm_tn_acc counts it: tiles of the table x 128 x 128 x
    2 K per launch; the K of the launches of a spin block add up to 48 rows per weight-2 kL (Re and Im planes) and 24 per
    weight-1 kL; blocks aa and bb run the symmetric table, ab the rectangular one."""
    K = sum(48 if run["weights"][k] == 2 else 24 for k in run["kL"])
    return 2.0 * 128 * 128 * K * (2 * _count(True, skip) + _count(False, skip))


def _same(ctx, a, b, what):
    x, y = a.get(), b.get()
    assert np.array_equal(x, y), "%s: max |difference| %.3e" % (what, np.abs(x - y).max())


def _plane_part(st):
    return {k: st[k] for k in ("entries", "bytes", "drops")}


# ---------------------------------------------------------------------------------------------
# the product alone
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("symm", [True, False])
def test_product_with_a_skipped_corner(ctx, symm):
    from libdmet_preview_amd._lib import lib
    M, K, sentinel = 680, 24, 0.4375
    rng = np.random.default_rng(21)
    X = rng.standard_normal((K, M))
    d_X = ctx.to_device(X)
    d_Y = d_X if symm else ctx.to_device(rng.standard_normal((K, M)))
    d_C = ctx.empty((M, M), np.float64)

    def product(skip):
        d_C.set(np.full((M, M), sentinel))
        ctx.profile_read_flops(reset=True)
        ctx.check(lib.dmk_dgemm_tn_acc_skip(ctx.h, M, M, K, 1.5, d_X.ptr, M, d_Y.ptr, M, d_C.ptr, M, skip))
        ctx.sync()
        return d_C.get(), ctx.profile_read_flops(reset=True)["dgemm"]

    dense, f0 = product(0)
    assert f0 == 2.0 * _count(symm, 0, 6) * 128 * 128 * K
    # against numpy: a sum of K products, (K + 2) eps sum |x| |y| with |x|, |y| <= 5 and the factor 1.5
    assert np.abs(dense - sentinel - 1.5 * X.T @ d_Y.get()).max() < (K + 2) * 2.3e-16 * 1.5 * K * 25
    for skip in (1, 3, 6):
        got, f = product(skip)
        n = min(M, skip * 128)
        assert np.array_equal(got[:n, :n].view(np.uint64), np.full((n, n), sentinel).view(np.uint64)), skip
        mask = np.ones((M, M), dtype=bool)
        mask[:n, :n] = False
        assert np.array_equal(got[mask], dense[mask]), skip
        assert f == 2.0 * _count(symm, skip, 6) * 128 * 128 * K, skip
    assert _count(symm, 6, 6) == 0


def test_product_off_the_table_kernel_refuses_a_skip(ctx):
    """K = 20 runs on the register-staged kernel: with a skip the launch is refused, C stays as it was; without one it runs."""
    from libdmet_preview_amd._lib import lib
    M, K = 256, 20
    d_X = ctx.to_device(np.random.default_rng(22).standard_normal((K, M)))
    d_C = ctx.zeros((M, M), np.float64)
    assert lib.dmk_dgemm_tn_acc_skip(ctx.h, M, M, K, 1.0, d_X.ptr, M, d_X.ptr, M, d_C.ptr, M, 1) != 0
    ctx.sync()
    assert not d_C.get().any()
    ctx.check(lib.dmk_dgemm_tn_acc_skip(ctx.h, M, M, K, 1.0, d_X.ptr, M, d_X.ptr, M, d_C.ptr, M, 0))
    ctx.sync()
    assert d_C.get().any()


# ---------------------------------------------------------------------------------------------
# the engine, table path
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ninv", sorted(CASES))
def test_cold_warm_and_column_changes(ctx, bufs, ninv):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    S = CASES[ninv]
    Ce, df = _C(30 + ninv), _df()
    ref = _run(ctx, Ce, df, bufs[0])
    _run(ctx, Ce, df, bufs[1])
    _same(ctx, bufs[1], bufs[0], "dense vs dense")                       # the yardstick
    assert ref["dgemm_flops"] == _flops(ref, 0)
    n_kL = len(ref["kL"])
    assert sorted(ref["weights"][k] for k in ref["kL"]) == [1, 1, 2, 2]
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        assert cold["attached"] and cold["cols_used"] == 32 and cold["tiles"] == S
        bs = cache.block_stats()
        assert bs == {"hits": 0, "misses": 1, "bytes": NBLK * (S * 128) ** 2 * 8, "tiles": S}, bs
        _same(ctx, bufs[1], bufs[0], "cold")
        assert cold["dgemm_flops"] == _flops(cold, 0)
        warm = _run(ctx, Ce, df, bufs[2], cache=cache, inv_cols=ninv)
        bs = cache.block_stats()
        assert (bs["hits"], bs["misses"]) == (1, 1), bs
        assert cache.stats()["hits"] == n_kL
        _same(ctx, bufs[2], bufs[0], "warm")
        assert warm["dgemm_flops"] == _flops(warm, S) < ref["dgemm_flops"]

        # the bath changes, the invariant columns do not: still a hit, equal to a fresh dense transform
        C2 = Ce.copy()
        C2[..., ninv:] = _C(77)[..., ninv:]
        _run(ctx, C2, df, bufs[0])
        _run(ctx, C2, df, bufs[1], cache=cache, inv_cols=ninv)
        bs = cache.block_stats()
        assert (bs["hits"], bs["misses"]) == (2, 1), bs
        assert cache.stats()["hits"] == 2 * n_kL and cache.stats()["drops"] == 0
        _same(ctx, bufs[1], bufs[0], "bath columns changed")
        assert not np.array_equal(bufs[0].get(), bufs[2].get())

        if ninv == 40:
            # column 35 is outside the plane region (A = 32) and inside the block's columns: the planes still hit, the block goes
            C3 = C2.copy()
            C3[1, 4, NAO - 1, 35] += 1e-9
            _run(ctx, C3, df, bufs[0])
            r = _run(ctx, C3, df, bufs[1], cache=cache, inv_cols=ninv)
            st, bs = cache.stats(), cache.block_stats()
            assert (st["hits"], st["drops"], st["entries"]) == (3 * n_kL, 0, n_kL), st
            assert (bs["hits"], bs["misses"]) == (2, 2), bs
            assert r["dgemm_flops"] == _flops(r, 0)
            _same(ctx, bufs[1], bufs[0], "column 35 changed")
            r = _run(ctx, C3, df, bufs[1], cache=cache, inv_cols=ninv)
            assert cache.block_stats()["hits"] == 3 and r["dgemm_flops"] == _flops(r, S)
            _same(ctx, bufs[1], bufs[0], "column 35 changed, warm")
    finally:
        cache.close()


def test_dense_fallbacks(ctx, bufs):
    """A non-zero ERI on entry, a band contraction and a budget below the block: dense, equal to dense, plane entries untouched."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    ninv, S = 40, CASES[40]
    Ce, df = _C(3), _df()
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        assert cache.block_stats()["hits"] == 1 and r["dgemm_flops"] == _flops(r, S)
        planes0, n_kL = cache.stats(), len(r["kL"])

        # (i) one non-zero element in the corner of the middle spin block; (ii) a negative zero
        for i, value in enumerate((1.0, -0.0)):
            pre = np.zeros((NBLK, NPAIR, NPAIR))
            pre[1, S * 128 - 1, 5] = value
            _run(ctx, Ce, df, bufs[0], prefill=pre)
            r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, prefill=pre)
            assert r["dgemm_flops"] == _flops(r, 0)
            bs = cache.block_stats()
            assert (bs["hits"], bs["misses"], bs["tiles"]) == (1, 2 + i, S), bs
            assert _plane_part(cache.stats()) == _plane_part(planes0)
            x, y = bufs[1].get(), bufs[0].get()
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "ERI not zero on entry (%r)" % value
        # non-zero OUTSIDE the corner does not matter
        pre = np.zeros((NBLK, NPAIR, NPAIR))
        pre[:, S * 128:, :] = 0.25
        pre[:, :, S * 128:] = -0.5
        _run(ctx, Ce, df, bufs[0], prefill=pre)
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, prefill=pre)
        assert r["dgemm_flops"] == _flops(r, S) and cache.block_stats()["hits"] == 2
        _same(ctx, bufs[1], bufs[0], "non-zero outside the corner")

        # a band contraction
        ref = _run(ctx, Ce, df, bufs[0], bands=True)
        before = cache.block_stats()
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, bands=True)
        assert r["dgemm_flops"] == ref["dgemm_flops"]
        assert cache.block_stats() == before
        assert _plane_part(cache.stats()) == _plane_part(planes0) and cache.stats()["hits"] == planes0["hits"] + 4 * n_kL
        _same(ctx, bufs[1], bufs[0], "band contraction")
    finally:
        cache.close()

    # a budget that holds every plane entry (1.3 MB) and not the block (14 MB)
    block_bytes = NBLK * (S * 128) ** 2 * 8
    budget = 4 << 20
    assert budget < block_bytes
    cache = et.EriInvariantCache(ctx, budget_gb=budget / float(1 << 30))
    try:
        _run(ctx, Ce, df, bufs[0])
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        assert r["tiles"] == S
        planes0 = cache.stats()
        assert planes0["entries"] == len(r["kL"]) and 0 < planes0["bytes"] <= budget
        _same(ctx, bufs[1], bufs[0], "small budget, cold")
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        assert r["dgemm_flops"] == _flops(r, 0)
        bs = cache.block_stats()
        assert (bs["hits"], bs["misses"], bs["bytes"], bs["tiles"]) == (0, 2, 0, 0), bs
        assert _plane_part(cache.stats()) == _plane_part(planes0) and cache.stats()["hits"] == planes0["entries"]
        _same(ctx, bufs[1], bufs[0], "small budget, warm planes")
    finally:
        cache.close()


def test_cut_visiting_list_replaces_the_entry(ctx, bufs):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    ninv, S = 32, CASES[32]
    Ce, df = _C(4), _df()
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        for what, mb, hits, misses in (("max_blocks=2", 2, 0, 2), ("max_blocks=2 again", 2, 1, 2), ("full again", None, 1, 3),
                                       ("full, warm", None, 2, 3)):
            _run(ctx, Ce, df, bufs[0], max_blocks=mb)
            r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, max_blocks=mb)
            bs = cache.block_stats()
            assert (bs["hits"], bs["misses"], bs["tiles"]) == (hits, misses, S), (what, bs)
            _same(ctx, bufs[1], bufs[0], what)
    finally:
        cache.close()


def test_short_stack_uses_the_block_in_the_first_round_only(ctx, bufs):
    """Two slots under four kL: the full stack is contracted when the third kL begins (round one, zeroed corner) and the rest at
    the end (round two: the corner is not zero any more)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    ninv, S = 40, CASES[40]
    Ce, df = _C(6), _df()
    ref = _run(ctx, Ce, df, bufs[0], nslots=2)
    assert len(ref["kL"]) == 4
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, nslots=2)
        bs = cache.block_stats()
        assert (bs["hits"], bs["misses"], bs["tiles"]) == (0, 2, S), bs
        assert cold["dgemm_flops"] == ref["dgemm_flops"]
        _same(ctx, bufs[1], bufs[0], "two slots, cold")
        warm = _run(ctx, Ce, df, bufs[2], cache=cache, inv_cols=ninv, nslots=2)
        bs = cache.block_stats()
        assert (bs["hits"], bs["misses"]) == (1, 3), bs
        _same(ctx, bufs[2], bufs[0], "two slots, warm")
        # round one holds the first two kL of the visiting order: their rows are the only ones contracted without the corner
        K1 = sum(48 if warm["weights"][k] == 2 else 24 for k in warm["kL"][:2])
        saved = 2.0 * 128 * 128 * K1 * (2 * (_count(True, 0) - _count(True, S)) + _count(False, 0) - _count(False, S))
        assert warm["dgemm_flops"] == ref["dgemm_flops"] - saved
    finally:
        cache.close()


def test_freivalds_on_a_warm_call(ctx, bufs):
    """eri x against the yref the pipeline accumulates from its planes, at the bound of bench.py, when the corner of eri came from
    the cache."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    ninv = 40
    Ce, df = _C(9), _df()
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, NPAIR))
        d_y = ctx.zeros((NBLK, NPAIR), np.float64)
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, probe=(d_x, d_y))
        assert cache.block_stats()["hits"] == 1
        y = et.eri_times_vector_dev(ctx, bufs[1], NBLK, NPAIR, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        assert np.abs(y - yref).max() <= 1e-10 * max(1.0, np.abs(yref).max()), np.abs(y - yref).max()
    finally:
        cache.close()


def test_switched_off(ctx, bufs):
    """EriEngine(inv_block=False) and pipelines the block is not for arm nothing."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    Ce = _C(8)
    C_dev = ctx.to_device(Ce)
    cache = et.EriInvariantCache(ctx)
    try:
        for kw, tiles in (({"inv_block": False}, 0), ({}, CASES[40]), ({"rows_only": True}, 0)):
            eng = et.EriEngine(ctx, MESH, NAO, NAUX, NEMB, SPIN, C_dev, bufs[0], inv_cache=cache, inv_cols=40, **kw)
            try:
                assert eng.inv_attached and eng.inv_block_tiles == tiles, (kw, eng.inv_block_tiles)
            finally:
                eng.close()
        eng = et.EriEngine(ctx, MESH, NAO, NAUX, NEMB, SPIN, C_dev, bufs[0], inv_cache=cache, inv_cols=15)     # no plane region: no block
        try:
            assert not eng.inv_attached and eng.inv_block_tiles == 0
        finally:
            eng.close()
        assert cache.block_stats() == {"hits": 0, "misses": 0, "bytes": 0, "tiles": 0}
    finally:
        cache.close()
