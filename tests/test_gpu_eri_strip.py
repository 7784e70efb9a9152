"""
Strip step 1 of the ERI half transform (EriEngine(strip_step1=True), dmk_eri_begin flag 16; run with -m gpu on an
MI355X): on top of the split step 1 (K6l) plane rows [192,256) x columns [128,256) come from a strip workgroup of type 1's geometry
(direct segment Ut[:, 192:256] x C_j[:, 128:256], partner segment W x conj(C_i[:, 128:256])), the triangle [128,192)^2 from a corner
workgroup that joins the cached region (the pairs b <= a < 192: 18528 doubles per auxiliary row and plane), and a kL whose region
came from the cache runs step 1 over columns [192,256) only.

Shapes: those of tests/test_gpu_eri_split_step1.py -- mesh 3 x 2 x 1 (weight-1 and weight-2 kL; the plan has a kL whose single
group carries the partner flags 0, 0, 1, 1), naux 24, nemb 256, two spins, queues of 8, 4 and 2, nao 24 / 40 on the K tile (one / two
K tiles of step 1) and 30 off it.

Bounds.  Inside the mode everything is the same sum in the same order: the dense run is made twice and, where the two are
bit-identical, every cold, warm, fused and unfused run of the same queue cut must equal it bit for bit (otherwise 4 x their
difference).  Another queue cut changes the order of the sum over the blocks of a kL: across cuts the oracle tolerance applies, as
in the split tests.  Mode against the split alone: entries outside rows [192,256) x columns [128,256) of every plane are
bit-identical (the corner workgroup gives every accumulator the products type 3 gave it, in the same sequence); the entries inside
are the same sum in another order and are held to the project's oracle tolerance, 1e-8 (measured: profiles/eri_strip_notes.txt).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eri_sample as ES                  # the checker

MESH, NK, NAUX, NEMB, SPIN = (3, 2, 1), 6, 24, 256, 2
NPAIR = NEMB * (NEMB + 1) // 2
NBLK = SPIN * (SPIN + 1) // 2
ORBS = [0, 1, 127, 128, 191, 192, 255]
REGION = 192 * 193 // 2                               # doubles per auxiliary row and plane of a cache entry in the mode


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


def _C(nao, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((SPIN, NK, nao, NEMB)) + 1j * rng.standard_normal((SPIN, NK, nao, NEMB))) / np.sqrt(nao)


def _df(nao, seed=5):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((NK, 3)), NAUX, nao, seed=seed)


def _maxabs(ctx, a, b):
    """max |a - b| of two device arrays; exactly 0.0 when they hold the same values."""
    from libdmet_preview_amd._lib import lib
    ss = ctx.zeros((1,), np.float64)
    ctx.check(lib.dmk_sub_sumsq(ctx.h, a.size, a.ptr, b.ptr, None, ss.ptr))
    if float(ss.get()[0]) == 0.0:
        return 0.0
    rows, ld = a.size // a.shape[-1], a.shape[-1]
    worst = 0.0
    for r0 in range(0, rows, 4096):
        n = min(4096, rows - r0)
        worst = max(worst, float(np.abs(a.offset(r0 * ld, (n, ld)).get() - b.offset(r0 * ld, (n, ld)).get()).max()))
    return worst


def _run(ctx, Ce, df, eri_dev, monkeypatch, strip=True, split=True, group=8, fuse=True, cache=None, planes=True, stack=False,
         probe=None, kLs=None):
    """One whole transform.  Returns the modes the engine reports, the planes of every kL, the cache attach flag, the fused launches
    and the launch counts / executed flop of both half-transform families."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    if fuse:
        monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
    else:
        monkeypatch.setenv("DMK_ERI_FUSE", "0")
    nao = Ce.shape[2]
    eri_dev.zero_()
    eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, ctx.to_device(Ce), eri_dev, inv_cache=cache, split_step1=split,
                       strip_step1=strip)
    out = {"split": eng.split_step1, "strip": eng.strip_step1, "planes": {}, "weights": eng.weights, "by_kL": eng.by_kL,
           "attached": eng.inv_attached, "group": group}
    try:
        assert eng.ring_slots == group
        todo = eng.irreducible_kL() if kLs is None else list(kLs)
        out["kLs"] = todo
        if stack:
            eng.set_stack(n_kL=len(todo))
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        ctx.profile_read(reset=True)
        ctx.profile_read_flops(reset=True)
        for kL in todo:
            eng.run_kL(kL, df)
            if planes:
                out["planes"][kL] = eng.planes().get()
        eng.contract()
        ctx.sync()
        out["fused"] = eng.fused_launches
        prof, flops = ctx.profile_read(reset=True), ctx.profile_read_flops(reset=True)
        out["launches"] = (prof["zgemm_half1"][1], prof["zgemm_half2"][1])
        out["flops"] = (flops["zgemm_half1"], flops["zgemm_half2"])
    finally:
        eng.close()
    return out


def _assert_same(ctx, got, ref, noise, what):
    d = _maxabs(ctx, got, ref)
    print("%s: max |difference| %.3e (dense vs dense %.3e)" % (what, d, noise))
    if noise == 0.0:
        assert d == 0.0, "%s: differs by %.3e although dense vs dense is bit-identical" % (what, d)
    else:
        assert d <= 4.0 * noise, "%s: differs by %.3e, dense vs dense by %.3e" % (what, d, noise)


def _assert_planes(got, ref, noise, what):
    assert sorted(got) == sorted(ref)
    for kL in ref:
        d = float(np.abs(got[kL] - ref[kL]).max())
        assert d <= 4.0 * noise, (what, kL, d)
        assert noise != 0.0 or np.array_equal(got[kL], ref[kL]), (what, kL)


def _groups(run):
    """The partner flags of every group of every kL the run visited (EriEngine.run_kL cuts a kL into groups of equal length)."""
    out = []
    for kL in run["kLs"]:
        sym = [int(r[4]) for r in run["by_kL"][kL]]
        ngrp = 1 if len(sym) <= run["group"] else -(-len(sym) // run["group"])
        per = -(-len(sym) // ngrp)
        out += [(kL, sym[g0:g0 + per]) for g0 in range(0, len(sym), per)]
    return out


# 16 x 16 block products per (L, spin) and queued block of every workgroup type of step 2 in the mode (zhot_half2_body.inc): the
# direct segment, and the partner segment of a block that carries the term -- without the diagonal blocks of the two triangle types
# when every block of the group carries it (they are folded in the epilogue instead).
#   type 0, type 1, strip: 64 x 128 rectangles, 32 blocks, 32 partner products
#   type 2: the triangle [0,128)^2, 36 blocks, 36 - 8 folded partner products
#   corner: the triangle [128,192)^2, 10 blocks, 10 - 4 folded partner products
TILES = {"type0": (32, 32, 32), "type1": (32, 32, 32), "type2": (36, 36, 28), "corner": (10, 10, 6), "strip": (32, 32, 32)}
DENSE_TYPES, WARM_TYPES = ("type0", "type1", "type2", "corner", "strip"), ("type1", "strip")


def _half2_flops(run, nao, warm):
    """Executed flop of step 2: the block products launched, from the tile lists above."""
    types = WARM_TYPES if warm else DENSE_TYPES
    total = 0.0
    for kL, grp in _groups(run):
        fold = all(grp)
        full = sum(TILES[t][0] for t in types)
        part = sum(TILES[t][2 if fold else 1] for t in types)
        blocks = sum(full + (part if s else 0.0) for s in grp)
        total += (4.0 if run["weights"][kL] == 1 else 6.0) * blocks * 256.0 * nao * NAUX * SPIN
    return total


def test_step2_block_counts():
    """The tile lists give 142 (+ 130 | 142) block products dense and 64 (+ 64) warm -- against 136 (+ 120 | 136) and 68 (+ 60 | 68)
    of the split alone (host only)."""
    dense = [sum(TILES[t][i] for t in DENSE_TYPES) for i in range(3)]
    warm = [sum(TILES[t][i] for t in WARM_TYPES) for i in range(3)]
    assert dense == [142, 142, 130] and warm == [64, 64, 64]


def _half1_flops(run, nao, ut_cols, w):
    """Executed flop of step 1: 128 x 64 tiles over the flat rows of a block, `ut_cols` columns of Ut for every block and (w) the 64
    columns of W for every block with the partner term."""
    tiles_m = -(-NAUX * nao // 128)
    total = 0.0
    for kL, grp in _groups(run):
        cols = sum(ut_cols + (64 if (w and s) else 0) for s in grp)
        total += 6.0 * tiles_m * 128 * cols * nao * SPIN
    return total


def _strip_mask():
    """Pair indices of rows [192,256) x columns [128,256) (b <= a)."""
    m = np.zeros(NPAIR, bool)
    for a in range(192, 256):
        m[a * (a + 1) // 2 + 128: a * (a + 1) // 2 + a + 1] = True
    return m


def _oracle(Ce, kLs):
    return ES.eri_sample(MESH, 5, Ce, NAUX, ORBS, sorted(kLs))


def _check_oracle(buf, want, idx, what):
    for blk in range(NBLK):
        got = np.stack([buf.offset((blk * NPAIR + int(r)) * NPAIR, (NPAIR,)).get()[idx] for r in idx])
        d = np.abs(got - want[blk]).max()
        print("%s, spin block %d: against the sampled oracle %.3e" % (what, blk, d))
        assert d < 1e-8


@pytest.mark.parametrize("nao", [24, 40, 30])
def test_cold_warm_dense(ctx, bufs, monkeypatch, nao):
    """Mode on: dense twice, then cold and warm with the cache against dense (ERI and planes of every kL), every kL hits, entry
    bytes, the K6j block hits on a warm stacked run, flop accounting of both families; nao 24: the sampled oracle on dense and on
    warm.  nao 30 is off the K tile: the engine reports the mode off and computes what it computes without the request bit for bit."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    Ce, df = _C(nao, 300 + nao), _df(nao)
    old = _run(ctx, Ce, df, bufs[2], monkeypatch, strip=False)
    assert not old["strip"]
    ref = _run(ctx, Ce, df, bufs[0], monkeypatch)
    if nao == 30:
        assert not ref["strip"] and not ref["split"] and not old["split"]
        assert _maxabs(ctx, bufs[0], bufs[2]) == 0.0
        for kL in old["planes"]:
            assert np.array_equal(ref["planes"][kL], old["planes"][kL])
        assert ref["flops"] == old["flops"]
        return
    assert ref["strip"] and ref["split"] and old["split"]
    again = _run(ctx, Ce, df, bufs[1], monkeypatch)
    noise = _maxabs(ctx, bufs[1], bufs[0])
    print("dense vs dense, mode on: %.3e" % noise)
    _assert_planes(again["planes"], ref["planes"], noise, "dense again")
    n_kL = len(ref["planes"])
    if nao == 24:
        want, idx, _ = _oracle(Ce, ref["planes"])
        _check_oracle(bufs[0], want, idx, "dense")
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache)
        assert cold["strip"] and cold["attached"]
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], noise, "cold")
        _assert_planes(cold["planes"], ref["planes"], noise, "cold")
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"], st["drops"]) == (n_kL, n_kL, n_kL, 0), st
        assert st["bytes"] == sum(SPIN * (1 if ref["weights"][k] == 1 else 2) * NAUX * REGION * 8 for k in ref["planes"])
        _assert_same(ctx, bufs[1], bufs[0], noise, "warm")
        _assert_planes(warm["planes"], ref["planes"], noise, "warm")
        if nao == 24:
            _check_oracle(bufs[1], want, idx, "warm")
        # flop accounting: both families follow the tiles launched
        assert ref["flops"][1] == cold["flops"][1] == _half2_flops(ref, nao, False)
        assert warm["flops"][1] == _half2_flops(warm, nao, True)
        assert ref["flops"][0] == cold["flops"][0] == old["flops"][0] == _half1_flops(ref, nao, 256, True)
        assert warm["flops"][0] == _half1_flops(warm, nao, 64, True)
        assert warm["launches"] == ref["launches"] == old["launches"]
        # the K6j block: a stacked contraction keeps the corner on the first keyed run and hits on the next
        _run(ctx, Ce, df, bufs[2], monkeypatch, stack=True, planes=False)
        _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, stack=True, planes=False)
        before = cache.block_stats()
        _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, stack=True, planes=False)
        bs = cache.block_stats()
        assert bs["hits"] == before["hits"] + 1 and bs["tiles"] > 0, (before, bs)
        _assert_same(ctx, bufs[1], bufs[2], noise, "warm, stacked, block hit")
    finally:
        cache.close()


def test_flop_ratios_where_every_block_has_the_partner(ctx, bufs, monkeypatch):
    """On the kL whose blocks all carry the partner term (one of weight 1, one of weight 2): step 1 of a warm run issues 0.5 x the
    flop of the old dense run, a dense run in the mode 1.25 x; step 2 counts 64 + 64 warm and 142 + 130 dense block products."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 331), _df(nao)
    w, rec = et.eri_plan(MESH, True)
    kLs = [kL for kL in range(len(w)) if w[kL] > 0 and all(int(r[4]) for r in rec if int(r[0]) == kL)]
    assert sorted(int(w[k]) for k in kLs) == [1, 2]
    old = _run(ctx, Ce, df, bufs[0], monkeypatch, strip=False, split=False, kLs=kLs, planes=False)
    dense = _run(ctx, Ce, df, bufs[0], monkeypatch, kLs=kLs, planes=False)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs, planes=False)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs, planes=False)
        assert cache.stats()["hits"] == len(kLs)
    finally:
        cache.close()
    assert dense["strip"] and warm["strip"] and not old["split"] and old["flops"][0] > 0
    assert warm["flops"][0] == 0.5 * old["flops"][0]
    assert dense["flops"][0] == 1.25 * old["flops"][0]
    assert dense["flops"][1] == _half2_flops(dense, nao, False) == old["flops"][1] * 272.0 / 256.0
    assert warm["flops"][1] == _half2_flops(warm, nao, True) == old["flops"][1] * 128.0 / 256.0
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


@pytest.mark.parametrize("nao", [24, 40])
def test_mode_against_split_alone(ctx, bufs, monkeypatch, nao):
    """Planes of both orders: bit-identical outside rows [192,256) x columns [128,256); inside, the same sum in another order, within
    the oracle tolerance.  A weight-1 kL (the real-part-only instantiation) keeps its Im planes zero."""
    Ce, df = _C(nao, 340 + nao), _df(nao)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, strip=False)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch)
    assert on["strip"] and off["split"] and not off["strip"]
    inside = _strip_mask()
    worst, scale = 0.0, 0.0
    for kL in off["planes"]:
        a, b = on["planes"][kL], off["planes"][kL]
        assert np.array_equal(a[..., ~inside], b[..., ~inside]), kL
        worst = max(worst, float(np.abs(a[..., inside] - b[..., inside]).max()))
        scale = max(scale, float(np.abs(b[..., inside]).max()))
        if on["weights"][kL] == 1:
            assert not a[:, 1].any() and a[:, 0][..., inside].any()
    print("nao %d: rows [192,256) x cols [128,256), mode vs split alone: max |difference| %.3e (entries up to %.3e)" % (nao, worst, scale))
    assert worst <= 1e-8
    d = _maxabs(ctx, bufs[1], bufs[0])
    print("nao %d: ERI, mode vs split alone: %.3e" % (nao, d))
    assert d <= 1e-8


@pytest.mark.parametrize("group", [2, 4])
def test_fused_equals_unfused_and_queue_lengths(ctx, bufs, monkeypatch, group):
    """Queues of 2 and 4 cut a kL into several groups (both halves of Ut and of W in use with 2): fused and DMK_ERI_FUSE=0 runs are
    bit-identical, dense and warm, over weight-1 and weight-2 kL and the kL with the partner flags 0, 0, 1, 1."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 350), _df(nao)
    one = _run(ctx, Ce, df, bufs[2], monkeypatch)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, group=group, fuse=False)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group)
    assert on["strip"] and off["strip"] and off["fused"] == 0
    assert (on["fused"] > 0) == (group == 2)
    assert sorted(set(int(on["weights"][k]) for k in on["planes"])) == [1, 2]
    assert any(g == [0, 0, 1, 1] for _, g in _groups(one))
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    for kL in off["planes"]:
        assert np.array_equal(on["planes"][kL], off["planes"][kL]), kL
    assert on["flops"] == off["flops"] and on["launches"] == off["launches"]
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache)
        assert cache.stats()["hits"] == len(off["planes"]) and (warm["fused"] > 0) == (group == 2)
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        for kL in off["planes"]:
            assert np.array_equal(warm["planes"][kL], off["planes"][kL]), kL
        assert warm["flops"][0] == _half1_flops(warm, nao, 64, True)
        assert warm["flops"][1] == _half2_flops(warm, nao, True)
        warm_off = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache, fuse=False)
        assert warm_off["fused"] == 0 and _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        for kL in off["planes"]:
            assert np.array_equal(warm_off["planes"][kL], off["planes"][kL]), kL
    finally:
        cache.close()
    # another cut of the queue changes the order of the sum over the blocks of a kL: across cuts the oracle tolerance applies
    assert _maxabs(ctx, bufs[0], bufs[2]) <= 1e-8
    assert one["strip"]


def test_mixed_group(ctx, bufs, monkeypatch):
    """The kL whose single group carries the partner flags 0, 0, 1, 1: dense, cold and warm are bit-identical, step 1 issues W for the
    two flagged blocks only and step 2 the partner products of those two, none of them folded."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 360), _df(nao)
    w, rec = et.eri_plan(MESH, True)
    kLs = [kL for kL in range(len(w)) if w[kL] > 0 and [int(r[4]) for r in rec if int(r[0]) == kL] == [0, 0, 1, 1]]
    assert kLs
    old = _run(ctx, Ce, df, bufs[0], monkeypatch, strip=False, split=False, kLs=kLs, planes=False)
    dense = _run(ctx, Ce, df, bufs[0], monkeypatch, kLs=kLs)
    assert dense["strip"]
    assert dense["flops"][0] == old["flops"][0] * (1.0 + 0.25 * 2 / 4) == _half1_flops(dense, nao, 256, True)
    assert dense["flops"][1] == _half2_flops(dense, nao, False)
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs)
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs)
        assert cache.stats()["hits"] == len(kLs)
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        for kL in kLs:
            assert np.array_equal(cold["planes"][kL], dense["planes"][kL]) and np.array_equal(warm["planes"][kL], dense["planes"][kL])
        assert warm["flops"][0] == _half1_flops(warm, nao, 64, True) and warm["flops"][1] == _half2_flops(warm, nao, True)
    finally:
        cache.close()


def test_planes_in_the_middle_of_a_kL(ctx, bufs, monkeypatch):
    """dmk_eri_planes after the first of two groups of a kL (the deferred step 2 goes out alone, then the kL goes on): the same
    planes with and without fused launches, in the mode, at that point and at the end."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    from libdmet_preview_amd._lib import lib
    nao, group = 24, 2
    Ce, df = _C(nao, 370), _df(nao)
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    got = {}
    for fuse in (False, True):
        if fuse:
            monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
        else:
            monkeypatch.setenv("DMK_ERI_FUSE", "0")
        bufs[int(fuse)].zero_()
        eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, ctx.to_device(Ce), bufs[int(fuse)], strip_step1=True)
        try:
            assert eng.strip_step1 and eng.split_step1          # the mode implies the split
            kL = [k for k in eng.irreducible_kL() if len(eng.by_kL[k]) == 4 and eng.weights[k] == 2][0]
            ctx.check(lib.dmk_eri_begin_kL_weighted(eng.h, int(kL), int(eng.weights[kL])))
            recs, mid = eng.by_kL[kL], None
            for g0 in range(0, len(recs), group):
                for pos, r in enumerate(recs[g0:g0 + group]):
                    df.load_block(ctx, int(r[1]), int(r[2]), eng.ring[pos])
                    ctx.check(lib.dmk_eri_push_ring_slot(eng.h, int(r[1]), int(r[2]), int(r[4])))
                ctx.check(lib.dmk_eri_flush(eng.h))
                if g0 == 0:
                    mid = eng.planes().get()
            last = eng.planes().get()
            ctx.check(lib.dmk_eri_end_kL(eng.h, int(eng.weights[kL])))
            ctx.sync()
            got[fuse] = (mid, last)
        finally:
            eng.close()
    assert got[False][0].any() and np.array_equal(got[False][0], got[True][0])
    assert np.array_equal(got[False][1], got[True][1]) and not np.array_equal(got[False][0], got[False][1])
    assert got[False][1][..., _strip_mask()].any()
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


def test_freivalds_on_a_warm_fused_stacked_run(ctx, bufs, monkeypatch):
    """eri x against the yref the pipeline accumulates from its planes (stacked, warm, fused, mode on), at the bound of bench.py."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao, group = 24, 2
    Ce, df = _C(nao, 380), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache, stack=True, planes=False)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, NPAIR))
        d_y = ctx.zeros((NBLK, NPAIR), np.float64)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache, stack=True, planes=False, probe=(d_x, d_y))
        assert warm["strip"] and warm["fused"] > 0
        assert cache.stats()["hits"] == cache.stats()["entries"] > 0
        y = et.eri_times_vector_dev(ctx, bufs[1], NBLK, NPAIR, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        d = np.abs(y - yref).max()
        print("Freivalds: %.3e against %.3e" % (d, np.abs(yref).max()))
        assert d <= 1e-10 * max(1.0, np.abs(yref).max()), d
    finally:
        cache.close()


def test_cache_invalidation(ctx, bufs, monkeypatch):
    """A change of the bath columns [192,256) alone hits, and the warm result is the dense one of the new coefficients bit for bit (the
    corner [128,192)^2 of the cached region does not depend on them); a change in column 191 drops every entry."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 390), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[0], monkeypatch, cache=cache, planes=False)
        n = cache.stats()["entries"]
        assert cold["strip"] and n == len(cold["kLs"])
        C2 = Ce.copy()
        C2[..., 192:] = _C(nao, 391)[..., 192:]
        dense = _run(ctx, C2, df, bufs[0], monkeypatch)
        warm = _run(ctx, C2, df, bufs[1], monkeypatch, cache=cache)
        st = cache.stats()
        assert (st["hits"], st["entries"], st["drops"]) == (n, n, 0), st
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        for kL in dense["planes"]:
            assert np.array_equal(warm["planes"][kL], dense["planes"][kL]), kL
        assert warm["flops"][0] == _half1_flops(warm, nao, 64, True)
        C3 = C2.copy()
        C3[0, 0, 0, 191] += 1e-3
        dense3 = _run(ctx, C3, df, bufs[0], monkeypatch, planes=False)
        again = _run(ctx, C3, df, bufs[1], monkeypatch, cache=cache, planes=False)
        st = cache.stats()
        assert (st["hits"], st["drops"], st["entries"]) == (n, n, n), st
        assert again["flops"] == dense3["flops"] and _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    finally:
        cache.close()


def test_entries_of_one_order_are_not_served_to_the_other(ctx, bufs, monkeypatch):
    """One cache, first an engine in the split order alone, then one in the mode, then the split again: each attaches to an empty
    cache (shape tuple)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 400), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[0], monkeypatch, strip=False, cache=cache, planes=False)
        n = cache.stats()["entries"]
        assert n > 0
        _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, planes=False)
        st = cache.stats()
        assert st["hits"] == 0 and st["entries"] == n and st["bytes"] % (REGION * 8) == 0, st
        _run(ctx, Ce, df, bufs[1], monkeypatch, strip=False, cache=cache, planes=False)
        st = cache.stats()
        assert st["hits"] == 0 and st["entries"] == n and st["bytes"] % (16448 * 8) == 0, st
    finally:
        cache.close()


def _spy(monkeypatch, seen, force_strip_off=False):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    real = et.EriEngine

    class Spy(real):
        def __init__(self, *a, **kw):
            if force_strip_off:
                kw["strip_step1"] = False
            real.__init__(self, *a, **kw)
            seen.append((self.split_step1, self.strip_step1, self.inv_attached))
    monkeypatch.setattr(et, "EriEngine", Spy)


def _pipeline_run(ctx, monkeypatch, bufs_by_iteration, force_off=False, **env):
    """Iterations of pipeline.iteration on one 224 + 32 system, iteration i into bufs_by_iteration[i].  Returns what every engine
    reported and the hits of the system's cache (None: it has none)."""
    from libdmet_preview_amd import pipeline
    mesh, nlo, naux, nval = (2, 2, 1), 224, 8, 32
    seen = []
    with monkeypatch.context() as m:
        for k in ("DMK_ERI_INV", "DMK_ERI_SPLIT1", "DMK_ERI_STRIP"):
            m.delenv(k, raising=False)
        _spy(m, seen, force_off)
        for k, v in env.items():
            m.setenv(k, v)
        s = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=11, name="strip")
        for buf in bufs_by_iteration:
            buf.zero_()
            out = pipeline.iteration(ctx, s, eri_dev=buf)
            assert out["nemb"] == 256
        hits = None
        if getattr(s, "eri_inv_cache", None) is not None:
            hits = s.eri_inv_cache.stats()["hits"]
            s.eri_inv_cache.close()
    return seen, hits


def test_pipeline_mode_on_with_and_without_cache(ctx, bufs, monkeypatch):
    """pipeline.eri_stage on a 224 + 32 system whose provider has a token: the mode is on, the second iteration is warm and equals
    the first bit for bit, and the uncached A/B run (DMK_ERI_INV=0) stays in the mode with the same ERI."""
    seen, hits = _pipeline_run(ctx, monkeypatch, [bufs[0], bufs[1]])
    assert seen == [(True, True, True)] * 2 and hits > 0
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    seen, hits = _pipeline_run(ctx, monkeypatch, [bufs[2]], DMK_ERI_INV="0")
    assert seen == [(True, True, False)] and hits is None
    assert _maxabs(ctx, bufs[2], bufs[0]) == 0.0


def test_pipeline_strip_switch(ctx, bufs, monkeypatch):
    """DMK_ERI_STRIP=0 gives the split order alone -- bit for bit what a caller that never passes the strip request computes."""
    seen, _ = _pipeline_run(ctx, monkeypatch, [bufs[0]], DMK_ERI_STRIP="0")
    assert seen == [(True, False, True)]
    seen, _ = _pipeline_run(ctx, monkeypatch, [bufs[1]], force_off=True)
    assert seen == [(True, False, True)]
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


def test_pipeline_caller_that_can_never_go_warm(ctx, bufs, monkeypatch):
    """A 256-orbital system with fewer than 192 impurity columns (160 + 96) never gets a cache, so it never asks for the mode: the
    engine reports it off and the ERI is that of DMK_ERI_STRIP=0 bit for bit."""
    from libdmet_preview_amd import pipeline
    for k in ("DMK_ERI_INV", "DMK_ERI_SPLIT1", "DMK_ERI_STRIP"):
        monkeypatch.delenv(k, raising=False)
    mesh, nlo, naux, nval = (2, 2, 1), 160, 8, 96
    seen = []
    _spy(monkeypatch, seen)
    s = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=13, name="strip-cold")
    bufs[0].zero_()
    out = pipeline.iteration(ctx, s, eri_dev=bufs[0])
    assert out["nemb"] == 256 and len(s.imp_idx) < 192
    assert seen == [(False, False, False)] and getattr(s, "eri_inv_cache", None) is None
    monkeypatch.setenv("DMK_ERI_STRIP", "0")
    s2 = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=13, name="strip-cold-off")
    bufs[1].zero_()
    pipeline.iteration(ctx, s2, eri_dev=bufs[1])
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
