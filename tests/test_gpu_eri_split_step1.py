"""
Split step 1 of the ERI half transform (EriEngine(split_step1=True), dmk_eri_begin flag 8; run with -m gpu on an
MI355X): the time-reversal partner term of the type-1 workgroups of step 2 (plane rows [192,256) x columns [0,128)) is summed as
sum_p W[p][a] conj(C_i[p][b]) with W[L][p][a] = sum_q Lpq[L][p][q] C_j[q][a], for every kL of the transform, and a kL whose invariant
region came from the cache runs step 1 over columns [128,256) only.

Shapes: those of tests/test_gpu_eri_invariant.py -- mesh 3 x 2 x 1 (weight-1 and weight-2 kL; its time-reversal plan has blocks
without the partner term, alone in a group and mixed with others), nemb 256, two spins, queue of 8 (2 and 4 where a kL must be cut
into groups), nao 24 / 40 on the K tile and 30 off it.  naux is 24 as there: the hot step-1 kernel wants naux * nao >= 512 rows, so
naux 8 only serves the pipeline tests, whose nao is 224 / 160.

Without time reversal no block carries the partner term and no cache can attach, so the engine cannot grant the mode there: that
case is checked as "reports off, result unchanged".  The paths the issue names under it -- blocks with sym == 0 and mixed partner
flags in one group, in the W kernel and in the split step 2 -- run through the time-reversal plan of this mesh, which has both
(test_plan_has_blocks_without_partner, test_mixed_group_issues_W_flop_for_flagged_blocks_only).

Bounds.  Inside the mode: the dense run is made twice; where the two are bit-identical every cached run must equal it bit for bit,
otherwise 4 x their difference.  Mode against the old order: entries outside rows [192,256) x columns [0,128) of every plane are
bit-identical (nothing that computes them changed); the entries inside are the same sum in another order and are held to the
project's oracle tolerance, 1e-8 (measured: see profiles/eri_split_step1_notes.txt).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eri_sample as ES                  # the checker

MESH, NK, NAUX, NEMB, SPIN = (3, 2, 1), 6, 24, 256, 2
NPAIR = NEMB * (NEMB + 1) // 2
NBLK = SPIN * (SPIN + 1) // 2
ORBS = [0, 1, 127, 128, 191, 192, 255]


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


def _run(ctx, Ce, df, eri_dev, monkeypatch, split=True, group=8, fuse=True, cache=None, planes=True, stack=False, probe=None, tr=True,
         kLs=None):
    """One whole transform.  Returns the mode the engine reports, the planes of every kL, the cache attach flag, the fused launches
    and the launch counts / executed flop of both half-transform families."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    if fuse:
        monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
    else:
        monkeypatch.setenv("DMK_ERI_FUSE", "0")
    nao = Ce.shape[2]
    eri_dev.zero_()
    eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, ctx.to_device(Ce), eri_dev, inv_cache=cache, t_reversal_symm=tr,
                       split_step1=split)
    out = {"split": eng.split_step1, "planes": {}, "weights": eng.weights, "by_kL": eng.by_kL, "attached": eng.inv_attached,
           "group": group}
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


def _half2_flops(run, nao, warm):
    """Executed flop of step 2 as launch_half2_hot counts it (tests/test_gpu_eri_fused.py): 136 (+ 120 | 136) block products per
    block dense, 68 (+ 60 | 68) warm."""
    total = 0.0
    for kL, grp in _groups(run):
        fold = all(grp)
        full, part = (68.0, 60.0 if fold else 68.0) if warm else (136.0, 120.0 if fold else 136.0)
        blocks = sum(full + (part if s else 0.0) for s in grp)
        total += (4.0 if run["weights"][kL] == 1 else 6.0) * blocks * 256.0 * nao * NAUX * SPIN
    return total


def _half1_flops(run, nao, ut_cols, w):
    """Executed flop of step 1: 128 x 64 tiles over the flat rows of a block, `ut_cols` columns of Ut for every block and (w) the 64
    columns of W for every block with the partner term."""
    tiles_m = -(-NAUX * nao // 128)
    total = 0.0
    for kL, grp in _groups(run):
        cols = sum(ut_cols + (64 if (w and s) else 0) for s in grp)
        total += 6.0 * tiles_m * 128 * cols * nao * SPIN
    return total


def _region_mask():
    """Pair indices of rows [192,256) x columns [0,128)."""
    m = np.zeros(NPAIR, bool)
    for a in range(192, 256):
        m[a * (a + 1) // 2: a * (a + 1) // 2 + 128] = True
    return m


def test_plan_has_blocks_without_partner():
    """The time-reversal plan of this mesh has a group of blocks without the partner term, mixed groups and full ones (host only)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    w, rec = et.eri_plan(MESH, True)
    sym = {kL: [int(r[4]) for r in rec if int(r[0]) == kL] for kL in range(len(w)) if w[kL] > 0}
    assert any(0 < sum(s) < len(s) for s in sym.values()) and any(all(s) for s in sym.values())
    assert sorted(int(w[k]) for k in sym) == [1, 1, 2, 2]


@pytest.mark.parametrize("nao", [24, 40, 30])
def test_cold_warm_dense(ctx, bufs, monkeypatch, nao):
    """Mode on: dense twice, then cold and warm with the cache against dense (ERI and planes of every kL), every kL hits, the K6j
    block hits on a warm stacked run, flop accounting of both families; nao 24: the sampled oracle on dense and on warm.  nao 30 is
    off the K tile: the engine declines the mode for the whole transform and computes the old order bit for bit."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    Ce, df = _C(nao, 100 + nao), _df(nao)
    old = _run(ctx, Ce, df, bufs[2], monkeypatch, split=False)
    assert not old["split"]
    ref = _run(ctx, Ce, df, bufs[0], monkeypatch)
    if nao == 30:
        assert not ref["split"]
        assert _maxabs(ctx, bufs[0], bufs[2]) == 0.0
        for kL in old["planes"]:
            assert np.array_equal(ref["planes"][kL], old["planes"][kL])
        assert ref["flops"] == old["flops"]
        return
    assert ref["split"]
    again = _run(ctx, Ce, df, bufs[1], monkeypatch)
    noise = _maxabs(ctx, bufs[1], bufs[0])
    print("dense vs dense, mode on: %.3e" % noise)
    _assert_planes(again["planes"], ref["planes"], noise, "dense again")
    n_kL = len(ref["planes"])
    A = ORBS
    if nao == 24:
        want, idx, _ = ES.eri_sample(MESH, 5, Ce, NAUX, A, sorted(ref["planes"]))

        def oracle(buf, what):
            for blk in range(NBLK):
                got = np.stack([buf.offset((blk * NPAIR + int(r)) * NPAIR, (NPAIR,)).get()[idx] for r in idx])
                d = np.abs(got - want[blk]).max()
                print("%s, spin block %d: against the sampled oracle %.3e" % (what, blk, d))
                assert d < 1e-8
        oracle(bufs[0], "dense")
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache)
        assert cold["split"] and cold["attached"]
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], noise, "cold")
        _assert_planes(cold["planes"], ref["planes"], noise, "cold")
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"], st["drops"]) == (n_kL, n_kL, n_kL, 0), st
        assert st["bytes"] == sum(SPIN * (1 if ref["weights"][k] == 1 else 2) * NAUX * 16448 * 8 for k in ref["planes"])
        _assert_same(ctx, bufs[1], bufs[0], noise, "warm")
        _assert_planes(warm["planes"], ref["planes"], noise, "warm")
        if nao == 24:
            oracle(bufs[1], "warm")
        # flop accounting: step 2 as before, step 1 follows the tiles launched
        assert old["flops"][1] == ref["flops"][1] == cold["flops"][1] == _half2_flops(ref, nao, False)
        assert warm["flops"][1] == _half2_flops(warm, nao, True)
        assert old["flops"][0] == _half1_flops(old, nao, 256, False)
        assert ref["flops"][0] == cold["flops"][0] == _half1_flops(ref, nao, 256, True)
        assert warm["flops"][0] == _half1_flops(warm, nao, 128, True)
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
    """On the kL whose blocks all carry the partner term (one of weight 1, one of weight 2): step 1 of a warm run issues 0.75 x the
    flop of the old dense run, a dense run in the mode 1.25 x; step 2 counts 68 / 60 warm and 136 / 120 dense block products."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 131), _df(nao)
    w, rec = et.eri_plan(MESH, True)
    kLs = [kL for kL in range(len(w)) if w[kL] > 0 and all(int(r[4]) for r in rec if int(r[0]) == kL)]
    assert sorted(int(w[k]) for k in kLs) == [1, 2]
    old = _run(ctx, Ce, df, bufs[0], monkeypatch, split=False, kLs=kLs, planes=False)
    dense = _run(ctx, Ce, df, bufs[0], monkeypatch, kLs=kLs, planes=False)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs, planes=False)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, cache=cache, kLs=kLs, planes=False)
        assert cache.stats()["hits"] == len(kLs)
    finally:
        cache.close()
    assert dense["split"] and warm["split"] and old["flops"][0] > 0
    assert warm["flops"][0] == 0.75 * old["flops"][0]
    assert dense["flops"][0] == 1.25 * old["flops"][0]
    assert dense["flops"][1] == old["flops"][1] == _half2_flops(old, nao, False)
    assert warm["flops"][1] == _half2_flops(warm, nao, True)
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


@pytest.mark.parametrize("nao", [24, 40])
def test_mode_on_against_mode_off(ctx, bufs, monkeypatch, nao):
    """Planes of both orders: bit-identical outside rows [192,256) x columns [0,128); inside, the same sum in another order, within
    the oracle tolerance.  A weight-1 kL (the real-part-only instantiation) keeps its Im planes zero."""
    Ce, df = _C(nao, 140 + nao), _df(nao)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, split=False)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch)
    assert on["split"] and not off["split"]
    inside = _region_mask()
    worst, scale = 0.0, 0.0
    for kL in off["planes"]:
        a, b = on["planes"][kL], off["planes"][kL]
        assert np.array_equal(a[..., ~inside], b[..., ~inside]), kL
        worst = max(worst, float(np.abs(a[..., inside] - b[..., inside]).max()))
        scale = max(scale, float(np.abs(b[..., inside]).max()))
        if on["weights"][kL] == 1:
            assert not a[:, 1].any() and a[:, 0][..., inside].any()
    print("nao %d: rows [192,256) x cols [0,128), mode on vs off: max |difference| %.3e (entries up to %.3e)" % (nao, worst, scale))
    assert worst <= 1e-8
    d = _maxabs(ctx, bufs[1], bufs[0])
    print("nao %d: ERI, mode on vs off: %.3e" % (nao, d))
    assert d <= 1e-8


@pytest.mark.parametrize("group", [2, 4])
def test_fused_equals_unfused_and_queue_lengths(ctx, bufs, monkeypatch, group):
    """Queues of 2 and 4 cut a kL into several groups (both halves of Ut and of W in use with 2): fused and DMK_ERI_FUSE=0 runs are
    bit-identical, and both equal the run with the whole kL in one group, dense and warm."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 150), _df(nao)
    one = _run(ctx, Ce, df, bufs[2], monkeypatch)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, group=group, fuse=False)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group)
    assert on["split"] and off["split"] and off["fused"] == 0
    assert (on["fused"] > 0) == (group == 2)
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
        assert warm["flops"][0] == _half1_flops(warm, nao, 128, True)
    finally:
        cache.close()
    # another cut of the queue changes the order of the sum over the blocks of a kL: the bound of the dense-vs-dense rule does not
    # apply across cuts, the oracle tolerance does
    assert _maxabs(ctx, bufs[0], bufs[2]) <= 1e-8
    assert one["split"]


def test_without_time_reversal_the_mode_is_off(ctx, bufs, monkeypatch):
    """No partner term anywhere and no cache to go warm from: the engine reports the mode off and computes what it computed."""
    nao = 24
    Ce, df = _C(nao, 160), _df(nao)
    a = _run(ctx, Ce, df, bufs[0], monkeypatch, split=False, group=2, tr=False, planes=False)
    b = _run(ctx, Ce, df, bufs[1], monkeypatch, split=True, group=2, tr=False, planes=False)
    assert not a["split"] and not b["split"]
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0 and a["flops"] == b["flops"]


def test_planes_in_the_middle_of_a_kL(ctx, bufs, monkeypatch):
    """dmk_eri_planes after the first of two groups of a kL (the deferred step 2 goes out alone, then the kL goes on): the same
    planes with and without fused launches, in the mode, at that point and at the end."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    from libdmet_preview_amd._lib import lib
    nao, group = 24, 2
    Ce, df = _C(nao, 170), _df(nao)
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    got = {}
    for fuse in (False, True):
        if fuse:
            monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
        else:
            monkeypatch.setenv("DMK_ERI_FUSE", "0")
        bufs[int(fuse)].zero_()
        eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, ctx.to_device(Ce), bufs[int(fuse)], split_step1=True)
        try:
            assert eng.split_step1
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
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


def test_freivalds_on_a_warm_fused_stacked_run(ctx, bufs, monkeypatch):
    """eri x against the yref the pipeline accumulates from its planes (stacked, warm, fused, mode on), at the bound of bench.py."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao, group = 24, 2
    Ce, df = _C(nao, 180), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache, stack=True, planes=False)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, NPAIR))
        d_y = ctx.zeros((NBLK, NPAIR), np.float64)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, group=group, cache=cache, stack=True, planes=False, probe=(d_x, d_y))
        assert warm["split"] and warm["fused"] > 0
        assert cache.stats()["hits"] == cache.stats()["entries"] > 0
        y = et.eri_times_vector_dev(ctx, bufs[1], NBLK, NPAIR, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        d = np.abs(y - yref).max()
        print("Freivalds: %.3e against %.3e" % (d, np.abs(yref).max()))
        assert d <= 1e-10 * max(1.0, np.abs(yref).max()), d
    finally:
        cache.close()


def test_entries_of_one_order_are_not_served_to_the_other(ctx, bufs, monkeypatch):
    """One cache, first an engine in the old order, then one in the mode: the second attaches to an empty cache (shape tuple)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 190), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[0], monkeypatch, split=False, cache=cache, planes=False)
        n = cache.stats()["entries"]
        assert n > 0
        _run(ctx, Ce, df, bufs[1], monkeypatch, split=True, cache=cache, planes=False)
        st = cache.stats()
        assert st["hits"] == 0 and st["entries"] == n, st
    finally:
        cache.close()


class _NoToken(object):
    """A provider that cannot promise an immutable tensor."""
    def __init__(self, df):
        self._df = df

    def __getattr__(self, name):
        if name == "df_token":
            raise AttributeError(name)
        return getattr(self._df, name)


def test_pipeline_switches(ctx, bufs, monkeypatch):
    """pipeline.eri_stage on a 224 + 32 system: a provider with a token runs the mode, with or without DMK_ERI_INV; one without a
    token runs the old order; DMK_ERI_SPLIT1=0 gives the old order's ERI bit for bit."""
    from libdmet_preview_amd import pipeline
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.delenv("DMK_ERI_INV", raising=False)
    monkeypatch.delenv("DMK_ERI_SPLIT1", raising=False)
    mesh, nlo, naux, nval = (2, 2, 1), 224, 8, 32
    seen = []
    real = et.EriEngine

    class Spy(real):
        def __init__(self, *a, **kw):
            real.__init__(self, *a, **kw)
            seen.append(self.split_step1)
    monkeypatch.setattr(et, "EriEngine", Spy)

    def run(buf, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=11, name="split1")
        buf.zero_()
        del seen[:]
        out = pipeline.iteration(ctx, s, eri_dev=buf)
        assert out["nemb"] == 256
        for k in env:
            monkeypatch.delenv(k)
        if getattr(s, "eri_inv_cache", None) is not None:
            s.eri_inv_cache.close()
        return list(seen), s

    assert run(bufs[0])[0] == [True]
    assert run(bufs[1], DMK_ERI_INV="0")[0] == [True]
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    assert run(bufs[2], DMK_ERI_SPLIT1="0")[0] == [False]
    d = _maxabs(ctx, bufs[2], bufs[0])
    print("pipeline ERI, mode on vs DMK_ERI_SPLIT1=0: %.3e" % d)
    assert 0.0 < d <= 1e-8
    # the old order again, through a provider without a token: bit for bit the DMK_ERI_SPLIT1=0 result
    s = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=11, name="split1-notoken")
    s.df = _NoToken(s.df)
    if getattr(s, "df_resident", None) is not None:
        s.df_resident = None
    bufs[1].zero_()
    del seen[:]
    pipeline.iteration(ctx, s, eri_dev=bufs[1])
    assert seen == [False]
    assert _maxabs(ctx, bufs[1], bufs[2]) == 0.0


def test_pipeline_caller_that_can_never_go_warm(ctx, bufs, monkeypatch):
    """A 256-orbital system with fewer than 192 impurity columns (160 + 96) never gets a cache, so it must not ask for the mode: the
    engine reports it off and the ERI is that of DMK_ERI_SPLIT1=0 bit for bit."""
    from libdmet_preview_amd import pipeline
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.delenv("DMK_ERI_INV", raising=False)
    monkeypatch.delenv("DMK_ERI_SPLIT1", raising=False)
    mesh, nlo, naux, nval = (2, 2, 1), 160, 8, 96
    seen = []
    real = et.EriEngine

    class Spy(real):
        def __init__(self, *a, **kw):
            real.__init__(self, *a, **kw)
            seen.append((self.split_step1, self.inv_attached))
    monkeypatch.setattr(et, "EriEngine", Spy)
    s = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=13, name="split1-cold")
    bufs[0].zero_()
    out = pipeline.iteration(ctx, s, eri_dev=bufs[0])
    assert out["nemb"] == 256 and len(s.imp_idx) < 192
    assert seen == [(False, False)] and getattr(s, "eri_inv_cache", None) is None
    monkeypatch.setenv("DMK_ERI_SPLIT1", "0")
    s2 = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=13, name="split1-cold-off")
    bufs[1].zero_()
    pipeline.iteration(ctx, s2, eri_dev=bufs[1])
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0


def test_mixed_group_issues_W_flop_for_flagged_blocks_only(ctx, bufs, monkeypatch):
    """The kL whose single group mixes blocks with and without the partner term (flags 0, 0, 1, 1): the dense run in the mode issues
    the old step-1 flop plus 64 columns of W for the two flagged blocks, nothing for the other two."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 200), _df(nao)
    w, rec = et.eri_plan(MESH, True)
    kLs = [kL for kL in range(len(w)) if w[kL] > 0 and 0 < sum(int(r[4]) for r in rec if int(r[0]) == kL) < sum(1 for r in rec if int(r[0]) == kL)]
    assert kLs
    old = _run(ctx, Ce, df, bufs[0], monkeypatch, split=False, kLs=kLs, planes=False)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch, kLs=kLs, planes=False)
    assert on["split"]
    nblk = sum(len(g) for _, g in _groups(on))
    nsym = sum(sum(g) for _, g in _groups(on))
    assert 0 < nsym < nblk
    assert on["flops"][0] == old["flops"][0] * (1.0 + 0.25 * nsym / nblk) == _half1_flops(on, nao, 256, True)
