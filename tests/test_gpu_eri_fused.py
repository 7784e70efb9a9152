"""
Fused launches of the ERI half transform (zhot.hip half12_kernel; run with -m gpu on an MI355X): inside a kL the
nemb = 256 path launches step 2 of a group together with step 1 of the next group.  Every workgroup does what it does in the
separate launches, so the reference of every comparison is the same engine with DMK_ERI_FUSE=0 on the same inputs and the
bound is zero: ERIs and planes must be bit-identical.

Shapes: mesh 3 x 2 x 1, naux 24, nemb 256, two spins, nao 24 (on the K tile) and 30 (K padding) -- the smallest the hot kernels
accept.  The default queue (8 blocks) holds a whole kL of this mesh, which leaves nothing to fuse, so every test sets
DMK_ERI_GROUP.  With time reversal the plan has weight-1 and weight-2 kL of 4 and 3 blocks: a queue of 2 cuts them into groups of
2 + 2 and 2 + 1 (one fused launch per kL, for the 3-block kL with a shorter step-1 queue than step-2 queue); a queue of 4 holds a
whole kL (nothing fuses).  Without time reversal every kL has 6 blocks: a queue of 2 gives three groups (two fused launches per
kL, through both halves of Ut and back), a queue of 4 two groups of 3 (the engine sends groups of equal length) and, with the
visiting list cut to 5 blocks, groups of 3 and 2.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eri_sample as ES                  # the checker

MESH, NK, NAUX, NEMB, SPIN = (3, 2, 1), 6, 24, 256, 2
NPAIR = NEMB * (NEMB + 1) // 2
NBLK = SPIN * (SPIN + 1) // 2


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@pytest.fixture(scope="module")
def bufs(ctx):
    """Two ERI buffers shared by every test of the module (zeroed before each transform)."""
    b = [ctx.zeros((NBLK, NPAIR, NPAIR), np.float64) for _ in range(2)]
    yield b
    for x in b:
        x.free()


def _C(nao, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((SPIN, NK, nao, NEMB)) + 1j * rng.standard_normal((SPIN, NK, nao, NEMB))) / np.sqrt(nao)


def _df(nao, seed=5):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((NK, 3)), NAUX, nao, seed=seed)


def _same(ctx, a, b):
    """Do two device arrays hold the same values?  (One reduction on the device.)"""
    from libdmet_preview_amd._lib import lib
    ss = ctx.zeros((1,), np.float64)
    ctx.check(lib.dmk_sub_sumsq(ctx.h, a.size, a.ptr, b.ptr, None, ss.ptr))
    return float(ss.get()[0]) == 0.0


def _groups(nblocks, queue):
    """Groups the engine cuts a kL of `nblocks` into with a queue of `queue` slots (EriEngine.run_kL: equal lengths)."""
    if nblocks <= queue:
        return 1
    per = -(-nblocks // -(-nblocks // queue))
    return -(-nblocks // per)


def _run(ctx, Ce, df, eri_dev, monkeypatch, fuse, group, cache=None, max_blocks=None, planes=True, probe=None, stack=False, tr=True):
    """One whole transform with DMK_ERI_FUSE / DMK_ERI_GROUP set before the engine exists.  Returns the planes of every kL, the
    fused launches of every kL and the launch counts / executed flop of both half-transform families."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    if fuse:
        monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
    else:
        monkeypatch.setenv("DMK_ERI_FUSE", "0")
    nao = Ce.shape[2]
    eri_dev.zero_()
    C_dev = ctx.to_device(Ce)
    eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, C_dev, eri_dev, inv_cache=cache, t_reversal_symm=tr)
    out = {"planes": {}, "fused": {}, "weights": eng.weights, "by_kL": eng.by_kL, "attached": eng.inv_attached}
    try:
        assert eng.ring_slots == group
        if stack:
            eng.set_stack(n_kL=len(eng.irreducible_kL()))
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        ctx.profile_read(reset=True)
        ctx.profile_read_flops(reset=True)
        for kL in eng.irreducible_kL():
            before = eng.fused_launches
            eng.run_kL(kL, df, max_blocks=max_blocks)
            out["fused"][kL] = eng.fused_launches - before
            if planes:
                out["planes"][kL] = eng.planes().get()
        eng.contract()
        ctx.sync()
        out["fused_total"] = eng.fused_launches
        prof, flops = ctx.profile_read(reset=True), ctx.profile_read_flops(reset=True)
        out["launches"] = (prof["zgemm_half1"][1], prof["zgemm_half2"][1])
        out["flops"] = (flops["zgemm_half1"], flops["zgemm_half2"])
    finally:
        eng.close()
    return out


def _expected_fused(run, group, max_blocks=None):
    return {kL: _groups(len(r) if max_blocks is None else min(len(r), max_blocks), group) - 1
            for kL, r in run["by_kL"].items() if run["weights"][kL] > 0}


def _assert_planes_equal(got, ref, what):
    assert sorted(got) == sorted(ref)
    for kL in ref:
        assert np.array_equal(got[kL], ref[kL]), (what, kL, float(np.abs(got[kL] - ref[kL]).max()))


def _half2_flops(run, nao, warm):
    """Executed flop of step 2 as the launcher counts it (tests/test_gpu_eri_invariant.py), summed over the groups of every kL:
    per queued block 136 (+ 120 | 136 partner) block products dense, 68 (+ 60 | 68) warm; the diagonal blocks of the partner term
    are folded when every block of a GROUP carries it; weight-1 kL run the real-part-only product (4 instead of 6)."""
    kdim = (nao + 7) // 8 * 8
    total = 0.0
    for kL, recs in run["by_kL"].items():
        if run["weights"][kL] <= 0:
            continue
        sym = [int(r[4]) for r in recs]
        ngrp = _groups(len(sym), run["group"])
        per = -(-len(sym) // ngrp)
        for g0 in range(0, len(sym), per):
            grp = sym[g0:g0 + per]
            fold = all(grp)
            full, part = (68.0, 60.0 if fold else 68.0) if warm else (136.0, 120.0 if fold else 136.0)
            blocks = sum(full + (part if s else 0.0) for s in grp)
            total += (4.0 if run["weights"][kL] == 1 else 6.0) * blocks * 256.0 * kdim * NAUX * SPIN
    return total


def test_plan_and_group_cut():
    """The block counts the cases above rest on (host only)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    w, rec = et.eri_plan(MESH, True)
    assert 1 in set(int(x) for x in w) and 2 in set(int(x) for x in w)
    assert sorted(sum(1 for r in rec if int(r[0]) == kL) for kL in range(len(w)) if w[kL] > 0) == [3, 3, 4, 4]
    w, rec = et.eri_plan(MESH, False)
    assert [sum(1 for r in rec if int(r[0]) == kL) for kL in range(len(w)) if w[kL] > 0] == [6] * 6
    assert [_groups(*a) for a in ((6, 2), (6, 4), (5, 4), (4, 2), (3, 2), (4, 4), (2, 2), (6, 8))] == [3, 2, 2, 2, 2, 1, 1, 1]


@pytest.mark.parametrize("nao,group,tr,max_blocks", [(24, 2, True, None), (30, 2, True, None), (24, 4, True, None), (30, 4, True, None),
                                                    (24, 2, False, None), (30, 2, False, None), (24, 4, False, None),
                                                    (30, 4, False, None), (30, 4, False, 5)])
def test_fused_equals_unfused(ctx, bufs, monkeypatch, nao, group, tr, max_blocks):
    """Fusing on: one fused launch per group after the first of every kL; off: none.  ERI, planes, launch counts and executed flop
    of both families are the same in both modes."""
    Ce, df = _C(nao, 20 + nao + group), _df(nao)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, False, group, max_blocks=max_blocks, tr=tr)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, max_blocks=max_blocks, tr=tr)
    want = _expected_fused(on, group, max_blocks)
    assert (sum(want.values()) > 0) == (not (tr and group == 4))      # a queue of 4 holds a whole kL of the time-reversal plan
    assert on["fused"] == want and on["fused_total"] == sum(want.values())
    assert off["fused_total"] == 0 and not any(off["fused"].values())
    assert _same(ctx, bufs[1], bufs[0])
    _assert_planes_equal(on["planes"], off["planes"], "fused vs separate")
    ngroups = sum(v + 1 for v in want.values())
    assert on["launches"] == off["launches"] == (ngroups, ngroups)
    assert on["flops"] == off["flops"] and min(on["flops"]) > 0.0


@pytest.mark.parametrize("nao", [24, 30])
def test_cold_and_warm_cache_fused(ctx, bufs, monkeypatch, nao):
    """With EriInvariantCache, fused: cold and warm ERIs and planes equal the dense, unfused run bit for bit; every kL hits; the
    warm call fuses (skip_invariant through half12_kernel), also on weight-1 kL (the RE instantiation: their Im planes stay zero
    and the family reports the real-part-only flop); nao 24: the sampled oracle at 1e-8."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    group = 2
    Ce, df = _C(nao, 40 + nao), _df(nao)
    ref = _run(ctx, Ce, df, bufs[0], monkeypatch, False, group)
    n_kL = len(ref["planes"])
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, cache=cache)
        assert cold["attached"]
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, n_kL, n_kL), st
        assert _same(ctx, bufs[1], bufs[0])
        _assert_planes_equal(cold["planes"], ref["planes"], "cold")
        assert cold["fused"] == _expected_fused(cold, group)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, cache=cache)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["drops"]) == (n_kL, n_kL, 0), st
        assert _same(ctx, bufs[1], bufs[0])
        _assert_planes_equal(warm["planes"], ref["planes"], "warm")
        assert warm["fused_total"] > 0 and warm["fused"] == _expected_fused(warm, group)
        w1 = [kL for kL in warm["planes"] if warm["weights"][kL] == 1]
        assert w1
        for kL in w1:
            assert warm["fused"][kL] > 0
            assert not warm["planes"][kL][:, 1].any()            # Im planes of a real-part-only kL
            assert warm["planes"][kL][:, 0].any()
        for r in (ref, cold, warm):
            r["group"] = group
        assert ref["flops"][1] == cold["flops"][1] == _half2_flops(ref, nao, False)
        assert warm["flops"][1] == _half2_flops(warm, nao, True)
        assert warm["flops"][0] == ref["flops"][0] and warm["launches"] == ref["launches"]
        if nao == 24:
            A = [0, 1, 127, 128, 191, 192, 255]
            want, idx, _ = ES.eri_sample(MESH, 5, Ce, NAUX, A, sorted(ref["planes"]))
            for blk in range(NBLK):
                got = np.stack([bufs[1].offset((blk * NPAIR + int(r)) * NPAIR, (NPAIR,)).get()[idx] for r in idx])
                assert np.abs(got - want[blk]).max() < 1e-8
    finally:
        cache.close()


def test_resident_and_ring_feed(ctx, bufs, monkeypatch):
    """Blocks read in place (GDFResident, dmk_eri_push_resident) and blocks generated into the ring give the same ERI, and both
    feeds fuse."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao, group = 30, 2
    Ce, df = _C(nao, 61), _df(nao)
    ring = _run(ctx, Ce, df, bufs[0], monkeypatch, True, group, planes=False)
    res = et.GDFResident(ctx, df, MESH, nao, NAUX)
    try:
        resident = _run(ctx, Ce, res, bufs[1], monkeypatch, True, group, planes=False)
    finally:
        res.free()
    want = _expected_fused(ring, group)
    assert ring["fused"] == want and resident["fused"] == want and sum(want.values()) > 0
    assert _same(ctx, bufs[1], bufs[0])
    assert resident["launches"] == ring["launches"] and resident["flops"] == ring["flops"]


def _drive_kL(ctx, eng, df, kL, group, look_after):
    """One kL fed group by group through the ring; returns the planes after `look_after` flushed groups and at the end of the
    queue (before the kL is closed)."""
    from libdmet_preview_amd._lib import lib
    ctx.check(lib.dmk_eri_begin_kL_weighted(eng.h, int(kL), int(eng.weights[kL])))
    recs, mid, ngrp = eng.by_kL[kL], None, 0
    for g0 in range(0, len(recs), group):
        for pos, r in enumerate(recs[g0:g0 + group]):
            df.load_block(ctx, int(r[1]), int(r[2]), eng.ring[pos])
            ctx.check(lib.dmk_eri_push_ring_slot(eng.h, int(r[1]), int(r[2]), int(r[4])))
        ctx.check(lib.dmk_eri_flush(eng.h))
        ngrp += 1
        if ngrp == look_after:
            mid = eng.planes().get()
    last = eng.planes().get()
    ctx.check(lib.dmk_eri_end_kL(eng.h, int(eng.weights[kL])))
    return mid, last


def test_mid_kL_drain(ctx, bufs, monkeypatch):
    """planes() in the middle of a kL, after an odd number of flushed groups: the deferred step 2 goes out alone and the planes
    are those of the unfused engine at the same point; the kL then goes on fusing."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao, group = 24, 2
    Ce, df = _C(nao, 71), _df(nao)
    monkeypatch.setenv("DMK_ERI_GROUP", str(group))
    got = {}
    for fuse in (False, True):
        if fuse:
            monkeypatch.delenv("DMK_ERI_FUSE", raising=False)
        else:
            monkeypatch.setenv("DMK_ERI_FUSE", "0")
        bufs[int(fuse)].zero_()
        eng = et.EriEngine(ctx, MESH, nao, NAUX, NEMB, SPIN, ctx.to_device(Ce), bufs[int(fuse)], t_reversal_symm=False)
        try:
            kLs = eng.irreducible_kL()
            assert len(eng.by_kL[kLs[0]]) == len(eng.by_kL[kLs[1]]) == 6          # three groups each
            got[fuse] = [_drive_kL(ctx, eng, df, kLs[0], group, 1), _drive_kL(ctx, eng, df, kLs[1], group, 3)]
            ctx.sync()
            # first kL: group 1 drained alone, group 2 launched alone, group 3 fused; second: two fused launches, the look comes last
            assert eng.fused_launches == (1 + 2 if fuse else 0)
        finally:
            eng.close()
    for (mid_a, last_a), (mid_b, last_b) in zip(got[False], got[True]):
        assert mid_a.any() and np.array_equal(mid_a, mid_b)
        assert np.array_equal(last_a, last_b)
    assert _same(ctx, bufs[1], bufs[0])


def test_single_group_per_kL_never_fuses(ctx, bufs, monkeypatch):
    """A visiting list cut to one group per kL: nothing to fuse, the result is that of the unfused engine."""
    nao, group = 24, 2
    Ce, df = _C(nao, 81), _df(nao)
    off = _run(ctx, Ce, df, bufs[0], monkeypatch, False, group, max_blocks=2)
    on = _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, max_blocks=2)
    assert on["fused_total"] == 0 and off["fused_total"] == 0
    assert _same(ctx, bufs[1], bufs[0])
    _assert_planes_equal(on["planes"], off["planes"], "one group per kL")
    assert on["launches"] == off["launches"] and on["flops"] == off["flops"]


def test_freivalds_on_a_fused_warm_call(ctx, bufs, monkeypatch):
    """eri x against the yref the pipeline accumulates from its planes (stacked run, warm cache, fused), at the bound of bench.py."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao, group = 30, 2
    Ce, df = _C(nao, 91), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, cache=cache, stack=True, planes=False)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, NPAIR))
        d_y = ctx.zeros((NBLK, NPAIR), np.float64)
        warm = _run(ctx, Ce, df, bufs[1], monkeypatch, True, group, cache=cache, stack=True, planes=False, probe=(d_x, d_y))
        assert cache.stats()["hits"] == cache.stats()["entries"] > 0
        assert warm["fused_total"] == sum(_expected_fused(warm, group).values()) > 0
        y = et.eri_times_vector_dev(ctx, bufs[1], NBLK, NPAIR, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        assert np.abs(y - yref).max() <= 1e-10 * max(1.0, np.abs(yref).max()), np.abs(y - yref).max()
    finally:
        cache.close()
