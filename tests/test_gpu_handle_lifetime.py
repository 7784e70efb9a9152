"""
Lifetime of the device resources behind the dmk_eri, dmk_eri_cache and dmk_dfjk handles (run with -m gpu on an MI355X).

Every resource a handle creates lazily -- the host feed (copy stream, events, staging blocks, the transposed block), the block ring
and its producer stream, the imaginary-part buffer, a replaced plane buffer, the second half of Ut and W, the entries and the block of
the invariant cache, the workspaces of the J/K build -- is built and released once per round, one pipeline per case.  The loop and the
bound are those of test_engines_with_padded_geometry_give_their_memory_back (tests/test_gpu_production.py): 10 warm-up rounds, 30
measured ones, ctx.sync(), ctx.trim() and mem_info() after each; the free device memory after the last round is no more than 1 MiB
below the mark after round 10.  Only the public ABI and EriEngine are used.

Shapes.  Table path: the off-tile shape of that test (mesh 2 x 2 x 1, nao 27, naux 45, nemb 41, two spins).  nemb = 256: mesh
3 x 2 x 1, naux 24, with nao 16 and nao 24.  At nao 16 the hot step-1 kernel declines the shape (naux nao = 384 rows, it wants
512), so that pipeline has no queue and runs the generic kernels; nao 24 is the smallest shape on which fused launches and the split
step 1 exist, and the case asserts that both are on.  The nemb = 256 pipelines are rows-only or have one spin: no round allocates
the three-block ERI; the one-spin ERI (8.7 GB) is allocated once for the module.
"""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAB = {"mesh": (2, 2, 1), "nk": 4, "nao": 27, "naux": 45, "nemb": 41, "spin": 2}
HOT = {"mesh": (3, 2, 1), "nk": 6, "naux": 24, "nemb": 256}
WARMUP, MEASURED, BOUND = 10, 30, 1 << 20


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _coeff(seed, spin, nk, nao, nemb):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((spin, nk, nao, nemb)) + 1j * rng.standard_normal((spin, nk, nao, nemb))) / np.sqrt(nao)


def _philox(nk, naux, nao, seed=3):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((nk, 3)), naux, nao, seed=seed)


def _rounds(ctx, body, what):
    """The loop of the existing test around `body(round)`; returns (mark after the warm-up, free after the last round)."""
    mark = free = None
    for it in range(WARMUP + MEASURED):
        body(it)
        ctx.sync()
        ctx.trim()
        free, _ = ctx.mem_info()
        if it == WARMUP - 1:
            mark = free
    print("%s: free after round %d: %d, after round %d: %d, lost %d bytes" % (what, WARMUP, mark, WARMUP + MEASURED, free, mark - free))
    return mark, free


@pytest.fixture(scope="module")
def shared(ctx):
    """What the rounds reuse and never free: inputs, output buffers, two host blocks."""
    t = TAB
    npair_t = t["nemb"] * (t["nemb"] + 1) // 2
    npair_h = HOT["nemb"] * (HOT["nemb"] + 1) // 2
    df = _philox(t["nk"], t["naux"], t["nao"])
    buf = ctx.empty((t["naux"], t["nao"], t["nao"]), np.complex128)
    host = []
    for i, j in ((0, 0), (1, 0)):
        df.load_block(ctx, i, j, buf)
        host.append(np.ascontiguousarray(buf.get()))
    buf.free()
    rng = np.random.default_rng(11)
    nk = 2
    dm = rng.standard_normal((2, nk, t["nao"], t["nao"])) + 1j * rng.standard_normal((2, nk, t["nao"], t["nao"]))
    s = {
        "C_tab": _coeff(0, t["spin"], t["nk"], t["nao"], t["nemb"]),
        "C_hot": {nao: _coeff(nao, 2, HOT["nk"], nao, HOT["nemb"]) for nao in (16, 24)},
        "eri_tab": ctx.zeros((3, npair_t, npair_t), np.float64),
        "eri_hot": ctx.zeros((1, npair_h, npair_h), np.float64),
        "df_tab": df,
        "host": host,
        "jk_dm": ctx.to_device(dm),
        "jk_vj": ctx.empty(dm.shape, np.complex128),
        "jk_vk": ctx.empty(dm.shape, np.complex128),
        "jk_ovlp": ctx.to_device(np.broadcast_to(np.eye(t["nao"], dtype=np.complex128), (nk, t["nao"], t["nao"]))),
    }
    yield s
    for k in ("eri_tab", "eri_hot", "jk_dm", "jk_vj", "jk_vk", "jk_ovlp"):
        s[k].free()


def _tab_engine(ctx, s, **kw):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    t = TAB
    d_C = ctx.to_device(s["C_tab"])
    return et.EriEngine(ctx, t["mesh"], t["nao"], t["naux"], t["nemb"], t["spin"], d_C, s["eri_tab"], **kw), d_C


def _host_feed(ctx, s):
    """One normal and one swapped block through dmk_eri_push_block_host: both staging blocks and the transposed block."""
    from libdmet_preview_amd._lib import lib
    eng, d_C = _tab_engine(ctx, s)
    try:
        kL = eng.irreducible_kL()[0]
        w = int(eng.weights[kL])
        ctx.check(lib.dmk_eri_begin_kL_weighted(eng.h, kL, w))
        for slot, r in enumerate(eng.by_kL[kL][:2]):
            flags = int(r[4]) | (2 if slot == 1 else 0)
            ctx.check(lib.dmk_eri_push_block_host(eng.h, int(r[1]), int(r[2]), flags, s["host"][slot].ctypes.data, slot))
        for slot in (0, 1):
            ctx.check(lib.dmk_eri_host_slot_wait(eng.h, slot))
        ctx.check(lib.dmk_eri_end_kL(eng.h, w))
    finally:
        eng.close()
        d_C.free()


def _ring(ctx, s, **kw):
    """One kL through the block ring (GDFPhilox writes the blocks into the ring slots on the stream the pipeline hands out)."""
    eng, d_C = _tab_engine(ctx, s, **kw)
    try:
        assert eng.ring_slots > 0
        eng.run_kL(eng.irreducible_kL()[0], s["df_tab"])
    finally:
        eng.close()
        d_C.free()


def _stack_replaces_planes(ctx, s):
    """A first pipeline holds the workspaces parked in the context, so the second one begins with a plane buffer of exactly one
    slot and dmk_eri_stack has to replace it."""
    holder, d_C0 = _tab_engine(ctx, s)
    eng, d_C = _tab_engine(ctx, s)
    try:
        assert eng.set_stack(nslots=3) == 3
        eng.run_kL(eng.irreducible_kL()[0], s["df_tab"])
        eng.contract()
    finally:
        eng.close()
        holder.close()
        d_C.free()
        d_C0.free()


def _cached(ctx, s, make_engine, eri):
    """A cold and a warm pass over one kL with an EriInvariantCache attached (plane entry and the block of the result), then drop()
    and close()."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    cache = et.EriInvariantCache(ctx)
    try:
        for _ in ("cold", "warm"):
            eri.zero_()
            eng, d_C, df = make_engine(cache)
            try:
                assert eng.inv_attached and eng.inv_block_tiles > 0
                assert eng.set_stack(nslots=2) == 2
                eng.run_kL(eng.irreducible_kL()[0], df)
                eng.contract()
            finally:
                eng.close()
                d_C.free()
        st, bs = cache.stats(), cache.block_stats()
        assert (st["hits"], st["misses"], st["entries"]) == (1, 1, 1), st
        assert (bs["hits"], bs["misses"]) == (1, 1) and bs["bytes"] > 0, bs
        cache.drop()
        assert cache.stats()["entries"] == 0 and cache.block_stats()["bytes"] == 0
    finally:
        cache.close()


def _hot_rows_only(ctx, s, nao, monkeypatch):
    """nemb = 256, rows-only, two spins, a queue of 2 so that a kL is several groups: at nao 24 the second half of Ut and W."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    monkeypatch.setenv("DMK_ERI_GROUP", "2")
    d_C = ctx.to_device(s["C_hot"][nao])
    eng = et.EriEngine(ctx, HOT["mesh"], nao, HOT["naux"], HOT["nemb"], 2, d_C, None, rows_only=True, split_step1=True)
    try:
        assert eng.set_stack(nslots=2) == 2
        eng.run_kL(eng.irreducible_kL()[0], _philox(HOT["nk"], HOT["naux"], nao))
        if nao == 24:
            assert eng.ring_slots == 2 and eng.split_step1 and eng.fused_launches > 0
        else:
            assert eng.ring_slots == 0 and not eng.split_step1          # (naux nao = 384 rows: the generic kernels)
    finally:
        eng.close()
        d_C.free()
        monkeypatch.delenv("DMK_ERI_GROUP")


def _dfjk(ctx, s):
    """J and K at nk 2: the Coulomb passes and row 0 of K through dmk_dfjk_push_block_host on both slots, row 1 of K through the
    block ring, the Ewald term, finish, free."""
    from libdmet_preview_amd._lib import lib
    t, nk = TAB, 2
    h = C.c_void_p()
    ctx.check(lib.dmk_dfjk_begin(ctx.h, nk, t["nao"], t["naux"], 2, 3, s["jk_dm"].ptr, s["jk_vj"].ptr, s["jk_vk"].ptr, C.byref(h)))
    try:
        ring, nslots = C.c_void_p(), C.c_int()
        ctx.check(lib.dmk_dfjk_block_ring(h, C.byref(ring), C.byref(nslots)))
        assert ring.value and nslots.value >= 1
        ctx.check(lib.dmk_dfjk_set_ewald(h, 0.37, s["jk_ovlp"].ptr))
        blk = s["host"]
        for what in (1, 2):
            for k in range(nk):
                ctx.check(lib.dmk_dfjk_push_block_host(h, k, k, what, blk[k].ctypes.data, k))
        for kj in range(nk):
            ctx.check(lib.dmk_dfjk_push_block_host(h, 0, kj, 0, blk[kj].ctypes.data, kj))
        slot0 = ctx.wrap(ring.value, blk[0].shape, np.complex128)
        for kj in range(nk):
            slot0.set(blk[kj])
            ctx.check(lib.dmk_dfjk_push_block(h, 1, kj, 0, slot0.ptr))
        for slot in (0, 1):
            ctx.check(lib.dmk_dfjk_host_slot_wait(h, slot))
        ctx.check(lib.dmk_dfjk_finish(h))
    finally:
        assert lib.dmk_dfjk_free(h) == 0


def test_every_lazily_created_resource_is_given_back(ctx, shared, monkeypatch):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    s = shared

    def tab_cached(cache):
        eng, d_C = _tab_engine(ctx, s, inv_cache=cache, inv_cols=32)
        return eng, d_C, s["df_tab"]

    def hot_cached(cache):
        d_C = ctx.to_device(s["C_hot"][24][:1])
        eng = et.EriEngine(ctx, HOT["mesh"], 24, HOT["naux"], HOT["nemb"], 1, d_C, s["eri_hot"], inv_cache=cache, split_step1=True)
        return eng, d_C, _philox(HOT["nk"], HOT["naux"], 24)

    def one_round(_it):
        _host_feed(ctx, s)
        _ring(ctx, s)
        monkeypatch.setenv("DMK_ERI_GEN_STREAM", "1")
        try:
            _ring(ctx, s)
        finally:
            monkeypatch.delenv("DMK_ERI_GEN_STREAM")
        _ring(ctx, s, t_reversal_symm=False, track_imag=True)
        _stack_replaces_planes(ctx, s)
        _cached(ctx, s, tab_cached, s["eri_tab"])
        for nao in (16, 24):
            _hot_rows_only(ctx, s, nao, monkeypatch)
        _cached(ctx, s, hot_cached, s["eri_hot"])
        _dfjk(ctx, s)

    mark, free = _rounds(ctx, one_round, "pipelines of every kind")
    assert mark - free < BOUND, (mark, free)


def test_handles_that_never_pushed_finish_cleanly(ctx, shared):
    """dmk_eri_finish and dmk_dfjk_free on handles without a single block, and on a dmk_dfjk whose host feed saw one slot only: the
    events and staging blocks that were never created are not there to destroy.  Both return DMK_OK and the memory mark holds."""
    from libdmet_preview_amd._lib import lib, mesh3
    s, t = shared, TAB

    def one_round(_it):
        d_C = ctx.to_device(s["C_tab"])
        h = C.c_void_p()
        ctx.check(lib.dmk_eri_begin(ctx.h, mesh3(t["mesh"]), t["nao"], t["naux"], t["nemb"], t["spin"], 1, d_C.ptr, s["eri_tab"].ptr,
                                    C.byref(h)))
        assert lib.dmk_eri_finish(h) == 0
        d_C.free()
        for host_slot in (None, 1):
            h = C.c_void_p()
            ctx.check(lib.dmk_dfjk_begin(ctx.h, 2, t["nao"], t["naux"], 2, 3, s["jk_dm"].ptr, s["jk_vj"].ptr, s["jk_vk"].ptr, C.byref(h)))
            if host_slot is not None:
                ctx.check(lib.dmk_dfjk_push_block_host(h, 0, 0, 1, s["host"][0].ctypes.data, host_slot))
                assert lib.dmk_dfjk_host_slot_wait(h, 0) == 0 and lib.dmk_dfjk_host_slot_wait(h, 1) == 0
            assert lib.dmk_dfjk_free(h) == 0

    mark, free = _rounds(ctx, one_round, "handles that never pushed")
    assert mark - free < BOUND, (mark, free)
