"""
Iteration-invariant step-2 planes on the TABLE-DRIVEN kernel (dmk_eri_attach_cache_cols / EriEngine(inv_cols=), run with -m gpu on
an MI355X): with `ninv` invariant leading columns of C_ao_emb and A = 16 floor(ninv / 16), a transform whose columns [0, A) are
bit-identical to those of an earlier one copies the prefix [0, A (A + 1) / 2) of every plane row from the cache and launches the
block table without the block rows below A / 16.

Reference of every comparison: the same engine WITHOUT a cache (the dense path of the same build) on the same inputs.
Tolerance: the dense path is run twice first; when its two ERIs are bit-identical (expected: one writer per plane element per
launch, stream-ordered launches) the cached ERI and planes must be bit-identical to them, otherwise they may differ by at most
4 x the dense-vs-dense max-abs difference.  Shapes: mesh 3 x 2 x 1 (weight-1 and weight-2 kL), naux 24, nao 24 (30: off the K tile),
GDFPhilox input -- the smallest the hot kernels accept:
    a  nemb 136 / ninv 104  A 96   two spins   wide items, occupancy 3 (the block grid of BASELINE config 4)
    b  nemb  90 / ninv  50  A 48   two spins   odd pair count 4095: padded plane pitch, one warm workgroup
    c  nemb  48 / ninv  20  A 16   two spins   the smallest region: one dropped block
    d  nemb 200 / ninv 150  A 144  one spin    segment layout, occupancy 2: the cut at block row 9 goes through the second
                                               segment's triangle and a 4-row rectangle
"""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import eri_sample as ES                  # the checker

MESH, NK, NAUX = (3, 2, 1), 6, 24
CASES = {"a": (136, 104, 2, 24), "a30": (136, 104, 2, 30), "b": (90, 50, 2, 24), "c": (48, 20, 2, 24), "d": (200, 150, 1, 24)}


def _npair(nemb):
    return nemb * (nemb + 1) // 2


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


@pytest.fixture(scope="module")
def pool(ctx):
    """Three ERI buffers per (nemb, spin), allocated at that size on first use, shared by the tests of the module."""
    held = {}

    def get(nemb, spin):
        if (nemb, spin) not in held:
            held[(nemb, spin)] = [ctx.zeros((spin * (spin + 1) // 2, _npair(nemb), _npair(nemb)), np.float64) for _ in range(3)]
        return held[(nemb, spin)]
    yield get
    for b in held.values():
        for x in b:
            x.free()


def _C(nao, seed, nemb, spin):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((spin, NK, nao, nemb)) + 1j * rng.standard_normal((spin, NK, nao, nemb))) / np.sqrt(nao)


def _df(nao, seed=5):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((NK, 3)), NAUX, nao, seed=seed)


def _maxabs(ctx, a, b):
    """max |a - b| of two device arrays; 0.0 exactly when they hold the same values."""
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


def _run(ctx, Ce, df, eri_dev, cache=None, inv_cols=None, planes=False, probe=None, stack=False, **kw):
    """One whole transform.  Returns a dict: the engine's attach flag and compared columns, the planes of every kL (on request) and
    the zgemm_half2 launch count / executed flop of the call."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    spin, _, nao, nemb = Ce.shape
    eri_dev.zero_()
    C_dev = ctx.to_device(Ce)
    eng = et.EriEngine(ctx, MESH, nao, NAUX, nemb, spin, C_dev, eri_dev, inv_cache=cache, inv_cols=inv_cols, **kw)
    out = {"attached": eng.inv_attached, "cols_used": eng.inv_cols_used, "planes": {}, "weights": eng.weights, "by_kL": eng.by_kL,
           "ring_slots": eng.ring_slots}
    try:
        if stack:
            eng.set_stack(n_kL=len(eng.irreducible_kL()))
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        ctx.profile_read(reset=True)
        ctx.profile_read_flops(reset=True)
        for kL in eng.irreducible_kL():
            eng.run_kL(kL, df)
            if planes:
                out["planes"][kL] = eng.planes().get()
        eng.contract()
        ctx.sync()
        out["half2_launches"] = ctx.profile_read(reset=True)["zgemm_half2"][1]
        out["half2_flops"] = ctx.profile_read_flops(reset=True)["zgemm_half2"]
    finally:
        eng.close()
    return out


@pytest.fixture(scope="module")
def noise(ctx, pool):
    """max-abs difference of two dense transforms of the same inputs, per shape: the yardstick of every comparison below."""
    known = {}

    def get(nemb, spin, nao):
        if (nemb, spin, nao) not in known:
            bufs = pool(nemb, spin)
            Ce, df = _C(nao, 1, nemb, spin), _df(nao)
            _run(ctx, Ce, df, bufs[0])
            _run(ctx, Ce, df, bufs[1])
            known[(nemb, spin, nao)] = _maxabs(ctx, bufs[0], bufs[1])
            print("dense vs dense, nemb %d spin %d nao %d: %.3e" % (nemb, spin, nao, known[(nemb, spin, nao)]))
        return known[(nemb, spin, nao)]
    return get


def _assert_same(ctx, got, ref, noise, what):
    d = _maxabs(ctx, got, ref)
    print("%s: max |cached - dense| = %.3e (dense vs dense %.3e)" % (what, d, noise))
    if noise == 0.0:
        assert d == 0.0, "%s: differs from dense by %.3e although dense vs dense is bit-identical" % (what, d)
    else:
        assert d <= 4.0 * noise, "%s: differs from dense by %.3e, dense vs dense by %.3e" % (what, d, noise)


def _table_stats(nemb, lo):
    """(useful, folded) blocks of the table the kernel launches by default: occupancy 3 for wide items (nb <= 12), else 2."""
    from libdmet_preview_amd._lib import lib
    n, st = C.c_int(), (C.c_double * 3)()
    assert lib.dmk_half2_tab_table(nemb, 3 if (nemb + 15) // 16 <= 12 else 2, lo, None, 0, C.byref(n), st) == 0
    return st[0], st[2]


def _half2_flops(run, nao, nemb, spin, lo, folded):
    """Executed flop of step 2 as launch_half2_tab counts it, for a table without the block rows below `lo` in every kL: per
    queued block `useful` block products, plus, for a symmetrised one, the partner segment of all of them but -- when the whole
    launch is symmetrised -- the `folded` diagonal blocks."""
    kdim = (nao + 7) // 8 * 8
    nb = (nemb + 15) // 16
    useful = nb * (nb + 1) // 2 - lo * (lo + 1) // 2
    total = 0.0
    for kL, recs in run["by_kL"].items():
        if run["weights"][kL] <= 0:
            continue
        for g0 in range(0, len(recs), run["ring_slots"]):
            sym = [int(r[4]) for r in recs[g0:g0 + run["ring_slots"]]]
            seg2 = sum(sym) * (useful - (folded if all(sym) else 0.0))
            total += (4.0 if run["weights"][kL] == 1 else 6.0) * (len(sym) * useful + seg2) * 256.0 * kdim * NAUX * spin
    return total


def test_plan_has_both_weights():
    from libdmet_preview_amd.basis_transform import eri_transform as et
    w, _ = et.eri_plan(MESH, True)
    assert 1 in set(int(x) for x in w) and 2 in set(int(x) for x in w)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cold_then_warm(ctx, pool, noise, case):
    """Second call: a hit for every kL, ERI and planes equal dense, step 2 issues the flop count of the table without the
    region's block rows; case a also against the sampled oracle at 1e-8."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, ninv, spin, nao = CASES[case]
    A, nb, npair, nblk = 16 * (ninv // 16), (nemb + 15) // 16, _npair(nemb), spin * (spin + 1) // 2
    lo = A // 16
    bufs, dn = pool(nemb, spin), noise(nemb, spin, nao)
    Ce, df = _C(nao, 10 + nao + nemb, nemb, spin), _df(nao)
    ref = _run(ctx, Ce, df, bufs[0], planes=True)
    assert ref["ring_slots"] == 16 and ref["half2_launches"] > 0           # the grouped table path
    assert ref["half2_flops"] == _half2_flops(ref, nao, nemb, spin, 0, _table_stats(nemb, 0)[1])
    n_kL = len(ref["planes"])
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, planes=True)
        assert cold["attached"] and cold["cols_used"] == A
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "cold")
        assert cold["half2_flops"] == ref["half2_flops"]
        warm = _run(ctx, Ce, df, bufs[2], cache=cache, inv_cols=ninv, planes=True)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"], st["drops"]) == (n_kL, n_kL, n_kL, 0), st
        assert st["bytes"] == sum(spin * (1 if ref["weights"][k] == 1 else 2) * NAUX * (A * (A + 1) // 2) * 8 for k in ref["planes"])
        _assert_same(ctx, bufs[2], bufs[0], dn, "warm")
        for kL in ref["planes"]:
            d = float(np.abs(warm["planes"][kL] - ref["planes"][kL]).max())
            assert d <= 4.0 * dn, (kL, d)
            assert dn != 0.0 or np.array_equal(warm["planes"][kL], ref["planes"][kL])
        assert warm["half2_launches"] == ref["half2_launches"]
        useful, folded = _table_stats(nemb, lo)
        assert useful == nb * (nb + 1) // 2 - lo * (lo + 1) // 2 and 0 <= folded <= nb - lo
        print("half2 flop dense %.6e warm %.6e ratio %.4f" % (ref["half2_flops"], warm["half2_flops"], warm["half2_flops"] / ref["half2_flops"]))
        assert warm["half2_flops"] < ref["half2_flops"]
        assert (_half2_flops(warm, nao, nemb, spin, lo, nb - lo) <= warm["half2_flops"] <= _half2_flops(warm, nao, nemb, spin, lo, 0))
        assert warm["half2_flops"] == _half2_flops(warm, nao, nemb, spin, lo, folded)
        if case == "a":
            # 48 of 84 segment slots stay occupied, 45 of 81 useful block products (all-symmetrised launches; fewer otherwise)
            assert warm["half2_flops"] <= 0.60 * ref["half2_flops"]
            orbs = [0, 95, 96, 103, 104, 135]
            want, idx, _ = ES.eri_sample(MESH, 5, Ce, NAUX, orbs, sorted(ref["planes"]))
            for blk in range(nblk):
                got = np.stack([bufs[2].offset((blk * npair + int(r)) * npair, (npair,)).get()[idx] for r in idx])
                assert np.abs(got - want[blk]).max() < 1e-8
    finally:
        cache.close()


def _flip_lowest_bit(Ce, idx):
    """One bit of the real part of one element."""
    out = Ce.copy()
    bits = np.array([out[idx].real]).view(np.uint64)
    bits ^= np.uint64(1)
    out[idx] = complex(bits.view(np.float64)[0], out[idx].imag)
    assert out[idx] != Ce[idx]
    return out


def test_bath_only_change_hits_and_an_impurity_bit_drops(ctx, pool, noise):
    """The boundary at case a (ninv 104, A 96): columns >= ninv may change freely, and so may column A, which lies beyond the
    compared prefix although it is below ninv (hits); one bit of column A - 1 drops everything."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, ninv, spin, nao = CASES["a"]
    A = 16 * (ninv // 16)
    bufs, dn = pool(nemb, spin), noise(nemb, spin, nao)
    Ce, df = _C(nao, 2, nemb, spin), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        n_kL = cache.stats()["entries"]
        assert n_kL > 0
        C2 = Ce.copy()
        C2[..., ninv:] = _C(nao, 3, nemb, spin)[..., ninv:]
        _run(ctx, C2, df, bufs[0])
        _run(ctx, C2, df, bufs[1], cache=cache, inv_cols=ninv)
        st = cache.stats()
        assert (st["hits"], st["drops"]) == (n_kL, 0), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "bath columns changed")
        C3 = C2.copy()
        C3[..., A] = _C(nao, 4, nemb, spin)[..., A]
        _run(ctx, C3, df, bufs[0])
        _run(ctx, C3, df, bufs[1], cache=cache, inv_cols=ninv)
        st = cache.stats()
        assert (st["hits"], st["drops"]) == (2 * n_kL, 0), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "column A changed")
        C4 = _flip_lowest_bit(C3, (spin - 1, 4, nao - 1, A - 1))
        _run(ctx, C4, df, bufs[0])
        _run(ctx, C4, df, bufs[1], cache=cache, inv_cols=ninv)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["drops"], st["entries"]) == (2 * n_kL, 2 * n_kL, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "one bit of column A - 1 changed")
        _run(ctx, C4, df, bufs[1], cache=cache, inv_cols=ninv)
        assert cache.stats()["hits"] == 3 * n_kL
        _assert_same(ctx, bufs[1], bufs[0], dn, "one bit of column A - 1 changed, warm")
    finally:
        cache.close()


def test_hint_changes(ctx, pool, noise):
    """Another ninv with the same A keeps the entries; one that maps to another A drops them and stays correct."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, ninv, spin, nao = CASES["b"]                 # ninv 50: A 48
    bufs, dn = pool(nemb, spin), noise(nemb, spin, nao)
    Ce, df = _C(nao, 6, nemb, spin), _df(nao)
    _run(ctx, Ce, df, bufs[0])
    cache = et.EriInvariantCache(ctx)
    try:
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv)
        n_kL = cache.stats()["entries"]
        assert r["cols_used"] == 48 and n_kL > 0
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=63)
        st = cache.stats()
        assert r["cols_used"] == 48 and (st["hits"], st["drops"], st["entries"]) == (n_kL, 0, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "ninv 63, same A")
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=40)
        st = cache.stats()
        assert r["cols_used"] == 32 and (st["hits"], st["drops"], st["entries"]) == (n_kL, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "ninv 40, A 32, cold")
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=47)
        st = cache.stats()
        assert r["cols_used"] == 32 and (st["hits"], st["drops"]) == (2 * n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "ninv 47, A 32, warm")
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=1000)        # more than nemb: A = 16 floor(90 / 16) = 80
        st = cache.stats()
        assert r["cols_used"] == 80 and (st["hits"], st["drops"]) == (2 * n_kL, 2 * n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dn, "ninv beyond nemb, cold")
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=1000)
        assert cache.stats()["hits"] == 3 * n_kL
        _assert_same(ctx, bufs[1], bufs[0], dn, "ninv beyond nemb, warm")
    finally:
        cache.close()


@pytest.mark.parametrize("how", ["ninv15", "no_time_reversal", "gso", "tab_sub2"])
def test_refusals(ctx, pool, how, monkeypatch):
    """Hints and modes without the region attach nothing and compute what they compute without a cache (case c otherwise attaches)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, ninv, spin, nao = CASES["c"]
    if how == "ninv15":
        ninv = 15
    if how == "tab_sub2":
        monkeypatch.setenv("DMK_ERI_TAB_SUB", "2")
    kw = {"t_reversal_symm": False} if how == "no_time_reversal" else {"gso": True} if how == "gso" else {}
    bufs = pool(nemb, spin)
    Ce, df = _C(nao, 8, nemb, spin), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[0], **kw)
        for _ in range(2):
            r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, **kw)
            assert not r["attached"] and r["cols_used"] == 0
            st = cache.stats()
            assert (st["hits"], st["misses"], st["entries"], st["bytes"]) == (0, 0, 0, 0), st
            assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    finally:
        cache.close()


def test_nemb_256_through_the_new_entry_point(ctx, monkeypatch):
    """On the nemb = 256 kernel the region is fixed: ninv >= 192 attaches with 192 columns and behaves as dmk_eri_attach_cache,
    anything less does not attach.  Routed through the table kernel (DMK_ERI_TAB256=1) the table rule applies."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, spin, nao = 256, 1, 24
    bufs = [ctx.zeros((1, _npair(nemb), _npair(nemb)), np.float64) for _ in range(2)]
    Ce, df = _C(nao, 9, nemb, spin), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        ref = _run(ctx, Ce, df, bufs[0])
        assert ref["ring_slots"] == 8
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=100)
        assert not r["attached"] and r["cols_used"] == 0 and cache.stats()["misses"] == 0
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=200)
        n_kL = cache.stats()["entries"]
        assert r["attached"] and r["cols_used"] == 192 and n_kL > 0
        assert cache.stats()["bytes"] == sum(spin * (1 if ref["weights"][k] == 1 else 2) * NAUX * 16448 * 8
                                             for k in ref["by_kL"] if ref["weights"][k] > 0)
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=200)
        st = cache.stats()
        assert (st["hits"], st["drops"]) == (n_kL, 0), st
        assert r["half2_flops"] < 0.51 * ref["half2_flops"]
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        r = _run(ctx, Ce, df, bufs[1], cache=cache)                     # the old entry point shares the entries
        assert r["attached"] and cache.stats()["hits"] == 2 * n_kL and _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        monkeypatch.setenv("DMK_ERI_TAB256", "1")
        ref = _run(ctx, Ce, df, bufs[0])
        assert ref["ring_slots"] == 16
        r = _run(ctx, Ce, df, bufs[1], cache=cache)
        assert not r["attached"]                                          # dmk_eri_attach_cache: the nemb = 256 kernel only
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=100)
        st = cache.stats()
        assert r["attached"] and r["cols_used"] == 96 and (st["drops"], st["entries"]) == (n_kL, n_kL), st
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
        r = _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=100)
        assert cache.stats()["hits"] == 3 * n_kL and r["half2_flops"] < ref["half2_flops"]
        assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    finally:
        cache.close()
        for b in bufs:
            b.free()


def test_freivalds_on_a_warm_call(ctx, pool):
    """eri x against the yref the pipeline accumulates from its (partly cached) planes, at the bound of bench.py."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nemb, ninv, spin, nao = CASES["a"]
    npair, nblk = _npair(nemb), spin * (spin + 1) // 2
    bufs = pool(nemb, spin)
    Ce, df = _C(nao, 9, nemb, spin), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, stack=True)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, npair))
        d_y = ctx.zeros((nblk, npair), np.float64)
        _run(ctx, Ce, df, bufs[1], cache=cache, inv_cols=ninv, stack=True, probe=(d_x, d_y))
        assert cache.stats()["hits"] == cache.stats()["entries"] > 0
        y = et.eri_times_vector_dev(ctx, bufs[1], nblk, npair, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        assert np.abs(y - yref).max() <= 1e-10 * max(1.0, np.abs(yref).max()), np.abs(y - yref).max()
    finally:
        cache.close()


def test_pipeline_iterations_hit(ctx, pool, monkeypatch):
    """pipeline.iteration on a system with 104 impurity + 32 bath orbitals (nemb 136): the second iteration hits and reproduces the
    first; after a change of the correlation potential (another bath, the same impurity columns) it still hits and equals the
    dense result of a fresh system."""
    from libdmet_preview_amd import pipeline
    monkeypatch.delenv("DMK_ERI_INV", raising=False)
    mesh, nlo, naux, nval, spin = (2, 2, 1), 104, 8, 32, 2
    bufs = pool(136, spin)

    def ham_equal(a, b):
        for k in ("H1", "JK_core"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k

    sysm = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, spin, seed=11, name="inv-tab")
    bufs[0].zero_()
    o1 = pipeline.iteration(ctx, sysm, eri_dev=bufs[0])
    assert o1["nemb"] == 136
    h1 = o1["emb_ham"]
    st = sysm.eri_inv_cache.stats()
    n_kL = st["entries"]
    assert n_kL > 0 and st["hits"] == 0
    bufs[1].zero_()
    o2 = pipeline.iteration(ctx, sysm, eri_dev=bufs[1])
    st = sysm.eri_inv_cache.stats()
    assert (st["hits"], st["drops"]) == (n_kL, 0), st
    assert _maxabs(ctx, bufs[1], bufs[0]) == 0.0
    ham_equal(o2["emb_ham"], h1)

    rng = np.random.default_rng(12)
    v = 0.05 * rng.standard_normal((2, nlo, nlo))
    v = v + v.transpose(0, 2, 1)

    def set_vcor(s):
        s.vcor = v
        s.d_vcor = ctx.to_device(v[:spin])

    set_vcor(sysm)
    bufs[1].zero_()
    o3 = pipeline.iteration(ctx, sysm, eri_dev=bufs[1])
    st = sysm.eri_inv_cache.stats()
    assert (st["hits"], st["drops"]) == (2 * n_kL, 0), st
    assert _maxabs(ctx, bufs[1], bufs[0]) > 0.0                      # the bath did change
    monkeypatch.setenv("DMK_ERI_INV", "0")
    fresh = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, spin, seed=11, name="inv-tab-dense")
    set_vcor(fresh)
    bufs[2].zero_()
    o4 = pipeline.iteration(ctx, fresh, eri_dev=bufs[2])
    assert fresh.eri_inv_cache is None
    assert _maxabs(ctx, bufs[1], bufs[2]) == 0.0
    ham_equal(o3["emb_ham"], o4["emb_ham"])
    sysm.eri_inv_cache.close()


def test_get_emb_eri_fast_gdf_with_resident_df(ctx, monkeypatch):
    """The patched entry point: with RESIDENT_DF and INVARIANT_PLANES an [I_imp | bath] basis at nemb 136 gives the hint itself; the
    second call hits and equals the first, which agrees with a call with both switches off."""
    from libdmet_preview_amd import synth
    from libdmet_preview_amd.basis_transform import eri_transform as et
    from libdmet_preview_amd.system import fourier
    from libdmet_preview_amd.system.lattice import _UnitCell
    mesh, nao, naux, nimp, nbath = (2, 2, 1), 104, 8, 104, 32
    nk = 4
    cell = _UnitCell(nao)
    mydf = et.GDFPhilox(cell.get_abs_kpts(fourier.make_kpts_scaled(mesh)), naux, nao, seed=21)
    Clo = synth.make_C_ao_lo(mesh, nao, nao, spin=1, seed=3)
    rng = np.random.default_rng(5)
    basis = np.zeros((1, nk, nao, nimp + nbath))
    basis[0, 0, np.arange(nimp), np.arange(nimp)] = 1.0
    basis[0, 1:, :, nimp:] = rng.standard_normal((nk - 1, nao, nbath)) / np.sqrt(nao * (nk - 1))
    assert et.leading_identity_columns(basis) == nimp
    monkeypatch.delenv("DMK_ERI_INV", raising=False)
    e0 = et.get_emb_eri_fast_gdf(cell, mydf, C_ao_lo=Clo, basis=basis)
    monkeypatch.setattr(et, "RESIDENT_DF", True)
    monkeypatch.setattr(et, "INVARIANT_PLANES", True)
    try:
        e1 = et.get_emb_eri_fast_gdf(cell, mydf, C_ao_lo=Clo, basis=basis)
        (_, res), = et._resident_cache.values()
        st = res.inv_cache.stats()
        n_kL = st["entries"]
        assert n_kL > 0 and (st["hits"], st["bytes"]) == (0, sum(w * naux * (96 * 97 // 2) * 8 for w in et.eri_plan(mesh, True)[0]))
        e2 = et.get_emb_eri_fast_gdf(cell, mydf, C_ao_lo=Clo, basis=basis)
        st = res.inv_cache.stats()
        assert (st["hits"], st["drops"], st["entries"]) == (n_kL, 0, n_kL), st
        assert np.array_equal(e1, e2)
        assert np.abs(e1 - e0).max() <= 1e-10 * max(1.0, np.abs(e0).max())          # (blocks read in place: another feed, the same sums)
        # the C_ao_eo= entry carries no hint: it neither hits nor stores
        Ce = et.make_C_ao_emb_dev(ctx, list(mesh), C_ao_lo=Clo, basis=basis, nao=nao).get() * nk ** 0.75
        e3 = et.get_emb_eri_fast_gdf(cell, mydf, C_ao_eo=Ce[0])
        assert res.inv_cache.stats() == st
        assert np.abs(e3 - e1).max() <= 1e-10 * max(1.0, np.abs(e1).max())
    finally:
        et.drop_resident()
