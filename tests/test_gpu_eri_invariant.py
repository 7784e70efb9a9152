"""
Iteration-invariant step-2 planes (dmk_eri_cache / EriInvariantCache, run with -m gpu on an MI355X): a transform whose leading 192
columns of C_ao_emb are bit-identical to those of an earlier one copies the impurity-only part of the planes (workgroup types 0
and 2 of the nemb = 256 step-2 kernel) from the cache and launches types 1 and 3 only.

Reference of every comparison: the same engine WITHOUT a cache (the dense path of the same build) on the same inputs.
Tolerance: the dense path is run twice first; when its two ERIs are bit-identical (expected: one writer per plane element per
launch, stream-ordered launches) the cached ERI must be bit-identical to them, otherwise it may differ by at most 4 x the
dense-vs-dense max-abs difference.  Shapes: mesh 3 x 2 x 1 (weight-1 and weight-2 kL), naux 24, nao 24 / 40 (on the K tile) and
30 (off it: kdim / padded C), nemb 256, two spins -- the smallest the hot kernels accept.
"""
import os
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
    """Three ERI buffers shared by every test of the module (zeroed before each transform)."""
    b = [ctx.zeros((NBLK, NPAIR, NPAIR), np.float64) for _ in range(3)]
    yield b
    for x in b:
        x.free()


def _C(nao, seed, nemb=NEMB):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((SPIN, NK, nao, nemb)) + 1j * rng.standard_normal((SPIN, NK, nao, nemb))) / np.sqrt(nao)


def _df(nao, seed=5):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    return et.GDFPhilox(np.zeros((NK, 3)), NAUX, nao, seed=seed)


def _maxabs(ctx, a, b):
    """max |a - b| of two device arrays; 0.0 exactly when they hold the same values (one reduction on the device, the rows are
    only brought to the host when they differ)."""
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


def _run(ctx, Ce, df, eri_dev, cache=None, nemb=NEMB, max_blocks=None, planes=False, probe=None, stack=False, **kw):
    """One whole transform.  Returns a dict: the engine's attach flag, the planes of every kL (on request) and the zgemm_half2
    launch count / executed flop of the call."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = Ce.shape[2]
    eri_dev.zero_()
    C_dev = ctx.to_device(Ce)
    eng = et.EriEngine(ctx, MESH, nao, NAUX, nemb, SPIN, C_dev, eri_dev, inv_cache=cache, **kw)
    out = {"attached": eng.inv_attached, "planes": {}, "weights": eng.weights, "by_kL": eng.by_kL, "ring_slots": eng.ring_slots}
    try:
        if stack:
            eng.set_stack(n_kL=len(eng.irreducible_kL()))
        if probe is not None:
            eng.set_probe(probe[0], probe[1])
        ctx.profile_read(reset=True)
        ctx.profile_read_flops(reset=True)
        for kL in eng.irreducible_kL():
            eng.run_kL(kL, df, max_blocks=max_blocks)
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
def dense_noise(ctx, bufs):
    """max-abs difference of two dense transforms of the same inputs (nao 24): the yardstick of every comparison below."""
    Ce, df = _C(24, 1), _df(24)
    _run(ctx, Ce, df, bufs[0])
    _run(ctx, Ce, df, bufs[1])
    return _maxabs(ctx, bufs[0], bufs[1])


def _assert_same(ctx, got, ref, noise, what):
    d = _maxabs(ctx, got, ref)
    if noise == 0.0:
        assert d == 0.0, "%s: differs from dense by %.3e although dense vs dense is bit-identical" % (what, d)
    else:
        assert d <= 4.0 * noise, "%s: differs from dense by %.3e, dense vs dense by %.3e" % (what, d, noise)


def _half2_flops(run, nao, warm_kL):
    """Executed flop of step 2 as launch_half2_hot counts it: per queued block 136 (+ 120 / 136 partner) 16 x 16 block products
    dense, 68 (+ 60 / 68) with the invariant region skipped; one launch per kL here (6 blocks, queue of 8)."""
    kdim = (nao + 7) // 8 * 8
    total = 0.0
    for kL, recs in run["by_kL"].items():
        if run["weights"][kL] <= 0:
            continue
        assert len(recs) <= run["ring_slots"]
        sym = [int(r[4]) for r in recs]
        fold = all(sym)
        full, part = ((68.0, 60.0 if fold else 68.0) if kL in warm_kL else (136.0, 120.0 if fold else 136.0))
        blocks = sum(full + (part if s else 0.0) for s in sym)
        re_only = run["weights"][kL] == 1
        total += (4.0 if re_only else 6.0) * blocks * 256.0 * kdim * NAUX * SPIN
    return total


def test_plan_has_both_weights():
    from libdmet_preview_amd.basis_transform import eri_transform as et
    w, _ = et.eri_plan(MESH, True)
    assert 1 in set(int(x) for x in w) and 2 in set(int(x) for x in w)


@pytest.mark.parametrize("nao", [24, 40, 30])
def test_cold_then_warm(ctx, bufs, dense_noise, nao):
    """Second call: a hit for every kL, ERI and planes equal dense, step 2 issues the two-type flop count; against the sampled
    oracle at 1e-8 (nao 24)."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    Ce, df = _C(nao, 10 + nao), _df(nao)
    ref = _run(ctx, Ce, df, bufs[0], planes=True)
    assert ref["ring_slots"] == 8 and ref["half2_launches"] > 0          # the grouped nemb = 256 path
    n_kL = len(ref["planes"])
    cache = et.EriInvariantCache(ctx)
    try:
        cold = _run(ctx, Ce, df, bufs[1], cache=cache, planes=True)
        assert cold["attached"]
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dense_noise, "cold")
        assert cold["half2_flops"] == _half2_flops(cold, nao, set()) == ref["half2_flops"]
        warm = _run(ctx, Ce, df, bufs[2], cache=cache, planes=True)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"], st["drops"]) == (n_kL, n_kL, n_kL, 0), st
        assert st["bytes"] == sum(SPIN * (1 if ref["weights"][k] == 1 else 2) * NAUX * 16448 * 8 for k in ref["planes"])
        _assert_same(ctx, bufs[2], bufs[0], dense_noise, "warm")
        for kL in ref["planes"]:
            d = float(np.abs(warm["planes"][kL] - ref["planes"][kL]).max())
            assert d <= 4.0 * dense_noise, (kL, d)
            assert dense_noise != 0.0 or np.array_equal(warm["planes"][kL], ref["planes"][kL])
        assert warm["half2_launches"] == ref["half2_launches"]
        assert warm["half2_flops"] == _half2_flops(warm, nao, set(ref["planes"]))
        assert warm["half2_flops"] < 0.51 * ref["half2_flops"]
        if nao == 24:
            A = [0, 1, 127, 128, 191, 192, 255]
            want, idx, _ = ES.eri_sample(MESH, 5, Ce, NAUX, A, sorted(ref["planes"]))
            for blk in range(NBLK):
                got = np.stack([bufs[2].offset((blk * NPAIR + int(r)) * NPAIR, (NPAIR,)).get()[idx] for r in idx])
                assert np.abs(got - want[blk]).max() < 1e-8
    finally:
        cache.close()


def test_bath_only_change_hits_and_column_191_drops(ctx, bufs, dense_noise):
    """The boundary: columns >= 192 may change freely (hits), one element of column 191 drops everything."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 2), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache)
        n_kL = cache.stats()["entries"]
        assert n_kL > 0
        C2 = Ce.copy()
        C2[..., 192:] = _C(nao, 3)[..., 192:]
        _run(ctx, C2, df, bufs[0])
        _run(ctx, C2, df, bufs[1], cache=cache)
        st = cache.stats()
        assert (st["hits"], st["drops"]) == (n_kL, 0), st
        _assert_same(ctx, bufs[1], bufs[0], dense_noise, "bath columns changed")
        C3 = C2.copy()
        C3[1, 4, nao - 1, 191] += 1e-9
        _run(ctx, C3, df, bufs[0])
        _run(ctx, C3, df, bufs[1], cache=cache)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["drops"], st["entries"]) == (n_kL, 2 * n_kL, n_kL, n_kL), st
        _assert_same(ctx, bufs[1], bufs[0], dense_noise, "column 191 changed")
        _run(ctx, C3, df, bufs[1], cache=cache)
        assert cache.stats()["hits"] == 2 * n_kL
        _assert_same(ctx, bufs[1], bufs[0], dense_noise, "column 191 changed, warm")
    finally:
        cache.close()


def test_key_changes_miss(ctx, bufs, dense_noise, monkeypatch):
    """Another Philox seed, a cut visiting list (and back) and the Re-only switch never serve a stale plane."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 4), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        first = _run(ctx, Ce, df, bufs[1], cache=cache)
        n_kL = cache.stats()["entries"]
        n_w1 = sum(1 for k in first["by_kL"] if first["weights"][k] == 1)
        assert 0 < n_w1 < n_kL

        def step(what, expect_miss, df=df, **kw):
            before = cache.stats()
            _run(ctx, Ce, df, bufs[0], **kw)
            _run(ctx, Ce, df, bufs[1], cache=cache, **kw)
            after = cache.stats()
            assert after["misses"] - before["misses"] == expect_miss, (what, before, after)
            assert after["hits"] - before["hits"] == n_kL - expect_miss, (what, before, after)
            assert after["drops"] == 0
            _assert_same(ctx, bufs[1], bufs[0], dense_noise, what)

        step("another seed", n_kL, df=_df(nao, seed=6))
        step("max_blocks=2", n_kL, max_blocks=2)
        step("full after max_blocks=2", 0)
        step("max_blocks=2 again", 0, max_blocks=2)
        monkeypatch.setenv("DMK_ERI_RE_ONLY", "0")
        step("Re-only off", n_w1)               # weight-2 kL never were Re-only: their entries still apply
        monkeypatch.delenv("DMK_ERI_RE_ONLY")
        step("Re-only on again", 0)
    finally:
        cache.close()


def test_budget(ctx, bufs, dense_noise):
    """A budget below the shard: the kL that fit hit, the others stay dense on every call; budget 0: nothing is kept."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    Ce, df = _C(nao, 7), _df(nao)
    _run(ctx, Ce, df, bufs[0])
    _run(ctx, Ce, df, bufs[2], stack=True)           # the deferred, K-stacked contraction sums the kL in another order: its own reference
    w2 = SPIN * 2 * NAUX * 16448 * 8
    for budget, lo in ((1.6 * w2, 1), (0.0, 0)):
        cache = et.EriInvariantCache(ctx, budget_gb=budget / (1 << 30))
        try:
            run = _run(ctx, Ce, df, bufs[1], cache=cache)
            n_kL = sum(1 for k in run["by_kL"] if run["weights"][k] > 0)
            st = cache.stats()
            assert lo <= st["entries"] < n_kL and st["bytes"] <= budget, st
            assert lo == 0 or st["entries"] > 0
            _assert_same(ctx, bufs[1], bufs[0], dense_noise, "budget %g, cold" % budget)
            kept = st["entries"]
            _run(ctx, Ce, df, bufs[1], cache=cache, stack=True)
            st = cache.stats()
            assert st["hits"] == kept and st["entries"] == kept and st["misses"] == 2 * n_kL - kept, st
            _assert_same(ctx, bufs[1], bufs[2], dense_noise, "budget %g, warm, plane stack" % budget)
        finally:
            cache.close()


class _NoToken(object):
    """A provider that cannot promise an immutable tensor."""
    def __init__(self, df):
        self._df, self.kpts, self.naux = df, df.kpts, df.naux

    def load_block(self, ctx, i, j, out):
        return self._df.load_block(ctx, i, j, out)


@pytest.mark.parametrize("case", ["nemb250", "no_time_reversal", "gso", "no_token"])
def test_refusals(ctx, bufs, case):
    """Shapes and modes without the invariant region attach nothing and compute what they compute without a cache."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 24
    nemb = 250 if case == "nemb250" else NEMB
    kw = {"t_reversal_symm": False} if case == "no_time_reversal" else {"gso": True} if case == "gso" else {}
    Ce = _C(nao, 8, nemb)
    df = _NoToken(_df(nao)) if case == "no_token" else _df(nao)
    npair = nemb * (nemb + 1) // 2
    e0, e1 = [ctx.wrap(b.address, (NBLK, npair, npair), np.float64, keepalive=b) for b in bufs[:2]]
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, e0, nemb=nemb, **kw)
        for _ in range(2):
            r = _run(ctx, Ce, df, e1, cache=cache, nemb=nemb, **kw)
            assert r["attached"] == (case == "no_token")
            st = cache.stats()
            assert (st["hits"], st["misses"], st["entries"], st["bytes"]) == (0, 0, 0, 0), st
            assert _maxabs(ctx, e1, e0) == 0.0
    finally:
        cache.close()


def test_freivalds_on_a_warm_call(ctx, bufs):
    """eri x against the yref the pipeline accumulates from its (partly cached) planes, at the bound of bench.py."""
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nao = 40
    Ce, df = _C(nao, 9), _df(nao)
    cache = et.EriInvariantCache(ctx)
    try:
        _run(ctx, Ce, df, bufs[1], cache=cache, stack=True)
        d_x = ctx.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, NPAIR))
        d_y = ctx.zeros((NBLK, NPAIR), np.float64)
        _run(ctx, Ce, df, bufs[1], cache=cache, stack=True, probe=(d_x, d_y))
        assert cache.stats()["hits"] == cache.stats()["entries"] > 0
        y = et.eri_times_vector_dev(ctx, bufs[1], NBLK, NPAIR, d_x).get()
        yref = d_y.get()
        assert np.abs(yref).max() > 0
        assert np.abs(y - yref).max() <= 1e-10 * max(1.0, np.abs(yref).max()), np.abs(y - yref).max()
    finally:
        cache.close()


def test_pipeline_iterations_hit(ctx, bufs, monkeypatch):
    """pipeline.iteration on a system with 224 impurity + 32 bath orbitals: the second iteration hits and reproduces the first;
    after a change of the correlation potential (another bath, the same impurity columns) it still hits and equals the dense
    result of a fresh system."""
    from libdmet_preview_amd import pipeline
    monkeypatch.delenv("DMK_ERI_INV", raising=False)
    mesh, nlo, naux, nval = (2, 2, 1), 224, 8, 32

    def ham_equal(a, b):
        for k in ("H1", "JK_core"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k

    sysm = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=11, name="inv")
    bufs[0].zero_()
    o1 = pipeline.iteration(ctx, sysm, eri_dev=bufs[0])
    assert o1["nemb"] == 256
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
        s.d_vcor = ctx.to_device(v[:SPIN])

    set_vcor(sysm)
    bufs[1].zero_()
    o3 = pipeline.iteration(ctx, sysm, eri_dev=bufs[1])
    st = sysm.eri_inv_cache.stats()
    assert (st["hits"], st["drops"]) == (2 * n_kL, 0), st
    assert _maxabs(ctx, bufs[1], bufs[0]) > 0.0                      # the bath did change
    monkeypatch.setenv("DMK_ERI_INV", "0")
    fresh = pipeline.SyntheticSystem(ctx, mesh, nlo, naux, nval, SPIN, seed=11, name="inv-dense")
    set_vcor(fresh)
    bufs[2].zero_()
    o4 = pipeline.iteration(ctx, fresh, eri_dev=bufs[2])
    assert fresh.eri_inv_cache is None
    assert _maxabs(ctx, bufs[1], bufs[2]) == 0.0
    ham_equal(o3["emb_ham"], o4["emb_ham"])
    sysm.eri_inv_cache.close()
