"""
The tile table of the contraction kernel with a skipped corner (dmk_dgemm_tile_table: host only, no GPU).

For every grid of 1 .. 20 and of 257 tiles per side, symmetric and rectangular, with and without a band, and every
skip in [0, tiles]: the table holds exactly the expected tiles minus the corner tm < skip && tn < skip, each once, and it is
the skip = 0 table with the corner tiles taken out -- the order of the others stays.
"""
import ctypes as C
import numpy as np
import pytest

SIZES = list(range(1, 21)) + [257]


def _table(tm, tn, symm, lo, hi, skip):
    from libdmet_preview_amd._lib import lib
    n = C.c_int64(-1)
    assert lib.dmk_dgemm_tile_table(tm, tn, int(symm), lo, hi, skip, None, 0, C.byref(n)) == 0
    out = np.zeros(max(int(n.value), 1), dtype=np.uint32)
    m = C.c_int64(-1)
    assert lib.dmk_dgemm_tile_table(tm, tn, int(symm), lo, hi, skip, out.ctypes.data_as(C.POINTER(C.c_uint32)), int(n.value),
                                    C.byref(m)) == 0
    assert m.value == n.value
    return out[:int(n.value)]


def _expected(tm, tn, symm, lo, hi, skip):
    """The set of packed tiles, from the definition."""
    a, b = np.meshgrid(np.arange(tm), np.arange(tn), indexing="ij")
    keep = np.ones_like(a, dtype=bool)
    if symm:
        keep &= b <= a
    if lo >= 0:
        sel = b if symm else a
        keep &= (sel >= lo) & (sel < hi)
    keep &= ~((a < skip) & (b < skip))
    return np.sort(((a[keep].astype(np.uint32) << 16) | b[keep].astype(np.uint32)))


def _bands(t):
    out = [(-1, -1)]
    if t >= 2:
        out.append((t // 3, max(t // 3 + 1, (2 * t) // 3)))
        out.append((t - 1, t))
    out.append((0, 1))
    return out


SAMPLED_257 = (0, 1, 7, 8, 9, 64, 157, 248, 255, 256, 257)


@pytest.mark.parametrize("symm", [True, False])
@pytest.mark.parametrize("t", SIZES)
def test_skip_tables(t, symm):
    shapes = [(t, t)] if symm else [(t, t), (t, max(1, t // 2)), (max(1, t // 2), t)]
    if t == 257 and not symm:
        shapes = [(t, t)]
    for tm, tn in shapes:
        for lo, hi in _bands(tn if symm else tm):
            dense = _table(tm, tn, symm, lo, hi, 0)
            for skip in range(0, max(tm, tn) + 1):
                tab = _table(tm, tn, symm, lo, hi, skip)
                what = (tm, tn, symm, lo, hi, skip)
                # the set from the definition, each tile once (at 257 for a sample of skips: the comparison with the dense table
                # below, whose own set is checked at skip = 0, carries it to every other skip)
                if t <= 20 or skip in SAMPLED_257:
                    assert len(np.unique(tab)) == len(tab), what
                    assert np.array_equal(np.sort(tab), _expected(tm, tn, symm, lo, hi, skip)), what
                corner = ((dense >> 16) < skip) & ((dense & 0xffff) < skip)
                assert np.array_equal(tab, dense[~corner]), what                   # same order as the dense table
                if tm == tn and skip >= tm:
                    assert len(tab) == 0, what


def test_counts_at_the_c5_grid():
    """npair 32896 = 257 tiles, corner of 157: the tiles a symmetric / a rectangular launch loses."""
    assert len(_table(257, 257, True, -1, -1, 0)) == 33153 and len(_table(257, 257, False, -1, -1, 0)) == 66049
    assert 33153 - len(_table(257, 257, True, -1, -1, 157)) == 12403
    assert 66049 - len(_table(257, 257, False, -1, -1, 157)) == 24649


def test_bad_arguments():
    from libdmet_preview_amd._lib import lib
    n = C.c_int64(0)
    assert lib.dmk_dgemm_tile_table(4, 4, 0, -1, -1, -1, None, 0, C.byref(n)) != 0
    assert lib.dmk_dgemm_tile_table(4, 5, 1, -1, -1, 0, None, 0, C.byref(n)) != 0
    out = np.zeros(4, dtype=np.uint32)
    assert lib.dmk_dgemm_tile_table(4, 4, 0, -1, -1, 0, out.ctypes.data_as(C.POINTER(C.c_uint32)), 4, C.byref(n)) != 0
    assert n.value == 16
