"""
Host-side pieces of the invariant planes of the table-driven step-2 kernel (no GPU): the block table with a first block row
(dmk_half2_tab_table) still covers exactly the remaining block rows, the basis hint `leading_identity_columns` finds the
impurity columns of [I_imp | bath], and the C ABI declares the new entry points.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEM = 48                                    # DMK_TAB_ITEM_INTS
MAXBLK = {2: 8, 3: 5}
SEG = {2: 7, 3: 5}                           # blocks per segment of the triangle / rectangle layout (nb > 12)
NEMBS = [32, 48, 90, 136, 192, 200, 208, 250, 256, 272, 320, 512]


def _table(nemb, occ, lo):
    from libdmet_preview_amd._lib import lib
    n, st = C.c_int(-1), (C.c_double * 3)()
    assert lib.dmk_half2_tab_table(nemb, occ, lo, None, 0, C.byref(n), st) == 0
    sizes = (n.value, tuple(st))
    buf = (C.c_int * max(1, n.value * ITEM))()
    assert lib.dmk_half2_tab_table(nemb, occ, lo, buf, n.value * ITEM, C.byref(n), st) == 0
    assert (n.value, tuple(st)) == sizes            # the size query and the filling call agree
    return np.asarray(buf[:n.value * ITEM], dtype=np.int64).reshape(n.value, ITEM), tuple(st)


@pytest.mark.parametrize("occ", [2, 3])
@pytest.mark.parametrize("nemb", NEMBS)
def test_table_covers_the_remaining_block_rows_once(nemb, occ):
    nb = (nemb + 15) // 16
    mb = MAXBLK[occ]
    for lo in range(nb + 1):
        tab, (useful, slots, folded) = _table(nemb, occ, lo)
        seen, nfold, nslots = [], 0, 0
        for it in tab:
            kind, R0, C0 = int(it[0]), int(it[1]), int(it[2])
            assert kind in (0, 1, 2)
            # panel origins: a rectangle lies a whole segment below the diagonal (occ 2: R0 > C0 + 6), a triangle on it
            if kind == 1:
                assert R0 > C0 + SEG[occ] - 1
            elif kind == 0:
                assert R0 == C0
            else:
                assert (R0, C0) == (0, 0) and nb <= 12
            assert kind == 2 or nb > 12
            lens = [int(it[3 + w]) for w in range(4)]
            assert sum(lens) > 0                    # an item left without a block is not pushed
            assert max(lens) <= mb
            nslots += 4 * max(lens)
            for w in range(4):
                blocks = [(R0 + (int(e) >> 8), C0 + (int(e) & 255)) for e in it[8 + w * mb: 8 + w * mb + lens[w]]]
                assert all(int(e) == 0 for e in it[8 + w * mb + lens[w]: 8 + (w + 1) * mb])
                nd = (int(it[7]) >> (8 * w)) & 255
                ndiag = sum(1 for r, c in blocks if r == c)
                assert nd <= 2 and nd == min(2, ndiag)
                assert all(r == c for r, c in blocks[len(blocks) - nd:])        # the counted diagonal blocks come last
                if kind == 1:
                    assert ndiag == 0
                    assert all(0 <= r - R0 < 4 and 0 <= c - C0 < 8 for r, c in blocks)     # inside the 64 x 128 panels
                else:
                    width = 12 if kind == 2 else 8
                    assert all(0 <= r - R0 < width and 0 <= c - C0 < width for r, c in blocks)
                nfold += nd
                seen += blocks
        want = sorted((r, c) for r in range(lo, nb) for c in range(r + 1))
        assert sorted(seen) == want, (nemb, occ, lo)
        assert useful == len(want) == nb * (nb + 1) // 2 - lo * (lo + 1) // 2
        assert slots == nslots and folded == nfold
        if lo == nb:
            assert len(tab) == 0 and (useful, slots, folded) == (0.0, 0.0, 0.0)


def test_table_rejects_bad_arguments():
    from libdmet_preview_amd._lib import lib
    n, st = C.c_int(), (C.c_double * 3)()
    assert lib.dmk_half2_tab_table(136, 4, 0, None, 0, C.byref(n), st) != 0          # occ is 2 or 3
    assert lib.dmk_half2_tab_table(16, 3, 0, None, 0, C.byref(n), st) != 0           # below the kernel's smallest nemb
    assert lib.dmk_half2_tab_table(136, 3, -1, None, 0, C.byref(n), st) != 0
    buf = (C.c_int * ITEM)()
    assert lib.dmk_half2_tab_table(136, 3, 0, buf, ITEM, C.byref(n), st) != 0        # three items do not fit one
    assert lib.dmk_half2_tab_table(136, 3, 0, None, 0, C.byref(n), None) == 0 and n.value == 3


def test_slot_counts_of_the_design_note():
    """Occupied block slots dense / warm at the kernel's default occupancy point (wide items: 3, segments: 2)."""
    for nemb, ninv, dense, warm in ((136, 104, 48, 24), (200, 150, 96, 52), (250, 200, 144, 68), (272, 200, 164, 88), (90, 50, 24, 16)):
        occ = 3 if (nemb + 15) // 16 <= 12 else 2
        assert _table(nemb, occ, 0)[1][1] == dense
        assert _table(nemb, occ, ninv // 16)[1][1] == warm


def _basis(spin, ncells, nlo, nimp, nbath, seed=0):
    rng = np.random.default_rng(seed)
    b = np.zeros((spin, ncells, nlo, nimp + nbath))
    b[:, 0, np.arange(nimp), np.arange(nimp)] = 1.0
    b[:, :, :, nimp:] = rng.standard_normal((spin, ncells, nlo, nbath))
    b[:, 0, :nimp, nimp:] = 0.0
    return b


@pytest.mark.parametrize("ncells", [1, 2, 3])
@pytest.mark.parametrize("spin", [1, 2])
def test_leading_identity_columns(ncells, spin):
    from libdmet_preview_amd.basis_transform import eri_transform as et
    nlo, nimp, nbath = 24, 20, 9
    b = _basis(spin, ncells, nlo, nimp, nbath)
    assert et.leading_identity_columns(b) == nimp
    if spin == 1:
        assert et.leading_identity_columns(b[0]) == nimp              # (ncells, nlo, nemb)
    for j, cell, row in ((7, 0, 7), (3, 0, 15), (12, ncells - 1, 2)):
        p = b.copy()
        p[spin - 1, cell, row, j] += 1e-13
        assert et.leading_identity_columns(p) == j
    # a rotated impurity spans the same space but is no identity block: no hint
    q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((nimp, nimp)))
    r = b.copy()
    r[:, 0, :nimp, :nimp] = q
    assert et.leading_identity_columns(r) == 0
    assert et.leading_identity_columns(np.zeros((spin, ncells, nlo, 5))) == 0
    assert et.leading_identity_columns(np.eye(nlo * ncells).reshape(1, ncells, nlo, nlo * ncells)) == nlo


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "libdmetk.h")).read()
    for name in ("dmk_eri_attach_cache_cols", "dmk_half2_tab_table"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+DMK_TAB_ITEM_INTS\s+%d\b" % ITEM, text)
    from libdmet_preview_amd import _lib
    assert "dmk_eri_attach_cache_cols" in _lib.PROTOTYPES and "dmk_half2_tab_table" in _lib.PROTOTYPES
