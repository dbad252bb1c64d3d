"""
The five-class tile census of the fp32 fused PGD tile kernel (pxa_pgd_tv2d_tile_census; csrc/tile2d.hpp tile_class), on
the host: no GPU.

A 32 x 64 tile at (ty0, tx0) of an n0 x n1 image with blur reach R reads a window of 2R rows above and below and of
CA = 2R rounded up to 4 columns left and right.  The classes, written out here from their definitions:

  interior  the whole window lies inside the image;
  col       the window's rows lie inside, the tile's own columns end exactly on one border (tx0 == 0 or
            tx0 + 64 == n1) and the other side's CA columns are inside;
  row       the window's columns lie inside, the tile's own rows end exactly on one border (ty0 == 0 or ty0 + 32 == n0)
            and the other side's 2R rows are inside;
  corner    the tile's own rows end exactly on one horizontal border with the other side's 2R rows inside, AND its own
            columns end exactly on one vertical border with the other side's CA columns inside;
  generic   everything else, and every tile when the arrays are not 16-B aligned or n1 is no multiple of 4.

pxa_pgd_tv2d_tile_classes keeps its four counts (interior, col, row, generic), corners under generic.
"""
import ctypes as ct

import numpy as np
import pytest

import pyxu_amd

TY, TX, V = 32, 64, 4
INTERIOR, COL, ROW, CORNER, GENERIC = range(5)


def _brute(n0, n1, R, aligned):
    ca = -(-2 * R // V) * V
    out = {}
    for ty0 in range(0, n0, TY):
        for tx0 in range(0, n1, TX):
            rows_in = all(0 <= r < n0 for r in range(ty0 - 2 * R, ty0 + TY + 2 * R))
            cols_in = all(0 <= c < n1 for c in range(tx0 - ca, tx0 + TX + ca))
            # own columns / rows end exactly on one border, the halo of the other side is inside
            col_end = ((tx0 == 0 and all(c < n1 for c in range(TX, TX + ca)))
                       or (tx0 + TX == n1 and all(c >= 0 for c in range(tx0 - ca, tx0))))
            row_end = ((ty0 == 0 and all(r < n0 for r in range(TY, TY + 2 * R)))
                       or (ty0 + TY == n0 and all(r >= 0 for r in range(ty0 - 2 * R, ty0))))
            if not aligned or n1 % V:
                cls = GENERIC
            elif rows_in and cols_in:
                cls = INTERIOR
            elif rows_in and col_end:
                cls = COL
            elif cols_in and row_end:
                cls = ROW
            elif row_end and col_end:
                cls = CORNER
            else:
                cls = GENERIC
            out[(ty0, tx0)] = cls
    return out


def _census(n0, n1, R, aligned=1, stack=1):
    counts = (ct.c_int64 * 5)()
    assert pyxu_amd.lib.pxa_pgd_tv2d_tile_census(stack, n0, n1, R, aligned, counts) == 0
    return tuple(int(c) for c in counts)


def _old(n0, n1, R, aligned=1, stack=1):
    counts = (ct.c_int64 * 6)(*([-7] * 6))  # two guard words: the old export writes four counts and no more
    assert pyxu_amd.lib.pxa_pgd_tv2d_tile_classes(stack, n0, n1, R, aligned, counts) == 0
    assert (counts[4], counts[5]) == (-7, -7)
    return tuple(int(c) for c in counts[:4])


def _brute_counts(n0, n1, R, aligned=1, stack=1):
    cls = list(_brute(n0, n1, R, aligned).values())
    return tuple(stack * cls.count(c) for c in range(5))


def _agree(n0, n1, R, aligned=1, stack=1):
    """New export == brute force; corner + generic == the old export's generic, whose other counts are unchanged."""
    new, old = _census(n0, n1, R, aligned, stack), _old(n0, n1, R, aligned, stack)
    assert new == _brute_counts(n0, n1, R, aligned, stack), (n0, n1, R, aligned)
    assert old == (new[INTERIOR], new[COL], new[ROW], new[CORNER] + new[GENERIC]), (n0, n1, R, aligned)
    assert sum(new) == stack * -(-n0 // TY) * -(-n1 // TX)
    return new


@pytest.mark.parametrize("n0,n1,R,want", [
    (2048, 2048, 6, (1860, 124, 60, 4, 0)),
    (512, 512, 6, (84, 28, 12, 4, 0)),
] + [(96, 192, R, (1, 2, 2, 4, 0)) for R in range(1, 9)]
  + [(64, 128, R, (0, 0, 0, 4, 0)) for R in range(1, 9)])
def test_pinned_census(n0, n1, R, want):
    assert _agree(n0, n1, R) == want


@pytest.mark.parametrize("n0,n1,R,want", [
    (2048, 2048, 6, (1860, 124, 60, 4)),
    (512, 512, 6, (84, 28, 12, 4)),
    (160, 320, 6, (9, 6, 6, 4)),
    (96, 200, 6, (1, 1, 2, 8)),
    (70, 130, 6, (0, 0, 0, 9)),
] + [(96, 192, R, (1, 2, 2, 4)) for R in range(1, 9)])
def test_old_export_is_unchanged(n0, n1, R, want):
    assert _old(n0, n1, R) == want


def test_stack_scales_the_census():
    assert _agree(512, 512, 6, stack=512) == tuple(512 * c for c in (84, 28, 12, 4, 0))
    assert _agree(64, 128, 6, stack=2) == (0, 0, 0, 8, 0)


@pytest.mark.parametrize("R", range(1, 9))
def test_each_corner_orientation(R):
    """64 x 128 is four tiles, one corner of each orientation; 96 x 192 has them around every other class."""
    assert set(_brute(64, 128, R, 1).values()) == {CORNER}
    cls = _brute(96, 192, R, 1)
    assert [k for k, c in cls.items() if c == CORNER] == [(0, 0), (0, 128), (64, 0), (64, 128)]


@pytest.mark.parametrize("n0,n1,aligned", [
    (32, 128, 1),    # one tile high: the rows end on both borders
    (64, 64, 1),     # one tile wide
    (70, 130, 1),    # ragged in both axes, n1 % 4 != 0
    (64, 128, 0), (96, 192, 0), (2048, 2048, 0),  # some pointer off a 16-B boundary
])
@pytest.mark.parametrize("R", [1, 3, 6, 8])
def test_all_generic(n0, n1, aligned, R):
    tiles = -(-n0 // TY) * -(-n1 // TX)
    assert _agree(n0, n1, R, aligned) == (0, 0, 0, 0, tiles)


@pytest.mark.parametrize("R", [1, 3, 6, 8])
def test_ragged_and_grazing_tiles_are_generic(R):
    """96 x 200: the last tile column is 8 wide (ragged); the tiles at columns 128-191 end 8 columns before the border,
    so their halo grazes it once CA > 8 (R >= 5).  Neither kind is a corner or a col tile, in any tile row."""
    cls = _brute(96, 200, R, 1)
    ca = -(-2 * R // V) * V
    for ty0 in (0, 32, 64):
        assert cls[(ty0, 192)] == GENERIC
    for ty0 in (0, 64):
        assert cls[(ty0, 128)] == (GENERIC if ca > 8 else ROW)
        assert cls[(ty0, 0)] == CORNER
    assert [k for k, c in cls.items() if c == CORNER] == [(0, 0), (64, 0)]
    new = _agree(96, 200, R)
    assert new == ((1, 1, 2, 2, 6) if ca > 8 else (2, 1, 4, 2, 3))


def test_brute_force_agrees_over_a_sweep_of_shapes():
    rng = np.random.default_rng(0)
    shapes = [(int(a), int(b)) for a, b in zip(rng.integers(1, 300, 40), rng.integers(1, 400, 40))]
    shapes += [(int(a), 4 * int(b)) for a, b in zip(rng.integers(1, 300, 20), rng.integers(1, 100, 20))]
    shapes += [(32 * i, 64 * j) for i in range(1, 6) for j in range(1, 6)]
    seen = set()
    for n0, n1 in shapes:
        for R in range(1, 9):
            for aligned in (1, 0):
                seen.update(c for c, k in enumerate(_agree(n0, n1, R, aligned)) if k)
    assert seen == {INTERIOR, COL, ROW, CORNER, GENERIC}


def test_bad_arguments():
    """Rejected as pxa_pgd_tv2d_tile_classes rejects them."""
    for f, n in ((pyxu_amd.lib.pxa_pgd_tv2d_tile_census, 5), (pyxu_amd.lib.pxa_pgd_tv2d_tile_classes, 4)):
        counts = (ct.c_int64 * n)()
        assert f(1, 96, 192, 0, 1, counts) == -1
        assert f(1, 96, 192, 9, 1, counts) == -1
        assert f(0, 96, 192, 6, 1, counts) == -1
        assert f(1, 0, 192, 6, 1, counts) == -1
        assert f(1, 96, 0, 6, 1, counts) == -1
        assert f(1, 96, 192, 6, 1, None) == -1
