"""
The tile-class census of the fp32 fused PGD tile kernel (pxa_pgd_tv2d_tile_classes; csrc/tile2d.hpp tile_class), on the
host: no GPU.

A 32 x 64 tile at (ty0, tx0) of an n0 x n1 image with blur reach R reads a window of 2R rows above and below and of
CA = 2R rounded up to 4 columns left and right.  The classes, written out here from their definitions:

  interior  the whole window lies inside the image;
  col       the window's rows lie inside, the tile's own columns end exactly on one border (tx0 == 0 or
            tx0 + 64 == n1) and the other side's CA columns are inside;
  row       the window's columns lie inside, the tile's own rows end exactly on one border (ty0 == 0 or ty0 + 32 == n0)
            and the other side's 2R rows are inside;
  generic   everything else, and every tile when the arrays are not 16-B aligned or n1 is no multiple of 4.
"""
import ctypes as ct

import numpy as np
import pytest

import pyxu_amd

TY, TX, V = 32, 64, 4
INTERIOR, COL, ROW, GENERIC = range(4)


def _brute(n0, n1, R, aligned):
    ca = -(-2 * R // V) * V
    out = {}
    for ty0 in range(0, n0, TY):
        for tx0 in range(0, n1, TX):
            rows_in = all(0 <= r < n0 for r in range(ty0 - 2 * R, ty0 + TY + 2 * R))
            cols_in = all(0 <= c < n1 for c in range(tx0 - ca, tx0 + TX + ca))
            if not aligned or n1 % V:
                cls = GENERIC
            elif rows_in and cols_in:
                cls = INTERIOR
            elif rows_in and ((tx0 == 0 and all(c < n1 for c in range(TX, TX + ca)))
                              or (tx0 + TX == n1 and all(c >= 0 for c in range(tx0 - ca, tx0)))):
                cls = COL
            elif cols_in and ((ty0 == 0 and all(r < n0 for r in range(TY, TY + 2 * R)))
                              or (ty0 + TY == n0 and all(r >= 0 for r in range(ty0 - 2 * R, ty0)))):
                cls = ROW
            else:
                cls = GENERIC
            out[(ty0, tx0)] = cls
    return out


def _census(n0, n1, R, aligned=1, stack=1):
    counts = (ct.c_int64 * 4)()
    assert pyxu_amd.lib.pxa_pgd_tv2d_tile_classes(stack, n0, n1, R, aligned, counts) == 0
    return tuple(int(c) for c in counts)


def _brute_counts(n0, n1, R, aligned=1, stack=1):
    cls = list(_brute(n0, n1, R, aligned).values())
    return tuple(stack * cls.count(c) for c in range(4))


@pytest.mark.parametrize("n0,n1,R,want", [
    (2048, 2048, 6, (1860, 124, 60, 4)),
    (512, 512, 6, (84, 28, 12, 4)),
    (160, 320, 6, (9, 6, 6, 4)),
] + [(96, 192, R, (1, 2, 2, 4)) for R in range(1, 9)])
def test_census(n0, n1, R, want):
    assert _census(n0, n1, R) == want
    assert _brute_counts(n0, n1, R) == want


def test_stack_scales_the_census():
    assert _census(512, 512, 6, stack=512) == tuple(512 * c for c in (84, 28, 12, 4))


@pytest.mark.parametrize("R", [1, 3, 6, 8])
def test_grazing_halo_is_generic(R):
    """96 x 200: the tile at columns 128-191 ends 8 columns before the border (its halo grazes it for R >= 3), the last
    tile is 8 columns wide: neither is a col tile, so no right-hand col tile exists."""
    cls = _brute(96, 200, R, 1)
    assert cls[(32, 192)] == GENERIC
    ca = -(-2 * R // V) * V
    assert cls[(32, 128)] == (GENERIC if 192 + ca > 200 else INTERIOR)
    assert cls[(32, 0)] == COL and cls[(0, 64)] == ROW and cls[(64, 64)] == ROW
    assert [k for k, c in cls.items() if c == COL and k[1] != 0] == []
    assert _census(96, 200, R) == _brute_counts(96, 200, R)
    if R == 6:
        assert _census(96, 200, R) == (1, 1, 2, 8)


@pytest.mark.parametrize("n0,n1,aligned", [(70, 130, 1), (32, 64, 1), (96, 64, 1), (32, 192, 1), (96, 192, 0),
                                           (2048, 2048, 0), (160, 320, 0)])
@pytest.mark.parametrize("R", [1, 6, 8])
def test_all_generic(n0, n1, aligned, R):
    tiles = -(-n0 // TY) * -(-n1 // TX)
    assert _census(n0, n1, R, aligned) == (0, 0, 0, tiles)
    assert _brute_counts(n0, n1, R, aligned) == (0, 0, 0, tiles)


def test_brute_force_agrees_over_a_sweep_of_shapes():
    rng = np.random.default_rng(0)
    shapes = [(int(a), int(b)) for a, b in zip(rng.integers(1, 300, 40), rng.integers(1, 400, 40))]
    shapes += [(32 * i, 64 * j) for i in range(1, 6) for j in range(1, 6)]
    for n0, n1 in shapes:
        for R in range(1, 9):
            assert _census(n0, n1, R) == _brute_counts(n0, n1, R), (n0, n1, R)


def test_bad_arguments():
    counts = (ct.c_int64 * 4)()
    f = pyxu_amd.lib.pxa_pgd_tv2d_tile_classes
    assert f(1, 96, 192, 0, 1, counts) == -1
    assert f(1, 96, 192, 9, 1, counts) == -1
    assert f(0, 96, 192, 6, 1, counts) == -1
    assert f(1, 96, 192, 6, 1, None) == -1
