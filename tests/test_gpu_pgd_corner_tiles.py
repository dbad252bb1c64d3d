"""
The corner tile class of the fp32 fused PGD tile kernel (csrc/tile2d.hpp tile_class; csrc/pgd_tv2d.hip has_col and the
row class's body): a tile whose own rows end on one horizontal border and whose own columns end on one vertical border
of a 16-B aligned image skips the halo vectors beyond both, runs the row class's pass A with its ghost rows, then the
col class's ghost columns and sweep corrections, and takes both the "first row" and the "first column" handling of the
TV dual.

Method of test_gpu_pgd_edge_classes.py (its helpers are used here): launch on 16-B aligned arrays, where the census
confirms that corners are taken, and on copies one element past a 16-B boundary, where every tile is generic; compare.

Shapes (tiles are 32 x 64; interior / col / row / corner / generic by pxa_pgd_tv2d_tile_census, for every R up to 8: the
far halos of R = 8 need 48 <= 64 rows and 80 <= 128 columns):
  64 x 128    0 / 0 / 0 / 4 / 0: one corner of each orientation, nothing else;
  64 x 192    0 / 0 / 2 / 4 / 0: corners next to row tiles;
  96 x 128    0 / 2 / 0 / 4 / 0: corners next to col tiles;
  96 x 192    1 / 2 / 2 / 4 / 0: all classes;
  a stack of 2 images at 64 x 128 sharing one y.
R = 1 and 3 (TV dual in its window form; ring sweep), 6 (the benchmark's reach) and 8 in fp32; R = 6 in fp64.  The fp64
kernel and the fp32 kernels of R = 7, 8 run their corners as generic tiles (next to col and row tiles on the class
paths); the checks are the same.

Every case runs prox in {none, positive orthant, l1} x lam in {0, > 0} on independent random x and x_prev (border values
non-zero) and checks, per case: x_new of the aligned and the misaligned run bit for bit; their epilogue partials and
window partials (win_part launch) bit for bit; x_new against the oracle's PGD step within 1e-5; a second launch gives
identical bytes.

One more case at 64 x 128 has asymmetric, off-centre, per-axis different taps of reach 6: the corrections index the taps
by side on both axes at once, which a symmetric Gaussian cannot show.
"""
import ctypes as ct

import numpy as np
import pytest

import _asym_cases as ac
import oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import test_gpu_pgd_edge_classes as ec  # noqa: E402  (helpers: _plan, _solver, _run)
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd._lib import lib  # noqa: E402
from pyxu_amd.util import to_device  # noqa: E402


def _census(sh, stack, R, aligned):
    counts = (ct.c_int64 * 5)()
    assert lib.pxa_pgd_tv2d_tile_census(stack, sh[0], sh[1], R, aligned, counts) == 0
    return tuple(int(c) for c in counts)


def _check(sh, stack, R, dt, want):
    sigma = ec.SIGMA[R]
    s, y, _ = ec._plan(sh, stack, sigma, dt)
    p = s._plan
    assert max(abs(o) for o in list(p["taps0"][0]) + list(p["taps1"][0])) == R  # the reach the plan reports
    assert (p["stack"], p["B"]) == (stack, 1)
    # the aligned arrays take the corner path (fp32), the misaligned copies the generic one
    assert _census(sh, stack, R, 1) == tuple(stack * c for c in want)
    ntiles = stack * -(-sh[0] // 32) * -(-sh[1] // 64)
    assert _census(sh, stack, R, 0) == (0, 0, 0, 0, ntiles)
    taps, c = orc.gaussian_taps(sigma, 3.0, dt)
    blur = dict(arg_shape=sh, kernel=[taps, taps], center=[c, c])
    grad = lambda yk, lam: orc.deblur_tv_grad(yk, blur, y, lam, ec.MU, dict(arg_shape=sh))  # noqa: E731
    ec._run(s, sh, stack, dt, grad, f"{sh} x{stack} R={R} {np.dtype(dt).name}")


CASES = [(1, np.float32), (3, np.float32), (6, np.float32), (8, np.float32), (6, np.float64)]
IDS = ["f32-R1", "f32-R3", "f32-R6", "f32-R8", "f64-R6"]


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_four_corners_and_nothing_else(R, dt):
    _check((64, 128), 1, R, dt, (0, 0, 0, 4, 0))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_corners_next_to_row_tiles(R, dt):
    _check((64, 192), 1, R, dt, (0, 0, 2, 4, 0))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_corners_next_to_col_tiles(R, dt):
    _check((96, 128), 1, R, dt, (0, 2, 0, 4, 0))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_all_five_classes(R, dt):
    _check((96, 192), 1, R, dt, (1, 2, 2, 4, 0))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_stack_of_two_images_sharing_one_y(R, dt):
    _check((64, 128), 2, R, dt, (0, 0, 0, 4, 0))


def test_asymmetric_taps_index_the_corrections_by_side_on_both_axes():
    """Off-centre taps of reach 6, different per axis, negative ones among them, per-axis sampling, on four corner tiles:
    a correction that took the other side's taps, or the other axis's, moves the border rows / columns far beyond the
    tolerance."""
    dt = np.float32
    e = ac._e("corner_tiles", (64, 128), [([.1, .05, -.1, .2, .15, .1, .25, .05], 6),
                                          ([.2, .3, .1, -.1, .05, .05, .1, .05, .05], 2)], (1.3, 0.7), "iso", "pos", dt)
    assert ac.reach(e.taps, e.centers) == [6, 6]
    y, _ = ac.data(e, dt)
    N = y.size
    rng = np.random.default_rng(0)
    with pxrt.Precision(ec.WIDTH[dt]):
        S = pxo.Stencil(arg_shape=e.shape, kernel=ac.kernels(e, dt), center=list(e.centers), mode="constant")
        K = pxo.Gradient(arg_shape=e.shape, directions=e.dirs, sampling=e.sampling)
        f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(y)) * S
        f = f + ec.LAM * pxo.L21Norm(arg_shape=(2, *e.shape)).moreau_envelope(ec.MU) * K
        f.diff_lipschitz = 1 + 4 * (ec.LAM / ec.MU) * sum(1 / h ** 2 for h in e.sampling)
        s = ec._solver(f, N, 1, dt, rng)
    assert _census(e.shape, 1, 6, 1) == (0, 0, 0, 4, 0)
    blur, gk = ac.blur_of(e, dt), ac.grad_kw(e)
    grad = lambda yk, lam: orc.deblur_tv_grad(yk, blur, y, lam, ec.MU, gk)  # noqa: E731
    ec._run(s, e.shape, 1, dt, grad, "asymmetric taps (64, 128) R=6 float32")
