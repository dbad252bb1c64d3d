"""
The col and row tile classes of the fp32 fused PGD tile kernel (csrc/tile2d.hpp tile_class, ghost_cols_side, ghost_sub;
csrc/pgd_tv2d.hip win_issue, ghost_rows_coop, pass_a, tv_block, pass_b_blocks): a tile whose window is cut by exactly
one border of a 16-B aligned image skips the halo vectors beyond that border, runs the interior code on its interior
axis and corrects the R boundary rows / columns of G from ghost terms with compile-time tap indices.

Shapes (tiles are 32 x 64; interior / col / row / generic tiles by pxa_pgd_tv2d_tile_classes):
  96 x 192    3 x 3 tiles: 1 / 2 / 2 / 4 for every R up to 8 -- a left and a right col tile, a top and a bottom row tile;
  160 x 320   5 x 5 tiles: 9 / 6 / 6 / 4 -- col and row tiles next to each other and next to interior ones;
  96 x 200    a last tile of 8 columns: no right-hand col tile, and the tile at columns 128-191 (halo grazing the
              border for R >= 3) stays generic;
  70 x 130    ragged in both axes, n1 % 4 != 0: every tile generic (the parent's path, unchanged);
  a stack of 2 images at 96 x 192 sharing one y.
R = 1 and 3 (TV dual in its window form; ring sweep), 6 (the benchmark's reach: exchange form, rows-live sweep, both
blocks of a border hold corrected columns) and 8 (largest window) in fp32; R = 6 in fp64, whose col and row tiles run as
generic ones.

Every case runs prox in {none, positive orthant, l1} x lam in {0, > 0} on independent random x and x_prev (so the border
values are not zero) and checks

1. x_new from 16-B aligned arrays (col and row paths; the census confirms the classes) against x_new from copies one
   element past a 16-B boundary (every tile generic), bit for bit;
2. the epilogue partials and the window partials (win_part launch) of the two, bit for bit;
3. x_new against the oracle's PGD step within test_gpu_bench_shapes.py's 1e-5;
4. a second launch: identical bytes.

One more case has asymmetric, off-centre, per-axis different taps of reach 6 at 96 x 192: the corrections index the taps
by side, which a symmetric Gaussian cannot show.
"""
import ctypes as ct

import numpy as np
import pytest

import _asym_cases as ac
import oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import lib  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

TOL = 1e-5  # tests/test_gpu_bench_shapes.py
LAM, MU, A = 0.02, 0.01, 0.37
L1_W = 0.05  # l1 weight: the prox threshold is tau * L1_W
SIGMA = {1: 0.3, 3: 0.9, 6: 2.0, 8: 2.5}  # Gaussian radius int(3 sigma + 0.5)
WIDTH = {np.float32: pxrt.Width.SINGLE, np.float64: pxrt.Width.DOUBLE}
PROX = {0: "none", 1: "positive orthant", 2: "l1"}


def _census(sh, stack, R, aligned):
    counts = (ct.c_int64 * 4)()
    assert lib.pxa_pgd_tv2d_tile_classes(stack, sh[0], sh[1], R, aligned, counts) == 0
    return tuple(int(c) for c in counts)


def _solver(f, N, stack, dt, rng):
    s = pxs.PGD(f=f, g=pxo.PositiveOrthant(dim=N), show_progress=False)
    x0 = rng.uniform(0, 1, (stack, N) if stack > 1 else N).astype(dt)
    s.fit(x0=to_device(x0), stop_crit=pxst.MaxIter(1))
    assert s._plan is not None
    return s


def _plan(sh, stack, sigma, dt):
    """A PGD solver's fused-step plan (taps, H^T y, tau) for `stack` images of shape sh that share one y."""
    rng = np.random.default_rng(0)
    N = int(np.prod(sh))
    y = rng.standard_normal(N).astype(dt)
    with pxrt.Precision(WIDTH[dt]):
        H = pxo.Gaussian(arg_shape=sh, sigma=sigma)
        G = pxo.Gradient(arg_shape=sh, directions=(0, 1))
        l21 = pxo.L21Norm(arg_shape=(2, *sh))
        f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(y)) * H + LAM * l21.moreau_envelope(MU) * G
        f.diff_lipschitz = 1 + 8 * LAM / MU
        s = _solver(f, N, stack, dt, rng)
    return s, y, rng


def _launch(s, x, xp, hty, lam, prox, prox_w, parts=None):
    p, m = s._plan, s._mstate
    out = _dev.empty_like(x)
    _dev.pgd_tv2d_step(x, xp, hty, out, p["stack"], p["B"], p["n0"], p["n1"], p["taps0"], p["taps1"], p["h0"],
                       p["h1"], lam, p["mu"], A, m["tau"], prox, prox_w, partials=parts)
    assert int(lib.pxa_pgd_tv2d_last_kernel()) == 1  # the tile kernel
    return out


def _launch_win(s, x, xp, hty, lam, prox, prox_w, parts):
    """The win_part launch: the partials are the window's (x - x_prev) statistics over each tile's own pixels."""
    p, m = s._plan, s._mstate
    pl = _dev.PgdPlan(x, p["stack"], p["B"], p["n0"], p["n1"], p["taps0"], p["taps1"], p["h0"], p["h1"], lam, p["mu"], prox)
    out = _dev.empty_like(x)
    pl.step_wpub(x, xp, hty, out, A, m["tau"], prox_w, parts)
    torch.cuda.synchronize()
    return out


def _misaligned(t):
    """A copy of t whose data pointer is one element past a 16-B boundary (every tile on the generic path)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _parts(s):
    p = s._plan
    n = int(lib.pxa_pgd_tv2d_partials_count(p["stack"], p["n0"], p["n1"]))
    return torch.full((2 * n,), -1.0, dtype=torch.float64, device="cuda")


def _run(s, sh, stack, dt, grad, tag0):
    """The four checks for every prox and lam; grad(yk, lam) = the oracle's gradient of the smooth part at yk."""
    p, m = s._plan, s._mstate
    rng = np.random.default_rng(1)
    N = int(np.prod(sh))
    # x in [-0.5, 1): both signs, so that the positive orthant and the l1 threshold each move pixels
    xh = rng.uniform(-0.5, 1, stack * N).astype(dt)
    xph = rng.uniform(-0.5, 1, stack * N).astype(dt)
    x = to_device(xh).view(m["x"].shape)
    xp = to_device(xph).view(m["x"].shape)
    hty = p["hty"]
    for t in (x, xp, hty):
        assert t.data_ptr() % 16 == 0
    xm, xpm, htym = _misaligned(x), _misaligned(xp), _misaligned(hty)
    tau = m["tau"]
    for lam in (0.0, LAM):
        z = []
        for i in range(stack):  # the oracle's z = yk - tau grad(yk), once per lam
            sl = slice(i * N, (i + 1) * N)
            yk = xh[sl] - xph[sl]
            yk *= dt(A)
            yk += xh[sl]
            zi = grad(yk, lam).copy()
            zi *= -dt(tau)
            zi += yk
            z.append(zi)
        for prox in PROX:
            pw = tau * L1_W if prox == 2 else 0.0
            pa, pb, pr, wa, wb, wr = (_parts(s) for _ in range(6))
            a = _launch(s, x, xp, hty, lam, prox, pw, pa)
            b = _launch(s, xm, xpm, htym, lam, prox, pw, pb)
            c = _launch(s, x, xp, hty, lam, prox, pw)
            r = _launch(s, x, xp, hty, lam, prox, pw, pr)
            e = _launch_win(s, x, xp, hty, lam, prox, pw, wa)
            g = _launch_win(s, xm, xpm, htym, lam, prox, pw, wb)
            h = _launch_win(s, x, xp, hty, lam, prox, pw, wr)
            torch.cuda.synchronize()
            a, b, c, r, e, g, h = (to_NUMPY(t).reshape(-1) for t in (a, b, c, r, e, g, h))
            pa, pb, pr, wa, wb, wr = (to_NUMPY(t) for t in (pa, pb, pr, wa, wb, wr))
            tag = f"{tag0} lam={lam} prox={PROX[prox]}"
            assert a.tobytes() == b.tobytes(), tag                             # 1. x_new, aligned against generic
            assert a.tobytes() == c.tobytes() and a.tobytes() == e.tobytes() and a.tobytes() == g.tobytes(), tag
            assert pa.tobytes() == pb.tobytes() and np.all(np.isfinite(pa)) and np.all(pa >= 0), tag  # 2. epilogue partials
            assert wa.tobytes() == wb.tobytes() and np.all(np.isfinite(wa)) and np.all(wa >= 0), tag  # 2. window partials
            assert not np.array_equal(wa, pa), tag
            assert a.tobytes() == r.tobytes() and pa.tobytes() == pr.tobytes(), tag                   # 4. second launch
            assert a.tobytes() == h.tobytes() and wa.tobytes() == wr.tobytes(), tag
            for i in range(stack):                                                                    # 3. the oracle
                sl = slice(i * N, (i + 1) * N)
                ref = orc.positive_orthant_prox(z[i]) if prox == 1 else orc.l1_prox(z[i], pw) if prox == 2 else z[i]
                err = rel_err(a[sl], ref)
                print(f"{tag} image {i}: rel_err {err:.3e}")
                assert err <= TOL, (tag, i, err)


def _check(sh, stack, R, dt, census):
    sigma = SIGMA[R]
    s, y, _ = _plan(sh, stack, sigma, dt)
    p = s._plan
    assert max(abs(o) for o in list(p["taps0"][0]) + list(p["taps1"][0])) == R  # the reach the plan reports
    assert (p["stack"], p["B"]) == (stack, 1)
    # the aligned arrays take the col and row paths, the misaligned copies the generic one
    want = census(R) if callable(census) else census
    assert _census(sh, stack, R, 1) == tuple(stack * c for c in want)
    ntiles = stack * -(-sh[0] // 32) * -(-sh[1] // 64)
    assert _census(sh, stack, R, 0) == (0, 0, 0, ntiles)
    taps, c = orc.gaussian_taps(sigma, 3.0, dt)
    blur = dict(arg_shape=sh, kernel=[taps, taps], center=[c, c])
    grad = lambda yk, lam: orc.deblur_tv_grad(yk, blur, y, lam, MU, dict(arg_shape=sh))  # noqa: E731
    _run(s, sh, stack, dt, grad, f"{sh} x{stack} R={R} {np.dtype(dt).name}")


CASES = [(1, np.float32), (3, np.float32), (6, np.float32), (8, np.float32), (6, np.float64)]
IDS = ["f32-R1", "f32-R3", "f32-R6", "f32-R8", "f64-R6"]


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_one_col_and_one_row_tile_per_side(R, dt):
    """96 x 192: a left and a right col tile, a top and a bottom row tile, four corners, one interior tile."""
    _check((96, 192), 1, R, dt, (1, 2, 2, 4))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_col_and_row_tiles_side_by_side(R, dt):
    """160 x 320: three col tiles per side, three row tiles per side, around 3 x 3 interior tiles."""
    _check((160, 320), 1, R, dt, (9, 6, 6, 4))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_grazing_halo_and_ragged_last_column(R, dt):
    """96 x 200: the last tile is 8 columns wide (generic); the tile at columns 128-191 is interior while its halo of
    rup(2R, 4) columns fits into those 8 and generic beyond (R >= 3): never a col tile."""
    census = lambda r: (2, 1, 4, 5) if -(-2 * r // 4) * 4 <= 8 else (1, 1, 2, 8)  # noqa: E731
    _check((96, 200), 1, R, dt, census)


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_unaligned_rows_stay_generic(R, dt):
    """70 x 130: n1 % 4 != 0 and ragged last tiles: every tile generic, aligned pointers or not."""
    _check((70, 130), 1, R, dt, (0, 0, 0, 9))


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_stack_of_two_images_sharing_one_y(R, dt):
    _check((96, 192), 2, R, dt, (1, 2, 2, 4))


def test_asymmetric_taps_index_the_corrections_by_side():
    """Off-centre taps of reach 6, different per axis, negative ones among them, per-axis sampling: a correction that took
    the other side's taps, or the other axis's, moves the border rows / columns far beyond the tolerance."""
    dt = np.float32
    e = ac._e("edge_classes", (96, 192), [([.1, .05, -.1, .2, .15, .1, .25, .05], 6),
                                          ([.2, .3, .1, -.1, .05, .05, .1, .05, .05], 2)], (1.3, 0.7), "iso", "pos", dt)
    assert ac.reach(e.taps, e.centers) == [6, 6]
    y, _ = ac.data(e, dt)
    N = y.size
    rng = np.random.default_rng(0)
    with pxrt.Precision(WIDTH[dt]):
        S = pxo.Stencil(arg_shape=e.shape, kernel=ac.kernels(e, dt), center=list(e.centers), mode="constant")
        K = pxo.Gradient(arg_shape=e.shape, directions=e.dirs, sampling=e.sampling)
        f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(y)) * S
        f = f + LAM * pxo.L21Norm(arg_shape=(2, *e.shape)).moreau_envelope(MU) * K
        f.diff_lipschitz = 1 + 4 * (LAM / MU) * sum(1 / h ** 2 for h in e.sampling)
        s = _solver(f, N, 1, dt, rng)
    assert _census(e.shape, 1, 6, 1) == (1, 2, 2, 4)
    blur, gk = ac.blur_of(e, dt), ac.grad_kw(e)
    grad = lambda yk, lam: orc.deblur_tv_grad(yk, blur, y, lam, MU, gk)  # noqa: E731
    _run(s, e.shape, 1, dt, grad, "asymmetric taps (96, 192) R=6 float32")
