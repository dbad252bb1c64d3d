"""
The window order of the fused PGD tile kernel (csrc/pgd_tv2d.hip, Window::item: own vectors, side halo, vertical halo),
for every blur reach R = 1 .. 8 and both precisions, on the smallest grid in which one tile takes the interior path.

A 96 x 192 image is 3 x 3 tiles of 32 x 64; the tile at (32, 64) needs window rows 16 .. 80 and columns 48 .. 144 at
R = 8, all inside the image, so it runs the interior code (wave-uniform base + 32-bit lane offset, no bounds tests) for
every R, and the 8 tiles around it the edge code.  Each case checks

1. x_new from 16-B aligned arrays against x_new from copies one element past a 16-B boundary (every tile on the all-scalar
   edge path), bit for bit, with and without the RelError partials buffer;
2. the RelError partials of the two, equal and >= 0;
3. x_new against the oracle's PGD step (oracle.deblur_tv_grad + prox) within test_gpu_bench_shapes.py's tolerance.

The launches here take no window statistics (`win_part`); those sum over the tile's own items, which the order leaves as
they were, and stay covered by tests/test_gpu_solver_lag.py.

x and x_prev are independent random arrays, so yk = x + a (x - x_prev) differs from x everywhere: a mis-mapped or dropped
window vector moves pixels by O(1).
"""
import numpy as np
import pytest

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
SIGMA = {1: 0.3, 2: 0.6, 3: 1.0, 4: 1.3, 5: 1.5, 6: 2.0, 7: 2.3, 8: 2.5}  # Gaussian radius int(3 sigma + 0.5)
WIDTH = {np.float32: pxrt.Width.SINGLE, np.float64: pxrt.Width.DOUBLE}


def _problem(sh, y_images, sigma, dt, seed=0):
    rng = np.random.default_rng(seed)
    N = int(np.prod(sh))
    y = rng.standard_normal(y_images * N).astype(dt)
    with pxrt.Precision(WIDTH[dt]):
        full = sh if y_images == 1 else (y_images, *sh)
        dirs = (0, 1) if y_images == 1 else (1, 2)
        H = pxo.Gaussian(arg_shape=full, sigma=sigma if y_images == 1 else (0, sigma, sigma))
        G = pxo.Gradient(arg_shape=full, directions=dirs)
        dim = y_images * N
        l21 = pxo.L21Norm(arg_shape=(2, *full))
        f = 0.5 * pxo.SquaredL2Norm(dim=dim).asloss(to_device(y)) * H + LAM * l21.moreau_envelope(MU) * G
        f.diff_lipschitz = 1 + 8 * LAM / MU
        g = pxo.PositiveOrthant(dim=dim)
    return f, g, dim, y, rng


def _plan(sh, stack, y_images, sigma, dt):
    f, g, dim, y, rng = _problem(sh, y_images, sigma, dt)
    with pxrt.Precision(WIDTH[dt]):
        s = pxs.PGD(f=f, g=g, show_progress=False)
        rows = stack // y_images
        x0 = rng.uniform(0, 1, (rows, dim) if rows > 1 else dim).astype(dt)
        s.fit(x0=to_device(x0), stop_crit=pxst.MaxIter(1))
        assert s._plan is not None
    return s, y, rng


def _launch(s, x, xp, hty, a, parts=None):
    p, m = s._plan, s._mstate
    out = _dev.empty_like(x)
    _dev.pgd_tv2d_step(x, xp, hty, out, p["stack"], p["B"], p["n0"], p["n1"], p["taps0"], p["taps1"], p["h0"],
                       p["h1"], p["lam"], p["mu"], a, m["tau"], p["prox"], m["tau"] * p["prox_scale"], partials=parts)
    assert int(lib.pxa_pgd_tv2d_last_kernel()) == 1  # the tile kernel
    return out


def _misaligned(t):
    """A copy of t whose data pointer is one element past a 16-B boundary (the kernel's scalar path)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _parts(s):
    p = s._plan
    n = int(lib.pxa_pgd_tv2d_partials_count(p["stack"], p["n0"], p["n1"]))
    return torch.full((2 * n,), -1.0, dtype=torch.float64, device="cuda")


def _oracle_step(sh, x, xp, y, sigma, tau, dt):
    """One PGD step as oracle.pgd takes it (pgd.py:179-191), from the given x, x_prev and momentum A."""
    taps, c = orc.gaussian_taps(sigma, 3.0, dt)
    blur = dict(arg_shape=sh, kernel=[taps, taps], center=[c, c])
    yk = x - xp
    yk *= dt(A)
    yk += x
    z = orc.deblur_tv_grad(yk, blur, y, LAM, MU, dict(arg_shape=sh)).copy()
    z *= -dt(tau)
    z += yk
    return orc.positive_orthant_prox(z)


def _check(sh, images, R, dt):
    sigma = SIGMA[R]
    s, y, rng = _plan(sh, images, images, sigma, dt)
    p, m = s._plan, s._mstate
    assert max(abs(o) for o in list(p["taps0"][0]) + list(p["taps1"][0])) == R  # the reach the plan reports
    N = int(np.prod(sh))
    xh = rng.uniform(0, 1, images * N).astype(dt)
    xph = rng.uniform(0, 1, images * N).astype(dt)
    x = to_device(xh).view(m["x"].shape)
    xp = to_device(xph).view(m["x"].shape)
    hty = p["hty"]
    pa, pb = _parts(s), _parts(s)
    a = _launch(s, x, xp, hty, A, pa)
    b = _launch(s, _misaligned(x), _misaligned(xp), _misaligned(hty), A, pb)
    c = _launch(s, x, xp, hty, A)
    d = _launch(s, _misaligned(x), _misaligned(xp), _misaligned(hty), A)
    torch.cuda.synchronize()
    a, b, c, d = (to_NUMPY(t).reshape(-1) for t in (a, b, c, d))
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)
    assert np.array_equal(a, d)
    assert np.array_equal(to_NUMPY(pa), to_NUMPY(pb)) and np.all(to_NUMPY(pa) >= 0)
    for i in range(images):
        sl = slice(i * N, (i + 1) * N)
        ref = _oracle_step(sh, xh[sl], xph[sl], y[sl], sigma, m["tau"], dt)
        err = rel_err(a[sl], ref)
        print(f"{sh} image {i} R={R} {np.dtype(dt).name}: rel_err {err:.3e}")
        assert err <= TOL, (i, err)


@pytest.mark.parametrize("R", range(1, 9))
def test_fp32_every_reach(R):
    """fp32, R = 1 .. 8: one interior tile at (32, 64), 8 edge tiles around it."""
    _check((96, 192), 1, R, np.float32)


@pytest.mark.parametrize("R", [1, 6, 7, 8])
def test_fp64(R):
    """fp64 (2 elements per vector: wider side halo, twice the wave-slots); R = 7 is the one instantiation whose
    side halo takes the column form."""
    _check((96, 192), 1, R, np.float64)


def test_stack_of_two_images_with_their_own_y():
    _check((96, 192), 2, 6, np.float32)


def test_ragged_grid():
    """100 x 204: a fourth tile row and column of 4 x 12 pixels; the tile at (32, 64) is still interior."""
    _check((100, 204), 1, 6, np.float32)


def test_rows_not_vector_aligned():
    """97 x 203: n1 % 4 != 0, so every tile of both launches takes the edge path (a sanity case of the edge code's
    own use of the window order)."""
    _check((97, 203), 1, 6, np.float32)
