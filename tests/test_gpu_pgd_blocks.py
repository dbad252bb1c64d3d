"""
The row-major 2 x 4 pass-B blocks of the fp32 fused PGD tile kernel (csrc/pgd_tv2d.hip pass_b_blocks, tv_block;
csrc/tile2d.hpp BlockB, sweep_w, RowSweep): the G1 sweep over b64 rows of PT in both its forms (every row live, R >= 4;
a ring of 4 rows, R <= 3), the TV dual in its exchange form (R >= 6) and its window form (smaller R), and the epilogue
that loads H^T y / x and stores x_new from the sweeping thread's registers.

Shapes: 96 x 192 is 3 x 3 tiles of 32 x 64 whose centre tile takes the interior path (wave-uniform base + 32-bit lane
offset, no bounds tests) for every R up to 8, the 8 around it the edge path; 70 x 130 has ragged last tiles in both axes
(6 rows, 2 columns) and rows that are no multiple of a 16-B vector; a stack of 2 images shares one y.
R = 1 (window form, ring sweep), 6 (the benchmark's reach: exchange form, rows-live sweep) and 8 (largest window) in
fp32, and R = 6 in fp64 (whose items and staged epilogue are unchanged) beside them.

Every case runs prox in {none, positive orthant, l1} x lam in {0, > 0} on independent random x and x_prev and checks

1. x_new from 16-B aligned arrays against x_new from copies one element past a 16-B boundary (every tile on the all-scalar
   edge path), bit for bit, with and without the RelError partials buffer;
2. the epilogue partials of the two: equal, finite and >= 0;
3. x_new against the oracle's PGD step (oracle.deblur_tv_grad + prox) within test_gpu_bench_shapes.py's 1e-5;
4. a second launch: identical bytes of x_new and of the partials.
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
L1_W = 0.05  # l1 weight: the prox threshold is tau * L1_W
SIGMA = {1: 0.3, 6: 2.0, 8: 2.5}  # Gaussian radius int(3 sigma + 0.5)
WIDTH = {np.float32: pxrt.Width.SINGLE, np.float64: pxrt.Width.DOUBLE}
PROX = {0: "none", 1: "positive orthant", 2: "l1"}


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
        s = pxs.PGD(f=f, g=pxo.PositiveOrthant(dim=N), show_progress=False)
        x0 = rng.uniform(0, 1, (stack, N) if stack > 1 else N).astype(dt)
        s.fit(x0=to_device(x0), stop_crit=pxst.MaxIter(1))
        assert s._plan is not None
    return s, y, rng


def _launch(s, x, xp, hty, lam, prox, prox_w, parts=None):
    p, m = s._plan, s._mstate
    out = _dev.empty_like(x)
    _dev.pgd_tv2d_step(x, xp, hty, out, p["stack"], p["B"], p["n0"], p["n1"], p["taps0"], p["taps1"], p["h0"],
                       p["h1"], lam, p["mu"], A, m["tau"], prox, prox_w, partials=parts)
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


def _oracle_step(sh, x, xp, y, sigma, tau, lam, prox, prox_w, dt):
    """One PGD step as oracle.pgd takes it (pgd.py:179-191), from the given x, x_prev and momentum A."""
    taps, c = orc.gaussian_taps(sigma, 3.0, dt)
    blur = dict(arg_shape=sh, kernel=[taps, taps], center=[c, c])
    yk = x - xp
    yk *= dt(A)
    yk += x
    z = orc.deblur_tv_grad(yk, blur, y, lam, MU, dict(arg_shape=sh)).copy()
    z *= -dt(tau)
    z += yk
    if prox == 1:
        return orc.positive_orthant_prox(z)
    if prox == 2:
        return orc.l1_prox(z, prox_w)
    return z


def _check(sh, stack, R, dt):
    sigma = SIGMA[R]
    s, y, rng = _plan(sh, stack, sigma, dt)
    p, m = s._plan, s._mstate
    assert max(abs(o) for o in list(p["taps0"][0]) + list(p["taps1"][0])) == R  # the reach the plan reports
    assert (p["stack"], p["B"]) == (stack, 1)
    N = int(np.prod(sh))
    # x in [-0.5, 1): both signs, so that the positive orthant and the l1 threshold each move pixels
    xh = rng.uniform(-0.5, 1, stack * N).astype(dt)
    xph = rng.uniform(-0.5, 1, stack * N).astype(dt)
    x = to_device(xh).view(m["x"].shape)
    xp = to_device(xph).view(m["x"].shape)
    hty = p["hty"]
    xm, xpm, htym = _misaligned(x), _misaligned(xp), _misaligned(hty)
    tau = m["tau"]
    for lam in (0.0, LAM):
        for prox in PROX:
            pw = tau * L1_W if prox == 2 else 0.0
            pa, pb, pr = _parts(s), _parts(s), _parts(s)
            a = _launch(s, x, xp, hty, lam, prox, pw, pa)
            b = _launch(s, xm, xpm, htym, lam, prox, pw, pb)
            c = _launch(s, x, xp, hty, lam, prox, pw)
            d = _launch(s, xm, xpm, htym, lam, prox, pw)
            r = _launch(s, x, xp, hty, lam, prox, pw, pr)
            torch.cuda.synchronize()
            a, b, c, d, r = (to_NUMPY(t).reshape(-1) for t in (a, b, c, d, r))
            pa, pb, pr = (to_NUMPY(t) for t in (pa, pb, pr))
            tag = f"{sh} x{stack} R={R} {np.dtype(dt).name} lam={lam} prox={PROX[prox]}"
            assert np.array_equal(a, b), tag
            assert np.array_equal(a, c), tag
            assert np.array_equal(a, d), tag
            assert a.tobytes() == r.tobytes() and pa.tobytes() == pr.tobytes(), tag
            assert np.array_equal(pa, pb) and np.all(np.isfinite(pa)) and np.all(pa >= 0), tag
            for i in range(stack):
                sl = slice(i * N, (i + 1) * N)
                ref = _oracle_step(sh, xh[sl], xph[sl], y, sigma, tau, lam, prox, pw, dt)
                err = rel_err(a[sl], ref)
                print(f"{tag} image {i}: rel_err {err:.3e}")
                assert err <= TOL, (tag, i, err)


CASES = [(1, np.float32), (6, np.float32), (8, np.float32), (6, np.float64)]
IDS = ["f32-R1", "f32-R6", "f32-R8", "f64-R6"]


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_interior_tile_among_edge_tiles(R, dt):
    """96 x 192: the tile at (32, 64) is interior for every R, the 8 around it take the edge path."""
    _check((96, 192), 1, R, dt)


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_ragged_last_tiles(R, dt):
    """70 x 130: last tiles of 6 rows and of 2 columns; n1 % 4 != 0, so every tile takes the scalar edge path."""
    _check((70, 130), 1, R, dt)


@pytest.mark.parametrize("R,dt", CASES, ids=IDS)
def test_stack_of_two_images_sharing_one_y(R, dt):
    _check((96, 192), 2, R, dt)
