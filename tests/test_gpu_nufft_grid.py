"""
GPU tests of the gridded NUFFT operator (NUFFT.type1 / type2 with method="grid": pxa_nufft_spread / interp / deconv
around pxa_fft_ex).

* Every golden type-1 / type-2 case (tests/golden/nufft_*.npz), apply and adjoint, real and complex, stacked
  included; eps = 1e-4 in fp32 and 1e-9 in fp64, upsampling factor 2 (mode order 0) or 1.25 (mode order 1).  With
  e_ref64 the distance of the float64 host restatement (tests/_nufft_grid_refs.py) from the golden, the device must
  be within e_ref64 + 1e-12 of the golden in fp64, and within e_ref64 + max(1e-5, 4 d32) in fp32, d32 being the
  distance between the float32 and float64 restatements (a CPU quantity; the factor 4 is the one the large-phase
  NUDFT test allows over the fp32 restatement).
* At eps = 1e-2 the device result is within the standing tolerance of the float64 restatement, which itself sits
  some 1e-3 from the exact sum: an operator that ignored `method` and returned the exact sum fails this.
* <A x, y> = <x, A^H y> to 1e-5 / 1e-12: one plan serves both directions, so the pair is adjoint to rounding.
* Two constructions and two calls give the same bits; eps = 0 and method="direct" give the exact operator's bits.
* real=True: the adjoint's output is real.  Permuting the points permutes a type-2 output (bit for bit: each
  point's sum is its own) and leaves a type-1 output within the rounding tolerance.
"""
import warnings

import numpy as np
import pytest

import _nudft_refs as R
import _nufft_grid_refs as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

WIDTHS = {"f32": (np.float32, pxrt.Width.SINGLE, 0), "f64": (np.float64, pxrt.Width.DOUBLE, 1)}
EPS = {"f32": 1e-4, "f64": 1e-9}
GOLDEN = [(w, c) for w in WIDTHS for c in R.golden_cases(w) if c["typ"] in (1, 2)]


def _operator(c, eps, sigma=2.0, **kw):
    make = pxo.NUFFT.type1 if c["typ"] == 1 else pxo.NUFFT.type2
    return make(c["x"], c["N"], isign=c["isign"], eps=eps, real=c["real"], modeord=c["modeord"], method="grid",
                upsampfac=sigma, **kw)


def _device(A, c):
    return {"apply": to_NUMPY(A.apply(to_device(c["a_in"]))), "adjoint": to_NUMPY(A.adjoint(to_device(c["t_in"])))}


@pytest.mark.parametrize("w, c", GOLDEN, ids=[f"{w}-{c['id']}" for w, c in GOLDEN])
def test_golden(w, c):
    dt, width, code = WIDTHS[w]
    eps, sigma = EPS[w], (1.25 if c["modeord"] == 1 else 2.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a gridded operator does not warn about eps
        with pxrt.Precision(width):
            got = _device(_operator(c, eps, sigma), c)
    bins = _dev.nufft_grid_tiles(code, c["D"])[0]
    for which, y in got.items():
        assert y.shape == c[which].shape and y.dtype == dt
        ref64 = R.op_output(c, which, G.op_transform(c, which, eps, sigma, np.float64, bins))
        e_ref64, e_dev = R.rel_err(ref64, c[which]), R.rel_err(y, c[which])
        if dt == np.float64:
            slack = 1e-12
        else:
            ref32 = R.op_output(c, which, G.op_transform(c, which, eps, sigma, np.float32, bins))
            d32 = R.rel_err(ref32, ref64)
            slack = max(1e-5, 4 * d32)
        print(f"{w}-{c['id']} {which}: device {e_dev:.3e}, float64 restatement {e_ref64:.3e}, slack {slack:.1e}")
        assert e_dev <= e_ref64 + slack, which


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("cid", ["t1-d1-r0-s1-o0", "t2-d2-r1-s-1-o1", "t1-d3-r0-s-1-o1", "t2-d3-r0-s1-o0"])
def test_coarse_eps_follows_the_gridding_chain_not_the_exact_sum(w, cid):
    dt, width, code = WIDTHS[w]
    (c,) = [c for c in R.golden_cases(w) if c["id"] == cid]
    with pxrt.Precision(width):
        got = _device(_operator(c, 1e-2), c)
    bins = _dev.nufft_grid_tiles(code, c["D"])[0]
    for which, y in got.items():
        ref64 = R.op_output(c, which, G.op_transform(c, which, 1e-2, 2.0, np.float64, bins))
        gap = R.rel_err(ref64, c[which])
        err = R.rel_err(y, ref64)
        print(f"{w}-{cid} {which}: device vs restatement {err:.2e}; restatement vs exact {gap:.2e}")
        assert gap >= 1e-4  # the algorithm's own error at this eps: far outside the tolerance below
        assert err <= R.NORMWISE_TOL[np.dtype(dt)], which


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("D, N", [(1, (13,)), (2, (16, 9)), (3, (6, 5, 8))])
def test_dot(w, D, N):
    dt, width, _ = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    rng = np.random.default_rng([7, D])
    x = rng.uniform(-3 * np.pi, 3 * np.pi, size=(211, D)).astype(dt)
    with pxrt.Precision(width):
        for make in (pxo.NUFFT.type1, pxo.NUFFT.type2):
            for sigma in G.SIGMAS:
                for isign in (1, -1):
                    A = make(x, N, isign=isign, eps=EPS[w], method="grid", upsampfac=sigma, modeord=int(isign > 0))
                    v = rng.standard_normal((2, A.dim)).astype(dt)
                    y = rng.standard_normal((2, A.codim)).astype(dt)
                    Av = to_NUMPY(A.apply(to_device(v))).astype(np.float64)
                    Aty = to_NUMPY(A.adjoint(to_device(y))).astype(np.float64)
                    lhs, rhs = np.sum(Av * y, axis=-1), np.sum(v * Aty, axis=-1)
                    scale = np.linalg.norm(Av, axis=-1) * np.linalg.norm(y, axis=-1)
                    assert np.all(np.abs(lhs - rhs) <= tol * scale), (make.__name__, sigma, isign)


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_same_bits_and_direct_method(w):
    dt, width, _ = WIDTHS[w]
    rng = np.random.default_rng(9)
    x = rng.uniform(-np.pi, np.pi, size=(700, 2)).astype(dt)
    N = (24, 17)
    with pxrt.Precision(width):
        v = to_device(rng.standard_normal((3, 2 * 700)).astype(dt))
        A, B = (pxo.NUFFT.type1(x, N, eps=EPS[w], method="grid") for _ in range(2))
        first = A.apply(v)
        assert torch.equal(first, A.apply(v)) and torch.equal(first, B.apply(v))
        back = A.adjoint(first)
        assert torch.equal(back, A.adjoint(first)) and torch.equal(back, B.adjoint(first))
        # eps = 0 and method="direct" are the exact operator, bit for bit
        exact = pxo.NUFFT.type1(x, N, eps=0)
        direct = pxo.NUFFT.type1(x, N, eps=EPS[w], method="direct", enable_warnings=False)
        auto = pxo.NUFFT.type1(x, N, eps=0, method="auto")
        grid = to_device(R.mesh_unit(N, 0).reshape(-1, 2).astype(dt))
        want = _dev.nudft(to_device(x), grid, 1, v)
        for op in (exact, direct, auto):
            assert torch.equal(op.apply(v), want)
        assert not torch.equal(first, want)  # the gridded result differs (by about eps)
        assert R.rel_err(to_NUMPY(first), to_NUMPY(want)) <= G.RATIO_CAP * EPS[w] + R.NORMWISE_TOL[np.dtype(dt)]


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_real_adjoint_and_point_order(w):
    dt, width, _ = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    rng = np.random.default_rng(10)
    M, N = 300, (10, 12)
    x = rng.uniform(-np.pi, np.pi, size=(M, 2)).astype(dt)
    order = rng.permutation(M)
    with pxrt.Precision(width):
        for make, n_in in ((pxo.NUFFT.type1, M), (pxo.NUFFT.type2, 120)):
            Ar = make(x, N, eps=EPS[w], method="grid", real=True)
            Ac = make(x, N, eps=EPS[w], method="grid")
            assert Ar.dim == n_in and Ac.dim == 2 * n_in
            y = to_device(rng.standard_normal((2, Ar.codim)).astype(dt))
            back = Ar.adjoint(y)
            assert tuple(back.shape) == (2, n_in)
            assert torch.equal(back, Ac.adjoint(y)[..., 0::2].contiguous())  # the real part of the complex adjoint
            v = rng.standard_normal((2, n_in)).astype(dt)
            vc = np.zeros((2, 2 * n_in), dtype=dt)
            vc[..., 0::2] = v
            assert torch.equal(Ar.apply(to_device(v)), Ac.apply(to_device(vc)))
        u = to_device(rng.standard_normal((2, 2 * 120)).astype(dt))
        A2, A2p = (pxo.NUFFT.type2(p, N, eps=EPS[w], method="grid") for p in (x, x[order]))
        out = to_NUMPY(A2.apply(u)).reshape(2, M, 2)
        assert np.array_equal(to_NUMPY(A2p.apply(u)).reshape(2, M, 2), out[:, order])
        c = rng.standard_normal((2, M, 2)).astype(dt)
        A1, A1p = (pxo.NUFFT.type1(p, N, eps=EPS[w], method="grid") for p in (x, x[order]))
        a = to_NUMPY(A1.apply(to_device(c.reshape(2, -1))))
        b = to_NUMPY(A1p.apply(to_device(np.ascontiguousarray(c[:, order]).reshape(2, -1))))
        assert R.rel_err(a, b) <= tol
