"""
GPU tests of the gridded type-3 NUFFT operator (NUFFT.type3 with method="grid3": pxa_nufft_spread_fac, pxa_nufft_deconv,
pxa_fft_ex, pxa_nufft_interp_fac), per width.

* Every golden type-3 case (tests/golden/nufft_*.npz), apply and adjoint, real and complex, stacked included.  At
  eps = 1e-2 the device is within the standing tolerance (1e-5 / 1e-12) of the float64 host restatement
  (tests/_nufft_type3_refs.py), which itself sits at least 1e-4 from the exact golden output: an operator that
  ignored `method` and returned the exact sum fails.  At eps = 1e-6 (fp64) / 1e-3 (fp32) the device is within
  RATIO_CAP_T3 eps + the standing tolerance of the golden output.
* <A x, y> = <x, A^H y> to the standing tolerance, both signs and both upsampling factors: the adjoint is the
  transposed chain on the same plans.
* real=True; sources centred at 1e4 with targets centred at -300; a zero half-width on an axis, a single target, one
  source and one target, a space-bandwidth product far below 1: within the standing tolerance of the restatement,
  plus the float64 rounding of the factors' phases (2 (D + 3) u64 max |<z, C>|: 7e-9 for the offset centres, nothing
  to speak of elsewhere).
* Two calls and two operators give the same bits; a stacked (2, 3, .) input run in several chunks of rows
  (GRID_MAX_CELLS lowered) gives the bits of the unchunked run; method="direct" is the exact operator, bit for bit.
"""
import warnings

import numpy as np
import pytest

import _nudft_refs as R
import _nufft_type3_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.operator.linop import nufft as nufft_mod  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

WIDTHS = {"f32": (np.float32, pxrt.Width.SINGLE, 0), "f64": (np.float64, pxrt.Width.DOUBLE, 1)}
EPS = {"f32": 1e-3, "f64": 1e-6}
GOLDEN = [(w, c) for w in WIDTHS for c in R.golden_cases(w) if c["typ"] == 3]


def _operator(c, eps, **kw):
    return pxo.NUFFT.type3(c["x"], c["z"], isign=c["isign"], eps=eps, real=c["real"], method="grid3", **kw)


def _device(A, c):
    return {"apply": to_NUMPY(A.apply(to_device(c["a_in"]))), "adjoint": to_NUMPY(A.adjoint(to_device(c["t_in"])))}


@pytest.mark.parametrize("w, c", GOLDEN, ids=[f"{w}-{c['id']}" for w, c in GOLDEN])
def test_golden(w, c):
    dt, width, code = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a gridded operator does not warn about eps
        with pxrt.Precision(width):
            coarse = _device(_operator(c, 1e-2), c)
            fine = _device(_operator(c, EPS[w]), c)
    bins = _dev.nufft_grid_tiles(code, c["D"])[0]
    for which in ("apply", "adjoint"):
        y = coarse[which]
        assert y.shape == c[which].shape and y.dtype == dt
        ref64 = R.op_output(c, which, T.op_transform(c, which, 1e-2, 2.0, np.float64, bins))
        err, gap = R.rel_err(y, ref64), R.rel_err(y, c[which])
        e_fine = R.rel_err(fine[which], c[which])
        print(f"{w}-{c['id']} {which}: eps=1e-2 device vs restatement {err:.2e}, vs exact {gap:.2e}; "
              f"eps={EPS[w]:g} device vs exact {e_fine:.2e}")
        assert err <= tol, which
        assert gap >= 1e-4, which  # the gridded chain, not the exact sum
        assert e_fine <= T.RATIO_CAP_T3 * EPS[w] + tol, which


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_dot(w, D):
    dt, width, _ = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    rng = np.random.default_rng([7, D])
    x = rng.uniform(-2.0, 3.0, size=(211, D)).astype(dt)
    z = rng.uniform(-9.0, 5.0, size=(157, D)).astype(dt)
    with pxrt.Precision(width):
        for sigma in (2.0, 1.25):
            for isign in (1, -1):
                A = pxo.NUFFT.type3(x, z, isign=isign, eps=EPS[w], method="grid3", upsampfac=sigma)
                v = rng.standard_normal((2, A.dim)).astype(dt)
                y = rng.standard_normal((2, A.codim)).astype(dt)
                Av = to_NUMPY(A.apply(to_device(v))).astype(np.float64)
                Aty = to_NUMPY(A.adjoint(to_device(y))).astype(np.float64)
                lhs, rhs = np.sum(Av * y, axis=-1), np.sum(v * Aty, axis=-1)
                scale = np.linalg.norm(Av, axis=-1) * np.linalg.norm(y, axis=-1)
                assert np.all(np.abs(lhs - rhs) <= tol * scale), (sigma, isign)
                # and the pair is the transform: against the exact sum, to the algorithm's error
                exact = R.nudft64(R.as_complex(v), x, z, isign)
                assert R.rel_err(R.as_complex(Av), exact) <= T.RATIO_CAP_T3 * EPS[w] + tol


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_real(w):
    dt, width, _ = WIDTHS[w]
    rng = np.random.default_rng(10)
    M, N = 300, 120
    x = rng.uniform(-np.pi, np.pi, size=(M, 2)).astype(dt)
    z = rng.uniform(-8.0, 8.0, size=(N, 2)).astype(dt)
    with pxrt.Precision(width):
        Ar = pxo.NUFFT.type3(x, z, eps=EPS[w], method="grid3", real=True)
        Ac = pxo.NUFFT.type3(x, z, eps=EPS[w], method="grid3")
        assert Ar.shape == (2 * N, M) and Ac.shape == (2 * N, 2 * M)
        y = to_device(rng.standard_normal((2, 2 * N)).astype(dt))
        back = Ar.adjoint(y)
        assert tuple(back.shape) == (2, M)
        assert torch.equal(back, Ac.adjoint(y)[..., 0::2].contiguous())  # the real part of the complex adjoint
        v = rng.standard_normal((2, M)).astype(dt)
        vc = np.zeros((2, 2 * M), dtype=dt)
        vc[..., 0::2] = v
        assert torch.equal(Ar.apply(to_device(v)), Ac.apply(to_device(vc)))


def _offset_and_degenerate(dt):
    rng = np.random.default_rng(6)
    x = 1e4 + 2.5 * rng.uniform(-1, 1, (41, 2))
    z = -300.0 + 7.0 * rng.uniform(-1, 1, (23, 2))
    flat = x.copy()
    flat[:, 1] = 3.0  # a zero half-width on an axis
    cases = dict(offset=(x, z), flat=(flat, z), one_target=(x, z[:1]), one_each=(x[:1], z[:1]),
                 tiny=(1e-3 * (x - 1e4), 1e-2 * z))
    return {k: (a.astype(dt), b.astype(dt)) for k, (a, b) in cases.items()}


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("name", ["offset", "flat", "one_target", "one_each", "tiny"])
def test_offset_centres_and_degenerate_inputs(w, name):
    dt, width, code = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    x, z = _offset_and_degenerate(dt)[name]
    rng = np.random.default_rng(8)
    v = rng.standard_normal((2, 2 * x.shape[0])).astype(dt)
    y = rng.standard_normal((2, 2 * z.shape[0])).astype(dt)
    bins = _dev.nufft_grid_tiles(code, 2)[0]
    ch = T.Chain3(x, z, EPS[w], bin_shape=bins)  # float64 chain on the points as the operator got them
    # The factors' phases <z, C> and <Dc, x - C> are computed in float64 on both sides, each to (D + 3) u64 Phi
    # (tests/_nudft_refs.py::bound: the dot product and its reduction), Phi the largest sum_d |z_d C_d| or
    # |Dc_d (x - C)_d|: 6e6 for the offset centres, where the exact sum's own float64 phase is no better.
    p = ch.p
    Phi = max(np.max(np.abs(z.astype(np.float64)) @ np.abs(p["C"])),
              np.max(np.abs(x.astype(np.float64) - p["C"]) @ np.abs(p["Dc"])))
    tol = tol + 2 * (2 + 3) * R.U[np.dtype(np.float64)] * Phi
    with pxrt.Precision(width):
        for isign in (1, -1):
            A = pxo.NUFFT.type3(x, z, isign=isign, eps=EPS[w], method="grid3")
            assert (A._nf1, A._nf2) == (ch.nf1, ch.nf2)
            got = R.as_complex(to_NUMPY(A.apply(to_device(v))))
            back = R.as_complex(to_NUMPY(A.adjoint(to_device(y))))
            # the phase of the factors is rounded once from float64: a large <Dc, x - C> or <z, C> costs nothing
            assert R.rel_err(got, ch.forward(R.as_complex(v), isign)) <= tol
            assert R.rel_err(back, ch.adjoint(R.as_complex(y), isign)) <= tol
            assert R.rel_err(got, R.nudft64(R.as_complex(v), x, z, isign)) <= T.RATIO_CAP_T3 * EPS[w] + tol


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_same_bits_chunking_and_direct_method(w, monkeypatch):
    dt, width, _ = WIDTHS[w]
    rng = np.random.default_rng(9)
    M, N = 700, 450
    x = rng.uniform(-np.pi, np.pi, size=(M, 2)).astype(dt)
    z = rng.uniform(-12.0, 12.0, size=(N, 2)).astype(dt)
    with pxrt.Precision(width):
        v = to_device(rng.standard_normal((2, 3, 2 * M)).astype(dt))
        A, B = (pxo.NUFFT.type3(x, z, eps=EPS[w], method="grid3") for _ in range(2))
        first = A.apply(v)
        assert tuple(first.shape) == (2, 3, 2 * N)
        assert torch.equal(first, A.apply(v)) and torch.equal(first, B.apply(v))
        back = A.adjoint(first)
        assert tuple(back.shape) == (2, 3, 2 * M)
        assert torch.equal(back, A.adjoint(first)) and torch.equal(back, B.adjoint(first))
        # the six rows in chunks of 6, 4 (a ragged last chunk), 2 and 1 rows: the same bits
        cells = int(np.prod(A._nf2))
        for rows in (6, 4, 2, 1):
            monkeypatch.setattr(nufft_mod, "GRID_MAX_CELLS", rows * cells + 1)
            assert A._rows(6) == rows
            assert torch.equal(A.apply(v), first) and torch.equal(A.adjoint(first), back)
        monkeypatch.setattr(nufft_mod, "GRID_MAX_CELLS", cells - 1)  # below one row: one row at a time
        assert A._rows(6) == 1 and torch.equal(A.apply(v), first)
        monkeypatch.undo()
        # method="direct" and eps = 0 are the exact operator, bit for bit
        want = _dev.nudft(to_device(x), to_device(z), 1, v.reshape(6, -1)).reshape(2, 3, -1)
        direct = pxo.NUFFT.type3(x, z, eps=EPS[w], method="direct", enable_warnings=False)
        for op in (direct, pxo.NUFFT.type3(x, z, eps=0), pxo.NUFFT.type3(x, z, eps=0, method="auto")):
            assert type(op) is nufft_mod._NUDFT and torch.equal(op.apply(v), want)
        assert not torch.equal(first, want)  # the gridded result differs (by about eps)
        assert R.rel_err(to_NUMPY(first), to_NUMPY(want)) <= T.RATIO_CAP_T3 * EPS[w] + R.NORMWISE_TOL[np.dtype(dt)]
