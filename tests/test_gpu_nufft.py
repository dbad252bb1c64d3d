"""
GPU tests of the NUFFT operator (pyxu_amd/operator/linop/nufft.py on pxa_nudft).

* Every golden case (tests/golden/nufft_*.npz: the reference's own eps = 0 results; types 1, 2, 3, D = 1, 2, 3,
  real / complex, both signs, both mode orders, stacked inputs): each output within the element-wise bound of the
  float64 sum (tests/_nudft_refs.py) and norm-wise within 1e-5 (fp32) / 1e-12 (fp64) of the golden.
* ``A.asarray() @ v`` against ``apply(v)``, the dot test <A x, y> = <x, A^H y>, non-contiguous and stacked inputs,
  inputs of the other width (cast with a PrecisionWarning).
* One large-phase type-3 case (|x| <= 5, |z| <= 200): no fixed figure applies; the device's norm-wise error against
  float64 must be at most 4 x the error of the fp32 restatement of the reference's formula on the same inputs (the
  phase-rounding term is common to both; summation order and sine / cosine differ).
"""
import warnings

import numpy as np
import pytest

import _nudft_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.operator.linop.stencil import PrecisionWarning  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

WIDTHS = {"f32": (np.float32, pxrt.Width.SINGLE), "f64": (np.float64, pxrt.Width.DOUBLE)}
GOLDEN = [(w, c) for w in WIDTHS for c in R.golden_cases(w)]


def _operator(c, **kw):
    if c["typ"] == 1:
        return pxo.NUFFT.type1(c["x"], c["N"], isign=c["isign"], eps=0, real=c["real"], modeord=c["modeord"], **kw)
    if c["typ"] == 2:
        return pxo.NUFFT.type2(c["x"], c["N"], isign=c["isign"], eps=0, real=c["real"], modeord=c["modeord"], **kw)
    return pxo.NUFFT.type3(c["x"], c["z"], isign=c["isign"], eps=0, real=c["real"], **kw)


@pytest.mark.parametrize("w, c", GOLDEN, ids=[f"{w}-{c['id']}" for w, c in GOLDEN])
def test_golden(w, c):
    dt, width = WIDTHS[w]
    with pxrt.Precision(width):
        A = _operator(c)
        got = {"apply": to_NUMPY(A.apply(to_device(c["a_in"]))), "adjoint": to_NUMPY(A.adjoint(to_device(c["t_in"])))}
    for which, y in got.items():
        assert y.shape == c[which].shape and y.dtype == dt
        ratio, err = R.op_worst_ratio(c, which, y, dt), R.rel_err(y, c[which])
        print(f"{w}-{c['id']} {which}: worst |dev - ref64| / bound {ratio:.3f}, norm-wise vs golden {err:.2e}")
        assert ratio <= 1.0, which
        assert err <= R.NORMWISE_TOL[np.dtype(dt)], which


def _small_ops(rng, dt):
    x = rng.uniform(-np.pi, np.pi, size=(41, 2)).astype(dt)
    z = rng.uniform(-6, 6, size=(23, 2)).astype(dt)
    for real in (False, True):
        yield pxo.NUFFT.type1(x, (4, 5), isign=-1, eps=0, real=real, modeord=1)
        yield pxo.NUFFT.type2(x, (4, 5), isign=1, eps=0, real=real)
        yield pxo.NUFFT.type3(x, z, isign=-1, eps=0, real=real)


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_matrix_and_dot(w):
    dt, width = WIDTHS[w]
    tol = R.NORMWISE_TOL[np.dtype(dt)]
    rng = np.random.default_rng(5)
    with pxrt.Precision(width):
        for A in _small_ops(rng, dt):
            Amat = A.asarray(xp=np, dtype=np.float64)
            assert Amat.shape == A.shape
            v = rng.standard_normal((3, A.dim)).astype(dt)
            y = rng.standard_normal((3, A.codim)).astype(dt)
            Av, Aty = to_NUMPY(A.apply(to_device(v))), to_NUMPY(A.adjoint(to_device(y)))
            assert R.rel_err(Av, v.astype(np.float64) @ Amat.T) <= tol
            assert R.rel_err(Aty, y.astype(np.float64) @ Amat) <= tol
            lhs = np.sum(Av.astype(np.float64) * y, axis=-1)
            rhs = np.sum(v * Aty.astype(np.float64), axis=-1)
            scale = np.linalg.norm(Av, axis=-1) * np.linalg.norm(y, axis=-1)
            assert np.all(np.abs(lhs - rhs) <= tol * scale)
            # the device matrix is the host one, uploaded
            assert np.array_equal(to_NUMPY(A.asarray(dtype=np.float64)), Amat)


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_noncontiguous_and_stacked_inputs(w):
    dt, width = WIDTHS[w]
    rng = np.random.default_rng(6)
    with pxrt.Precision(width):
        for A in _small_ops(rng, dt):
            base = to_device(rng.standard_normal((2, 3, 2 * A.dim)).astype(dt))
            v = base[..., ::2]  # a strided view
            assert not v.is_contiguous()
            out = A.apply(v)
            assert tuple(out.shape) == (2, 3, A.codim)
            rows = torch.stack([A.apply(v[i, j].contiguous()) for i in range(2) for j in range(3)]).reshape(2, 3, -1)
            assert torch.equal(out, rows)  # a stack is its rows, bit for bit
            back = A.adjoint(out.transpose(0, 1))
            assert tuple(back.shape) == (3, 2, A.dim)
            assert torch.equal(back, A.adjoint(out.transpose(0, 1).contiguous()))
            assert tuple(A.apply(v[0, 0]).shape) == (A.codim,)


def test_other_width_is_cast_with_a_warning():
    rng = np.random.default_rng(7)
    x = rng.uniform(-np.pi, np.pi, size=(30, 1))
    with pxrt.Precision(pxrt.Width.SINGLE):
        A = pxo.NUFFT.type1(x, 8, eps=0)
        quiet = pxo.NUFFT.type1(x, 8, eps=0, enable_warnings=False)
        v32 = to_device(rng.standard_normal(A.dim).astype(np.float32))
        want = to_NUMPY(A.apply(v32))
    with pxrt.Precision(pxrt.Width.DOUBLE):
        v64 = to_device(to_NUMPY(v32).astype(np.float64))
        with pytest.warns(PrecisionWarning):
            got = A.apply(v64)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got_quiet = quiet.apply(v64)
    assert got.dtype == torch.float64  # computed in the operator's width, returned in the runtime's
    assert np.array_equal(to_NUMPY(got), want.astype(np.float64))
    assert torch.equal(got, got_quiet)


@pytest.mark.parametrize("D", [1, 3])
def test_large_phase_type3(D):
    rng = np.random.default_rng(8)
    x = rng.uniform(-5, 5, size=(300, D)).astype(np.float32)
    z = rng.uniform(-200, 200, size=(211, D)).astype(np.float32)
    w = rng.standard_normal((2, 2 * 300)).astype(np.float32)
    assert R.phi(x, z).max() > R.PHI_CAP  # outside the norm-wise cap: no fixed figure applies
    with pxrt.Precision(pxrt.Width.SINGLE):
        A = pxo.NUFFT.type3(x, z, isign=1, eps=0)
        dev = R.as_complex(to_NUMPY(A.apply(to_device(w))))
    wc = R.as_complex(w)
    ref = R.nudft64(wc, x, z, 1)
    e_dev, e_ref = R.rel_err(dev, ref), R.rel_err(R.nudft32_restated(wc, x, z, 1), ref)
    print(f"large phase D={D}: max Phi {R.phi(x, z).max():.0f}, device {e_dev:.3e}, fp32 restatement {e_ref:.3e}")
    assert e_dev <= 4 * e_ref
    ok, worst = R.within_bound(dev, wc, x, z, 1, np.float32)
    assert ok, worst
