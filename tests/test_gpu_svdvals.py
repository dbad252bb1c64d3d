"""
``LinOp.svdvals(k, which)`` on the device, in both precisions, against ``numpy.linalg.svd`` of the operator's own
matrix (``asarray(xp=numpy)``, taken to float64).

Bound (derived in tests/_svdvals_refs.py; on the squares, because the method computes eigenvalues of the Gram):

    |sigma_hat^2 - sigma^2| <= (tol + 2 (M + N) eps) sigma_max^2,      tol = 0 -> 32 eps,

with eps of the runtime precision: the Ritz residual theorem for the first term, the worst-case summation error of the
two products A v and A^T u for the second.  It covers null values (A3: sigma_hat can only be O(sqrt(eps)) sigma_max).
The cases keep their wanted values at least 10x the float64 bound away from the unwanted ones
(tests/test_svdvals_refs.py asserts it); in float32 the tightest one, the SM end of A1, keeps 4.5x (gap 0.0446 on the
squares, bound 0.00997), still more than the 2x that makes the sorted comparison unambiguous.
"""
import warnings

import numpy as np
import pytest

import _svdvals_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.math._lanczos as lz  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.info.warning import DenseWarning  # noqa: E402

WIDTHS = [pxrt.Width.SINGLE, pxrt.Width.DOUBLE]
IDS = ["f32", "f64"]


def _from_array(A, width):
    return pxa.LinOp.from_array(np.ascontiguousarray(A, dtype=width.value))


def _convolve(width):
    return pxo.Convolve(arg_shape=R.A2_SHAPE, kernel=[np.asarray(t, dtype=width.value) for t in R.A2_KERNEL],
                        center=list(R.A2_CENTER), mode="constant")


# name -> (operator factory (width) -> LinOp, k, which, extra keywords)
CASES = {
    "A1-LM": (lambda w: _from_array(R.matrix_a1(), w), 4, "LM", {}),
    "A1-SM": (lambda w: _from_array(R.matrix_a1(), w), 4, "SM", {}),
    "A1T-LM": (lambda w: _from_array(R.matrix_a1(True), w), 4, "LM", {}),
    "A1T-SM": (lambda w: _from_array(R.matrix_a1(True), w), 4, "SM", {}),
    "A1-LM-ncv12": (lambda w: _from_array(R.matrix_a1(), w), 4, "LM", dict(ncv=12)),  # forced restarts
    "A2-LM": (lambda w: _from_array(R.matrix_a2(), w), 3, "LM", {}),
    "A2-conv-LM": (_convolve, 3, "LM", {}),
    "A3-LM": (lambda w: _from_array(R.matrix_a3(), w), 5, "LM", {}),
    "A3-SM": (lambda w: _from_array(R.matrix_a3(), w), 5, "SM", {}),
    "A4-LM": (lambda w: _from_array(R.matrix_a4(), w), 3, "LM", {}),
    "A4-SM": (lambda w: _from_array(R.matrix_a4(), w), 3, "SM", {}),
    "3xA1-LM": (lambda w: 3 * _from_array(R.matrix_a1(), w), 4, "LM", {}),
    "A1.T-LM": (lambda w: _from_array(R.matrix_a1(), w).T, 4, "LM", {}),
    "blockdiag-LM": (lambda w: pxo.block_diag([_from_array(R.matrix_a4(), w), _from_array(R.matrix_b12(), w)]), 5, "LM", {}),
    "blockdiag-small-LM": (lambda w: pxo.block_diag([_from_array(R.matrix_b12(), w),
                                                      _from_array(np.diag([20.0, 0.5, 0.25]), w)]), 5, "LM", {}),
}


def _reference(op, k, which):
    A = np.asarray(op.asarray(xp=np), dtype=np.float64)
    s = np.sort(np.linalg.svd(A, compute_uv=False))
    return (s[-k:] if which == "LM" else s[:k]), s[-1]


def _check(got, ref, smax, shape, width, k, tol=0.0):
    eps = float(np.finfo(width.value).eps)
    bound = R.sq_bound(shape, smax, eps, tol)
    got64 = np.asarray(got, dtype=np.float64)
    print(f"max |d sigma^2| {np.abs(got64**2 - ref**2).max():.3e}  bound {bound:.3e}")
    assert got.shape == (k,) and got.dtype == width.value
    assert np.all(np.diff(got64) >= 0)
    # sigma_hat is returned in the runtime precision: its rounding moves the square by at most 2 eps sigma_max^2
    assert np.all(np.abs(got64**2 - ref**2) <= bound + 2 * eps * smax**2)


@pytest.mark.parametrize("width", WIDTHS, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_svdvals_matches_dense_svd(name, width):
    make, k, which, kw = CASES[name]
    with pxrt.Precision(width), warnings.catch_warnings():
        warnings.simplefilter("ignore", DenseWarning)  # the 3 x 3 block of blockdiag-small takes the dense path
        op = make(width)
        stats = {}
        got = op.svdvals(k=k, which=which, _stats=stats, **kw)
        ref, smax = _reference(op, k, which)
    print(name, IDS[WIDTHS.index(width)], stats)
    _check(got, ref, smax, op.shape, width, k)


@pytest.mark.parametrize("width", WIDTHS, ids=IDS)
def test_lanczos_k1_agrees_with_power_iteration(width):
    with pxrt.Precision(width):
        op = _from_array(R.matrix_a2(), width)
        # The power iteration's tol stops it when two successive iterates agree, which is no bound on its error: on
        # this blur ((sigma_2 / sigma_1)^2 = 0.957 per step) the default tol = 1e-6 leaves sigma 9.5e-6 off.  With
        # tol = 0 it runs to its fixed point (335 steps in float64) or to n_iter, and its own tol adds nothing to the
        # bound: what is left is the rounding of both results to the runtime precision.
        power = op.svdvals(k=1, which="LM", tol=0.0, n_iter=1000)
        lanc = op.svdvals(k=1, solver="lanczos")
        ref, smax = _reference(op, 1, "LM")
    _check(lanc, ref, smax, op.shape, width, 1)
    eps = float(np.finfo(width.value).eps)
    print(f"power {float(power[0]):.17g} lanczos {float(lanc[0]):.17g} svd {float(ref[0]):.17g}")
    assert abs(float(lanc[0]) ** 2 - float(power[0]) ** 2) <= R.sq_bound(op.shape, smax, eps) + 4 * eps * smax**2
    assert power.shape == (1,) and power.dtype == width.value


@pytest.mark.parametrize("width", WIDTHS, ids=IDS)
@pytest.mark.parametrize("which", ["LM", "SM"])
def test_dense_path(width, which):
    A = R.matrix_b12()[:, :10]  # 12 x 10: min(shape) // 2 = 5
    with pxrt.Precision(width):
        op = _from_array(A, width)
        with pytest.warns(DenseWarning):
            got = op.svdvals(k=5, which=which)
        ref, smax = _reference(op, 5, which)
    assert got.shape == (5,) and got.dtype == width.value and np.all(np.diff(got) >= 0)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 8 * 10 * float(np.finfo(width.value).eps) * smax)


def test_argument_errors():
    with pxrt.Precision(pxrt.Width.SINGLE):
        op = _from_array(R.matrix_b12(), pxrt.Width.SINGLE)
        with pytest.raises(ValueError):
            op.svdvals(k=13)
        with pytest.raises(ValueError):
            op.svdvals(k=2, which="XX")
        with pytest.raises(ValueError):
            op.svdvals(k=1, which="XX")
        assert op.svdvals(k=2, which=" lm ", gpu=True, unknown_keyword=1).shape == (2,)


@pytest.mark.parametrize("width", WIDTHS, ids=IDS)
def test_cycle_cap_raises(width):
    with pxrt.Precision(width):
        op = _from_array(R.matrix_a1(), width)
        with pytest.raises(RuntimeError, match="converged"):
            op.svdvals(k=4, which="SM", maxiter=1)


@pytest.mark.parametrize("width", WIDTHS, ids=IDS)
def test_fused_and_composed_agree(width, monkeypatch):
    with pxrt.Precision(width):
        op = _from_array(R.matrix_a1(), width)
        ref, smax = _reference(op, 4, "LM")
        out = {}
        for fused in (True, False):
            monkeypatch.setattr(lz, "_FUSED", fused)
            out[fused] = op.svdvals(k=4, which="LM", ncv=12)
            _check(out[fused], ref, smax, op.shape, width, 4)
    eps = float(np.finfo(width.value).eps)
    d = np.abs(out[True].astype(np.float64) ** 2 - out[False].astype(np.float64) ** 2)
    assert np.all(d <= R.sq_bound(op.shape, smax, eps) + 2 * eps * smax**2)


def test_v0_and_seed():
    with pxrt.Precision(pxrt.Width.DOUBLE):
        op = _from_array(R.matrix_a1(), pxrt.Width.DOUBLE)
        ref, smax = _reference(op, 2, "LM")
        a = op.svdvals(k=2, seed=3)
        b = op.svdvals(k=2, v0=np.random.default_rng(3).standard_normal(200))
        np.testing.assert_array_equal(a, b)  # the default start vector is the seeded host draw
        _check(a, ref, smax, op.shape, pxrt.Width.DOUBLE, 2)
