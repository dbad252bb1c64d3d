"""
Row reductions (csrc/reduce.hip) through pyxu_amd._dev.row_reduce / row_reduce_pow at every partition the launcher
can choose: one workgroup per row, nb = 2, nb > 64 (row_final_kernel's lane-strided loop), nb = 1024, the
cap-limited nb of many rows, rows that are no multiple of 4, and more rows than grid.y takes (two slabs).  Sums are
held to the classical n 2^-53 sum |t| bound against float64 NumPy (tests/_prim_refs.py), the order statistics and
counts to exact equality; NaN and +-inf follow numpy.linalg.norm / numpy.min / numpy.max.
"""
import functools

import numpy as np
import pytest

import _prim_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.opt.stop as pxst  # noqa: E402
from pyxu_amd import _dev  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
POWS = (0, 0.5, 1, 3)


def _cases():
    out = []
    for shape, which in R.RED_SHAPES:
        for d in ("f32", "f64"):
            if which == "both" or d == "f32":
                out.append(pytest.param(shape, d, which == "f32_few", id=f"{shape[0]}x{shape[1]}-{d}"))
    return out


def _check(tag, got, ref, bound, delta):
    got = R.to_host(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, (tag, got.shape, ref.shape)
    if delta is None:  # exact
        np.testing.assert_array_equal(got, ref, err_msg=tag)
        return
    err = np.abs(got - ref)
    print(tag, "max err", float(err.max()), "bound", float(bound.max()), "min |term|", float(np.min(delta)))
    assert (delta >= 10 * bound).all(), (tag, "a dropped element must stand 10x above the bound")
    assert (err <= bound).all(), (tag, float(err.max()), float(bound.max()), int(np.argmax(err > bound)))


@pytest.mark.parametrize("shape,d,few", _cases())
def test_row_reduce_paths(shape, d, few):
    """All nine PXA_RED_* ops and row_reduce_pow for p in {0, 0.5, 1, 3}, with and without y; twice, same bits."""
    dt = DT[d]
    x, y = R.sum_values_pair(shape, dt)
    xd, yd = R.to_dev(x), R.to_dev(y)
    for op in (("SUMSQ", "MAX", "MAXABS") if few else tuple(R.RED)):
        needs_y = op in R.RED_NEEDS_Y
        ref, bound, delta = R.red_ref(op, x, y if needs_y else None)
        for with_y in ((True,) if needs_y else (False,) if few else (False, True)):  # y is ignored when not needed
            got = _dev.row_reduce(R.RED[op], xd, yd if with_y else None)
            tag = f"{op} y={with_y} {shape} {d}"
            _check(tag, got, ref, bound, delta)
            assert torch.equal(got, _dev.row_reduce(R.RED[op], xd, yd if with_y else None)), f"{tag}: bits differ"
    if few:
        return
    for p in (0.5, 1, 3):
        for with_y in (False, True):
            ref, bound, delta = R.pow_ref(p, x, y if with_y else None)
            got = _dev.row_reduce_pow(p, xd, yd if with_y else None)
            _check(f"pow p={p} y={with_y} {shape} {d}", got, ref, bound, delta)
            assert torch.equal(got, _dev.row_reduce_pow(p, xd, yd if with_y else None))
    # p = 0 counts the non-zeros of x - y: one planted zero in the last row (of the last slab)
    xz, yz = x.copy(), y.copy()
    xz[-1, 0] = yz[-1, 0] = 0
    for with_y in (False, True):
        ref = R.pow_ref(0, xz, yz if with_y else None)[0]
        assert ref[-1] == shape[1] - 1
        _check(f"pow p=0 y={with_y} {shape} {d}", _dev.row_reduce_pow(0, R.to_dev(xz), R.to_dev(yz) if with_y else None),
               ref, None, None)


@pytest.mark.parametrize("d", ["f32", "f64"])
def test_last_rows_of_the_second_slab(d):
    """(65538, 3): rows 65535.. come from a second launch; every row is checked, the last three by name."""
    dt = DT[d]
    x = R.sum_values((65538, 3), dt)
    xd = R.to_dev(x)
    for op in ("SUMSQ", "MAXABS", "MIN"):
        got = R.to_host(_dev.row_reduce(R.RED[op], xd))
        ref, bound, _ = R.red_ref(op, x)
        assert (np.abs(got[-3:] - ref[-3:]) <= bound[-3:]).all(), op
        assert (np.abs(got - ref) <= bound).all(), op
    out = torch.empty((65538,), dtype=torch.float64, device="cuda")
    res = _dev.row_reduce_pow(1.0, xd, out=out)
    assert res.data_ptr() == out.data_ptr()
    ref, bound, _ = R.pow_ref(1, x)
    assert (np.abs(R.to_host(out) - ref) <= bound).all()


@pytest.mark.parametrize("d", ["f32", "f64"])
def test_empty_rows(d):
    x = torch.empty((3, 0), dtype=torch.float32 if d == "f32" else torch.float64, device="cuda")
    for op in R.RED_SUMS:
        got = R.to_host(_dev.row_reduce(R.RED[op], x, x if op in R.RED_NEEDS_Y else None))
        np.testing.assert_array_equal(got, np.zeros(3))
    for p in POWS:
        np.testing.assert_array_equal(R.to_host(_dev.row_reduce_pow(p, x)), np.zeros(3))


@functools.lru_cache(maxsize=4)
def _nan_base(n, d):
    x = R.sum_values((3, n), DT[d])
    x.setflags(write=False)
    return x


def _nan_positions(n):
    chunk = -(-n // R.blocks_per_row(3, n))
    return sorted({0, 63, 64, 255, 256, chunk - 1, chunk, n - 1})


@pytest.mark.parametrize("d", ["f32", "f64"])
@pytest.mark.parametrize("n", [4097, 262145])
def test_nan_propagates_from_every_position(n, d):
    """One NaN in row 1 of a 3-row input, at the first / last lane of a wavefront, of a workgroup pass and of a
    chunk: MIN, MAX, MAXABS, SUMSQ, ABS, SUM and row_reduce_pow(p > 0) give NaN for that row only; NEGCNT does not
    count it; p = 0 counts it as a non-zero (numpy.linalg.norm(ord=0))."""
    base = _nan_base(n, d)
    clean = {op: R.red_ref(op, base) for op in ("MIN", "MAX", "MAXABS", "SUMSQ", "ABS", "SUM", "NEGCNT")}
    for pos in _nan_positions(n):
        x = base.copy()
        x[1, pos] = np.nan
        xd = R.to_dev(x)
        for op in ("MIN", "MAX", "MAXABS", "SUMSQ", "ABS", "SUM"):
            got = R.to_host(_dev.row_reduce(R.RED[op], xd))
            assert np.isnan(got[1]), (op, pos, got)
            ref, bound, _ = clean[op]
            assert (np.abs(got[[0, 2]] - ref[[0, 2]]) <= bound[[0, 2]]).all(), (op, pos)
        for p in (0.5, 1, 3):
            got = R.to_host(_dev.row_reduce_pow(p, xd))
            assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all(), (p, pos, got)
        np.testing.assert_array_equal(R.to_host(_dev.row_reduce(R.RED["NEGCNT"], xd)), R.red_ref("NEGCNT", x)[0])
        np.testing.assert_array_equal(R.to_host(_dev.row_reduce_pow(0, xd)), np.full(3, float(n)))


@pytest.mark.parametrize("d", ["f32", "f64"])
def test_infinities_and_negative_zero(d):
    dt = DT[d]
    x = R.sum_values((3, 4097), dt)
    x[0, 100] = np.inf
    x[1, 4096] = -np.inf
    xd = R.to_dev(x)
    for op in ("MAXABS", "MIN", "MAX"):
        np.testing.assert_array_equal(R.to_host(_dev.row_reduce(R.RED[op], xd)), R.red_ref(op, x)[0], err_msg=op)
    assert R.to_host(_dev.row_reduce(R.RED["MAXABS"], xd))[1] == np.inf
    assert R.to_host(_dev.row_reduce(R.RED["MIN"], xd))[1] == -np.inf
    assert R.to_host(_dev.row_reduce(R.RED["MAX"], xd))[0] == np.inf
    z = np.abs(R.sum_values((2, 300), dt))
    z[0, ::3] = -0.0
    z[1, 7] = -1.0
    np.testing.assert_array_equal(R.to_host(_dev.row_reduce(R.RED["NEGCNT"], R.to_dev(z))), [0.0, 1.0])


# ----------------------------------------------------------------------------- callers
@pytest.mark.parametrize("d", ["f32", "f64"])
@pytest.mark.parametrize("norm", [1, 2, np.inf, 3])
def test_rownorm_of_a_nan_iterate_is_nan(norm, d):
    x = R.sum_values((2, 4097), DT[d])
    x[1, 1] = np.nan  # not the last element its thread folds: a NaN-dropping max loses it
    v = pxst._rownorm(R.to_dev(x), norm)
    assert v.shape == (2, 1)
    assert np.isnan(v[1, 0]) and np.isfinite(v[0, 0]), v


@pytest.mark.parametrize("d", ["f32", "f64"])
def test_abs_error_inf_norm_does_not_fire_on_nan(d):
    """numpy.linalg.norm(ord=inf) of a diverged iterate is NaN, and NaN <= eps is false."""
    x = R.sum_values((4097,), DT[d])
    x[1] = np.nan
    crit = pxst.AbsError(eps=1e3, var="x", norm=np.inf)
    assert crit.stop({"x": R.to_dev(x)}) is False
    x[1] = 1.0
    assert crit.stop({"x": R.to_dev(x)}) is True


@pytest.mark.parametrize("d", ["f32", "f64"])
@pytest.mark.parametrize("ord_", [None, 0, 1, 3, np.inf])
def test_xp_norm_shapes(ord_, d):
    import pyxu_amd.xp as xp

    dt = DT[d]
    x = R.sum_values((2, 3, 17), dt)
    x[0, 0, 0] = 0
    xd = R.to_dev(x)
    ref = np.linalg.norm(x.astype(np.float64), ord=ord_, axis=-1)
    v = xp.linalg.norm(xd, ord=ord_, axis=-1)
    assert tuple(v.shape) == (2, 3) and R.to_host(v).dtype == dt
    assert (np.abs(R.to_host(v) - ref) <= R.OP_TOL[dt] * ref).all()
    vk = xp.linalg.norm(xd, ord=ord_, axis=-1, keepdims=True)
    assert tuple(vk.shape) == (2, 3, 1)
    np.testing.assert_array_equal(R.to_host(vk)[..., 0], R.to_host(v))
