"""
Array primitives (csrc/array.hip) through pyxu_amd._dev and the NumPy-named xp shim, bit for bit against NumPy in
the same dtype (every one of them rounds at most once; BIN_POW is held to OP_TOL): strided 2-D copies in their
vector and scalar kernels and three accumulate modes, ragged transposes, casts, diagonal writes, the unary / binary /
where maps with special values, and the any / all reduction, each also past the grid-stride wrap.
"""
import numpy as np
import pytest

import _prim_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.xp as xp  # noqa: E402
from pyxu_amd import _dev  # noqa: E402

DTS = [np.float32, np.float64]
IDS = ["f32", "f64"]
SPECIAL = [0.0, -0.0, np.nan, np.inf, -np.inf]


def _with_specials(n, dt, key=0):
    x = R.values(n, dt, key)
    k = min(n, len(SPECIAL))
    if n >= len(SPECIAL):
        x[:k] = np.roll(SPECIAL, key)[:k]
    return x


# ----------------------------------------------------------------------------- pxa_copy2d
def _copy2d_case(dt, rows, n, lds, ldd, so=0, do=0, acc=0, cs=1, neg_zero=False, expect_vec=None):
    V = R.vec_n(dt)
    ns = so + (rows - 1) * lds + (n - 1) * cs + 1
    nd = do + (rows - 1) * ldd + n
    src = R.values(ns + 3, dt, 1)
    dst = R.values(nd + 3, dt, 2)
    if neg_zero:
        src[so::2] = -0.0
    vec = cs == 1 and n % V == 0 and lds % V == 0 and ldd % V == 0 and so % V == 0 and do % V == 0
    if expect_vec is not None:
        assert vec == expect_vec, "the case does not take the kernel it is meant for"
    ri = np.arange(rows)[:, None]
    si = so + ri * lds + np.arange(n)[None, :] * cs
    di = do + ri * ldd + np.arange(n)[None, :]
    ref = dst.copy()
    s = src[si]
    ref[di] = s if acc == 0 else (ref[di] + s if acc == 1 else dt(0) + s)
    sd, dd = R.to_dev(src), R.to_dev(dst)
    _dev.copy2d(sd, dd, rows, n, lds, ldd, src_off=so, dst_off=do, accumulate=acc, col_stride=cs)
    got = R.to_host(dd)
    np.testing.assert_array_equal(got, ref)  # includes every element of dst outside the written band
    np.testing.assert_array_equal(R.to_host(sd), src)
    if acc == 2 and neg_zero:  # 0 + (-0.0) = +0.0: the one place a zero's sign is part of the contract
        assert not np.signbit(got[di][s == 0]).any()
    if acc == 0 and neg_zero:
        assert np.signbit(got[di][s == 0]).all()


@pytest.mark.parametrize("acc", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_copy2d_vector_and_scalar_kernels(dt, acc):
    V = R.vec_n(dt)
    nz = acc != 1
    _copy2d_case(dt, 7, 16 * V, 18 * V, 20 * V, so=V, do=2 * V, acc=acc, neg_zero=nz, expect_vec=True)
    _copy2d_case(dt, 7, 16 * V + 1, 18 * V, 20 * V, acc=acc, neg_zero=nz, expect_vec=False)  # odd n
    _copy2d_case(dt, 7, 16 * V, 18 * V, 20 * V, so=1, acc=acc, neg_zero=nz, expect_vec=False)  # odd src_off
    _copy2d_case(dt, 7, 16 * V, 18 * V, 20 * V, do=1, acc=acc, expect_vec=False)  # odd dst_off
    _copy2d_case(dt, 7, 16 * V, 18 * V + 1, 20 * V, acc=acc, expect_vec=False)  # odd lds
    _copy2d_case(dt, 3, 300 * V, 300 * V, 300 * V, acc=acc, expect_vec=True)  # more than one block per row
    _copy2d_case(dt, 3, 1031, 1031, 1040, acc=acc, expect_vec=False)


@pytest.mark.parametrize("acc", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_copy2d_broadcasts_and_diagonal(dt, acc):
    V = R.vec_n(dt)
    _copy2d_case(dt, 5, 8 * V, 0, 8 * V, acc=acc, expect_vec=True)  # lds = 0: one row repeated
    _copy2d_case(dt, 5, 8 * V + 1, 0, 8 * V + 3, acc=acc, expect_vec=False)
    _copy2d_case(dt, 5, 9, 1, 12, acc=acc, cs=0)  # col_stride = 0: one value per row
    _copy2d_case(dt, 1, 9, 0, 9, acc=acc, cs=0)
    _copy2d_case(dt, 33, 1, 34, 1, acc=acc)  # diagonal of a 33 x 33 matrix: lds = n + 1, n = 1
    _copy2d_case(dt, 33, 1, 34, 1, so=3, acc=acc)  # super-diagonal


@pytest.mark.parametrize("rows", [1, 7, 70000])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_copy2d_row_counts(dt, rows):
    """70000 rows: more than grid.y takes, every workgroup row loops."""
    V = R.vec_n(dt)
    for acc in (0, 1, 2):
        _copy2d_case(dt, rows, 5, 6, 7, acc=acc, expect_vec=False)
    _copy2d_case(dt, rows, 2 * V, 2 * V, 3 * V, acc=1, expect_vec=True)


# ----------------------------------------------------------------------------- pxa_transpose
@pytest.mark.parametrize("shape", [(1, 1), (31, 33), (32, 32), (33, 65), (1, 5000), (5000, 1), (40000, 3)])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_transpose(dt, shape):
    """Ragged 32 x 32 tiles; (40000, 3) has more than 1024 tile rows, so the grid wraps."""
    x = R.values(shape[0] * shape[1], dt).reshape(shape)
    xd = R.to_dev(x)
    got = _dev.transpose(xd)
    assert tuple(got.shape) == shape[::-1] and got.is_contiguous()
    np.testing.assert_array_equal(R.to_host(got), x.T)
    np.testing.assert_array_equal(R.to_host(xd), x)


# ----------------------------------------------------------------------------- pxa_cast
def test_cast_bits():
    n = R.K_MAX_GRID * R.K_BLOCK + 1001  # odd, and past the grid-stride wrap
    x = R.values(n, np.float64)
    x[:12] = [1 + 2.0**-24 + 2.0**-40, 1 + 2.0**-24, 1 + 3 * 2.0**-24, 2 - 2.0**-30, -(4 - 2.0**-40), 1e39, -1e39,
              2.0**128 - 2.0**103, np.nan, np.inf, 0.0, -0.0]
    # x[7] lies exactly half an ulp above the largest float32: ties-to-even gives inf
    x[-1] = 2 - 2.0**-26  # rounds up to the next binade, in the wrapped part
    with np.errstate(over="ignore"):
        ref32 = x.astype(np.float32)
    assert ref32[3] == 2.0 and np.isinf(ref32[5]) and np.isinf(ref32[7]) and np.isnan(ref32[8])
    like32 = torch.empty((1,), dtype=torch.float32, device="cuda")
    like64 = torch.empty((1,), dtype=torch.float64, device="cuda")
    xd = R.to_dev(x)
    d32 = _dev.cast(xd, like32)
    assert d32.dtype == torch.float32
    np.testing.assert_array_equal(R.to_host(d32), ref32)
    d64 = _dev.cast(d32, like64)
    assert d64.dtype == torch.float64
    np.testing.assert_array_equal(R.to_host(d64), ref32.astype(np.float64))
    np.testing.assert_array_equal(R.to_host(_dev.cast(xd, like64)), x)  # same-dtype copy
    np.testing.assert_array_equal(R.to_host(xd), x)


# ----------------------------------------------------------------------------- pxa_set_diag
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("N,M,k", [(1, 1, 0), (300, 7, 3), (7, 300, -4), (300, 7, -290), (5, 5, 1)])
def test_eye(N, M, k, dt):
    got = xp.eye(N, M, k=k, dtype=dt)
    assert tuple(got.shape) == (N, M)
    np.testing.assert_array_equal(R.to_host(got), np.eye(N, M, k=k, dtype=dt))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_set_diag_leaves_the_rest(dt):
    rows, ld, off = 300, 11, 4
    buf = R.values((rows - 1) * ld + off + rows + 7, dt)
    ref = buf.copy()
    ref[np.arange(rows) * ld + off + np.arange(rows)] = dt(-2.5)
    bd = R.to_dev(buf)
    _dev.set_diag(bd, rows, ld, off, -2.5)
    np.testing.assert_array_equal(R.to_host(bd), ref)


# ----------------------------------------------------------------------------- pxa_unary / pxa_binary / pxa_where
UNARY = {
    "UN_SQRT": np.sqrt,
    "UN_SIGN": np.sign,
    "UN_ABS": np.abs,
    "UN_NEG": np.negative,
    "UN_SQUARE": lambda x: x * x,
    "UN_RECIP": lambda x: x.dtype.type(1) / x,
    "UN_POSINF": lambda x: np.where(x > 0, x.dtype.type(np.inf), x.dtype.type(0)),
}
BINARY = {
    "BIN_FMAX": np.fmax, "BIN_FMIN": np.fmin, "BIN_ADD": np.add, "BIN_SUB": np.subtract, "BIN_MUL": np.multiply,
    "BIN_DIV": np.divide, "BIN_MAXIMUM": np.maximum, "BIN_MINIMUM": np.minimum,
}
SIZES = [1, 257, R.N_WRAP]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_unary(dt, n):
    x = _with_specials(n, dt)
    xd = R.to_dev(x)
    for name, fn in UNARY.items():
        with np.errstate(all="ignore"):
            ref = fn(x)
        assert ref.dtype == dt
        np.testing.assert_array_equal(R.to_host(_dev.unary(getattr(_dev, name), xd)), ref, err_msg=name)
    got = _dev.unary(_dev.UN_NEG, xd, out=xd)  # in place
    assert got.data_ptr() == xd.data_ptr()
    np.testing.assert_array_equal(R.to_host(xd), -x)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_unary_named_values(dt):
    x = np.array([0.0, 1.0, 2.5, -1.0, np.nan], dtype=dt)
    np.testing.assert_array_equal(R.to_host(_dev.unary(_dev.UN_POSINF, R.to_dev(x))), [0, np.inf, np.inf, 0, 0])
    r = R.to_host(_dev.unary(_dev.UN_RECIP, R.to_dev(np.array([0.0, 4.0], dtype=dt))))
    assert r[0] == np.inf and r[1] == 0.25


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_binary(dt, n):
    """array-array, array-scalar and scalar-array; fmax / fmin ignore NaN, maximum / minimum propagate it."""
    x, y = _with_specials(n, dt, 0), _with_specials(n, dt, 2)
    xd, yd = R.to_dev(x), R.to_dev(y)
    s = 0.7
    for name, fn in BINARY.items():
        op = getattr(_dev, name)
        with np.errstate(all="ignore"):
            refs = (fn(x, y), fn(x, dt(s)), fn(dt(s), y))
        gots = (_dev.binary(op, xd, yd), _dev.binary(op, xd, s), _dev.binary(op, s, yd))
        for form, got, ref in zip(("aa", "as", "sa"), gots, refs):
            assert ref.dtype == dt
            np.testing.assert_array_equal(R.to_host(got), ref, err_msg=f"{name} {form}")
    if n >= 257:
        nan_x = np.isnan(x) & ~np.isnan(y)
        assert nan_x.any()
        assert not np.isnan(R.to_host(_dev.binary(_dev.BIN_FMAX, xd, yd))[nan_x]).any()
        assert np.isnan(R.to_host(_dev.binary(_dev.BIN_MAXIMUM, xd, yd))[nan_x]).all()
        assert np.isnan(R.to_host(_dev.binary(_dev.BIN_MINIMUM, yd, xd))[nan_x]).all()
    # power: positive bases, OP_TOL relative, element-wise
    b = np.abs(R.values(n, dt, 3))
    e = R.rng_for("pow", n).uniform(-2.0, 2.0, n).astype(dt)
    bd, ed = R.to_dev(b), R.to_dev(e)
    for form, got, ref in (("aa", _dev.binary(_dev.BIN_POW, bd, ed), b.astype(np.float64) ** e.astype(np.float64)),
                           ("as", _dev.binary(_dev.BIN_POW, bd, s), b.astype(np.float64) ** float(dt(s))),
                           ("sa", _dev.binary(_dev.BIN_POW, s, ed), float(dt(s)) ** e.astype(np.float64))):
        err = np.abs(R.to_host(got).astype(np.float64) - ref)
        assert (err <= R.OP_TOL[dt] * np.abs(ref)).all(), (form, float((err / np.abs(ref)).max()))
    got = _dev.binary(_dev.BIN_ADD, xd, yd, out=xd)  # in place
    assert got.data_ptr() == xd.data_ptr()
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(R.to_host(xd), x + y)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_where_and_isnan(dt, n):
    x, y = _with_specials(n, dt, 0), _with_specials(n, dt, 2)
    c = R.rng_for("cond", n).integers(0, 2, n).astype(bool)
    xd, yd, cd = R.to_dev(x), R.to_dev(y), R.to_dev(c)
    np.testing.assert_array_equal(R.to_host(_dev.where(cd, xd, yd)), np.where(c, x, y))
    np.testing.assert_array_equal(R.to_host(_dev.where(cd, xd, 0.7)), np.where(c, x, dt(0.7)))
    np.testing.assert_array_equal(R.to_host(_dev.where(cd, 0.7, yd)), np.where(c, dt(0.7), y))
    np.testing.assert_array_equal(R.to_host(_dev.where(cd, 0.7, -0.3, like=xd)), np.where(c, dt(0.7), dt(-0.3)))
    got = _dev.isnan(xd)
    assert got.dtype == torch.bool
    np.testing.assert_array_equal(R.to_host(got), np.isnan(x))


# ----------------------------------------------------------------------------- pxa_bool_reduce
@pytest.mark.parametrize("n", SIZES)
def test_bool_reduce(n):
    """The deciding element at index 0, at n - 1 and behind the grid-stride wrap."""
    spots = sorted({0, n - 1, min(n - 1, R.K_MAX_GRID * R.K_BLOCK + 5)})
    for mode, neutral in ((0, False), (1, True)):
        base = np.full(n, neutral, dtype=bool)
        assert bool(_dev.bool_reduce(R.to_dev(base), mode).cpu()) is neutral
        for i in spots:
            c = base.copy()
            c[i] = not neutral
            assert bool(_dev.bool_reduce(R.to_dev(c), mode).cpu()) is (not neutral), (mode, i)


def test_bool_reduce_empty():
    c = torch.empty((0,), dtype=torch.bool, device="cuda")
    assert bool(_dev.bool_reduce(c, 0).cpu()) is False
    assert bool(_dev.bool_reduce(c, 1).cpu()) is True
    assert bool(xp.any(c).cpu()) is False and bool(xp.all(c).cpu()) is True
