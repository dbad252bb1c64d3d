"""
Element-wise kernels (csrc/elementwise.hip) at their path edges, through pyxu_amd._dev, against the float64
references and derived bounds of tests/_prim_refs.py: the 16-byte vector loop of map_kernel with its n % V tail,
the scalar path of a view that starts one element into its allocation, `out` aliasing an input, the grid-stride
wrap (more than kMaxGrid * kBlock work items), the broadcast / per-row variants, and the L21 family in both its
vector kernel (group 2 / 3, second in-flight column block, outer on grid.y) and its scalar kernel.
"""
import functools

import numpy as np
import pytest

import _prim_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402

DTS = [np.float32, np.float64]
SIZES = [1, 3, 4, 5, 1023, R.N_WRAP]

# name -> (number of array inputs, scalars); bit-equal maps
EXACT = {
    "mul": (2, ()),
    "div": (1, (0.7,)),
    "add_scalar": (1, (0.7,)),
    "fill": (1, (0.7,)),
    "clip_lo": (1, (-0.5, None)),
    "clip_lohi": (1, (-0.5, 0.5)),
    "clip_hi0": (1, (-0.5, 0.0)),
}
MAPS = {**R.CHAINS, **EXACT}


@functools.lru_cache(maxsize=8)
def _inputs(n, dt, nin, nan):
    xs = [R.values(n, dt, k) for k in range(nin)]
    if nan:
        xs[0][n // 2] = np.nan
    for a in xs:
        a.setflags(write=False)
    return xs


def _call(name, ins, p, out):
    x = ins[0]
    if name == "scale":
        return _dev.axpby(p[0], x, out=out)  # y=None
    if name == "axpby":
        return _dev.axpby(p[0], x, p[1], ins[1], out=out)
    if name == "lincomb3":
        return _dev.lincomb3(p[0], x, p[1], ins[1], p[2], ins[2], out=out)
    if name == "extrapolate":
        return _dev.extrapolate(p[0], x, ins[1], out=out)
    if name == "prox_l1":
        return _dev.prox_l1(x, p[0], out=out)
    if name == "fenchel_prox_l1":
        return _dev.fenchel_prox_l1(x, p[0], p[1], out=out)
    if name == "moreau_grad_l1":
        return _dev.moreau_grad_l1(x, p[0], p[1], out=out)
    if name == "mul":
        return _dev.mul(x, ins[1], out=out)
    if name == "div":
        return _dev.div(x, p[0], out=out)
    if name == "add_scalar":
        return _dev.add_scalar(x, p[0], out=out)
    if name == "fill":
        return _dev.fill(out if out is not None else torch.empty_like(x), p[0])
    if name.startswith("clip"):
        return _dev.clip(x, p[0], p[1], out=out)
    raise KeyError(name)


def _verify(name, dt, got, xs, p, tag):
    assert got.dtype == dt and got.shape == xs[0].shape
    if name in R.CHAINS:
        ref, S = R.chain_ref(name, dt, xs, p)
        err = np.abs(got.astype(np.float64) - ref)
        bad = err > R.chain_bound(dt, S)
        assert not bad.any(), (tag, int(bad.sum()), int(np.argmax(bad)), float((err / (R.eps(dt) * S)).max()))
        if name == "scale":  # one rounding
            np.testing.assert_array_equal(got, dt(p[0]) * xs[0], err_msg=tag)
    else:
        np.testing.assert_array_equal(got, R.exact_ref(name.split("_")[0] if name.startswith("clip") else name,
                                                       dt, xs, p), err_msg=tag)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_map_entry_points(name, dt, n):
    """Every launch_map entry point: aligned, last input unaligned, output unaligned, and out aliasing each input."""
    nin, p = MAPS[name]
    xs = _inputs(n, dt, nin, name.startswith("clip"))
    for place in ("aligned", "in_unaligned", "out_unaligned"):
        ins = [R.placed(a, 1 if (place == "in_unaligned" and k == nin - 1) else 0)[1] for k, a in enumerate(xs)]
        off = 1 if place == "out_unaligned" else 0
        obase, out = R.placed(np.zeros(n, dtype=dt), off)
        res = _call(name, ins, p, out)
        assert res.data_ptr() == out.data_ptr()
        _verify(name, dt, R.to_host(out), xs, p, f"{name} {place} n={n}")
        assert R.guards_intact(obase, off, n), f"{name} {place} n={n}: wrote outside out"
        for k, a in enumerate(xs):  # inputs untouched
            np.testing.assert_array_equal(R.to_host(ins[k]), a)
    # out=None allocates
    ins = [R.to_dev(a) for a in xs]
    _verify(name, dt, R.to_host(_call(name, ins, p, None)), xs, p, f"{name} out=None n={n}")
    # out is x / y / z, on the vector path and on the scalar path
    if name == "fill":
        return
    for off in (0, 1):
        for k in range(nin):
            placed = [R.placed(a, off) for a in xs]
            ins = [v for _, v in placed]
            _call(name, ins, p, ins[k])
            _verify(name, dt, R.to_host(ins[k]), xs, p, f"{name} out is input {k} off={off} n={n}")
            assert R.guards_intact(placed[k][0], off, n)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("n,ny", [(21, 7), (4099 * 3, 4099), (5, 1)])
def test_axpby_bcast(n, ny, dt):
    x, y = R.values(n, dt, 1), R.values(ny, dt, 2)
    ref, S = R.bcast_ref(dt, 0.7, x, -1.3, y)
    for alias in (False, True):
        xd, yd = R.to_dev(x), R.to_dev(y)
        out = _dev.axpby_bcast(0.7, xd, -1.3, yd, out=xd if alias else None)
        got = R.to_host(out)
        assert (np.abs(got.astype(np.float64) - ref) <= R.chain_bound(dt, S)).all(), (n, ny, alias)
        np.testing.assert_array_equal(R.to_host(yd), y)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 1001])
@pytest.mark.parametrize("rows", [1, 3])
def test_axpy_rows(rows, n, dt):
    """out[r] = y[r] + s c[r] x[r], fresh out, out is x, out is y; one coefficient 0 leaves its row equal to y."""
    x = R.values(rows * n, dt, 1).reshape(rows, n)
    y = R.values(rows * n, dt, 2).reshape(rows, n)
    c = R.values(rows, dt, 3)
    c[rows // 2] = 0
    ref, S = R.axpy_rows_ref(dt, c, -0.7, x, y)
    for alias in (None, "x", "y"):
        xd, yd, cd = R.to_dev(x), R.to_dev(y), R.to_dev(c)
        out = _dev.axpy_rows(cd, -0.7, xd, yd, out={None: None, "x": xd, "y": yd}[alias])
        got = R.to_host(out)
        assert got.shape == (rows, n)
        assert (np.abs(got.astype(np.float64) - ref) <= R.chain_bound(dt, S)).all(), (rows, n, alias)
        np.testing.assert_array_equal(got[rows // 2], y[rows // 2])
        np.testing.assert_array_equal(R.to_host(cd), c)


# ----------------------------------------------------------------------------- L21 family
def _l21_call(mode, xd, p, outer, group, inner, out=None):
    if mode == "prox":
        return _dev.prox_l21(xd, p[0], outer, group, inner, out=out)
    if mode == "fenchel":
        return _dev.fenchel_prox_l21(xd, p[0], p[1], outer, group, inner, out=out)
    if mode == "moreau":
        return _dev.moreau_grad_l21(xd, p[0], p[1], outer, group, inner, out=out)
    return _dev.group_norm(xd, outer, group, inner)


def _l21_run(mode, dt, x, off, tag, inplace=True):
    """One L21 call on x (outer, group, inner) placed at element offset `off`, checked; then in place."""
    outer, group, inner = x.shape
    p = R.L21_PARAMS[mode]
    base, xd = R.placed(x, off)
    got = R.to_host(_l21_call(mode, xd, p, outer, group, inner))
    got = got.reshape(outer, inner) if mode == "norm" else got.reshape(x.shape)
    R.l21_check(mode, dt, x, got, p, tag)
    np.testing.assert_array_equal(R.to_host(xd).reshape(x.shape), x)
    if mode != "norm" and inplace:
        _l21_call(mode, xd, p, outer, group, inner, out=xd)
        np.testing.assert_array_equal(R.to_host(xd).reshape(x.shape), got, err_msg=f"{tag} in place")
        assert R.guards_intact(base, off, x.size)
    return got


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("group", [2, 3])
@pytest.mark.parametrize("mode", R.L21_MODES)
def test_l21_vector_kernel(mode, group, dt):
    """group_vec_kernel: one column block, a partial second block (`two` partly true), gx = 2; outer on grid.y."""
    V = R.vec_n(dt)
    for outer in (1, 3):
        for iv in (1, 256, 257, 511, 513):
            x = R.l21_values(outer, group, iv * V, dt)
            _l21_run(mode, dt, x, 0, f"vec {mode} G={group} outer={outer} iv={iv}")


@functools.lru_cache(maxsize=1)
def _l21_wrap_input():
    x = R.l21_values(1, 2, (2048 * 512 + 300) * 4, np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("mode", R.L21_MODES)
def test_l21_vector_kernel_grid_stride_wrap(mode):
    """inner / V = 2048 * 512 + 300: the grid is capped and every thread loops (fp32, group 2, outer 1)."""
    _l21_run(mode, np.float32, _l21_wrap_input(), 0, f"wrap {mode}", inplace=(mode == "prox"))


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", R.L21_MODES)
def test_l21_scalar_kernel(mode, dt):
    """group_kernel: group 4; group 2 with inner % V != 0; group 2 with an unaligned x."""
    V = R.vec_n(dt)
    _l21_run(mode, dt, R.l21_values(3, 4, 1028, dt), 0, f"scalar {mode} G=4")
    _l21_run(mode, dt, R.l21_values(3, 2, 257 * V + 1, dt), 0, f"scalar {mode} ragged inner")
    _l21_run(mode, dt, R.l21_values(3, 2, 257 * V, dt), 1, f"scalar {mode} unaligned")
    _l21_run(mode, dt, R.l21_values(1, 1, 1000, dt), 0, f"scalar {mode} G=1")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("off", [0, 1], ids=["vector", "scalar"])
def test_l21_planted_groups(off, dt):
    """An all-zero group gives zeros without NaN, n = tau / 2 an exact zero, and one 1e6 entry stays in bound."""
    V = R.vec_n(dt)
    x = R.l21_values(1, 2, 64 * V, dt)
    x[0, :, 0] = 0
    x[0, :, 1] = (0.5, 0.0)
    x[0, :, 2] = (1e6, 0.25)
    x[0, :, 5] = (0.25, -1e6)
    for mode in R.L21_MODES:
        got = _l21_run(mode, dt, x, off, f"planted {mode} off={off}")
        assert np.isfinite(got).all()
        if mode == "norm":
            assert got[0, 0] == 0 and got[0, 1] == 0.5
        else:
            assert (got[0, :, 0] == 0).all(), mode
        if mode == "prox":
            assert (got[0, :, 1] == 0).all()


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
@pytest.mark.parametrize("group", [2, 3])
def test_l21_vector_and_scalar_kernels_agree(group, dt):
    """The vector kernel on an aligned array and the scalar kernel on the same values in an unaligned view do the
    same arithmetic: bit-equal results."""
    V = R.vec_n(dt)
    x = R.l21_values(3, group, 513 * V, dt)
    for mode in R.L21_MODES:
        p = R.L21_PARAMS[mode]
        a = R.to_host(_l21_call(mode, R.placed(x, 0)[1], p, *x.shape))
        b = R.to_host(_l21_call(mode, R.placed(x, 1)[1], p, *x.shape))
        np.testing.assert_array_equal(a, b, err_msg=mode)
