"""
CPU check of tests/_prim_refs.py: each kernel's stated operation order (csrc/elementwise.hip), emulated in NumPy
with dtype T on the generators the GPU tests use, stays inside the derived bounds, with either fma-contraction
choice.  This shows that the references and bounds test_gpu_prims_*.py rely on are sound without a GPU, and that
they are not vacuous: a dropped element or a one-ulp-of-|x| error per operation count is far outside them.
"""
import numpy as np
import pytest

import _prim_refs as R

DTS = [np.float32, np.float64]
N = 200_000


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", sorted(R.CHAINS))
def test_chain_emulation_inside_bound(name, dt, fused):
    nin, p = R.CHAINS[name]
    xs = [R.values(N, dt, k) for k in range(nin)]
    ref, S = R.chain_ref(name, dt, xs, p)
    got = R.chain_emulate(name, dt, xs, p, fused)
    assert got.dtype == dt
    ratio = np.abs(got.astype(np.float64) - ref) / (R.eps(dt) * S)
    print(name, np.dtype(dt).name, "fused" if fused else "plain", "max err / (eps S) =", float(ratio.max()))
    assert ratio.max() <= R.CHAIN_FACTOR
    assert (np.abs(got.astype(np.float64) - ref) <= R.chain_bound(dt, S)).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fused", [False, True])
def test_axpy_rows_and_bcast_emulation_inside_bound(dt, fused):
    rows, n = 3, 1001
    x, y = R.values(rows * n, dt, 1).reshape(rows, n), R.values(rows * n, dt, 2).reshape(rows, n)
    c = R.values(rows, dt, 3)
    c[1] = 0
    ref, S = R.axpy_rows_ref(dt, c, -0.7, x, y)
    got = R.axpy_rows_emulate(dt, c, -0.7, x, y, fused)
    assert (np.abs(got.astype(np.float64) - ref) <= R.chain_bound(dt, S)).all()
    np.testing.assert_array_equal(got[1], y[1])  # a zero coefficient leaves the row alone
    yb = R.values(7, dt, 4)
    xb = R.values(21, dt, 5)
    ref, S = R.bcast_ref(dt, 0.7, xb, -1.3, yb)
    got = R.chain_emulate("axpby", dt, [xb, np.tile(yb, 3)], (0.7, -1.3), fused)
    assert (np.abs(got.astype(np.float64) - ref) <= R.chain_bound(dt, S)).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("group", [2, 3, 4])
@pytest.mark.parametrize("mode", R.L21_MODES)
def test_l21_emulation_inside_bound(mode, group, dt):
    x = R.l21_values(3, group, N // 4, dt)
    p = R.L21_PARAMS[mode]
    got = R.l21_emulate(mode, dt, x, p)
    assert got.dtype == dt
    share = R.l21_check(mode, dt, x, got, p, tag="emulation")
    r = R.l21_ref(mode, dt, x, p)
    if mode != "norm":
        frac = float(r["clamp"].mean())
        assert 0.1 <= frac <= 0.9, frac  # both branches of the clamp are exercised
        assert share <= 0.01
    scale = np.abs(x.astype(np.float64)) if mode != "norm" else r["ref"]
    if mode == "moreau":
        scale = scale * abs(p[1] / p[0])
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / (R.eps(dt) * scale)
    print(mode, group, np.dtype(dt).name, "max err / (eps |v|) =", float(ratio.max()))


@pytest.mark.parametrize("dt", DTS)
def test_l21_planted_groups(dt):
    """All-zero group, n = tau / 2 and a group with one 1e6 entry, through the emulation."""
    x = R.l21_values(1, 2, 8, dt)
    x[0, :, 0] = 0
    x[0, :, 1] = (0.5, 0.0)
    x[0, :, 2] = (1e6, 0.25)
    for mode in R.L21_MODES:
        p = R.L21_PARAMS[mode]
        got = R.l21_emulate(mode, dt, x, p)
        assert np.isfinite(got).all()
        R.l21_check(mode, dt, x, got, p, tag="planted")
    out = R.l21_emulate("prox", dt, x, (1.0,))
    assert (out[0, :, 0] == 0).all() and (out[0, :, 1] == 0).all()


@pytest.mark.parametrize("dt", DTS)
def test_reduction_refs_and_bounds(dt):
    """A float32-free restatement: sums in another order (and with one element dropped) against the bound."""
    for (rows, n), _ in R.RED_SHAPES[:7]:
        x, y = R.sum_values_pair((rows, n), dt)
        for op in R.RED_SUMS:
            ref, bound, delta = R.red_ref(op, x, y if op in R.RED_NEEDS_Y else None)
            t = R.red_terms(op, x, y)
            other = t[:, ::-1].cumsum(axis=-1)[:, -1]  # sequential, reversed: a different summation order
            assert (np.abs(other - ref) <= bound).all(), (op, rows, n)
            assert (delta >= 10 * bound).all(), (op, rows, n)
            if n > 1:
                assert (np.abs(t[:, 1:].sum(axis=-1) - ref) > bound).all(), (op, rows, n)  # a dropped element is seen
        for p in (0.5, 1, 3):
            ref, bound, delta = R.pow_ref(p, x, y)
            assert (delta >= 10 * bound).all(), (p, rows, n)
            ref, bound, delta = R.pow_ref(p, x)
            assert (delta >= 10 * bound).all(), (p, rows, n)
        x[0, 0] = 0
        assert R.pow_ref(0, x)[0][0] == n - 1


def test_reduce_partition_of_the_shapes():
    """The shapes of the GPU reduction tests take the paths their comment names."""
    nb = {s: R.blocks_per_row(min(s[0], 65535), s[1]) for s, _ in R.RED_SHAPES}
    assert nb[(1, 257)] == 1 and nb[(5, 4096)] == 1 and nb[(1, 4097)] == 2 and nb[(3, 12293)] == 4
    assert nb[(1, 262145)] == 65 and nb[(1, 4 * 2**20 + 5)] == 1024 and nb[(2048, 8193)] == 2
    assert R.N_WRAP // R.vec_n(np.float32) > R.K_MAX_GRID * R.K_BLOCK and R.N_WRAP % 4 == 3


def test_exact_refs_are_dtype_T():
    for dt in DTS:
        x = R.values(100, dt)
        x[3] = np.nan
        for name, p in (("mul", ()), ("div", (0.7,)), ("add_scalar", (0.7,)), ("fill", (0.7,)), ("clip", (-0.5, None)),
                        ("clip", (-0.5, 0.0))):
            r = R.exact_ref(name, dt, [x, x], p)
            assert r.dtype == dt
            if name != "fill":
                assert np.isnan(r[3])
