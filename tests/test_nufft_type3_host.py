"""
CPU tests of the gridded type-3 NUFFT's host side (pyxu_amd/operator/linop/nufft.py) and of the restatement the GPU
tests lean on (tests/_nufft_type3_refs.py).

* Parameters: centres, outer grid nf1 and scale gamma for hand-checked inputs, the degenerate ones included (a zero
  half-width of the sources on an axis, a single target, one source and one target, a space-bandwidth product far
  below 1, centres at 1e4 and -300); no footprint of the rescaled sources leaves (-nf1/2, nf1/2); the rescaled
  targets stay within pi / sigma; the operator's plan, factors and correction against the restatement's.
* The achieved error of the float64 restatement against the exact sum (tests/_nudft_refs.py::nudft64), divided by
  eps, on every golden type-3 case, apply and adjoint: printed, and below RATIO_CAP_T3.
* The restated pair is adjoint to rounding.
* Dispatch: method="grid3" builds a gridded operator silently (this fails without the feature), "grid" stays
  NotImplementedError, "auto" follows GRID_CROSSOVER_T3, T3_PAIRS_PER_CELL and GRID_MAX_CELLS; the argument errors.
* The new entry points reject NULL operands and out-of-envelope arguments before any launch.
"""
import math
import warnings

import numpy as np
import pytest

import _nudft_refs as R
import _nufft_grid_refs as G
import _nufft_type3_refs as T

import pyxu_amd.operator as pxo
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.operator.linop import nufft as nufft_mod

GOLDEN3 = [c for c in R.golden_cases("f64") if c["typ"] == 3]


def _both(x, z, eps, sigma=2.0):
    """The operator's and the restatement's parameters of one input."""
    return nufft_mod._t3_params(x, z, eps, sigma), T.params(x, z, eps, sigma)


# ------------------------------------------------------------------ parameters
def test_parameters_by_hand():
    # X = 2, C = 1; S = 20, Dc = 10; eps = 1e-4: w = 5; 2 sigma X S / pi + 6 = 56.93 -> 56 = 2^3 7
    x, z = np.array([[-1.0], [0.3], [3.0]]), np.array([[-10.0], [30.0]])
    for p in _both(x, z, 1e-4):
        assert p["w"] == 5 and p["nf1"] == (56,) and p["nf2"] == (112,)
        assert p["C"][0] == 1.0 and p["Dc"][0] == 10.0 and p["X"][0] == 2.0 and p["S"][0] == 20.0
        assert p["gamma"][0] == pytest.approx(56 / 80, rel=1e-15)
    # upsampling factor 1.25: w = 7; 2.5 40 / pi + 8 = 39.83 -> 39 -> 40
    for p in _both(x, z, 1e-4, 1.25):
        assert p["w"] == 7 and p["nf1"] == (40,) and p["nf2"] == (50,)
        assert p["gamma"][0] == pytest.approx(40 / 50, rel=1e-15)


def test_parameters_degenerate():
    one = np.array([[5.0]])
    # X = 0: Xs = 1 / S, S stays; 4 / pi + 6 = 7.27 -> the 2 w floor
    for p in _both(np.array([[5.0], [5.0]]), np.array([[-20.0], [20.0]]), 1e-4):
        assert (p["Xs"][0], p["Ss"][0]) == (1 / 20, 20.0) and p["nf1"] == (10,) and p["gamma"][0] == 10 / 80
    # a single target: S = 0 -> Ss = 1 / X
    for p in _both(np.array([[-2.0], [2.0]]), one, 1e-4):
        assert (p["Xs"][0], p["Ss"][0]) == (2.0, 0.5) and p["nf1"] == (10,) and p["gamma"][0] == 5.0
        assert p["Dc"][0] == 5.0 and p["C"][0] == 0.0
    # one source, one target: both widths 1
    for p in _both(one, one, 1e-4):
        assert (p["Xs"][0], p["Ss"][0]) == (1.0, 1.0) and p["nf1"] == (10,) and p["gamma"][0] == 2.5
    # X S << 1: only S is enlarged, the grid stays at the 2 w floor (enlarging both would give X S = 1e5)
    rng = np.random.default_rng(0)
    x, z = 1e-3 * rng.uniform(-1, 1, (9, 2)), 1e-2 * rng.uniform(-1, 1, (7, 2))
    for p in _both(x, z, 1e-4):
        assert p["nf1"] == (10, 10) and p["nf2"] == (20, 20)
        assert np.array_equal(p["Xs"], p["X"]) and np.allclose(p["Xs"] * p["Ss"], 1.0, rtol=1e-15)
    # mixed: one axis degenerate, the other not
    x, z = np.array([[0.0, 7.0], [2.0, 7.0]]), np.array([[3.0, 1.0], [3.0, 2.0]])
    for p in _both(x, z, 1e-2):
        assert list(p["Xs"]) == [1.0, 2.0] and list(p["Ss"]) == [1.0, 0.5] and p["nf1"] == (6, 6)


@pytest.mark.parametrize("sigma", G.SIGMAS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_rescaled_points_stay_inside(D, sigma):
    rng = np.random.default_rng([D, 5])
    for scale_x, scale_z, cx, cz in ((1.0, 30.0, 0.0, 0.0), (2.5, 7.0, 1e4, -300.0), (1e-3, 1e-2, 0.0, 5.0),
                                     (40.0, 0.01, -3.0, 2.0)):
        x = cx + scale_x * rng.uniform(-1, 1, (67, D))
        z = cz + scale_z * rng.uniform(-1, 1, (29, D))
        for eps in (1e-2, 1e-6):
            p, q = _both(x, z, eps, sigma)
            assert p["nf1"] == q["nf1"] and p["nf2"] == q["nf2"] and np.array_equal(p["gamma"], q["gamma"])
            assert np.allclose(p["C"], cx, atol=scale_x) and np.allclose(p["Dc"], cz, atol=scale_z)
            xp, zp = nufft_mod._t3_rescale(x, z, p)
            xr, zr = T.rescale(x, z, q)
            assert np.allclose(xp, xr, rtol=0, atol=1e-14) and np.allclose(zp, zr, rtol=0, atol=1e-14)
            nf1, w = np.asarray(p["nf1"], dtype=np.float64), p["w"]
            xi = xp * nf1 / (2 * np.pi)
            # the footprint [ceil(xi - w/2), ceil(xi - w/2) + w - 1] stays inside (-nf1/2, nf1/2): nothing wraps
            lo = np.ceil(xi - w / 2)
            assert np.all(lo > -nf1 / 2) and np.all(lo + w - 1 < nf1 / 2)
            assert np.max(np.abs(zp)) <= np.pi / sigma * (1 + 1e-14)
            assert all(n % 2 == 0 and G._smooth(n) and n >= 2 * w for n in p["nf1"])


def test_operator_plan_matches_the_restatement():
    c = GOLDEN3[8]
    assert c["D"] == 3
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A = pxo.NUFFT.type3(c["x"], c["z"], eps=1e-6, method="grid3")
    bins = _dev.nufft_grid_tiles(1, 3)[0]
    ch = T.Chain3(c["x"], c["z"], 1e-6, bin_shape=bins)
    assert (A._nf1, A._nf2, A._w) == (ch.nf1, ch.nf2, ch.w) and A._beta == ch.beta
    for k in ("l0", "off", "perm", "bin_start"):
        assert np.array_equal(A._plan_x[k], ch.plan_x[k]) and np.array_equal(A._plan_z[k], ch.inner.plan[k]), k
    pre = R.as_complex(A._plan_x["fac"]).ravel()
    post = R.as_complex(A._plan_z["fac"]).ravel()
    assert pre.shape == (67,) and post.shape == (29,)
    assert np.max(np.abs(pre - ch.pre[ch.plan_x["perm"]])) <= 1e-14  # sorted order: entry s is point perm[s]
    assert np.max(np.abs(post - ch.post[ch.inner.plan["perm"]]) / np.abs(post)) <= 1e-13
    assert np.max(np.abs(A._corr - ch.inner.corr) / ch.inner.corr) <= 1e-13
    assert np.allclose(np.abs(pre), 1.0, rtol=0, atol=1e-15)
    # float32: rounded once from the float64 factors
    with pxrt.Precision(pxrt.Width.SINGLE):
        A32 = pxo.NUFFT.type3(c["x"].astype(np.float32), c["z"].astype(np.float32), eps=1e-3, method="grid3")
    assert A32._plan_x["fac"].dtype == np.float32 and A32._plan_z["off"].dtype == np.float32


def test_quadrature_at_real_frequencies():
    w, beta = G.kernel_params(1e-9)
    # at omega = k 2 pi / nf it is the correction of the uniform modes
    n, nf = 16, 32
    k = np.arange(-(n // 2), (n - 1) // 2 + 1)
    a = nufft_mod._t3_psi_hat(k * 2 * np.pi / nf, w, beta)
    assert np.max(np.abs(a - G.psi_hat(n, nf, w, beta))) <= 1e-14 * a.max()
    om = np.random.default_rng(1).uniform(-np.pi / 2, np.pi / 2, 3 * nufft_mod._T3_CHUNK // 2 + 1)  # more than one chunk
    a, b = nufft_mod._t3_psi_hat(om, w, beta), nufft_mod._t3_psi_hat(om, w, beta, nodes=256)
    assert np.all(a > 0) and np.max(np.abs(a - b)) <= 1e-14 * a.max()
    assert np.max(np.abs(a[:50] - T.psi_hat_at(om[:50], w, beta))) <= 1e-14 * a.max()


# ------------------------------------------------------------------ the algorithm's achieved error
@pytest.mark.parametrize("sigma", G.SIGMAS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_achieved_error(D, sigma):
    worst = 0.0
    cases = [c for c in GOLDEN3 if c["D"] == D]
    assert cases and all(c["x"].shape[0] == 67 and c["z"].shape[0] == 29 for c in cases)
    for c in cases:
        for which in ("apply", "adjoint"):
            exact, *_ = R.op_transform(R.nudft64, c, which)
            for eps in (G.EPS64 if sigma == 2.0 else T.EPS_125):
                ratio = R.rel_err(T.op_transform(c, which, eps, sigma), exact) / eps
                print(f"{c['id']} {which} sigma={sigma} eps={eps:g}: rel l2 error / eps = {ratio:.3f}")
                worst = max(worst, ratio)
                assert ratio <= T.RATIO_CAP_T3, (c["id"], which, eps)
    print(f"D={D} sigma={sigma}: worst ratio {worst:.3f} (RATIO_CAP_T3 {T.RATIO_CAP_T3})")


def test_achieved_error_offset_and_degenerate():
    rng = np.random.default_rng(6)
    w = rng.standard_normal((2, 41)) + 1j * rng.standard_normal((2, 41))
    x = 1e4 + 2.5 * rng.uniform(-1, 1, (41, 2))
    z = -300.0 + 7.0 * rng.uniform(-1, 1, (23, 2))
    flat = x.copy()
    flat[:, 1] = 3.0  # X = 0 on an axis
    for src, tgt in ((x, z), (flat, z), (x, z[:1]), (x[:1], z[:1]), (1e-3 * (x - 1e4), 1e-2 * z)):
        c = w[:, : src.shape[0]]
        for isign in (1, -1):
            got = T.Chain3(src, tgt, 1e-6).forward(c, isign)
            assert R.rel_err(got, R.nudft64(c, src, tgt, isign)) <= T.RATIO_CAP_T3 * 1e-6


def test_restatement_pair_is_adjoint_to_rounding():
    rng = np.random.default_rng(3)
    for c, sigma in ((GOLDEN3[0], 2.0), (GOLDEN3[4], 1.25), (GOLDEN3[8], 2.0)):
        M, N = c["x"].shape[0], c["z"].shape[0]
        ch = T.Chain3(c["x"], c["z"], 1e-4, sigma)
        a = rng.standard_normal((1, M)) + 1j * rng.standard_normal((1, M))
        y = rng.standard_normal((1, N)) + 1j * rng.standard_normal((1, N))
        for isign in (1, -1):
            Aa = ch.forward(a, isign)
            lhs, rhs = np.vdot(y, Aa), np.vdot(ch.adjoint(y, isign), a)
            assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(Aa) * np.linalg.norm(y)


def test_float32_restatement_is_close_to_float64():
    for c in GOLDEN3[::4]:
        for which in ("apply", "adjoint"):
            a = T.op_transform(c, which, 1e-3, dtype=np.float32)
            assert a.dtype == np.complex64
            assert R.rel_err(a, T.op_transform(c, which, 1e-3)) <= 1e-5


# ------------------------------------------------------------------ entry points, host side
def test_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes as ct

    import pyxu_amd

    lib = pyxu_amd.lib
    nf2 = (ct.c_int64 * 2)(10, 12)
    spread = lambda dt, D, Q, M, nf, w, beta, conj=0: lib.pxa_nufft_spread_fac(  # noqa: E731
        dt, D, Q, M, nf, w, beta, None, None, None, None, None, None, None, conj, None)
    interp = lambda dt, D, Q, M, nf, w, beta, conj=0: lib.pxa_nufft_interp_fac(  # noqa: E731
        dt, D, Q, M, nf, w, beta, None, None, None, None, None, None, conj, None)
    for fn in (spread, interp):
        assert fn(7, 2, 1, 1, nf2, 5, 11.5) == -2
        assert fn(0, 4, 1, 1, nf2, 5, 11.5) == -3
        assert fn(0, 2, 1, 1, nf2, 1, 11.5) == -1 and fn(0, 2, 1, 1, nf2, 17, 11.5) == -1  # w outside [2, 16]
        assert fn(0, 2, 1, 1, nf2, 6, 11.5) == -1  # nf < 2 w
        assert fn(0, 2, 1, 1, nf2, 5, 0.0) == -1  # beta
        assert fn(0, 2, -1, 1, nf2, 5, 11.5) == -1 and fn(0, 2, 1, -1, nf2, 5, 11.5) == -1
        assert fn(0, 2, 0, 1, nf2, 5, 11.5, 2) == -1 and fn(0, 2, 0, 1, nf2, 5, 11.5, -1) == -1  # conj_fac
        assert fn(0, 2, 1, 1, nf2, 5, 11.5) == -1 and fn(1, 2, 3, 1, nf2, 5, 11.5, 1) == -1  # NULL operands
        assert fn(0, 2, 0, 1, nf2, 5, 11.5) == 0  # Q = 0: nothing to do
    assert interp(1, 2, 3, 0, nf2, 5, 11.5) == 0  # M = 0: nothing to do
    assert spread(1, 2, 3, 0, nf2, 5, 11.5) == -1  # M = 0 still writes the grid: NULL grid


# ------------------------------------------------------------------ dispatch
def test_dispatch_grid3():
    rng = np.random.default_rng(4)
    x, z = rng.uniform(-np.pi, np.pi, size=(67, 2)), rng.uniform(-9, 9, size=(29, 2))
    with pxrt.Precision(pxrt.Width.DOUBLE):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # a gridded operator does not warn about eps
            for real in (False, True):
                A = pxo.NUFFT.type3(x, z, eps=1e-4, method="grid3", real=real)
                assert type(A) is nufft_mod._NUFFTGrid3 and isinstance(A, nufft_mod._NUDFT)
                assert A.shape == (58, 67 if real else 134)
                assert np.isclose(A.lipschitz, np.sqrt(67 * 29))
            B = pxo.NUFFT.type3(x, z, eps=1e-9, method="grid3", upsampfac=1.25, isign=-1)
        assert (A._w, A._sigma, A._nf1, A._nf2) == (5, 2.0) + tuple(T.params(x, z, 1e-4)[k] for k in ("nf1", "nf2"))
        assert (B._w, B._sigma, B._isign) == (G.kernel_params(1e-9, 1.25)[0], 1.25, -1)
        # the matrix is the exact transform's
        assert np.allclose(B.ascomplexarray(), np.exp(-1j * (z @ x.T)), rtol=0, atol=1e-13)
        with pytest.raises(NotImplementedError):
            A.mesh()
        with pytest.raises(ValueError, match="eps > 0"):
            pxo.NUFFT.type3(x, z, eps=0, method="grid3")
        for make in (pxo.NUFFT.type1, pxo.NUFFT.type2):
            with pytest.raises(ValueError, match="grid3"):
                make(x, (5, 6), eps=1e-4, method="grid3")
        with pytest.raises(NotImplementedError, match="grid3"):
            pxo.NUFFT.type3(x, z, eps=1e-4, method="grid")
        with pytest.raises(NotImplementedError):
            pxo.NUFFT.type3(x, z, eps=1e-4, method="grid3", chunked=True)
        with pytest.raises(ValueError):
            pxo.NUFFT.type3(x, z, eps=1e-4, method="grid3", upsampfac=1.5)
        # upsampling factor 1.25 cannot reach a tolerance whose width is clamped
        with pytest.raises(ValueError, match="1.25"):
            pxo.NUFFT.type3(x, z, eps=1e-12, method="grid3", upsampfac=1.25)
        assert nufft_mod._t3_width_ok(1e-9, 1.25) and not nufft_mod._t3_width_ok(1e-10, 1.25)
        assert nufft_mod._t3_width_ok(1e-30, 2.0)
        pxo.NUFFT.type1(x, (5, 6), eps=1e-12, method="grid", upsampfac=1.25)  # types 1 / 2 keep their clamp
        # method="direct" and eps = 0: the exact operator
        assert type(pxo.NUFFT.type3(x, z, eps=0)) is nufft_mod._NUDFT
        with pytest.warns(UserWarning, match="direct evaluation"):
            assert type(pxo.NUFFT.type3(x, z, eps=1e-4, method="direct")) is nufft_mod._NUDFT


def _factor_pair(n):
    """(a, b), a b = n, as balanced as n allows."""
    a = math.isqrt(n)
    while n % a:
        a -= 1
    return a, n // a


def test_dispatch_auto():
    rng = np.random.default_rng(5)
    cross, per_cell, cap = nufft_mod.GRID_CROSSOVER_T3, nufft_mod.T3_PAIRS_PER_CELL, nufft_mod.GRID_MAX_CELLS
    assert cross >= 1 << 20 and per_cell >= 1 and cap == 1 << 30
    side = math.isqrt(cross - 1) + 1  # side^2 >= cross
    x = rng.uniform(-np.pi, np.pi, size=(side, 1))
    unit = rng.uniform(-1, 1, size=(side + 2, 1))
    unit[0], unit[1] = -1.0, 1.0  # the half-width is the scale, whatever the number of targets
    with pxrt.Precision(pxrt.Width.DOUBLE):
        # a tiny transform warns and is exact
        with pytest.warns(UserWarning, match="direct evaluation"):
            assert type(pxo.NUFFT.type3(x[:67], unit[:29], eps=1e-4)) is nufft_mod._NUDFT
        # from the crossover on, on a grid that the pairs pay for: gridded, silently
        S = 64.0
        cells = nufft_mod._t3_params(x, S * unit[:side], 1e-4, 2.0)["cells"]
        assert per_cell * cells <= cross <= side * side
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            A = pxo.NUFFT.type3(x, S * unit[:side], eps=1e-4)
        assert type(A) is nufft_mod._NUFFTGrid3 and A.shape == (2 * side, 2 * side)
        assert type(pxo.NUFFT.type3(x, S * unit[:side], eps=0)) is nufft_mod._NUDFT
        # one pair short of the crossover (or as close below it as two balanced factors come)
        a, b = _factor_pair(cross - 1)
        if a < side // 4:
            a, b = side - 1, side - 1
        assert a * b < cross and a <= side and b <= side + 2
        with pytest.warns(UserWarning, match=r"O\(M N\)"):
            assert type(pxo.NUFFT.type3(x[:a], S * unit[:b], eps=1e-4)) is nufft_mod._NUDFT
        # a grid the pairs do not pay for: prod(nf2) ~ 4 S cells per axis
        S = float(1 << max(1, (2 * side * side // per_cell).bit_length()))
        prm = nufft_mod._t3_params(x, S * unit[:side], 1e-4, 2.0, cap)
        if prm["nf2"] is not None and prm["cells"] <= cap:
            assert per_cell * prm["cells"] > side * side
            with pytest.warns(UserWarning, match="direct evaluation"):
                assert type(pxo.NUFFT.type3(x, S * unit[:side], eps=1e-4)) is nufft_mod._NUDFT
        # a space-bandwidth product past GRID_MAX_CELLS: auto is direct, "grid3" is an error naming the grid
        S = float(cap)
        with pytest.warns(UserWarning, match="direct evaluation"):
            assert type(pxo.NUFFT.type3(x, S * unit[:side], eps=1e-4)) is nufft_mod._NUDFT
        with pytest.raises(ValueError, match="cells"):
            pxo.NUFFT.type3(x[:67], S * unit[:29], eps=1e-4, method="grid3")
        with pytest.raises(ValueError, match="GRID_MAX_CELLS"):
            pxo.NUFFT.type3(1e6 * x[:67], 1e300 * unit[:29], eps=1e-4, method="grid3")
        # upsampling factor 1.25 with a clamped width: auto takes the exact sum
        with pytest.warns(UserWarning, match="direct evaluation"):
            assert type(pxo.NUFFT.type3(x, 64.0 * unit[:side], eps=1e-12, upsampfac=1.25)) is nufft_mod._NUDFT
