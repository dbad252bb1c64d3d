"""
CPU tests of the gridding NUFFT's host side (pyxu_amd/operator/linop/nufft.py) and of the restatement the GPU
tests lean on (tests/_nufft_grid_refs.py).

* Kernel width / shape and fine-grid sizes against hand-computed values; the operator's parameters, correction
  vectors and plan against the restatement's.
* Plan invariants: the permutation is one, the bin offsets are monotone and end at M, the offsets lie in
  [w/2 - 1, w/2], and points at +-pi, 0 and 7 pi fold to the right cells.
* The achieved error of the float64 restatement against the exact sum (tests/_nudft_refs.py::nudft64), divided by
  eps, on every golden type-1 / type-2 case, both upsampling factors, eps from 1e-2 to 1e-12: printed, and below
  RATIO_CAP.  This is the algorithm's error, not the device's.
* Dispatch: method="auto" below the floor is the exact operator and warns; method="grid" builds a gridded operator
  without a warning; the argument errors.
"""
import warnings

import numpy as np
import pytest

import _nudft_refs as R
import _nufft_grid_refs as G

import pyxu_amd.operator as pxo
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.operator.linop import nufft as nufft_mod

GOLDEN12 = [c for c in R.golden_cases("f64") if c["typ"] in (1, 2)]


# ------------------------------------------------------------------ parameters
@pytest.mark.parametrize("eps, w, beta", [(1e-2, 3, 6.78), (1e-4, 5, 11.5), (1e-6, 7, 16.1), (1e-9, 10, 23.0),
                                          (1e-12, 13, 29.9)])
def test_kernel_parameters_sigma_2(eps, w, beta):
    for fn in (G.kernel_params, nufft_mod._grid_kernel):
        got_w, got_beta = fn(eps, 2.0)
        assert got_w == w and abs(got_beta - beta) < 1e-12


def test_kernel_parameters_other():
    for fn in (G.kernel_params, nufft_mod._grid_kernel):
        w, beta = fn(1e-4, 1.25)
        assert w == 7 and abs(beta - 0.97 * np.pi * 0.6 * 7) < 1e-12 and abs(beta - 12.80) < 5e-3
        # the small widths have their own shape constants; the width is clamped to [2, 16]
        assert fn(1e-1, 2.0) == (2, pytest.approx(4.40)) and fn(1e-3, 2.0) == (4, pytest.approx(9.52))
        assert fn(0.5, 2.0)[0] == 2 and fn(1e-15, 2.0)[0] == 16 and fn(1e-30, 2.0)[0] == 16
        assert fn(1e-15, 1.25)[0] == 16
        assert fn(1e-30, 2.0)[1] == pytest.approx(2.30 * 16)


def test_fine_grid_sizes():
    for fn in (G.fine_size, nufft_mod._grid_size):
        assert fn((13,), 2.0, 5) == (28,)  # 26 = 2 x 13 is not smooth
        assert fn((5, 6), 2.0, 10) == (20, 20)  # the 2 w floor
        assert fn((16, 20, 12), 2.0, 5) == (32, 40, 24)
        assert fn((13,), 1.25, 7) == (16,)
        assert fn((100,), 1.25, 7) == (126,)  # 125 is odd
        assert fn((1,), 2.0, 2) == (4,)
    assert nufft_mod._grid_sigma(None) == 2.0 and nufft_mod._grid_sigma(2) == 2.0
    assert nufft_mod._grid_sigma(1.25) == 1.25
    with pytest.raises(ValueError):
        nufft_mod._grid_sigma(1.5)


@pytest.mark.parametrize("eps, sigma", [(1e-1, 2.0), (1e-4, 2.0), (1e-12, 2.0), (1e-15, 2.0), (1e-4, 1.25),
                                        (1e-12, 1.25)])
def test_correction_quadrature_converged(eps, sigma):
    w, beta = G.kernel_params(eps, sigma)
    for n in (13, 16, 1):
        (nf,) = G.fine_size((n,), sigma, w)
        a, b = G.psi_hat(n, nf, w, beta, nodes=128), G.psi_hat(n, nf, w, beta, nodes=256)
        assert np.all(a > 0)
        # measured against psi_hat(0), the size of the terms the quadrature adds: the sums for the outer modes cancel
        # (psi_hat(k) / psi_hat(0) ~ 0.1), so their rounding is a larger share of the result than of the terms
        scale = b.max()
        assert np.max(np.abs(a - b)) <= 1e-14 * scale
        got = 1.0 / nufft_mod._grid_correction(n, nf, w, beta)
        assert np.max(np.abs(got - b)) <= 1e-14 * scale
        doubled = 1.0 / nufft_mod._grid_correction(n, nf, w, beta, nodes=2 * nufft_mod._GL_NODES)
        assert np.max(np.abs(got - doubled)) <= 1e-14 * scale


def test_psi_hat_is_the_transform_of_the_sampled_kernel():
    # sum_l phi(2 (l - xi) / w) exp(2 pi i k l / nf) = psi_hat(k) exp(2 pi i k xi / nf) up to aliasing (~eps)
    eps = 1e-9
    w, beta = G.kernel_params(eps)
    n, nf, xi = 16, 32, 11.3
    l = np.arange(np.ceil(xi - w / 2), np.ceil(xi - w / 2) + w)
    vals = G.phi(2 * (l - xi) / w, beta)
    k = np.arange(-(n // 2), (n - 1) // 2 + 1)
    lhs = (vals[None, :] * np.exp(2j * np.pi * k[:, None] * l[None, :] / nf)).sum(axis=1)
    rhs = G.psi_hat(n, nf, w, beta) * np.exp(2j * np.pi * k * xi / nf)
    assert np.max(np.abs(lhs - rhs) / np.abs(rhs)) <= 10 * eps


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("D, N", [(1, (13,)), (2, (40, 6)), (3, (16, 20, 12))])
@pytest.mark.parametrize("eps", [1e-2, 1e-9])
def test_plan_invariants(D, N, eps):
    rng = np.random.default_rng([D, len(N)])
    M = 301
    x = rng.uniform(-3 * np.pi, 3 * np.pi, size=(M, D))
    w, beta = G.kernel_params(eps)
    nf = G.fine_size(N, 2.0, w)
    shape, q_chunk, batch = _dev.nufft_grid_tiles(1, D)
    assert len(shape) == D and all(e >= 8 for e in shape) and q_chunk >= 1 and batch >= 64
    for dt in (np.float32, np.float64):
        p = nufft_mod._grid_plan(x, nf, w, shape, dt)
        ref = G.plan(x, nf, w, shape, dt)
        for k in ("l0", "off", "perm", "bin_start"):
            assert np.array_equal(p[k], ref[k]), k
        assert p["l0"].dtype == np.int32 and p["off"].dtype == dt and p["l0"].shape == p["off"].shape == (M, D)
        assert np.array_equal(np.sort(p["perm"]), np.arange(M))
        assert p["bin_start"][0] == 0 and p["bin_start"][-1] == M and np.all(np.diff(p["bin_start"]) >= 0)
        assert p["bin_start"].shape == (int(np.prod(ref["nb"])) + 1,)
        assert np.all(p["off"] >= w / 2 - 1) and np.all(p["off"] <= w / 2)
        xi = G.fold(x, nf)[p["perm"]]
        assert np.all((xi >= 0) & (xi < np.asarray(nf)))
        tol = 1e-12 if dt == np.float64 else w * 2.0**-24
        assert np.max(np.abs(p["l0"] + p["off"].astype(np.float64) - xi)) <= tol
        # sorted by bin, the given order inside a bin
        cell = np.floor(xi).astype(np.int64)
        bins = np.zeros(M, dtype=np.int64)
        for d in range(D):
            bins = bins * ref["nb"][d] + cell[:, d] // shape[d]
        assert np.all(np.diff(bins) >= 0)
        for b in np.unique(bins):
            lo, hi = p["bin_start"][b], p["bin_start"][b + 1]
            assert np.all(bins[lo:hi] == b) and np.all(np.diff(p["perm"][lo:hi]) > 0)


def test_plan_folds_special_points():
    w, nf = 5, (28,)
    x = np.array([[np.pi], [-np.pi], [0.0], [7 * np.pi], [-1e-20], [2 * np.pi]])
    p = nufft_mod._grid_plan(x, nf, w, (256,), np.float64)
    assert np.array_equal(p["perm"], np.arange(6))  # one bin: the given order
    xi = p["l0"][:, 0] + p["off"][:, 0]
    assert np.allclose(xi[[0, 1, 3]], 14.0, rtol=0, atol=1e-12)  # +-pi and 7 pi are the middle of the grid
    assert np.all(p["l0"][[0, 1, 3], 0] == 12)  # ceil(14 - 2.5)
    assert xi[2] == 0.0 and p["l0"][2, 0] == -2 and p["off"][2, 0] == 2.0
    assert np.all((xi[4:] >= 0) & (xi[4:] < 28)) and np.all(np.abs(xi[4:] % 28) < 1e-9)
    # an even width at a cell boundary: the footprint is [xi - w/2, xi + w/2 - 1]
    p = nufft_mod._grid_plan(np.array([[0.0]]), (16,), 4, (256,), np.float64)
    assert p["l0"][0, 0] == -2 and p["off"][0, 0] == 2.0


# ------------------------------------------------------------------ the algorithm's achieved error
@pytest.mark.parametrize("sigma", G.SIGMAS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_achieved_error(D, sigma):
    worst = 0.0
    for c in GOLDEN12:
        if c["D"] != D:
            continue
        for which in ("apply", "adjoint"):
            exact, *_ = R.op_transform(R.nudft64, c, which)
            for eps in G.EPS64:
                ratio = R.rel_err(G.op_transform(c, which, eps, sigma), exact) / eps
                print(f"{c['id']} {which} sigma={sigma} eps={eps:g}: rel l2 error / eps = {ratio:.3f}")
                worst = max(worst, ratio)
                assert ratio <= G.RATIO_CAP, (c["id"], which, eps)
    print(f"D={D} sigma={sigma}: worst ratio {worst:.3f} (RATIO_CAP {G.RATIO_CAP})")


def test_restatement_pair_is_adjoint_to_rounding():
    rng = np.random.default_rng(3)
    x = rng.uniform(-3 * np.pi, 3 * np.pi, size=(40, 2))
    ch = G.Chain(x, (5, 6), 1e-2, modeord=1)
    c = rng.standard_normal((1, 40)) + 1j * rng.standard_normal((1, 40))
    u = rng.standard_normal((1, 30)) + 1j * rng.standard_normal((1, 30))
    lhs, rhs = np.vdot(u, ch.type1(c, 1)), np.vdot(ch.type2(u, -1), c)
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


def test_float32_restatement_is_close_to_float64():
    for c in GOLDEN12[::5]:
        for which in ("apply", "adjoint"):
            a = G.op_transform(c, which, 1e-4, dtype=np.float32)
            assert a.dtype == np.complex64
            assert R.rel_err(a, G.op_transform(c, which, 1e-4)) <= 1e-5


# ------------------------------------------------------------------ entry points, host side
def test_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes as ct

    import pyxu_amd

    lib = pyxu_amd.lib
    nf2, n2 = (ct.c_int64 * 2)(10, 12), (ct.c_int64 * 2)(5, 6)
    for code in (0, 1):
        for D, shape in ((1, (256,)), (2, (16, 16)), (3, (8, 8, 8))):
            got, q_chunk, batch = _dev.nufft_grid_tiles(code, D)
            assert got == shape and q_chunk == 4 and batch == 256
    assert lib.pxa_nufft_grid_tiles(7, 2, nf2, nf2, nf2) == -2  # dtype
    assert lib.pxa_nufft_grid_tiles(0, 4, nf2, nf2, nf2) == -3  # D
    assert lib.pxa_nufft_grid_tiles(0, 2, None, None, None) == -1
    spread = lambda dt, D, Q, M, nf, w, beta: lib.pxa_nufft_spread(  # noqa: E731
        dt, D, Q, M, nf, w, beta, None, None, None, None, None, None, None)
    interp = lambda dt, D, Q, M, nf, w, beta: lib.pxa_nufft_interp(  # noqa: E731
        dt, D, Q, M, nf, w, beta, None, None, None, None, None, None)
    for fn in (spread, interp):
        assert fn(7, 2, 1, 1, nf2, 5, 11.5) == -2
        assert fn(0, 4, 1, 1, nf2, 5, 11.5) == -3
        assert fn(0, 2, 1, 1, nf2, 1, 11.5) == -1 and fn(0, 2, 1, 1, nf2, 17, 11.5) == -1  # w outside [2, 16]
        assert fn(0, 2, 1, 1, nf2, 6, 11.5) == -1  # nf < 2 w
        assert fn(0, 2, 1, 1, nf2, 5, 0.0) == -1  # beta
        assert fn(0, 2, -1, 1, nf2, 5, 11.5) == -1 and fn(0, 2, 1, -1, nf2, 5, 11.5) == -1
        assert fn(0, 2, 1, 1, nf2, 5, 11.5) == -1  # NULL operands
        assert fn(0, 2, 0, 1, nf2, 5, 11.5) == 0  # Q = 0: nothing to do
    assert interp(1, 2, 3, 0, nf2, 5, 11.5) == 0  # M = 0: nothing to do
    deconv = lambda dt, D, Q, n, nf, o: lib.pxa_nufft_deconv(dt, D, Q, n, nf, o, 1, None, None, None, None)  # noqa: E731
    assert deconv(7, 2, 1, n2, nf2, 0) == -2 and deconv(0, 0, 1, n2, nf2, 0) == -3
    assert deconv(0, 2, 1, n2, nf2, 2) == -1  # modeord
    assert deconv(0, 2, 1, nf2, n2, 0) == -1  # more modes than cells
    assert deconv(0, 2, 1, n2, nf2, 0) == -1  # NULL operands
    assert deconv(0, 2, 0, n2, nf2, 1) == 0


# ------------------------------------------------------------------ dispatch
def test_dispatch():
    rng = np.random.default_rng(4)
    x = rng.uniform(-np.pi, np.pi, size=(67, 2))
    floor = nufft_mod.GRID_CROSSOVER
    assert floor >= 1 << 20
    with pxrt.Precision(pxrt.Width.DOUBLE):
        # below the floor "auto" is the exact operator, and warns
        with pytest.warns(UserWarning, match=r"O\(M N\)"):
            A = pxo.NUFFT.type1(x, (5, 6), eps=1e-4)
        assert type(A) is nufft_mod._NUDFT
        with pytest.warns(UserWarning, match="direct evaluation"):
            A = pxo.NUFFT.type2(x, (5, 6), eps=1e-4, method="direct")
        assert type(A) is nufft_mod._NUDFT
        # method="grid": a gridded operator, no warning
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for real in (False, True):
                A1 = pxo.NUFFT.type1(x, (5, 6), eps=1e-4, method="grid", real=real)
                A2 = pxo.NUFFT.type2(x, (5, 6), eps=1e-9, method="grid", real=real, upsampfac=1.25, modeord=1)
                assert isinstance(A1, nufft_mod._NUFFTGrid) and isinstance(A2, nufft_mod._NUFFTGrid)
                assert A1.shape == (60, 67 if real else 134) and A2.shape == (134, 30 if real else 60)
                assert np.isclose(A1.lipschitz, np.sqrt(67 * 30))
                assert np.array_equal(A2.mesh(), R.mesh_unit((5, 6), 1))
            assert (A1._w, A1._nf, A1._sigma) == (5, (10, 12), 2.0)
            assert (A2._w, A2._sigma) == G.kernel_params(1e-9, 1.25)[:1] + (1.25,)
            assert A2._nf == G.fine_size((5, 6), 1.25, A2._w)
            # the matrix is the exact transform's
            assert np.allclose(A2.asarray(xp=np), R.type2_matrix64(x, (5, 6), 1, True, modeord=1), rtol=0, atol=1e-14)
            # "auto" from the floor on grids, silently
            side = 1 << (floor.bit_length() // 2)  # M = N = sqrt(floor), or the next power of two
            big = rng.uniform(-np.pi, np.pi, size=(-(-floor // side), 1))
            assert isinstance(pxo.NUFFT.type1(big, side, eps=1e-4), nufft_mod._NUFFTGrid)
            assert type(pxo.NUFFT.type1(big, side, eps=0)) is nufft_mod._NUDFT
        with pytest.warns(UserWarning, match="direct evaluation"):
            # one point short of the floor
            assert type(pxo.NUFFT.type1(big[: (floor - 1) // side], side, eps=1e-4)) is nufft_mod._NUDFT
        with pytest.raises(ValueError):
            pxo.NUFFT.type1(x, (5, 6), eps=0, method="grid")
        with pytest.raises(ValueError):
            pxo.NUFFT.type2(x, (5, 6), eps=1e-4, method="gridding")
        with pytest.raises(ValueError):
            pxo.NUFFT.type2(x, (5, 6), eps=1e-4, method="grid", upsampfac=1.5)
        with pytest.raises(NotImplementedError):
            pxo.NUFFT.type3(x, x, eps=1e-4, method="grid")
        with pytest.raises(ValueError):
            pxo.NUFFT.type3(x, x, eps=0, method="nope")
        with pytest.warns(UserWarning, match="direct evaluation"):
            pxo.NUFFT.type3(x, x, eps=1e-4, method="auto")
