"""
Host checks of the Toeplitz gram of a type-2 NUFFT (no GPU): the float64 restatement in tests/_nufft_gram_refs.py
against the exact matrix A^H diag(w) A, the plan sizes and argument handling of ``NUFFT.gram`` / ``cogram``, and the
error the algorithm makes when its kernel t comes from the gridding transform instead of the exact sum.
"""
import ctypes as ct

import numpy as np
import pytest

import _nudft_refs as R
import _nufft_grid_refs as G
import _nufft_gram_refs as T
import pyxu_amd.abc as pxa
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd._lib import i64_array, lib
from pyxu_amd.operator.linop import nufft as nf
from pyxu_amd.operator.linop.nufft import NUFFT, _NUFFTGram

GOLDEN2 = [c for c in R.golden_cases("f64") if c["typ"] == 2]

# (N, modeord, isign, weighted): odd / even / unit lengths in every dimension, both orders and signs
EXACT_CASES = [
    ((7,), 0, 1, False), ((8,), 1, -1, True), ((1,), 0, 1, True), ((1,), 1, -1, False), ((2,), 1, 1, False),
    ((5, 6), 0, -1, True), ((6, 5), 1, 1, False), ((1, 4), 1, 1, True), ((3, 1), 0, -1, False),
    ((3, 4, 2), 0, 1, True), ((4, 3, 5), 1, -1, False), ((2, 1, 3), 1, 1, True),
]


def _points(N, M=23):
    rng = np.random.default_rng([len(N), *N])
    return rng.uniform(-np.pi, np.pi, size=(M, len(N))), rng.uniform(0.2, 2.0, size=M)


def test_plan_sizes_and_splits():
    assert [T.smooth_even(2 * n - 1) for n in (1, 2, 3, 13, 64, 105, 2048)] == [2, 4, 6, 28, 128, 210, 4096]
    for N in [(1,), (2,), (13,), (5, 6), (3, 4, 2), (105, 12, 13)]:
        for modeord in (0, 1):
            P, split = nf._toeplitz_sizes(N, modeord)
            assert (P, split) == T.sizes(N, modeord)
            assert all(p >= 2 * n - 1 and p % 2 == 0 for p, n in zip(P, N))
            assert split == (tuple(N) if modeord == 0 else tuple((n - 1) // 2 + 1 for n in N))
    # the operator's FFT-order split is where the reference's mode grid turns negative
    for n in (1, 2, 5, 6):
        k = R.mesh_unit((n,), 1).ravel()
        assert int((k >= 0).sum()) == (n - 1) // 2 + 1


@pytest.mark.parametrize("N,modeord,isign,weighted", EXACT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_restatement_is_the_exact_gram(N, modeord, isign, weighted):
    x, w = _points(N)
    w = w if weighted else None
    Gm = T.gram_matrix64(x, N, isign, modeord, w)
    rng = np.random.default_rng(5)
    u = rng.standard_normal((3, Gm.shape[0])) + 1j * rng.standard_normal((3, Gm.shape[0]))
    got = T.gram_apply64(x, N, isign, modeord, u, w)
    err = R.rel_err(got, u @ Gm.T)
    print(f"N={N} modeord={modeord} isign={isign} weighted={weighted}: rel err {err:.2e}")
    assert err <= 1e-12
    # a longer P than the least one serves too
    P, split = T.sizes(N, modeord)
    P2 = tuple(T.smooth_even(p + 3) for p in P)
    kh, _ = T.khat64(T.psf64(x, N, isign, w), N, P2)
    got2 = T.toeplitz_apply64(u.reshape(-1, *N), N, P2, split, kh).reshape(3, -1)
    assert R.rel_err(got2, u @ Gm.T) <= 1e-12


@pytest.mark.parametrize("N,modeord,isign,weighted", EXACT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_spectrum_is_real_to_rounding(N, modeord, isign, weighted):
    x, w = _points(N)
    P, _ = T.sizes(N, modeord)
    kh, imag = T.khat64(T.psf64(x, N, isign, w if weighted else None), N, P)
    assert imag <= 64 * np.finfo(np.float64).eps * np.abs(kh).max()


def test_gram_and_cogram_return_the_toeplitz_operator_without_a_gpu():
    x, w = _points((5, 6), M=31)
    with pxrt.Precision(pxrt.Width.DOUBLE):
        for kw in (dict(eps=0), dict(eps=1e-6, method="grid")):
            A = NUFFT.type2(x, (5, 6), isign=-1, enable_warnings=False, **kw)
            Gop = A.gram()
            assert isinstance(Gop, _NUFFTGram) and isinstance(Gop, pxa.SelfAdjointOp)
            assert Gop.shape == (A.dim, A.dim) == (60, 60)
            assert Gop._isign == -1 and Gop._eps == kw["eps"] and Gop._fused
            assert float(Gop.lipschitz) == pytest.approx(float(A.lipschitz) ** 2, rel=1e-12)
            Gw = A.gram(weights=w)
            assert float(Gw.lipschitz) == pytest.approx(np.abs(w).sum() * 30, rel=1e-12)
            assert A.gram(fused=False)._fused is False and A.gram(eps=1e-3)._eps == 1e-3
        Ar = NUFFT.type2(x, (5, 6), eps=0, real=True)
        assert isinstance(Ar.gram(), _NUFFTGram) and Ar.gram().shape == (30, 30) and Ar.gram()._real
        B = NUFFT.type1(x, (5, 6), isign=1, eps=0, modeord=1)
        C = B.cogram(weights=w)
        assert isinstance(C, _NUFFTGram) and C.shape == (B.codim, B.codim) == (60, 60)
        assert C._isign == -1 and C._split == (3, 3) and C._P == (10, 12)


def test_gram_argument_errors():
    x, w = _points((5, 6), M=31)
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A = NUFFT.type2(x, (5, 6), eps=0)
        with pytest.raises(ValueError):
            A.gram(weights=w.astype(np.complex128))
        with pytest.raises(ValueError):
            A.gram(weights=w[:-1])
        with pytest.raises(ValueError):
            A.gram(weights=w.reshape(1, -1))
        with pytest.raises(ValueError):
            A.gram(eps=-1.0)
        with pytest.raises(ValueError):  # weights belong to the Toeplitz form only
            A.cogram(weights=w)
        long = NUFFT.type2(x[:, :1], (2600,), eps=0)  # P = 5250 > 5120 cells of fp64
        assert long.gram()._fused is False
        with pytest.raises(ValueError):
            long.gram(fused=True)
    with pxrt.Precision(pxrt.Width.SINGLE):
        x32 = x.astype(np.float32)
        assert NUFFT.type2(x32[:, :1], (2600,), eps=0).gram()._fused is True
        # fused=None in two and three dimensions: the fused kernel while a workgroup holds 4 lines (P <= 1024 in fp32)
        assert NUFFT.type2(x32, (512, 300), eps=0).gram()._fused is True  # P = (1024, 600)
        wide = NUFFT.type2(x32, (300, 520), eps=0)  # P = (600, 1050)
        assert wide.gram()._fused is False and wide.gram(fused=True)._fused is True
    with pxrt.Precision(pxrt.Width.DOUBLE):
        assert NUFFT.type2(x, (256, 256), eps=0).gram()._fused is True  # P = 512
        assert NUFFT.type2(x, (256, 300), eps=0).gram()._fused is False  # P = (512, 600)


def test_other_normal_operators_stay_generic():
    x, _ = _points((5, 6), M=31)
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A2, A1 = NUFFT.type2(x, (5, 6), eps=0), NUFFT.type1(x, (5, 6), eps=0)
        A1r = NUFFT.type1(x, (5, 6), eps=0, real=True)
        A3 = NUFFT.type3(x, x[:9] * 3.0, eps=0)
        A3g = NUFFT.type3(x, x[:9] * 3.0, eps=1e-4, method="grid3")
        for op, shape in [(A2.cogram(), 62), (A1.gram(), 62), (A1r.cogram(), 60), (A3.gram(), 62), (A3.cogram(), 18),
                          (A3g.gram(), 62), (A3g.cogram(), 18)]:
            assert not isinstance(op, _NUFFTGram)
            assert isinstance(op, pxa.SelfAdjointOp) and op.shape == (shape, shape)


def test_resident_lengths_match_the_library():
    for dt, code in ((np.float32, 0), (np.float64, 1)):
        top = nf._TOEPLITZ_RESIDENT[np.dtype(dt)]
        assert _dev.toeplitz_workspace_bytes(code, 1, (top // 2,), (top,)) == 0
        assert _dev.toeplitz_workspace_bytes(code, 1, (top // 2,), (T.smooth_even(top + 2),)) is None
    # D = 2 and 3: (Q, p0, n1[, n2]) plus (Q, p0, p1, n2) complex elements
    assert _dev.toeplitz_workspace_bytes(0, 3, (5, 6), (10, 12)) == 3 * 10 * 6 * 8
    assert _dev.toeplitz_workspace_bytes(1, 2, (3, 4, 2), (6, 8, 4)) == 2 * (6 * 4 * 2 + 6 * 8 * 2) * 16


def test_entry_point_rejects_bad_lengths_before_any_launch():
    """Every refusal is decided from the arguments: null data pointers are never dereferenced."""
    def call(code, n, p, split, Q=1):
        return lib.pxa_toeplitz_apply(code, len(n), Q, i64_array(n), i64_array(p), i64_array(split), None, None, None,
                                      None, None)

    assert call(0, (5,), (11,), (5,)) == -3  # 11 is prime
    assert call(0, (5,), (8,), (5,)) == -3  # below 2 n - 1
    assert call(1, (2600,), (5250,), (2600,)) == -3  # smooth, not resident in fp64
    assert call(0, (5, 6), (10, 13), (5, 6)) == -3
    assert call(0, (5,), (10,), (0,)) == -3 and call(0, (5,), (10,), (6,)) == -3  # split outside [1, n]
    assert call(0, (5,), (10,), (5,), Q=0) == 0  # nothing to do
    assert call(0, (5,), (10,), (5,)) == -1  # valid lengths, null arrays: an argument error, still no launch
    assert call(7, (5,), (10,), (5,)) == -2
    four = (ct.c_int64 * 4)(5, 5, 5, 5)
    assert lib.pxa_toeplitz_workspace_bytes(0, 4, 1, four, four) == (1 << 64) - 1


@pytest.mark.parametrize("D", [1, 2, 3])
def test_achieved_error_gridded_psf(D):
    """||G_eps u - G u|| / (||G u|| eps) with t from the float64 gridding chain (upsampling factor 2)."""
    worst = {}
    for c in GOLDEN2:
        if c["D"] != D:
            continue
        N, x = c["N"], np.asarray(c["x"], dtype=np.float64)
        u = R.op_weights(c, "apply")
        ref = u.astype(np.complex128) @ T.gram_matrix64(x, N, c["isign"], c["modeord"]).T
        for eps in T.EPS_GRAM:
            n2 = tuple(2 * n - 1 for n in N)
            t = G.Chain(x, n2, eps, 2.0, 0).type1(np.ones((1, x.shape[0])), -c["isign"]).reshape(n2)
            got = T.gram_apply64(x, N, c["isign"], c["modeord"], u, psf=t)
            ratio = R.rel_err(got, ref) / eps
            worst[eps] = max(worst.get(eps, 0.0), ratio)
            assert ratio <= T.RATIO_CAP_GRAM, (c["id"], eps, ratio)
    print(f"D={D}: worst ratio per eps " + "  ".join(f"{e:g}: {r:.3f}" for e, r in worst.items())
          + f"  (RATIO_CAP_GRAM {T.RATIO_CAP_GRAM:.3f})")
