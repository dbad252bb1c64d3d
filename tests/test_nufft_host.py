"""
CPU tests of the NUFFT operator's host side and of the references the GPU tests lean on (tests/_nudft_refs.py).

* The float64 restatement of the exponential sum reproduces the reference's goldens (tests/golden/nufft_*.npz,
  recorded from the reference's own eps = 0 path) to 1e-12 norm-wise; in single precision the goldens and the
  fp32 restatement of the reference's formula both lie within the element-wise bound of the float64 sum.
* Operator construction from host coordinates needs no GPU: shapes, mesh for both mode orders, lipschitz, the
  eps > 0 warning, argument errors.
* Every case the GPU tests check norm-wise stays inside the cap that figure assumes: max Phi <= 256 and an
  fp32-restatement error <= 1e-5 (the reference itself would pass).
"""
import ctypes as ct
import warnings

import numpy as np
import pytest

import _nudft_refs as R

import pyxu_amd
import pyxu_amd.operator as pxo
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev

WIDTHS = {"f32": (np.float32, pxrt.Width.SINGLE), "f64": (np.float64, pxrt.Width.DOUBLE)}


# ------------------------------------------------------------------ references against the goldens
@pytest.mark.parametrize("which", ["apply", "adjoint"])
def test_float64_restatement_matches_goldens(which):
    for c in R.golden_cases("f64"):
        out, *_ = R.op_transform(R.nudft64, c, which)
        got = R.op_output(c, which, out)
        assert got.shape == c[which].shape, c["id"]
        assert R.rel_err(got, c[which]) <= 1e-12, c["id"]


@pytest.mark.parametrize("which", ["apply", "adjoint"])
def test_single_precision_goldens_and_restatement_within_bound(which):
    for c in R.golden_cases("f32"):
        assert R.op_worst_ratio(c, which, c[which], np.float32) <= 1.0, c["id"]
        out, *_ = R.op_transform(R.nudft32_restated, c, which)
        assert out.dtype == np.complex64
        assert R.op_worst_ratio(c, which, R.op_output(c, which, out), np.float32) <= 1.0, c["id"]


def test_golden_coverage():
    for w in WIDTHS:
        cases = R.golden_cases(w)
        keys = {(c["typ"], c["D"], c["real"], c["isign"]) for c in cases}
        assert keys == {(t, d, r, s) for t in (1, 2, 3) for d in (1, 2, 3) for r in (False, True) for s in (1, -1)}
        assert {c["typ"] for c in cases if c["modeord"] == 1} == {1, 2}
        assert any(c["a_in"].shape[:-1] == (2, 3) for c in cases)


def test_bound_terms():
    # one source, one target, unit weight: B = u ((D + 3) Phi + 8 + 3)
    src, tgt, w = np.array([[2.0, -3.0]]), np.array([[0.5, 4.0]]), np.array([[1.0 + 0j]])
    assert np.allclose(R.phi(src, tgt), [[13.0]])
    assert np.allclose(R.bound(w, src, tgt, 0.25), 0.25 * (5 * 13.0 + 8 + 3))


# ------------------------------------------------------------------ the cap of the norm-wise GPU cases
def _tiles(code):
    v = [ct.c_int64(0) for _ in range(3)]
    assert pyxu_amd.lib.pxa_nudft_tiles(code, *[ct.byref(a) for a in v]) == 0
    return tuple(int(a.value) for a in v)


def test_tiles_and_host_argument_checks():
    lib = pyxu_amd.lib
    for code in (0, 1):
        tn, tm, qc = _tiles(code)
        assert tn >= 64 and tm >= 64 and qc >= 1
        assert _dev.nudft_tiles(code) == (tn, tm, qc)
    assert lib.pxa_nudft_tiles(7, None, None, None) != 0
    big = (1 << 64) - 1
    assert lib.pxa_nudft_workspace_bytes(7, 2, 1, 10, 10, 1) == big  # dtype
    assert lib.pxa_nudft_workspace_bytes(0, 4, 1, 10, 10, 1) == big  # D
    assert lib.pxa_nudft_workspace_bytes(0, 2, 1, 10, 10, -1) == big
    assert lib.pxa_nudft_workspace_bytes(0, 2, 1, 10, 10, 1) == 0
    assert lib.pxa_nudft_workspace_bytes(0, 2, 3, 10, 11, 5) == 5 * 3 * 11 * 8
    assert lib.pxa_nudft_workspace_bytes(1, 2, 3, 10, 11, 5) == 5 * 3 * 11 * 16
    # rejected on the host, before any launch
    assert lib.pxa_nudft(7, 2, 1, 1, 1, None, None, 1, None, None, 1, None, None) == -2
    assert lib.pxa_nudft(0, 4, 1, 1, 1, None, None, 1, None, None, 1, None, None) == -3
    assert lib.pxa_nudft(0, 2, 1, 1, 1, None, None, 0, None, None, 1, None, None) == -1  # isign
    assert lib.pxa_nudft(0, 2, 1, 1, 1, None, None, 1, None, None, 1, None, None) == -1  # NULL operands
    assert lib.pxa_nudft(0, 2, 1, 1, 0, None, None, 1, None, None, 1, None, None) == 0  # N = 0: nothing to do


def test_auto_splits_depend_on_shapes_only():
    tn, tm, qc = _tiles(0)
    assert _dev.nudft_splits(0, 2, 1, 8 * tm + 5, tn - 1) == 2  # few targets, many sources
    assert _dev.nudft_splits(0, 2, 5, 8 * tm + 5, tn - 1) == 2  # the stack does not enter
    assert _dev.nudft_splits(0, 2, 1, 2 * tm + 3, tn + 1) == 1  # too few sources to split
    assert _dev.nudft_splits(0, 2, 1, 1 << 20, 64 * 64) > 1  # type 1 onto a 64 x 64 grid
    assert _dev.nudft_splits(0, 2, 1, 1 << 20, 256 * tn) == 1  # the target tiles fill the chip


@pytest.mark.parametrize("code, dtype", [(0, np.float32), (1, np.float64)])
def test_kernel_cases_inside_the_normwise_cap(code, dtype):
    cases = R.kernel_cases(*_tiles(code))
    assert len({R.case_id(c) for c in cases}) == len(cases)
    for c in cases:
        src, tgt, w = R.kernel_inputs(c, dtype)
        assert R.phi(src, tgt).max() <= R.PHI_CAP, R.case_id(c)
        wc = R.as_complex(w)
        err = R.rel_err(R.nudft32_restated(wc, src, tgt, c["isign"]), R.nudft64(wc, src, tgt, c["isign"]))
        print(f"{R.case_id(c)}: fp32 restatement rel err {err:.2e}")
        assert err <= 1e-5, R.case_id(c)


def test_golden_cases_inside_the_normwise_cap():
    for c in R.golden_cases("f32"):
        assert R.phi(c["src"], c["tgt"]).max() <= R.PHI_CAP, c["id"]
        for which in ("apply", "adjoint"):
            a, *_ = R.op_transform(R.nudft32_restated, c, which)
            b, *_ = R.op_transform(R.nudft64, c, which)
            assert R.rel_err(a, b) <= 1e-5, (c["id"], which)


# ------------------------------------------------------------------ operator, host side
@pytest.mark.parametrize("w", ["f32", "f64"])
def test_operator_shapes_mesh_lipschitz(w):
    dt, width = WIDTHS[w]
    rng = np.random.default_rng(0)
    M = 67
    with pxrt.Precision(width):
        for D, N in ((1, (13,)), (2, (5, 6)), (3, (3, 4, 2))):
            x = rng.uniform(-np.pi, np.pi, size=(M, D))
            P = int(np.prod(N))
            for real in (False, True):
                A1 = pxo.NUFFT.type1(x, N, eps=0, real=real)
                assert A1.shape == (2 * P, M if real else 2 * M)
                A2 = pxo.NUFFT.type2(x, N, eps=0, real=real)
                assert A2.shape == (2 * M, P if real else 2 * P)
                z = rng.uniform(-8, 8, size=(29, D))
                A3 = pxo.NUFFT.type3(x, z, eps=0, real=real)
                assert A3.shape == (2 * 29, M if real else 2 * M)
                for A in (A1, A2):
                    assert isinstance(A, pxo.NUFFT)
                    assert np.isclose(A.lipschitz, np.sqrt(M * P))
                assert np.isclose(A3.lipschitz, np.sqrt(M * 29))
            for modeord in (0, 1):
                A = pxo.NUFFT.type1(x, N, eps=0, modeord=modeord)
                g = A.mesh()
                assert g.shape == (*N, D) and g.dtype == dt
                assert np.array_equal(g, R.mesh_unit(N, modeord))
                assert np.array_equal(pxo.NUFFT.type2(x, N, eps=0, modeord=modeord).mesh(), g)
        # an integer N is the same size on every axis; a 1-D x is (M, 1)
        assert pxo.NUFFT.type1(rng.uniform(-1, 1, size=(M, 2)), 4, eps=0).shape == (2 * 16, 2 * M)
        assert pxo.NUFFT.type1(rng.uniform(-1, 1, size=M), 5, eps=0).shape == (10, 2 * M)


def test_mesh_orders():
    x = np.zeros((3, 1))
    assert pxo.NUFFT.type1(x, 5, eps=0).mesh().ravel().tolist() == [-2, -1, 0, 1, 2]
    assert pxo.NUFFT.type1(x, 4, eps=0).mesh().ravel().tolist() == [-2, -1, 0, 1]
    assert pxo.NUFFT.type1(x, 5, eps=0, modeord=1).mesh().ravel().tolist() == [0, 1, 2, -2, -1]
    assert pxo.NUFFT.type1(x, 4, eps=0, modeord=1).mesh().ravel().tolist() == [0, 1, -2, -1]


def test_matrix_on_the_host():
    rng = np.random.default_rng(1)
    x = rng.uniform(-np.pi, np.pi, size=(7, 2))
    for real in (False, True):
        A = pxo.NUFFT.type2(x, (3, 4), isign=-1, eps=0, real=real, modeord=1)
        assert np.allclose(A.asarray(xp=np), R.type2_matrix64(x, (3, 4), -1, real, modeord=1), rtol=0, atol=1e-14)
        C = A.ascomplexarray()
        assert C.shape == (7, 12) and C.dtype == np.complex128
    z = rng.uniform(-4, 4, size=(5, 2))
    C = pxo.NUFFT.type3(x, z, isign=1, eps=0).ascomplexarray(dtype=np.complex64)
    assert C.dtype == np.complex64 and np.allclose(C, np.exp(1j * z @ x.T), atol=1e-6)


def test_eps_warning_and_unsupported_arguments():
    x = np.linspace(-1, 1, 9).reshape(-1, 1)
    with pytest.warns(UserWarning, match=r"O\(M N\)"):
        pxo.NUFFT.type1(x, 4, eps=1e-3)
    with pytest.warns(UserWarning, match="direct evaluation"):
        pxo.NUFFT.type3(x, x)  # the default eps is positive
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pxo.NUFFT.type2(x, 4, eps=1e-3, enable_warnings=False)
        pxo.NUFFT.type1(x, 4, eps=0, n_trans=5, upsampfac=1.25, plan_fw=False, nthreads=3)  # accepted, no effect
    with pytest.raises(NotImplementedError):
        pxo.NUFFT.type3(x, x, eps=0, chunked=True)
    with pytest.raises(ValueError):
        pxo.NUFFT.type1(np.zeros((4, 2, 2)), 4, eps=0)  # neither (M,) nor (M, D)
    with pytest.raises(AssertionError):
        pxo.NUFFT.type1(np.zeros((4, 4)), 4, eps=0)  # D > 3
    with pytest.raises(ValueError):
        pxo.NUFFT.type1(np.zeros((4, 3)), (4, 4), eps=0)  # x vs N
    with pytest.raises(AssertionError):
        pxo.NUFFT.type1(x, 0, eps=0)
    with pytest.raises(AssertionError):
        pxo.NUFFT.type3(np.zeros((4, 2)), np.zeros((4, 3)), eps=0)
    with pytest.raises(ValueError):
        pxo.NUFFT.type1(x, 4, eps=0, modeord=2)
