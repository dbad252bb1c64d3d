"""
``NUFFT.type2(..).gram()`` / ``NUFFT.type1(..).cogram()`` on the device against the float64 matrix A^H diag(w) A
(tests/_nufft_gram_refs.py::gram_matrix64).  Coordinates in [-pi, pi] and N_d <= 40 keep the largest phase of the
kernel t (differences up to N - 1 per axis) inside the max Phi <= 256 regime in which the exact transform is checked
norm-wise (tests/_nudft_refs.py): 1e-5 (fp32) / 1e-12 (fp64).
"""
import numpy as np
import pytest

import _nudft_refs as R
import _nufft_gram_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.operator.linop.nufft import _NUFFTGram  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

TOL = R.NORMWISE_TOL
WIDTH = {np.float32: pxrt.Width.SINGLE, np.float64: pxrt.Width.DOUBLE}
M = 61

# (typ, N, isign, modeord, real, weighted, lead)
CASES = [
    (2, (33,), 1, 0, False, False, ()), (2, (40,), -1, 1, False, True, (3,)), (2, (1,), 1, 1, True, False, ()),
    (2, (12, 11), 1, 0, True, True, (2, 3)), (2, (11, 12), -1, 1, False, False, ()), (2, (6, 1), 1, 1, True, True, (2,)),
    (2, (5, 6, 4), -1, 0, False, True, ()), (2, (4, 5, 7), 1, 1, True, False, (2,)),
    (1, (33,), 1, 1, False, True, (2,)), (1, (12, 11), -1, 0, False, False, ()), (1, (5, 6, 4), 1, 1, False, True, (3,)),
]


def _cid(c):
    typ, N, s, o, real, wt, lead = c
    return f"t{typ}-N{'x'.join(map(str, N))}-s{s}-o{o}-r{int(real)}-w{int(wt)}-q{'x'.join(map(str, lead)) or '1'}"


def _setup(c, dtype):
    typ, N, s, o, real, wt, lead = c
    rng = np.random.default_rng([typ, o, *N])
    x = rng.uniform(-np.pi, np.pi, size=(M, len(N))).astype(dtype)
    w = rng.uniform(0.2, 2.0, size=M).astype(dtype) if wt else None
    cells = int(np.prod(N))
    u = rng.standard_normal((*lead, cells if real else 2 * cells)).astype(dtype)
    # the type 1 of sign s is the adjoint of the type 2 of sign -s
    Gm = T.gram_matrix64(x.astype(np.float64), N, s if typ == 2 else -s, o, w)
    return x, w, u, Gm


def _expected(u, Gm, real):
    u2 = u.reshape(-1, u.shape[-1]).astype(np.float64)
    uc = u2.astype(np.complex128) if real else R.as_complex(u2)
    out = uc @ Gm.T
    out = np.ascontiguousarray(out.real) if real else R.as_real(np.ascontiguousarray(out))
    return out.reshape(*u.shape[:-1], -1)


def _operator(c, x, w, **kw):
    typ, N, s, o, real, wt, lead = c
    make = pxo.NUFFT.type2 if typ == 2 else pxo.NUFFT.type1
    A = make(x, N, isign=s, eps=kw.pop("eps", 0), real=real, modeord=o, enable_warnings=False, **kw.pop("parent", {}))
    Gop = A.gram(weights=w, **kw) if typ == 2 else A.cogram(weights=w, **kw)
    assert isinstance(Gop, _NUFFTGram)
    return A, Gop


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_gram_matches_the_float64_matrix(case, dtype):
    x, w, u, Gm = _setup(case, dtype)
    want = _expected(u, Gm, case[4])
    with pxrt.Precision(WIDTH[dtype]):
        _, Gop = _operator(case, x, w)
        ud = to_device(u)
        got = {f: to_NUMPY(_operator(case, x, w, fused=f)[1].apply(ud)) for f in (True, False)}
        got[None] = to_NUMPY(Gop.apply(ud))
        again = to_NUMPY(Gop.apply(ud))
    assert got[None].shape == want.shape and np.array_equal(again, got[None])
    for f, g in got.items():
        err = R.rel_err(g, want)
        print(f"{_cid(case)} {np.dtype(dtype).name} fused={f}: rel err {err:.2e}")
        assert err <= TOL[np.dtype(dtype)]
    # the two forms share khat and differ by the rounding of their transforms: each is within TOL of the exact
    # convolution (the FFT tests' tolerance), so they are within 2 TOL of each other
    assert R.rel_err(got[True], got[False]) <= 2 * TOL[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[3], CASES[6], CASES[8]], ids=_cid)
def test_gram_is_self_adjoint_and_is_the_composition(case, dtype):
    x, w, u, _ = _setup(case, dtype)
    tol = TOL[np.dtype(dtype)]
    v = np.random.default_rng(3).standard_normal(u.shape).astype(dtype)
    with pxrt.Precision(WIDTH[dtype]):
        A, Gop = _operator(case, x, None)
        ud, vd = to_device(u), to_device(v)
        Gu, Gv = to_NUMPY(Gop.apply(ud)).astype(np.float64), to_NUMPY(Gop.apply(vd)).astype(np.float64)
        assert np.array_equal(to_NUMPY(Gop.adjoint(ud)).astype(np.float64), Gu)
        comp = to_NUMPY(A.adjoint(A.apply(ud)) if case[0] == 2 else A.apply(A.adjoint(ud)))
        L = float(Gop.lipschitz)
    # <G u, v> = <u, G v>: each product is within tol ||G|| ||u|| of the exact one, ||G|| <= lipschitz
    a, b = float(np.vdot(Gu, v.astype(np.float64))), float(np.vdot(u.astype(np.float64), Gv))
    scale = L * np.linalg.norm(u) * np.linalg.norm(v)
    print(f"{_cid(case)} {np.dtype(dtype).name}: |<Gu,v> - <u,Gv>| / (L |u| |v|) = {abs(a - b) / scale:.2e}")
    assert abs(a - b) <= 2 * tol * scale
    # against A^H (A u) by the exact transforms on the device: both are within tol of the exact gram
    err = R.rel_err(Gu, comp)
    print(f"{_cid(case)} {np.dtype(dtype).name}: gram vs adjoint(apply): {err:.2e}")
    assert err <= 2 * tol


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6]], ids=_cid)
def test_gram_of_a_gridded_parent(case):
    """The parent's eps = 1e-6 (method="grid") becomes the tolerance of t: within RATIO_CAP_GRAM eps of the exact
    gram (tests/test_nufft_gram_host.py::test_achieved_error_gridded_psf measures the ratio)."""
    eps = 1e-6
    x, w, u, Gm = _setup(case, np.float64)
    want = _expected(u, Gm, case[4])
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A, Gop = _operator(case, x, w, eps=eps, parent=dict(method="grid"))
        assert Gop._eps == eps
        got = to_NUMPY(Gop.apply(to_device(u)))
        plan_before = A._plan_dev
        to_NUMPY(Gop.apply(to_device(u)))
        assert A._plan_dev is plan_before is None  # the parent's point plan is never uploaded
    err = R.rel_err(got, want)
    print(f"{_cid(case)}: gridded t (eps {eps:g}): rel err {err:.2e} = {err / eps:.3f} eps (cap {T.RATIO_CAP_GRAM:.3f})")
    assert 0 < err <= T.RATIO_CAP_GRAM * eps
