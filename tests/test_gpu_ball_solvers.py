"""
Solvers on the new proximable functionals: the l1-constrained LASSO  PGD(0.5 ||A x - y||^2, L1Ball(N, r)),  the same
with g = 0.1 SquaredL1Norm(N), and PD3O / CondatVu with h = lam ||.||_inf on a Gradient.  Each run is compared with
the same iteration in float64 NumPy (oracle.pgd / pd3o / condat_vu) whose proxes are the sort rule of
tests/_threshold_refs.py, at the project's operator tolerance.
"""
import numpy as np
import pytest
from conftest import rel_err

import _prim_refs as R
import _threshold_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import oracle as orc  # noqa: E402
import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.util import to_NUMPY  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
M, N, ITERS = 48, 160, 60


def W(dt):
    return pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE


def _lasso(dt):
    rng = np.random.default_rng(7)
    A = (rng.standard_normal((M, N)) / np.sqrt(M)).astype(dt)
    xt = np.zeros(N)
    xt[rng.choice(N, 12, replace=False)] = rng.uniform(1.0, 3.0, 12) * rng.choice([-1.0, 1.0], 12)
    y = (A.astype(np.float64) @ xt + 0.05 * rng.standard_normal(M)).astype(dt)
    L = 1.01 * np.linalg.norm(A.astype(np.float64), 2) ** 2
    return A, y, xt, L


def _run_pgd(dt, make_g, prox64):
    A, y, xt, L = _lasso(dt)
    with pxrt.Precision(W(dt)):
        f = 0.5 * pxo.SquaredL2Norm(dim=M).asloss(R.to_dev(y)) * pxa.LinOp.from_array(R.to_dev(A))
        f.diff_lipschitz = L
        s = pxs.PGD(f=f, g=make_g(), show_progress=False)
        s.fit(x0=R.to_dev(np.zeros(N, dtype=dt)), stop_crit=pxst.MaxIter(ITERS))
        got = to_NUMPY(s.solution())
        tau = float(s._mstate["tau"])
    assert got.dtype == dt
    A64, y64 = A.astype(np.float64), y.astype(np.float64)
    ref, _ = orc.pgd(np.zeros(N), lambda v: A64.T @ (A64 @ v - y64), prox64, tau, ITERS)
    return got, ref, xt


@pytest.mark.parametrize("d", list(DT))
def test_pgd_l1_ball(d):
    dt = DT[d]
    r = 10.0  # about half of ||x_true||_1: the constraint is active
    got, ref, xt = _run_pgd(dt, lambda: pxo.L1Ball(dim=N, radius=r), lambda z, tau: T.project_l1(z, r))
    assert np.abs(xt).sum() > 1.5 * r and abs(np.abs(ref).sum() - r) < 1e-9 * r
    err = rel_err(got, ref)
    print("PGD L1Ball", d, "rel err", err, "||x||_1", float(np.abs(got.astype(np.float64)).sum()))
    assert err < R.OP_TOL[dt], err
    assert np.abs(got.astype(np.float64)).sum() <= r * (1 + 4 * R.eps(dt))


@pytest.mark.parametrize("d", list(DT))
def test_pgd_squared_l1(d):
    dt = DT[d]
    got, ref, _ = _run_pgd(dt, lambda: 0.1 * pxo.SquaredL1Norm(dim=N), lambda z, tau: T.prox_sql1(z, 0.1 * tau))
    assert 0 < (ref != 0).sum() < N  # a sparse, non-trivial solution
    err = rel_err(got, ref)
    print("PGD SquaredL1Norm", d, "rel err", err)
    assert err < R.OP_TOL[dt], err


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("algo", ["pd3o", "cv"])
def test_pds_linf_dual(algo, d):
    dt = DT[d]
    sh = (24, 24)
    n, lam, iters = sh[0] * sh[1], 30.0, 20
    rng = np.random.default_rng(11)
    y = rng.standard_normal(n).astype(dt)
    tau, sigma, rho = 0.25, 0.25, 1.0
    with pxrt.Precision(W(dt)):
        f = 0.5 * pxo.SquaredL2Norm(dim=n).asloss(R.to_dev(y))
        f.diff_lipschitz = 1.0
        K = pxo.Gradient(arg_shape=sh)
        h = lam * pxo.LInfinityNorm(dim=2 * n)
        klass = pxs.PD3O if algo == "pd3o" else pxs.CondatVu
        s = klass(f=f, g=None, h=h, K=K, show_progress=False)
        s.fit(x0=R.to_dev(np.zeros(n, dtype=dt)), tau=tau, sigma=sigma, rho=rho, stop_crit=pxst.MaxIter(iters))
        data, _ = s.stats()
        gx, gz = to_NUMPY(data["x"]), to_NUMPY(data["z"])
        tau, sigma, rho = (float(s._mstate[k]) for k in ("tau", "sigma", "rho"))
    y64 = y.astype(np.float64)
    grad = lambda v: v - y64
    Kf = lambda v: orc.gradient_apply(v, sh)
    KT = lambda z: orc.gradient_adjoint(z, sh)
    fprox = lambda z, sg: T.project_l1(z, lam)  # prox of (lam ||.||_inf)^*: the projection on the l1 ball of radius lam
    loop = orc.pd3o if algo == "pd3o" else orc.condat_vu
    out = loop(np.zeros(n), grad, None, Kf, KT, fprox, tau, sigma, rho, iters)
    rx, rz = out[0], out[1]
    assert abs(np.abs(rz).sum() - lam) < 1e-9 * lam  # the dual constraint is active
    ex, ez = rel_err(gx, rx), rel_err(gz, rz)
    print(algo, d, "rel err x", ex, "z", ez)
    assert ex < R.OP_TOL[dt] and ez < R.OP_TOL[dt], (ex, ez)
