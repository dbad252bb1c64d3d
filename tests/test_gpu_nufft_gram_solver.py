"""
The sparse-recovery problem of tests/test_gpu_nufft_grid_solver.py (A = NUFFT.type2(x, N=(12, 11), real=True),
M = 150 samples, f = 1/2 ||A u - y||^2, g = lam L1Norm) in fp64 on the exact operator, K = 50 plain PGD steps at
tau = 1 / L^2, once with f = QuadraticFunc(Q = A.gram(), c = -A^H y, t = 1/2 ||y||^2) (the Toeplitz gram: no
non-uniform point is touched inside the loop) and once with f = 1/2 SquaredL2Norm.asloss(y) * A.

Bound.  A PGD step u -> prox(u - tau (A^H A u - A^H y)) is non-expansive in u for tau <= 1 / L^2.  The two gradients
apply the same matrix A^H A through different arithmetic; each is within delta = 1e-12 of the exact product norm-wise
(tests/test_gpu_nufft_gram.py, tests/test_gpu_nufft.py), so one step perturbs the iterate by at most
tau L^2 2 delta max(||u||, ||y|| / L), and K steps add up to 2 K delta = 1e-10 relative to max(||u||, ||y|| / L).

``A.pinv(y, damp)`` runs CG on G + damp I with the Toeplitz G; CG stops at ||residual||_2 <= 1e-4 (its default
AbsError), and the smallest eigenvalue of G + damp I is at least damp, so the iterate is within 1e-4 / damp of the
float64 solution of the normal equations.
"""
import numpy as np
import pytest

import _nudft_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.operator.linop.nufft import _NUFFTGram  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

N, M, K = (12, 11), 150, 50


def _problem():
    rng = np.random.default_rng(11)
    x = rng.uniform(-np.pi, np.pi, size=(M, 2))
    u = np.zeros(int(np.prod(N)))
    u[rng.choice(u.size, size=9, replace=False)] = rng.uniform(1.0, 3.0, size=9) * rng.choice([-1.0, 1.0], size=9)
    A64 = R.type2_matrix64(x, N, 1, real=True)
    y = A64 @ u + 0.05 * np.random.default_rng(12).standard_normal(2 * M)
    return x, u, A64, y


def test_pgd_on_the_toeplitz_gram_tracks_the_composed_loss():
    x, u, A64, y = _problem()
    lam = 0.1 * float(np.abs(A64.T @ y).max())
    sols = {}
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A = pxo.NUFFT.type2(x, N, isign=1, real=True, eps=0)
        L, yd = float(A.lipschitz), to_device(y)
        Gop = A.gram()
        assert isinstance(Gop, _NUFFTGram)
        c = pxa.LinFunc.from_array(to_device(-to_NUMPY(A.adjoint(yd))))
        fs = dict(gram=pxa.QuadraticFunc(shape=(1, A.dim), Q=Gop, c=c, t=0.5 * float(y @ y)),
                  loss=0.5 * pxo.SquaredL2Norm(dim=2 * M).asloss(yd) * A)
        for name, f in fs.items():
            f.diff_lipschitz = L**2
            s = pxs.PGD(f=f, g=lam * pxo.L1Norm(dim=u.size), show_progress=False)
            s.fit(x0=to_device(np.zeros(u.size)), stop_crit=pxst.MaxIter(K), tau=1 / L**2, acceleration=False)
            sols[name] = to_NUMPY(s.solution())
    a, b = sols["gram"], sols["loss"]
    assert np.count_nonzero(b) > 0  # the threshold leaves a support: the comparison is not 0 against 0
    diff = np.linalg.norm(a - b) / max(np.linalg.norm(b), np.linalg.norm(y) / L)
    print(f"PGD({K}): Toeplitz gram vs composed loss {diff:.2e} (bound 1e-10), support {np.count_nonzero(b)}")
    assert diff <= 1e-10
    assert np.array_equal(a != 0, b != 0)


def test_pinv_runs_cg_on_the_toeplitz_gram():
    x, _, A64, y = _problem()
    damp = 0.1
    want = np.linalg.solve(A64.T @ A64 + damp * np.eye(A64.shape[1]), A64.T @ y)
    with pxrt.Precision(pxrt.Width.DOUBLE):
        A = pxo.NUFFT.type2(x, N, isign=1, real=True, eps=0)
        got = to_NUMPY(A.pinv(to_device(y), damp=damp))
    err = float(np.linalg.norm(got - want))
    print(f"pinv(damp={damp}): ||x - x*||_2 = {err:.2e} (CG stops at ||r|| <= 1e-4: bound {1e-4 / damp:.1e})")
    assert err <= 1e-4 / damp
