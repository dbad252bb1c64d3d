"""
Sparse recovery from non-uniform Fourier samples on the device: A = NUFFT.type2(x, N=(12, 11), real=True, eps=0) with
M = 150 samples, f = 1/2 ||A u - y||^2 (diff_lipschitz = A.lipschitz^2), g = lam L1Norm, 15 PGD iterations.

The comparison is the NumPy oracle's PGD (oracle.pgd, the reference's m_init / m_step restated) run in float64 on the
dense float64 matrix of the transform (tests/_nudft_refs.py::type2_matrix64); the device trajectory must agree to the
project's parity tolerance, 1e-5 relative in fp32 and 1e-10 in fp64.
"""
import numpy as np
import pytest

import _nudft_refs as R
import oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

N, M, ITERS = (12, 11), 150, 15
TOL = {np.float32: 1e-5, np.float64: 1e-10}


def _problem():
    rng = np.random.default_rng(11)
    x = rng.uniform(-np.pi, np.pi, size=(M, 2))
    u = np.zeros(int(np.prod(N)))
    u[rng.choice(u.size, size=9, replace=False)] = rng.uniform(1.0, 3.0, size=9) * rng.choice([-1.0, 1.0], size=9)
    return x, u


@pytest.mark.parametrize("dt, width", [(np.float32, pxrt.Width.SINGLE), (np.float64, pxrt.Width.DOUBLE)])
def test_pgd_sparse_recovery_matches_dense_oracle(dt, width):
    x, u = _problem()
    x = x.astype(dt)  # the sample points the operator sees
    A64 = R.type2_matrix64(x, N, 1, real=True)
    assert A64.shape == (2 * M, u.size)
    y = (A64 @ u + 0.05 * np.random.default_rng(12).standard_normal(2 * M)).astype(dt)
    lam = 0.1 * float(np.abs(A64.T @ y).max())
    with pxrt.Precision(width):
        A = pxo.NUFFT.type2(x, N, isign=1, real=True, eps=0)
        assert A.shape == A64.shape
        f = 0.5 * pxo.SquaredL2Norm(dim=2 * M).asloss(to_device(y)) * A
        f.diff_lipschitz = A.lipschitz**2
        g = lam * pxo.L1Norm(dim=u.size)
        s = pxs.PGD(f=f, g=g, show_progress=False)
        s.fit(x0=to_device(np.zeros(u.size, dtype=dt)), stop_crit=pxst.MaxIter(ITERS))
        got = to_NUMPY(s.solution())
    tau = float(dt(1 / (A.lipschitz**2)))  # the step the solver coerced to its precision
    y64 = y.astype(np.float64)
    ref, _ = orc.pgd(np.zeros(u.size), lambda v: A64.T @ (A64 @ v - y64), lambda z, t: orc.l1_prox(z, lam * t), tau, ITERS)
    assert got.dtype == dt
    assert np.count_nonzero(ref) > 0  # the threshold leaves a support: the comparison is not 0 against 0
    err = rel_err(got, ref)
    print(f"{np.dtype(dt).name}: PGD({ITERS}) vs float64 dense oracle, rel err {err:.2e}")
    assert err <= TOL[dt]
