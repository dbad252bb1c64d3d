"""
Recovery of a few point sources from non-uniform Fourier samples through the gridded type 3: A = NUFFT.type3(x, z,
real=True) with M = 200 candidate positions x in [-pi, pi)^2 and N = 150 frequencies z in [-6, 6]^2 (300 real
equations), f = 1/2 ||A u - y||^2, g = lam L1Norm, in fp64; K = 40 PGD iterations at the fixed step 1 / L^2 (no stop
criterion but the count), once with the gridded operator (eps = 1e-6, method="grid3") and once with the exact one
(eps = 0).

Bound.  The gridded operator is within delta = RATIO_CAP_T3 eps of the exact one (tests/_nufft_type3_refs.py), a PGD
step at tau <= 1 / L^2 is non-expansive, and each step's perturbation is a small multiple of delta relative to the
iterate, so the two solves agree to a modest multiple of delta: the iterates must be within 10 RATIO_CAP_T3 eps of
each other, relative to the exact solve's, and recover the same support.
"""
import numpy as np
import pytest

import _nufft_type3_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.operator.linop import nufft as nufft_mod  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

M, N, K, EPS = 200, 150, 40, 1e-6


def test_pgd_with_the_gridded_type3_tracks_the_exact_one():
    rng = np.random.default_rng(21)
    x = rng.uniform(-np.pi, np.pi, size=(M, 2))
    z = rng.uniform(-6.0, 6.0, size=(N, 2))
    u = np.zeros(M)
    u[rng.choice(M, size=9, replace=False)] = rng.uniform(1.0, 3.0, size=9) * rng.choice([-1.0, 1.0], size=9)
    E = np.exp(1j * (z @ x.T))  # (N, M)
    A64 = np.empty((2 * N, M))
    A64[0::2], A64[1::2] = E.real, E.imag
    y = A64 @ u + 0.05 * rng.standard_normal(2 * N)
    lam = 0.1 * float(np.abs(A64.T @ y).max())
    sols = {}
    with pxrt.Precision(pxrt.Width.DOUBLE):
        for name, kw in (("grid", dict(eps=EPS, method="grid3")), ("exact", dict(eps=0))):
            A = pxo.NUFFT.type3(x, z, isign=1, real=True, **kw)
            assert type(A) is (nufft_mod._NUFFTGrid3 if name == "grid" else nufft_mod._NUDFT)
            assert A.shape == A64.shape
            f = 0.5 * pxo.SquaredL2Norm(dim=2 * N).asloss(to_device(y)) * A
            f.diff_lipschitz = A.lipschitz**2
            s = pxs.PGD(f=f, g=lam * pxo.L1Norm(dim=M), show_progress=False)
            s.fit(x0=to_device(np.zeros(M)), stop_crit=pxst.MaxIter(K), tau=1 / A.lipschitz**2, acceleration=False)
            sols[name] = to_NUMPY(s.solution())
    a, b = sols["grid"], sols["exact"]
    assert np.count_nonzero(b) > 0  # the threshold leaves a support: the comparison is not 0 against 0
    diff, bound = np.linalg.norm(a - b) / np.linalg.norm(b), 10 * T.RATIO_CAP_T3 * EPS
    print(f"PGD({K}): gridded vs exact iterate {diff:.2e} (bound {bound:.2e}), support {np.count_nonzero(b)}")
    assert 0 < diff <= bound  # different operators, iterates within the bound
    assert np.array_equal(a != 0, b != 0)
