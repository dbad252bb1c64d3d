"""
The fused PGD, PD3O and Condat-Vu steps and pxa_tv_dual_update on asymmetric, off-centre, per-axis
different taps and per-axis different sampling (tests/_asym_cases.py), against the CPU oracle.

The fused steps apply H^T H as a sweep of the taps' autocorrelation (symmetric by construction) and correct the R
boundary rows / columns with ghost terms (csrc/tile2d.hpp ghost_fix / ghost_cols_coop / ghost_fix_pre; the axis-0
marches of pds3d.hpp / pds_march.hpp); the forward-difference coefficients arrive per axis, direction d being axis
d + 3 - D.  With a symmetric Gaussian on every axis and unit sampling (every other test of these kernels) a flipped
kernel in a ghost term, exchanged axes or exchanged coefficients give the same numbers.  test_oracle_asymmetric.py
proves on the CPU that with these inputs each such mistake moves the result by >= 1e-3; the tolerances here are the
project's 1e-5 (fp32) and 1e-12 / 1e-10 (fp64).
"""
import numpy as np
import pytest

import _asym_cases as ac
import oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

ALGOS = {"pd3o": pxs.PD3O, "cv": pxs.CondatVu}
DTYPES = [np.float32, np.float64]


def W(dt):
    return pxrt.Width.SINGLE if np.dtype(dt) == np.float32 else pxrt.Width.DOUBLE


def D(a):
    return to_device(np.ascontiguousarray(a))


def _operators(e, dt):
    """(data term, Gradient, g by kind, x0) of an entry on the device; inside a Precision context."""
    y, x0 = ac.data(e, dt)
    N = y.size
    S = pxo.Stencil(arg_shape=e.shape, kernel=ac.kernels(e, dt), center=list(e.centers), mode="constant")
    f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(D(y)) * S
    K = pxo.Gradient(arg_shape=e.shape, directions=e.dirs, sampling=e.sampling)
    g = {"none": None, "pos": pxo.PositiveOrthant(dim=N), "l1": ac.G_L1 * pxo.L1Norm(dim=N)}
    return f, K, g, x0


# ----------------------------------------------------------------------------- PGD
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("g_kind", ["pos", "l1"])
@pytest.mark.parametrize("e", ac.PGD_ENTRIES, ids=ac.ident)
def test_fused_pgd_vs_oracle(e, g_kind, dt):
    """6 fused PGD iterations (pxa_pgd_tv2d_*) against the oracle's, and against the generic rule-by-rule path."""
    out = {}
    with pxrt.Precision(W(dt)):
        f, K, g, x0 = _operators(e, dt)
        f = f + ac.PGD_LAM * pxo.L21Norm(arg_shape=(len(e.dirs), *e.shape)).moreau_envelope(ac.PGD_MU) * K
        f.diff_lipschitz = ac.pgd_lipschitz(e)
        for fused in (True, False):
            s = pxs.PGD(f=f, g=g[g_kind], show_progress=False)
            s.fit(x0=D(x0), stop_crit=pxst.MaxIter(ac.PGD_ITERS), fused=fused)
            assert (s._plan is not None) == fused
            out[fused] = to_NUMPY(s.solution())
    ref = ac.oracle_pgd(e, g_kind, dt, tau=dt(1 / dt(f.diff_lipschitz)))
    err = rel_err(out[True], ref)
    print(f"pgd {e.name} {g_kind} {np.dtype(dt).name}: fused {err:.3e} generic {rel_err(out[False], ref):.3e}")
    assert err <= (1e-5 if dt == np.float32 else 1e-12)
    assert rel_err(out[True], out[False]) <= 1e-5


# ----------------------------------------------------------------------------- PD3O / Condat-Vu
def _pds_run(algo, e, h_kind, lookahead, nseg=0, n=ac.PDS_ITERS):
    dt = e.dtype
    with pxrt.Precision(W(dt)):
        f, K, g, x0 = _operators(e, dt)
        f.diff_lipschitz = 1.0
        Dd, N = len(e.dirs), x0.size
        h = ac.PDS_LAM * (pxo.L21Norm(arg_shape=(Dd, *e.shape)) if h_kind == "iso" else pxo.L1Norm(dim=Dd * N))
        s = ALGOS[algo](f=f, g=g[e.g], h=h, K=K, show_progress=False)
        s._LOOKAHEAD = lookahead
        s.fit(x0=D(x0), stop_crit=pxst.MaxIter(10 ** 6), mode=pxa.Mode.MANUAL)
        assert s._plan is not None and s._plan["la"] == lookahead, "fused path not selected"
        s._plan["nseg"] = nseg
        it = s.steps()
        for _ in range(n):
            next(it)
        m = s._mstate
        return to_NUMPY(m["x"]), to_NUMPY(m["z"]), (m["tau"], m["sigma"], m["rho"])


def _pds_check(algo, e, h_kind, nseg=0):
    dt = e.dtype
    x, z, steps = _pds_run(algo, e, h_kind, True, nseg)
    x3, z3, _ = _pds_run(algo, e, h_kind, False, nseg)
    xr, zr = ac.oracle_pds(e, algo, h_kind, e.g, dt, steps)
    ex, ez = rel_err(x, xr), rel_err(z, zr)
    print(f"pds {algo} {e.name} {h_kind} {np.dtype(dt).name} nseg {nseg}: x {ex:.3e} z {ez:.3e}")
    tol = 1e-5 if dt == np.float32 else 1e-10
    assert ex <= tol and ez <= tol, (ex, ez)
    assert np.array_equal(x, x3) and np.array_equal(z, z3), (rel_err(x, x3), rel_err(z, z3))
    return x, z


@pytest.mark.parametrize("algo", ["pd3o", "cv"])
@pytest.mark.parametrize("h_kind", ["l1", "iso"])
@pytest.mark.parametrize("e", ac.ENTRIES, ids=ac.ident)
def test_fused_pds_vs_oracle(e, h_kind, algo):
    """8 iterations of the look-ahead step (pxa_pds_step_la) and of the three-launch step (pxa_pds_step): x and z
    against the oracle's, and the two steps bit for bit."""
    _pds_check(algo, e, h_kind)


@pytest.mark.parametrize("algo", ["pd3o", "cv"])
def test_fused_pds_axis0_segments_vs_oracle(algo):
    """The axis-0 march in 3 segments (n0 = 11 >= 2 nseg), axis 0 blurred with its own taps: the halo planes."""
    e = ac.BY_NAME["vol_ragged"]
    x, z = _pds_check(algo, e, e.tv, nseg=3)
    x1, z1, _ = _pds_run(algo, e, e.tv, True, nseg=1)
    assert np.array_equal(x, x1) and np.array_equal(z, z1)


# ----------------------------------------------------------------------------- the dual update alone
def np_forward(x, axis, c0, c1):
    """c0 x[i] + c1 x[i + e_axis], x = 0 outside."""
    nxt = np.zeros_like(x)
    src, dst = [slice(None)] * x.ndim, [slice(None)] * x.ndim
    src[axis], dst[axis] = slice(1, None), slice(0, -1)
    nxt[tuple(dst)] = x[tuple(src)]
    return c0 * x + c1 * nxt


# per AXIS of the kernel's (n0, n1, n2) geometry; with D = 2 the axes are 1 and 2 and axis 0's pair is never read
# (a value that would be seen at once if it were)
AXIS_C0 = {3: [-1 / 0.7, -1 / 1.9, -1 / 1.3], 2: [1e3, -1 / 0.7, -1 / 1.9]}
AXIS_C1 = {3: [1 / 0.7, 1 / 1.9, 1 / 1.3], 2: [-1e3, 1 / 0.7, 1 / 1.9]}


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("h_kind", ["l1", "iso"])
@pytest.mark.parametrize("sh", [(67, 129), (9, 33, 70)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relax", [0, 1])
def test_tv_dual_update_per_axis_coefficients(dt, h_kind, sh, relax):
    """pxa_tv_dual_update with a different (c0, c1) on every axis: relax(fenchel_prox_{sigma h}(z + sigma K w)) with
    K restated in NumPy; the tolerances of test_tv_dual_update_vs_oracle."""
    rng = np.random.default_rng(3)
    N, Dd = int(np.prod(sh)), len(sh)
    d = np.dtype(dt).type
    w = rng.standard_normal(N).astype(dt)
    z = (0.05 * rng.standard_normal(Dd * N)).astype(dt)
    sigma, lam, rho = 0.37, 0.05, 0.7
    geom = (1, 1, *sh, 2) if Dd == 2 else (1, *sh, 3)
    c0, c1 = AXIS_C0[Dd], AXIS_C1[Dd]
    out = to_NUMPY(_dev.tv_dual_update(D(w), D(z), geom, c0, c1, sigma, lam, rho, 0 if h_kind == "l1" else 1, relax=relax))
    Kw = np.concatenate([np_forward(w.reshape(sh), a, d(c0[a + 3 - Dd]), d(c1[a + 3 - Dd])).reshape(-1) for a in range(Dd)])
    if h_kind == "iso":
        hp = lambda v, t: orc.l21_prox(v, t * d(lam), (Dd, *sh))  # noqa: E731
    else:
        hp = lambda v, t: orc.l1_prox(v, t * d(lam))  # noqa: E731
    zt = orc.fenchel_prox(hp, z + d(sigma) * Kw, sigma)
    ref = (d(1 - rho) * z + d(rho) * zt) if relax == 0 else (d(rho) * zt + d(1 - rho) * z)
    err = rel_err(out, ref)
    print(f"dual {sh} {h_kind} {np.dtype(dt).name} relax {relax}: {err:.3e}")
    assert err <= (1e-5 if dt == np.float32 else 1e-10), err
