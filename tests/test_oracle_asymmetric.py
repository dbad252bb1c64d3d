"""
The CPU oracle on asymmetric, per-axis different taps and per-axis sampling (tests/_asym_cases.py), pinned
independently of itself, and the proof that those inputs discriminate:

* stencil_apply against scipy.ndimage.correlate1d (origin = centre - len // 2), axis by axis;
* stencil_adjoint, gradient_apply (tuple sampling; also against a NumPy restatement of the forward difference)
  and gradient_adjoint against dense matrices built column by column, at the shapes with N <= 3000;
* the oracle's PGD / PD3O / Condat-Vu trajectories against goldens recorded from the reference itself
  (tests/golden/asym_*.npz, make_goldens.py gen_asym);
* every wrong convention of _asym_cases.mutants() moves the oracle trajectory of every entry, over the iterations
  the GPU tests run, by >= 1e-3 norm-wise relative: 100x the fp32 tolerance of test_gpu_fused_asymmetric.py.
"""
import numpy as np
import pytest
import scipy.ndimage as snd

import _asym_cases as ac
import oracle as orc
from conftest import golden_names, load_golden, rel_err

MUTANT_MIN = 1e-3
DENSE = [e for e in ac.ENTRIES if int(np.prod(e.shape)) <= 3000]


@pytest.mark.parametrize("e", ac.ENTRIES, ids=ac.ident)
def test_table_is_normalised_and_distinct(e):
    ks = ac.kernels(e, np.float64)
    for k in ks:
        assert abs(np.abs(k).sum() - 1) <= 1e-15
    assert max(ac.reach(e.taps, e.centers)) <= 8
    assert len(set(e.sampling)) == len(e.sampling)
    blurred = [(tuple(k), c) for k, c in zip(e.taps, e.centers) if len(k) > 1]
    assert len(set(blurred)) == len(blurred)
    for k, c in blurred:
        assert list(k) != list(k[::-1]) or 2 * c != len(k) - 1  # not symmetric about its centre


def test_table_coverage():
    """What the table must contain across its entries."""
    ax = [(len(k), c, min(k) < 0) for e in ac.ENTRIES for k, c in zip(e.taps, e.centers) if len(k) > 1]
    assert any(c == 0 for n, c, _ in ax) and any(c == n - 1 for n, c, _ in ax)  # one-sided, both sides
    assert any(0 < c < n - 1 and 2 * c != n - 1 and neg for n, c, neg in ax)  # two-sided asymmetric, negative tap
    reaches = [ac.reach(e.taps, e.centers) for e in ac.ENTRIES]
    assert any(8 in r for r in reaches) and any(2 in r and 7 in r for r in reaches)
    two_d = [[len(k) > 1 for k in e.taps] for e in ac.ENTRIES if len(e.shape) == 2]
    assert [True, False] in two_d and [False, True] in two_d
    three_d = [e for e in ac.ENTRIES if len(e.shape) == 3]
    assert any(len(e.taps[0]) > 1 and e.dirs == (0, 1, 2) for e in three_d)
    assert any(len(e.taps[0]) == 1 and e.dirs == (0, 1, 2) for e in three_d)
    assert any(e.dirs == (1, 2) for e in three_d)
    assert {e.shape for e in ac.ENTRIES} == {(7, 12), (30, 60), (37, 70), (40, 68), (6, 9, 11), (11, 37, 70), (4, 33, 66)}


# ----------------------------------------------------------------------------- operators
@pytest.mark.parametrize("e", ac.ENTRIES, ids=ac.ident)
def test_stencil_apply_vs_scipy(e):
    rng = np.random.default_rng(0)
    x = rng.standard_normal(e.shape)
    ks = ac.kernels(e, np.float64)
    ref = x
    for a, (k, c) in enumerate(zip(ks, e.centers)):
        ref = snd.correlate1d(ref, k, axis=a, mode="constant", cval=0.0, origin=c - len(k) // 2)
    got = orc.stencil_apply(x.reshape(-1), e.shape, ks, e.centers)
    assert rel_err(got, ref.reshape(-1)) <= 1e-13


def _dense(fn, N):
    """Matrix of a linear map, one unit vector (column) at a time."""
    cols = []
    for j in range(N):
        u = np.zeros(N)
        u[j] = 1.0
        cols.append(fn(u))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("e", DENSE, ids=ac.ident)
def test_stencil_adjoint_vs_dense_transpose(e):
    N = int(np.prod(e.shape))
    ks = ac.kernels(e, np.float64)
    M = _dense(lambda u: orc.stencil_apply(u, e.shape, ks, e.centers), N)
    z = np.random.default_rng(1).standard_normal(N)
    assert rel_err(orc.stencil_adjoint(z, e.shape, ks, e.centers), M.T @ z) <= 1e-13


def _forward_diff(x, axis, h):
    """(x[i + e] - x[i]) / h, x = 0 outside."""
    nxt = np.zeros_like(x)
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    src[axis], dst[axis] = slice(1, None), slice(0, -1)
    nxt[tuple(dst)] = x[tuple(src)]
    return (nxt - x) / h


@pytest.mark.parametrize("e", ac.ENTRIES, ids=ac.ident)
def test_gradient_apply_tuple_sampling(e):
    x = np.random.default_rng(2).standard_normal(e.shape)
    ref = np.concatenate([_forward_diff(x, a, e.sampling[a]).reshape(-1) for a in e.dirs])
    assert rel_err(orc.gradient_apply(x.reshape(-1), **ac.grad_kw(e)), ref) <= 1e-13


@pytest.mark.parametrize("e", DENSE, ids=ac.ident)
def test_gradient_adjoint_vs_dense_transpose(e):
    N = int(np.prod(e.shape))
    gk = ac.grad_kw(e)
    M = _dense(lambda u: orc.gradient_apply(u, **gk), N)  # (D N, N)
    x = np.random.default_rng(3).standard_normal(N)
    z = np.random.default_rng(4).standard_normal(M.shape[0])
    assert rel_err(orc.gradient_apply(x, **gk), M @ x) <= 1e-13
    assert rel_err(orc.gradient_adjoint(z, **gk), M.T @ z) <= 1e-13


# ----------------------------------------------------------------------------- goldens from the reference
def _golden_entry(g):
    e = ac.BY_NAME[str(g["entry"])]
    # the golden carries the kernels and sampling it was recorded with: the table must not have drifted since
    dt = g["x0"].dtype.type
    for a, k in enumerate(ac.kernels(e, dt)):
        np.testing.assert_array_equal(k, g[f"kernel{a}"])
    np.testing.assert_array_equal(g["center"], e.centers)
    np.testing.assert_array_equal(g["sampling"], e.sampling)
    y, x0 = ac.data(e, dt)
    np.testing.assert_array_equal(y, g["y"])
    np.testing.assert_array_equal(x0, g["x0"])
    return e, dt


TOL = {np.float32: 1e-6, np.float64: 1e-13}


@pytest.mark.parametrize("name", golden_names("asym_pgd"))
def test_pgd_trajectory_vs_reference(name):
    g = load_golden(name)
    e, dt = _golden_entry(g)
    assert float(g["diff_lipschitz"]) == ac.pgd_lipschitz(e)
    snap = {1: None, 10: None}
    ac.oracle_pgd(e, str(g["g"]), dt, n=10, snap=snap)
    for n in (1, 10):
        assert rel_err(snap[n], g[f"x_{n}"]) <= TOL[dt] * 10, n


@pytest.mark.parametrize("name", golden_names("asym_pds"))
def test_pds_trajectory_vs_reference(name):
    g = load_golden(name)
    e, dt = _golden_entry(g)
    for algo in ("pd3o", "cv"):
        steps = tuple(dt(g[f"{algo}_{k}"]) for k in ("tau", "sigma", "rho"))
        snap = {1: None, 10: None}
        ac.oracle_pds(e, algo, str(g["tv"]), str(g["g"]), dt, steps, n=10, snap=snap)
        for n in (1, 10):
            assert rel_err(snap[n][0], g[f"{algo}_x_{n}"]) <= TOL[dt] * 10, (algo, n)
            assert rel_err(snap[n][1], g[f"{algo}_z_{n}"]) <= TOL[dt] * 10, (algo, n)


# ----------------------------------------------------------------------------- the inputs discriminate
@pytest.mark.parametrize("g_kind", ["pos", "l1"])
@pytest.mark.parametrize("e", ac.PGD_ENTRIES, ids=ac.ident)
def test_pgd_mutants_move_the_trajectory(e, g_kind):
    dt = e.dtype
    ref = ac.oracle_pgd(e, g_kind, dt)
    for name, conv in ac.mutants(e).items():
        d = rel_err(ac.oracle_pgd(e, g_kind, dt, conv), ref)
        assert d >= MUTANT_MIN, (name, d)


@pytest.mark.parametrize("algo", ["pd3o", "cv"])
@pytest.mark.parametrize("h_kind", ["l1", "iso"])
@pytest.mark.parametrize("e", ac.ENTRIES, ids=ac.ident)
def test_pds_mutants_move_the_trajectory(e, h_kind, algo):
    dt = e.dtype
    steps = ac.pds_steps(e, dt)
    xr, zr = ac.oracle_pds(e, algo, h_kind, e.g, dt, steps)
    for name, conv in ac.mutants(e).items():
        x, z = ac.oracle_pds(e, algo, h_kind, e.g, dt, steps, conv)
        dx, dz = rel_err(x, xr), rel_err(z, zr)
        assert dx >= MUTANT_MIN and dz >= MUTANT_MIN, (name, dx, dz)


def test_fp32_oracle_is_far_below_the_mutants():
    """The fp32 oracle against the fp64 one on the same (fp32-rounded) inputs: orders of magnitude under 1e-3."""
    e = ac.BY_NAME["onetile"]
    y, x0 = ac.data(e, np.float32)
    out = {}
    for dt in (np.float32, np.float64):
        blur = dict(arg_shape=e.shape, kernel=[k.astype(dt) for k in ac.kernels(e, np.float32)], center=e.centers)
        grad = lambda v: orc.deblur_tv_grad(v, blur, y.astype(dt), ac.PGD_LAM, ac.PGD_MU, ac.grad_kw(e))  # noqa: E731
        tau = dt(np.float32(1 / np.float32(ac.pgd_lipschitz(e))))
        out[dt], _ = orc.pgd(x0.astype(dt), grad, ac.g_prox("pos", dt), tau, ac.PGD_ITERS)
    assert rel_err(out[np.float32], out[np.float64]) <= 1e-6
