"""
CPU checks of the row threshold search's references (tests/_threshold_refs.py) and of the public surface of the norm
balls, LInfinityNorm.prox and SquaredL1Norm: the NumPy model of the kernels' Newton loop, run with the kernels'
partition, stays inside the derived bounds and reaches the sort rule's active set; the goldens agree with the
restatement; the classes exist with the reference's shapes and lipschitz values; host arrays are rejected.
"""
import math

import numpy as np
import pytest
from conftest import golden_names, load_golden, rel_err

import _prim_refs as R
import _threshold_refs as T

import pyxu_amd.operator as pxo
import pyxu_amd.runtime as pxrt
from pyxu_amd.operator import L1Ball, L2Ball, LInfinityBall, SquaredL1Norm  # noqa: F401  (what this file is about)

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", T.N_CPU)
def test_newton_model_reaches_sort_rule(n, dt):
    x = R.values(n, dt)
    S = T.l1(x)
    for name in T.COEFS:
        a, b, c = T.coef(name, S)
        ref = T.Ref(x[None], a, b, c)
        assert ref.ratio >= 390, (name, ref.ratio)  # the margin the inputs were chosen for
        mu, passes, k = T.newton_model(x, a, b, c)
        ref.check_mu([mu], [passes], tag=f"{name} n={n}")
        assert k == ref.K[0], (name, k, ref.K[0])
        assert 2 <= passes <= 17, (name, passes)
        for mode in (T.CLAMP, T.SOFT):  # the output rule in T: one rounding of the float64 value
            ref.check_out(T.shrink_ref(x, mu, mode).astype(dt)[None], mode, tag=f"{name} n={n}")


def test_newton_model_edges():
    dt = np.float32
    x = R.values(1027, dt)
    S = T.l1(x)
    assert T.newton_model(x, 1.0, 0.0, 1.5 * S) == (0.0, 1, 1027)  # inside the ball
    assert T.sort_rule(x, 1.0, 0.0, 1.5 * S)[:2] == (0.0, 0)
    assert T.newton_model(np.zeros(9, dtype=dt), 2.0, 1.0, 0.0)[0] == 0.0
    bad = x.copy()
    bad[17] = np.nan
    assert math.isnan(T.newton_model(bad, 1.0, 0.0, 1.0)[0])
    t = T.tie_row(1027, dt)
    ref = T.Ref(t[None], 1.0, 0.0, 0.3 * T.l1(t))
    assert 1.0 < ref.mu[0] < 3.0 and ref.mu[0] != round(ref.mu[0])  # between two levels
    mu, passes, k = T.newton_model(t, 1.0, 0.0, 0.3 * T.l1(t))
    ref.check_mu([mu], [passes])
    assert k == ref.K[0]


def test_partition_sums_are_sums():
    for dt in DTYPES:
        for n in (1, 5, 1027, T.RESIDENT_MAX[dt]):
            m = np.abs(R.values(n, dt).astype(np.float64))
            assert abs(T.resident_sum(m, dt) - math.fsum(m)) <= n * 2.0**-53 * math.fsum(m)
    for rows, n in ((1, 70001), (3, 40000), (1, 2**20 + 3)):
        m = np.abs(R.values(n, np.float32).astype(np.float64))
        assert abs(T.stream_sum(m, rows) - math.fsum(m)) <= n * 2.0**-53 * math.fsum(m)


@pytest.mark.parametrize("name", golden_names("balls_"))
def test_goldens_agree_with_restatement(name):
    g = load_golden(name)
    x = g["x"]
    dt = x.dtype.type
    tol = R.OP_TOL[dt]
    r, tau = float(g["radius"]), float(g["tau"])
    X = x.reshape(-1, x.shape[-1]).astype(np.float64)
    rows = lambda f: np.stack([f(v) for v in X]).reshape(x.shape)
    assert (np.abs(X).sum(axis=-1) > max(r, tau)).all()  # outside the ball: the reference raises inside it
    assert rel_err(g["l1ball_prox"], rows(lambda v: T.project_l1(v, r))) < tol
    assert rel_err(g["linf_prox"], rows(lambda v: T.prox_linf(v, tau))) < tol
    for algo in ("sort", "root"):
        assert rel_err(g[f"sql1_prox_{algo}"], rows(lambda v: T.prox_sql1(v, tau))) < tol
    assert rel_err(g["l2ball_prox"], rows(lambda v: v * min(1.0, r / np.linalg.norm(v)))) < tol
    assert rel_err(g["linfball_prox"], np.clip(X, -r, r).reshape(x.shape)) < tol
    assert rel_err(g["sql1_apply"], (np.abs(X).sum(axis=-1) ** 2).reshape(*x.shape[:-1], 1)) < tol
    for ball in ("l1ball", "l2ball", "linfball"):
        assert g[f"{ball}_apply"].shape == (*x.shape[:-1], 1) and g[f"{ball}_apply"].dtype == x.dtype
        assert (g[f"{ball}_apply_small"] == 0).all()
    assert np.isinf(g["l1ball_apply"]).all()


def test_public_names_shapes_and_lipschitz():
    import pyxu_amd.operator.func.indicator as ind
    import pyxu_amd.operator.func.norm as nrm

    assert {"L1Ball", "L2Ball", "LInfinityBall", "PositiveOrthant"} <= set(ind.__all__)
    assert "SquaredL1Norm" in nrm.__all__
    for klass, name in ((pxo.L1Ball, "L1Ball"), (pxo.L2Ball, "L2Ball"), (pxo.LInfinityBall, "LInfinityBall")):
        op = klass(dim=7, radius=2.5)
        assert op.shape == (1, 7) and op.dim == 7 and op.lipschitz == np.inf
        assert op._name == name and op._radius == 2.5 and name in repr(op)
        assert klass(dim=3)._radius == 1.0
        assert hasattr(op, "asloss") and hasattr(op, "fenchel_prox") and hasattr(op, "moreau_envelope")
    op = pxo.SquaredL1Norm(dim=5)
    assert op.shape == (1, 5) and op.lipschitz == np.inf and op._algo == "sort"
    assert pxo.SquaredL1Norm(dim=5, prox_algo=" Root ")._algo == "root"
    with pytest.raises(AssertionError):
        pxo.SquaredL1Norm(dim=5, prox_algo="bisect")
    assert pxo.LInfinityNorm(dim=5).lipschitz == 1
    # scaling keeps the functional proximable (generic rule)
    assert (0.1 * pxo.SquaredL1Norm(dim=5)).shape == (1, 5)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_host_arrays_are_rejected(dt):
    x = np.ones((2, 5), dtype=dt)
    with pxrt.Precision(pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE):
        ops = [pxo.L1Ball(5), pxo.L2Ball(5), pxo.LInfinityBall(5), pxo.LInfinityNorm(5), pxo.SquaredL1Norm(5)]
        for op in ops:
            with pytest.raises(TypeError):
                op.prox(x, 1.0)
            with pytest.raises(TypeError):
                op.apply(x)
        with pytest.raises(TypeError):
            pxo.L1Ball(5).fenchel_prox(x, 1.0)


def test_device_layer_validates_before_any_launch():
    from pyxu_amd import _dev, lib

    with pytest.raises(TypeError):
        _dev.row_threshold(np.ones((2, 5), dtype=np.float32), 1.0, 0.0, 1.0)
    with pytest.raises(TypeError):
        _dev.row_shrink(np.ones((2, 5), dtype=np.float32), np.ones(2), _dev.SHRINK_SOFT)
    assert lib.pxa_row_threshold_resident_max(0) == T.RESIDENT_MAX[np.float32]
    assert lib.pxa_row_threshold_resident_max(1) == T.RESIDENT_MAX[np.float64]
    assert lib.pxa_row_threshold_prox(0, 0, 1, T.RESIDENT_MAX[np.float32] + 1, 1, 1.0, 0.0, 1.0, 1, 1, 1, None) == -1
    assert lib.pxa_row_threshold_prox(0, 0, 1, 8, 1, 0.0, 0.0, 1.0, 1, 1, 1, None) == -1  # a must be positive
    assert lib.pxa_row_threshold_prox(0, 7, 1, 8, 1, 1.0, 0.0, 1.0, 1, 1, 1, None) == -1  # bad mode
    assert lib.pxa_row_threshold_prox(9, 0, 1, 8, 1, 1.0, 0.0, 1.0, 1, 1, 1, None) == -2  # bad dtype
    assert lib.pxa_row_threshold_stream(0, 70000, 8, 1, 1.0, 0.0, 1.0, 1, 1, 1, 1, 1, 1, None) == -1  # rows > grid.y
    assert lib.pxa_row_shrink(0, 5, 1, 8, 1, 1, 1, None) == -1
    assert lib.pxa_row_threshold_workspace_bytes(3, 70001) == 3 * (R.blocks_per_row(3, 70001) * 16 + 8)
