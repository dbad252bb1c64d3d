"""
The row threshold search and shrink (csrc/threshold.hip) through pyxu_amd._dev and through the public classes built
on it (LInfinityNorm.prox, L1Ball, SquaredL1Norm), with L2Ball / LInfinityBall beside them.

Every parity case is held to the derived bounds of tests/_threshold_refs.py against the float64 sort rule, after that
module has asserted on the reference alone that no magnitude lies within 10 bounds of mu*: the active set is then
determined, and the support / clamped set must equal the reference's exactly.  Shapes: the vector tail alone (1, 2,
5), one workgroup (1027), the resident limit and the first streaming row, few and many blocks per row; 1, 3 and 300
rows, and more rows than grid.y takes.
"""
import functools

import numpy as np
import pytest
from conftest import golden_names, load_golden, rel_err

import _prim_refs as R
import _threshold_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
MODES = ((T.CLAMP, "clamp"), (T.SOFT, "soft"))


def W(dt):
    return pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE


@functools.lru_cache(maxsize=None)
def _input(rows, n, d):
    x2 = T.rows_input(rows, n, DT[d])
    x2.setflags(write=False)
    return x2


@functools.lru_cache(maxsize=None)
def _ref(rows, n, d, cname):
    x2 = _input(rows, n, d)
    a, b, c = T.coef(cname, T.l1(x2[0]))
    return (a, b, c), T.Ref(x2, a, b, c)


def _bits(t):
    return R.to_host(t).tobytes()


def _path_cases():
    return [pytest.param(n, d, id=f"{n}-{d}") for d in DT for n in T.shapes(DT[d])]


@pytest.mark.parametrize("n,d", _path_cases())
def test_paths_one_row(n, d):
    """mu*, pass count, both outputs and their support for the four coefficient sets; a second run and (streaming
    rows) batches of one pass give the same bits."""
    dt = DT[d]
    xd = R.to_dev(_input(1, n, d))
    streaming = n > T.RESIDENT_MAX[dt]
    assert _dev.row_threshold_resident_max(xd) == T.RESIDENT_MAX[dt]
    for cname in T.COEFS:
        (a, b, c), ref = _ref(1, n, d, cname)
        mu, passes = _dev.row_threshold(xd, a, b, c)
        assert mu.dtype == torch.float64 and passes.dtype == torch.int32 and mu.shape == passes.shape == (1,)
        print(cname, n, d, "mu", float(mu[0]), "ref", ref.mu[0], "bound", ref.bound[0], "passes", int(passes[0]))
        ref.check_mu(R.to_host(mu), R.to_host(passes), tag=f"{cname} {n} {d}")
        assert 2 <= int(passes[0]) <= 17
        for mode, mname in MODES:
            out, mu2, p2 = _dev.row_threshold_prox(xd, a, b, c, mode, info=True)
            ref.check_out(R.to_host(out), mode, tag=f"{cname} {mname} {n} {d}")
            assert _bits(mu2) == _bits(mu) and _bits(p2) == _bits(passes)
            out2 = _dev.row_threshold_prox(xd, a, b, c, mode)
            assert _bits(out2) == _bits(out)
            # the two-step form: shrink at the device mu
            assert _bits(_dev.row_shrink(xd, mu, mode)) == _bits(out)
        if streaming:
            mu1, p1 = _dev.row_threshold(xd, a, b, c, batch=1)
            assert _bits(mu1) == _bits(mu) and _bits(p1) == _bits(passes)
            mu3, p3 = _dev.row_threshold(xd, a, b, c, batch=3)
            assert _bits(mu3) == _bits(mu) and _bits(p3) == _bits(passes)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n", [(3, 5), (3, 1027), (300, 1027), (3, 70001)])
def test_several_rows(rows, n, d):
    """Every row gets its own threshold; a row's result does not depend on the rows it is stacked with on the
    resident path (one workgroup per row)."""
    dt = DT[d]
    xd = R.to_dev(_input(rows, n, d))
    for cname in ("l1_30", "sq_10"):
        (a, b, c), ref = _ref(rows, n, d, cname)
        for mode, mname in MODES:
            out, mu, passes = _dev.row_threshold_prox(xd, a, b, c, mode, info=True)
            ref.check_mu(R.to_host(mu), R.to_host(passes), tag=f"{cname} {rows}x{n} {d}")
            ref.check_out(R.to_host(out), mode, tag=f"{cname} {mname} {rows}x{n} {d}")
        if n <= T.RESIDENT_MAX[dt]:
            mu0, _ = _dev.row_threshold(xd[1:2], a, b, c)
            assert _bits(mu0) == _bits(mu[1:2])


def test_more_rows_than_grid_y():
    rows, n, dt = 65536 + 5, 5, np.float32
    r = R.rng_for("slabs", rows, n)
    x2 = (10.0 ** r.uniform(-2.0, 2.0, (rows, n)) * r.choice([-1.0, 1.0], (rows, n))).astype(dt)
    a, b, c = 1.0, 0.0, 3.0  # some rows inside the ball, most outside
    ref = T.Ref(x2, a, b, c)
    assert 0 < (ref.K == 0).sum() < rows // 2
    out, mu, passes = _dev.row_threshold_prox(R.to_dev(x2), a, b, c, T.SOFT, info=True)
    ref.check_mu(R.to_host(mu), R.to_host(passes), tag="slabs")
    ref.check_out(R.to_host(out), T.SOFT, tag="slabs")
    got = R.to_host(_dev.row_shrink(R.to_dev(x2), mu, T.CLAMP))
    ref.check_out(got, T.CLAMP, tag="slabs shrink")


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n", [(1, 5), (1, 1027), (3, 1027), (1, 70001), (3, 70001)])
def test_unaligned_views_and_aliasing(rows, n, d):
    """x and out one element into their allocations (scalar loads and stores): same results, guards intact; out = x."""
    x2 = _input(rows, n, d)
    (a, b, c), ref = _ref(rows, n, d, "l1_30")
    mu_al, _ = _dev.row_threshold(R.to_dev(x2), a, b, c)
    for mode, mname in MODES:
        xb, xv = R.placed(x2, off=1)
        ob, ov = R.placed(np.zeros_like(x2), off=1)
        xv, ov = xv.reshape(rows, n), ov.reshape(rows, n)
        out, mu, passes = _dev.row_threshold_prox(xv, a, b, c, mode, out=ov, info=True)
        assert out.data_ptr() == ov.data_ptr()
        assert R.guards_intact(ob, 1, rows * n) and R.guards_intact(xb, 1, rows * n)
        np.testing.assert_array_equal(R.to_host(xv), x2)
        assert _bits(mu) == _bits(mu_al)  # the fold order does not depend on the alignment
        ref.check_out(R.to_host(ov), mode, tag=f"unaligned {mname} {rows}x{n} {d}")
        # in place, aligned and not
        for off in (0, 1):
            xb, xv = R.placed(x2, off=off)
            xv = xv.reshape(rows, n)
            got = _dev.row_threshold_prox(xv, a, b, c, mode, out=xv)
            assert got.data_ptr() == xv.data_ptr() and R.guards_intact(xb, off, rows * n)
            assert _bits(xv) == _bits(ov)
            xb, xv = R.placed(x2, off=off)
            xv = xv.reshape(rows, n)
            _dev.row_shrink(xv, mu, mode, out=xv)
            assert R.guards_intact(xb, off, rows * n) and _bits(xv) == _bits(ov)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("n", [5, 1027, 70001])
def test_edges(n, d):
    dt = DT[d]
    x2 = _input(3, n, d)
    S = max(T.l1(r) for r in x2)
    xd = R.to_dev(x2)
    with pxrt.Precision(W(dt)):
        # inside the ball: the projection is x bit for bit, the LInfinityNorm prox is 0 (the reference raises)
        ball = R.to_host(pxo.L1Ball(dim=n, radius=1.5 * S).prox(xd, tau=1.0))
        np.testing.assert_array_equal(ball, x2)
        assert ball.tobytes() == x2.tobytes()
        np.testing.assert_array_equal(R.to_host(pxo.LInfinityNorm(dim=n).prox(xd, tau=1.5 * S)), np.zeros_like(x2))
        mu, passes = _dev.row_threshold(xd, 1.0, 0.0, 1.5 * S)
        assert (R.to_host(mu) == 0).all() and (R.to_host(passes) == 1).all()
        # on the boundary ||x||_1 == r exactly (small integers: the sum is exact)
        e = np.zeros((1, n), dtype=dt)
        e[0, : min(n, 3)] = [3.0, -2.0, 1.0][: min(n, 3)]
        got = R.to_host(pxo.L1Ball(dim=n, radius=float(np.abs(e).sum())).prox(R.to_dev(e), tau=1.0))
        assert got.tobytes() == e.tobytes()
        # an all-zero row
        z = np.zeros((2, n), dtype=dt)
        for op in (pxo.L1Ball(dim=n, radius=1.0), pxo.LInfinityNorm(dim=n), pxo.SquaredL1Norm(dim=n)):
            np.testing.assert_array_equal(R.to_host(op.prox(R.to_dev(z), tau=0.5)), z)
    # ties: integers 1..3, mu* between two levels
    t = np.stack([T.tie_row(n, dt), -T.tie_row(n, dt)])
    c = 0.3 * T.l1(t[0])
    ref = T.Ref(t, 1.0, 0.0, c)
    if n > 5:
        assert 1.0 < ref.mu[0] < 3.0 and ref.mu[0] != round(ref.mu[0])
    for mode, mname in MODES:
        out, mu, passes = _dev.row_threshold_prox(R.to_dev(t), 1.0, 0.0, c, mode, info=True)
        ref.check_mu(R.to_host(mu), R.to_host(passes), tag=f"ties {n} {d}")
        ref.check_out(R.to_host(out), mode, tag=f"ties {mname} {n} {d}")
    # one NaN (or inf) in the middle row: that row is all NaN, its neighbours are what they are without it
    (a, b, c), ref = _ref(3, n, d, "l1_30")
    for poison in (np.nan, np.inf):
        bad = x2.copy()
        bad[1, n // 2] = poison
        for mode, mname in MODES:
            out, mu, passes = _dev.row_threshold_prox(R.to_dev(bad), a, b, c, mode, info=True)
            out, mu = R.to_host(out), R.to_host(mu)
            assert np.isnan(out[1]).all() and np.isnan(mu[1]) and int(passes[1]) == 1
            good, mu_good = _dev.row_threshold_prox(xd, a, b, c, mode, info=True)[:2]
            good = R.to_host(good)
            if n <= T.RESIDENT_MAX[dt]:  # one workgroup per row: the same bits
                assert out[[0, 2]].tobytes() == good[[0, 2]].tobytes()
            assert mu[[0, 2]].tobytes() == R.to_host(mu_good)[[0, 2]].tobytes()
            ref.check_out(np.where(np.isnan(out), good, out), mode, tag=f"nan neighbours {mname} {n} {d}")


@pytest.mark.parametrize("d", list(DT))
def test_empty_inputs(d):
    dt = DT[d]
    for shape in ((0, 7), (3, 0), (0, 0)):
        xd = torch.empty(shape, dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
        mu, passes = _dev.row_threshold(xd, 1.0, 0.0, 1.0)
        assert mu.shape == passes.shape == (shape[0],)
        assert (R.to_host(mu) == 0).all()
        for mode, _ in MODES:
            assert _dev.row_threshold_prox(xd, 1.0, 0.0, 1.0, mode).shape == shape
            assert _dev.row_shrink(xd, mu, mode).shape == shape
    with pytest.raises(ValueError):
        _dev.row_threshold(torch.ones((2, 3), device="cuda"), 0.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        _dev.row_threshold_prox(torch.ones((2, 3), device="cuda"), 1.0, 0.0, 1.0, 5)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("n", [1027, 70001])
def test_public_classes_and_stacking(n, d):
    """LInfinityNorm.prox, L1Ball.prox and SquaredL1Norm.prox (both prox_algo values) on a (2, 3, n) stack: every
    row its own result, in the runtime precision."""
    dt = DT[d]
    x2 = _input(6, n, d)
    x3 = x2.reshape(2, 3, n)
    S = T.l1(x2[0])
    tau = 0.3 * S
    with pxrt.Precision(W(dt)):
        xd = R.to_dev(x3)
        got = R.to_host(pxo.LInfinityNorm(dim=n).prox(xd, tau=tau))
        assert got.shape == x3.shape and got.dtype == dt
        T.Ref(x2, 1.0, 0.0, float(dt(tau))).check_out(got.reshape(6, n), T.CLAMP, tag="LInfinityNorm.prox")
        got = R.to_host(pxo.L1Ball(dim=n, radius=tau).prox(xd, tau=123.0))  # tau is ignored
        assert got.shape == x3.shape and got.dtype == dt
        ref = T.Ref(x2, 1.0, 0.0, tau)
        ref.check_out(got.reshape(6, n), T.SOFT, tag="L1Ball.prox")
        assert (np.abs(got.astype(np.float64)).sum(axis=-1) <= tau * (1 + 4 * R.eps(dt))).all()
        one = R.to_host(pxo.L1Ball(dim=n, radius=tau).prox(R.to_dev(x2[4]), tau=1.0))
        assert one.shape == (n,)
        if n <= T.RESIDENT_MAX[dt]:
            assert one.tobytes() == got[1, 1].tobytes()
        ref.check_out(np.where(np.arange(6)[:, None] == 4, one[None], got.reshape(6, n)), T.SOFT, tag="L1Ball.prox 1-D")
        for algo in ("sort", "root"):
            t = 0.05
            got = R.to_host(pxo.SquaredL1Norm(dim=n, prox_algo=algo).prox(xd, tau=t))
            T.Ref(x2, 2.0 * float(dt(t)), 1.0, 0.0).check_out(got.reshape(6, n), T.SOFT, tag=f"SquaredL1Norm.prox {algo}")
        # apply
        sq = R.to_host(pxo.SquaredL1Norm(dim=n).apply(xd))
        assert sq.shape == (2, 3, 1) and sq.dtype == dt
        np.testing.assert_allclose(sq.reshape(6), np.abs(x2.astype(np.float64)).sum(axis=1) ** 2, rtol=4 * R.eps(dt))
        X = x2.astype(np.float64)
        norms = {pxo.L1Ball: np.abs(X).sum(axis=1), pxo.L2Ball: np.sqrt((X * X).sum(axis=1)),
                 pxo.LInfinityBall: np.abs(X).max(axis=1)}
        for klass, nr in norms.items():
            radius = float(np.sort(nr)[2] * (1 + 1e-3))  # three rows inside, three outside
            ind = R.to_host(klass(dim=n, radius=radius).apply(xd))
            assert ind.shape == (2, 3, 1) and ind.dtype == dt
            np.testing.assert_array_equal(ind.reshape(6), np.where(nr <= radius, 0.0, np.inf))
        bad = x3.copy()
        bad[0, 1, 3] = np.nan
        ind = R.to_host(pxo.L2Ball(dim=n, radius=1e30).apply(R.to_dev(bad))).reshape(6)
        np.testing.assert_array_equal(ind, [0, np.inf, 0, 0, 0, 0])
        # L2Ball / LInfinityBall projections
        r2 = float(np.median(norms[pxo.L2Ball]))
        got = R.to_host(pxo.L2Ball(dim=n, radius=r2).prox(xd, tau=1.0)).reshape(6, n)
        # x - L2Norm.prox(x, r) as the reference composes it; L2Norm.prox (the L21 kernel with one group spanning the
        # row) adds the n squares one after the other in T: the sum is off by at most n u, the norm and with it the
        # factor r / ||x|| by n u / 2 = n eps / 4 relative; the few roundings after that are covered by 8 eps
        err = rel_err(got, X * np.minimum(1.0, r2 / norms[pxo.L2Ball])[:, None])
        print("L2Ball.prox", n, d, "rel err", err)
        assert err < (0.25 * n + 8) * R.eps(dt), err
        got = R.to_host(pxo.LInfinityBall(dim=n, radius=0.5).prox(xd, tau=1.0))
        np.testing.assert_array_equal(got, np.clip(x3, dt(-0.5), dt(0.5)))


@pytest.mark.parametrize("name", golden_names("balls_"))
def test_goldens(name):
    g = load_golden(name)
    x = g["x"]
    dt = x.dtype.type
    dim, r, tau = int(g["dim"]), float(g["radius"]), float(g["tau"])
    tol = R.OP_TOL[dt]
    with pxrt.Precision(W(dt)):
        xd, sd = R.to_dev(x), R.to_dev(g["small"])
        for key, klass in (("l1ball", pxo.L1Ball), ("l2ball", pxo.L2Ball), ("linfball", pxo.LInfinityBall)):
            op = klass(dim=dim, radius=r)
            got = R.to_host(op.prox(xd, tau=tau))
            assert got.dtype == x.dtype and got.shape == x.shape
            assert rel_err(got, g[f"{key}_prox"]) < tol, (key, rel_err(got, g[f"{key}_prox"]))
            np.testing.assert_array_equal(R.to_host(op.apply(xd)), g[f"{key}_apply"])
            np.testing.assert_array_equal(R.to_host(op.apply(sd)), g[f"{key}_apply_small"])
        got = R.to_host(pxo.LInfinityNorm(dim=dim).prox(xd, tau=tau))
        assert rel_err(got, g["linf_prox"]) < tol, rel_err(got, g["linf_prox"])
        for algo in ("sort", "root"):
            got = R.to_host(pxo.SquaredL1Norm(dim=dim, prox_algo=algo).prox(xd, tau=tau))
            assert rel_err(got, g[f"sql1_prox_{algo}"]) < tol, (algo, rel_err(got, g[f"sql1_prox_{algo}"]))
        assert rel_err(R.to_host(pxo.SquaredL1Norm(dim=dim).apply(xd)), g["sql1_apply"]) < tol


def test_generic_rules_fp64():
    """fenchel_prox (Moreau identity) and the Moreau envelope's gradient come from the generic ProxFunc rules:
    fenchel_prox_{sigma}(||.||_inf) is the projection on the unit l1 ball, that of the ball's indicator is
    x - sigma P(x / sigma), and grad of the mu-envelope of ||.||_inf is P_{mu}(x) / mu."""
    dt, n = np.float64, 1027
    x2 = _input(3, n, "f64")
    X = x2.astype(np.float64)
    tol = R.OP_TOL[dt]
    with pxrt.Precision(pxrt.Width.DOUBLE):
        xd = R.to_dev(x2)
        got = R.to_host(pxo.LInfinityNorm(dim=n).fenchel_prox(xd, sigma=0.7))
        assert rel_err(got, np.stack([T.project_l1(v, 1.0) for v in X])) < tol
        lam = 2.5  # (lam f)^* prox: projection on the ball of radius lam
        got = R.to_host((lam * pxo.LInfinityNorm(dim=n)).fenchel_prox(xd, sigma=0.7))
        assert rel_err(got, np.stack([T.project_l1(v, lam) for v in X])) < tol
        r, sigma = 40.0, 0.7
        got = R.to_host(pxo.L1Ball(dim=n, radius=r).fenchel_prox(xd, sigma=sigma))
        assert rel_err(got, np.stack([v - sigma * T.project_l1(v / sigma, r) for v in X])) < tol
        mu = 3.0
        env = pxo.LInfinityNorm(dim=n).moreau_envelope(mu)
        got = R.to_host(env.grad(xd))
        assert rel_err(got, np.stack([T.project_l1(v, mu) for v in X]) / mu) < tol
        val = R.to_host(env.apply(xd)).reshape(3)
        P = np.stack([T.prox_linf(v, mu) for v in X])
        np.testing.assert_allclose(val, np.abs(P).max(axis=1) + ((X - P) ** 2).sum(axis=1) / (2 * mu), rtol=1e-12)
