"""
NLCG and the backtracking line search on the device (csrc/nlcg.hip, pyxu_amd/math/linesearch.py,
pyxu_amd/opt/solver/nlcg.py) against the float64 NumPy restatement of tests/_nlcg_refs.py, on the cases whose
comparability conditions tests/test_nlcg_refs.py asserts.

Bounds of the kernel-level checks (derived, in the style of tests/_prim_refs.py; eps = finfo(T).eps):
* sum g1^2, <g1, p_new>: double accumulation of products of T values, any order: |got - ref| <= (n + 4) 2^-53 sum |t_i|.
* beta = (T)(num / gg0): one rounding to T of a double quotient whose numerator carries the sum bound above:
  |beta - beta_ref| <= eps |beta_ref| + 2 (n + 4) 2^-53 sum |t_i| / gg0.
* p_new = fma(beta, p, -g1): |got - (beta_ref p - g1)| <= |p| dbeta + 8 eps (|beta_ref p| + |g1|) (CHAIN_FACTOR of
  _prim_refs: either contraction choice).  beta == 0 (PR clipped, restart): p_new == -g1 bit for bit.
"""
import numpy as np
import pytest
from conftest import load_golden

import _nlcg_refs as N
import _prim_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.math as pxm  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.solver.nlcg as nlcg_mod  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_NUMPY  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
TRAJ_TOL = {np.float32: 1e-5, np.float64: 1e-10}  # test_gpu_parity.py
FUSED_TOL = {np.float32: 1e-6, np.float64: 1e-13}
TRAJ_CASES = [(name, d) for name in N.CASES for d in DT if d == "f64" or N.CASES[name][1]]


def W(dt):
    return pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE


def _objective(gold, dt):
    """The golden's objective on the device (call under pxrt.Precision(W(dt)))."""
    if "A" in gold:
        return pxo.SquaredL2Norm(dim=24).asloss(R.to_dev(gold["b"].astype(dt))) * pxa.LinOp.from_array(
            R.to_dev(gold["A"].astype(dt)))
    G = pxo.Gradient(tuple(int(s) for s in gold["shape"]), diff_method="fd", mode="constant")
    return 0.5 * pxo.SquaredL2Norm(dim=99).asloss(R.to_dev(gold["y"].astype(dt))) + float(gold["lam"]) * (
        pxo.L1Norm(dim=198).moreau_envelope(float(gold["mu"])) * G)


def _fit(gold, dt, fused=True):
    prev = nlcg_mod._FUSED
    nlcg_mod._FUSED = fused
    try:
        with pxrt.Precision(W(dt)):
            f = _objective(gold, dt)
            s = pxs.NLCG(f, show_progress=False)
            crit = pxst.MaxIter(int(gold["iters"])) | pxst.AbsError(eps=1e-30, var="gradient")
            s.fit(x0=R.to_dev(gold["x0"].astype(dt)), variant=str(gold["variant"]), restart_rate=int(gold["restart_rate"]),
                  a0=float(gold["a0"]), r=float(gold["r"]), c=float(gold["c"]), stop_crit=crit,
                  mode=pxa.Mode.MANUAL)
            a_k, gn = [], [np.linalg.norm(to_NUMPY(s._mstate["gradient"]).astype(np.float64), axis=-1)]
            for _ in s.steps():
                a_k.append(to_NUMPY(s._mstate["ls_a_k"]).reshape(-1))
                gn.append(np.linalg.norm(to_NUMPY(s._mstate["gradient"]).astype(np.float64), axis=-1))
            data, hist = s.stats()
            return s, np.array(a_k), np.array(gn), to_NUMPY(data["x"]), hist
    finally:
        nlcg_mod._FUSED = prev


_FITS = {}


def _fused_fit(name, d):
    if (name, d) not in _FITS:
        gold = load_golden(N.CASES[name][0])
        _FITS[name, d] = (gold, N.run_case(name, gold)) + _fit(gold, DT[d])[1:]
    return _FITS[name, d]


@pytest.mark.parametrize("name,d", TRAJ_CASES)
def test_trajectory(name, d):
    """12 iterations in MANUAL mode: every step size equals (T)a0 r^k of the restatement exactly; ||gradient||_2 (of
    the yielded gradients and in the AbsError[gradient] history) and the final x are within TRAJ_TOL, relative per row.

    T-PR in f32 rests on L1Norm.moreau_envelope forming its gradient as clip(x, -mu, mu) / mu: with the generic
    (x - prox(x)) / mu the f32 trajectory ends 4.0e-5 (||g||) / 2.8e-6 (x) from the float64 one, as the reference's
    own f32 run does (3.4e-5 / 2.8e-6), and misses the ||g|| bound (test_l1_moreau_gradient_has_no_cancellation)."""
    dt = DT[d]
    gold, ref, a_k, gn, x, hist = _fused_fit(name, d)
    assert x.dtype == dt and a_k.dtype == dt
    want_a = (dt(float(gold["a0"])) * dt(float(gold["r"])) ** ref["halvings"].astype(dt)).astype(dt)
    assert a_k.shape == want_a.shape
    assert np.array_equal(a_k, want_a), np.argwhere(a_k != want_a)
    eg = float(np.abs(gn / ref["gnorm"] - 1.0).max())
    ex = N.row_rel(x, ref["x"])
    # the AbsError[gradient] history (published sum g^2, no reduction by the criterion) holds the same norms
    h_min, h_max = np.asarray(hist["AbsError[gradient]_min"]), np.asarray(hist["AbsError[gradient]_max"])
    eh = max(float(np.abs(h_min / ref["gnorm"].min(axis=1) - 1.0).max()),
             float(np.abs(h_max / ref["gnorm"].max(axis=1) - 1.0).max()))
    print(name, d, "gnorm", eg, "x", ex, "history", eh)
    assert len(h_min) == int(gold["iters"]) + 1
    assert np.abs(h_min / gn.min(axis=1) - 1.0).max() <= 8 * R.eps(dt)  # ... of the yielded gradients themselves
    assert np.abs(h_max / gn.max(axis=1) - 1.0).max() <= 8 * R.eps(dt)
    assert ex <= TRAJ_TOL[dt]
    assert eg <= TRAJ_TOL[dt] and eh <= TRAJ_TOL[dt]


@pytest.mark.parametrize("name,d", TRAJ_CASES)
def test_fused_matches_chain(name, d):
    dt = DT[d]
    gold, ref, a_k, gn, x, hist = _fused_fit(name, d)
    _, a_c, gn_c, x_c, _ = _fit(gold, dt, fused=False)
    assert np.array_equal(a_k, a_c)
    err = N.row_rel(x, x_c)
    print(name, d, "fused vs chain", err)
    assert err <= FUSED_TOL[dt]


# ------------------------------------------------------------------------------------------------ direction kernels
NS = [1, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 65539]


def _direction_inputs(kind, shape, dt):
    """g1, g0, p (stack shape + (n,)) in T, and gg0 (float64): kind in FR / PR / PRclip / restart."""
    g1 = R.sum_values(shape, dt, 1)
    p = R.sum_values(shape, dt, 2)
    noise = R.sum_values(shape, dt, 3)
    scale = 1.5 if kind == "PRclip" else 0.5  # sum g1 (g1 - g0) = (1 - scale) sum g1^2 - 0.05 sum g1 noise
    g0 = (dt(scale) * g1 + dt(0.05) * noise).astype(dt)
    gg0 = (g0.astype(np.float64) ** 2).sum(axis=-1)
    return g1, g0, p, gg0


def _direction_run(kind, g1, g0, p, gg0):
    rows, n = int(np.prod(g1.shape[:-1])), g1.shape[-1]
    d = [R.to_dev(v).reshape(rows, n) for v in (g1, g0, p)]
    p_new = torch.full_like(d[2], R.GUARD)
    gg0_d = R.to_dev(gg0.reshape(-1))
    gg_out = torch.zeros_like(gg0_d)
    fb = _dev.HostFlagBuffer(rows, rows, rows)
    work = torch.zeros((int(_dev.lib.pxa_nlcg_workspace_bytes(rows)) // 8,), dtype=torch.float64, device="cuda")
    var = _dev.NLCG_FR if kind == "FR" else _dev.NLCG_PR
    seq = _dev.nlcg_direction(var, kind == "restart", d[0], d[1], d[2], p_new, gg0_d, gg_out, fb, work)
    fb.wait(seq)
    nb = _dev.nlcg_blocks(n)
    parts = R.to_host(_dev.nlcg_gp_partials(work, rows))[: rows * nb].reshape(rows, nb)
    return R.to_host(p_new), R.to_host(gg_out), fb.values.copy(), parts


def _direction_check(kind, shape, dt):
    g1, g0, p, gg0 = _direction_inputs(kind, shape, dt)
    n = shape[-1]
    got = _direction_run(kind, g1, g0, p, gg0)
    again = _direction_run(kind, g1, g0, p, gg0)
    for a, b in zip(got, again):  # fixed partition and order, no atomics: the same bits run to run
        assert np.array_equal(a, b)
    p_new, gg_dev, gg_host, parts = got
    G1, G0, P = (v.astype(np.float64).reshape(-1, n) for v in (g1, g0, p))
    u = (n + 4) * 2.0**-53
    gg_ref = (G1 * G1).sum(axis=-1)
    assert np.array_equal(gg_dev, gg_host)
    assert (np.abs(gg_dev - gg_ref) <= u * gg_ref).all()
    e = R.eps(dt)
    if kind in ("PRclip", "restart"):
        if kind == "PRclip":
            assert ((G1 * (g1 - g0).astype(np.float64).reshape(-1, n)).sum(axis=-1) < 0).all()
        assert np.array_equal(p_new, -g1.reshape(-1, n))  # beta == 0 exactly
    else:
        if kind == "FR":
            num, nabs = gg_ref, gg_ref
        else:
            t = G1 * (g1 - g0).astype(np.float64).reshape(-1, n)  # the difference in T, as the kernel forms it
            num, nabs = t.sum(axis=-1), np.abs(t).sum(axis=-1)
            assert (num > 0).all()
        beta = num / gg0.reshape(-1)
        dbeta = e * np.abs(beta) + 2 * u * nabs / gg0.reshape(-1)
        ref = beta[:, None] * P - G1
        bound = np.abs(P) * dbeta[:, None] + R.CHAIN_FACTOR * e * (np.abs(beta[:, None] * P) + np.abs(G1))
        assert (np.abs(p_new.astype(np.float64) - ref) <= bound).all()
    t = G1 * p_new.astype(np.float64)  # <g1, p_new> of the p_new the kernel wrote
    assert (np.abs(parts.sum(axis=-1) - t.sum(axis=-1)) <= u * np.abs(t).sum(axis=-1)).all()


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("n", NS)
def test_direction_kernels(n, d):
    for kind in ("FR", "PR", "PRclip", "restart"):
        for rows in (1, 3):
            _direction_check(kind, (rows, n), DT[d])


@pytest.mark.parametrize("d", list(DT))
def test_direction_kernels_stack(d):
    for kind in ("FR", "PR", "PRclip", "restart"):
        _direction_check(kind, (2, 3, 257), DT[d])


def test_direction_wrapper_rejects_bad_operands():
    g = torch.ones((2, 8), device="cuda")
    gg = torch.ones((2,), dtype=torch.float64, device="cuda")
    work = torch.zeros((int(_dev.lib.pxa_nlcg_workspace_bytes(2)) // 8,), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        _dev.nlcg_direction(_dev.NLCG_FR, False, g, None, g, g, gg, torch.zeros_like(gg), None, work)  # p_new aliases
    with pytest.raises(ValueError):
        _dev.nlcg_direction(_dev.NLCG_PR, False, g, None, g, torch.empty_like(g), gg, torch.zeros_like(gg), None, work)
    with pytest.raises(ValueError):
        _dev.nlcg_direction(_dev.NLCG_FR, False, g, None, g, torch.empty_like(g), gg, gg, None, work)  # gg_out is gg0
    with pytest.raises(ValueError):
        _dev.nlcg_direction(_dev.NLCG_FR, False, g, None, g, torch.empty_like(g), gg, torch.zeros_like(gg), None, work[:8])


# ------------------------------------------------------------------------------------------------ line search alone
def _q_search_setup(dt):
    gold = load_golden(N.CASES["Q-FR"][0])
    apply, grad = N.objective_Q(gold["A"], gold["b"])
    x0 = gold["x0"]
    return gold, apply, grad, x0, grad(x0)


@pytest.mark.parametrize("d", list(DT))
def test_linesearch_matches_restatement(d):
    dt = DT[d]
    gold, apply, grad, x0, g0 = _q_search_setup(dt)
    L = 2.0 * np.linalg.norm(gold["A"], 2) ** 2
    with pxrt.Precision(W(dt)):
        f = _objective(gold, dt)
        f.diff_lipschitz = L
        x, g = R.to_dev(x0.astype(dt)), R.to_dev(g0.astype(dt))
        p = R.to_dev((-g0).astype(dt))
        for a0 in (1.0, None):
            a0_ref = float(dt(1.0) / dt(L)) if a0 is None else a0  # coerce(1 / f.diff_lipschitz), in T
            margins = []
            a_ref, k_ref, _ = N.linesearch(apply, x0, -g0, g0, a0_ref, 0.5, 1e-4, margins=margins)
            assert min(margins) >= N.ARMIJO_MARGIN  # no decision of this search rests on rounding
            assert a0 is None or k_ref.max() >= 2  # (a0 = 1 backtracks; 1 / L is accepted at once)
            want = (dt(a0_ref) * dt(0.5) ** k_ref.astype(dt)).astype(dt).reshape(-1, 1)
            for grad_arg in (g, None):
                a = pxm.backtracking_linesearch(f, x, p, gradient=grad_arg, a0=a0, r=0.5, c=1e-4)
                assert tuple(a.shape) == (3, 1) and to_NUMPY(a).dtype == dt
                assert np.array_equal(to_NUMPY(a), want), (a0, grad_arg is None)


@pytest.mark.parametrize("d", list(DT))
def test_linesearch_ascent_direction_terminates(d):
    dt = DT[d]
    gold, apply, grad, x0, g0 = _q_search_setup(dt)
    with pxrt.Precision(W(dt)):
        f = _objective(gold, dt)
        a = to_NUMPY(pxm.backtracking_linesearch(f, R.to_dev(x0.astype(dt)), R.to_dev(g0.astype(dt)),
                                                 gradient=R.to_dev(g0.astype(dt)), a0=1.0))
    assert np.isfinite(a).all() and (a > 0).all() and (a <= 1.0).all()


@pytest.mark.parametrize("d", list(DT))
def test_linesearch_nan_row_keeps_a0(d):
    dt = DT[d]
    gold, apply, grad, x0, g0 = _q_search_setup(dt)
    with pxrt.Precision(W(dt)):
        f = _objective(gold, dt)
        p = R.to_dev((-g0).astype(dt))
        clean = to_NUMPY(pxm.backtracking_linesearch(f, R.to_dev(x0.astype(dt)), p, a0=1.0))
        xn = x0.astype(dt).copy()
        xn[1] = np.nan
        got = to_NUMPY(pxm.backtracking_linesearch(f, R.to_dev(xn), p, a0=1.0))
    assert got[1, 0] == dt(1.0)  # NaN on both sides of the test: not a failure, as in the reference
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    assert (clean < 1.0).any()


def test_linesearch_parameter_checks():
    gold, apply, grad, x0, g0 = _q_search_setup(np.float64)
    f = _objective(gold, np.float64)
    x, p = R.to_dev(x0), R.to_dev(-g0)
    for kw in (dict(r=0.0), dict(r=1.0), dict(c=0.0), dict(c=1.0), dict(a0=0.0), dict(a0=-1.0)):
        with pytest.raises(AssertionError):
            pxm.backtracking_linesearch(f, x, p, **{**dict(a0=1.0), **kw})


# ------------------------------------------------------------------------------------------------ the solver
def test_default_stop_crit():
    """Q-FR in float64 until the default AbsError(1e-4, var="gradient") fires (the reference needs 146 iterations)."""
    gold = load_golden(N.CASES["Q-FR"][0])
    with pxrt.Precision(pxrt.Width.DOUBLE):
        f = _objective(gold, np.float64)
        s = pxs.NLCG(f, show_progress=False)
        s.fit(x0=R.to_dev(gold["x0"]), variant="FR", restart_rate=5, a0=1.0, r=0.5, c=1e-4,
              stop_crit=pxst.MaxIter(1000) | s.default_stop_crit())
        x = to_NUMPY(s.solution())
    print("iterations", s._astate["idx"])
    assert 0 < s._astate["idx"] < 1000
    _, grad = N.objective_Q(gold["A"], gold["b"])
    assert (np.linalg.norm(grad(x.astype(np.float64)), axis=-1) <= 1e-4).all()
    best = np.linalg.lstsq(gold["A"], gold["b"], rcond=None)[0]
    assert N.row_rel(x, np.broadcast_to(best, x.shape)) <= 1e-3


@pytest.mark.parametrize("fused", [True, False])
def test_held_iterates_keep_their_values(fused):
    gold = load_golden(N.CASES["Q-PR"][0])
    names = ("x", "gradient", "conjugate_dir")
    prev = nlcg_mod._FUSED
    nlcg_mod._FUSED = fused
    try:
        with pxrt.Precision(pxrt.Width.SINGLE):
            f = _objective(gold, np.float32)
            s = pxs.NLCG(f, show_progress=False, log_var=names)
            s.fit(x0=R.to_dev(gold["x0"].astype(np.float32)), variant="PR", restart_rate=5, a0=0.35,
                  stop_crit=pxst.MaxIter(20), mode=pxa.Mode.MANUAL)
            it = s.steps()
            next(it)
            held = next(it)
            clones = {k: held[k].clone() for k in names}
            for _ in range(6):
                next(it)
            it.close()
    finally:
        nlcg_mod._FUSED = prev
    for k in names:
        assert torch.equal(held[k], clones[k]), k


def test_errors():
    gold = load_golden(N.CASES["Q-FR"][0])
    f = _objective(gold, np.float64)
    x0 = R.to_dev(gold["x0"])
    with pytest.raises(ValueError, match="Unsupported variant 'XX'"):
        pxs.NLCG(f, show_progress=False).fit(x0=x0, variant="XX", a0=1.0, stop_crit=pxst.MaxIter(1))
    msg = r"\[NLCG\] cannot auto-infer initial step size: specify `a0` manually in NLCG.fit\(\)"
    for dl in (np.inf, 0.0):
        f.diff_lipschitz = dl
        with pytest.raises(ValueError, match=msg):
            pxs.NLCG(f, show_progress=False).fit(x0=x0, stop_crit=pxst.MaxIter(1))


def test_long_rows_take_the_chain():
    """Rows of up to _FUSED_MAX_N entries run the two-launch direction update (64 partials per row here), longer
    ones the row-op chain, which measured faster there; both give the restatement's step sizes
    (f = ||x - y||^2 from a0 = 0.25: the first trial passes and halves the gradient) and the same x."""
    res = {}
    with pxrt.Precision(pxrt.Width.SINGLE):
        for n in (nlcg_mod._FUSED_MAX_N, nlcg_mod._FUSED_MAX_N + 1):
            y = R.to_dev(R.sum_values((n,), np.float32, 5))
            x0 = R.to_dev(R.sum_values((n,), np.float32, 6))
            s = pxs.NLCG(pxo.SquaredL2Norm(dim=n).asloss(y), show_progress=False)
            s.fit(x0=x0, variant="FR", a0=0.25, stop_crit=pxst.MaxIter(3))
            res[n] = (s._gp is not None, to_NUMPY(s._mstate["ls_a_k"]), to_NUMPY(s.solution()), to_NUMPY(y), to_NUMPY(x0))
    for n, (fused, a_k, x, y, x0) in res.items():
        assert fused == (n <= nlcg_mod._FUSED_MAX_N)
        assert a_k.shape == (1,) and a_k[0] == np.float32(0.25)
        # the float64 restatement on the same inputs
        apply, grad = (lambda v: ((v - y) ** 2).sum(axis=-1, keepdims=True)), (lambda v: 2.0 * (v - y))
        ref = N.nlcg(apply, grad, x0[None, :].astype(np.float64), "fr", n, 0.25, 0.5, 1e-4, 3)
        assert np.array_equal(ref["ls_a_k"], np.full((3, 1), 0.25))
        assert N.row_rel(x[None, :], ref["x"]) <= TRAJ_TOL[np.float32]


@pytest.mark.parametrize("d", list(DT))
def test_l1_moreau_gradient_has_no_cancellation(d):
    """grad of L1Norm.moreau_envelope(mu), the Huber function: x / mu in T where |x| <= mu, exactly +-1 beyond
    (the generic (x - prox(x)) / mu is off by up to ulp(x) / mu there), and apply is the Huber value."""
    dt = DT[d]
    mu = 0.05
    x = R.values(4099, dt, 9).reshape(1, -1)  # magnitudes in [1e-2, 1e2]: both regions
    x[0, :3] = [mu, -mu, 0.0]
    muT = dt(mu)
    with pxrt.Precision(W(dt)):
        env = pxo.L1Norm(dim=x.shape[-1]).moreau_envelope(mu)
        got = to_NUMPY(env.grad(R.to_dev(x)))
        val = to_NUMPY(env.apply(R.to_dev(x)))
    lin = np.abs(x) <= muT
    assert lin.sum() > 100 and (~lin).sum() > 100
    assert got.dtype == dt and np.array_equal(got[lin], (x / muT)[lin])
    assert np.array_equal(got[~lin], np.sign(x)[~lin])
    a = np.abs(x.astype(np.float64))
    huber = np.where(a <= mu, a * a / (2 * mu), a - mu / 2).sum()
    assert abs(float(val.reshape(-1)[0]) - huber) <= R.OP_TOL[dt] * huber
