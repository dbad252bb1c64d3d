"""
ProxAdam on the device (csrc/proxadam.hip, pyxu_amd/opt/solver/prox_adam.py) against the float64 NumPy restatement of
tests/_proxadam_refs.py, on the cases whose comparability conditions tests/test_proxadam_refs.py asserts, and the two
kernels alone at the edges of their partition.  The bounds are derived in the docstring of tests/_proxadam_refs.py.
"""
import warnings

import numpy as np
import pytest
from conftest import load_golden

import _prim_refs as R
import _proxadam_refs as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.solver.prox_adam as pa_mod  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.opt.solver.pgd import AutoInferenceWarning  # noqa: E402
from pyxu_amd.util import to_NUMPY  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
TRAJ_TOL = {np.float32: 1e-5, np.float64: 1e-10}  # test_gpu_parity.py
TRAJ_CASES = [(name, d) for name in P.CASES for d in DT if d == "f64" or P.CASES[name][1]]
KIND_CODE = {"l1": _dev.PROX_L1, "pos": _dev.PROX_POS, "posl1": _dev.PROX_POSL1, "box": _dev.PROX_BOX}
N, M = 17, 24


def W(dt):
    return pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE


def _g(kind, pw, n=N):
    if kind == "l1":
        return pw * pxo.L1Norm(dim=n)
    if kind == "pos":
        return pxo.PositiveOrthant(dim=n)
    if kind == "posl1":
        return pw * pxo.PositiveL1Norm(dim=n)
    if kind == "box":
        return pxo.LInfinityBall(dim=n, radius=pw)
    return None


def _objective(gold, dt):
    return pxo.SquaredL2Norm(dim=M).asloss(R.to_dev(gold["b"].astype(dt))) * pxa.LinOp.from_array(
        R.to_dev(gold["A"].astype(dt)))


def _fit(gold, dt, fused=True, lookahead=None, **over):
    """The golden's run on the device: (solver, final x, per-step sub-iteration counts (iters, rows))."""
    prev = pa_mod._FUSED, pa_mod._LOOKAHEAD
    pa_mod._FUSED = fused
    if lookahead is not None:
        pa_mod._LOOKAHEAD = lookahead
    try:
        with pxrt.Precision(W(dt)):
            kind = str(gold["g_kind"])
            s = pxs.ProxAdam(_objective(gold, dt), _g(kind, float(gold["g_pw"])), show_progress=False)
            kw = dict(variant=str(gold["variant"]), a=float(gold["a"]), b1=float(gold["b1"]), b2=float(gold["b2"]),
                      p=float(gold["p"]))
            if bool(gold["use_v0"]):
                kw["v0"] = R.to_dev(gold["v0"].astype(dt))
            kw.update(over)
            s.fit(x0=R.to_dev(gold["x0"].astype(dt)), stop_crit=pxst.MaxIter(int(gold["iters"])), mode=pxa.Mode.MANUAL,
                  **kw)
            counts = []
            for _ in s.steps():
                if s._sub_iters is not None:
                    counts.append(np.array(s._sub_iters))
            return s, to_NUMPY(s.solution()), np.array(counts, dtype=np.int64).reshape(-1, gold["x0"].shape[0])
    finally:
        pa_mod._FUSED, pa_mod._LOOKAHEAD = prev


_FITS = {}


def _fused_fit(name, d):
    if (name, d) not in _FITS:
        gold = load_golden(P.CASES[name][0])
        _FITS[name, d] = (gold, P.run_case(name, gold)) + _fit(gold, DT[d])[1:]
    return _FITS[name, d]


# ------------------------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize("name,d", TRAJ_CASES)
def test_trajectory(name, d):
    """6 iterations: the final x within TRAJ_TOL of the restatement, relative per row, and every row's sub-iteration
    count of every step equal to the restatement's."""
    dt = DT[d]
    gold, ref, x, counts = _fused_fit(name, d)
    err = P.row_rel(x, ref["x"])
    print(name, d, "x", err, "counts", counts.tolist())
    assert x.dtype == dt
    assert np.array_equal(counts, ref["counts"])
    assert err <= TRAJ_TOL[dt]


@pytest.mark.parametrize("name,d", TRAJ_CASES)
def test_fused_matches_fallback(name, d):
    """_FUSED = False: the chain of element-wise operations and the reference's per-row PGD construction."""
    dt = DT[d]
    gold, ref, x, counts = _fused_fit(name, d)
    _, x_c, counts_c = _fit(gold, dt, fused=False)
    err = P.row_rel(x, x_c)
    print(name, d, "fused vs fallback", err)
    assert np.array_equal(counts, counts_c)
    assert err <= TRAJ_TOL[dt]


@pytest.mark.parametrize("name", ["padam-posl1", "adam-l1"])
def test_fused_runs_repeat_bit_for_bit(name):
    gold, ref, x, counts = _fused_fit(name, "f32")
    for la in (None, 1):  # (the lookahead changes what the host waits for, never a value)
        _, x2, counts2 = _fit(gold, np.float32, lookahead=la)
        assert np.array_equal(x, x2) and np.array_equal(counts, counts2)


# ------------------------------------------------------------------------------------------------ the moment kernel
# (rows, n, element offset of every operand in its allocation)
MOM_SHAPES = [(1, 1, 0), (1, 3, 0), (3, 17, 0), (1, 4096, 0), (1, 4097, 0), (2, 8193, 0), (5, 4099, 1), (4097, 5, 0),
              (1, 2**20 + 3, 0)]
B1, B2, EPS_ADAM, EPS_VAR, A_STEP, T_STEP = 0.9, 0.999, 1e-6, 1e-6, 0.05, 3


def _mom_scalars(dt, p):
    """The scalars in T as the solver forms them on the host, as Python floats."""
    b1, b2 = dt(B1), dt(B2)
    return dict(b1=float(b1), omb1=float(1 - b1), b2=float(b2), omb2=float(1 - b2), eps_var=float(dt(EPS_VAR)),
                c1=float(1 - b1**T_STEP), c2=float(np.sqrt(1 - b2**T_STEP)), eps_adam=float(dt(EPS_ADAM)),
                a=float(dt(A_STEP)), p=float(dt(p)))


def _mom_inputs(rows, n, dt):
    g = R.sum_values((rows, n), dt, 11)
    m = R.sum_values((rows, n), dt, 12)
    v = np.abs(R.sum_values((rows, n), dt, 13))
    vh = np.abs(R.sum_values((rows, n), dt, 14))
    x = R.sum_values((rows, n), dt, 15)
    g[0, 0], v[0, 0] = 0, 0  # v_u = 0 < eps_var: the clip acts
    return g, m, v, vh, x


def _mom_run(variant, first, ins, sc, off=0, with_psi=True, inplace=False):
    """Launch on operands placed `off` elements into their allocations; returns (outputs m', v', vhat', x', psi as host
    arrays, psimax per row after pxa_proxadam_sub_init, whether inputs and guard elements are intact)."""
    rows, n = ins[0].shape
    bases, views = zip(*[R.placed(a, off) for a in ins])
    dev = [v.reshape(rows, n) for v in views]
    keep = [t.clone() for t in dev]
    nout = 5 if with_psi else 4
    obases, oviews = zip(*[R.placed(np.full((rows, n), R.GUARD, dtype=ins[0].dtype), off) for _ in range(nout)])
    outs = [v.reshape(rows, n) for v in oviews]
    if inplace:
        outs[0], outs[1], outs[2] = dev[1], dev[2], dev[3]
    work = _dev.proxadam_workspace(rows, n, dev[0]).zero_() if with_psi else None
    _dev.proxadam_moments(_dev.PROXADAM_VARIANTS[variant], first, dev[0], dev[1], dev[2], None if first else dev[3], dev[4],
                          outs[0], outs[1], outs[2], outs[3], psi_out=outs[4] if with_psi else None, work=work, **sc)
    psimax = None
    if with_psi:
        _dev.proxadam_sub_init(rows, n, work)
        psimax = R.to_host(_dev.proxadam_work_views(work, rows, n)[1])
    intact = all(R.guards_intact(b, off, rows * n) for b in bases + obases)
    if not inplace:
        intact = intact and all(torch.equal(a, b) for a, b in zip(dev, keep))
    return [R.to_host(o) for o in outs], psimax, intact


def _mom_check(variant, first, p, rows, n, off, dt):
    ins = _mom_inputs(rows, n, dt)
    sc = _mom_scalars(dt, p)
    outs, psimax, intact = _mom_run(variant, first, ins, sc, off)
    assert intact
    g, m, v, vh, x = (a.astype(np.float64) for a in ins)
    ref = P.moments(variant, T_STEP, first, g, m, v, vh, x, sc["a"], sc["b1"], sc["b2"], sc["p"], sc["eps_adam"],
                    sc["eps_var"], omb1=sc["omb1"], omb2=sc["omb2"], c1=sc["c1"], c2=sc["c2"])
    bounds = P.moments_bounds(dt, variant, g, m, v, x, ref, sc["a"], sc["b1"], sc["omb1"], sc["b2"], sc["omb2"], sc["c1"],
                              sc["p"])
    for name, got, want, bound in zip(("m", "v", "vhat", "x", "psi"), outs, ref[:5], bounds):
        assert got.dtype == dt
        bad = np.abs(got.astype(np.float64) - want) > bound
        assert not bad.any(), (variant, first, name, int(bad.sum()))
    assert outs[1][0, 0] == dt(EPS_VAR)
    # the folded maximum is the maximum of the psi the kernel stored, exactly
    assert np.array_equal(psimax, outs[4].astype(np.float64).max(axis=-1))
    return outs


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n,off", MOM_SHAPES)
def test_moments_kernel(rows, n, off, d):
    dt = DT[d]
    for variant, p in (("adam", 0.5), ("amsgrad", 0.5), ("padam", 0.25), ("padam", 0.5)):
        for first in (True, False):
            _mom_check(variant, first, p, rows, n, off, dt)


@pytest.mark.parametrize("d", list(DT))
def test_moments_in_place_and_without_psi(d):
    """m, v, vhat updated in place and no psi output: the same bits as the out-of-place launch."""
    dt = DT[d]
    ins, sc = _mom_inputs(3, 4099, dt), _mom_scalars(dt, 0.25)
    for variant in ("adam", "padam"):
        want, _, _ = _mom_run(variant, False, ins, sc)
        got, _, intact = _mom_run(variant, False, ins, sc, with_psi=False, inplace=True)
        assert intact
        for a, b in zip(got, want[:4]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n", [(1, 4097), (2, 8193), (1, 2**20 + 3)])
def test_psi_maximum_position(rows, n, d):
    """The maximum in the first element, in the last (tail) element and on either side of a workgroup boundary."""
    dt = DT[d]
    sc = _mom_scalars(dt, 0.5)
    c = P.chunk(dt, rows, n)
    assert P.blocks_per_row(rows, n) >= 2 and c < n
    for pos in (0, n - 1, c - 1, c):
        ins = _mom_inputs(rows, n, dt)
        ins[0][rows - 1, pos] = 40.0  # by far the largest gradient: the largest psi of the last row
        outs, psimax, _ = _mom_run("amsgrad", True, ins, sc)
        assert outs[4][rows - 1].argmax() == pos
        assert np.array_equal(psimax, outs[4].astype(np.float64).max(axis=-1))


@pytest.mark.parametrize("d", list(DT))
def test_moments_nan_gradient_entry(d):
    dt = DT[d]
    rows, n, at = 2, 4099, (1, 2051)
    ins, sc = _mom_inputs(rows, n, dt), _mom_scalars(dt, 0.25)
    ins[0][at] = np.nan
    for variant in ("adam", "amsgrad", "padam"):
        for first in (True, False):
            outs, _, _ = _mom_run(variant, first, ins, sc, with_psi=False)
            for got in outs[:4]:
                mask = np.isnan(got)
                assert mask[at] and mask.sum() == 1, (variant, first)


def test_moments_wrapper_rejects_bad_operands():
    t = torch.ones((2, 8), device="cuda")
    sc = _mom_scalars(np.float32, 0.5)
    new = lambda: torch.empty_like(t)  # noqa: E731
    with pytest.raises(ValueError):
        _dev.proxadam_moments(0, True, t, t, t, None, t, new(), new(), new(), t, **sc)  # x_out aliases x
    with pytest.raises(ValueError):
        _dev.proxadam_moments(0, False, t, t, t, None, t, new(), new(), new(), new(), **sc)  # vhat missing
    with pytest.raises(ValueError):
        _dev.proxadam_moments(3, True, t, t, t, None, t, new(), new(), new(), new(), **sc)  # variant
    with pytest.raises(ValueError):
        _dev.proxadam_moments(0, True, t, t, t, None, t, new(), new(), new(), new(), psi_out=new(), **sc)  # no workspace
    with pytest.raises(ValueError):
        _dev.proxadam_moments(0, True, t, t, t, None, t, new(), new(), new(), new().double(), **sc)  # dtype


# ------------------------------------------------------------------------------------------------ the sub-step kernel
SUB_SHAPES = [(1, 1, 0), (1, 3, 0), (3, 17, 0), (1, 4096, 0), (1, 4097, 0), (2, 8193, 0), (5, 4099, 1), (4097, 5, 0),
              (1, 2**20 + 3, 0)]
KIND_PW = {"l1": 0.3, "pos": 0.0, "posl1": 0.3, "box": 0.6}


def _sub_state(rows, n, psi_dev, running=True):
    """A workspace as pxa_proxadam_sub_init leaves it for `psi_dev`; with `running`, partials in both planes that fail
    the stop test (num = den)."""
    work = _dev.proxadam_workspace(rows, n, psi_dev).zero_()
    nb = _dev.proxadam_blocks(rows, n)
    _, psimax, state = _dev.proxadam_work_views(work, rows, n)
    psimax.copy_(psi_dev.double().amax(dim=1))
    if running:
        work[rows * nb: 5 * rows * nb] = 1.0
    return work, state


def _sub_inputs(rows, n, dt):
    xt = R.sum_values((rows, n), dt, 21)
    psi = np.abs(R.sum_values((rows, n), dt, 22))  # in [0.5, 1.5]
    z = (xt + dt(0.3) * R.sum_values((rows, n), dt, 23)).astype(dt)
    zp = (xt + dt(0.3) * R.sum_values((rows, n), dt, 24)).astype(dt)
    return xt, psi, zp, z


def _sub_launch(kind, k, ins, off, eps=1e-4, a=A_STEP, work=None):
    """One launch of sub-iteration k on fresh buffers: (z_new, out, work, state, running rows, guards intact)."""
    rows, n = ins[0].shape
    dt = ins[0].dtype.type
    bases, views = zip(*[R.placed(a_, off) for a_ in ins])
    xt, psi, zp, z = (v.reshape(rows, n) for v in views)
    obases, oviews = zip(*[R.placed(np.full((rows, n), R.GUARD, dtype=dt), off) for _ in range(2)])
    zn, out = (v.reshape(rows, n) for v in oviews)
    state = None
    if work is None:
        work, state = _sub_state(rows, n, psi)
    fb = _dev.HostFlagBuffer(1, 1, 1)
    mom = float(dt((k - 1) / (k + 75)))
    seq = _dev.proxadam_sub_step(KIND_CODE[kind], k, mom, eps, a, KIND_PW[kind], xt, psi, zp, z, zn, out, work, fb)
    nrun = _dev.proxadam_running(fb, seq)
    intact = all(R.guards_intact(b, off, rows * n) for b in bases + obases)
    return R.to_host(zn), R.to_host(out), work, state, nrun, intact


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n,off", SUB_SHAPES)
def test_sub_step_kernel(rows, n, off, d):
    """One launch (k = 3: momentum 2 / 78) against NumPy: z_new within its bound, the out buffer untouched, every
    row counted as running, the folded partials within the double-sum bound."""
    dt = DT[d]
    ins = _sub_inputs(rows, n, dt)
    k = 3
    for kind in P.KINDS:
        zn, out, work, state, nrun, intact = _sub_launch(kind, k, ins, off)
        assert intact and nrun == rows
        assert (out == dt(R.GUARD)).all() and (R.to_host(state) == 0).all()
        want, bound, _ = P.sub_step_ref(dt, kind, KIND_PW[kind], (k - 1) / (k + 75), A_STEP, *ins)
        bad = np.abs(zn.astype(np.float64) - want) > bound
        assert not bad.any(), (kind, int(bad.sum()))
        parts = R.to_host(_dev.proxadam_stat_partials(work, rows, n, k)).sum(axis=-1)
        z64, zn64 = ins[3].astype(np.float64), zn.astype(np.float64)
        u = (n + 4) * 2.0**-53
        for got, t in zip(parts, ((zn64 - z64) ** 2, z64**2)):
            assert (np.abs(got - t.sum(axis=-1)) <= u * t.sum(axis=-1)).all(), kind


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("kind", ["l1", "posl1", "box"])
def test_sub_step_is_exact_where_psi_is_its_maximum(kind, d):
    """psi == psimax everywhere: w = xt exactly whatever z and z_prev are, so z_new is the prox of xt bit for bit and
    inputs at +-threshold and 0 land in the same support set."""
    dt = DT[d]
    rows, n = 2, 4099
    xt, _, zp, z = _sub_inputs(rows, n, dt)
    psi = np.full((rows, n), 1.25, dtype=dt)
    _, _, thr = P.sub_step_ref(dt, kind, KIND_PW[kind], 0.0, A_STEP, xt, psi, zp, z)
    t = thr[0, 0]
    xt[:, :8] = [t, -t, 0.0, np.nextafter(t, dt(np.inf)), np.nextafter(t, dt(0)), -np.nextafter(t, dt(np.inf)),
                 -np.nextafter(t, dt(0)), 2 * t]
    xt[:, -3:] = [t, -t, 0.0]  # (the scalar tail)
    zn, _, _, _, nrun, intact = _sub_launch(kind, 3, (xt, psi, zp, z), 0)
    if kind == "l1":
        want = np.sign(xt) * np.maximum(np.abs(xt) - t, dt(0))
    elif kind == "posl1":
        want = np.clip(xt + (-t), dt(0), None)
    else:
        want = np.clip(xt, -t, t)
    assert intact and nrun == rows
    assert np.array_equal(zn, want.astype(dt))
    assert np.array_equal(zn != 0, want != 0)


def _drive(kind, rows, n, dt, eps, lookahead_extra=2):
    """The whole sub-solve through the kernels with every z_k kept on the host."""
    xt = R.sum_values((rows, n), dt, 31)
    spread = np.array([0.0, 1.0, 20.0, 200.0])[np.arange(rows) % 4].reshape(rows, 1)  # rows of unequal conditioning
    u = R.rng_for("drive", rows, n).uniform(0.0, 1.0, (rows, n))
    psi = (1.0 + spread * u).astype(dt)
    xt_d, psi_d = R.to_dev(xt), R.to_dev(psi)
    work = _dev.proxadam_workspace(rows, n, xt_d).zero_()
    # the psi maxima as pxa_proxadam_moments leaves them: through the kernel path, from a launch that reproduces psi
    nb = _dev.proxadam_blocks(rows, n)
    c = P.chunk(dt, rows, n)
    pm = np.full((rows, nb), -np.inf)
    for b in range(nb):
        if b * c < n:
            pm[:, b] = psi[:, b * c: (b + 1) * c].astype(np.float64).max(axis=-1)
    _dev.proxadam_work_views(work, rows, n)[0].copy_(R.to_dev(pm))
    _dev.proxadam_sub_init(rows, n, work)
    _, psimax, state = _dev.proxadam_work_views(work, rows, n)
    assert np.array_equal(R.to_host(psimax), psi.astype(np.float64).max(axis=-1))
    zs = [torch.full_like(xt_d, R.GUARD) for _ in range(3)]
    out = torch.full_like(xt_d, R.GUARD)
    fb = _dev.HostFlagBuffer(1, 1, 1)
    hist, nruns, k = [xt], [], 0
    while True:
        k += 1
        assert k < 2000
        if k == 1:
            zp_, z_, zn_ = xt_d, xt_d, zs[0]
        elif k == 2:
            zp_, z_, zn_ = xt_d, zs[0], zs[1]
        else:
            zp_, z_, zn_ = zs[(k - 3) % 3], zs[(k - 2) % 3], zs[(k - 1) % 3]
        mom = float(dt((k - 1) / (k + 75)))
        seq = _dev.proxadam_sub_step(KIND_CODE[kind], k, mom, eps, A_STEP, KIND_PW[kind], xt_d, psi_d, zp_, z_, zn_, out,
                                     work, fb)
        nruns.append(_dev.proxadam_running(fb, seq))
        hist.append(R.to_host(zn_))  # (rows frozen by now hold stale values there: never looked at below)
        if nruns[-1] == 0:
            break
    snap = [t.clone() for t in zs + [out, work]]
    for extra in range(lookahead_extra):  # launches after every row froze: nothing changes
        k += 1
        zp_, z_, zn_ = zs[(k - 3) % 3], zs[(k - 2) % 3], zs[(k - 1) % 3]
        seq = _dev.proxadam_sub_step(KIND_CODE[kind], k, 0.5, eps, A_STEP, KIND_PW[kind], xt_d, psi_d, zp_, z_, zn_, out,
                                     work, fb)
        assert _dev.proxadam_running(fb, seq) == 0
    assert all(torch.equal(a, b) for a, b in zip(snap, zs + [out, work]))
    return hist, nruns, R.to_host(state), R.to_host(out)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("rows,n", [(3, 17), (4, 4097), (2, 8193), (4097, 5)])
def test_rows_freeze_at_their_own_launch(rows, n, d):
    """Driven to the end: a row's state word holds the launch k that saw ||z_{k-1} - z_{k-2}|| <= eps ||z_{k-2}|| (and
    no earlier launch did, decisions within 1e-6 of the threshold aside), its row of the output buffer is z_{k-1} bit
    for bit, the host word is the number of rows still running and counts down to 0, and further launches change
    nothing."""
    dt = DT[d]
    eps = 1e-3
    hist, nruns, state, out = _drive("l1", rows, n, dt, eps)
    assert (state >= 2).all() and nruns[-1] == 0
    assert len(np.unique(state)) > 1  # rows freeze at different launches
    want_run = [(state > k).sum() for k in range(1, len(nruns) + 1)]
    assert nruns == want_run and all(a >= b for a, b in zip(nruns, nruns[1:]))
    z = [h.astype(np.float64) for h in hist]
    for r in range(min(rows, 64)):  # (every row's solution below; the decisions of the first 64 rows)
        kr = int(state[r])
        for k in range(2, kr + 1):
            num = np.linalg.norm(z[k - 1][r] - z[k - 2][r])
            den = np.linalg.norm(z[k - 2][r])
            if abs(num / (eps * den) - 1.0) > 1e-6:
                assert (num <= eps * den) == (k == kr), (r, k, kr)
    for r in range(rows):
        assert np.array_equal(out[r], hist[int(state[r]) - 1][r]), r


def test_sub_step_wrapper_rejects_bad_operands():
    t = torch.ones((2, 8), device="cuda")
    work, _ = _sub_state(2, 8, t)
    fb = _dev.HostFlagBuffer(1, 1, 1)
    new = lambda: torch.empty_like(t)  # noqa: E731
    with pytest.raises(ValueError):
        _dev.proxadam_sub_step(1, 1, 0.0, 1e-4, 0.05, 0.1, t, t, t, t, t, new(), work, fb)  # z_new aliases
    with pytest.raises(ValueError):
        _dev.proxadam_sub_step(1, 1, 0.0, 1e-4, 0.05, 0.1, t, t, t, t, new(), t, work, fb)  # out aliases
    with pytest.raises(ValueError):
        _dev.proxadam_sub_step(5, 1, 0.0, 1e-4, 0.05, 0.1, t, t, t, t, new(), new(), work, fb)  # kind
    with pytest.raises(ValueError):
        _dev.proxadam_sub_step(1, 0, 0.0, 1e-4, 0.05, 0.1, t, t, t, t, new(), new(), work, fb)  # k
    with pytest.raises(ValueError):
        _dev.proxadam_sub_step(1, 1, 0.0, 1e-4, 0.05, 0.1, t, t, t, t, new(), new(), work[:4], fb)  # workspace


# ------------------------------------------------------------------------------------------------ the interface
def _q(dt=np.float64):
    gold = load_golden(P.CASES["ams-l1-v0"][0])
    return gold, _objective(gold, dt), R.to_dev(gold["x0"].astype(dt))


def test_errors():
    gold, f, x0 = _q()
    fit = lambda **kw: pxs.ProxAdam(f, show_progress=False).fit(x0=x0, stop_crit=pxst.MaxIter(1), **{"a": 0.05, **kw})  # noqa: E731
    with pytest.raises(ValueError, match="Unsupported variant 'XX'"):
        fit(variant="XX")
    for a in (0.0, -1.0, "abc"):
        with pytest.raises(ValueError, match="`a` must be positive"):
            fit(a=a)
    for kw, msg in ((dict(p=0.0), r"p: expected value in \(0, 0.5\], got"), (dict(p=0.6), r"p: expected value in \(0, 0.5\]"),
                    (dict(b1=1.0), r"b1: expected value in \[0, 1\), got"), (dict(b1=-0.1), r"b1: expected value in \[0, 1\)"),
                    (dict(b2=1.0), r"b2: expected value in \[0, 1\), got"), (dict(b2=-0.1), r"b2: expected value in \[0, 1\)"),
                    (dict(eps_adam=0.0), "eps_adam: expected positive value, got"),
                    (dict(eps_var=0.0), "eps_var: expected positive value, got")):
        with pytest.raises(AssertionError, match=msg):
            fit(**kw)


def test_state_keys_and_defaults():
    gold, f, x0 = _q()
    s = pxs.ProxAdam(f, _g("l1", 0.1), show_progress=False)
    s.fit(x0=x0, a=0.05, stop_crit=pxst.MaxIter(1))
    assert set(s._mstate) >= {"x", "a", "variant", "padam_p", "eps_adam", "mean", "variance", "variance_hat", "b1", "b2",
                              "eps_variance", "subproblem_init_kwargs", "subproblem_stop_crit"}
    assert s._astate["log_var"] == frozenset({"x"}) and s._mstate["variant"] == "adam"
    crit = s.default_stop_crit()
    assert type(crit) is pxst.RelError and crit._eps == 1e-4 and crit._var == "x"
    assert tuple(s.objective_func().shape) == (3, 1)


@pytest.mark.parametrize("fused", [True, False])
def test_inputs_are_not_mutated_and_moments_broadcast(fused):
    gold, f, x0 = _q(np.float64)
    ref = P.proxadam(P.objective_Q(gold["A"], gold["b"]), gold["x0"], "amsgrad", 0.05, 3, m0=gold["v0"][1] - 1.0,
                     v0=gold["v0"][0], g=("l1", 0.1))
    prev = pa_mod._FUSED
    pa_mod._FUSED = fused
    try:
        with pxrt.Precision(pxrt.Width.DOUBLE):
            m0 = R.to_dev((gold["v0"][1] - 1.0).astype(np.float64))  # (n,): broadcast over the rows
            v0 = R.to_dev(gold["v0"][0].astype(np.float64))
            keep = [t.clone() for t in (x0, m0, v0)]
            s = pxs.ProxAdam(f, _g("l1", 0.1), show_progress=False)
            s.fit(x0=x0, variant="amsgrad", a=0.05, m0=m0, v0=v0, stop_crit=pxst.MaxIter(3))
            x = to_NUMPY(s.solution())
    finally:
        pa_mod._FUSED = prev
    for a, b in zip((x0, m0, v0), keep):
        assert torch.equal(a, b)
    assert tuple(s._mstate["mean"].shape) == (3, N)
    assert P.row_rel(x, ref["x"]) <= TRAJ_TOL[np.float64]


@pytest.mark.parametrize("fused", [True, False])
def test_held_iterates_keep_their_values(fused):
    gold, f, x0 = _q(np.float32)
    names = ("x", "mean", "variance", "variance_hat")
    prev = pa_mod._FUSED
    pa_mod._FUSED = fused
    try:
        with pxrt.Precision(pxrt.Width.SINGLE):
            for g in (_g("l1", 0.1), None):
                s = pxs.ProxAdam(f, g, show_progress=False, log_var=names)
                s.fit(x0=x0, variant="amsgrad", a=0.05, stop_crit=pxst.MaxIter(8), mode=pxa.Mode.MANUAL)
                it = s.steps()
                first = next(it)
                clones = {k: first[k].clone() for k in names}
                held = next(it)
                clones2 = {k: held[k].clone() for k in names}
                for _ in range(4):
                    next(it)
                it.close()
                for k in names:
                    assert torch.equal(first[k], clones[k]) and torch.equal(held[k], clones2[k]), k
    finally:
        pa_mod._FUSED = prev


def test_step_size_defaults():
    gold, f, x0 = _q()
    L = 2.0 * np.linalg.norm(gold["A"], 2) ** 2
    f.diff_lipschitz = L
    s = pxs.ProxAdam(f, show_progress=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", AutoInferenceWarning)
        s.fit(x0=x0, stop_crit=pxst.MaxIter(1))
    assert float(s._mstate["a"]) == 1.0 / L
    f.diff_lipschitz = np.inf
    s = pxs.ProxAdam(f, show_progress=False)
    with pytest.warns(AutoInferenceWarning, match="auto-set to 1"):
        s.fit(x0=x0, stop_crit=pxst.MaxIter(1))
    assert float(s._mstate["a"]) == 1.0


def test_docstring_example_takes_the_fallback():
    """min ||x - 1||_2^2 + ||x - 1||_1 from zeros(3) (prox_adam.py:200-227): g built with asloss is not one of the four
    element-wise kinds, so the sub-problems run the per-row PGD."""
    n = 3
    with pxrt.Precision(pxrt.Width.DOUBLE):
        f = pxo.SquaredL2Norm(dim=n).asloss(1)
        g = pxo.L1Norm(dim=n).asloss(1)
        s = pxs.ProxAdam(f, g, show_progress=False)
        s.fit(x0=torch.zeros((n,), dtype=torch.float64, device="cuda"), variant="padam", p=0.25)
        assert s._sub_plan(1, n) is None and s._sub_iters is not None
        x = to_NUMPY(s.solution())
    print("iterations", s._astate["idx"], x)
    assert np.allclose(x, 1)


def test_custom_sub_stop_criterion_takes_the_fallback():
    gold = load_golden(P.CASES["padam-l1"][0])
    ref = P.run_case("padam-l1", gold, sub_max_iter=4)
    s, x, counts = _fit(gold, np.float64, stop_crit_sub=pxst.MaxIter(4))
    assert s._sub_plan(3, N) is None
    assert (counts == 4).all() and np.array_equal(counts, ref["counts"])
    assert P.row_rel(x, ref["x"]) <= TRAJ_TOL[np.float64]
    s, _, _ = _fit(gold, np.float64, kwargs_sub=dict(verbosity=100))
    assert s._sub_plan(3, N) is None
    s, _, _ = _fit(gold, np.float64, stop_crit_sub=pxst.RelError(eps=1e-4, var="x", norm=1))
    assert s._sub_plan(3, N) is None
    s, _, _ = _fit(gold, np.float64, stop_crit_sub=pxst.RelError(eps=1e-3, var="x"))
    assert s._sub_plan(3, N) == (_dev.PROX_L1, 0.1, 1e-3)
