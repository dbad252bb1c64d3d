"""
The fused PGD, Condat-Vu and PD3O steps write into iterates that have left the solver state instead of allocating
(opt/solver/_recycle.py), but never into an array something else can still reach.  The reference allocates every
iterate, so whatever a user holds keeps its values there.  Here, on the smallest shapes that take the fused paths
(PGD: one 32 x 64 tile plus edge tiles; PDS: one march with a halo), under every stop-check engine / look-ahead mode:

* held arrays keep their values: x0 (z0), also as rows of a larger user tensor, the x / z of steps() items, a slice
  view and a to_dlpack capsule of two of them whose items were dropped, the x of a stats() call;
* the result does not depend on reuse: a run that keeps every steps() item alive (nothing can be recycled) and one
  that keeps none end in the same bits;
* reuse is on: the number of _dev.empty_like calls over a window of steps with nothing held is the one measured with
  this file on the commit before the recycler (d1eff09).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from torch.utils.dlpack import from_dlpack, to_dlpack  # noqa: E402

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device  # noqa: E402

from test_gpu_pds_fused import _problem as _pds_problem  # noqa: E402

# ---------------------------------------------------------------------------------------------------------- engines
# (the class attributes test_gpu_solver_lag._engine patches)
ENGINES = {
    "sync": dict(lag=0, spec=False, stop_rate=1),
    "spec_sr1": dict(lag=0, spec=True, stop_rate=1),
    "spec_sr3": dict(lag=0, spec=True, stop_rate=3),
    "lag_window_pub": dict(lag=8, spec=True, stop_rate=1, window=True, pub=True),
    "lag_window_fold_launch": dict(lag=8, spec=True, stop_rate=1, window=True, pub=False),
    "lag_epilogue": dict(lag=8, spec=True, stop_rate=1, window=False, pub=True),
}


def _engine(name, monkeypatch):
    e = ENGINES[name]
    monkeypatch.setattr(pxa.Solver, "_LAG", e["lag"])
    monkeypatch.setattr(pxa.Solver, "_LAG_INKERNEL", False)
    monkeypatch.setattr(pxa.Solver, "_LAG_WINDOW", e.get("window", True))
    monkeypatch.setattr(pxs.PGD, "_LAG_PUB", e.get("pub", True))
    if not e["spec"]:
        monkeypatch.setattr(pxs.PGD, "_spec_supported", lambda self: False)
    return e


class _Held:
    """Arrays a user keeps, each with a clone taken when it was taken."""

    def __init__(self):
        self.kept = []

    def keep(self, what, t):
        self.kept.append((what, t, t.clone()))

    def keep_capsule(self, what, t):
        self.kept.append((what, to_dlpack(t), t.clone()))

    def check(self):
        assert len(self.kept) > 0
        for what, t, clone in self.kept:
            if not isinstance(t, torch.Tensor):
                t = from_dlpack(t)
            assert torch.equal(t, clone), what


def _march(s, n, held, take, stats_at, log_var):
    """n items of s.steps().  At the three steps of `take` the item's arrays are kept: the first as they are, of the
    second only a slice view, of the third only a to_dlpack capsule; at `stats_at` the x of stats()."""
    it = s.steps()
    for k in range(n):
        item = next(it)
        if k == take[0]:
            for v in log_var:
                held.keep(f"steps() item {k} {v}", item[v])
        elif k == take[1]:
            for v in log_var:
                held.keep(f"slice view of steps() item {k} {v}", item[v][..., 5:-3])
        elif k == take[2]:
            for v in log_var:
                held.keep_capsule(f"to_dlpack capsule of steps() item {k} {v}", item[v])
        if k == stats_at:
            held.keep(f"stats() x after item {k}", s.stats()[0]["x"])
        del item
    it.close()


def _row_of_big(t):
    """`t` as row 1 of a larger user tensor: (the tensor, the row)."""
    big = torch.rand((3, *t.shape), dtype=t.dtype, device=t.device)
    big[1] = t
    return big, big[1]


class _Count:
    def __init__(self, monkeypatch):
        self.n = 0
        inner = _dev.empty_like

        def counted(*a, **k):
            self.n += 1
            return inner(*a, **k)

        monkeypatch.setattr(_dev, "empty_like", counted)


# -------------------------------------------------------------------------------------------------------------- PGD
PGD_SHAPE, PGD_STEPS = (40, 72), 30


def _pgd_problem(stack):
    """fp32 TV deblurring, Gaussian sigma 1, PositiveOrthant; stack 2 in the batch-as-axis form of
    test_gpu_solver_lag._problem."""
    sh = PGD_SHAPE
    N = stack * int(np.prod(sh))
    lam, mu = 0.02, 0.01
    y = np.random.default_rng(3).standard_normal(N).astype(np.float32)
    if stack == 1:
        H = pxo.Gaussian(arg_shape=sh, sigma=1.0)
        G = pxo.Gradient(arg_shape=sh)
        l21 = pxo.L21Norm(arg_shape=(2, *sh))
    else:
        H = pxo.Gaussian(arg_shape=(stack, *sh), sigma=(0, 1.0, 1.0))
        G = pxo.Gradient(arg_shape=(stack, *sh), directions=(1, 2))
        l21 = pxo.L21Norm(arg_shape=(2, stack, *sh))
    f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(y)) * H + lam * l21.moreau_envelope(mu) * G
    f.diff_lipschitz = 1 + 8 * lam / mu
    return f, pxo.PositiveOrthant(dim=N), N


def _pgd_fit(engine, stack, x0, tmp_path, tag):
    f, g, _ = _pgd_problem(stack)
    s = pxs.PGD(f=f, g=g, show_progress=False, stop_rate=engine["stop_rate"], folder=tmp_path / tag)
    s.fit(x0=x0, stop_crit=pxst.MaxIter(10 ** 6) | pxst.RelError(eps=1e-30), mode=pxa.Mode.MANUAL)
    assert s._plan is not None, "fused path not selected"
    assert (s._lag_plan() is not None) == (engine["lag"] > 0)
    assert s._spec_supported() == engine["spec"]
    return s


def _pgd_x0(stack):
    N = stack * int(np.prod(PGD_SHAPE))
    return to_device(np.random.default_rng(7).uniform(0, 1, N).astype(np.float32))


@pytest.mark.parametrize("x0_form", ["own", "row_of_big"])
@pytest.mark.parametrize("stack", [1, 2])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_pgd_held_arrays_keep_their_values(engine, stack, x0_form, monkeypatch, tmp_path):
    e = _engine(engine, monkeypatch)
    held = _Held()
    with pxrt.Precision(pxrt.Width.SINGLE):
        x0 = _pgd_x0(stack)
        if x0_form == "row_of_big":
            big, x0 = _row_of_big(x0)
            held.keep("big", big)
        held.keep("x0", x0)
        s = _pgd_fit(e, stack, x0, tmp_path, "held")
        _march(s, PGD_STEPS, held, take=(4, 9, 14), stats_at=19, log_var=("x",))
        torch.cuda.synchronize()
    held.check()


@pytest.mark.parametrize("stack", [1, 2])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_pgd_result_does_not_depend_on_reuse(engine, stack, monkeypatch, tmp_path):
    e = _engine(engine, monkeypatch)
    out = {}
    with pxrt.Precision(pxrt.Width.SINGLE):
        for keep_all in (True, False):
            s = _pgd_fit(e, stack, _pgd_x0(stack), tmp_path, f"keep{keep_all}")
            it = s.steps()
            items = [next(it) for _ in range(PGD_STEPS)] if keep_all else None
            if not keep_all:
                for _ in range(PGD_STEPS):
                    next(it)
            it.close()
            assert s._astate["idx"] == PGD_STEPS
            out[keep_all] = s._mstate["x"].clone()
            del items
    assert torch.equal(out[True], out[False])


# _dev.empty_like calls over steps 6 .. 25 with nothing held, measured with this test on d1eff09 (the commit before
# opt/solver/_recycle.py): the same for both stacks
PGD_ALLOCS = {
    "sync": 0,
    "spec_sr1": 0,
    "spec_sr3": 6,  # (the x a stop check saw is kept for the next check's RelError: still held when it is retired)
    "lag_window_pub": 0,  # (the pool)
    "lag_window_fold_launch": 0,
    "lag_epilogue": 20,  # (the epilogue steps do not pool what they retire)
}


@pytest.mark.parametrize("stack", [1, 2])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_pgd_allocations_per_step_are_the_parents(engine, stack, monkeypatch, tmp_path):
    e = _engine(engine, monkeypatch)
    with pxrt.Precision(pxrt.Width.SINGLE):
        s = _pgd_fit(e, stack, _pgd_x0(stack), tmp_path, "allocs")
        it = s.steps()
        for _ in range(6):
            next(it)
        count = _Count(monkeypatch)
        for _ in range(6, 26):
            next(it)
        n = count.n
        it.close()
    print(f"PGD {engine} stack {stack}: {n} empty_like calls over steps 6..25")
    assert n == PGD_ALLOCS[engine]


# -------------------------------------------------------------------------------------------- Condat-Vu and PD3O
PDS_ALGOS = {"pd3o": pxs.PD3O, "cv": pxs.CondatVu}
PDS_STEPS = 12
PDS_CASES = {  # shape, sigma, rows of the start (None: a single (N,) start)
    "6x9x11": ((6, 9, 11), 0.8, None),
    "9x20x36-s2": ((9, 20, 36), 1.0, 2),
}


def _pds_fit(algo, case, lookahead, x0, z0):
    sh, sigma, _ = PDS_CASES[case]
    f, g, h, K, _ = _pds_problem(sh, sigma, "l1", "none", np.float32)
    s = PDS_ALGOS[algo](f=f, g=g, h=h, K=K, show_progress=False)
    s._LOOKAHEAD = lookahead
    s.fit(x0=x0, z0=z0 if z0 is not None else K(x0), stop_crit=pxst.MaxIter(10 ** 6), mode=pxa.Mode.MANUAL)
    assert s._plan is not None and s._plan["la"] == lookahead, "fused path / look-ahead not as asked"
    return s


def _pds_x0(case):
    sh, _, rows = PDS_CASES[case]
    N = int(np.prod(sh))
    shape = (N,) if rows is None else (rows, N)
    return to_device(np.random.default_rng(4).uniform(0, 1, shape).astype(np.float32))


def _pds_z0(case, x0):
    sh, sigma, _ = PDS_CASES[case]
    return _pds_problem(sh, sigma, "l1", "none", np.float32)[3](x0)


@pytest.mark.parametrize("x0_form", ["own", "row_of_big"])
@pytest.mark.parametrize("lookahead", [True, False], ids=["lookahead", "three_launch"])
@pytest.mark.parametrize("case", list(PDS_CASES))
@pytest.mark.parametrize("algo", list(PDS_ALGOS))
def test_pds_held_arrays_keep_their_values(algo, case, lookahead, x0_form, tmp_path):
    held = _Held()
    with pxrt.Precision(pxrt.Width.SINGLE):
        x0 = _pds_x0(case)
        z0 = _pds_z0(case, x0)
        if x0_form == "row_of_big":
            xbig, x0 = _row_of_big(x0)
            zbig, z0 = _row_of_big(z0)
            held.keep("big of x0", xbig)
            held.keep("big of z0", zbig)
        held.keep("x0", x0)
        held.keep("z0", z0)
        s = _pds_fit(algo, case, lookahead, x0, z0)
        _march(s, PDS_STEPS, held, take=(1, 4, 7), stats_at=9, log_var=("x", "z"))
        torch.cuda.synchronize()
    held.check()


@pytest.mark.parametrize("lookahead", [True, False], ids=["lookahead", "three_launch"])
@pytest.mark.parametrize("case", list(PDS_CASES))
@pytest.mark.parametrize("algo", list(PDS_ALGOS))
def test_pds_result_does_not_depend_on_reuse(algo, case, lookahead):
    out = {}
    with pxrt.Precision(pxrt.Width.SINGLE):
        for keep_all in (True, False):
            s = _pds_fit(algo, case, lookahead, _pds_x0(case), None)
            it = s.steps()
            items = [next(it) for _ in range(PDS_STEPS)] if keep_all else None
            if not keep_all:
                for _ in range(PDS_STEPS):
                    next(it)
            it.close()
            out[keep_all] = {k: v.clone() for k, v in s._mstate.items() if k in ("x", "u", "z")}
            del items
    assert set(out[True]) == set(out[False]) >= {"x", "z"}
    for k in out[True]:
        assert torch.equal(out[True][k], out[False][k]), k


# _dev.empty_like calls over steps 4 .. 11 with nothing held, measured with this test on d1eff09: the same for both
# cases.  Per step: the look-ahead steps reuse the retired x and z; PD3O's u, and every output of the three-launch steps
# but Condat-Vu's x, are new arrays
PDS_ALLOCS = {
    ("pd3o", True): 8,
    ("pd3o", False): 24,
    ("cv", True): 0,
    ("cv", False): 8,
}


@pytest.mark.parametrize("lookahead", [True, False], ids=["lookahead", "three_launch"])
@pytest.mark.parametrize("case", list(PDS_CASES))
@pytest.mark.parametrize("algo", list(PDS_ALGOS))
def test_pds_allocations_per_step_are_the_parents(algo, case, lookahead, monkeypatch):
    with pxrt.Precision(pxrt.Width.SINGLE):
        s = _pds_fit(algo, case, lookahead, _pds_x0(case), None)
        it = s.steps()
        for _ in range(4):
            next(it)
        count = _Count(monkeypatch)
        for _ in range(4, 12):
            next(it)
        n = count.n
        it.close()
    print(f"PDS {algo} {case} lookahead {lookahead}: {n} empty_like calls over steps 4..11")
    assert n == PDS_ALLOCS[(algo, lookahead)]
