"""
Lagged stop checks (abc/solver.py _lag_loop; VERDICT r05 Next #2): at stop_rate 1 the fused PGD solver keeps up to
_LAG RelError checks unresolved while the device runs ahead, and ends in the state of the check that fired.  Against
the synchronous reference order (solver.py:588-663, stop.py:353-382) on the same problem: the same stop iteration,
the same iterate bit for bit, the same history records (MaxIter counts checks), the same steps() items, also when
steps() is consumed in pieces, and the same log lines.  With the default window statistics (the next step's
(x, x_prev) loads: the same sums in another order) the RelError values agree to 1e-12 relative instead of bit for
bit; with the epilogue statistics they are bit-identical.  The criterion ends as on the synchronous path too (info()
is the last history record, the RelError leaf keeps the solution tensor), and nothing of a run survives it: the same
solver and criterion objects fitted again, or the criterion reused elsewhere, give a fresh object's result.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

import _asym_cases as ac  # noqa: E402


def _problem(sh=(96, 128), stack=1, entry=None):
    rng = np.random.default_rng(3)
    lam, mu = 0.02, 0.01
    if entry is not None:  # an entry of tests/_asym_cases.py: asymmetric per-axis taps, per-axis sampling
        sh = entry.shape
        N = int(np.prod(sh))
        y = rng.standard_normal(N).astype(np.float32)
        H = pxo.Stencil(arg_shape=sh, kernel=ac.kernels(entry, np.float32), center=list(entry.centers), mode="constant")
        G = pxo.Gradient(arg_shape=sh, sampling=entry.sampling)
        f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(y)) * H + lam * pxo.L21Norm(arg_shape=(2, *sh)).moreau_envelope(mu) * G
        f.diff_lipschitz = 1 + 4 * lam / mu * sum(1 / h ** 2 for h in entry.sampling)
        return f, pxo.PositiveOrthant(dim=N), N
    N = int(np.prod(sh))
    y = rng.standard_normal(stack * N).astype(np.float32)
    if stack == 1:
        H = pxo.Gaussian(arg_shape=sh, sigma=1.5)
        G = pxo.Gradient(arg_shape=sh)
        l21 = pxo.L21Norm(arg_shape=(2, *sh))
    else:
        H = pxo.Gaussian(arg_shape=(stack, *sh), sigma=(0, 1.5, 1.5))
        G = pxo.Gradient(arg_shape=(stack, *sh), directions=(1, 2))
        l21 = pxo.L21Norm(arg_shape=(2, stack, *sh))
    f = 0.5 * pxo.SquaredL2Norm(dim=stack * N).asloss(to_device(y)) * H + lam * l21.moreau_envelope(mu) * G
    f.diff_lipschitz = 1 + 8 * lam / mu
    return f, pxo.PositiveOrthant(dim=stack * N), stack * N


def _rel_leaf(crit):
    if isinstance(crit, pxst.RelError):
        return crit
    for side in ("_lhs", "_rhs"):
        leaf = _rel_leaf(getattr(crit, side)) if hasattr(crit, side) else None
        if leaf is not None:
            return leaf
    return None


def _engine(lagged, monkeypatch, depth=8, inkernel=False, window=True, pub=True):
    monkeypatch.setattr(pxa.Solver, "_LAG", depth if lagged else 0)
    monkeypatch.setattr(pxa.Solver, "_LAG_INKERNEL", inkernel)
    monkeypatch.setattr(pxa.Solver, "_LAG_WINDOW", window)
    monkeypatch.setattr(pxs.PGD, "_LAG_PUB", pub)
    if not lagged:  # the synchronous reference order itself (no speculative checks either)
        monkeypatch.setattr(pxs.PGD, "_spec_supported", lambda self: False)


def _collect(s, crit, folder, items=(), stats_eq=True):
    """What a finished fit left: the result, the history, the log, and the criterion's end state (`end`: its info(),
    the last history row cast back from it, and whether the RelError leaf keeps the solution tensor itself)."""
    data, hist = s.stats()
    log = (folder / "solver.log").read_text()
    log = re.sub(r"\[[0-9: .-]+\]", "[t]", log)  # time stamps differ
    info = crit.info()
    end = dict(info=info, keeps_x=_rel_leaf(crit).snapshot()[0].data_ptr() == data["x"].data_ptr(),
               is_last_row=all(np.asarray(v, dtype=hist.dtype[k]) == hist[k][-1] for k, v in info.items()))
    return dict(x=to_NUMPY(data["x"]), idx=s._astate["idx"], a=next(s._mstate["a"]), items=list(items), stats_eq=stats_eq,
                hist={k: np.asarray(hist[k]) for k in hist.dtype.names}, log=log, end=end)


def _run(lagged, crit_fn, mode, monkeypatch, tmp_path, tag, depth=8, inkernel=False, pieces=None, stack=1, window=True,
         pub=True, entry=None):
    _engine(lagged, monkeypatch, depth, inkernel, window, pub)
    with pxrt.Precision(pxrt.Width.SINGLE):
        f, g, N = _problem(stack=stack, entry=entry)
        s = pxs.PGD(f=f, g=g, show_progress=False, stop_rate=1, folder=tmp_path / tag)
        x0 = to_device(np.zeros(N, np.float32))
        items, stats_eq = [], True
        crit = crit_fn()
        if mode == "BLOCK":
            s.fit(x0=x0, stop_crit=crit)
        else:
            s.fit(x0=x0, stop_crit=crit, mode=pxa.Mode.MANUAL)
            for n in (pieces or [None]):
                for it in s.steps(n):
                    items.append(to_NUMPY(it["x"]))
                    stats_eq &= bool(torch.equal(s.stats()[0]["x"], it["x"]))  # stats() between items: that item
        return _collect(s, crit, tmp_path / tag, items, stats_eq)


def _same(a, b, exact_rel=True, items=True):
    """Same run.  exact_rel=False (window statistics: the RelError sums of the same terms in another order): the
    RelError history values within 1e-12 relative, the log lines identical once their numbers are rounded to 9
    significant digits; everything else bit for bit."""
    assert a["idx"] == b["idx"] and a["a"] == b["a"]
    assert np.array_equal(a["x"], b["x"])
    # the criterion's end state: info() is the run's last history row, the same in both runs
    assert a["end"]["is_last_row"] and b["end"]["is_last_row"] and set(a["end"]["info"]) == set(b["end"]["info"])
    for k, v in b["end"]["info"].items():
        if k.startswith("RelError") and not exact_rel:
            np.testing.assert_allclose(a["end"]["info"][k], v, rtol=1e-12, atol=0, err_msg=k)
        else:
            assert a["end"]["info"][k] == v, k
    assert set(a["hist"]) == set(b["hist"])
    for k in b["hist"]:
        if k.startswith("RelError") and not exact_rel:
            np.testing.assert_allclose(a["hist"][k], b["hist"][k], rtol=1e-12, atol=0, err_msg=k)
        else:
            np.testing.assert_array_equal(a["hist"][k], b["hist"][k], err_msg=k)
    if exact_rel:
        assert a["log"] == b["log"]
    else:
        rnd = lambda t: re.sub(r"[0-9]+\.[0-9]+(e[-+][0-9]+)?", lambda m: f"{float(m.group(0)):.9g}", t)  # noqa: E731
        assert rnd(a["log"]) == rnd(b["log"])
    if items:
        assert len(a["items"]) == len(b["items"])
        for u, v in zip(a["items"], b["items"]):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("mode", ["BLOCK", "MANUAL"])
@pytest.mark.parametrize("stats", ["window", "window_fold_launch", "epilogue_fold_launch", "epilogue_inkernel_fold"])
def test_lagged_checks_match_synchronous_relerr_stop(mode, stats, monkeypatch, tmp_path):
    """RelError fires mid-run (~ iteration 60 of a MaxIter(500) budget).  Statistics from the next step's window
    (default), or from the step's epilogue folded by a fold launch / the step's last workgroup (bit-identical
    history)."""
    crit = lambda: pxst.MaxIter(500) | pxst.RelError(eps=3e-3)  # noqa: E731
    a = _run(True, crit, mode, monkeypatch, tmp_path, "lag", inkernel=stats == "epilogue_inkernel_fold",
             window=stats.startswith("window"), pub=stats == "window")
    b = _run(False, crit, mode, monkeypatch, tmp_path, "sync")
    monkeypatch.undo()
    assert 20 < b["idx"] < 500
    _same(a, b, exact_rel=not stats.startswith("window"))
    assert a["stats_eq"]
    # after the stop both engines leave the RelError leaf with the stopping check's x: the solution tensor itself
    assert a["end"]["keeps_x"] and b["end"]["keeps_x"]
    assert a["end"]["info"]["N_iter"] == b["idx"] + 1


@pytest.mark.parametrize("depth", [1, 3, 16])
def test_lagged_checks_maxiter_stop_and_depths(depth, monkeypatch, tmp_path):
    """MaxIter fires first (every pending check resolved in order before it), at several lag depths; a stack of
    3 images (rows of the RelError statistics)."""
    crit = lambda: pxst.RelError(eps=1e-9) | pxst.MaxIter(37)  # noqa: E731
    a = _run(True, crit, "MANUAL", monkeypatch, tmp_path, "lag", depth=depth, stack=3)
    b = _run(False, crit, "MANUAL", monkeypatch, tmp_path, "sync", stack=3)
    assert b["idx"] == 37 and b["hist"]["N_iter"][-1] == 38
    _same(a, b, exact_rel=False)


def test_lagged_checks_asymmetric_taps(monkeypatch, tmp_path):
    """Lag depth 3 on asymmetric, per-axis different taps and sampling ((40, 68): 2 x 2 tiles; the window statistics
    and the publishing workgroup run beside the boundary-row corrections): MaxIter fires first."""
    crit = lambda: pxst.RelError(eps=1e-9) | pxst.MaxIter(37)  # noqa: E731
    e = ac.BY_NAME["vec"]
    a = _run(True, crit, "MANUAL", monkeypatch, tmp_path, "lag", depth=3, entry=e)
    b = _run(False, crit, "MANUAL", monkeypatch, tmp_path, "sync", entry=e)
    assert b["idx"] == 37 and b["hist"]["N_iter"][-1] == 38
    _same(a, b, exact_rel=False)


def test_lagged_steps_consumed_in_pieces(monkeypatch, tmp_path):
    """steps(n) closed while checks are in flight returns to the state of its last item (the launches after it
    dropped); the next steps() continues exactly as the synchronous path."""
    crit = lambda: pxst.MaxIter(500) | pxst.RelError(eps=3e-3)  # noqa: E731
    a = _run(True, crit, "MANUAL", monkeypatch, tmp_path, "lag", pieces=[5, 1, 17, None])
    b = _run(False, crit, "MANUAL", monkeypatch, tmp_path, "sync")
    _same(a, b, exact_rel=False)


def _fit(s, crit, N, mode=pxa.Mode.BLOCK):
    s.fit(x0=to_device(np.zeros(N, np.float32)), stop_crit=crit, mode=mode)


@pytest.mark.parametrize("first", ["stopped", "abandoned"])
@pytest.mark.parametrize("window", [True, False], ids=["window", "epilogue"])
def test_refit_with_the_same_solver_and_criterion(first, window, monkeypatch, tmp_path):
    """One solver object and one criterion object fitted twice under the lagged engine give, the second time, the
    first fit's result and a fresh solver's: nothing of a run survives into the next.  The first run is stopped by
    RelError (launches in flight are dropped), or abandoned: MANUAL mode, steps(5) consumed and closed."""
    new_crit = lambda: pxst.MaxIter(500) | pxst.RelError(eps=3e-3)  # noqa: E731
    fresh = _run(True, new_crit, "BLOCK", monkeypatch, tmp_path, "fresh", window=window)
    with pxrt.Precision(pxrt.Width.SINGLE):
        f, g, N = _problem()
        s = pxs.PGD(f=f, g=g, show_progress=False, stop_rate=1, folder=tmp_path / "twice")
        crit = new_crit()
        if first == "stopped":
            _fit(s, crit, N)
            one = _collect(s, crit, tmp_path / "twice")
            assert 20 < one["idx"] < 500
            _same(one, fresh, exact_rel=not window)
        else:
            _fit(s, crit, N, pxa.Mode.MANUAL)
            assert len([it for it in s.steps(5)]) == 5 and s._astate["idx"] == 5
        _fit(s, crit, N)
        two = _collect(s, crit, tmp_path / "twice")
    _same(two, fresh, exact_rel=not window)
    assert two["end"]["keeps_x"]


def test_criterion_of_a_lagged_fit_reused_at_another_stop_rate(monkeypatch, tmp_path):
    """What the lagged engine configured on a criterion for its run (the flag-buffer count, its choice of the fold)
    ends with the run: reused in a stop_rate 3 fit, the criterion gives a fresh criterion's result."""
    new_crit = lambda: pxst.MaxIter(500) | pxst.RelError(eps=3e-3)  # noqa: E731
    _engine(True, monkeypatch, inkernel=True, window=False)
    res = {}
    with pxrt.Precision(pxrt.Width.SINGLE):
        f, g, N = _problem()
        used = new_crit()
        _fit(pxs.PGD(f=f, g=g, show_progress=False, stop_rate=1, folder=tmp_path / "lag"), used, N)
        leaf = _rel_leaf(used)
        assert leaf._lag is None and leaf._window_stats is False  # (results alone would not show a leftover)
        for tag, crit in (("reused", used), ("fresh", new_crit())):
            s = pxs.PGD(f=f, g=g, show_progress=False, stop_rate=3, folder=tmp_path / tag)
            _fit(s, crit, N)
            res[tag] = _collect(s, crit, tmp_path / tag)
    assert 20 < res["fresh"]["idx"] < 1500
    _same(res["reused"], res["fresh"], exact_rel=True)
