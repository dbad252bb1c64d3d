"""Backtracking line search (mirrors reference ``pyxu.math.linesearch``, src/pyxu/math/linesearch.py:19-94)."""
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev

__all__ = ["backtracking_linesearch"]

LINESEARCH_DEFAULT_R = 0.5
LINESEARCH_DEFAULT_C = 1e-4

_ROW_LIMIT = 65535  # rows of one pxa_ls_armijo launch


class _Workspace:
    """Buffers a search needs besides its arrays: the step vector is fresh per search (it is returned); the trial
    counters and the host flag buffer of the failing-row count are kept by the caller across searches."""

    def __init__(self, rows, like):
        import torch

        self.rows = rows
        self.trials = torch.zeros((rows,), dtype=torch.int32, device=like.device)
        # one flag buffer per slab of _ROW_LIMIT rows (one pxa_ls_armijo launch each)
        self.fbs = [_dev.HostFlagBuffer(1, 1, 1) for _ in range(0, rows, _ROW_LIMIT)]


def _rows2d(x):
    return x.reshape(-1, x.shape[-1])


def _search(f, x, direction, gradient=None, a0=None, r=LINESEARCH_DEFAULT_R, c=LINESEARCH_DEFAULT_C, f_x=None, gp=None,
            gp_nb=0, ws=None):
    """The search of backtracking_linesearch; returns (a, x_trial, f_trial, trials): the (..., 1) steps, the last
    trial's buffer, which holds x + a * direction for EVERY row (all rows are re-evaluated on every trial with their
    current a, as in the reference), f.apply of that buffer, and the number of launches of the Armijo test.

    f_x: f.apply(x) if the caller has it (NLCG: the previous search's accepted f_trial); gp / gp_nb: <gradient,
    direction> per row as float64 device values (gp_nb == 0) or as the gp_nb partials per row that
    pxa_nlcg_direction left (then `gradient` is not read)."""
    assert 0 < r < 1
    assert 0 < c < 1
    if a0 is None:
        a0 = pxrt.coerce(1 / f.diff_lipschitz)
        assert a0 > 0, "a0: cannot auto-set step size."
    else:
        assert a0 > 0
    x = _dev.require(x, "x")
    direction = _dev.require(direction, "direction")
    x2, d2 = _rows2d(x), _rows2d(direction)
    rows = x2.shape[0]
    if rows < 1:
        raise ValueError("backtracking_linesearch: x holds no rows.")
    if gp is None:
        if gradient is None:
            gradient = f.grad(x)
        gp, gp_nb = _dev.row_reduce(_dev.RED_DOT, _rows2d(gradient), d2), 0
    if f_x is None:
        f_x = f.apply(x)
    if ws is None or ws.rows != rows or ws.trials.device != x.device:
        ws = _Workspace(rows, x)
    a = _dev.fill(_dev.empty((rows,), x), float(a0))
    trials = 0
    while True:
        x_trial = _dev.axpy_rows(a, 1.0, d2, x2, out=_dev.empty_like(x))  # x + a * direction, a fresh buffer
        f_trial = f.apply(x_trial)
        if rows <= _ROW_LIMIT:
            seq = _dev.ls_armijo(f_trial, f_x, gp, gp_nb, c, r, a, ws.trials, ws.fbs[0])
            failed = _dev.ls_failed(ws.fbs[0], seq)  # the loop's one host read per trial
        else:  # slabs of the launch's row limit (gp is then one folded value per row)
            ft, fx = f_trial.reshape(-1), f_x.reshape(-1)
            seqs = [_dev.ls_armijo(ft[r0:r0 + _ROW_LIMIT], fx[r0:r0 + _ROW_LIMIT], gp.reshape(-1)[r0:r0 + _ROW_LIMIT], 0, c,
                                   r, a[r0:r0 + _ROW_LIMIT], ws.trials[r0:r0 + _ROW_LIMIT], fb)
                    for r0, fb in zip(range(0, rows, _ROW_LIMIT), ws.fbs)]
            failed = sum(_dev.ls_failed(fb, seq) for fb, seq in zip(ws.fbs, seqs))
        trials += 1
        if failed == 0:
            break
    return a.reshape(*x.shape[:-1], 1), x_trial, f_trial, trials


@pxrt.enforce_precision(i=("x", "direction", "gradient", "a0", "r", "c"), allow_None=True)
def backtracking_linesearch(f, x, direction, gradient=None, a0=None, r=LINESEARCH_DEFAULT_R, c=LINESEARCH_DEFAULT_C):
    r"""
    Backtracking line search based on the Armijo-Goldstein condition (linesearch.py:19-94).

    Parameters
    ----------
    f: DiffFunc
        Differentiable functional.
    x: device array
        (..., N) initial search point(s).
    direction: device array
        (..., N) search direction(s).
    gradient: device array
        (..., N) gradient of `f` at `x`; computed with ``f.grad`` if unspecified.
    a0: Real
        Initial step size; ``1 / f.diff_lipschitz`` if unspecified.
    r: Real
        Step reduction factor, ``0 < r < 1``.
    c: Real
        Bound reduction factor, ``0 < c < 1``.

    Returns
    -------
    a: device array
        (..., 1) step sizes, of `x`'s dtype.

    Every trial is ``pxa_axpy_rows`` -> ``f.apply`` -> one launch of the Armijo test for all rows
    (``pxa_ls_armijo``), and the host reads one word: the number of rows that failed.  Rows that pass keep their
    step; rows that fail get ``a *= r``.  A NaN on either side of the test is not a failure, as in the reference.

    There is no cap on the number of trials, as in the reference.  The loop ends by itself: once ``a * direction``
    is below an ulp of ``x`` the trial point equals ``x`` and ``f_trial == f_x``, while ``a c <g, d>`` has shrunk
    below an ulp of ``f_x`` (or is positive, for an ascent direction), so ``f_trial <= f_x + a c <g, d>`` holds.
    That takes about 25 to 30 halvings in float32 and about 55 in float64 (``r = 0.5``, ``|a0 direction| ~ |x|``).
    """
    return _search(f, x, direction, gradient=gradient, a0=a0, r=r, c=c)[0]
