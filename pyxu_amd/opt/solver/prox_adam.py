"""Proximal Adam (mirrors reference opt/solver/prox_adam.py:18-478)."""
import collections
import math
import warnings

import numpy as np

import pyxu_amd.abc as pxa
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.opt.solver._fused import _unscale
from pyxu_amd.opt.solver.pgd import PGD, AutoInferenceWarning

__all__ = ["ProxAdam"]

# The moment update and gradient step in one launch (pxa_proxadam_moments) and, for an element-wise g, the metric-prox
# sub-problems of all rows as batched device sub-iterations (pxa_proxadam_sub_step).  False: the chain of generic
# element-wise operations and the reference's literal per-row PGD construction: the A/B partner and cross-check.
_FUSED = True
_ROW_LIMIT = 65535
# Sub-step launches enqueued ahead of the running-row count the host reads (a launch after every row has finished
# changes nothing): the host read then overlaps the next launches.  1: every launch waits for its own count.
_LOOKAHEAD = 4
_SUB_MAX_ITER = 1_000_000  # a sub-solve that never meets its RelError (a NaN iterate) raises instead of spinning


def _rows2d(x):
    return x.reshape(-1, x.shape[-1])


def _chain_moments(variant, first, g, m, v, vh, x, sc):
    """prox_adam.py:341-370 as a chain of generic element-wise operations, every result in a fresh buffer; `sc`: the
    scalars of ProxAdam._scalars.  Returns (x', psi, m', v', vhat')."""
    m = _dev.axpby(sc["b1"], m, sc["omb1"], g)
    g2 = _dev.mul(g, g)
    vu = _dev.axpby(sc["b2"], v, sc["omb2"], g2, out=g2)
    v = _dev.clip(vu, sc["eps_var"], out=vu)
    vh = v if first else _dev.binary(_dev.BIN_MAXIMUM, vh, v)
    if variant == "adam":
        phi = _dev.div(m, sc["c1"])
        psi = _dev.unary(_dev.UN_SQRT, v)
        psi = _dev.div(psi, sc["c2"], out=psi)
        psi = _dev.add_scalar(psi, sc["eps_adam"], out=psi)
    elif variant == "amsgrad":
        phi, psi = m, _dev.unary(_dev.UN_SQRT, vh)
    else:
        phi, psi = m, _dev.binary(_dev.BIN_POW, vh, float(sc["p"]))
    q = _dev.binary(_dev.BIN_DIV, phi, psi)
    x_new = _dev.axpby(1.0, x, -sc["a"], q, out=q)
    return x_new, psi, m, v, vh


def _sub_kind(g, n):
    """(prox kind, parameter) when g is one of the element-wise functionals the batched sub-solve knows: lam L1Norm,
    PositiveOrthant, lam PositiveL1Norm, LInfinityBall(r); else None."""
    from pyxu_amd.operator.func.indicator import PositiveOrthant, _NormBall
    from pyxu_amd.operator.func.norm import L1Norm, PositiveL1Norm

    gi, gs = _unscale(g)
    if not gs > 0 or getattr(gi, "dim", None) != n:
        return None
    if type(gi) is L1Norm:
        return _dev.PROX_L1, gs
    if type(gi) is PositiveOrthant:
        return _dev.PROX_POS, 0.0
    if type(gi) is PositiveL1Norm:
        return _dev.PROX_POSL1, gs
    if type(gi) is _NormBall and gi._ord == np.inf:
        return _dev.PROX_BOX, gi._radius
    return None


def _plain_relerr(crit):
    """eps of a plain RelError on x (norm 2, f=None, satisfy_all), else None."""
    from pyxu_amd.opt.stop import RelError, _identity

    if (type(crit) is RelError and crit._var == "x" and crit._norm == 2 and crit._f is _identity and crit._satisfy_all
            and crit._reduce is None):
        return float(crit._eps)
    return None


class ProxAdam(pxa.Solver):
    r"""
    Proximal Adam (prox_adam.py:18-227): minimises ``f + g`` with ``f`` differentiable and ``g`` proximable, without
    ``f.diff_lipschitz`` and without a line search.

    ``fit()`` parameters: ``x0`` (..., N); ``variant`` "adam" (default), "amsgrad" or "padam"; ``a`` step size (default
    ``1 / f.diff_lipschitz``); ``b1``, ``b2`` decay rates in [0, 1); ``m0``, ``v0`` initial moments (broadcast to x0);
    ``kwargs_sub``, ``stop_crit_sub`` for the sub-problems; ``p`` in (0, 0.5] (padam); ``eps_adam``, ``eps_var`` > 0.

    One iteration is ``f.grad``, one launch for the moments and the step ``x - a phi / psi`` (csrc/proxadam.hip), and,
    with ``g``, the metric prox ``min_z g(z) + 1/(2a) ||z - x||^2_diag(psi)`` per stacked row by accelerated PGD.  For
    ``lam L1Norm``, ``PositiveOrthant``, ``lam PositiveL1Norm`` and ``LInfinityBall`` with the default sub-problem
    settings all rows advance in one launch per sub-iteration, the stop test runs on the device and the host reads one
    word per sub-iteration; anything else runs the reference's per-row ``PGD``.  ``_sub_iters`` holds the last step's
    sub-iteration count per row.  Neither ``x0``, ``m0`` nor ``v0`` is written; arrays handed out by ``steps()`` /
    ``stats()`` are never written again.
    """

    def __init__(self, f, g=None, **kwargs):
        kwargs.update(log_var=kwargs.get("log_var", ("x",)))
        super().__init__(**kwargs)
        self._f = f
        self._prox_required = g is not None
        self._g = g
        self._sub_iters = None

    @pxrt.enforce_precision(i=("x0", "b1", "b2", "m0", "v0", "p", "eps_adam", "eps_var"))
    def m_init(self, x0, variant="adam", a=None, b1=0.9, b2=0.999, m0=None, v0=None, kwargs_sub=None, stop_crit_sub=None,
               p=0.5, eps_adam=1e-6, eps_var=1e-6):
        from pyxu_amd.operator.linop import NullFunc

        mst = self._mstate
        x0 = _dev.require(x0, "x0")
        mst["x"] = x0
        if self._g is None:
            self._g = NullFunc(dim=x0.shape[-1])
        if a is None:
            with np.errstate(divide="ignore"):
                mst["a"] = pxrt.coerce(np.float64(1.0) / np.float64(self._f.diff_lipschitz))
            if math.isinf(mst["a"]) or mst["a"] == 0:  # f is constant-valued, or its constant is unknown
                mst["a"] = pxrt.coerce(1)
                msg = "\n".join([rf"The gradient step size `a` is auto-set to {mst['a']}.",
                                 r"Choosing a manually may lead to faster convergence."])
                warnings.warn(msg, AutoInferenceWarning)
        else:
            try:
                assert a > 0
                mst["a"] = pxrt.coerce(a)
            except Exception:
                raise ValueError(f"`a` must be positive, got {a}.")
        mst["variant"] = self.__parse_variant(variant)
        assert 0 < p <= 0.5, f"p: expected value in (0, 0.5], got {p}."
        mst["padam_p"] = p
        assert eps_adam > 0, f"eps_adam: expected positive value, got {eps_adam}."
        mst["eps_adam"] = eps_adam
        mst["mean"] = self.__moment(m0, x0, "m0")
        mst["variance"] = self.__moment(v0, x0, "v0")
        # (the reference's variance_hat IS its variance array, updated in place before the first maximum: the first
        # step takes variance_hat = variance whatever v0 was -- m_step's `first`)
        mst["variance_hat"] = mst["variance"]
        self._first = True
        mst["subproblem_init_kwargs"] = dict() if kwargs_sub is None else kwargs_sub
        mst["subproblem_stop_crit"] = self.default_stop_crit() if stop_crit_sub is None else stop_crit_sub
        assert 0 <= b1 < 1, f"b1: expected value in [0, 1), got {b1}."
        mst["b1"] = b1
        assert 0 <= b2 < 1, f"b2: expected value in [0, 1), got {b2}."
        mst["b2"] = b2
        assert eps_var > 0, f"eps_var: expected positive value, got {eps_var}."
        mst["eps_variance"] = eps_var
        self._sub_iters = None
        self._ws = None

    @staticmethod
    def __moment(m0, x0, name):
        """The solver's own copy of an initial moment, broadcast to x0 (zeros when None)."""
        if m0 is None:
            return _dev.zeros(x0.shape, x0)
        m0 = _dev.require(m0, name)
        if m0.shape != x0.shape:
            import torch

            m0 = torch.broadcast_to(m0, x0.shape)
        return _dev.copy(m0)

    # ------------------------------------------------------------------ the step
    def _scalars(self):
        """The step's scalars in the run's precision, formed on the host as the reference forms them."""
        mst = self._mstate
        t = self._astate["idx"]
        b1, b2 = mst["b1"], mst["b2"]
        c1 = 1 - (b1 ** t)
        c2 = np.sqrt(1 - b2 ** t)
        return dict(b1=b1, omb1=1 - b1, b2=b2, omb2=1 - b2, eps_var=mst["eps_variance"], c1=c1, c2=c2,
                    eps_adam=mst["eps_adam"], a=mst["a"], p=mst["padam_p"])

    def _workspace(self, rows, n, like):
        ws = self._ws
        if ws is None or ws["key"] != (rows, n, like.dtype, like.device):
            ws = self._ws = dict(key=(rows, n, like.dtype, like.device), work=_dev.proxadam_workspace(rows, n, like),
                                 psi=_dev.empty((rows, n), like), xt=_dev.empty((rows, n), like), z=None, ring=None)
        return ws

    def m_step(self):
        mst = self._mstate
        x = mst["x"]
        shape, n = x.shape, x.shape[-1]
        rows = _rows2d(x).shape[0]
        g = _dev.require(self._f.grad(x), "gradient")
        sc = self._scalars()
        first, self._first = self._first, False
        logged = self._astate["log_var"]
        if _FUSED and rows <= _ROW_LIMIT:
            m, v, vh = mst["mean"], mst["variance"], mst["variance_hat"]
            m_out = _dev.empty_like(m) if "mean" in logged else m
            v_out = _dev.empty_like(v) if "variance" in logged else v
            vh_out = _dev.empty_like(vh) if ("variance_hat" in logged or first) else vh
            if self._prox_required:
                ws = self._workspace(rows, n, x)
                x_new, psi, work = ws["xt"], ws["psi"], ws["work"]
            else:
                x_new, psi, work = _dev.empty((rows, n), x), None, None
            _dev.proxadam_moments(_dev.PROXADAM_VARIANTS[mst["variant"]], first, _rows2d(g), _rows2d(m), _rows2d(v),
                                  None if first else _rows2d(vh), _rows2d(x), _rows2d(m_out), _rows2d(v_out),
                                  _rows2d(vh_out), x_new, psi_out=psi, work=work, **sc)
            mst["mean"], mst["variance"], mst["variance_hat"] = m_out, v_out, vh_out
        else:
            x_new, psi = self._chain_moments(g, sc, first)
            x_new, psi = _rows2d(x_new), _rows2d(psi)
        if self._prox_required:
            x_new = self._sub_problems(x_new, psi, rows, n)
        mst["x"] = x_new.reshape(shape)

    def _chain_moments(self, g, sc, first):
        mst = self._mstate
        x_new, psi, mst["mean"], mst["variance"], mst["variance_hat"] = _chain_moments(
            mst["variant"], first, g, mst["mean"], mst["variance"], mst["variance_hat"], mst["x"], sc)
        return x_new, psi

    def _sub_plan(self, rows, n):
        """(prox kind, parameter, eps) when the batched device sub-solve applies, else None."""
        mst = self._mstate
        if not _FUSED or rows > _ROW_LIMIT or mst["subproblem_init_kwargs"]:
            return None
        kind = _sub_kind(self._g, n)
        eps = _plain_relerr(mst["subproblem_stop_crit"])
        if kind is None or eps is None:
            return None
        return kind[0], kind[1], eps

    def _sub_problems(self, xt, psi, rows, n):
        """prox_adam.py:373-416: x' of every row replaced by the solution of its metric-prox sub-problem."""
        plan = self._sub_plan(rows, n)
        if plan is None:
            return self._sub_rows(xt, psi, rows, n)
        kind, pw, eps = plan
        ws = self._workspace(rows, n, xt)
        if ws["z"] is None:
            ws["z"] = [_dev.empty((rows, n), xt) for _ in range(3)]
        depth = max(1, int(_LOOKAHEAD))
        if ws["ring"] is None or len(ws["ring"]) < depth + 1:  # (host allocations: made once, kept)
            ws["ring"] = [_dev.HostFlagBuffer(1, 1, 1) for _ in range(depth + 1)]
        zs, ring, work = ws["z"], ws["ring"], ws["work"]
        out = _dev.empty((rows, n), xt)  # handed out as x: a fresh buffer every step
        a = float(self._mstate["a"])
        _dev.proxadam_sub_init(rows, n, work)
        pend = collections.deque()
        k = 0
        while True:
            k += 1
            if k > _SUB_MAX_ITER:
                raise RuntimeError(f"ProxAdam: a sub-problem did not meet its stop criterion in {_SUB_MAX_ITER} iterations")
            if k == 1:
                z_prev, z, z_new = xt, xt, zs[0]
            elif k == 2:
                z_prev, z, z_new = xt, zs[0], zs[1]
            else:
                z_prev, z, z_new = zs[(k - 3) % 3], zs[(k - 2) % 3], zs[(k - 1) % 3]
            mom = pxrt.coerce((k - 1) / (k + 75))  # PGD's k / (k + 1 + d), d = 75, k from 0
            fb = ring[k % len(ring)]
            pend.append((fb, _dev.proxadam_sub_step(kind, k, mom, eps, a, pw, xt, psi, z_prev, z, z_new, out, work, fb)))
            if len(pend) >= depth:
                if _dev.proxadam_running(*pend.popleft()) == 0:
                    break
        state = _dev.proxadam_work_views(work, rows, n)[2]
        self._sub_iters = state.cpu().numpy().astype(np.int64) - 1  # (the word holds the launch that saw the row stop)
        return out

    def _sub_rows(self, xt, psi, rows, n):
        """The reference's construction: one PGD per row on f_sub = (0.5 / a) ||sqrt(psi) (z - x')||^2 and g."""
        from pyxu_amd.operator.func.norm import SquaredL2Norm
        from pyxu_amd.operator.linop import DiagonalOp

        mst = self._mstate
        a = mst["a"]
        scale = pxrt.coerce(0.5 / a)
        psi_max = _dev.row_reduce(_dev.RED_MAX, psi).reshape(-1).cpu().numpy()
        out, iters = _dev.empty((rows, n), xt), []
        for r in range(rows):
            _x, _psi = xt[r], psi[r]
            gamma = pxrt.coerce(a / pxrt.coerce(psi_max[r]))
            h_half = DiagonalOp(_dev.unary(_dev.UN_SQRT, _psi))
            f1 = SquaredL2Norm(dim=n).asloss(h_half.apply(_x)) * h_half
            f = f1 * scale
            kwargs = mst["subproblem_init_kwargs"].copy()
            kwargs.update(show_progress=False)
            slvr = PGD(f=f, g=self._g, **kwargs)
            slvr.fit(x0=_x, tau=gamma, stop_crit=mst["subproblem_stop_crit"])
            _dev.copy2d(_dev.require(slvr.solution()), out, 1, n, n, n, dst_off=r * n)
            iters.append(slvr._astate["idx"])
        self._sub_iters = np.array(iters, dtype=np.int64)
        return out

    def default_stop_crit(self):
        from pyxu_amd.opt.stop import RelError

        return RelError(eps=1e-4, var="x", f=None, norm=2, satisfy_all=True)

    def objective_func(self):
        x = self._mstate["x"]
        return _dev.axpby(1.0, self._f.apply(x), 1.0, self._g.apply(x))

    def solution(self):
        data, _ = self.stats()
        return data.get("x")

    def __parse_variant(self, variant):
        supported_variants = {"adam", "amsgrad", "padam"}
        if (v := variant.lower().strip()) not in supported_variants:
            raise ValueError(f"Unsupported variant '{variant}'.")
        return v
