"""Nonlinear Conjugate Gradient (mirrors reference opt/solver/nlcg.py:14-271)."""
import numpy as np

import pyxu_amd.abc as pxa
import pyxu_amd.math.linesearch as ls
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.opt.solver.cg import _HostRows, _KernelRows

__all__ = ["NLCG"]

# The direction update in two launches (pxa_nlcg_direction) and the next search's <g, p> from its partials.  False:
# the generic row-op chain below (also taken for more than 65535 stacked rows): the A/B partner and cross-check.
_FUSED = True
_ROW_LIMIT = 65535
# Rows longer than this take the chain as well: the fused kernels keep the CG tail's partition of at most 64
# workgroups per row, which cannot fill the device on one long row (measured: profiles/nlcg_bench.txt).
_FUSED_MAX_N = 2**21


def _rows2d(x):
    return x.reshape(-1, x.shape[-1])


def _chain_direction(variant, restart, g_kp1, g_k, p_k, gg_k):
    """The direction update as a chain of generic row operations (nlcg.py:213-227, :254-265): returns (sum g_kp1^2
    (device float64 per row), p_kp1 = beta p_k - g_kp1 in a fresh buffer).  The same arithmetic as
    pxa_nlcg_direction: the PR difference in the working type, sums in double, beta = (T)(double ratio)."""
    rows = _rows2d(g_kp1).shape[0]
    gg_kp1 = _dev.row_reduce(_dev.RED_SUMSQ, _rows2d(g_kp1))
    neg_g = _dev.axpby(-1.0, g_kp1)
    if restart:
        beta = _dev.fill(_dev.empty((rows,), g_kp1), 0.0)
    elif variant == "fr":
        beta = _dev.row_ratio(gg_kp1.reshape(-1), gg_k.reshape(-1), g_kp1)
    else:
        diff = _dev.axpby(1.0, g_kp1, -1.0, g_k)
        num = _dev.row_reduce(_dev.RED_DOT, _rows2d(g_kp1), _rows2d(diff))
        beta = _dev.row_ratio(num.reshape(-1), gg_k.reshape(-1), g_kp1)
        beta = _dev.clip(beta, 0.0, out=beta)
    p_kp1 = _dev.axpy_rows(beta, 1.0, _rows2d(p_k), _rows2d(neg_g), out=_dev.empty_like(p_k))  # beta p - g
    return gg_kp1, p_kp1


class NLCG(pxa.Solver):
    r"""
    Nonlinear Conjugate Gradient method (nlcg.py:14-127): a local minimum of a differentiable ``f``.

    ``fit()`` parameters: ``x0`` (..., N) initial point(s); ``variant`` "PR" (Polak-Ribiere+, default) or "FR"
    (Fletcher-Reeves); ``restart_rate`` (default N); ``a0``, ``r``, ``c`` forwarded to
    :py:func:`pyxu_amd.math.linesearch.backtracking_linesearch` (``a0`` defaults to ``1 / f.diff_lipschitz``).

    One iteration is the line search (one host read per trial), ``f.grad`` at the accepted trial point -- which IS
    the search's last trial buffer -- and the direction update in two launches (csrc/nlcg.hip): beta, ``p = beta p - g``,
    ``sum g^2`` published for the default stop criterion, and the ``<g, p>`` partials of the next search.  ``f(x)`` of
    a search is the accepted value of the search before it (the same array through the same kernels).  Arrays handed
    out by ``steps()`` / ``stats()`` are never written again: every iteration's x, gradient and direction are fresh
    buffers.
    """

    def __init__(self, f, **kwargs):
        kwargs.update(log_var=kwargs.get("log_var", ("x",)))
        super().__init__(**kwargs)
        self._f = f

    @pxrt.enforce_precision(i="x0")
    def m_init(self, x0, variant="PR", restart_rate=None, **kwargs):
        mst = self._mstate
        if (a0 := kwargs.get("a0")) is None:
            d_l = self._f.diff_lipschitz
            if np.isclose(d_l, np.inf) or np.isclose(d_l, 0):
                msg = "[NLCG] cannot auto-infer initial step size: specify `a0` manually in NLCG.fit()"
                raise ValueError(msg)
            else:
                a0 = pxrt.coerce(1 / d_l)
        if restart_rate is not None:
            assert restart_rate >= 1
            mst["restart_rate"] = int(restart_rate)
        else:
            mst["restart_rate"] = x0.shape[-1]
        x0 = _dev.require(x0, "x0")
        mst["x"] = x0
        mst["gradient"] = g = self._f.grad(x0)
        mst["conjugate_dir"] = _dev.axpby(-1.0, g)
        mst["variant"] = self.__parse_variant(variant)
        mst["ls_a0"] = a0
        mst["ls_r"] = kwargs.get("r", ls.LINESEARCH_DEFAULT_R)
        mst["ls_c"] = kwargs.get("c", ls.LINESEARCH_DEFAULT_C)
        mst["ls_a_k"] = mst["ls_a0"]
        # sum g0^2: the first beta's denominator and, published, the first stop check's statistic
        gg = _HostRows(_dev.row_reduce(_dev.RED_SUMSQ, _rows2d(g)))
        self._gg = (gg, g)
        mst.link.rowstat = {"gradient": (g, 2, gg)}
        self._f_x = None  # (f(x) array, x) carried from the previous search
        self._gp = None  # (<g, p> partials, nb, g, p) left by the previous direction update
        self._ls_ws = None

    def _buffers(self, rows, like):
        """(device float64 (rows,), HostFlagBuffer) for sum g^2, two sets used alternately (a step reads the previous
        step's device value while its kernel writes the other), and the direction update's workspace."""
        import torch

        bufs = self.__dict__.get("_gg_bufs")
        if bufs is None or bufs[0][0].numel() != rows or bufs[0][0].device != like.device:
            bufs = [(torch.empty((rows,), dtype=torch.float64, device=like.device), _dev.HostFlagBuffer(rows, rows, rows))
                    for _ in range(2)]
            need = max(int(_dev.lib.pxa_nlcg_workspace_bytes(rows)) // 8, 1)
            self._gg_bufs, self._gg_flip = bufs, 0
            self._work = torch.empty((need,), dtype=torch.float64, device=like.device)
        self._gg_flip ^= 1
        return bufs[self._gg_flip]

    def m_step(self):
        """nlcg.py:192-227."""
        mst = self._mstate
        x_k, g_k, p_k = mst["x"], mst["gradient"], mst["conjugate_dir"]
        rows = _rows2d(x_k).shape[0]
        fused = _FUSED and rows <= _ROW_LIMIT and x_k.shape[-1] <= _FUSED_MAX_N
        if self._ls_ws is None or self._ls_ws.rows != rows:
            self._ls_ws = ls._Workspace(rows, x_k)
        f_x = self._f_x[0] if self._f_x is not None and self._f_x[1] is x_k else None
        gp, nb = None, 0
        if self._gp is not None and self._gp[2] is g_k and self._gp[3] is p_k:
            gp, nb = self._gp[0], self._gp[1]
        with pxrt.EnforcePrecision(False):  # (the state already has the run's precision)
            a_k, x_kp1, f_kp1, _ = ls._search(self._f, x_k, p_k, gradient=g_k, a0=mst["ls_a0"], r=mst["ls_r"],
                                              c=mst["ls_c"], f_x=f_x, gp=gp, gp_nb=nb, ws=self._ls_ws)
        # x_kp1 = x_k + a_k p_k is the accepted trial buffer, f_kp1 the objective there
        self._f_x = (f_kp1, x_kp1)
        g_kp1 = self._f.grad(x_kp1)
        restart = self._astate["idx"] % mst["restart_rate"] == 0
        mst.link.rowstat = {}
        if self._gg is not None and self._gg[1] is g_k:
            gg_k = self._gg[0].dev
        else:
            gg_k = _dev.row_reduce(_dev.RED_SUMSQ, _rows2d(g_k))
        if fused:
            p_kp1 = _dev.empty_like(p_k)
            gg_out, fb = self._buffers(rows, x_k)
            var = _dev.NLCG_PR if mst["variant"] == "pr" else _dev.NLCG_FR
            seq = _dev.nlcg_direction(var, restart, _rows2d(g_kp1), _rows2d(g_k), _rows2d(p_k), _rows2d(p_kp1),
                                      gg_k.reshape(-1), gg_out, fb, self._work)
            hr = _KernelRows(gg_out, fb, seq)
            self._gp = (_dev.nlcg_gp_partials(self._work, rows), _dev.nlcg_blocks(x_k.shape[-1]), g_kp1, p_kp1)
        else:
            gg_kp1, p_kp1 = _chain_direction(mst["variant"], restart, g_kp1, g_k, p_k, gg_k)
            hr = _HostRows(gg_kp1)  # async copy of sum g^2 for the stop check
            self._gp = None
        self._gg = (hr, g_kp1)
        mst.link.rowstat = {"gradient": (g_kp1, 2, hr)}
        mst["x"], mst["gradient"], mst["conjugate_dir"], mst["ls_a_k"] = x_kp1, g_kp1, p_kp1, a_k

    def default_stop_crit(self):
        from pyxu_amd.opt.stop import AbsError

        return AbsError(eps=1e-4, var="gradient", f=None, norm=2, satisfy_all=True)

    def objective_func(self):
        return self._f(self._mstate["x"])

    def solution(self):
        data, _ = self.stats()
        return data.get("x")

    def __parse_variant(self, variant):
        supported_variants = {"fr", "pr"}
        if (v := variant.lower().strip()) not in supported_variants:
            raise ValueError(f"Unsupported variant '{variant}'.")
        return v
