"""Indicator functions (reference operator/func/indicator.py): PositiveOrthant and the norm balls."""
import numpy as np

import pyxu_amd.abc as pxa
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.operator.func.norm import L2Norm, _ShiftLossMixin

__all__ = ["L1Ball", "L2Ball", "LInfinityBall", "PositiveOrthant"]


class PositiveOrthant(pxa.ProxFunc):
    """Indicator of {x >= 0} (indicator.py:174-206); prox = clip(0, None)."""

    def __init__(self, dim):
        super().__init__(shape=(1, dim))
        self.lipschitz = np.inf

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        neg = _dev.row_reduce(_dev.RED_NEGCNT, arr.reshape(-1, arr.shape[-1]))
        return _dev.cast(_dev.unary(_dev.UN_POSINF, neg), arr).reshape(*arr.shape[:-1], 1)

    @pxrt.enforce_precision(i=("arr", "tau"))
    def prox(self, arr, tau):
        return _dev.clip(arr, 0.0)


class _NormBall(_ShiftLossMixin, pxa.ProxFunc):
    """Indicator of {||x||_ord <= radius}, ord in (1, 2, inf) (indicator.py:41-69).

    apply: 0 / inf per row, from the device row reduction with no host read.  prox (tau is ignored, as in the
    reference) is the projection x - prox_{radius * dual norm}(x):

    * ord = 1: the soft-threshold at the root of sum_i max(|x_i| - mu, 0) = radius (device threshold search);
    * ord = 2: x - L2Norm.prox(x, radius), as the reference composes it;
    * ord = inf: clip(x, -radius, radius).

    Declared difference: inside the l1 ball the reference's brentq raises ValueError; here the projection returns x
    bit for bit.
    """

    def __init__(self, dim, ord, radius):
        super().__init__(shape=(1, dim))
        self.lipschitz = np.inf
        assert ord in (1, 2, np.inf)
        self._ord = ord
        self._radius = float(radius)

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        x2 = arr.reshape(-1, arr.shape[-1])
        op = {1: _dev.RED_ABS, 2: _dev.RED_SUMSQ, np.inf: _dev.RED_MAXABS}[self._ord]
        nrm = _dev.row_reduce(op, x2)
        if self._ord == 2:
            nrm = _dev.unary(_dev.UN_SQRT, nrm, out=nrm)
        # +inf where norm > radius, and where the norm is NaN (NaN <= radius is False in the reference)
        ind = _dev.unary(_dev.UN_POSINF, _dev.add_scalar(nrm, -self._radius))
        ind = _dev.where(_dev.isnan(nrm), np.inf, ind)
        return _dev.cast(ind, arr).reshape(*arr.shape[:-1], 1)

    @pxrt.enforce_precision(i=("arr", "tau"))
    def prox(self, arr, tau):
        r = self._radius
        if self._ord == 1:
            x2 = _dev.require(arr).reshape(-1, arr.shape[-1])
            return _dev.row_threshold_prox(x2, 1.0, 0.0, r, _dev.SHRINK_SOFT).reshape(arr.shape)
        if self._ord == 2:
            p = L2Norm(dim=self.dim).prox(arr, tau=r)
            return _dev.axpby(1.0, arr, -1.0, p, out=p)
        return _dev.clip(arr, -r, r)


def L1Ball(dim, radius=1):
    """Indicator of the l1 ball of `radius` (indicator.py:72-103)."""
    op = _NormBall(dim=dim, ord=1, radius=radius)
    op._name = "L1Ball"
    return op


def L2Ball(dim, radius=1):
    """Indicator of the l2 ball of `radius` (indicator.py:106-137)."""
    op = _NormBall(dim=dim, ord=2, radius=radius)
    op._name = "L2Ball"
    return op


def LInfinityBall(dim, radius=1):
    """Indicator of the l-infinity ball of `radius` (indicator.py:140-171)."""
    op = _NormBall(dim=dim, ord=np.inf, radius=radius)
    op._name = "LInfinityBall"
    return op
