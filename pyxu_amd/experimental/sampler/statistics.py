"""Online statistics of a sampler's output (mirrors reference experimental/sampler/statistics.py)."""
import math
import numbers
import types

import numpy as np

from pyxu_amd import _dev

__all__ = ["OnlineMoment", "OnlineCenteredMoment", "OnlineVariance", "OnlineStd", "OnlineSkewness", "OnlineKurtosis"]


def _is_scalar(v):
    return isinstance(v, (numbers.Real, np.integer, np.floating)) and not isinstance(v, bool)


def _nan_ratio(a, b):
    """a / b, NaN where b == 0 (statistics.py:81-85): 0 / b is 0 for every other b and NaN there."""
    q = _dev.binary(_dev.BIN_DIV, a, b)
    return _dev.binary(_dev.BIN_ADD, q, _dev.binary(_dev.BIN_DIV, 0.0, b), out=q)


class _OnlineStat:
    """
    Base class of the online statistics of one sampler's output.  ``update(x)`` folds a sample in and returns the
    statistic, a fresh device array; ``stat()`` returns the last value.  ``+ - * / **`` compose statistics (with each
    other, or ``* / **`` with scalars); a composite evaluates each operand once per sample.
    """

    def __init__(self):
        self._num_samples = 0
        self._stat = None

    def update(self, x):
        raise NotImplementedError

    def stat(self):
        return self._stat

    @staticmethod
    def _composite(fn):
        stat = _OnlineStat()

        def stat_update(_, x):
            _._stat = fn(x)
            _._num_samples += 1
            return _._stat

        stat.update = types.MethodType(stat_update, stat)
        return stat

    def __add__(self, other):
        if not isinstance(other, _OnlineStat):
            return NotImplemented
        return self._composite(lambda x: _dev.binary(_dev.BIN_ADD, self.update(x), other.update(x)))

    def __sub__(self, other):
        if not isinstance(other, _OnlineStat):
            return NotImplemented
        return self._composite(lambda x: _dev.binary(_dev.BIN_SUB, self.update(x), other.update(x)))

    def __mul__(self, other):
        if isinstance(other, _OnlineStat):
            return self._composite(lambda x: _dev.mul(self.update(x), other.update(x)))
        if _is_scalar(other):
            return self._composite(lambda x: _dev.axpby(float(other), self.update(x)))
        return NotImplemented

    def __rmul__(self, other):
        return self.__mul__(other)

    def __truediv__(self, other):
        if isinstance(other, _OnlineStat):
            return self._composite(lambda x: _nan_ratio(self.update(x), other.update(x)))
        if _is_scalar(other):
            return self._composite(lambda x: _dev.div(self.update(x), float(other)))
        return NotImplemented

    def __pow__(self, expo):
        if not _is_scalar(expo):
            return NotImplemented
        if expo == 0.5:
            return self._composite(lambda x: _dev.unary(_dev.UN_SQRT, self.update(x)))
        return self._composite(lambda x: _dev.binary(_dev.BIN_POW, self.update(x), float(expo)))


def _power(x, order):
    if order == 1:
        return _dev.copy(x)
    if order == 2:
        return _dev.mul(x, x)
    return _dev.binary(_dev.BIN_POW, x, float(order))


class OnlineMoment(_OnlineStat):
    r"""Pointwise online moment :math:`\frac{1}{K}\sum_k x_k^d` (statistics.py:103-123)."""

    def __init__(self, order=1):
        super().__init__()
        self._order = order

    def update(self, x):
        x = _dev.require(x, "x")
        p = _power(x, self._order)
        if self._num_samples > 0:
            p = _dev.axpby(float(self._num_samples), self._stat, 1.0, p, out=p)
        self._num_samples += 1
        self._stat = _dev.div(p, float(self._num_samples), out=p)
        return self._stat


class OnlineCenteredMoment(_OnlineStat):
    r"""
    Pointwise online centred moment :math:`\mu_d = \frac{1}{K}\sum_k (x_k - \mu)^d`, :math:`d \geq 2`, by the Welford
    recurrence of statistics.py:126-171: the running mean in the samples' precision (``_mean``) and the corrected sums
    of orders 2 .. d in float64 (``_corrected_sums``, (d - 1, n)).  Orders 2 to 4 update in one launch
    (``pxa_online_moments``); higher orders run the same recurrence as a chain of element-wise launches.  The statistic
    is returned in the samples' precision.
    """

    def __init__(self, order=2):
        super().__init__()
        if int(order) != order or order < 2:
            raise ValueError(f"order: expected an integer >= 2, got {order}")
        self._order = int(order)
        self._corrected_sums = None
        self._mean = None

    def _fold(self, x):
        k, flat = self._num_samples, x.reshape(-1)
        if k == 0:
            self._corrected_sums = _dev.empty_f64((self._order - 1, flat.numel()), x)
            self._mean = _dev.empty_like(flat)
        elif tuple(x.shape) != self._shape or x.dtype != self._mean.dtype:
            raise ValueError("OnlineCenteredMoment: every sample must have the first one's shape and dtype")
        self._shape = tuple(x.shape)
        if self._order <= 4:
            _dev.online_moments(self._order, k, flat, self._mean, self._corrected_sums)
        else:
            self._chain(k, flat)
        self._num_samples += 1

    def _chain(self, k, x):
        S, mean = self._corrected_sums, self._mean
        if k == 0:
            _dev.fill(S, 0.0)
            mean.copy_(x)
            return
        temp = _dev.axpby(1.0, x, -1.0, mean)
        temp = _dev.div(temp, float(k + 1), out=temp)
        a = _dev.cast(_dev.unary(_dev.UN_NEG, temp), S)
        b = _dev.cast(_dev.axpby(float(k), temp), S)
        for r in range(self._order, 1, -1):  # descending: an order reads the lower orders' previous sums
            Sr = S[r - 2]
            for s in range(2, r):
                p = a if r - s == 1 else _dev.binary(_dev.BIN_POW, a, float(r - s))
                _dev.axpby(1.0, Sr, float(math.comb(r, s)), _dev.mul(S[s - 2], p), out=Sr)
            _dev.axpby(1.0, Sr, float(k), _dev.binary(_dev.BIN_POW, a, float(r)), out=Sr)
            _dev.axpby(1.0, Sr, 1.0, _dev.binary(_dev.BIN_POW, b, float(r)), out=Sr)
        _dev.axpby(k / (k + 1), mean, 1.0, _dev.div(x, float(k + 1)), out=mean)

    def _moment(self, r):
        """mu_r in float64, flat."""
        return _dev.div(self._corrected_sums[r - 2], float(self._num_samples))

    def _finish(self, v, x):
        v = v if v.dtype == x.dtype else _dev.cast(v, x)
        self._stat = v.reshape(self._shape)
        return self._stat

    def update(self, x):
        x = _dev.require(x, "x")
        self._fold(x)
        return self._finish(self._moment(self._order), x)


def OnlineVariance():
    r"""Pointwise online variance :math:`\sigma^2 = \frac{1}{K}\sum_k (x_k - \mu)^2`."""
    return OnlineCenteredMoment(order=2)


def OnlineStd():
    r"""Pointwise online standard deviation."""
    return OnlineVariance() ** (1 / 2)


class _Standardized(OnlineCenteredMoment):
    """mu_r / mu_2^(r / 2) from one order-r Welford state; NaN where the variance is 0."""

    def update(self, x):
        x = _dev.require(x, "x")
        self._fold(x)
        var = self._moment(2)
        den = _dev.mul(var, var) if self._order == 4 else _dev.mul(var, _dev.unary(_dev.UN_SQRT, var))
        return self._finish(_nan_ratio(self._moment(self._order), den), x)


def OnlineSkewness():
    r"""
    Pointwise online skewness :math:`\frac{1}{K}\sum_k ((x_k - \mu) / \sigma)^3 = \mu_3 / \mu_2^{3/2}`, NaN where
    the variance is 0.  (The reference's composite calls its divisor's ``update`` three times per sample and does not
    return this quantity: README, deviations.)
    """
    return _Standardized(order=3)


def OnlineKurtosis():
    r"""Pointwise online kurtosis :math:`\mu_4 / \mu_2^2` (3 for a Gaussian), NaN where the variance is 0."""
    return _Standardized(order=4)
