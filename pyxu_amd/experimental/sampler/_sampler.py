"""ULA and MYULA (mirrors reference experimental/sampler/_sampler.py:105-488)."""
import math

import numpy as np

import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.util import copy_if_unsafe

__all__ = ["ULA", "MYULA"]

# MYULA with an element-wise g: the Moreau-Yosida gradient is formed inside the step's launch (csrc/sampler.hip), so a
# step is grad f_diff plus one launch.  False: (f_diff + g.moreau_envelope(lamb)).grad through the generic operators and
# the step kernel without a g: the A/B partner and cross-check.
_FUSED = True


class _Sampler:
    """Abstract base class for samplers."""

    def samples(self, rng=None, **kwargs):
        """An endless generator: ``next()`` draws the next sample."""
        self._sample_init(rng, **kwargs)

        def _generator():
            while True:
                yield self._sample()

        return _generator()

    def _sample_init(self, rng, **kwargs):
        pass

    def _sample(self):
        raise NotImplementedError


class ULA(_Sampler):
    r"""
    Unadjusted Langevin algorithm (_sampler.py:127-378): samples from ``p(x) ~ exp(-f(x))`` by the chain
    ``x' = x - gamma grad f(x) + sqrt(2 gamma) z``, ``gamma = 0.98 / f.diff_lipschitz`` unless given.

    ``samples(rng=None, x0=...)``: ``x0`` is (..., N), stacked independent chains.  With a ``numpy.random.Generator``
    every step draws ``rng.standard_normal(size=x.shape, dtype=x.dtype)`` on the host and uploads it, exactly the
    reference's stream.  With ``None`` or an ``int`` the noise is made on the device inside the step's launch from
    Philox4x32-10 keyed by (``seed``, ``step``, element): ``seed`` is that int or 64 bits of fresh entropy, ``step`` starts
    at 0 and counts the samples drawn; both are attributes, and setting them (with ``x``) resumes a chain.  Every sample
    is a fresh device array; ``x0`` is not written.
    """

    def __init__(self, f, gamma=None):
        self._f = f
        self._beta = f.diff_lipschitz
        self._gamma = self._set_gamma(gamma)
        self._rng = None
        self.x = None
        self.seed = None
        self.step = 0

    def _sample_init(self, rng, x0):
        self.x = _dev.copy(_dev.require(x0, "x0"))
        self.step = 0
        if rng is None or isinstance(rng, (int, np.integer)):
            self._rng = None
            self.seed = (int(np.random.SeedSequence().entropy) if rng is None else int(rng)) & ((1 << 64) - 1)
        else:
            self._rng, self.seed = rng, None

    def _step_terms(self):
        """(kind, lam, pw, the functional whose gradient the step takes)."""
        return 0, 1.0, 0.0, self._f

    @pxrt.enforce_precision()
    def _sample(self):
        x = self.x
        kind, lam, pw, f = self._step_terms()
        g = _dev.require(f.grad(x), "gradient").reshape(x.shape)
        out = _dev.empty_like(x)
        if self._rng is not None:
            z = self._rng.standard_normal(size=tuple(x.shape), dtype=_dev.scalar_dt(x))
            _dev.langevin_step(kind, self._gamma, lam, pw, x, g, out, noise=_dev.to_device_like(z, x))
        else:
            _dev.langevin_step(kind, self._gamma, lam, pw, x, g, out, seed=self.seed, step=self.step)
        self.step += 1
        self.x = out
        return out

    def objective_func(self):
        """-log p (up to a constant) at the chain's current state: (..., 1)."""
        return copy_if_unsafe(self._f.apply(self.x))

    def _set_gamma(self, gamma=None):
        if gamma is None:
            if math.isfinite(self._beta):
                return pxrt.coerce(0.98 / self._beta)
            raise ValueError("If f has unbounded Lipschitz gradient, the gamma parameter must be provided.")
        try:
            assert gamma > 0
        except Exception:
            raise ValueError(f"gamma must be positive, got {gamma}.")
        return pxrt.coerce(gamma)


class MYULA(ULA):
    r"""
    Moreau-Yosida unadjusted Langevin algorithm (_sampler.py:381-488): samples from ``p(x) ~ exp(-f(x) - g(x))`` with
    ``f`` differentiable and ``g`` proximable, by ULA on ``f + g^lamb``, ``g^lamb`` the Moreau-Yosida envelope.

    ``lamb`` defaults to 1 without ``g``, else to ``min(2, 1 / f.diff_lipschitz)`` (2 when that constant is 0).  The
    Lipschitz constant of the smoothed objective is the sum of the stored constants, ``f.diff_lipschitz + 1 / lamb``.

    For ``g`` one of ``c L1Norm``, ``PositiveOrthant``, ``c PositiveL1Norm`` and ``LInfinityBall(r)`` the envelope's
    gradient is formed inside the step's launch (``clip(x, -c lamb, c lamb) / lamb`` for the first: the Huber form of
    ``L1Norm.moreau_envelope``); any other ``g`` goes through ``g.moreau_envelope(lamb).grad``.
    """

    def __init__(self, f=None, g=None, gamma=None, lamb=None):
        from pyxu_amd.operator.linop import NullFunc

        dim = None
        if f is not None:
            dim = f.dim
        if g is not None:
            if dim is None:
                dim = g.dim
            else:
                assert g.dim == dim
        if dim is None:
            raise ValueError("One of f or g must be nonzero.")
        self._f_diff = NullFunc(dim=dim) if (f is None) else f
        self._g = NullFunc(dim=dim) if (g is None) else g
        self._lambda = self._set_lambda(lamb)
        env = self._g.moreau_envelope(self._lambda)
        f = self._f_diff + env
        f.diff_lipschitz = float(self._f_diff.diff_lipschitz) + float(env.diff_lipschitz)
        super().__init__(f, gamma)

    def _step_terms(self):
        from pyxu_amd.opt.solver.prox_adam import _sub_kind

        plan = _sub_kind(self._g, self._g.dim) if _FUSED else None
        if plan is None:
            return 0, 1.0, 0.0, self._f
        return plan[0], float(self._lambda), float(plan[1]), self._f_diff

    def _set_lambda(self, lamb=None):
        if lamb is None:
            if self._g._name == "NullFunc":
                return pxrt.coerce(1)  # (irrelevant without g, but it must be positive)
            if math.isfinite(dl := self._f_diff.diff_lipschitz):
                return pxrt.coerce(2) if dl == 0 else pxrt.coerce(min(2, 1 / dl))
            raise ValueError("If f has unbounded Lipschitz gradient, the lambda parameter must be provided.")
        return pxrt.coerce(lamb)
