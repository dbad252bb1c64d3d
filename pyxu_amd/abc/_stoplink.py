"""
The hand-off between a solver's step, the stopping criteria and the engine (internal).

A solver's math state is a ``SolverState``: a dict of math variables, as in the reference, plus one ``link``
(``StopLink``) through which the step tells the criteria what it already knows or can compute for them, and
through which a criterion tells the next step where to put it.  A criterion called with a plain mapping
(``link_of`` returns None) takes its generic path.
"""
import collections

from pyxu_amd import _dev

__all__ = ["SolverState", "StopLink", "StepStats", "Sink", "Window", "FlagRing", "link_of"]

# a criterion's offer to the next step: fold your epilogue statistics of `var` into `buffer` (in the launch's last
# workgroup with `in_kernel`, else by a fold launch behind it)
Sink = collections.namedtuple("Sink", "var buffer in_kernel")
# a criterion's request to the next step: compute the statistics of the (x, x_prev) pair you read and publish them
# into `buffer` under publication number `seq`
Window = collections.namedtuple("Window", "buffer seq")


class StepStats:
    """What a fused step computed for a RelError check of `var`: per-tile partials of sum (x_new - x_ref)^2 and
    sum x_ref^2 (`rows` rows of `tiles_per_row`), and `folded` = (buffer, seq) when the launch also folded them."""

    __slots__ = ("var", "x_new", "x_ref", "partials", "rows", "tiles_per_row", "folded")

    def __init__(self, var, x_new, x_ref, partials, rows, tiles_per_row, folded=None):
        self.var, self.x_new, self.x_ref, self.partials = var, x_new, x_ref, partials
        self.rows, self.tiles_per_row, self.folded = rows, tiles_per_row, folded


class StopLink:
    """Solver -> criteria: `immutable` (variables whose published tensors the solver never writes: a criterion may
    keep a reference instead of a copy), `window_ok` (the step can serve a `window` request), `rowstat`
    ({var: (tensor, norm, host_rows)}: a row statistic the step already has for that very tensor) and `step_stats`.
    Criteria -> next step: `sink` and `window`."""

    __slots__ = ("immutable", "window_ok", "rowstat", "step_stats", "sink", "window")

    def __init__(self):
        self.reset()

    def reset(self):
        self.immutable, self.window_ok, self.rowstat = frozenset(), False, {}
        self.drop_offers()

    def drop_offers(self):
        """Forget what was offered for one particular step (the state moved: rollback, restore)."""
        self.step_stats = self.sink = self.window = None


class SolverState(dict):
    """A solver's math state: math variables only, plus the `link`."""

    __slots__ = ("link",)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.link = StopLink()

    def clear(self):
        super().clear()
        self.link.reset()


def link_of(state):
    """The StopLink of a solver's state, None for any other mapping (a user's own dict)."""
    return state.link if isinstance(state, SolverState) else None


class FlagRing:
    """`n` host flag buffers of `rows` rows, handed out round-robin: a check's statistics land in one while later
    launches publish into the others."""

    __slots__ = ("rows", "bufs", "_i")

    def __init__(self, rows, n, make=_dev.HostFlagBuffer):
        self.rows, self.bufs, self._i = rows, tuple(make(rows) for _ in range(n)), -1

    @classmethod
    def matching(cls, ring, rows, n, make=_dev.HostFlagBuffer):
        """`ring` if it has this shape (its buffers are reused across checks and runs), else a new one."""
        if ring is not None and ring.rows == rows and len(ring.bufs) == n:
            return ring
        return cls(rows, n, make)

    def take(self):
        self._i = (self._i + 1) % len(self.bufs)
        return self.bufs[self._i]

    def owns(self, buf):
        return any(b is buf for b in self.bufs)

    def after(self, buf):
        """The buffer following `buf` (one of the ring's), wrapping around."""
        i = next(i for i, b in enumerate(self.bufs) if b is buf)
        return self.bufs[(i + 1) % len(self.bufs)]
