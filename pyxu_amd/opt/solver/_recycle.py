"""
Output-buffer reuse of the fused solver steps (PGD, Condat-Vu, PD3O).

The reference allocates a fresh array for every iterate.  The fused steps overwrite an iterate that has left the
solver state instead, but only when nothing else can still reach it: an item of ``steps()``, the ``x`` of ``stats()``, a
user's ``x0`` / ``z0``, a view such as ``batch[i]``, a stop criterion that borrowed ``x`` (``link.immutable``) or a check
state the lagged engine holds.  `exclusive` is the one place that decides it; a `Recycler` keeps what may be written next.
"""
import sys

from pyxu_amd import _dev

__all__ = ["exclusive", "Recycler"]

# References a call of a Python function adds to an argument the caller passes from a local of its own: the callee's
# parameter, and before CPython 3.11 the caller's evaluation stack as well, which keeps the argument for the length
# of the call (from 3.11 on it is handed over to the parameter).
_CALL = 1 if sys.version_info >= (3, 11) else 2


def exclusive(t, known):
    """True iff nothing but the caller can reach tensor `t`, so that it may be overwritten.

    `known` is the number of references to `t` the caller accounts for itself: each of its own locals, each
    solver-state or list entry, what an engine token holds.  The Python count seen here is `known` + _CALL for this
    call + 1 for getrefcount's argument.  A function that passes `t` on from a parameter of its own adds _CALL for
    itself (`known + _CALL`).  The comparison is exact: a count below it would mean the caller overstated `known`.

    Any further Python reference raises the count: a second name, a ``to_dlpack`` capsule, a view (it references its
    base).  A view or a ``.numpy()`` alias also raises the storage's use count, which fails the view itself as well.
    A weak reference raises neither: a holder that reaches `t` only through one is not seen."""
    return sys.getrefcount(t) == known + _CALL + 1 and _dev.storage_exclusive(t)


class Recycler:
    """Retired iterates of one shape and dtype.  The spare is a retired iterate nothing else references: the next output
    buffer.  The pool holds retired iterates something still references (the lagged engine's check states keep every
    iterate of the last few steps, and each step would allocate): they are reused once they have become exclusive."""

    __slots__ = ("_spare", "_pool", "_engine")
    POOL_MAX = 16

    def __init__(self, engine=None):
        """`engine`: the solver's engine state; buffers wait in the pool only while its lagged loop runs (its "lag"
        entry).  None: never."""
        self._spare = None
        self._pool = []
        self._engine = engine

    def take(self, like, a=None, b=None):
        """An output buffer shaped as `like` that is neither `a` nor `b`: the spare, else a pooled buffer that has
        become exclusive, else a new one."""
        out, self._spare = self._spare, None
        if out is not None and out is not a and out is not b:
            return out
        pool = self._pool
        for i in range(len(pool)):
            c = pool[i]
            # known: the pool's entry and c (most entries are still held: the count rejects them first)
            if exclusive(c, 2) and c is not a and c is not b and c.shape == like.shape and c.dtype == like.dtype:
                del pool[i]
                return c
        return _dev.empty_like(like)

    def retire(self, t, known, alias=None, pool=False):
        """`t` has just left the state and the caller holds `known` references to it: the spare iff it is exclusive
        (and does not start where `alias` does).  Else, with `pool`, it waits in the pool (the newest POOL_MAX)."""
        if exclusive(t, known + _CALL) and (alias is None or t.data_ptr() != alias.data_ptr()):
            self._spare = t
            return
        self._spare = None
        if not pool:
            return
        held = self._pool
        if self._engine is None or self._engine.get("lag") is None:  # (emptied when the lagged loop has ended)
            held.clear()
            return
        held.append(t)
        if len(held) > self.POOL_MAX:
            del held[0]

    def clear(self):
        self._spare = None
        self._pool.clear()
