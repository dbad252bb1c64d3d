"""CPU-only tests of opt/solver/_recycle.py on torch CPU tensors: which holders `exclusive` sees, and what a Recycler
hands out (the spare, the pool, its cap, its shape / dtype test, the lagged-engine condition, clear())."""
import collections
import weakref

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from torch.utils.dlpack import to_dlpack  # noqa: E402

from pyxu_amd.opt.solver._recycle import Recycler, exclusive  # noqa: E402


def _new(shape=(4, 6), dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


# ------------------------------------------------------------------------------------------------------- exclusive
def test_exclusive_lone_tensor_and_a_second_reference():
    t = _new()
    assert exclusive(t, 1)  # known: the local t
    other = t
    assert not exclusive(t, 1)
    assert exclusive(t, 2)  # (a reference the caller accounts for is no holder)
    del other
    assert exclusive(t, 1)


@pytest.mark.parametrize("view_of", [lambda t: t[0], lambda t: t.reshape(-1)], ids=["t[0]", "t.reshape(-1)"])
def test_exclusive_sees_a_view_from_both_ends(view_of):
    t = _new()
    v = view_of(t)
    assert not exclusive(t, 1)  # the base: the view references it, and shares its storage
    assert not exclusive(v, 1)  # the view itself: its storage is shared
    del v
    assert exclusive(t, 1)


def test_exclusive_sees_a_dlpack_capsule():
    t = _new()
    cap = to_dlpack(t)
    assert not exclusive(t, 1)
    del cap
    assert exclusive(t, 1)


def test_exclusive_sees_a_numpy_alias():
    t = _new()
    a = t.numpy()
    assert not exclusive(t, 1)
    assert isinstance(a, np.ndarray)
    del a
    assert exclusive(t, 1)


def test_exclusive_does_not_see_a_weak_reference():
    """The declared limit: a holder that reaches the tensor only through a weak reference is not seen."""
    t = _new()
    w = weakref.ref(t)
    assert exclusive(t, 1) and w() is t


# --------------------------------------------------------------------------------------------------- take / retire
def _lagged():
    return Recycler({"lag": collections.deque()})  # (the engine state while the lagged loop runs)


def test_retired_exclusive_buffer_is_the_next_one_handed_out():
    r = Recycler()
    t, like = _new(), _new()
    r.retire(t, 1)
    assert r.take(like) is t
    assert r.take(like) is not t  # (handed out once)


def test_retired_buffer_that_starts_where_alias_does_is_not_kept():
    r = Recycler()
    t = _new()
    r.retire(t, 1, alias=t)
    assert r.take(t) is not t


def test_buffer_in_avoid_is_never_handed_out():
    for r in (Recycler(), _lagged()):
        t = _new()
        r.retire(t, 1, pool=True)
        assert r.take(t, t) is not t
        r.retire(t, 1, pool=True)
        assert r.take(t, None, t) is not t
    # a pooled buffer that has become exclusive but is the step's own input
    r = _lagged()
    t = _new()
    holder = t
    r.retire(t, 1, pool=True)
    del holder
    assert r.take(t, t) is not t
    assert r.take(t, None, t) is not t


def test_held_buffer_waits_in_the_pool_until_its_holder_is_dropped():
    r = _lagged()
    t, like = _new(), _new()
    holder, ptr = t, t.data_ptr()
    r.retire(t, 1, pool=True)
    del t
    assert r.take(like).data_ptr() != ptr  # still held: a new buffer
    del holder
    out = r.take(like)
    assert out.data_ptr() == ptr
    assert r.take(like).data_ptr() != ptr  # (it left the pool)


def test_held_buffer_retired_without_pooling_is_dropped():
    r = _lagged()
    t = _new()
    holder, w = t, weakref.ref(t)
    r.retire(t, 1)
    del t, holder
    assert w() is None


def test_the_17th_pooled_buffer_evicts_the_oldest():
    r = _lagged()
    like = _new()
    holders = [_new() for _ in range(17)]
    ptrs = [t.data_ptr() for t in holders]
    first = weakref.ref(holders[0])
    for t in holders:
        r.retire(t, 1, pool=True)  # (held by the list)
    del t
    keep_first_allocated = holders[0].untyped_storage()  # (its address is not given to a later buffer)
    del holders
    assert first() is None  # the pool dropped the oldest
    got = [r.take(like) for _ in range(17)]
    assert [t.data_ptr() for t in got[:16]] == ptrs[1:]  # the other 16, oldest first
    assert got[16].data_ptr() not in ptrs
    del keep_first_allocated


@pytest.mark.parametrize("other", [dict(shape=(3, 8)), dict(dtype=torch.float64)], ids=["shape", "dtype"])
def test_pooled_buffer_of_another_shape_or_dtype_is_skipped(other):
    r = _lagged()
    like = _new()
    odd, same = _new(**other), _new()
    odd_ptr, same_ptr = odd.data_ptr(), same.data_ptr()
    held = [odd, same]
    r.retire(odd, 1, pool=True)
    r.retire(same, 1, pool=True)
    del odd, same, held
    assert r.take(like).data_ptr() == same_ptr  # the first pooled buffer is skipped
    assert r.take(like).data_ptr() not in (odd_ptr, same_ptr)
    assert r.take(_new(**other)).data_ptr() == odd_ptr  # (it waited for a request like it)


@pytest.mark.parametrize("engine", [None, {}, {"lag": None}], ids=["no_engine", "no_lag_entry", "lag_none"])
def test_nothing_is_pooled_without_a_running_lagged_engine(engine):
    r = Recycler(engine)
    t = _new()
    holder, w, ptr = t, weakref.ref(t), t.data_ptr()
    r.retire(t, 1, pool=True)
    del t
    assert r.take(holder).data_ptr() != ptr
    del holder
    assert w() is None


def test_pool_is_emptied_when_the_lagged_engine_has_ended():
    engine = {"lag": collections.deque()}
    r = Recycler(engine)
    a, b = _new(), _new()
    ha, hb, wa = a, b, weakref.ref(a)
    r.retire(a, 1, pool=True)
    del engine["lag"]
    r.retire(b, 1, pool=True)
    del a, b, ha, hb
    assert wa() is None


def test_clear_empties_the_spare_and_the_pool():
    r = _lagged()
    spare, pooled = _new(), _new()
    holder = pooled
    ws, wp = weakref.ref(spare), weakref.ref(pooled)
    r.retire(pooled, 1, pool=True)
    r.retire(spare, 1, pool=True)
    r.clear()
    del spare, pooled, holder
    assert ws() is None and wp() is None
    like = _new()
    assert r.take(like) is not like
