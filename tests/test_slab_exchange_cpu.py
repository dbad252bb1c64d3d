"""
The ghost exchange of the slab solvers (pyxu_amd.distributed.ghost_exchange) on gloo worlds of 2 and 3 processes with
host tensors, and the slab case of the PD3O / Condat-Vu pattern matcher on host-constructed operators.
"""
import numpy as np
import pytest

import pyxu_amd.operator as pxo
import pyxu_amd.runtime as pxrt

torch = pytest.importorskip("torch")

import _slab_workers as sw  # noqa: E402
import pyxu_amd.distributed as pd  # noqa: E402


@pytest.mark.parametrize("world", [2, 3])
def test_ghost_exchange_matches_global_planes(world):
    shape, lo, hi, stack = (17, 3, 5), 5, 4, 2  # unequal depths (2 R0 + 1, 2 R0) at R0 = 2, stack = 2
    res = sw.spawn("ghost_exchange_host", world=world, shape=shape, lo=lo, hi=hi, stack=stack)
    for k, seed in enumerate((0, 1)):  # fresh buffers / a non-contiguous input into preallocated buffers
        G = sw.global_array(shape, stack, seed)
        for r in range(world):
            a, b = pd.shard_range(shape[0], r, world)
            got_lo, got_hi = res[r][f"lo{k}"], res[r][f"hi{k}"]
            if r == 0:
                assert isinstance(got_lo, str) and got_lo == "none"  # the volume's first slab
            else:
                np.testing.assert_array_equal(got_lo, G[:, a - lo:a])
            if r == world - 1:
                assert isinstance(got_hi, str) and got_hi == "none"
            else:
                np.testing.assert_array_equal(got_hi, G[:, b:b + hi])
    M = shape[1] * shape[2]
    for r in range(world):
        want = ["none" if r == 0 else (stack, lo, M), "none" if r == world - 1 else (stack, hi, M)]
        assert res[r]["buffers"] == want


def test_ghost_exchange_single_process_has_no_neighbours():
    x = torch.zeros((2, 6, 4))
    assert pd.ghost_exchange(x, 3, 2) == (None, None)
    assert pd.ghost_buffers(x, 3, 2) == (None, None)


def test_thin_slab_raises_on_every_rank():
    # 7 planes over 3 ranks: 3 / 2 / 2; depth 3 fits rank 0's own slab but not its neighbour's
    res = sw.spawn("ghost_thin_host", world=3, n0=7, lo=3, hi=1)
    assert [res[r]["nl"] for r in range(3)] == [3, 2, 2]
    for r in range(3):
        assert res[r]["raised"] is not None and "thinner" in res[r]["raised"], r
    res = sw.spawn("ghost_thin_host", world=3, n0=7, lo=2, hi=2)  # the deepest legal ghost
    assert all(res[r]["raised"] is None for r in range(3))


class _Group:
    """Stand-in for a process group of 3 ranks seen from rank 1 (the matcher only asks for rank and size)."""


def _slab_problem(monkeypatch, world, shape=(17, 9, 11), k_shape=None, k_group=None, halo=(2, 2), h_shape=None):
    monkeypatch.setattr(pd, "world", lambda group=None: (min(1, world - 1), world))
    e = sw.entry(shape)
    import _asym_cases as ac

    blur = lambda sh: pxo.Stencil(**{**ac.blur_of(e, np.float32), "arg_shape": sh})  # noqa: E731
    grad = lambda sh: pxo.Gradient(**{**ac.grad_kw(e), "arg_shape": sh})  # noqa: E731
    H = pd.SlabLinOp(blur, shape, halo)
    K = pd.SlabLinOp(grad, shape if k_shape is None else k_shape, (0, 1), group=k_group)
    nl = H._nl
    N = nl * shape[1] * shape[2]
    f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(torch.zeros(N)) * H
    lsh = (nl, *shape[1:]) if h_shape is None else h_shape
    return f, K, 0.05 * pxo.L21Norm(arg_shape=(3, *lsh)), torch.zeros(N), nl


def test_matcher_slab_plan(monkeypatch):
    from pyxu_amd.opt.solver._fused import match_pds_deblur

    with pxrt.Precision(pxrt.Width.SINGLE):
        f, K, h, x0, nl = _slab_problem(monkeypatch, 3)
        p = match_pds_deblur(f, None, h, K, x0)
        assert p is not None and p["slab"]["world"] == 3 and p["slab"]["rank"] == 1
        assert (p["n0"], p["n1"], p["n2"], p["D"]) == (nl, 9, 11, 3) and p["slab"]["nl"] == nl == 6
        assert p["slab"]["n_global"] == 17 and max(abs(o) for o in p["taps"][0][0]) == 2
        # h = lam L1 on the slab's layout
        p = match_pds_deblur(f, pxo.PositiveOrthant(dim=x0.numel()), 0.05 * pxo.L1Norm(dim=3 * x0.numel()), K, x0)
        assert p is not None and p["h_kind"] == 0 and p["prox"] == 1 and "slab" in p
        # a world of one process: the plain plan on the whole volume
        f1, K1, h1, x1, _ = _slab_problem(monkeypatch, 1)
        p1 = match_pds_deblur(f1, None, h1, K1, x1)
        assert p1 is not None and "slab" not in p1 and p1["n0"] == 17


def test_matcher_slab_fallbacks(monkeypatch):
    from pyxu_amd.opt.solver._fused import match_pds_deblur

    with pxrt.Precision(pxrt.Width.SINGLE):
        # mismatched global shapes between f's operator and K (same slab size)
        f, K, h, x0, _ = _slab_problem(monkeypatch, 3, k_shape=(18, 9, 11))
        assert K._nl == 6 and match_pds_deblur(f, None, h, K, x0) is None
        # mismatched groups
        f, K, h, x0, _ = _slab_problem(monkeypatch, 3, k_group=_Group())
        assert match_pds_deblur(f, None, h, K, x0) is None
        # a halo that does not cover the axis-0 reach of the stencil
        f, K, h, x0, _ = _slab_problem(monkeypatch, 3, halo=(2, 1))
        assert match_pds_deblur(f, None, h, K, x0) is None
        # h on the global layout instead of the slab's
        f, K, h, x0, _ = _slab_problem(monkeypatch, 3, h_shape=(17, 9, 11))
        assert match_pds_deblur(f, None, h, K, x0) is None
        # only one of the two operators is a slab operator
        f, K, h, x0, nl = _slab_problem(monkeypatch, 3)
        import _asym_cases as ac

        Kp = pxo.Gradient(**{**ac.grad_kw(sw.entry()), "arg_shape": (nl, 9, 11)})
        assert match_pds_deblur(f, None, h, Kp, x0) is None
