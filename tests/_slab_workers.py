"""
Worker bodies of the slab-solver and ghost-exchange tests (test_slab_exchange_cpu.py, test_gpu_slab_solver.py): one
process per rank over gloo on 127.0.0.1, GPU scenarios sharing cuda:0.  A module of its own because `run` looks a
scenario up in its own globals (as _dist_workers.run does).
"""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _dist_workers import _init  # noqa: E402

SHAPE = (17, 9, 11)
# per-axis (raw taps, centre): off-centre, signed, different on every axis; axis-0 reach 2
AXES = [([.2, .5, -.1, .2], 2), ([.1, -.2, .3, .4], 3), ([.2, .4, .1, -.2, .1], 1)]
SAMPLING = (1.9, 1.3, 0.7)
LAM = 0.05


def run(rank, world, port, scenario, q, kwargs):
    """One scenario; a failure is reported to the parent and nothing further is started."""
    try:
        dist = _init(rank, world, port, "gloo")
        out = globals()[scenario](rank, world, **dict(kwargs))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # pragma: no cover - reported by the parent
        q.put((rank, {"error": traceback.format_exc()}))


def spawn(scenario, world=2, **kwargs):
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=run, args=(r, world, port, scenario, q, kwargs)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, out = q.get(timeout=240)
        res[r] = out
    for p in procs:
        p.join(timeout=60)
    for r, out in res.items():
        assert "error" not in out, out.get("error")
    return res


# ------------------------------------------------------------------ CPU scenarios
def global_array(shape, stack, seed=0):
    n0 = shape[0]
    M = int(np.prod(shape[1:]))
    return np.random.default_rng(seed).standard_normal((stack, n0, M))


def ghost_exchange_host(rank, world, shape, lo, hi, stack):
    """ghost_exchange on host tensors: fresh buffers, preallocated buffers refilled, a non-contiguous input."""
    import torch

    import pyxu_amd.distributed as pd

    a, b = pd.shard_range(shape[0])
    out = {}
    bufs = None
    for k, seed in enumerate((0, 1)):
        G = global_array(shape, stack, seed)
        x = torch.from_numpy(G[:, a:b].copy())
        if k == 0:
            got = pd.ghost_exchange(x, lo, hi, n_global=shape[0])
            bufs = pd.ghost_buffers(x, lo, hi)
        else:  # a permuted view of a (nl, S, M) array, into the preallocated buffers
            xn = torch.from_numpy(np.ascontiguousarray(G[:, a:b].transpose(1, 0, 2))).permute(1, 0, 2)
            assert not xn.is_contiguous() or stack == 1
            got = pd.ghost_exchange(xn, lo, hi, out=bufs)
            assert all(g is None or g is bf for g, bf in zip(got, bufs))
        out[f"lo{k}"], out[f"hi{k}"] = ("none" if g is None else g.numpy().copy() for g in got)
    out["buffers"] = ["none" if t is None else tuple(t.shape) for t in bufs]
    return out


def ghost_thin_host(rank, world, n0, lo, hi):
    import torch

    import pyxu_amd.distributed as pd

    a, b = pd.shard_range(n0)
    x = torch.zeros((1, b - a, 4), dtype=torch.float64)
    try:
        pd.ghost_exchange(x, lo, hi, n_global=n0)
    except ValueError as e:
        return dict(raised=str(e), nl=b - a)
    return dict(raised=None, nl=b - a)


# ------------------------------------------------------------------ GPU scenarios
def entry(shape=SHAPE, name="slab17"):
    import _asym_cases as ac

    return ac._e(name, shape, AXES, SAMPLING, "iso", "pos", np.float32)


def _build(e, dt, sharded, algo, g_kind="pos", h_kind="iso"):
    """(solver, local slice, nl) of the entry's problem: slab operators on this rank, or the unsharded operators."""
    import _asym_cases as ac
    import pyxu_amd.distributed as pd
    import pyxu_amd.operator as pxo
    import pyxu_amd.opt.solver as pxs
    from pyxu_amd.util import to_device

    shape = e.shape
    M = int(np.prod(shape[1:]))
    y, x0 = ac.data(e, dt)
    blur = lambda sh: pxo.Stencil(**{**ac.blur_of(e, dt), "arg_shape": sh})  # noqa: E731
    grad = lambda sh: pxo.Gradient(**{**ac.grad_kw(e), "arg_shape": sh})  # noqa: E731
    if sharded:
        a, b = pd.shard_range(shape[0])
        H, K = pd.SlabLinOp(blur, shape, (2, 2)), pd.SlabLinOp(grad, shape, (0, 1))
    else:
        a, b = 0, shape[0]
        H, K = blur(shape), grad(shape)
    nl = b - a
    sl = slice(a * M, b * M)
    f = 0.5 * pxo.SquaredL2Norm(dim=nl * M).asloss(to_device(y[sl].copy())) * H
    f.diff_lipschitz = 1.0
    lsh = (nl, *shape[1:])
    h = LAM * (pxo.L21Norm(arg_shape=(3, *lsh)) if h_kind == "iso" else pxo.L1Norm(dim=3 * nl * M))
    g = {"none": None, "pos": pxo.PositiveOrthant(dim=nl * M), "l1": ac.G_L1 * pxo.L1Norm(dim=nl * M)}[g_kind]
    cls = {"pd3o": pxs.PD3O, "cv": pxs.CondatVu}[algo]
    return cls(f=f, g=g, h=h, K=K, show_progress=False), to_device(x0[sl].copy()), nl


def gpu_slab_solver(rank, world, algo, steps, fused=True, iters=40, eps=3e-2, shape=SHAPE):
    """PD3O / Condat-Vu on slab operators vs the unsharded fused solver (run in rank 0).  eps: the relative change of
    x per iteration falls from about 0.1 to 0.01 over the first 40 iterations (CPU oracle), so the global RelError
    decides the stop between iterations 15 and 20."""
    import torch

    torch.cuda.set_device(0)
    import pyxu_amd.distributed as pd
    import pyxu_amd.opt.stop as pxst
    import pyxu_amd.runtime as pxrt
    from pyxu_amd.util import to_NUMPY

    dt = np.float32
    e = entry(shape)
    M = int(np.prod(shape[1:]))
    kw = dict(tau=0.9, sigma=0.04) if steps == "explicit" else {}
    out = {}
    with pxrt.Precision(pxrt.Width.SINGLE):
        s, x0, nl = _build(e, dt, True, algo)
        crit = pxst.MaxIter(iters) if not fused else (pxst.MaxIter(iters) | pd.ShardedRelError(eps=eps))
        s.fit(x0=x0, stop_crit=crit, fused=fused, **kw)
        p = s._plan
        out.update(plan=None if p is None else ("slab" if "slab" in p else "plain"),
                   la=None if p is None else bool(p["la"]),
                   it=int(s.stats()[1]["iteration"][-1]),
                   steps=[float(s._mstate[k]) for k in ("tau", "sigma", "rho")])
        xl = s._mstate["x"].reshape(nl, M)
        out["x"] = to_NUMPY(pd.gather_slabs(xl, shape[0])).reshape(-1)
        if rank == 0 and fused:
            r, x0f, _ = _build(e, dt, False, algo)
            r.fit(x0=x0f, stop_crit=pxst.MaxIter(iters) | pxst.RelError(eps=eps), **kw)
            assert r._plan is not None
            out.update(x_ref=to_NUMPY(r._mstate["x"]), it_ref=int(r.stats()[1]["iteration"][-1]),
                       steps_ref=[float(r._mstate[k]) for k in ("tau", "sigma", "rho")])
    return out


def gpu_slab_thin(rank, world, algo):
    """(7, 9, 11) over 3 ranks: slabs of 3 / 2 / 2 planes, thinner than the 2 R0 (+ 1) ghost planes."""
    import torch

    torch.cuda.set_device(0)
    import pyxu_amd.opt.stop as pxst
    import pyxu_amd.runtime as pxrt

    with pxrt.Precision(pxrt.Width.SINGLE):
        s, x0, nl = _build(entry((7, 9, 11), "slab7"), np.float32, True, algo)
        try:
            s.fit(x0=x0, stop_crit=pxst.MaxIter(2))
        except ValueError as e:
            return dict(raised=str(e), nl=nl)
    return dict(raised=None, nl=nl)
