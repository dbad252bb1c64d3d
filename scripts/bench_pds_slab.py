"""Cost of the ghost handling of the slab step, without communication (one GPU).

Times the slab form of the fused PD3O / Condat-Vu iteration (pxa_pds_slab_primal + pxa_pds_slab_dual) on an INTERIOR
slab of nl x n x n planes (ghosts on both sides, the ghost buffers filled once) against pxa_pds_step on an nl x n x n
volume: the same planes and voxels, the same three kernels; the slab step additionally marches and reads the
2 R0 ghost planes per side.  Both are timed with HIP events over K back-to-back calls in alternating rounds of one
process, on random data; one JSON line per algorithm with the per-round times, their medians and the ratio.

S = Gaussian(sigma = 2) truncated at 3 sigma (13 taps per axis, R0 = 6), K = Gradient, h = lam L1, g = none, fp32:
the C3 configuration of scripts/bench_pds.py.  Env: PXA_NL (planes, default 128), PXA_N (in-plane edge, default
1024), PXA_STEPS (calls per round, default 10), PXA_ROUNDS (default 5).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pyxu_amd import _dev


def main():
    nl = int(os.environ.get("PXA_NL", "128"))
    n = int(os.environ.get("PXA_N", "1024"))
    steps = int(os.environ.get("PXA_STEPS", "10"))
    rounds = int(os.environ.get("PXA_ROUNDS", "5"))
    R0 = 6
    t = np.arange(-R0, R0 + 1)
    k = np.exp(-t.astype(np.float64) ** 2 / 8.0)
    k = (k / k.sum()).astype(np.float32)
    taps = [(list(map(int, t)), [float(v) for v in k])] * 3
    c0, c1 = [-1.0] * 3, [1.0] * 3
    tau, sigma, rho, lam = 0.9, 0.09, 1.0, 0.01
    pre = _dev.pds_args(1, 1, nl, n, n, 3, taps, c0, c1, tau, sigma, rho, lam, 0, 0.0, 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *sh: torch.rand(sh, device="cuda", dtype=torch.float32, generator=g) - 0.5  # noqa: E731
    x, u, hty = rnd(1, nl, n, n), rnd(1, nl, n, n), rnd(1, nl, n, n)
    z = 0.02 * rnd(1, 3, nl, n, n)
    xo, uo, q, w = (torch.empty_like(x) for _ in range(4))
    zo = torch.empty_like(z)
    gh = {a: dict(src_lo=rnd(1, 2 * R0, n, n), src_hi=rnd(1, 2 * R0, n, n),
                  z_lo=0.02 * (rnd(1, 3, 2 * R0 + 1, n, n) if a == 0 else rnd(1, 1, n, n)),
                  z_hi=0.02 * rnd(1, 3, 2 * R0, n, n) if a == 0 else None) for a in (0, 1)}
    w_hi = rnd(1, 1, n, n)

    def slab(a):
        _dev.pds_slab_primal(a, pre, x, u if a == 0 else None, z, hty, xo, uo if a == 0 else None, q, w, **gh[a])
        _dev.pds_slab_dual(w, z, (1, nl, n, n, 3), c0, c1, sigma, lam, rho, 0, relax=a, w_hi=w_hi, out=zo)

    def whole(a):
        _dev.pds_step(a, pre, x, u if a == 0 else None, z, hty, xo, uo if a == 0 else None, zo, q, w)

    def timed(fn, a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn(a)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for a, name in ((0, "pd3o"), (1, "cv")):
        for fn in (slab, whole):  # warm-up: code objects, clocks
            for _ in range(3):
                fn(a)
        torch.cuda.synchronize()
        ts, tw = [], []
        for _ in range(rounds):
            ts.append(timed(slab, a))
            tw.append(timed(whole, a))
        ms, mw = float(np.median(ts)), float(np.median(tw))
        ghost_planes = 4 * R0 + (4 * R0 * 3 + 1 if a == 0 else 1) + 1  # u / x, z, w planes read beyond the slab
        print(json.dumps({"algo": name, "nl": nl, "n": n, "steps": steps, "slab_ms": [round(v, 3) for v in ts],
                          "whole_ms": [round(v, 3) for v in tw], "slab_ms_median": round(ms, 3),
                          "whole_ms_median": round(mw, 3), "ratio_slab_over_whole": round(ms / mw, 4),
                          "ghost_planes_read": ghost_planes}), flush=True)


if __name__ == "__main__":
    main()
