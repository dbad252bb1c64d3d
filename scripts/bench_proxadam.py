#!/usr/bin/env python
"""
Interleaved A/B of the ProxAdam hot path (pyxu_amd/opt/solver/prox_adam.py, csrc/proxadam.hip), in fp32.

    python scripts/bench_proxadam.py [--rounds 5] [--reps 20] [--small] [--only moments,sub,lookahead] [--out FILE]

Per size rows x n (1 x 2^16, 1 x 2^20, 1 x 2^22, 1 x 2^24, 64 x 2^14) one JSON line each for

  moments    the fused moment launch (pxa_proxadam_moments, with the psi output a prox needs) against the `_FUSED = False`
             chain of generic element-wise launches, per variant: HIP events around `reps` back-to-back calls after a
             warm-up, the two sides alternating within a round; `ms` is the median over the rounds, `round_ms` every
             round.  `bytes`: what each side moves, from the shapes (array streams x rows x n x 4); `gbps` from it.
  sub        one outer step's metric-prox sub-problems (g = 0.1 L1Norm, psi uniform in [1, 3]): the batched device
             sub-solve against the per-row PGD loop, host clock around calls that end in a device synchronise; `iters`
             the sub-iteration counts (max over the rows), equal on both sides
  lookahead  the batched sub-solve with 1, 2, 4 and 8 launches enqueued ahead of the host's read of the running-row
             word, same timing

Nothing is timed without an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# array streams (reads + writes per element): fused = g, m, v, vhat, x in and m, v, vhat, x, psi out; chain = every
# launch of _chain_moments (adam: axpby 3, mul 2, axpby 3, clip 2, maximum 3, div 2, sqrt 2, div 2, add 2, div 3, axpby 3)
STREAMS = {"fused": 10, "chain": {"adam": 27, "amsgrad": 21, "padam": 21}}
SIZES = [(1, 2**16), (1, 2**20), (1, 2**22), (1, 2**24), (64, 2**14)]
SMALL = [(1, 2**12), (3, 2**10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal)")
    ap.add_argument("--skip-rows-loop-above", type=int, default=2**24, help="largest rows x n the per-row PGD loop is timed at")
    ap.add_argument("--only", type=lambda s: s.split(","), default=["moments", "sub", "lookahead"],
                    help="comma-separated subset of moments,sub,lookahead")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proxadam_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_proxadam.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.abc as pxa
    import pyxu_amd.operator as pxo
    import pyxu_amd.opt.solver as pxs
    import pyxu_amd.opt.solver.prox_adam as pa
    import pyxu_amd.opt.stop as pxst
    import pyxu_amd.runtime as pxrt
    from pyxu_amd import _dev
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)
    dt = np.float32

    def dev(shape, lo=None, hi=None):
        v = rng.standard_normal(shape) if lo is None else rng.uniform(lo, hi, shape)
        return to_device(v.astype(dt))

    def scalars(t=3, p=0.25):
        b1, b2 = dt(0.9), dt(0.999)
        return dict(b1=b1, omb1=1 - b1, b2=b2, omb2=1 - b2, eps_var=dt(1e-6), c1=1 - b1**t, c2=np.sqrt(1 - b2**t),
                    eps_adam=dt(1e-6), a=dt(0.05), p=dt(p))

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def rounds(fns, timer):
        for fn in fns.values():  # warm-up: every shape and kernel of the timed window
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                res[k].append(round(timer(fn), 4))
        return res

    def emit(out, rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def moments(out, rows, n):
        g, m, x = dev((rows, n)), dev((rows, n)), dev((rows, n))
        v, vh = dev((rows, n), 0.5, 1.5), dev((rows, n), 0.5, 1.5)
        mo, vo, vho, xo, psi = (torch.empty_like(g) for _ in range(5))
        work = _dev.proxadam_workspace(rows, n, g)
        sc = scalars()
        for variant in ("adam", "amsgrad", "padam"):
            code = _dev.PROXADAM_VARIANTS[variant]
            fns = {
                "fused": lambda: _dev.proxadam_moments(code, False, g, m, v, vh, x, mo, vo, vho, xo, psi_out=psi, work=work,
                                                       **sc),
                "chain": lambda: pa._chain_moments(variant, False, g, m, v, vh, x, sc),
            }
            res = rounds(fns, events)
            ms = {k: statistics.median(r) for k, r in res.items()}
            nbytes = {"fused": STREAMS["fused"] * rows * n * 4, "chain": STREAMS["chain"][variant] * rows * n * 4}
            emit(out, {"what": "moments", "variant": variant, "rows": rows, "n": n, "ms": ms, "round_ms": res,
                       "bytes": nbytes, "gbps": {k: round(nbytes[k] / ms[k] * 1e-6, 1) for k in ms},
                       "speedup": round(ms["chain"] / ms["fused"], 2)})

    def sub(out, rows, n):
        f = pxo.SquaredL2Norm(dim=n).asloss(dev((n,)))
        s = pxs.ProxAdam(f, 0.1 * pxo.L1Norm(dim=n), show_progress=False)
        s.fit(x0=dev((rows, n)), a=0.05, stop_crit=pxst.MaxIter(1), mode=pxa.Mode.MANUAL)
        xt, psi = dev((rows, n)), dev((rows, n), 1.0, 3.0)
        # the per-workgroup maxima of psi as pxa_proxadam_moments would have left them in the solver's workspace
        part_max = _dev.proxadam_work_views(s._workspace(rows, n, xt)["work"], rows, n)[0]
        nb = part_max.shape[1]
        c = -(-(-(-n // nb)) // 4) * 4
        host = psi.cpu().numpy().astype(np.float64)
        pm = np.full((rows, nb), -np.inf)
        for b in range(nb):
            if b * c < n:
                pm[:, b] = host[:, b * c: (b + 1) * c].max(axis=-1)
        pm = to_device(pm)
        iters = {}

        def batched(depth):
            def run():
                keep = pa._LOOKAHEAD
                pa._LOOKAHEAD = depth
                try:
                    part_max.copy_(pm)
                    s._sub_problems(xt, psi, rows, n)
                    iters[f"batched{depth}"] = int(s._sub_iters.max())
                finally:
                    pa._LOOKAHEAD = keep
            return run

        def loop():
            s._sub_rows(xt, psi, rows, n)
            iters["rows_loop"] = int(s._sub_iters.max())

        if "sub" in a.only:
            fns = {"batched": batched(pa._LOOKAHEAD)}
            if rows * n <= a.skip_rows_loop_above:
                fns["rows_loop"] = loop
            res = rounds(fns, clock)
            ms = {k: statistics.median(r) for k, r in res.items()}
            emit(out, {"what": "sub", "rows": rows, "n": n, "lookahead": pa._LOOKAHEAD, "ms": ms, "round_ms": res,
                       "iters": dict(iters),
                       "speedup": round(ms["rows_loop"] / ms["batched"], 2) if "rows_loop" in ms else None})
        if "lookahead" in a.only:
            batched(8)()  # (the largest ring of host flag buffers is allocated before anything is timed)
            res = rounds({f"la{d}": batched(d) for d in (1, 2, 4, 8)}, clock)
            emit(out, {"what": "lookahead", "rows": rows, "n": n, "ms": {k: statistics.median(r) for k, r in res.items()},
                       "round_ms": res, "iters": iters.get("batched1")})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out, pxrt.Precision(pxrt.Width.SINGLE):
        if "moments" in a.only:
            for rows, n in (SMALL if a.small else SIZES):
                moments(out, rows, n)
        if "sub" in a.only or "lookahead" in a.only:
            for rows, n in (SMALL if a.small else SIZES):
                sub(out, rows, n)


if __name__ == "__main__":
    main()
