#!/usr/bin/env python
"""
Interleaved A/B of the NLCG iteration tail: the two-launch direction update (pxa_nlcg_direction, `_FUSED = True` in
pyxu_amd/opt/solver/nlcg.py) against the chain of generic row operations (`_FUSED = False`), in fp32.

    python scripts/bench_nlcg.py [--rounds 5] [--iters 20] [--reps 20] [--small] [--out FILE]

Two problems:
  cheap      f = SquaredL2Norm(2^24).asloss(y): f.apply / f.grad are one pass each, so the tail is a large share
  headline   the benchmark's smooth objective 1/2 ||H x - y||^2 + lam env_mu(L21) o Grad at 2048^2 (bench.py
             build_problem, without the positivity constraint)

Per problem and variant (PR, FR) one JSON line with

    iter_ms     {fused, chain}: median over the rounds of the time per NLCG iteration (line search, f.grad,
                direction update, stop check on the published sum g^2), host clock around `iters` iterations that end
                in a device synchronise, after a warm-up fit; the two sides alternate within a round
    tail_ms     {fused, chain}: the direction update alone on fixed g1 / g0 / p, HIP events around `reps` back-to-back
                calls; the chain side includes the <g, p> pass of the next line search, which the fused side's
                partials replace
    round_ms    every round's value per side (the spread between rounds)
    trials      Armijo trials per iteration of the timed fits (the same on both sides)
    tail_bytes  bytes the tail moves per side, from the shapes (elements read + written times 4)
    rel_x       fused against chain final x (sanity check: rounding only)

then the tail alone ("sweep" lines) for one row of 2^14 .. 2^24 entries and for a stack of 8 rows of 2^14 .. 2^21: the
fused side keeps cg.hip's partition of at most 64 workgroups per row, so a long single row cannot fill the device;
`_FUSED_MAX_N` in pyxu_amd/opt/solver/nlcg.py (rows longer than that take the chain) comes from these lines.
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

# array passes (elements read + written per row element) of the tail: fused = dot launch + p launch; chain = sumsq,
# negate, [difference, dot,] axpy_rows, and the next search's <g, p>
PASSES = {"PR": {"fused": 2 + 3, "chain": 1 + 2 + 3 + 2 + 3 + 2}, "FR": {"fused": 1 + 3, "chain": 1 + 2 + 3 + 2}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="2^16 entries and a 128^2 image (a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlcg_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_nlcg.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.abc as pxa
    import pyxu_amd.operator as pxo
    import pyxu_amd.opt.solver as pxs
    import pyxu_amd.opt.solver.nlcg as nlcg_mod
    import pyxu_amd.opt.stop as pxst
    import pyxu_amd.runtime as pxrt
    from bench import build_problem
    from pyxu_amd import _dev
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)

    def cheap():
        n = 2**16 if a.small else 2**24
        y = to_device(rng.standard_normal(n).astype(np.float32))
        x0 = to_device(rng.standard_normal(n).astype(np.float32))
        return f"SquaredL2Norm(2^{int(np.log2(n))}).asloss(y)", pxo.SquaredL2Norm(dim=n).asloss(y), x0, 0.25

    def headline():
        n = 128 if a.small else 2048
        f, _, y = build_problem(n, n, seed=0)
        return f"1/2||Hx-y||^2 + lam env_mu(L21 o Grad), {n}^2", f, _dev.copy(y), float(1.0 / f.diff_lipschitz)

    def fit(f, x0, variant, a0, fused, iters):
        nlcg_mod._FUSED = fused
        nlcg_mod._FUSED_MAX_N = 2**62 if fused else keep_max  # the fused side at every size, default or not
        s = pxs.NLCG(f, show_progress=False)
        s.fit(x0=x0, variant=variant, a0=a0, stop_crit=pxst.MaxIter(iters), mode=pxa.Mode.MANUAL)
        base = int(s._ls_ws.trials.sum()) if s._ls_ws is not None else 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in s.steps():
            pass
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        trials = s._astate["idx"] + int(s._ls_ws.trials.sum()) - base  # one passing trial per search + the failures
        return ms, s.solution(), trials / iters

    def tail_fns(variant, rows, n):
        g1, g0, p = (to_device(rng.standard_normal(rows * n).astype(np.float32)).reshape(rows, n) for _ in range(3))
        gg0 = _dev.row_reduce(_dev.RED_SUMSQ, g0)
        gg_out = torch.empty_like(gg0)
        fb = _dev.HostFlagBuffer(rows, rows, rows)
        work = torch.empty((int(_dev.lib.pxa_nlcg_workspace_bytes(rows)) // 8,), dtype=torch.float64, device="cuda")
        p_new = torch.empty_like(p)
        var = _dev.NLCG_PR if variant == "PR" else _dev.NLCG_FR

        def fused():
            _dev.nlcg_direction(var, False, g1, g0, p, p_new, gg0, gg_out, fb, work)

        def chain():
            _, pn = nlcg_mod._chain_direction(variant.lower(), False, g1, g0, p, gg0)
            _dev.row_reduce(_dev.RED_DOT, g1, pn)

        return {"fused": fused, "chain": chain}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def tail_rounds(variant, rows, n):
        fns = tail_fns(variant, rows, n)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        tl = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                tl[k].append(round(timed(fn), 4))
        return tl

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")
    keep, keep_max = nlcg_mod._FUSED, nlcg_mod._FUSED_MAX_N
    try:
        with pxrt.Precision(pxrt.Width.SINGLE):
            for make in (cheap, headline):
                name, f, x0, a0 = make()
                for variant in ("PR", "FR"):
                    sides = {"fused": True, "chain": False}
                    xs, trials = {}, {}
                    for k, fused in sides.items():  # warm-up: every shape and kernel of the timed window
                        fit(f, x0, variant, a0, fused, 3)
                    it = {k: [] for k in sides}
                    for _ in range(a.rounds):
                        for k, fused in sides.items():
                            ms, xs[k], trials[k] = fit(f, x0, variant, a0, fused, a.iters)
                            it[k].append(round(ms, 4))
                    tl = tail_rounds(variant, 1, x0.numel())
                    rec = {
                        "problem": name, "variant": variant, "n": int(x0.numel()), "iters": a.iters, "rounds": a.rounds,
                        "iter_ms": {k: statistics.median(v) for k, v in it.items()},
                        "tail_ms": {k: statistics.median(v) for k, v in tl.items()},
                        "round_ms": {"iter": it, "tail": tl},
                        "trials": trials,
                        "tail_bytes": {k: int(v * x0.numel() * 4) for k, v in PASSES[variant].items()},
                        "rel_x": float((xs["fused"] - xs["chain"]).norm() / xs["chain"].norm()),
                    }
                    line = json.dumps(rec)
                    print(line, flush=True)
                    out.write(line + "\n")
                    out.flush()
            # the tail alone over the row length (and two stack heights): where the fused side stops winning
            for rows in (1, 8):
                for lg in range(14, (18 if a.small else 25) - (3 if rows == 8 else 0)):
                    for variant in ("PR", "FR"):
                        tl = tail_rounds(variant, rows, 2**lg)
                        rec = {"sweep": "tail", "variant": variant, "rows": rows, "n": 2**lg,
                               "tail_ms": {k: statistics.median(v) for k, v in tl.items()}, "round_ms": tl}
                        line = json.dumps(rec)
                        print(line, flush=True)
                        out.write(line + "\n")
                        out.flush()
    finally:
        nlcg_mod._FUSED, nlcg_mod._FUSED_MAX_N = keep, keep_max
        out.close()


if __name__ == "__main__":
    main()
