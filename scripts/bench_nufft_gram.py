#!/usr/bin/env python
"""
Measure the Toeplitz gram of a type-2 NUFFT (NUFFT.type2(..).gram(): pxa_toeplitz_apply, or the chain of existing
kernels on the full padded grid) against the composition A.adjoint(A.apply(u)) of the gridded operator, in fp32.

    python scripts/bench_nufft_gram.py [--rounds 5] [--reps 20] [--small] [--out FILE]

Workloads: the two of DESIGN.md §8i (N = 256^2, M = 65536; N = 64^3, M = 2^20) and a 1-D one (N = 4096, M = 65536),
each with a stack of Q = 1 and Q = 8, then larger ones at Q = 1, M = 2^20: N = 512^2, 1024^2, 2048^2 (the fused
kernel keeps 4, 2, 1 lines of the strided axis per workgroup) and N = 128^3; the padded grids of the last two are
128 MB.  Per workload one JSON line with

    P                         cells per axis of the circular convolution
    fused_ms                  G.apply, pxa_toeplitz_apply (1 / 3 / 5 launches)
    fallback_ms               G.apply, embed + FFT + product + inverse FFT + extract on the padded grid
    compose_ms                {eps: A.adjoint(A.apply(u))} of the gridded operator at eps = 1e-4 and 1e-6
    round_ms                  every round's time per side (the spread between rounds)
    plan_s                    one-off: the type-1 transform of the weights onto 2 N - 1 modes (eps = 1e-6, host plan
                              included), its FFT and the check of the spectrum, by the host clock
    rel_fused_vs_fallback, rel_fused_vs_compose   norm-wise distances (sanity checks: rounding, and about eps)

All times but plan_s are HIP-event times of `reps` back-to-back calls after a warm-up call; the sides alternate within
a round and the median over the rounds is reported.
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

EPS = (1e-4, 1e-6)
PSF_EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="1/4 of the modes per axis, 1/16 of the points (a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nufft_gram_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_nufft_gram.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.operator as pxo
    import pyxu_amd.runtime as pxrt
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def rounds(fns):
        """ms per round of each callable: a warm-up call each, then `rounds` rounds in which they alternate."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(round(timed(fn), 4))
        return t

    def rel(p, q):
        return float((p - q).norm() / q.norm())

    def measure(x, N, Q):
        ops = {eps: pxo.NUFFT.type2(x, N, isign=1, eps=eps, method="grid") for eps in EPS}
        A = ops[PSF_EPS]
        fused, fallback = A.gram(fused=True), A.gram(fused=False)
        u = to_device(rng.standard_normal((Q, A.dim)).astype(np.float32))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fused._plan()
        torch.cuda.synchronize()
        plan_s = time.perf_counter() - t0
        fns = {"fused": lambda: fused.apply(u), "fallback": lambda: fallback.apply(u)}
        for eps, op in ops.items():
            fns[f"compose_{eps:g}"] = (lambda op: lambda: op.adjoint(op.apply(u)))(op)
        t = rounds(fns)
        med = {k: round(statistics.median(v), 4) for k, v in t.items()}
        ref = A.adjoint(A.apply(u))
        return dict(D=len(N), N=list(N), M=x.shape[0], Q=Q, P=list(fused._P), fused_ms=med["fused"],
                    fallback_ms=med["fallback"], compose_ms={f"{e:g}": med[f"compose_{e:g}"] for e in EPS}, round_ms=t,
                    plan_s=round(plan_s, 3), rel_fused_vs_fallback=rel(fused.apply(u), fallback.apply(u)),
                    rel_fused_vs_compose=rel(fused.apply(u), ref))

    s = 4 if a.small else 1
    lines = []
    with pxrt.Precision(pxrt.Width.SINGLE):
        x2 = rng.uniform(-np.pi, np.pi, size=(65536 // (s * s), 2)).astype(np.float32)
        x3 = rng.uniform(-np.pi, np.pi, size=((1 << 20) // (s * s), 3)).astype(np.float32)
        x1 = rng.uniform(-np.pi, np.pi, size=(65536 // (s * s), 1)).astype(np.float32)
        work = [("N256x256_M65536", x2, (256 // s,) * 2), ("N64x64x64_M1048576", x3, (64 // s,) * 3),
                ("N4096_M65536", x1, (4096 // s,))]
        # padded grids of 128 MB, beyond the L2s: P = 4096^2 and 256^3 (the kernel t is gridded on 8192^2 / 512^3)
        # and the 2-D sizes between: the fused kernel holds 8 / 4 / 2 / 1 lines of P = 512 / 1024 / 2048 / 4096 cells
        x2b = x3[:, :2].copy()
        big = [("N512x512_M1048576", x2b, (512 // s,) * 2), ("N1024x1024_M1048576", x2b, (1024 // s,) * 2),
               ("N2048x2048_M1048576", x2b, (2048 // s,) * 2), ("N128x128x128_M1048576", x3, (128 // s,) * 3)]
        for name, x, N, Qs in [(*w, (1, 8)) for w in work] + [(*b, (1,)) for b in big]:
            for Q in Qs:
                lines.append(json.dumps(dict(workload=name, small=bool(a.small), **measure(x, N, Q))))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
