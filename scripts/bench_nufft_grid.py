#!/usr/bin/env python
"""
Measure the gridding NUFFT (NUFFT.type1 / type2 with method="grid": pxa_nufft_spread / pxa_nufft_interp /
pxa_nufft_deconv around pxa_fft_ex) against the exact transform on the same inputs (pxa_nudft), in fp32.

    python scripts/bench_nufft_grid.py [--rounds 5] [--reps 3] [--small] [--no-sweep] [--out FILE]

Workloads: the three of scripts/bench_nudft.py (type 2, N = 256^2, M = 65536, Q = 1 and Q = 8; type 1, N = 64^2,
M = 2^20) and one in three dimensions (type 1, N = 64^3, M = 2^20), each at eps = 1e-2, 1e-4 and 1e-6.  Per workload
and eps, one JSON line with

    w, nf                   kernel width and fine grid
    stage_ms                spread, interp, fft, deconv (extract), deconv (embed): each stage alone
    apply_ms / adjoint_ms   the operator's whole chains, Python launches included
    direct_apply_ms / direct_adjoint_ms   pxa_nudft on the same points, modes and weights
    rel_diff                norm-wise distance of the gridded apply from the exact one (a sanity check)

Then the crossover sweep: D = 1, 2, 3 at eps = 1e-4 and 1e-6, M prod(N) = 2^20 .. 2^32 in factors of 4 (M and
prod(N) both about the square root), gridded apply and adjoint against the exact ones; the crossover is the smallest
tested M prod(N) from which, for every D and eps, both gridded directions are faster at that size and every larger
tested one.  All times are HIP-event times of `reps` back-to-back calls after a warm-up call; the two sides alternate
within a round and the median over the rounds is reported.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS = (1e-2, 1e-4, 1e-6)
SWEEP_EPS = (1e-4, 1e-6)
SWEEP_LOG2 = (20, 22, 24, 26, 28, 30, 32)


def sweep_shape(D, log2_pairs):
    """(N, M) with M prod(N) ~ 2^log2_pairs and prod(N) ~ M."""
    side = max(2, int(round(2.0 ** (log2_pairs / 2.0 / D))))
    N = (side,) * D
    return N, max(1, (1 << log2_pairs) // int(np.prod(N)))


def crossover(rows, floor=1 << 20):
    """Smallest tested pair count from which every (D, eps) has both gridded directions faster, there and above."""
    sizes = sorted({r["log2_pairs"] for r in rows})
    good = None
    for s in reversed(sizes):
        here = [r for r in rows if r["log2_pairs"] == s]
        if all(r["apply_ms"] < r["direct_apply_ms"] and r["adjoint_ms"] < r["direct_adjoint_ms"] for r in here):
            good = 1 << s
        else:
            break
    return None if good is None else max(good, floor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="1/16 of the points and modes (a rehearsal, not a measurement)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nufft_grid_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_nufft_grid.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.operator as pxo
    import pyxu_amd.runtime as pxrt
    from pyxu_amd import _dev
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)

    def timed(fn, reps=None):
        reps = a.reps if reps is None else reps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def medians(fns, reps=None):
        """Median ms of each callable: a warm-up call each, then `rounds` rounds in which they alternate."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, reps))
        return {k: round(statistics.median(v), 4) for k, v in t.items()}

    def operators(typ, x, N, eps):
        make = pxo.NUFFT.type1 if typ == 1 else pxo.NUFFT.type2
        grid = make(x, N, isign=1, eps=eps, method="grid")
        exact = make(x, N, isign=1, eps=0)
        return grid, exact

    def measure(typ, x, N, Q, eps, stages, direct_reps=None):
        M, P = x.shape[0], int(np.prod(N))
        A, E = operators(typ, x, N, eps)
        v = to_device(rng.standard_normal((Q, A.dim)).astype(np.float32))
        y = to_device(rng.standard_normal((Q, A.codim)).astype(np.float32))
        rec = dict(type=typ, D=len(N), N=list(N), M=M, Q=Q, pairs=M * P, eps=eps, w=A._w, nf=list(A._nf))
        rec.update(medians({"apply_ms": lambda: A.apply(v), "adjoint_ms": lambda: A.adjoint(y)}))
        d = medians({"direct_apply_ms": lambda: E.apply(v), "direct_adjoint_ms": lambda: E.adjoint(y)}, direct_reps)
        rec.update(d)
        ref = E.apply(v)
        rec["rel_diff"] = float((A.apply(v) - ref).norm() / ref.norm())
        if stages:
            *plan, corr = A._device_plan()
            nf, w, beta = A._nf, A._w, A._beta
            c = to_device(rng.standard_normal((Q, 2 * M)).astype(np.float32))
            u = to_device(rng.standard_normal((Q, 2 * P)).astype(np.float32))
            g = _dev.nufft_spread(nf, w, beta, plan, c)
            g2 = torch.empty_like(g)
            rec["stage_ms"] = medians({
                "spread": lambda: _dev.nufft_spread(nf, w, beta, plan, c, out=g),
                "interp": lambda: _dev.nufft_interp(nf, w, beta, plan, g),
                "fft": lambda: _dev.fft(g, nf, tuple(range(len(nf))), Q, True, out=g2),
                "deconv_extract": lambda: _dev.nufft_deconv(N, nf, 0, False, corr, g),
                "deconv_embed": lambda: _dev.nufft_deconv(N, nf, 0, True, corr, u, out=g),
            })
        return rec

    s = 4 if a.small else 1
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with pxrt.Precision(pxrt.Width.SINGLE):
        x16 = rng.uniform(-np.pi, np.pi, size=(65536 // s, 2)).astype(np.float32)
        x20 = rng.uniform(-np.pi, np.pi, size=((1 << 20) // (s * s), 2)).astype(np.float32)
        x20_3 = rng.uniform(-np.pi, np.pi, size=((1 << 20) // (s * s), 3)).astype(np.float32)
        work = [  # (name, type, points, N, Q, reps of the exact transform)
            ("type2_N256x256_M65536", 2, x16, (256 // s,) * 2, 1, None),
            ("type2_N256x256_M65536", 2, x16, (256 // s,) * 2, 8, None),
            ("type1_N64x64_M1048576", 1, x20, (64,) * 2, 1, None),
            ("type1_N64x64x64_M1048576", 1, x20_3, (64 // s,) * 3, 1, 1),
        ]
        for name, typ, x, N, Q, dreps in work:
            for eps in EPS:
                emit(dict(workload=name, small=bool(a.small), **measure(typ, x, N, Q, eps, True, dreps)))
        if not a.no_sweep:
            rows = []
            for D in (1, 2, 3):
                for lg in SWEEP_LOG2:
                    N, M = sweep_shape(D, lg - (4 if a.small else 0))
                    x = rng.uniform(-np.pi, np.pi, size=(M, D)).astype(np.float32)
                    for eps in SWEEP_EPS:
                        rec = measure(2, x, N, 1, eps, False, 1 if lg >= 28 else None)
                        rows.append(dict(sweep=True, log2_pairs=lg, **rec))
                        emit(rows[-1])
            emit(dict(crossover_pairs=crossover(rows), floor=1 << 20, small=bool(a.small)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
