#!/usr/bin/env python
"""
Measure the gridded type-3 NUFFT (NUFFT.type3 with method="grid3": pxa_nufft_spread_fac, pxa_nufft_deconv, pxa_fft_ex,
pxa_nufft_interp_fac) against the exact transform on the same inputs (pxa_nudft), in fp32.

    python scripts/bench_nufft_type3.py [--rounds 5] [--reps 3] [--small] [--parts abcd] [--out FILE]

(a) Sweep: D = 1, 2, 3 at eps = 1e-4 and 1e-6, M = N, M N = 2^20 .. 2^32 in factors of 4, sources in [-pi, pi]^D and
    targets in [-S, S]^D with S chosen so that the outer grid has about M cells (prod nf1 ~ M).  Gridded apply and
    adjoint against the exact ones.  crossover_pairs: the smallest tested M N from which, for every D and eps, both
    gridded directions are faster at that size and every larger tested one (never below 2^20).
(b) At M N = 2^30 (M = N = 32768) and eps = 1e-6, the space-bandwidth product grows (prod nf1 = 2^12 .. in factors
    of 4, up to the largest FFT sizes the suite tests: 131072 cells in one dimension, 2048^2, 128^3) until the
    gridded chain loses.  pairs_per_cell: the smallest tested M N / prod(nf2) over (a) at or above the crossover and
    (b) from which both directions win there and at every larger tested ratio.
(c) A/B of the fused factors against the same chain with pxa_complex_mul before the plain spreading kernel and after
    the plain interpolation kernel, at a launch-bound size (M = N = 1024, D = 2) and a large one (M = N = 2^20,
    D = 2), both directions, alternating within a round; median, minimum and maximum over the rounds.
(d) Host plan-build time at N = 2^20 targets (and as many sources), D = 3: the rescaling, the two sorts
    (`_grid_plan`), and the factors (the phase and the correction quadrature at the targets).

All device times are HIP-event times of `reps` back-to-back calls after a warm-up call; the sides alternate within a
round and the median over the rounds is reported.  One JSON line per measurement.
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

SWEEP_EPS = (1e-4, 1e-6)
SWEEP_LOG2 = (20, 22, 24, 26, 28, 30, 32)
SBP_LOG2 = {1: (12, 14, 16), 2: (12, 14, 16, 18, 20), 3: (12, 15, 18)}  # log2 prod(nf1) of part (b)
FLOOR = 1 << 20


def points(rng, M, N, D, cells, sigma=2.0):
    """Sources in [-pi, pi]^D and targets in [-S, S]^D with 2 sigma pi S / pi = cells^(1/D) cells per axis."""
    S = max(cells ** (1.0 / D) / (2 * sigma), 1.0)
    x = rng.uniform(-np.pi, np.pi, size=(M, D)).astype(np.float32)
    z = rng.uniform(-S, S, size=(N, D)).astype(np.float32)
    return x, z


def crossover(rows):
    """Smallest tested pair count from which every (D, eps) has both gridded directions faster, there and above."""
    good = None
    for s in sorted({r["log2_pairs"] for r in rows}, reverse=True):
        here = [r for r in rows if r["log2_pairs"] == s]
        if all(r["apply_ms"] < r["direct_apply_ms"] and r["adjoint_ms"] < r["direct_adjoint_ms"] for r in here):
            good = 1 << s
        else:
            break
    return None if good is None else max(good, FLOOR)


def pairs_per_cell(rows):
    """Smallest tested M N / prod(nf2) from which both gridded directions win, there and at every larger ratio."""
    good = None
    for r in sorted(rows, key=lambda r: -r["pairs_per_cell"]):
        if r["apply_ms"] < r["direct_apply_ms"] and r["adjoint_ms"] < r["direct_adjoint_ms"]:
            good = r["pairs_per_cell"]
        else:
            break
    return good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="1/256 of the pairs (a rehearsal, not a measurement)")
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nufft_type3_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_nufft_type3.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.operator as pxo
    import pyxu_amd.runtime as pxrt
    from pyxu_amd import _dev
    from pyxu_amd.operator.linop import nufft as nufft_mod
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)
    shrink = 8 if a.small else 0  # log2

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def rounds(fns, reps=None):
        """ms per round of each callable: a warm-up call each, then `rounds` rounds in which they alternate."""
        reps = a.reps if reps is None else reps
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, reps))
        return t

    def medians(fns, reps=None):
        return {k: round(statistics.median(v), 4) for k, v in rounds(fns, reps).items()}

    def measure(x, z, eps, direct_reps=None):
        A = pxo.NUFFT.type3(x, z, isign=1, eps=eps, method="grid3")
        E = pxo.NUFFT.type3(x, z, isign=1, eps=0)
        v = to_device(rng.standard_normal((1, A.dim)).astype(np.float32))
        y = to_device(rng.standard_normal((1, A.codim)).astype(np.float32))
        cells = int(np.prod(A._nf2))
        rec = dict(D=x.shape[1], M=x.shape[0], N=z.shape[0], pairs=x.shape[0] * z.shape[0], eps=eps, w=A._w,
                   nf1=list(A._nf1), nf2=list(A._nf2), pairs_per_cell=round(x.shape[0] * z.shape[0] / cells, 2))
        rec.update(medians({"apply_ms": lambda: A.apply(v), "adjoint_ms": lambda: A.adjoint(y)}))
        rec.update(medians({"direct_apply_ms": lambda: E.apply(v), "direct_adjoint_ms": lambda: E.adjoint(y)},
                           direct_reps))
        ref = E.apply(v)
        rec["rel_diff"] = float((A.apply(v) - ref).norm() / ref.norm())
        return rec

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with pxrt.Precision(pxrt.Width.SINGLE):
        sweep, cross = [], None
        if "a" in a.parts:
            for D in (1, 2, 3):
                for lg in SWEEP_LOG2:
                    M = 1 << ((lg - shrink) // 2)
                    x, z = points(rng, M, M, D, M)
                    for eps in SWEEP_EPS:
                        sweep.append(dict(part="a", log2_pairs=lg, **measure(x, z, eps, 1 if lg >= 28 else None)))
                        emit(sweep[-1])
            cross = crossover(sweep)
            emit(dict(part="a", crossover_pairs=cross, floor=FLOOR, small=bool(a.small)))
        if "b" in a.parts:
            M = 1 << ((30 - shrink) // 2)
            grown = []
            for D, logs in SBP_LOG2.items():
                for lg in logs:
                    x, z = points(rng, M, M, D, 1 << lg)
                    grown.append(dict(part="b", log2_cells_nf1=lg, **measure(x, z, 1e-6, 1)))
                    emit(grown[-1])
            rows = grown + [r for r in sweep if cross is not None and r["pairs"] >= cross]
            emit(dict(part="b", pairs_per_cell=pairs_per_cell(rows), smallest_tested=min(r["pairs_per_cell"] for r in rows),
                      small=bool(a.small)))
        if "c" in a.parts:
            for M in (1024, (1 << 20) >> (shrink // 2)):
                x, z = points(rng, M, M, 2, M)
                A = pxo.NUFFT.type3(x, z, isign=1, eps=1e-6, method="grid3")
                (*px, fx), (*pz, fz), corr = A._device_plan()
                nf1, nf2, w, beta, axes = A._nf1, A._nf2, A._w, A._beta, (0, 1)

                def by_point(plan):  # the factors in the points' own order, for pxa_complex_mul
                    out = np.empty_like(plan["fac"])
                    out[plan["perm"]] = plan["fac"]
                    return to_device(out)

                ux, uz = by_point(A._plan_x), by_point(A._plan_z)
                v = to_device(rng.standard_normal((1, 2 * M)).astype(np.float32))
                y = to_device(rng.standard_normal((1, 2 * M)).astype(np.float32))

                def fused_apply():
                    g = _dev.nufft_spread(nf1, w, beta, px, v, fac=fx, conj=False)
                    g = _dev.nufft_deconv(nf1, nf2, 1, True, corr, g)
                    _dev.fft(g, nf2, axes, 1, True, out=g)
                    return _dev.nufft_interp(nf2, w, beta, pz, g, fac=fz, conj=False)

                def plain_apply():
                    g = _dev.nufft_spread(nf1, w, beta, px, _dev.complex_mul(v, ux))
                    g = _dev.nufft_deconv(nf1, nf2, 1, True, corr, g)
                    _dev.fft(g, nf2, axes, 1, True, out=g)
                    o = _dev.nufft_interp(nf2, w, beta, pz, g)
                    return _dev.complex_mul(o, uz, out=o)

                def fused_adjoint():
                    g = _dev.nufft_spread(nf2, w, beta, pz, y, fac=fz, conj=True)
                    _dev.fft(g, nf2, axes, 1, False, out=g)
                    g = _dev.nufft_deconv(nf1, nf2, 1, False, corr, g)
                    return _dev.nufft_interp(nf1, w, beta, px, g, fac=fx, conj=True)

                def plain_adjoint():
                    g = _dev.nufft_spread(nf2, w, beta, pz, _dev.complex_mul(y, uz, conj_b=True))
                    _dev.fft(g, nf2, axes, 1, False, out=g)
                    g = _dev.nufft_deconv(nf1, nf2, 1, False, corr, g)
                    o = _dev.nufft_interp(nf1, w, beta, px, g)
                    return _dev.complex_mul(o, ux, conj_b=True, out=o)

                same = [float((f() - p()).norm() / p().norm()) for f, p in ((fused_apply, plain_apply),
                                                                            (fused_adjoint, plain_adjoint))]
                t = rounds({"fused_apply": fused_apply, "plain_apply": plain_apply, "fused_adjoint": fused_adjoint,
                            "plain_adjoint": plain_adjoint})
                emit(dict(part="c", D=2, M=M, N=M, eps=1e-6, w=w, nf1=list(nf1), nf2=list(nf2), fused_vs_plain_rel=same,
                          ms={k: dict(median=round(statistics.median(u), 4), min=round(min(u), 4), max=round(max(u), 4))
                              for k, u in t.items()}))
        if "d" in a.parts:
            N = (1 << 20) >> shrink
            x, z = points(rng, N, N, 3, 1 << 18)
            t0 = time.perf_counter()
            prm = nufft_mod._t3_params(x, z, 1e-6, 2.0)
            xp, zp = nufft_mod._t3_rescale(x, z, prm)
            t1 = time.perf_counter()
            bins = _dev.nufft_grid_tiles(0, 3)[0]
            nufft_mod._grid_plan(xp, prm["nf1"], prm["w"], bins, np.float32)
            t2 = time.perf_counter()
            nufft_mod._grid_plan(zp, prm["nf2"], prm["w"], bins, np.float32)
            t3 = time.perf_counter()
            nufft_mod._t3_factors(x, z, zp, prm)
            t4 = time.perf_counter()
            emit(dict(part="d", D=3, M=N, N=N, nf1=list(prm["nf1"]), nf2=list(prm["nf2"]), w=prm["w"],
                      host_s=dict(params_and_rescale=round(t1 - t0, 3), sort_sources=round(t2 - t1, 3),
                                  sort_targets=round(t3 - t2, 3), factors=round(t4 - t3, 3))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
