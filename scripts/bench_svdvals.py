#!/usr/bin/env python
"""
Measurements behind LinOp.svdvals(k, which), written to profiles/svdvals_bench.txt:

  gs   one two-pass Gram-Schmidt step on the same V, w: the fused kernels (pxa_krylov_dots, pxa_krylov_update x 2)
       against the composed chain (pxa_dense_matmat x 4, pxa_axpby x 2, pxa_row_reduce), fp32 and fp64,
       n = 2^20 and 2^22, j = 8, 20, 41.  Device events around `--reps` back-to-back steps, median of `--rounds`
       rounds, the two variants alternating; the fused step's basis traffic (2 j n elements) over its time.
  k1   svdvals(k=1, solver="lanczos") against the power iteration of the default path on the benchmark's 2048^2
       Gaussian blur and on a dense 8192 x 4096 matrix (fp32): Gram applications and wall time until the value agrees
       with a float64 Lanczos reference to 1e-5 relative, and the value each path returns.
  k6   svdvals(k=6, "LM") wall time on the same two operators.

    python scripts/bench_svdvals.py [--part gs,k1,k6] [--out profiles/svdvals_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.math._lanczos as lz  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device  # noqa: E402


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per step


def part_gs(log, reps, rounds):
    log("# gs: one two-pass Gram-Schmidt step, ms (median of %d rounds of %d steps; min .. max)" % (rounds, reps))
    log("# dtype        n   j   fused_ms [min..max]   composed_ms [min..max]   composed/fused   fused GB/s of 2jn")
    for tdt in (torch.float32, torch.float64):
        es = torch.empty((), dtype=tdt).element_size()
        for n in (2**20, 2**22):
            for j in (8, 20, 41):
                g = torch.Generator(device="cuda").manual_seed(j + n % 1000)
                V = torch.randn((j, n), dtype=tdt, device="cuda", generator=g) / np.sqrt(n)
                w = torch.randn((n,), dtype=tdt, device="cuda", generator=g)
                work = _dev.krylov_workspace(j, n, w)
                c1 = torch.zeros(j, dtype=torch.float64, device="cuda")
                c2, nr = torch.zeros_like(c1), torch.zeros(1, dtype=torch.float64, device="cuda")
                w1, w2 = torch.empty_like(w), torch.empty_like(w)

                def fused():
                    _dev.krylov_dots(V, j, w, c1, work)
                    _dev.krylov_update(V, j, w, c1, w1, work, c_next=c2)
                    _dev.krylov_update(V, j, w1, c2, w2, work, nrm2_out=nr)

                def composed():
                    x = w
                    for _ in range(2):
                        ct = _dev.dense_matmat(V, x.reshape(1, -1), 0)
                        x = _dev.axpby(1.0, x, -1.0, _dev.dense_matmat(V, ct, 1).reshape(-1))
                    _dev.row_reduce(_dev.RED_SUMSQ, x.reshape(1, -1), out=nr)
                    return x

                fused()
                xc = composed()
                torch.cuda.synchronize()
                d = float((w2.double() - xc.double()).norm() / xc.double().norm())
                for fn in (fused, composed):
                    _timed(fn, 3)
                tf, tc = [], []
                for _ in range(rounds):
                    tf.append(_timed(fused, reps))
                    tc.append(_timed(composed, reps))
                mf, mc = statistics.median(tf), statistics.median(tc)
                log(f"{str(tdt)[6:]:8s} {n:8d} {j:3d}   {mf:8.4f} [{min(tf):.4f}..{max(tf):.4f}]   {mc:8.4f} [{min(tc):.4f}..{max(tc):.4f}]"
                    f"   {mc / mf:6.3f}   {2 * j * n * es / (mf * 1e-3) / 1e9:8.1f}   (rel diff of results {d:.2e})")
                del V, w, w1, w2, xc


def _operators():
    sh = (2048, 2048)
    yield "blur2048", lambda: pxo.Gaussian(arg_shape=sh, sigma=2.0, truncate=3.0)
    rng = np.random.default_rng(0)
    A = rng.standard_normal((8192, 4096))
    yield "dense8192x4096", lambda: pxa.LinOp.from_array(A.astype(pxrt.getPrecision().value))


MAXITER = 300  # restart cycles a timed call may take (clustered spectra converge slowly; the cap is reported)


def _wall(fn):
    """(result, seconds) of fn(); a RuntimeError (the cycle cap) is returned in place of the result."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        out = fn()
    except RuntimeError as e:
        out = e
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _vals(v):
    return f"NOT CONVERGED ({v})" if isinstance(v, Exception) else np.array2string(np.asarray(v, dtype=np.float64), precision=9)


def _power_trace(op, truth, rel, n_iter):
    """The default path's power iteration (LinOp._power_lipschitz, same start vector and arithmetic), followed step by
    step: Gram applications and seconds until |L - truth| <= rel truth, and until its own tol = 1e-6 stops it."""
    dt = pxrt.getPrecision().value
    x = np.random.default_rng(0).standard_normal(op.dim).astype(dt)
    x = to_device(x / np.linalg.norm(x))
    L_prev, hit, stop = 0.0, None, None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pxrt.EnforcePrecision(False):
        for it in range(1, n_iter + 1):
            y = op.adjoint(op.apply(x))
            nrm = float(_dev.row_reduce(_dev.RED_SUMSQ, y.reshape(1, -1)).cpu()[0]) ** 0.5
            L = nrm**0.5
            x = _dev.div(y, nrm)
            now = time.perf_counter() - t0
            if hit is None and abs(L - truth) <= rel * truth:
                hit = (it, now, L)
            if stop is None and abs(L - L_prev) <= 1e-6 * L:
                stop = (it, now, L)
            if hit and stop:
                break
            L_prev = L
    return hit, stop, (it, time.perf_counter() - t0, L)


def part_k1(log, n_iter):
    log("# k1: largest singular value, fp32; truth = svdvals(k=1, solver='lanczos', tol=1e-9) in float64")
    for name, make in _operators():
        with pxrt.Precision(pxrt.Width.DOUBLE):
            st = {}
            v, _ = _wall(lambda: make().svdvals(k=1, solver="lanczos", tol=1e-9, maxiter=4 * MAXITER, _stats=st))
        if isinstance(v, Exception):
            log(f"{name}: no float64 reference ({v}); skipped")
            continue
        truth = float(v[0])
        log(f"{name}: truth {truth:.12g}  (float64 Lanczos: {st})")
        with pxrt.Precision(pxrt.Width.SINGLE):
            op = make()
            op.svdvals(k=1, solver="lanczos", tol=1e-2)  # warm-up: code objects, allocator
            op.svdvals(n_iter=3)
            for tol in (1e-5, 0.0):
                st = {}
                v, t = _wall(lambda: op.svdvals(k=1, solver="lanczos", tol=tol, maxiter=MAXITER, _stats=st))
                rd = "n/a" if isinstance(v, Exception) else f"{abs(float(v[0]) - truth) / truth:.2e}"
                log(f"  lanczos tol={tol:g}: value {_vals(v)}  rel diff to truth {rd}"
                    f"  Gram applications {st['applications']}  cycles {st['cycles']}  wall {t * 1e3:.1f} ms")
            v, t = _wall(lambda: op.svdvals())
            log(f"  default path svdvals(): value {float(v[0]):.9g}  rel diff to truth {abs(float(v[0]) - truth) / truth:.2e}"
                f"  wall {t * 1e3:.1f} ms")
            hit, stop, last = _power_trace(op, truth, 1e-5, n_iter)
            fmt = lambda r: "not reached" if r is None else f"{r[0]} Gram applications, {r[1] * 1e3:.1f} ms, value {r[2]:.9g}"
            log(f"  power iteration to 1e-5 of truth: {fmt(hit)}")
            log(f"  power iteration to its own stop (tol 1e-6): {fmt(stop)}")
            log(f"  power iteration, last step followed: {fmt(last)}  rel diff to truth {abs(last[2] - truth) / truth:.2e}")
        del op


def part_k6(log):
    log("# k6: svdvals(k=6, 'LM'), fp32, wall time of the second call")
    for name, make in _operators():
        with pxrt.Precision(pxrt.Width.SINGLE):
            op = make()
            op.svdvals(k=6, tol=1e-2)
            st = {}
            v, t = _wall(lambda: op.svdvals(k=6, maxiter=MAXITER, _stats=st))
            log(f"{name}: {_vals(v)}  {st}  wall {t * 1e3:.1f} ms")
            for fused in (False,):
                lz._FUSED = fused
                try:
                    op.svdvals(k=6, tol=1e-2)
                    st = {}
                    v, t = _wall(lambda: op.svdvals(k=6, maxiter=MAXITER, _stats=st))
                finally:
                    lz._FUSED = True
                log(f"{name} (_FUSED = False): {_vals(v)}  {st}  wall {t * 1e3:.1f} ms")
        del op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="gs,k1,k6")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svdvals_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--power-iters", type=int, default=3000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_svdvals.py needs an MI355X")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:

        def log(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()

        log(f"# scripts/bench_svdvals.py --part {args.part}  ({torch.cuda.get_device_name(0)})")
        for part in args.part.split(","):
            if part == "gs":
                part_gs(log, args.reps, args.rounds)
            elif part == "k1":
                part_k1(log, args.power_iters)
            elif part == "k6":
                part_k6(log)
            else:
                raise SystemExit(f"unknown part {part!r}")


if __name__ == "__main__":
    main()
