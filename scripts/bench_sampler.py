#!/usr/bin/env python
"""
Interleaved A/B of the Langevin sampler hot path (pyxu_amd/experimental/sampler, csrc/sampler.hip), in fp32.

    python scripts/bench_sampler.py [--rounds 5] [--reps 20] [--small] [--out FILE]

Per size (one row of 2^20 and of 2^24 elements) one JSON line each for

  step      one MYULA step for f = 1/2 ||x - y||^2, g = 0.1 L1Norm.  `fused`: grad f plus pxa_langevin_step with the
            Moreau-Yosida term and the Philox noise made inside the launch.  `chain`: the `_FUSED = False` form,
            (f + g.moreau_envelope(lamb)).grad through the generic operators, noise from torch.randn, and the step
            kernel without a g reading that noise.  `kernel`: the fused launch alone (3 array streams), `kernel_noise`:
            the same launch reading supplied noise (4 streams), `normal`: pxa_philox_normal alone (1 stream)
  moments   pxa_online_moments at order 4 (x in, mean and three double planes in and out: 60 B per element) against the
            chain of element-wise launches OnlineCenteredMoment runs above order 4

HIP events around `reps` back-to-back calls after a warm-up, the sides alternating within a round; `ms` is the median
over the rounds, `round_ms` every round.  `bytes` is what a side must move, from the shapes; `tbps` from it, `frac`
against the 8 TB/s HBM figure of DESIGN.md section 4.  Nothing is timed without an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0
SIZES = [2**20, 2**24]
SMALL = [2**12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tiny size (a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.txt"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_sampler.py needs an MI355X: no timing is taken without one")
    import pyxu_amd.experimental.sampler as pxes
    import pyxu_amd.operator as pxo
    import pyxu_amd.runtime as pxrt
    from pyxu_amd import _dev
    from pyxu_amd.util import to_device

    rng = np.random.default_rng(0)
    dt = np.float32

    def dev(n):
        return to_device(rng.standard_normal(n).astype(dt))

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def rounds(fns):
        for fn in fns.values():  # warm-up: every shape and kernel of the timed window
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                res[k].append(round(events(fn), 5))
        return res

    def emit(out, what, n, res, nbytes, **extra):
        ms = {k: statistics.median(r) for k, r in res.items()}
        tbps = {k: round(nbytes[k] / ms[k] * 1e-9, 3) for k in nbytes}
        rec = dict(what=what, n=n, ms=ms, round_ms=res, bytes=nbytes, tbps=tbps,
                   frac={k: round(v / HBM_TBPS, 3) for k, v in tbps.items()}, **extra)
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def step(out, n):
        lamb, pw, gamma = 0.5, 0.1, 0.3
        f = 0.5 * pxo.SquaredL2Norm(dim=n).asloss(dev(n))
        s = pxes.MYULA(f, pw * pxo.L1Norm(dim=n), gamma=gamma, lamb=lamb)
        x, g0, z0, o = dev(n), dev(n), dev(n), dev(n)
        state = dict(k=0)

        def fused():
            state["k"] += 1
            _dev.langevin_step(_dev.PROX_L1, gamma, lamb, pw, x, s._f_diff.grad(x), o, seed=1, step=state["k"])

        def chain():
            _dev.langevin_step(0, gamma, 1.0, 0.0, x, s._f.grad(x), o, noise=torch.randn(n, dtype=x.dtype, device=x.device))

        fns = {
            "fused": fused,
            "chain": chain,
            "kernel": lambda: _dev.langevin_step(_dev.PROX_L1, gamma, lamb, pw, x, g0, o, seed=1, step=3),
            "kernel_noise": lambda: _dev.langevin_step(_dev.PROX_L1, gamma, lamb, pw, x, g0, o, noise=z0),
            "normal": lambda: _dev.philox_normal(o, 1, 3),
        }
        res = rounds(fns)
        nbytes = {"kernel": 3 * n * 4, "kernel_noise": 4 * n * 4, "normal": n * 4}
        ms = {k: statistics.median(r) for k, r in res.items()}
        emit(out, "step", n, res, nbytes, speedup=round(ms["chain"] / ms["fused"], 2))

    def moments(out, n):
        x = dev(n)
        mean, sums = dev(n), to_device(rng.standard_normal((3, n)))
        st = pxes.OnlineCenteredMoment(4)
        st._mean, st._corrected_sums = dev(n), to_device(rng.standard_normal((3, n)))
        fns = {"fused": lambda: _dev.online_moments(4, 5, x, mean, sums), "chain": lambda: st._chain(5, x)}
        res = rounds(fns)
        ms = {k: statistics.median(r) for k, r in res.items()}
        emit(out, "moments", n, res, {"fused": n * (4 + 8 + 3 * 16)}, speedup=round(ms["chain"] / ms["fused"], 2))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out, pxrt.Precision(pxrt.Width.SINGLE):
        for n in (SMALL if a.small else SIZES):
            step(out, n)
        for n in (SMALL if a.small else SIZES):
            moments(out, n)


if __name__ == "__main__":
    main()
