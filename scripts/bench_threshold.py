"""
Timings of the row threshold search (csrc/threshold.hip), HIP events, 50 launches after warm-up:

* streaming path at 1 x 2048^2 float32: one count pass (partial + update launch) against the yardstick
  pxa_row_reduce(ABS) over the same bytes; the S pass; a pass over a row already marked done; the shrink; the whole
  prox (search batches, the state read, the shrink) and its pass count;
* resident path at 4096 x 4096 float32 against pxa_prox_l1 at the same shape (both move 8 B per element).

    python scripts/bench_threshold.py [--out FILE]

Prints one JSON object per measurement (and appends them to FILE).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import check, lib  # noqa: E402

REPS, WARM = 50, 5


def timed(fn, reps=REPS, warm=WARM):
    """Median / min milliseconds of fn() over `reps` event-timed launches."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def values(shape, seed):
    r = np.random.default_rng(seed)
    x = 10.0 ** r.uniform(-2.0, 2.0, shape) * r.choice([-1.0, 1.0], shape)
    return torch.from_numpy(x.astype(np.float32)).cuda()


class Stream:
    """The streaming entry point with its buffers, one pass at a time."""

    def __init__(self, x, a, b, c):
        self.x, self.abc = x, (a, b, c)
        rows, n = x.shape
        self.mu = torch.zeros(rows, dtype=torch.float64, device="cuda")
        self.state = torch.zeros(rows, dtype=torch.int32, device="cuda")
        self.passes = torch.zeros(rows, dtype=torch.int32, device="cuda")
        self.work = torch.empty(int(lib.pxa_row_threshold_workspace_bytes(rows, n)) // 8 + 1, dtype=torch.float64, device="cuda")

    def run(self, first, npasses):
        x = self.x
        a, b, c = self.abc
        check(lib.pxa_row_threshold_stream(_dev.dtcode(x), x.shape[0], x.shape[1], x.data_ptr(), a, b, c, first, npasses,
                                           self.mu.data_ptr(), self.state.data_ptr(), self.passes.data_ptr(),
                                           self.work.data_ptr(), _dev.stream()), "pxa_row_threshold_stream")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        res.append(kw)

    # ---------------------------------------------------------------- streaming, 1 x 2048^2 float32
    n = 2048 * 2048
    x = values((1, n), 0)
    S = float(x.double().abs().sum())
    a, b, c = 1.0, 0.0, 0.3 * S
    gb = n * 4 / 1e9
    med, mn = timed(lambda: _dev.row_reduce(_dev.RED_ABS, x))
    emit(what="yardstick row_reduce(ABS) 1x2048^2 f32", ms_median=med, ms_min=mn, GBps=gb / (mn * 1e-3))
    yard = mn
    st = Stream(x, a, b, c)
    med, mn = timed(lambda: st.run(1, 0))
    emit(what="S pass (partial + update)", ms_median=med, ms_min=mn, vs_yardstick=mn / yard)
    # active count passes: restart the search before each timed pass so that the row is not done
    ms = []
    for _ in range(WARM + REPS):
        st.run(1, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.run(0, 1)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[WARM:]
    emit(what="count pass (partial + update), row active", ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
         GBps=gb / (np.min(ms) * 1e-3), vs_yardstick=float(np.min(ms)) / yard)
    st.run(1, 64)
    torch.cuda.synchronize()
    assert int(st.state[0]) == 1
    emit(what="search", passes=int(st.passes[0]), mu=float(st.mu[0]))
    med, mn = timed(lambda: st.run(0, 1))
    emit(what="pass over a row already done (2 launches)", ms_median=med, ms_min=mn)
    med16, mn16 = timed(lambda: st.run(0, 16))
    emit(what="16 passes over a row already done", ms_median=med16, ms_min=mn16, per_pass_ms=mn16 / 16)
    out = torch.empty_like(x)
    med, mn = timed(lambda: _dev.row_shrink(x, st.mu, _dev.SHRINK_SOFT, out=out))
    emit(what="row_shrink SOFT", ms_median=med, ms_min=mn, GBps=2 * gb / (mn * 1e-3))
    t0 = time.perf_counter()
    state_read = [st.state.cpu() for _ in range(REPS)]
    emit(what="state read (device-to-host copy of the state words), wall", ms=(time.perf_counter() - t0) * 1e3 / len(state_read))
    for batch in (4, 8, 16, 32):
        wall = []
        for _ in range(WARM + 20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _dev.row_threshold_prox(x, a, b, c, _dev.SHRINK_SOFT, out=out, batch=batch)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        emit(what="whole prox (L1Ball, c = 0.3 S), wall", first_batch=batch, ms_median=float(np.median(wall[WARM:])),
             ms_min=float(np.min(wall[WARM:])))
    for name, (a2, b2, c2) in {"SquaredL1 tau=5": (10.0, 1.0, 0.0), "LInf c=0.9S": (1.0, 0.0, 0.9 * S)}.items():
        _, mu2, p2 = _dev.row_threshold_prox(x, a2, b2, c2, _dev.SHRINK_SOFT, out=out, info=True)
        emit(what=f"search {name}", passes=int(p2[0]))

    # ---------------------------------------------------------------- resident, 4096 x 4096 float32
    rows = n2 = 4096
    x = values((rows, n2), 1)
    out = torch.empty_like(x)
    gb = rows * n2 * 4 / 1e9
    med, mn = timed(lambda: _dev.prox_l1(x, 0.5, out=out))
    emit(what="pxa_prox_l1 4096x4096 f32", ms_median=med, ms_min=mn, GBps=2 * gb / (mn * 1e-3))
    base = mn
    S = float(x[0].double().abs().sum())
    for name, (a2, b2, c2, mode) in {"L1Ball c=0.3S": (1.0, 0.0, 0.3 * S, _dev.SHRINK_SOFT),
                                     "LInf c=0.3S": (1.0, 0.0, 0.3 * S, _dev.SHRINK_CLAMP),
                                     "SquaredL1 tau=5": (10.0, 1.0, 0.0, _dev.SHRINK_SOFT)}.items():
        med, mn = timed(lambda: _dev.row_threshold_prox(x, a2, b2, c2, mode, out=out))
        _, _, p = _dev.row_threshold_prox(x, a2, b2, c2, mode, out=out, info=True)
        emit(what=f"resident prox {name} 4096x4096 f32", ms_median=med, ms_min=mn, GBps=2 * gb / (mn * 1e-3),
             vs_prox_l1=mn / base, passes_max=int(p.max()), passes_mean=float(p.double().mean()))
    med, mn = timed(lambda: _dev.row_threshold_prox(x, 1.0, 0.0, 1e9, _dev.SHRINK_SOFT, out=out))
    emit(what="resident prox inside the ball (S pass only) 4096x4096 f32", ms_median=med, ms_min=mn, vs_prox_l1=mn / base)
    for rows, n2 in ((65535, 256), (16384, 1024), (1024, 16384), (512, 32768)):
        x = values((rows, n2), 2)
        out = torch.empty_like(x)
        S = float(x[0].double().abs().sum())
        med, mn = timed(lambda: _dev.row_threshold_prox(x, 1.0, 0.0, 0.3 * S, _dev.SHRINK_SOFT, out=out), reps=20)
        med1, mn1 = timed(lambda: _dev.prox_l1(x, 0.5, out=out), reps=20)
        emit(what=f"resident prox L1Ball {rows}x{n2} f32", ms_min=mn, GBps=2 * rows * n2 * 4 / 1e9 / (mn * 1e-3),
             vs_prox_l1=mn / mn1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
