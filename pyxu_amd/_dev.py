"""
Device-array kernels: thin Python entry points over the C-ABI (``include/pyxu_amd.h``).

Every function takes/returns torch-ROCm tensors resident on the current device, launches on
``torch.cuda.current_stream()`` and raises on any non-zero status.  Host arrays are rejected with
a TypeError: this package has no CPU compute path.
"""
import ctypes as ct
import os

import numpy as np

from pyxu_amd._lib import check, f64_array, i32_array, i64_array, int_array, lib

__all__ = []  # internal module

RED_SUMSQ, RED_DIFFSQ, RED_DOT, RED_ABS, RED_MAXABS, RED_SUM, RED_NEGCNT, RED_MIN, RED_MAX = range(9)
MODES = {"constant": 0, "wrap": 1, "reflect": 2, "symmetric": 3, "edge": 4}


def _torch():
    import torch

    return torch


def wait_event(ev, spin_s=1e-3):
    """Wait for a recorded HIP event: poll it for up to `spin_s` seconds, then yield between polls so that a
    long wait does not starve other threads.  A stop check waits for the device queue the host has run ahead
    by (stop_rate x the step time at most: ~0.25 ms at 20 PGD steps of 2048^2), and the step enqueued
    behind the check covers only one step time after the event: a blocking hipEventSynchronize, or a
    sleep(0) between polls, wakes the host up tens of microseconds late and leaves the device idle."""
    import time

    if ev.query():
        return
    t_end = time.perf_counter() + spin_s
    while not ev.query():
        if time.perf_counter() > t_end:
            time.sleep(0)


def dtcode(t) -> int:
    torch = _torch()
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.float64:
        return 1
    raise TypeError(f"pyxu_amd: unsupported dtype {t.dtype} (float32/float64 only).")


class _DtypeMismatch(TypeError, ValueError):
    """An operand whose dtype differs from that of the call's other operands.  A TypeError like every dtype error of
    this module; also a ValueError, which the NUFFT, ProxAdam and sampler entries have always raised for it."""


_FLOATS = ()  # (torch.float32, torch.float64) once torch is in


def _floats():
    global _FLOATS
    _FLOATS = (_torch().float32, _torch().float64)
    return _FLOATS


def _operand(t, name, dtype, like, numel, shape, ctx, pinned=False):
    """The checks `require` (inputs) and `written` (outputs) share: a device tensor (with `pinned`, pinned host
    memory too) of float32 / float64 or of the torch dtype named `dtype`, optionally of like's dtype, of `numel`
    elements, of `shape`.  TypeError for kind, device and dtype, ValueError for size."""
    if not (type(t).__module__.startswith("torch") and hasattr(t, "is_cuda")):
        raise TypeError(
            f"pyxu_amd: `{name}` must be an MI355X device tensor (got {type(t).__name__}); "
            "move host data with pyxu_amd.util.to_device()."
        )
    if not (t.is_cuda or (pinned and t.is_pinned())):
        raise TypeError(f"pyxu_amd: `{name}` lives on {t.device}; pyxu_amd computes on the MI355X only.")
    if dtype is None:
        dtcode(t)
    elif t.dtype != getattr(_torch(), dtype):
        raise TypeError(f"pyxu_amd: `{name}` has dtype {t.dtype}, {ctx} needs {dtype}.")
    if like is not None and t.dtype != like.dtype:
        raise _DtypeMismatch(f"pyxu_amd: `{name}` has dtype {t.dtype}, {ctx} has {like.dtype}.")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"pyxu_amd: `{name}` holds {t.numel()} elements, {ctx} needs {numel}.")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"pyxu_amd: `{name}` has shape {tuple(t.shape)}, {ctx} needs {tuple(shape)}.")


def require(t, name="arr", dtype=None, like=None, numel=None, shape=None, ctx="the call"):
    """An input operand: a device tensor, float32 / float64 or the torch dtype named `dtype` ("float64", "int32",
    "int64", "bool"), optionally of like's dtype, `numel` elements, `shape`.  A non-contiguous input is copied."""
    if _TIMER is not None:  # other device work is about to be enqueued: close the timing window
        _TIMER.interrupt()
    # (a call that passes skips the nested call: host cost per call in profiles/dev_binding_host_ab.txt)
    if not (dtype is None and shape is None and getattr(t, "is_cuda", False)
            and (t.dtype in (_FLOATS or _floats()) if like is None else t.dtype == like.dtype)
            and (numel is None or t.numel() == numel)):
        _operand(t, name, dtype, like, numel, shape, ctx)
    return t if t.is_contiguous() else t.contiguous()


def require_bool(c):
    return require(c, "condition", dtype="bool")


def written(t, name="out", dtype=None, like=None, numel=None, at_least=None, apart=(), ctx="the call", pinned=False):
    """An operand a kernel writes (`out=`, an in-place operand, a workspace): as `require`, but taken as it is, so a
    non-contiguous one is a ValueError, never a copy.  Sizes go by `numel` (callers pass flat and shaped views of one
    buffer) or `at_least` elements; a contiguous view may start off a 16-byte boundary (the kernels then take their
    scalar path).  It must not start where any tensor of `apart` starts (None entries are skipped)."""
    if (dtype is None and at_least is None and not apart and getattr(t, "is_cuda", False) and t.is_contiguous()
            and (t.dtype in (_FLOATS or _floats()) if like is None else t.dtype == like.dtype)
            and (numel is None or t.numel() == numel)):
        return t  # (the common `out=` that passes, in one expression; everything else is named below)
    _operand(t, name, dtype, like, numel, None, ctx, pinned)
    if not t.is_contiguous():
        raise ValueError(f"pyxu_amd: `{name}` is written in place and must be contiguous.")
    if at_least is not None and t.numel() < at_least:
        raise ValueError(f"pyxu_amd: `{name}` holds {t.numel()} elements, {ctx} needs at least {at_least}.")
    for o in apart:
        if o is not None and o.data_ptr() == t.data_ptr():
            raise ValueError(f"pyxu_amd: `{name}` aliases another operand of {ctx}.")
    return t


def _out(out, like, shape=None, apart=()):
    """The result of a wrapper: a fresh contiguous tensor of `shape` (like's own when None) in like's dtype, or the
    caller's `out`, checked as `written` with that many elements."""
    if out is None:
        return empty_like(like) if shape is None else empty(shape, like)
    numel = like.numel() if shape is None else int(np.prod(shape))
    return written(out, "out", like=like, numel=numel, apart=apart)


def flag_buffer(fb, name, values, flags):
    """A HostFlagBuffer with at least `values` values and exactly `flags` flags."""
    if not isinstance(fb, HostFlagBuffer):
        raise TypeError(f"pyxu_amd: `{name}` must be a HostFlagBuffer (got {type(fb).__name__}).")
    if len(fb.values) < values or len(fb.flags) != flags:
        raise ValueError(f"pyxu_amd: `{name}` must be a HostFlagBuffer of >= {values} values and {flags} flags.")
    return fb


def _publication(host, name=None, rows=None):
    """(seq, values pointer, flags pointer) of a statistic a kernel publishes to `host`: a HostFlagBuffer (a new
    sequence number; checked to hold `rows` values and flags when `rows` is given), a pinned tensor, or None."""
    if isinstance(host, HostFlagBuffer):
        if rows is not None:
            flag_buffer(host, name, rows, rows)
        return host.next_seq(), host.vptr, host.fptr
    return 0, (None if host is None else host.data_ptr()), None


def ptr(t) -> int:
    return t.data_ptr()


def _p(t):
    return None if t is None else t.data_ptr()


def _launch(fn, *args):
    """The C entry fn(*args) under the bench timer hook (set_launch_timer; normally absent); a non-zero status raises."""
    timer = _TIMER
    if timer is not None:
        timer.begin()
    r = fn(*args)
    if r:
        check(r, fn.__name__)
    if timer is not None:
        timer.end()


def _workspace_bytes(name, *args, unsupported_ok=False):
    """lib.<name>(*args), a `*_workspace_bytes` query.  Its (size_t)-1 answer, arguments outside the kernel's
    envelope, raises as PXA_ERR_UNSUPPORTED (or returns None with `unsupported_ok`)."""
    n = int(getattr(lib, name)(*args))
    if n == (1 << 64) - 1:
        if unsupported_ok:
            return None
        check(-3, name)  # PXA_ERR_UNSUPPORTED
    return n


def _workspace(name, like, *args, f64=False):
    """The workspace that query asks for, on like's device: float64 of at least one element with `f64`, otherwise
    uint8, or None when no byte is needed."""
    n = _workspace_bytes(name, *args)
    torch = _torch()
    if f64:
        return torch.empty((max((n + 7) // 8, 1),), dtype=torch.float64, device=like.device)
    return torch.empty((n,), dtype=torch.uint8, device=like.device) if n else None


def _raw_stream_fn():
    torch = _torch()
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    dev = getattr(torch._C, "_cuda_getDevice", None)
    if get is None or dev is None:  # pragma: no cover - older torch
        return lambda: torch.cuda.current_stream().cuda_stream
    return lambda: get(dev())


_RAW_STREAM = None


def stream():
    """hipStream_t of torch's current stream on the current device (fast path: the raw-stream query,
    ~10x cheaper than torch.cuda.current_stream(), which matters at tens of us per solver step)."""
    global _RAW_STREAM
    if _RAW_STREAM is None:
        _RAW_STREAM = _raw_stream_fn()
    return ct.c_void_p(_RAW_STREAM())


_TSTREAM = (None, None)  # (raw hipStream_t, torch stream object) of the last record_event


def record_event(ev):
    """ev.record() on torch's current stream, without torch.cuda.current_stream()'s Python device lookup on
    every call (a few microseconds, paid once per solver step at stop_rate 1): the torch stream object is
    cached per raw stream."""
    global _TSTREAM
    torch = _torch()
    key = (_RAW_STREAM() if _RAW_STREAM is not None else None, torch._C._cuda_getDevice())
    if key[0] is None or key != _TSTREAM[0]:
        _TSTREAM = (key, torch.cuda.current_stream())
    ev.record(_TSTREAM[1])
    return ev


class LaunchTimer:
    """HIP-event windows around runs of back-to-back fused solver-step launches.

    Measurement hook for bench.py: while installed (``set_launch_timer``), the fused step kernels
    open a window (start event on the launch stream = torch's current stream, which the kernel runs
    on) and close it after ``window`` consecutive launches, or earlier when any other device work
    (a stop-criterion reduction / copy) is about to be enqueued (``interrupt``).  ``mean_ms()`` =
    total window time / launches inside windows = the average launch duration, measured live on
    the timed region's own launches, with one event pair per window rather than per launch.

    ``single=True``: ONE window over the whole timed region, opened right AFTER the first launch (so
    that the first launch's start-up latency on an idle device is not counted) and closed by
    ``close()``; interrupts are ignored, so the window also holds the stop checks' small kernels and
    any host-bound gap between launches (an upper bound on the kernel's own duration).  Two events in
    the region instead of two per interrupted window: the per-step windows cost ~2.4 us of host time
    per PGD step at 2048^2 (40.3 k vs 37.1 k image-it/s, profiles/r04p_timer_ab.txt).
    """

    def __init__(self, window=10, single=False):
        self.windows = []  # (ev0, ev1, launches)
        self.window = max(1, int(window))
        self.single = bool(single)
        self._open = None
        self._count = 0
        self._first = True
        # single mode: both events created here, outside the timed region (creating one costs host time)
        self._spare = [_torch().cuda.Event(enable_timing=True) for _ in range(2)] if self.single else []

    def _event(self):
        ev = self._spare.pop(0) if self._spare else _torch().cuda.Event(enable_timing=True)
        ev.record(_torch().cuda.current_stream())
        return ev

    def begin(self):
        if self.single:
            return True
        if self._open is None:
            self._open = self._event()
            self._count = 0
        return True

    def end(self, _tok=None):
        if self.single:
            if self._first:  # the window starts behind the first launch
                self._first = False
                self._open = self._event()
                self._count = 0
            else:
                self._count += 1
            return
        self._count += 1
        if self._count >= self.window:
            self.interrupt()

    def interrupt(self):
        if self.single:
            return
        self.close()

    def close(self):
        if self._open is not None and self._count > 0:
            self.windows.append((self._open, self._event(), self._count))
        self._open = None
        self._count = 0

    @property
    def launches(self):
        return sum(c for _, _, c in self.windows)

    def mean_ms(self):
        self.close()
        if not self.windows:
            return None
        self.windows[-1][1].synchronize()
        return sum(a.elapsed_time(b) for a, b, _ in self.windows) / self.launches


_TIMER = None


def set_launch_timer(timer):
    """Install (or remove, with None) the LaunchTimer of the fused solver-step kernels."""
    global _TIMER
    _TIMER = timer


_USE_COUNT = None


def storage_exclusive(t) -> bool:
    """True iff no other tensor shares `t`'s storage.  Solvers overwrite a buffer in place only when
    the Python reference count of the tensor object says nobody else holds it AND this holds: views
    such as ``img.reshape(-1)`` or ``batch[i]`` passed as x0 / z0 keep the storage's use count above
    that of a lone tensor.  The reference allocates fresh arrays every step, so anything a user can
    still reach must never be written."""
    global _USE_COUNT
    if _USE_COUNT is None:
        torch = _torch()
        _USE_COUNT = getattr(torch._C, "_storage_Use_Count", None) or (lambda _c: 1 << 30)
    # a lone tensor: its TensorImpl + the temporary storage wrapper created here
    return _USE_COUNT(t.untyped_storage()._cdata) <= 2


TUNE_NORMAL_KERNEL = 1  # PXA_TUNE_NORMAL_KERNEL: pxa_dense_normal A/B (0 row-split, 1 one workgroup per row, 2 row-split without the exchange)
TUNE_DENSE_KERNEL = 2  # PXA_TUNE_DENSE_KERNEL: 0 LDS-staged MFMA GEMM (B >= 32), 1 the register-streamed kernel
TUNE_DUAL_WGS = 4  # PXA_TUNE_DUAL_WGS: kernel C's target workgroup count (A/B; 0 = default)
TUNE_PGD_DIAG = 3  # PXA_TUNE_PGD_DIAG: bit 5 = s_memtime phase trace of the PGD tile kernel
TUNE_PDS_EVENTS = 5  # PXA_TUNE_PDS_EVENTS: per-kernel HIP events inside pxa_pds_step (pds_kernel_ms)
TUNE_FFT_KERNEL = 8  # PXA_TUNE_FFT_KERNEL: 0 in-place register-staged FFT kernel, 1 the ping-pong Stockham kernel
TUNE_GRAD_KERNEL = 9  # PXA_TUNE_GRAD_KERNEL: 0 axis-0 march gradient kernels, 1 the row kernels (same bits)
TUNE_STENCIL_ND = 10  # PXA_TUNE_STENCIL_ND: 0 LDS-tiled N-D stencil where it applies, 1 the generic kernel (same sums)
TUNE_DUAL_ROWS = 11  # PXA_TUNE_DUAL_ROWS: kernel C rows per thread (0 / 1 one-row kernel, 2 or 4 row-blocked; same bits)
# (keys 0, 6, 7, 12 are retired: pxa_tuning rejects them)


def tuning(key, value=-1):
    """Process-wide kernel-selection knob of the C-ABI (pxa_tuning): sets it when value >= 0 and
    returns the previous value.  For A/B measurements and variant-parity tests only."""
    r = int(lib.pxa_tuning(int(key), int(value)))
    if r < 0:
        check(r, "pxa_tuning")
    return r


def _tuning_from_env():
    """PXA_TUNE="key=value[,key=value...]" (keys: the PXA_TUNE_* numbers) sets knobs at import, so that A/B
    runs of bench.py / scripts need no code change."""
    spec = os.environ.get("PXA_TUNE", "").strip()
    for item in filter(None, (t.strip() for t in spec.split(","))):
        k, _, v = item.partition("=")
        try:
            tuning(int(k), int(v))
        except (ValueError, TypeError, RuntimeError) as e:  # a malformed item must not break the import
            import warnings

            warnings.warn(f"PXA_TUNE: ignoring {item!r} ({e})", RuntimeWarning, stacklevel=2)


def empty(shape, like):
    return _torch().empty(shape, dtype=like.dtype, device=like.device)


def empty_f64(shape, like):
    return _torch().empty(shape, dtype=_torch().float64, device=like.device)


def to_device_like(a, like):
    """Host numpy array -> device tensor of `like`'s dtype (an upload, no compute)."""
    return _torch().as_tensor(np.ascontiguousarray(a), device=like.device).to(like.dtype)


def empty_like(t):
    return _torch().empty_like(t, memory_format=_torch().contiguous_format)


def copy(x):
    x = require(x)
    return x.clone(memory_format=_torch().contiguous_format)


def scalar_dt(x):
    return np.float32 if dtcode(x) == 0 else np.float64


# ------------------------------------------------------------------ element-wise
# (`out` may be any input: include/pyxu_amd.h, element-wise kernels)
def axpby(a, x, b=0.0, y=None, out=None):
    """out = a*x + b*y."""
    x = require(x, "x")
    if y is not None:
        y = require(y, "y", like=x, numel=x.numel())
    out = _out(out, x)
    check(lib.pxa_axpby(dtcode(x), x.numel(), float(a), ptr(x), float(b), _p(y), ptr(out), stream()), "pxa_axpby")
    return out


def axpby_bcast(a, x, b, y, out=None):
    """out = a*x + b*y with y (M,) broadcast over x's leading dims (x: (..., M))."""
    x, y = require(x, "x"), require(y, "y")
    if y.numel() == x.numel():
        return axpby(a, x, b, y, out=out)
    out = _out(out, x)
    check(lib.pxa_axpby_bcast(dtcode(x), x.numel(), float(a), ptr(x), float(b), ptr(y), y.numel(), ptr(out), stream()), "pxa_axpby_bcast")
    return out


def axpy_rows(c, s, x, y, out=None):
    """out[r] = y[r] + s * c[r] * x[r] for x, y of shape (rows, n); c a (rows,) device vector."""
    x, y, c = require(x, "x"), require(y, "y"), require(c, "c")
    rows = c.numel()
    out = _out(out, y)
    check(lib.pxa_axpy_rows(dtcode(x), rows, x.numel() // max(rows, 1), ptr(c), float(s), ptr(x), ptr(y), ptr(out), stream()),
          "pxa_axpy_rows")
    return out


def row_ratio(num, den, like, out=None):
    """out[r] = num[r] / den[r] (float64 device vectors) cast to like's dtype, on the device."""
    num = require(num, "num", dtype="float64")
    den = require(den, "den", dtype="float64", numel=num.numel())
    out = _out(out, like, (num.numel(),))
    check(lib.pxa_row_ratio(dtcode(like), num.numel(), ptr(num), ptr(den), ptr(out), stream()), "pxa_row_ratio")
    return out


def lincomb3(a, x, b, y, c, z, out=None):
    x, y, z = require(x), require(y), require(z)
    out = _out(out, x)
    check(lib.pxa_lincomb3(dtcode(x), x.numel(), float(a), ptr(x), float(b), ptr(y), float(c), ptr(z), ptr(out), stream()), "pxa_lincomb3")
    return out


def extrapolate(a, x, y, out=None):
    """(x - y) * a + x."""
    x, y = require(x), require(y)
    out = _out(out, x)
    check(lib.pxa_extrapolate(dtcode(x), x.numel(), float(a), ptr(x), ptr(y), ptr(out), stream()), "pxa_extrapolate")
    return out


def div(x, d, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_div(dtcode(x), x.numel(), ptr(x), float(d), ptr(out), stream()), "pxa_div")
    return out


def add_scalar(x, s, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_add_scalar(dtcode(x), x.numel(), ptr(x), float(s), ptr(out), stream()), "pxa_add_scalar")
    return out


def fill(out, v):
    if _TIMER is not None:  # (as `require`: device work outside the fused steps closes the timing window)
        _TIMER.interrupt()
    out = written(out)
    check(lib.pxa_fill(dtcode(out), out.numel(), float(v), ptr(out), stream()), "pxa_fill")
    return out


def zeros(shape, like):
    return fill(empty(shape, like), 0.0)


def mul(x, y, out=None):
    x, y = require(x), require(y)
    out = _out(out, x)
    check(lib.pxa_mul(dtcode(x), x.numel(), ptr(x), ptr(y), ptr(out), stream()), "pxa_mul")
    return out


def clip(x, lo, hi=None, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_clip(dtcode(x), x.numel(), ptr(x), float(lo), float(hi or 0.0), int(hi is not None), ptr(out), stream()), "pxa_clip")
    return out


def prox_l1(x, tau, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_prox_l1(dtcode(x), x.numel(), ptr(x), float(tau), ptr(out), stream()), "pxa_prox_l1")
    return out


def admm_l1_update(x, z, u, cgrad, rho_m1, thr, tau):
    """ADMM outer update (h = lam L1, K = Id) + the next CG right-hand side in one launch
    (pxa_admm_l1_update): returns (u', z', b, r0, p0, x0), views of one (6, *x.shape) buffer."""
    x = require(x)
    n = x.numel()
    z, u, cgrad = (require(t, name, like=x, numel=n) for t, name in ((z, "z"), (u, "u"), (cgrad, "cgrad")))
    out = empty((6,) + tuple(x.shape), x)
    check(lib.pxa_admm_l1_update(dtcode(x), n, ptr(x), ptr(z), ptr(u), ptr(cgrad), float(rho_m1), float(thr),
                                 float(tau), ptr(out), stream()), "pxa_admm_l1_update")
    return tuple(out.unbind(0))


def fenchel_prox_l1(x, sigma, lam, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_fenchel_prox_l1(dtcode(x), x.numel(), ptr(x), float(sigma), float(lam), ptr(out), stream()), "pxa_fenchel_prox_l1")
    return out


def moreau_grad_l1(x, mu, scale, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_moreau_grad_l1(dtcode(x), x.numel(), ptr(x), float(mu), float(scale), ptr(out), stream()), "pxa_moreau_grad_l1")
    return out


def _grouped(x, outer, group, inner):
    """x of an (outer, group, inner) kernel, which reads outer * group * inner elements."""
    return require(x, "x", numel=int(outer) * int(group) * int(inner))


def prox_l21(x, tau, outer, group, inner, out=None):
    x = _grouped(x, outer, group, inner)
    out = _out(out, x)
    check(lib.pxa_prox_l21(dtcode(x), outer, group, inner, ptr(x), float(tau), ptr(out), stream()), "pxa_prox_l21")
    return out


def fenchel_prox_l21(x, sigma, lam, outer, group, inner, out=None):
    x = _grouped(x, outer, group, inner)
    out = _out(out, x)
    check(
        lib.pxa_fenchel_prox_l21(dtcode(x), outer, group, inner, ptr(x), float(sigma), float(lam), ptr(out), stream()),
        "pxa_fenchel_prox_l21",
    )
    return out


def moreau_grad_l21(x, mu, scale, outer, group, inner, out=None):
    x = _grouped(x, outer, group, inner)
    out = _out(out, x)
    check(
        lib.pxa_moreau_grad_l21(dtcode(x), outer, group, inner, ptr(x), float(mu), float(scale), ptr(out), stream()),
        "pxa_moreau_grad_l21",
    )
    return out


def group_norm(x, outer, group, inner):
    x = _grouped(x, outer, group, inner)
    out = empty((outer * inner,), x)
    check(lib.pxa_group_norm(dtcode(x), outer, group, inner, ptr(x), ptr(out), stream()), "pxa_group_norm")
    return out


# ------------------------------------------------------------------ array primitives (csrc/array.hip)
UN_SQRT, UN_SIGN, UN_ABS, UN_NEG, UN_SQUARE, UN_RECIP, UN_POSINF = range(7)
BIN_FMAX, BIN_FMIN, BIN_ADD, BIN_SUB, BIN_MUL, BIN_DIV, BIN_MAXIMUM, BIN_MINIMUM, BIN_POW = range(9)


def copy2d(src, dst, rows, n, lds, ldd, src_off=0, dst_off=0, accumulate=0, col_stride=1):
    """dst[dst_off + r*ldd + i] = src[src_off + r*lds + i*col_stride] for r < rows, i < n (element
    offsets; col_stride 0 repeats one value per row); accumulate 1: dst += src; 2: dst = 0 + src (the
    first term of a Python sum)."""
    es = src.element_size()
    check(lib.pxa_copy2d(dtcode(src), int(rows), int(n), ptr(src) + int(src_off) * es, int(lds), int(col_stride),
                         ptr(dst) + int(dst_off) * es, int(ldd), int(accumulate), stream()), "pxa_copy2d")
    return dst


def take_cols(x, off, n):
    """x[..., off:off + n] as a contiguous device array (a view when x has no leading stack)."""
    x = require(x)
    d = x.shape[-1]
    if x.ndim == 1 or x.numel() == d:
        return x.reshape(-1)[off:off + n].reshape(*x.shape[:-1], n)
    rows = x.numel() // d
    out = empty((*x.shape[:-1], n), x)
    return copy2d(x, out, rows, n, d, n, src_off=off)


def concat_cols(parts, out=None):
    """numpy.concatenate(parts, axis=-1) for device arrays with equal leading shapes."""
    parts = [require(p) for p in parts]
    lead = parts[0].shape[:-1]
    total = sum(p.shape[-1] for p in parts)
    out = _out(out, parts[0], (*lead, total), apart=parts)
    rows = out.numel() // max(total, 1)
    off = 0
    for p in parts:
        copy2d(p, out, rows, p.shape[-1], p.shape[-1], total, dst_off=off)
        off += p.shape[-1]
    return out


def unary(op, x, out=None):
    x = require(x)
    out = _out(out, x)
    check(lib.pxa_unary(dtcode(x), int(op), x.numel(), ptr(x), ptr(out), stream()), "pxa_unary")
    return out


def binary(op, x, y, out=None, like=None):
    """out = op(x, y); x / y device arrays of one shape or Python scalars (broadcast)."""
    xa = None if np.isscalar(x) else require(x, "x")
    ya = None if np.isscalar(y) else require(y, "y", like=xa, shape=None if xa is None else xa.shape)
    ref = xa if xa is not None else (ya if ya is not None else like)
    out = _out(out, ref)
    check(lib.pxa_binary(dtcode(ref), int(op), ref.numel(), _p(xa), float(x) if xa is None else 0.0, _p(ya),
                         float(y) if ya is None else 0.0, ptr(out), stream()), "pxa_binary")
    return out


def where(cond, x, y, like=None):
    cond = require_bool(cond)
    xa = None if np.isscalar(x) else require(x, "x", numel=cond.numel())
    ya = None if np.isscalar(y) else require(y, "y", like=xa, numel=cond.numel())
    ref = xa if xa is not None else (ya if ya is not None else like)
    out = empty(cond.shape, ref)
    check(lib.pxa_where(dtcode(ref), out.numel(), cond.data_ptr(), _p(xa), float(x) if xa is None else 0.0, _p(ya),
                        float(y) if ya is None else 0.0, ptr(out), stream()), "pxa_where")
    return out


def isnan(x):
    torch = _torch()
    x = require(x)
    out = torch.empty(x.shape, dtype=torch.bool, device=x.device)
    check(lib.pxa_isnan(dtcode(x), x.numel(), ptr(x), out.data_ptr(), stream()), "pxa_isnan")
    return out


def bool_reduce(c, mode):
    """any (mode 0) / all (mode 1) of a boolean device tensor -> 0-d boolean device tensor."""
    torch = _torch()
    c = require_bool(c)
    out = torch.empty((), dtype=torch.bool, device=c.device)
    check(lib.pxa_bool_reduce(c.numel(), int(mode), c.data_ptr(), out.data_ptr(), stream()), "pxa_bool_reduce")
    return out


def cast(x, dtype_like):
    """(dtype of dtype_like) copy of x (float32 <-> float64)."""
    x = require(x)
    out = _torch().empty(x.shape, dtype=dtype_like.dtype, device=x.device)
    check(lib.pxa_cast(dtcode(x), dtcode(out), x.numel(), ptr(x), ptr(out), stream()), "pxa_cast")
    return out


def set_diag(out, rows, ld, off, value):
    rows, ld, off = int(rows), int(ld), int(off)
    if min(rows, ld, off) < 0:
        raise ValueError(f"pyxu_amd: set_diag needs rows, ld, off >= 0, got {(rows, ld, off)}.")
    written(out, at_least=(rows - 1) * (ld + 1) + off + 1 if rows else 0)  # the last element it sets
    check(lib.pxa_set_diag(dtcode(out), rows, ld, off, float(value), ptr(out), stream()), "pxa_set_diag")
    return out


def dir_contract(w, wp, x, S, G, J, K, N, adjoint=False):
    """pxa_dir_contract: y = sum_j w[g, j] * x[j % K] (apply, (S, K, N) -> (S, G, N)) or its adjoint."""
    x, w = require(x, "x"), require(w, "w")
    y = empty((S, K if adjoint else G, N), x)
    check(lib.pxa_dir_contract(dtcode(x), int(S), int(G), int(J), int(K), int(N), ptr(w), int(wp), ptr(x), ptr(y),
                               int(bool(adjoint)), stream()), "pxa_dir_contract")
    return y


def transpose(x):
    """(rows, cols) -> contiguous (cols, rows)."""
    x = require(x)
    rows, cols = x.shape
    out = empty((cols, rows), x)
    check(lib.pxa_transpose(dtcode(x), rows, cols, ptr(x), ptr(out), stream()), "pxa_transpose")
    return out


# ------------------------------------------------------------------ reductions
def relerr_stats(x, x_prev, out, copy=True):
    """RelError statistics in one pass (pxa_relerr_stats): out[0] = sum (x - x_prev)^2 and
    out[1] = sum x_prev^2 per row (out: contiguous float64 (2, rows) buffer, device or pinned host);
    returns the copy of x the criterion keeps (or None with copy=False)."""
    x = require(x)
    x_prev = require(x_prev, "x_prev", like=x, shape=x.shape)
    n = x.shape[-1] if x.ndim > 0 else 1
    rows = x.numel() // max(n, 1) if x.numel() else 0
    written(out, "out", dtype="float64", numel=2 * max(rows, 1), pinned=True)
    if not 0 < rows <= 65535:
        raise ValueError(f"relerr_stats: rows must be in [1, 65535], got {rows} (use row_reduce)")
    xc = empty_like(x) if copy else None
    work = _workspace("pxa_relerr_stats_workspace_bytes", x, rows, n, f64=True)
    check(lib.pxa_relerr_stats(dtcode(x), rows, n, ptr(x), ptr(x_prev), _p(xc), out.data_ptr(), ptr(work), stream()),
          "pxa_relerr_stats")
    return xc


def cg_update(x, r, p, ap, rr, rr_out, rr_host, work, have_pap=False):
    """pxa_cg_update: the CG iteration tail after A p on (rows, n) x / r / p / A p (in place), from this
    step's ||r||^2 `rr` (device float64 (rows,)); ||r'||^2 lands in rr_out (device) and in rr_host: a
    HostFlagBuffer(rows, rows, rows) (returns the publication's sequence number, which its wait() takes), a
    pinned host tensor, or None.  have_pap: `work` already holds the <p, A p> partials (pxa_cg_update_tail;
    dense_normal(..., pdot=work) wrote them with A p)."""
    rows, n = x.shape
    seq, vp_, fp_ = _publication(rr_host)
    fn = lib.pxa_cg_update_tail if have_pap else lib.pxa_cg_update
    check(fn(dtcode(x), rows, n, ptr(x), ptr(r), ptr(p), ptr(ap), rr.data_ptr(), rr_out.data_ptr(), vp_, fp_, seq,
             work.data_ptr(), stream()), "pxa_cg_update")
    return seq


def cg_update_xr(x, r, p, ap, rr, work):
    """pxa_cg_update_xr: x += alpha p, r -= alpha A p and the ||r'||^2 partials (work + rows * _CG_BLOCKS doubles), with the
    <p, A p> partials already in `work` (dense_normal(..., pdot=work)); the p update is left to the next
    dense_normal_pfold."""
    rows, n = x.shape
    check(lib.pxa_cg_update_xr(dtcode(x), rows, n, ptr(x), ptr(r), ptr(p), ptr(ap), rr.data_ptr(), work.data_ptr(),
                               stream()), "pxa_cg_update_xr")


def krylov_chunk(like):
    """Columns per workgroup chunk of the pxa_krylov_* kernels for `like`'s dtype."""
    return int(lib.pxa_krylov_chunk(dtcode(like)))


_KRYLOV_WORK = {}  # (j, n) -> doubles of pxa_krylov_workspace_bytes: a Lanczos solve asks once per basis size


def _krylov_doubles(j, n):
    need = _KRYLOV_WORK.get((j, n))
    if need is None:
        if len(_KRYLOV_WORK) > 256:
            _KRYLOV_WORK.clear()
        need = _KRYLOV_WORK[(j, n)] = _workspace_bytes("pxa_krylov_workspace_bytes", j, n) // 8
    return need


def krylov_workspace(j, n, like):
    """Workspace of pxa_krylov_dots / pxa_krylov_update for up to j rows of n (float64 device tensor)."""
    return _torch().zeros((max(_krylov_doubles(int(j), int(n)), 2),), dtype=_torch().float64, device=like.device)


def _krylov_basis(V, j, w, work):
    """(ldv, n) of the first j rows of V, a (rows, n) tensor or view with unit column stride, against the flat device
    vector w (n,) the kernels read as it is; `work` from krylov_workspace."""
    _operand(w, "w", None, None, None, None, "the Krylov step")
    _operand(V, "V", None, w, None, None, "the Krylov step")
    n = w.numel()
    if not (w.ndim == 1 and w.is_contiguous()):
        raise ValueError("pyxu_amd: `w` must be a contiguous vector")
    if not (V.ndim == 2 and V.shape[0] >= j and V.shape[1] == n and V.stride(1) == 1):
        raise ValueError(f"pyxu_amd: `V` of shape {tuple(V.shape)} does not hold {j} unit-stride rows of {n} entries")
    written(work, "work", dtype="float64", at_least=_krylov_doubles(int(j), n))
    return (V.stride(0) if V.shape[0] > 1 else n), n


def krylov_dots(V, j, w, c_out, work, scale=None):
    """pxa_krylov_dots: c_out[i] = scale * <V[i], w>, i < j (float64 device vector); scale: float64 device scalar."""
    ldv, n = _krylov_basis(V, j, w, work)
    written(c_out, "c_out", dtype="float64", at_least=int(j))
    if scale is not None:
        scale = require(scale, "scale", dtype="float64")
    check(lib.pxa_krylov_dots(dtcode(w), int(j), n, ptr(V), ldv, ptr(w), _p(scale), ptr(c_out), ptr(work), stream()),
          "pxa_krylov_dots")
    return c_out


def krylov_update(V, j, w, c, w_out, work, c_next=None, nrm2_out=None):
    """pxa_krylov_update: w_out = w - sum_i c[i] V[i] (w_out may be w), c_next[i] = <V[i], w_out> and nrm2_out =
    ||w_out||^2 when given (float64 device)."""
    ldv, n = _krylov_basis(V, j, w, work)
    c = require(c, "c", dtype="float64")
    written(w_out, "w_out", like=w, numel=n)
    if c_next is not None:
        written(c_next, "c_next", dtype="float64", at_least=int(j), apart=(c,))
    if nrm2_out is not None:
        written(nrm2_out, "nrm2_out", dtype="float64", at_least=1)
    check(lib.pxa_krylov_update(dtcode(w), int(j), n, ptr(V), ldv, ptr(w), ptr(c), ptr(w_out), _p(c_next), _p(nrm2_out),
                                ptr(work), stream()), "pxa_krylov_update")
    return w_out


def krylov_normalize(x, nrm2, out):
    """pxa_krylov_normalize: out = x / sqrt(nrm2) with nrm2 a float64 device scalar (a zero row for nrm2 == 0); out
    may be x."""
    x = require(x, "x")
    nrm2 = require(nrm2, "nrm2", dtype="float64")
    written(out, "out", like=x, numel=x.numel())
    check(lib.pxa_krylov_normalize(dtcode(x), x.numel(), ptr(x), ptr(nrm2), ptr(out), stream()), "pxa_krylov_normalize")
    return out


# (the integer constants below mirror include/pyxu_amd.h's PXA_* #defines; tests/test_abi_table.py compares them)
NLCG_FR, NLCG_PR = 0, 1  # PXA_NLCG_*: pxa_nlcg_direction variants
_CG_BLOCKS = 64  # PXA_CG_BLOCKS: partials per row and plane of the CG / NLCG workspaces (layouts: include/pyxu_amd.h)


def nlcg_blocks(n):
    """Partials per row that pxa_nlcg_direction leaves for pxa_ls_armijo: min(PXA_CG_BLOCKS, ceil(n / 256))."""
    return min(_CG_BLOCKS, (int(n) + 255) // 256)


def nlcg_gp_partials(work, rows):
    """The <g1, p_new> partials of a pxa_nlcg_direction workspace (float64 device tensor `work`): its third plane."""
    return work[2 * rows * _CG_BLOCKS: 3 * rows * _CG_BLOCKS]


def nlcg_direction(variant, restart, g1, g0, p, p_new, gg0, gg_out, gg_host, work):
    """pxa_nlcg_direction on (rows, n) g1 / g0 / p -> p_new = beta p - g1 (out of place), beta from `variant`
    (NLCG_FR / NLCG_PR), this step's g1, the previous g0 (None allowed for FR or a restart) and gg0 = sum g0^2
    (device float64 (rows,)); sum g1^2 lands in gg_out (device, not gg0) and in gg_host (a
    HostFlagBuffer(rows, rows, rows): returns the publication's sequence number; a pinned tensor; or None).
    `work`: float64 device tensor of pxa_nlcg_workspace_bytes(rows) bytes; nlcg_gp_partials(work, rows) then
    holds the <g1, p_new> partials."""
    ctx = "nlcg_direction"
    g1 = require(g1, "g1", ctx=ctx)
    if g1.dim() != 2:
        raise ValueError("nlcg_direction: g1, p and p_new must be (rows, n) tensors of one dtype")
    rows, n = g1.shape
    if not (1 <= rows <= 65535 and n >= 1):
        raise ValueError(f"nlcg_direction: rows must be in [1, 65535] and n >= 1, got {(rows, n)}")
    if variant not in (NLCG_FR, NLCG_PR):
        raise ValueError(f"nlcg_direction: unknown variant {variant}")
    p = require(p, "p", like=g1, shape=g1.shape, ctx=ctx)
    if g0 is not None:
        g0 = require(g0, "g0", like=g1, shape=g1.shape, ctx=ctx)
    elif variant == NLCG_PR and not restart:
        raise ValueError("nlcg_direction: the PR variant needs g0")
    written(p_new, "p_new", like=g1, numel=rows * n, apart=(p, g1), ctx=ctx)
    gg0 = require(gg0, "gg0", dtype="float64", numel=rows, ctx=ctx)
    written(gg_out, "gg_out", dtype="float64", numel=rows, apart=(gg0,), ctx=ctx)
    written(work, "work", dtype="float64", at_least=_workspace_bytes("pxa_nlcg_workspace_bytes", rows) // 8, ctx=ctx)
    seq, vp_, fp_ = _publication(gg_host, "gg_host", rows)
    check(lib.pxa_nlcg_direction(dtcode(g1), int(variant), int(bool(restart)), rows, n, ptr(g1), _p(g0), ptr(p),
                                 ptr(p_new), gg0.data_ptr(), gg_out.data_ptr(), vp_, fp_, seq, work.data_ptr(), stream()),
          "pxa_nlcg_direction")
    return seq


def ls_armijo(f_trial, f_x, gp, nb, c, r, a, trials, fb):
    """pxa_ls_armijo: the Armijo test of one backtracking trial on every row.  f_trial, f_x, a: `rows` values of
    one dtype (a is updated in place: a *= r where f_trial > f_x + a c <g, p>); gp: float64 device, nb partials
    per row (nb > 0, as nlcg_gp_partials) or one folded value per row (nb == 0); trials: int32 device (rows,),
    incremented on failing rows; fb: a HostFlagBuffer(1, 1, 1) that receives the number of failing rows
    (ls_failed(fb, seq) reads it).  Returns the publication's sequence number."""
    ctx = "ls_armijo"
    written(a, "a", ctx=ctx)
    rows = a.numel()
    if not 1 <= rows <= 65535:
        raise ValueError(f"ls_armijo: rows must be in [1, 65535], got {rows}")
    f_trial = require(f_trial, "f_trial", like=a, numel=rows, ctx=ctx)
    f_x = require(f_x, "f_x", like=a, numel=rows, ctx=ctx)
    nb = int(nb)
    if not 0 <= nb <= _CG_BLOCKS:
        raise ValueError(f"ls_armijo: nb must be in [0, {_CG_BLOCKS}], got {nb}")
    written(gp, "gp", dtype="float64", at_least=rows * max(nb, 1), ctx=ctx)  # (read only, but taken as it is: a view)
    written(trials, "trials", dtype="int32", numel=rows, ctx=ctx)
    seq = flag_buffer(fb, "fb", 1, 1).next_seq()
    check(lib.pxa_ls_armijo(dtcode(a), rows, ptr(f_trial), ptr(f_x), gp.data_ptr(), nb, float(c), float(r), ptr(a),
                            trials.data_ptr(), fb.vptr, fb.fptr, seq, stream()), "pxa_ls_armijo")
    return seq


def ls_failed(fb, seq):
    """Number of rows that failed the Armijo test of publication `seq` (waits for its flag; one 4-byte read)."""
    fb.wait(seq)
    return int(fb.values.view(np.uint32)[0])


PROXADAM_VARIANTS = {"adam": 0, "amsgrad": 1, "padam": 2}  # PXA_PROXADAM_*: pxa_proxadam_moments variants
PROX_L1, PROX_POS, PROX_POSL1, PROX_BOX = 1, 2, 3, 4  # PXA_PROX_*: element-wise prox kinds
_PROXADAM_PLANES = 5  # planes of rows * nb doubles that open a ProxAdam workspace (layout: include/pyxu_amd.h)


def proxadam_blocks(rows, n):
    """Workgroups (= partials) per row of the ProxAdam kernels."""
    return int(lib.pxa_proxadam_blocks(int(rows), int(n)))


def proxadam_workspace(rows, n, like):
    """A float64 device tensor of pxa_proxadam_workspace_bytes(rows, n) bytes."""
    return _workspace("pxa_proxadam_workspace_bytes", like, int(rows), int(n), f64=True)


def proxadam_work_views(work, rows, n):
    """(psi partial maxima (rows, nb), psimax (rows,), state words int32 (rows,)) of a ProxAdam workspace."""
    plane = rows * proxadam_blocks(rows, n)
    psimax = _PROXADAM_PLANES * plane
    tail = work[psimax + rows:].view(_torch().int32)
    return work[:plane].reshape(rows, -1), work[psimax: psimax + rows], tail[:rows]


def proxadam_stat_partials(work, rows, n, k):
    """The (2, rows, nb) partials sum (z_new - z)^2 / sum z^2 that sub-step launch `k` left: the pair of planes
    behind the psi maxima's for even k, the next pair for odd k."""
    plane = rows * proxadam_blocks(rows, n)
    off = plane * (1 + 2 * (k & 1))
    return work[off: off + 2 * plane].reshape(2, rows, -1)


def _proxadam_work(work, rows, n, ctx):
    return written(work, "work", dtype="float64", ctx=ctx,
                   at_least=(_workspace_bytes("pxa_proxadam_workspace_bytes", rows, n) + 7) // 8)


def proxadam_moments(variant, first, g, m, v, vhat, x, m_out, v_out, vhat_out, x_out, b1, omb1, b2, omb2, eps_var, c1,
                     c2, eps_adam, a, p, psi_out=None, work=None):
    """pxa_proxadam_moments on (rows, n) operands: the ProxAdam moment update and gradient step in one launch
    (include/pyxu_amd.h).  m_out / v_out / vhat_out may be m / v / vhat; x_out is a buffer of its own; vhat may be
    None when `first`.  With psi_out, psi is stored and `work` (proxadam_workspace) receives its partial maxima."""
    if variant not in PROXADAM_VARIANTS.values():
        raise ValueError(f"proxadam_moments: unknown variant {variant}")
    if g.dim() != 2:
        raise ValueError("proxadam_moments: operands must be (rows, n) tensors")
    dtcode(g)
    rows, n = g.shape
    if not (1 <= rows <= 65535 and n >= 1):
        raise ValueError(f"proxadam_moments: rows must be in [1, 65535] and n >= 1, got {(rows, n)}")
    ops = dict(g=g, m=m, v=v, x=x, m_out=m_out, v_out=v_out, vhat_out=vhat_out, x_out=x_out)
    if not first or vhat is not None:
        ops["vhat"] = vhat
    if psi_out is not None:
        ops["psi_out"] = psi_out
    for name, t in ops.items():  # (every operand as it is, inputs too: the solver passes views of one state buffer)
        if t is None:
            raise ValueError(f"proxadam_moments: {name} is missing")
        written(t, name, like=g, numel=rows * n, ctx="proxadam_moments",
                apart=[o for k, o in ops.items() if k != name] if name in ("x_out", "psi_out") else ())
    if psi_out is not None:
        if work is None:
            raise ValueError("proxadam_moments: psi_out needs the workspace")
        _proxadam_work(work, rows, n, "proxadam_moments")
    check(lib.pxa_proxadam_moments(dtcode(g), int(variant), int(bool(first)), rows, n, float(b1), float(omb1), float(b2),
                                   float(omb2), float(eps_var), float(c1), float(c2), float(eps_adam), float(a), float(p),
                                   ptr(g), ptr(m), ptr(v), _p(vhat), ptr(x), ptr(m_out), ptr(v_out), ptr(vhat_out),
                                   ptr(x_out), _p(psi_out), _p(work), stream()), "pxa_proxadam_moments")
    return x_out


def proxadam_sub_init(rows, n, work):
    """pxa_proxadam_sub_init: psimax per row from the partial maxima pxa_proxadam_moments left in `work`; state words
    and counters cleared."""
    rows, n = int(rows), int(n)
    if not (1 <= rows <= 65535 and n >= 1):
        raise ValueError(f"proxadam_sub_init: rows must be in [1, 65535] and n >= 1, got {(rows, n)}")
    _proxadam_work(work, rows, n, "proxadam_sub_init")
    check(lib.pxa_proxadam_sub_init(rows, n, work.data_ptr(), stream()), "pxa_proxadam_sub_init")


def proxadam_sub_step(kind, k, mom, eps, a, pw, xt, psi, z_prev, z, z_new, out, work, fb):
    """pxa_proxadam_sub_step: sub-iteration `k` (1-based; z = z_prev = xt at k == 1) of the metric prox on every row
    that still runs (include/pyxu_amd.h).  fb: a HostFlagBuffer(1, 1, 1) that receives the number of rows that
    computed an update (proxadam_running(fb, seq) reads it).  Returns the publication's sequence number."""
    if kind not in (PROX_L1, PROX_POS, PROX_POSL1, PROX_BOX):
        raise ValueError(f"proxadam_sub_step: unknown prox kind {kind}")
    if xt.dim() != 2:
        raise ValueError("proxadam_sub_step: operands must be (rows, n) tensors")
    dtcode(xt)
    rows, n = xt.shape
    if not (1 <= rows <= 65535 and n >= 1 and int(k) >= 1):
        raise ValueError(f"proxadam_sub_step: rows must be in [1, 65535], n >= 1 and k >= 1, got {(rows, n, k)}")
    ops = dict(xt=xt, psi=psi, z_prev=z_prev, z=z, z_new=z_new, out=out)
    for name, t in ops.items():
        written(t, name, like=xt, numel=rows * n, ctx="proxadam_sub_step",
                apart=[o for q, o in ops.items() if q != name] if name in ("z_new", "out") else ())
    _proxadam_work(work, rows, n, "proxadam_sub_step")
    seq = flag_buffer(fb, "fb", 1, 1).next_seq()
    check(lib.pxa_proxadam_sub_step(dtcode(xt), int(kind), int(k), rows, n, float(mom), float(eps), float(a), float(pw),
                                    ptr(xt), ptr(psi), ptr(z_prev), ptr(z), ptr(z_new), ptr(out), work.data_ptr(),
                                    fb.vptr, fb.fptr, seq, stream()), "pxa_proxadam_sub_step")
    return seq


def proxadam_running(fb, seq):
    """Number of rows that computed an update in the sub-step launch of publication `seq` (waits for its flag)."""
    fb.wait(seq)
    return int(fb.values.view(np.uint32)[0])


# ------------------------------------------------------------------ Langevin samplers (csrc/sampler.hip)
def _counter(v, name):
    v = int(v)
    if v < 0 or v >> 64:
        raise ValueError(f"sampler: {name} must fit 64 unsigned bits, got {v}")
    return v


def philox_normal(out, seed, step, e0=0):
    """pxa_philox_normal: out (flat) = the standard normals of global elements e0 .. e0 + out.numel() - 1 of the
    stream (seed, step) (include/pyxu_amd.h)."""
    written(out)
    check(lib.pxa_philox_normal(dtcode(out), out.numel(), _counter(seed, "seed"), _counter(step, "step"),
                                _counter(e0, "e0"), ptr(out), stream()), "pxa_philox_normal")
    return out


def langevin_step(kind, gamma, lam, pw, x, grad, x_out, noise=None, seed=0, step=0, e0=0):
    """pxa_langevin_step: x_out = (x - gamma (grad + m)) + sqrt(2 gamma) z, m the Moreau-Yosida gradient of the
    element-wise g of `kind` (0: none, else PROX_*), z = noise or the Philox normal of (seed, step, e0 + i).  x_out
    may be x."""
    if kind not in (0, PROX_L1, PROX_POS, PROX_POSL1, PROX_BOX):
        raise ValueError(f"langevin_step: unknown kind {kind}")
    written(x, "x", ctx="langevin_step")  # (inputs as they are too: the samplers pass views of their chain state)
    n = x.numel()
    written(grad, "grad", like=x, numel=n, ctx="langevin_step")
    if noise is not None:
        written(noise, "noise", like=x, numel=n, ctx="langevin_step")
    written(x_out, "x_out", like=x, numel=n, apart=(grad, noise), ctx="langevin_step")  # (x_out may be x)
    if not float(gamma) > 0 or (kind != 0 and not float(lam) > 0):
        raise ValueError(f"langevin_step: gamma and lam must be positive, got {(gamma, lam)}")
    check(lib.pxa_langevin_step(dtcode(x), int(kind), n, float(gamma), float(lam), float(pw), _counter(seed, "seed"),
                                _counter(step, "step"), _counter(e0, "e0"), ptr(x), ptr(grad),
                                _p(noise), ptr(x_out), stream()), "pxa_langevin_step")
    return x_out


def online_moments(order, k, x, mean, sums):
    """pxa_online_moments: sample number k (0-based) folded into mean (x's dtype) and sums ((order - 1, n) float64)."""
    if order not in (2, 3, 4) or int(k) < 0:
        raise ValueError(f"online_moments: order must be 2, 3 or 4 and k >= 0, got {(order, k)}")
    written(x, "x", ctx="online_moments")  # (as it is: a view of the sampler's chain state)
    n = x.numel()
    written(mean, "mean", like=x, numel=n, apart=(x,), ctx="online_moments")
    written(sums, "sums", dtype="float64", numel=(order - 1) * n, apart=(x,), ctx="online_moments")
    check(lib.pxa_online_moments(dtcode(x), int(order), int(k), n, ptr(x), ptr(mean), ptr(sums), stream()),
          "pxa_online_moments")
    return mean, sums


def dense_normal_pfold(A, r, p, p_new, rr, rr_out, fb, seq, s, d, work, pdot):
    """pxa_dense_normal_pdot_pfold: p_new = r + beta p (the CG's previous p update, beta from cg_update_xr's ||r'||^2
    partials in pdot's second plane, the CG workspace layout of one row, and `rr`), then Y = s A^T (A p_new) + d p_new
    and the <p_new, Y> partials into pdot; ||r'||^2 into rr_out (device) and HostFlagBuffer `fb` under publication
    `seq`.  Returns Y."""
    M, N = A.shape
    if p.numel() != N:  # one right-hand side: the planes of the CG workspace hold rows * _CG_BLOCKS doubles each
        raise ValueError(f"pxa_dense_normal_pdot_pfold: p must be a single row of {N} entries, got {tuple(p.shape)}")
    wsz = int(lib.pxa_dense_normal_workspace_bytes(dtcode(p), M, N, 1))
    if wsz == 0 or work is None or work.numel() < wsz:
        raise ValueError("pxa_dense_normal_pdot_pfold: unsupported operand or workspace")
    Y = empty(p.shape, p)
    rr_parts = pdot.data_ptr() + _CG_BLOCKS * pdot.element_size()
    check(lib.pxa_dense_normal_pdot_pfold(dtcode(p), M, N, ptr(A), ptr(r), ptr(p), ptr(p_new), rr.data_ptr(),
                                          rr_parts, rr_out.data_ptr(), fb.vptr, fb.fptr, int(seq),
                                          float(s), float(d), ptr(Y), ptr(work), pdot.data_ptr(), stream()),
          "pxa_dense_normal_pdot_pfold")
    return Y


def tile_partials_fold(parts, rows, per_row, out):
    """RelError statistics from the fused PGD step's per-tile partials (pxa_tile_partials_fold):
    out (contiguous float64 (2, rows), device or pinned host) = per-row sum (x_new - x)^2, sum x^2."""
    written(out, "out", dtype="float64", numel=2 * rows, pinned=True)
    check(lib.pxa_tile_partials_fold(int(rows), int(per_row), parts.data_ptr(), out.data_ptr(), None, 0, stream()),
          "pxa_tile_partials_fold")
    return out


def tile_partials_publish(parts, rows, per_row, fb, seq):
    """pxa_tile_partials_fold of `parts` into HostFlagBuffer `fb` under an existing publication number `seq`."""
    check(lib.pxa_tile_partials_fold(int(rows), int(per_row), parts.data_ptr(), fb.vptr, fb.fptr, int(seq), stream()),
          "pxa_tile_partials_fold")


class FlagWaitError(RuntimeError):
    """A HostFlagBuffer publication never landed although its stream is idle."""


def wait_flags(flags, seq, spin_s, stream_idle):
    """Host side of HostFlagBuffer.wait: busy-poll `flags` (uint32 array in coherent host memory) for
    `spin_s` seconds, then poll with a yield, asking `stream_idle()` each round.  Once the stream reports idle
    every write of the kernels before it has landed, so flags that still differ from `seq` after one more
    look will never change: raise FlagWaitError (the wait used to spin forever there)."""
    import time

    if len(flags) == 2:  # (one row: two flags, compared as scalars -- ~20x cheaper than the array compare)
        if flags[0] == seq and flags[1] == seq:
            return
    elif (flags == seq).all():
        return
    t_end = time.perf_counter() + spin_s
    while not (flags == seq).all():
        if time.perf_counter() > t_end:
            if stream_idle() and not (flags == seq).all():
                raise FlagWaitError(
                    f"publication {seq} never landed (flags {np.unique(flags).tolist()[:4]}) and the stream is "
                    "idle: the publishing kernel did not run, or the sequence number was overwritten")
            time.sleep(0)


class HostFlagBuffer:
    """Coherent host memory (pxa_host_alloc) for statistics a kernel publishes to the host: `values`
    (float64 (nvals,)) and one completion flag per value group (`flags`, uint32 (nflags,)).  The device writes
    the values, then the flags (system-scope release); the host polls the flags -- no stream event between the
    statistics and the next kernel, and no event wake-up latency.  Used by the fused RelError fold (2 rows
    values, 2 rows flags: `stats` is the (2, rows) view) and by CG's ||r'||^2 (rows, rows)."""

    def __init__(self, rows, nvals=None, nflags=None):
        self.rows = int(rows)
        nv = 2 * self.rows if nvals is None else int(nvals)
        nf = nv if nflags is None else int(nflags)
        nb = 8 * nv + 4 * nf + 4
        p = ct.c_void_p()
        check(lib.pxa_host_alloc(nb, ct.byref(p)), "pxa_host_alloc")
        self._ptr = p.value
        raw = (ct.c_uint8 * nb).from_address(self._ptr)
        self.values = np.frombuffer(raw, dtype=np.float64, count=nv)
        self.flags = np.frombuffer(raw, dtype=np.uint32, count=nf, offset=8 * nv)
        self.flags[:] = 0
        self.vptr, self.fptr = self._ptr, self._ptr + 8 * nv
        self.seq = 0
        self._free = lib.pxa_host_free

    @property
    def stats(self):
        return self.values.reshape(2, self.rows)

    def landed(self, seq):
        """Whether every flag of publication `seq` is set (no wait)."""
        f = self.flags
        if len(f) == 2:
            return bool(f[0] == seq and f[1] == seq)
        return bool((f == seq).all())

    def next_seq(self):
        """A new publication number, for a kernel about to be launched on the CURRENT stream: that stream is
        remembered with it, so that wait() asks the publishing stream (not whichever stream is current by
        then) whether the publication can still land."""
        self.seq = (self.seq % 0xFFFFFFFE) + 1
        global _RAW_STREAM
        if _RAW_STREAM is None:
            _RAW_STREAM = _raw_stream_fn()
        streams = self.__dict__.setdefault("_streams", {})
        streams[self.seq] = int(_RAW_STREAM() or 0)  # the raw handle: ~10x cheaper than a torch stream object
        if len(streams) > 16:
            streams.pop(next(iter(streams)))
        return self.seq

    def fold(self, parts, per_row):
        """Enqueue pxa_tile_partials_fold into this buffer under a new sequence number; returns it."""
        seq = self.next_seq()
        check(lib.pxa_tile_partials_fold(self.rows, int(per_row), parts.data_ptr(), self.vptr, self.fptr, seq,
                                         stream()), "pxa_tile_partials_fold")
        return seq

    def wait(self, seq, spin_s=1e-3):
        """Poll the flags until every value of publication `seq` has landed (as wait_event).  Raises
        instead of spinning forever when the stream has drained without publishing `seq` (an earlier
        kernel faulted, the publishing kernel never ran, or `seq` was overwritten by a later publication);
        an asynchronous device error surfaces through the stream query."""
        raw = self.__dict__.get("_streams", {}).get(seq)

        def idle():  # only asked once the spin has expired: building the stream object here costs nothing
            torch = _torch()
            if raw is None:  # a sequence number this buffer did not hand out: the current stream is all we know
                return torch.cuda.current_stream().query()
            if raw == 0:
                return torch.cuda.default_stream().query()
            return torch.cuda.ExternalStream(raw).query()

        wait_flags(self.flags, seq, spin_s, idle)

    def __del__(self):
        if getattr(self, "_ptr", None):
            self._free(self._ptr)
            self._ptr = None


def _row_reduce(call, name, x, y, out):
    """Shared body of row_reduce / row_reduce_pow: `call(dtype, rows, n, x, y, out, work, stream)` on every slab of
    at most 65535 rows (the grid-y limit)."""
    x = require(x)
    n = x.shape[-1] if x.ndim > 0 else 1
    rows = int(np.prod(x.shape[:-1])) if x.ndim > 1 else 1  # rows of zero elements reduce to 0 (pxa_row_reduce)
    if y is not None:
        y = require(y, "y", like=x, shape=x.shape)
    if out is None:
        out = empty_f64((max(rows, 1),), x)
    else:
        written(out, "out", dtype="float64", numel=max(rows, 1), apart=(x, y))
    if x.numel() == 0:  # no rows, or rows without elements: the statistic of an empty row is 0
        out.zero_()
        return out.reshape(x.shape[:-1]) if x.ndim > 1 and rows > 0 else out
    es = x.element_size()
    for r0 in range(0, rows, _ROW_SLAB):
        r1 = min(rows, r0 + _ROW_SLAB)
        work = _workspace("pxa_row_reduce_workspace_bytes", x, r1 - r0, n, f64=True)
        check(call(dtcode(x), r1 - r0, n, ptr(x) + r0 * n * es, (ptr(y) + r0 * n * es) if y is not None else None,
                   out.data_ptr() + r0 * 8, ptr(work), stream()), name)
    return out.reshape(x.shape[:-1]) if x.ndim > 1 else out


def row_reduce(op, x, y=None, out=None):
    """Per-row reduction over the last axis -> float64 device tensor of shape x.shape[:-1] (or (1,)).
    `out`: optional contiguous float64 device buffer of max(rows, 1) elements to write into."""
    return _row_reduce(lambda dt, rows, n, *a: lib.pxa_row_reduce(dt, op, rows, n, *a), "pxa_row_reduce", x, y, out)


def row_reduce_pow(p, x, y=None, out=None):
    """Per-row sum |x - y|^p (p > 0) or non-zero count (p == 0) -> float64 device tensor of shape x.shape[:-1]
    (or (1,)).  `out`: as in row_reduce."""
    return _row_reduce(lambda dt, rows, n, *a: lib.pxa_row_reduce_pow(dt, rows, n, float(p), *a), "pxa_row_reduce_pow",
                       x, y, out)


# ------------------------------------------------------------------ row threshold search (csrc/threshold.hip)
SHRINK_CLAMP, SHRINK_SOFT = 0, 1
THRESHOLD_FIRST_BATCH = 8  # count passes enqueued before the first look at the state words
THRESHOLD_MAX_PASSES = 256
_ROW_SLAB = 65535  # grid.y limit


def row_threshold_resident_max(x):
    return int(lib.pxa_row_threshold_resident_max(dtcode(x)))


def _threshold_args(x2, a, b, c):
    x2 = require(x2)
    if x2.ndim != 2:
        raise ValueError(f"pyxu_amd: row threshold expects a (rows, n) array, got shape {tuple(x2.shape)}.")
    a, b, c = float(a), float(b), float(c)
    if not (a > 0 and b >= 0 and c >= 0 and np.isfinite(a + b + c)):
        raise ValueError(f"pyxu_amd: row threshold needs finite a > 0, b >= 0, c >= 0 (got {a}, {b}, {c}).")
    return x2, a, b, c


def _threshold_stream(x2, r0, r1, a, b, c, mu, passes, batch):
    """Streaming search of rows [r0, r1): batches of count passes until every state word is set."""
    torch = _torch()
    rows, n, es = r1 - r0, x2.shape[1], x2.element_size()
    state = torch.empty((rows,), dtype=torch.int32, device=x2.device)
    work = _workspace("pxa_row_threshold_workspace_bytes", x2, rows, n, f64=True)
    batch = THRESHOLD_FIRST_BATCH if batch is None else int(batch)
    if batch < 1:
        raise ValueError(f"pyxu_amd: the threshold search needs batch >= 1, got {batch}.")
    total, first = 0, 1
    while True:
        check(lib.pxa_row_threshold_stream(dtcode(x2), rows, n, ptr(x2) + r0 * n * es, a, b, c, first, batch,
                                           mu.data_ptr() + r0 * 8, state.data_ptr(), passes.data_ptr() + r0 * 4, ptr(work),
                                           stream()), "pxa_row_threshold_stream")
        total, first = total + batch, 0
        if bool(state.cpu().numpy().all()):  # the only host read of a prox
            return
        if total >= THRESHOLD_MAX_PASSES:
            raise RuntimeError("threshold search did not converge")
        batch = min(batch, THRESHOLD_MAX_PASSES - total)


def _threshold_run(x2, a, b, c, mode, out, batch):
    """(mu, passes, out): the search over every slab of rows and, with `out`, the shrink."""
    torch = _torch()
    rows, n = x2.shape
    mu = torch.zeros((rows,), dtype=torch.float64, device=x2.device)
    passes = torch.zeros((rows,), dtype=torch.int32, device=x2.device)
    if rows == 0 or n == 0:
        return mu, passes, out
    es = x2.element_size()
    resident = n <= row_threshold_resident_max(x2)
    for r0 in range(0, rows, _ROW_SLAB):
        r1 = min(rows, r0 + _ROW_SLAB)
        xo, oo = ptr(x2) + r0 * n * es, (ptr(out) + r0 * n * es) if out is not None else None
        if resident:
            check(lib.pxa_row_threshold_prox(dtcode(x2), int(mode), r1 - r0, n, xo, a, b, c, oo, mu.data_ptr() + r0 * 8,
                                             passes.data_ptr() + r0 * 4, stream()), "pxa_row_threshold_prox")
        else:
            _threshold_stream(x2, r0, r1, a, b, c, mu, passes, batch)
            if out is not None:
                check(lib.pxa_row_shrink(dtcode(x2), int(mode), r1 - r0, n, xo, mu.data_ptr() + r0 * 8, oo, stream()),
                      "pxa_row_shrink")
    return mu, passes, out


def row_threshold(x2, a, b, c, batch=None):
    """Per row of x2 (rows, n): the root mu* of a sum max(|x_i| - mu, 0) - b mu - c (0 when a ||x||_1 <= c, NaN for a
    row that holds a NaN or an inf) -> (mu float64 (rows,), passes int32 (rows,)) on the device.  `batch`: count passes
    per enqueued batch of the streaming path (long rows); mu* does not depend on it."""
    x2, a, b, c = _threshold_args(x2, a, b, c)
    mu, passes, _ = _threshold_run(x2, a, b, c, SHRINK_CLAMP, None, batch)
    return mu, passes


def row_shrink(x2, mu, mode, out=None):
    """out[r] = sign(x) min(|x|, mu[r]) (SHRINK_CLAMP) or sign(x) max(|x| - mu[r], 0) (SHRINK_SOFT); mu: float64
    device vector of one threshold per row.  `out` may be x2 itself."""
    x2 = require(x2)
    if x2.ndim != 2:
        raise ValueError(f"pyxu_amd: row_shrink expects a (rows, n) array, got shape {tuple(x2.shape)}.")
    if mode not in (SHRINK_CLAMP, SHRINK_SOFT):
        raise ValueError(f"pyxu_amd: unknown shrink mode {mode!r}.")
    rows, n = x2.shape
    mu = require(mu, "mu", dtype="float64", numel=rows)
    out = _out(out, x2)
    es = x2.element_size()
    for r0 in range(0, rows if n > 0 else 0, _ROW_SLAB):
        r1 = min(rows, r0 + _ROW_SLAB)
        check(lib.pxa_row_shrink(dtcode(x2), int(mode), r1 - r0, n, ptr(x2) + r0 * n * es, mu.data_ptr() + r0 * 8,
                                 ptr(out) + r0 * n * es, stream()), "pxa_row_shrink")
    return out


def row_threshold_prox(x2, a, b, c, mode, out=None, batch=None, info=False):
    """The threshold search and the shrink at its root: rows of up to row_threshold_resident_max elements in one
    launch, longer rows by streaming passes and pxa_row_shrink.  `out` may be x2 itself.  `info`: also return
    (mu, passes)."""
    x2, a, b, c = _threshold_args(x2, a, b, c)
    if mode not in (SHRINK_CLAMP, SHRINK_SOFT):
        raise ValueError(f"pyxu_amd: unknown shrink mode {mode!r}.")
    out = _out(out, x2)
    mu, passes, out = _threshold_run(x2, a, b, c, mode, out, batch)
    return (out, mu, passes) if info else out


# ------------------------------------------------------------------ stencils
_MAX_TAPS = 64  # PXA_MAX_TAPS: per-axis tap slots of pxa_stencil_sep's offsets / coefs


def stencil_axis(x, y, stack, shape, axis, offsets, coefs, zero_partial=False, xs=None, ys=None, beta=0.0, x_off=0, y_off=0):
    """One separable-axis pass (see pxa_stencil_axis).  `x_off`/`y_off`: element offsets into x/y."""
    N = int(np.prod(shape))
    es = x.element_size()
    check(
        lib.pxa_stencil_axis(
            dtcode(x), stack, len(shape), i64_array(shape), axis, len(offsets), i32_array(offsets), f64_array(coefs),
            int(zero_partial), ptr(x) + x_off * es, N if xs is None else xs, ptr(y) + y_off * es, N if ys is None else ys,
            float(beta), stream(),
        ),
        "pxa_stencil_axis",
    )
    return y


def stencil_sep(x, y, stack, shape, taps, beta=0.0, xs=None, ys=None, x_off=0, y_off=0):
    """Separable constant-mode filter; taps[d] = (offsets, coefs) or None (identity axis)."""
    D = len(shape)
    MT = _MAX_TAPS
    ntaps = [0 if t is None else len(t[0]) for t in taps]
    offs = [0] * (D * MT)
    cfs = [0.0] * (D * MT)
    for d, t in enumerate(taps):
        if t is not None:
            for q, (o, c) in enumerate(zip(*t)):
                offs[d * MT + q] = o
                cfs[d * MT + q] = c
    N = int(np.prod(shape))
    work = _workspace("pxa_stencil_sep_workspace_bytes", x, dtcode(x), stack, D, i64_array(shape), int_array(ntaps))
    es = x.element_size()
    check(
        lib.pxa_stencil_sep(
            dtcode(x), stack, D, i64_array(shape), int_array(ntaps), i32_array(offs), f64_array(cfs),
            ptr(x) + x_off * es, N if xs is None else xs, ptr(y) + y_off * es, N if ys is None else ys, float(beta),
            _p(work), stream(),
        ),
        "pxa_stencil_sep",
    )
    return y


def stencil_nd(x, y, stack, shape, offsets_dev, coefs_dev, zero_partial=False, beta=0.0, xs=None, ys=None, x_off=0, y_off=0,
               off_lo=None, off_hi=None):
    """N-D stencil; with the tap offsets' per-axis range (off_lo / off_hi, host ints) pxa_stencil_nd_box, which
    runs the LDS-tiled kernel where it applies."""
    N = int(np.prod(shape))
    ntaps = coefs_dev.numel()
    es = x.element_size()
    if off_lo is not None and off_hi is not None:
        lo, hi = (np.ascontiguousarray(v, dtype=np.int32) for v in (off_lo, off_hi))
        check(
            lib.pxa_stencil_nd_box(
                dtcode(x), stack, len(shape), i64_array(shape), ntaps, ptr(offsets_dev), ptr(coefs_dev),
                lo.ctypes.data, hi.ctypes.data, int(zero_partial), ptr(x) + x_off * es, N if xs is None else xs,
                ptr(y) + y_off * es, N if ys is None else ys, float(beta), stream(),
            ),
            "pxa_stencil_nd_box",
        )
        return y
    check(
        lib.pxa_stencil_nd(
            dtcode(x), stack, len(shape), i64_array(shape), ntaps, ptr(offsets_dev), ptr(coefs_dev), int(zero_partial),
            ptr(x) + x_off * es, N if xs is None else xs, ptr(y) + y_off * es, N if ys is None else ys, float(beta), stream(),
        ),
        "pxa_stencil_nd",
    )
    return y


def pad(x, stack, shape, lo, hi, modes):
    pshape = [n + l + h for n, l, h in zip(shape, lo, hi)]
    y = empty((stack * int(np.prod(pshape)),), x)
    check(
        lib.pxa_pad(dtcode(x), stack, len(shape), i64_array(shape), i64_array(lo), i64_array(hi),
                    int_array([MODES[m] for m in modes]), ptr(x), ptr(y), stream()),
        "pxa_pad",
    )
    return y


def pad_adjoint(x, stack, shape, lo, hi, modes):
    y = empty((stack * int(np.prod(shape)),), x)
    work = empty((x.numel(),), x)
    check(
        lib.pxa_pad_adjoint(dtcode(x), stack, len(shape), i64_array(shape), i64_array(lo), i64_array(hi),
                            int_array([MODES[m] for m in modes]), ptr(x), ptr(y), ptr(work), stream()),
        "pxa_pad_adjoint",
    )
    return y


def trim(x, stack, big_shape, lo, hi, embed):
    core = [n - l - h for n, l, h in zip(big_shape, lo, hi)]
    n_out = int(np.prod(big_shape if embed else core))
    y = empty((stack * n_out,), x)
    check(
        lib.pxa_trim(dtcode(x), stack, len(big_shape), i64_array(big_shape), i64_array(lo), i64_array(hi), int(embed),
                     ptr(x), ptr(y), stream()),
        "pxa_trim",
    )
    return y


def gather_cols(x, idx, out=None):
    """out[r, j] = x[r, idx[j]] for x (rows, n) and device int64 idx (m,)."""
    x = require(x)
    n = x.shape[-1]
    rows = int(np.prod(x.shape[:-1]))
    idx = require(idx, "idx", dtype="int64")
    m = idx.numel()
    out = _out(out, x, (*x.shape[:-1], m), apart=(x,))
    check(lib.pxa_gather_cols(dtcode(x), rows, n, ptr(x), m, ptr(idx), ptr(out), stream()), "pxa_gather_cols")
    return out


def scatter_cols(y, idx, n, out=None):
    """out (rows, n) = 0 then out[r, idx[j]] = y[r, j] (idx unique)."""
    y = require(y)
    m = y.shape[-1]
    rows = int(np.prod(y.shape[:-1]))
    idx = require(idx, "idx", dtype="int64", numel=m)
    out = _out(out, y, (*y.shape[:-1], n), apart=(y,))
    check(lib.pxa_scatter_cols(dtcode(y), rows, m, ptr(y), n, ptr(idx), ptr(out), stream()), "pxa_scatter_cols")
    return out


# ------------------------------------------------------------------ gradient
def gradient2(x, stack, shape, dirs, o0, c0, o1, c1, adjoint=False):
    D = len(dirs)
    N = int(np.prod(shape))
    out = empty((stack * (N if adjoint else D * N),), x)
    fn = lib.pxa_gradient2_adjoint if adjoint else lib.pxa_gradient2
    check(
        fn(dtcode(x), stack, len(shape), i64_array(shape), D, int_array(dirs), int_array(o0), f64_array(c0),
           int_array(o1), f64_array(c1), ptr(x), ptr(out), stream()),
        "pxa_gradient2",
    )
    return out


# ------------------------------------------------------------------ dense
def dense_matmat(A, X, trans):
    """trans=0: Y = X A^T (X: (B, N)); trans=1: Y = X A (X: (B, M))."""
    M, N = A.shape
    B = X.shape[0]
    Y = empty((B, N if trans else M), X)
    work = _workspace("pxa_dense_workspace_bytes", X, dtcode(X), int(trans), M, N, B)
    check(lib.pxa_dense_matmat(dtcode(X), int(trans), M, N, B, ptr(A), ptr(X), ptr(Y), _p(work), stream()),
          "pxa_dense_matmat")
    return Y


def dense_normal_supported(A, x):
    """True when pxa_dense_normal takes (A, x): one fp32 right-hand side, N % 4 == 0, N <= 65536."""
    M, N = A.shape
    B = x.numel() // max(N, 1)
    return (A.dtype == x.dtype and x.shape[-1] == N and B == 1 and A.is_contiguous() and x.is_contiguous()
            and int(lib.pxa_dense_normal_workspace_bytes(dtcode(x), M, N, 1)) > 0)


def dense_normal(A, x, s, d, work=None, pdot=None):
    """Y = s * A^T (A x) + d * x in one pass over A (pxa_dense_normal); `work`: a reusable uint8 device
    buffer of at least pxa_dense_normal_workspace_bytes bytes (allocated when None).  pdot: a float64 device
    buffer that receives the CG's <x, Y> partials in the same launches (pxa_dense_normal_pdot, for
    cg_update(..., have_pap=True) with pdot as its work)."""
    torch = _torch()
    M, N = A.shape
    wsz = int(lib.pxa_dense_normal_workspace_bytes(dtcode(x), M, N, 1))
    if wsz == 0:
        raise ValueError("pxa_dense_normal: unsupported operand (see dense_normal_supported)")
    if work is None or work.numel() < wsz:
        work = torch.empty((wsz,), dtype=torch.uint8, device=x.device)
    Y = empty(x.shape, x)
    if pdot is None:
        check(lib.pxa_dense_normal(dtcode(x), M, N, 1, ptr(A), ptr(x), float(s), float(d), ptr(Y), ptr(work), stream()),
              "pxa_dense_normal")
    else:
        written(pdot, "pdot", dtype="float64")
        check(lib.pxa_dense_normal_pdot(dtcode(x), M, N, ptr(A), ptr(x), float(s), float(d), ptr(Y), ptr(work),
                                        pdot.data_ptr(), stream()), "pxa_dense_normal_pdot")
    return Y


# ------------------------------------------------------------------ fused solver steps
def pgd_tv2d_args(stack, y_images, n0, n1, taps0, taps1, h0, h1, lam, mu, prox, prox_w):
    """Pre-built ctypes arguments of the iteration-invariant part of pxa_pgd_tv2d_step."""
    o0, k0 = taps0
    o1, k1 = taps1
    return (int(stack), int(y_images), int(n0), int(n1), len(o0), i32_array(o0), f64_array(k0), len(o1), i32_array(o1),
            f64_array(k1), float(h0), float(h1), float(lam), float(mu))


def pgd_tv2d_step(x, x_prev, hty, x_new, stack, y_images, n0, n1, taps0, taps1, h0, h1, lam, mu, a, tau, prox, prox_w, partials=None,
                  pre=None, x_ref=None):
    """One fused PGD iteration (pxa_pgd_tv2d_step).  `pre`: pgd_tv2d_args(...) cached by the caller.  With
    `partials`, the per-tile RelError statistics are taken against `x_ref` (None: against x)."""
    if pre is None:
        pre = pgd_tv2d_args(stack, y_images, n0, n1, taps0, taps1, h0, h1, lam, mu, prox, prox_w)
    _launch(lib.pxa_pgd_tv2d_step, dtcode(x), *pre, float(a), float(tau), int(prox), float(prox_w),
            x.data_ptr(), x_prev.data_ptr(), hty.data_ptr(), x_new.data_ptr(), _p(partials), _p(x_ref), stream())
    return x_new


class PgdPlan:
    """pxa_pgd_tv2d_plan: the fused PGD step's iteration-invariant parameters, prepared once per solve, and the
    device counter of its last-workgroup RelError fold.  ``step`` is one iteration (pxa_pgd_tv2d_plan_step) with
    the few per-step arguments, so a PGD step costs one short ctypes call."""

    def __init__(self, like, stack, y_images, n0, n1, taps0, taps1, h0, h1, lam, mu, prox):
        o0, k0 = taps0
        o1, k1 = taps1
        h = ct.c_void_p()
        check(lib.pxa_pgd_tv2d_plan(dtcode(like), int(stack), int(y_images), int(n0), int(n1), len(o0), i32_array(o0),
                                    f64_array(k0), len(o1), i32_array(o1), f64_array(k1), float(h0), float(h1),
                                    float(lam), float(mu), int(prox), ct.byref(h)), "pxa_pgd_tv2d_plan")
        self._h = h.value
        self._free = lib.pxa_pgd_tv2d_plan_free

    def _step(self, fn, x, x_prev, hty, x_new, a, tau, prox_w, *tail):
        """One of the pxa_pgd_tv2d_plan_step* forms: each takes the plan, the three scalars and the four arrays, then
        its own `tail` of partials / publication arguments, then the stream."""
        _launch(fn, self._h, float(a), float(tau), float(prox_w), x.data_ptr(), x_prev.data_ptr(),
                hty.data_ptr(), x_new.data_ptr(), *tail, stream())
        return x_new

    def step(self, x, x_prev, hty, x_new, a, tau, prox_w, partials=None, x_ref=None, sink=None, seq=0,
             fold_launch=False):
        """One iteration; with `sink` (a HostFlagBuffer of (2, rows) values) its partials are also folded there
        under publication `seq`: by the launch's last workgroup, or with `fold_launch` by a fold launch enqueued
        behind it in the same C call (pxa_pgd_tv2d_plan_step_fold)."""
        vp_, fp_ = (None, None) if sink is None else (sink.vptr, sink.fptr)
        fn = lib.pxa_pgd_tv2d_plan_step_fold if fold_launch else lib.pxa_pgd_tv2d_plan_step
        return self._step(fn, x, x_prev, hty, x_new, a, tau, prox_w, _p(partials), _p(x_ref), vp_, fp_, int(seq))

    def step_wpub(self, x, x_prev, hty, x_new, a, tau, prox_w, partials, prev=None):
        """One iteration with window partials into `partials`; `prev` = (partials of the previous such launch,
        HostFlagBuffer, seq): folded and published by an extra workgroup of this launch
        (pxa_pgd_tv2d_plan_step_wpub)."""
        pp, fb, seq = prev if prev is not None else (None, None, 0)
        vp_, fp_ = (None, None) if fb is None else (fb.vptr, fb.fptr)
        return self._step(lib.pxa_pgd_tv2d_plan_step_wpub, x, x_prev, hty, x_new, a, tau, prox_w, partials.data_ptr(),
                          _p(pp), vp_, fp_, int(seq))

    def step_window(self, x, x_prev, hty, x_new, a, tau, prox_w, partials, sink, seq):
        """One iteration whose partials are the RelError statistics of the (x, x_prev) pair it reads -- the stop
        check before it -- folded into `sink` under publication `seq` by a fold launch behind it
        (pxa_pgd_tv2d_plan_step_wfold)."""
        return self._step(lib.pxa_pgd_tv2d_plan_step_wfold, x, x_prev, hty, x_new, a, tau, prox_w, partials.data_ptr(),
                          sink.vptr, sink.fptr, int(seq))

    def __del__(self):
        if getattr(self, "_h", None):
            self._free(self._h)
            self._h = None


_PDS_W = 17  # PXA_PDS_TAP_SLOTS: per-axis tap slots of pxa_pds_step (2 * 8 + 1)


def pds_args(stack, y_images, n0, n1, n2, D, taps, c0, c1, tau, sigma, rho, lam, prox, prox_w, h_kind):
    """Pre-built ctypes arguments of pxa_pds_step (everything but the arrays)."""
    offs, cfs = [], []
    for o, c in taps:
        offs += list(o) + [0] * (_PDS_W - len(o))
        cfs += list(c) + [0.0] * (_PDS_W - len(c))
    return (i64_array([stack, y_images, n0, n1, n2, D]), i32_array([len(t[0]) for t in taps]), i32_array(offs),
            f64_array(cfs), f64_array(list(c0) + list(c1)), f64_array([tau, sigma, rho, lam, prox_w]), int(prox),
            int(h_kind))


def pds_step(algo, pre, x, u, z, hty, x_out, u_out, z_out, work_q, work_w, nseg=0):
    """One fused PD3O (algo 0) / Condat-Vu (algo 1) iteration (pxa_pds_step); `pre` from pds_args."""
    _launch(lib.pxa_pds_step, dtcode(z), int(algo), *pre, _p(x), _p(u), _p(z), _p(hty), _p(x_out),
            _p(u_out), _p(z_out), _p(work_q), _p(work_w), int(nseg), stream())


def pds_step_la(algo, pre, primed, x, u, z, hty, x_out, u_out, z_out, work_q, work_kt, work_w, nseg=0):
    """One look-ahead PD3O / Condat-Vu iteration (pxa_pds_step_la): kernel B + kernel D (dual update fused
    with the next iteration's axis-0 march); `primed` = the previous call left x / work_q / work_kt."""
    _launch(lib.pxa_pds_step_la, dtcode(z), int(algo), *pre, int(bool(primed)), _p(x), _p(u), _p(z),
            _p(hty), _p(x_out), _p(u_out), _p(z_out), _p(work_q), _p(work_kt), _p(work_w), int(nseg), stream())


_SLAB = "the slab geometry"


def _ghost_depth(t, name, like, per_plane):
    """Depth in planes of a ghost buffer whose planes hold `per_plane` elements each (0 for None)."""
    if t is None:
        return 0
    written(t, name, like=like, ctx=_SLAB)  # (read only, but never copied: the exchange fills exactly this buffer)
    d, rem = divmod(t.numel(), per_plane)
    if rem or d < 1:
        raise ValueError(f"pyxu_amd: ghost `{name}` of {t.numel()} elements is not a whole number of planes "
                         f"({per_plane} elements each)")
    return d


def pds_slab_primal(algo, pre, x, u, z, hty, x_out, u_out, work_q, work_w, src_lo=None, src_hi=None, z_lo=None,
                    z_hi=None, nseg=0):
    """Primal part (kernels A and B) of the fused PD3O (algo 0) / Condat-Vu (algo 1) iteration on one rank's slab of
    axis-0 planes (pxa_pds_slab_primal); `pre` from pds_args with n0 = the slab's planes.  Ghost buffers hold the
    neighbours' planes, (stack, depth, n1, n2) for src (u / x) and for Condat-Vu's z_lo (direction 0), (stack, D,
    depth, n1, n2) for PD3O's z; None = the volume's edge.  Writes x_out, u_out (PD3O) and work_w."""
    stack, y_images, n0, n1, n2, D = (int(v) for v in pre[0])
    Mp, N = n1 * n2, n0 * n1 * n2
    # state arrays as they are, inputs too: the kernels read from / write into exactly these buffers
    written(z, "z", numel=stack * D * N, ctx=_SLAB)
    for name, t, numel in (("hty", hty, y_images * N), ("x", x, stack * N), ("u", u, stack * N), ("x_out", x_out, stack * N),
                           ("u_out", u_out, stack * N), ("work_q", work_q, stack * N), ("work_w", work_w, stack * N)):
        if t is not None:
            written(t, name, like=z, numel=numel, ctx=_SLAB)
    zdirs = D if algo == 0 else 1
    depths = [_ghost_depth(src_lo, "src_lo", z, stack * Mp), _ghost_depth(src_hi, "src_hi", z, stack * Mp),
              _ghost_depth(z_lo, "z_lo", z, stack * zdirs * Mp), _ghost_depth(z_hi, "z_hi", z, stack * zdirs * Mp)]
    outs = [t.data_ptr() for t in (x_out, u_out, work_q, work_w) if t is not None]
    for name, t in (("src_lo", src_lo), ("src_hi", src_hi), ("z_lo", z_lo), ("z_hi", z_hi)):
        if t is not None and t.data_ptr() in outs:
            raise ValueError(f"pyxu_amd: ghost `{name}` aliases an output of the step")
    if algo == 1 and x_out is not None and x is not None and x_out.data_ptr() == x.data_ptr():
        raise ValueError("pyxu_amd: Condat-Vu's x_out must not alias x")
    _launch(lib.pxa_pds_slab_primal, dtcode(z), int(algo), *pre, _p(x), _p(u), _p(z), _p(hty), _p(x_out), _p(u_out),
            _p(work_q), _p(work_w), i64_array(depths), _p(src_lo), _p(src_hi), _p(z_lo), _p(z_hi), int(nseg), stream())


def pds_slab_dual(w, z, geom, c0, c1, sigma, lam, rho, h_kind, relax=0, w_hi=None, out=None):
    """Dual part (kernel C) of the slab step, and the ghost-aware form of tv_dual_update (pxa_pds_slab_dual):
    z_out = relax(fenchel_prox_{sigma h}(z + sigma Grad w)) on one rank's slab; w_hi = the first plane(s) of the next
    slab's w as (stack, depth, n1, n2), None at the volume's last slab.  geom = (stack, nl, n1, n2, D)."""
    stack, n0, n1, n2, D = (int(v) for v in geom)
    N = n0 * n1 * n2
    written(z, "z", numel=stack * D * N, ctx=_SLAB)
    written(w, "w", like=z, numel=stack * N, ctx=_SLAB)
    depth = _ghost_depth(w_hi, "w_hi", z, stack * n1 * n2)
    out = _out(out, z, apart=(w, w_hi))
    _launch(lib.pxa_pds_slab_dual, dtcode(z), int(relax), i64_array([stack, n0, n1, n2, D]),
            f64_array(list(c0) + list(c1)), float(sigma), float(lam), float(rho), int(h_kind), ptr(w), _p(w_hi), depth,
            ptr(z), ptr(out), stream())
    return out


def tv_dual_update(w, z, geom, c0, c1, sigma, lam, rho, h_kind, relax=0, out=None):
    """z_out = relax(fenchel_prox_{sigma h}(z + sigma Grad w)), h = lam L1 (h_kind 0) / lam L21 (1):
    the PDS dual update alone (pxa_tv_dual_update).  geom = (stack, n0, n1, n2, D); relax 0 PD3O, 1 CV."""
    w = require(w, "w")
    z = require(z, "z")
    if w.dtype != z.dtype:
        raise TypeError("pyxu_amd: w and z must share a dtype")
    stack, n0, n1, n2, D = (int(v) for v in geom)
    if w.numel() != stack * n0 * n1 * n2 or z.numel() != D * w.numel():
        raise ValueError(f"pyxu_amd: tv_dual_update geometry {tuple(geom)} does not match w {tuple(w.shape)}, "
                         f"z {tuple(z.shape)}")
    out = _out(out, z, apart=(w,))
    check(lib.pxa_tv_dual_update(dtcode(z), int(relax), i64_array([stack, n0, n1, n2, D]),
                                 f64_array(list(c0) + list(c1)), float(sigma), float(lam), float(rho), int(h_kind),
                                 ptr(w), ptr(z), ptr(out), stream()), "pxa_tv_dual_update")
    return out


def pds_kernel_ms(reset=True):
    """(steps, [ms A, ms B, ms C] summed) of the pxa_pds_step calls recorded under TUNE_PDS_EVENTS."""
    buf = (ct.c_double * 3)()
    n = int(lib.pxa_pds_kernel_ms(ct.cast(buf, ct.c_void_p), int(bool(reset))))
    if n < 0:
        check(n, "pxa_pds_kernel_ms")
    return n, [buf[0], buf[1], buf[2]]


# ------------------------------------------------------------------ FFT
def fft(z, shape, axes, stack, inverse, out=None):
    """Unnormalised DFT over `axes` of `stack` complex arrays of `shape`, interleaved (re, im) real
    tensors (pxa_fft).  inverse=False: exp(-2 pi i ..) (fftn, norm="backward"); True: exp(+..)
    (ifftn, norm="forward")."""
    z = require(z, "z")
    out = _out(out, z)  # (may be z)
    sh, ax = i64_array(shape), int_array(axes)
    work = _workspace("pxa_fft_workspace_bytes", z, dtcode(z), len(shape), sh, len(axes), ax, int(stack))
    check(lib.pxa_fft_ex(dtcode(z), len(shape), sh, len(axes), ax, int(stack), int(bool(inverse)), ptr(z), ptr(out),
                         _p(work), stream()), "pxa_fft_ex")
    return out


def real_to_complex(x):
    x = require(x, "x")
    z = empty((*x.shape[:-1], 2 * x.shape[-1]), x)
    check(lib.pxa_real_to_complex(dtcode(x), x.numel(), ptr(x), ptr(z), stream()), "pxa_real_to_complex")
    return z


def complex_real_part(z):
    z = require(z, "z")
    x = empty((*z.shape[:-1], z.shape[-1] // 2), z)
    check(lib.pxa_complex_real_part(dtcode(z), x.numel(), ptr(z), ptr(x), stream()), "pxa_complex_real_part")
    return x


def complex_mul(a, b, conj_b=False, out=None):
    """out = a * b (b broadcast over a's leading stack) for interleaved complex tensors."""
    a, b = require(a, "a"), require(b, "b")
    out = _out(out, a)
    check(lib.pxa_complex_mul(dtcode(a), a.numel() // 2, b.numel() // 2, ptr(a), ptr(b), int(bool(conj_b)), ptr(out),
                              stream()), "pxa_complex_mul")
    return out


# ------------------------------------------------------------------ NUDFT
def nudft_tiles(dtype_code):
    """(tile_n, tile_m, q_chunk) of pxa_nudft: targets per workgroup, sources per LDS tile, stack rows per pass."""
    v = [ct.c_int64(0) for _ in range(3)]
    check(lib.pxa_nudft_tiles(int(dtype_code), *[ct.byref(a) for a in v]), "pxa_nudft_tiles")
    return tuple(int(a.value) for a in v)


def nudft_splits(dtype_code, D, Q, M, N, splits=0):
    """Source splits pxa_nudft runs with for these shapes (`splits` = 0: the library's choice)."""
    wsz = _workspace_bytes("pxa_nudft_workspace_bytes", int(dtype_code), int(D), int(Q), int(M), int(N), int(splits))
    return 1 if wsz == 0 else wsz // (Q * N * 2 * (4 if dtype_code == 0 else 8))


def nudft(src, tgt, isign, w, splits=0, out=None):
    """out[q, n] = sum_m w[q, m] exp(i isign <src_m, tgt_n>) (pxa_nudft): src (M, D), tgt (N, D), w (Q, 2 M) and
    out (Q, 2 N) interleaved complex."""
    src, tgt, w = require(src, "src"), require(tgt, "tgt"), require(w, "w")
    if not (src.dtype == tgt.dtype == w.dtype):
        raise TypeError("pyxu_amd: nudft operands must share one dtype.")
    (M, D), N, Q = src.shape, tgt.shape[0], w.shape[0]
    if tgt.shape[1] != D or w.shape[1] != 2 * M:
        raise ValueError(f"nudft: src {tuple(src.shape)}, tgt {tuple(tgt.shape)}, w {tuple(w.shape)} do not match.")
    out = _out(out, w, (Q, 2 * N), apart=(src, tgt, w))
    dt = dtcode(w)
    work = _workspace("pxa_nudft_workspace_bytes", w, dt, D, Q, M, N, int(splits))
    check(lib.pxa_nudft(dt, D, Q, M, N, ptr(src), ptr(tgt), int(isign), ptr(w), ptr(out), int(splits), _p(work), stream()),
          "pxa_nudft")
    return out


# ------------------------------------------------------------------ gridding NUFFT
def nufft_grid_tiles(dtype_code, D):
    """(bin_shape, q_chunk, batch) of the gridding kernels: fine-grid cells per bin along each of the D axes, stack
    rows per workgroup, candidate points per batch of pxa_nufft_spread.  Needs no GPU."""
    shape = (ct.c_int64 * 3)()
    qc, batch = ct.c_int64(0), ct.c_int64(0)
    check(lib.pxa_nufft_grid_tiles(int(dtype_code), int(D), shape, ct.byref(qc), ct.byref(batch)),
          "pxa_nufft_grid_tiles")
    return tuple(int(v) for v in shape[:int(D)]), int(qc.value), int(batch.value)


def _nufft_plan_check(plan, name):
    torch = _torch()
    l0, off, perm, bin_start = plan
    M, D = off.shape
    if not (l0.dtype == torch.int32 and perm.dtype == torch.int64 and bin_start.dtype == torch.int64):
        raise TypeError(f"{name}: l0 must be int32, perm and bin_start int64.")
    if tuple(l0.shape) != (M, D) or perm.numel() != M or not all(a.is_cuda and a.is_contiguous() for a in plan):
        raise ValueError(f"{name}: plan arrays do not match.")
    return M, D


def _nufft_call(name, args, fac, conj, M, like, out):
    """lib.<name>(*args, stream), or with `fac` (2 M interleaved complex of like's dtype) its `_fac` form, which takes
    the factors and the conjugation flag behind them."""
    if fac is not None:
        fac = require(fac, "fac", like=like, numel=2 * M)
        name, args = name + "_fac", args + [ptr(fac), int(bool(conj))]
    check(getattr(lib, name)(*args, stream()), name)
    return out


def nufft_spread(nf, w, beta, plan, c, out=None, fac=None, conj=False):
    """grid (Q, 2 prod nf) = spread of c (Q, 2 M) with the plan (l0, off, perm, bin_start) (pxa_nufft_spread).  With
    `fac` (2 M interleaved complex, in the plan's sorted order) every point's weights are multiplied by its factor,
    conjugated with `conj` (pxa_nufft_spread_fac)."""
    c = require(c, "c")
    M, D = _nufft_plan_check(plan, "nufft_spread")
    l0, off, perm, bin_start = plan
    Q = c.shape[0]
    if len(nf) != D or c.shape[1] != 2 * M or off.dtype != c.dtype:
        raise ValueError(f"nufft_spread: nf {tuple(nf)}, off {tuple(off.shape)}, c {tuple(c.shape)} do not match.")
    nbins = int(np.prod([-(-int(f) // e) for f, e in zip(nf, nufft_grid_tiles(dtcode(c), D)[0])]))
    if bin_start.numel() != nbins + 1:
        raise ValueError(f"nufft_spread: bin_start has {bin_start.numel()} entries, the grid {nbins} bins.")
    out = _out(out, c, (Q, 2 * int(np.prod(nf))), apart=(c,))
    args = [dtcode(c), D, Q, M, i64_array(nf), int(w), float(beta), ptr(l0), ptr(off), ptr(perm), ptr(bin_start), ptr(c),
            ptr(out)]
    return _nufft_call("pxa_nufft_spread", args, fac, conj, M, c, out)


def nufft_interp(nf, w, beta, plan, grid, out=None, fac=None, conj=False):
    """out (Q, 2 M) = interpolation of grid (Q, 2 prod nf) at the plan's points (pxa_nufft_interp).  With `fac`
    (2 M interleaved complex, in the plan's sorted order) every point's result is multiplied by its factor,
    conjugated with `conj` (pxa_nufft_interp_fac)."""
    grid = require(grid, "grid")
    M, D = _nufft_plan_check(plan, "nufft_interp")
    l0, off, perm, _ = plan
    Q = grid.shape[0]
    if len(nf) != D or grid.shape[1] != 2 * int(np.prod(nf)) or off.dtype != grid.dtype:
        raise ValueError(f"nufft_interp: nf {tuple(nf)}, off {tuple(off.shape)}, grid {tuple(grid.shape)} do not match.")
    out = _out(out, grid, (Q, 2 * M), apart=(grid,))
    args = [dtcode(grid), D, Q, M, i64_array(nf), int(w), float(beta), ptr(l0), ptr(off), ptr(perm), ptr(grid), ptr(out)]
    return _nufft_call("pxa_nufft_interp", args, fac, conj, M, grid, out)


def nufft_deconv(N, nf, modeord, to_grid, corr, z, out=None):
    """to_grid: modes z (Q, 2 prod N) -> fine grid (Q, 2 prod nf), scaled by `corr` and zero-embedded; otherwise the
    fine grid's N central modes, scaled (pxa_nufft_deconv).  `corr`: the concatenated per-axis correction vectors."""
    z, corr = require(z, "z"), require(corr, "corr")
    Q, n_in, n_out = z.shape[0], int(np.prod(N if to_grid else nf)), int(np.prod(nf if to_grid else N))
    if len(N) != len(nf) or z.shape[1] != 2 * n_in or corr.numel() != sum(N) or corr.dtype != z.dtype:
        raise ValueError(f"nufft_deconv: N {tuple(N)}, nf {tuple(nf)}, z {tuple(z.shape)}, corr {tuple(corr.shape)} "
                         "do not match.")
    out = _out(out, z, (Q, 2 * n_out), apart=(z, corr))
    check(lib.pxa_nufft_deconv(dtcode(z), len(N), Q, i64_array(N), i64_array(nf), int(modeord), int(bool(to_grid)),
                               ptr(corr), ptr(z), ptr(out), stream()), "pxa_nufft_deconv")
    return out


# ------------------------------------------------------------------ Toeplitz convolution (NUFFT gram)
def toeplitz_workspace_bytes(dtype_code, Q, n, p):
    """Workspace of pxa_toeplitz_apply in bytes, or None for lengths outside the fused kernel's envelope (a `p`
    that is not {2, 3, 5, 7}-smooth, not LDS-resident or below 2 n - 1).  Needs no GPU."""
    return _workspace_bytes("pxa_toeplitz_workspace_bytes", int(dtype_code), len(n), int(Q), i64_array(n), i64_array(p),
                            unsupported_ok=True)


def toeplitz_apply(n, p, split, khat, z, out=None):
    """out (Q, 2 prod n) = crop(ifft(khat . fft(pad(z)))) on the cells p (pxa_toeplitz_apply): the circular
    convolution with the real spectrum `khat` (prod p values, every scaling folded in); sample i of axis d sits in
    cell i (i < split[d]) or i + p[d] - n[d].  `out` may be `z`."""
    z, khat = require(z, "z"), require(khat, "khat")
    Q, cells = z.shape[0], int(np.prod(n))
    if not (len(n) == len(p) == len(split)) or z.shape[1] != 2 * cells or khat.numel() != int(np.prod(p)) \
            or khat.dtype != z.dtype:
        raise ValueError(f"toeplitz_apply: n {tuple(n)}, p {tuple(p)}, split {tuple(split)}, z {tuple(z.shape)}, khat "
                         f"{tuple(khat.shape)} do not match.")
    out = _out(out, z, apart=(khat,))  # (may be z)
    work = _workspace("pxa_toeplitz_workspace_bytes", z, dtcode(z), len(n), Q, i64_array(n), i64_array(p))
    check(lib.pxa_toeplitz_apply(dtcode(z), len(n), Q, i64_array(n), i64_array(p), i64_array(split), ptr(khat), ptr(z),
                                 ptr(out), _p(work), stream()), "pxa_toeplitz_apply")
    return out


_tuning_from_env()
