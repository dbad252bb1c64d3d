"""Failure report shared by the FFT GPU tests (tests/test_gpu_fft.py, tests/test_gpu_fft_paths.py)."""
import os

import numpy as np


def _diagnose(got, want, sh, rerun):
    """Failure report: where the wrong elements are (flat index -> (stack, *arg_shape) coordinates of the
    complex element), how wrong (relative to the array's rms, and in ulps of T), and whether the same call,
    run again, gives the same bits.  Written to the assertion message and, with PXA_FAIL_DIR set, to an .npz
    (round-4 verdict: a one-off 4e-10 fp64 failure was lost for want of this)."""
    got = np.asarray(got)
    want = np.asarray(want, dtype=got.dtype)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rms = float(np.sqrt(np.mean(want.astype(np.float64) ** 2))) or 1.0
    tol = 64 * np.finfo(got.dtype).eps * rms
    bad = np.flatnonzero(err.ravel() > tol)
    again = np.asarray(rerun())
    lines = [f"{bad.size} of {err.size} elements off by > 64 eps rms; max {err.max() / rms:.3e} rms",
             f"rerun bit-identical to the failing call: {np.array_equal(again, got)}; "
             f"rerun rel err {np.linalg.norm(again - want) / np.linalg.norm(want):.3e}"]
    if bad.size:
        cplx = got.shape[-1] != int(np.prod(sh))  # interleaved (re, im) view
        el = bad // 2 if cplx else bad
        coords = np.stack(np.unravel_index(el, (got.shape[0], *sh)), axis=1)
        for ax in range(coords.shape[1]):
            u = np.unique(coords[:, ax])
            lines.append(f"axis {ax - 1 if ax else 'stack'}: {u.size} distinct values, first {u[:8].tolist()}")
        lines.append(f"first bad flat indices {bad[:16].tolist()}")
        fg, fw = got.ravel()[bad[:16]], want.ravel()[bad[:16]]
        lines.append(f"got {fg.tolist()} want {fw.tolist()}")
        if got.dtype == np.float64:
            xor = fg.view(np.uint64) ^ fw.view(np.uint64)
            lines.append("xor bits " + " ".join(f"{int(v):016x}" for v in xor))
    out = os.environ.get("PXA_FAIL_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        keep = bad[:4096]  # the wrong elements only (a whole 2048^2 pair would not travel back)
        np.savez(os.path.join(out, f"fft_fail_{'x'.join(map(str, sh))}_{got.dtype}.npz"), bad=keep,
                 got=got.ravel()[keep], want=want.ravel()[keep], again=again.ravel()[keep])
    return "\n".join(lines)
