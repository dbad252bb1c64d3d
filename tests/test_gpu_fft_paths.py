"""
The FFT kernels of pyxu_amd/csrc/fft.hip at every dispatch, grouping and addressing edge, against numpy.fft in
complex128.

The cases (tests/_fft_cases.py) are chosen with the host mirror of the dispatch (tests/_fft_paths.py), and
tests/test_fft_paths_host.py proves on a CPU that they reach the paths named there: every stage list of the
in-LDS power-of-two kernel, its three addressing modes on full, partial, tail and straddling groups, its fast
and generic load / store paths and the four-step transposed store; the ping-pong kernel up to both LDS edges
with every radix; the direct kernel at 2 .. 8 results per thread; four-step and Bluestein, contiguous and strided.

Tolerance: the project's norm-wise 1e-5 (fp32) / 1e-12 (fp64) of tests/test_gpu_fft.py, on the whole output AND
on every transformed line on its own (one wrong group of lines among thousands does not hide in the norm of the
rest).  The reference transforms the input as rounded to the working precision.  Further: unit impulses, whose
transform is a pure twiddle per element (element-wise bound); the fast against the generic addressing path of
the in-LDS kernel, bit for bit; the entry points' corner cases; the helper kernels.
"""
import zlib

import numpy as np
import pytest

import _fft_cases as C
import _fft_paths as P
from _fft_diag import _diagnose

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev, lib  # noqa: E402
from pyxu_amd._lib import i64_array, int_array  # noqa: E402

TOL = {"float32": 1e-5, "float64": 1e-12}
PXA_OK, PXA_ERR_ARG, PXA_ERR_UNSUPPORTED = 0, -1, -3


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _signal(key, stack, sh, dt):
    """complex normal samples, rounded to the working precision (the reference sees what the kernel sees)"""
    rng = np.random.default_rng(_seed(*key))
    x = rng.standard_normal((stack, *sh)) + 1j * rng.standard_normal((stack, *sh))
    return x.astype(np.complex64 if dt == "float32" else np.complex128).astype(np.complex128)


def _view(c, dt):
    """complex (stack, *shape) -> interleaved real (stack, 2 N)"""
    return np.stack([c.real, c.imag], axis=-1).reshape(c.shape[0], -1).astype(dt)


def _cplx(r, stack, sh):
    r = np.asarray(r, dtype=np.float64).reshape(stack, *sh, 2)
    return r[..., 0] + 1j * r[..., 1]


def _up(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _fft(z, sh, axes, stack, inverse, out=None):
    return _dev.fft(z, sh, axes, stack, inverse, out=out).cpu().numpy()


def _ref(x, axes, inverse):
    ax = [a + 1 for a in axes]
    return np.fft.ifftn(x, axes=ax, norm="forward") if inverse else np.fft.fftn(x, axes=ax, norm="backward")


def _line_errors(got, want, axes):
    """norm-wise relative error of every transformed line (sub-array over `axes`), vectorised"""
    ax = tuple(a + 1 for a in axes)
    num = np.sqrt(np.sum(np.abs(got - want) ** 2, axis=ax))
    den = np.sqrt(np.sum(np.abs(want) ** 2, axis=ax))
    return num / np.where(den > 0, den, 1.0)


def _check(got_r, want_c, sh, axes, stack, dt, rerun, what):
    got = _cplx(got_r, stack, sh)
    whole = float(np.linalg.norm(got - want_c) / np.linalg.norm(want_c))
    per = _line_errors(got, want_c, axes)
    worst = float(per.max())
    print(f"{what}: whole {whole:.3e}, worst line {worst:.3e} (line {int(per.argmax())} of {per.size})")
    if not (whole <= TOL[dt] and worst <= TOL[dt]):
        bad = np.flatnonzero(per.ravel() > TOL[dt])
        pytest.fail(f"{what}: rel err whole {whole:.3e}, worst line {worst:.3e} > {TOL[dt]:.0e}; "
                    f"{bad.size} of {per.size} lines over, first {bad[:16].tolist()} (flat index over the "
                    f"untransformed axes of (stack, *shape))\n" + _diagnose(got_r, _view(want_c, dt), sh, rerun))


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_fft_path_vs_numpy(case):
    _, dt, sh, axes, stack = case
    x = _signal(case, stack, sh, dt)
    z = _up(_view(x, dt))
    for inverse in (False, True):
        run = lambda: _fft(z, sh, axes, stack, inverse)  # noqa: E731
        _check(run(), _ref(x, axes, inverse), sh, axes, stack, dt, run, f"{C.case_id(case)} inverse={inverse}")


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("fam", sorted(C.IMPULSE))
def test_fft_unit_impulses(fam, dt):
    """x = delta_j, j = 1 and n - 1: X[k] = exp(-+2 pi i j k / n), modulus 1, so the element-wise error is the
    error of one twiddle chain at one output index (phase reduced in integers: the reference is exact to fp64)."""
    n = C.IMPULSE[fam]
    js = np.array([1, n - 1])
    x = np.zeros((2, n), dtype=np.complex128)
    x[np.arange(2), js] = 1.0
    z = _up(_view(x, dt))
    phase = (js[:, None].astype(np.int64) * np.arange(n, dtype=np.int64)[None, :]) % n
    for inverse in (False, True):
        want = np.exp((2j if inverse else -2j) * np.pi * phase / n)
        got = _cplx(_fft(z, (n,), (0,), 2, inverse), 2, (n,))
        err = np.abs(got - want)
        print(f"impulse {fam} n={n} {dt} inverse={inverse}: max element error {err.max():.3e}")
        assert err.max() <= TOL[dt], (inverse, np.unravel_index(err.argmax(), err.shape), float(err.max()))


@pytest.mark.parametrize("case", C.FAST_CASES, ids=C.case_id)
def test_fft_fast_path_equals_generic_bitwise(case):
    """The raw-buffer fast path and the generic 64-bit path of fft_lds_kernel (PXA_TUNE_FFT_KERNEL bit 1024 takes
    every group off the former) do the same arithmetic on the same lines: any differing bit is an addressing or
    store bug -- the deterministic form of the fp64 low-dword corruption the fast store once had (fft.hip, at the
    16-byte buffer stores).  Each mode runs once."""
    _, dt, sh, axes, stack = case
    x = _signal(("bits", *case), stack, sh, dt)
    z = _up(_view(x, dt))
    out = {}
    old = _dev.tuning(_dev.TUNE_FFT_KERNEL, 0)
    try:
        for mode in (0, 1024):
            _dev.tuning(_dev.TUNE_FFT_KERNEL, mode)
            out[mode] = [_fft(z, sh, axes, stack, inverse) for inverse in (False, True)]
    finally:
        _dev.tuning(_dev.TUNE_FFT_KERNEL, old)
    for inverse in (False, True):
        a, b = out[0][inverse], out[1024][inverse]
        if not np.array_equal(a, b):
            diff = np.flatnonzero(a.ravel() != b.ravel())
            pytest.fail(f"inverse={inverse}: {diff.size} of {a.size} values differ between the fast and the generic "
                        f"path, first flat indices {diff[:16].tolist()}: fast {a.ravel()[diff[:8]].tolist()} "
                        f"generic {b.ravel()[diff[:8]].tolist()}")


# ------------------------------------------------------------------ entry points
@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("sh,axes", [((3, 96, 210), (1, 2)), ((12000, 3), (0,)), ((2053, 3), (0,)), ((4096, 48), (0,))],
                         ids=lambda v: "x".join(map(str, v)))
def test_fft_in_place_equals_out_of_place(sh, axes, dt):
    stack = 2
    x = _signal(("inplace", sh, dt), stack, sh, dt)
    for inverse in (False, True):
        z = _up(_view(x, dt))
        want = _fft(z, sh, axes, stack, inverse)
        assert np.array_equal(z.cpu().numpy(), _view(x, dt))  # the input of an out-of-place call is left alone
        got = _dev.fft(z, sh, axes, stack, inverse, out=z)
        assert got.data_ptr() == z.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want), inverse


@pytest.mark.parametrize("dt", C.DTYPES)
def test_fft_entry_corner_cases(dt):
    code = 0 if dt == "float32" else 1
    sh, stack = (5, 3, 4), 2
    x = _signal(("entry", dt), stack, sh, dt)
    z = _up(_view(x, dt))
    # no axes: a copy
    y = _dev.fft(z, sh, (), stack, False)
    assert y.data_ptr() != z.data_ptr() and torch.equal(y, z)
    # an unsorted axis list reaches the C ABI as given
    got = _cplx(_fft(z, sh, (2, 0), stack, False), stack, sh)
    want = np.fft.fftn(x, axes=(3, 1))
    assert np.linalg.norm(got - want) / np.linalg.norm(want) <= TOL[dt]
    assert _line_errors(got, want, (2, 0)).max() <= TOL[dt]
    # stack = 0: nothing to do, nothing touched
    out = torch.full_like(z, 7.0)
    shp, ax = i64_array(sh), int_array((2, 0))
    assert lib.pxa_fft_ex(code, 3, shp, 2, ax, 0, 0, _dev.ptr(z), _dev.ptr(out), None, _dev.stream()) == PXA_OK
    assert lib.pxa_fft(code, 3, shp, 2, ax, 0, 0, None, None, _dev.stream()) == PXA_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(z, _up(_view(x, dt)))
    # a duplicate axis, an axis >= ndim: argument errors, nothing launched
    for bad in ((0, 0), (1, 3), (-1,)):
        assert lib.pxa_fft_ex(code, 3, shp, len(bad), int_array(bad), stack, 0, _dev.ptr(z), _dev.ptr(out), None,
                              _dev.stream()) == PXA_ERR_ARG, bad
        assert lib.pxa_fft_workspace_bytes(code, 3, shp, len(bad), int_array(bad), stack) == (1 << 64) - 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("dt", C.DTYPES)
def test_pxa_fft_refuses_lengths_that_need_a_workspace(dt):
    code = 0 if dt == "float32" else 1
    ax = int_array((0,))
    for n, want in ((12000, PXA_ERR_UNSUPPORTED), (2053, PXA_ERR_UNSUPPORTED), (2048, PXA_OK)):
        z = _up(_view(_signal(("nowork", n), 1, (n,), dt), dt))
        out = torch.empty_like(z)
        need = lib.pxa_fft_workspace_bytes(code, 1, i64_array((n,)), 1, ax, 1)
        assert need == P.workspace_bytes((n,), (0,), 1, dt) and (need == 0) == (want == PXA_OK)
        assert lib.pxa_fft(code, 1, i64_array((n,)), 1, ax, 1, 0, _dev.ptr(z), _dev.ptr(out), _dev.stream()) == want, n
        torch.cuda.synchronize()


# ------------------------------------------------------------------ helper kernels
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("conj_b", [False, True])
def test_complex_mul_broadcast(dt, conj_b):
    """out[i] = a[i] * b[i % nb] with nb = 37 against 5 x 37 (nb divides neither the block nor the grid), b
    conjugated or not, out-of-place and onto a.  Bound per component: 4 eps |a| |b| (two products and a sum, each
    rounded once: 2 u (|ar br| + |ai bi|) <= eps |a| |b| for the kernel, the same again for a reference in the
    working precision; this reference is extended precision, so the bound has room)."""
    rng = np.random.default_rng(_seed("cmul", dt, conj_b))
    a = rng.standard_normal((5, 37, 2)).astype(dt)
    b = rng.standard_normal((37, 2)).astype(dt)
    ar, ai, br, bi = _ld(a[..., 0]), _ld(a[..., 1]), _ld(b[..., 0])[None], _ld(b[..., 1])[None]
    if conj_b:
        bi = -bi
    want = np.stack([ar * br - ai * bi, ar * bi + ai * br], axis=-1)
    bound = 4 * np.finfo(dt).eps * (np.hypot(ar, ai) * np.hypot(br, bi))[..., None]
    ta, tb = _up(a.reshape(5, 74)), _up(b.reshape(74))
    got = _dev.complex_mul(ta, tb, conj_b=conj_b)
    assert np.array_equal(ta.cpu().numpy(), a.reshape(5, 74))
    err = np.abs(_ld(got.cpu().numpy().reshape(5, 37, 2)) - want)
    assert np.all(err <= bound), float((err / bound).max())
    same = _dev.complex_mul(ta, tb, conj_b=conj_b, out=ta)  # out is a
    assert same.data_ptr() == ta.data_ptr() and torch.equal(same, got)


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("n", [1, 257, 2 ** 20 + 3])
def test_real_complex_copies_exact(n, dt):
    rng = np.random.default_rng(_seed("copies", n))
    x = rng.standard_normal((1, n)).astype(dt)
    z = _dev.real_to_complex(_up(x)).cpu().numpy()
    assert z.shape == (1, 2 * n) and z.dtype == x.dtype
    assert np.array_equal(z[:, 0::2], x) and not z[:, 1::2].any()
    c = rng.standard_normal((1, 2 * n)).astype(dt)
    r = _dev.complex_real_part(_up(c)).cpu().numpy()
    assert r.shape == (1, n) and np.array_equal(r, c[:, 0::2])
