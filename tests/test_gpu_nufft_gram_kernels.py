"""
pxa_toeplitz_apply alone (no NUFFT): the pruned, fused-axis circular convolution against the float64 restatement
tests/_nufft_gram_refs.py::toeplitz_apply64 with a random real spectrum.  Both precisions, D = 1, 2, 3, unit / two /
odd / even lengths, both cell maps, a P with every radix (105 -> 210 = 2 3 5 7), a power-of-two P, a P above the least
one, line counts that do not fill the last workgroup, stacks of 1 / 3 / 5, `out` aliasing `in`, bit-for-bit repeats,
and the refusals, read from the return value.  Tolerance: norm-wise 1e-5 (fp32) / 1e-12 (fp64), the FFT tests' own:
the chain is two transforms of the same lengths.
"""
import numpy as np
import pytest

import _nudft_refs as R
import _nufft_gram_refs as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import i64_array, lib  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

TOL = {np.float32: 1e-5, np.float64: 1e-12}

# (n, P or None for the least one, Q).  Lines per workgroup are min(16, 4096 / P (fp32) or 2048 / P (fp64), inner):
# the line counts below leave the last workgroup short in every pass.
CASES = [
    ((1,), None, 1), ((2,), None, 3), ((7,), None, 5), ((8,), None, 1), ((105,), None, 3), ((64,), None, 5),
    ((33,), (128,), 3),  # a power of two above 2 n - 1 = 65
    ((300,), None, 5),  # P = 600: 6 (fp32) / 3 (fp64) lines per workgroup, 5 lines
    ((5, 6), None, 3), ((1, 4), None, 1), ((6, 1), None, 5), ((12, 11), None, 3), ((9, 105), None, 1),
    ((7, 8), (16, 20), 5),
    ((3, 4, 2), None, 3), ((2, 1, 3), None, 5), ((4, 3, 5), (8, 6, 12), 1),
    ((13, 12, 105), None, 1),  # the largest shape: P = (28, 24, 210)
]


def _case_id(c):
    n, P, Q = c
    return "n" + "x".join(map(str, n)) + ("" if P is None else "-P" + "x".join(map(str, P))) + f"-Q{Q}"


def _inputs(n, P, Q, dtype):
    rng = np.random.default_rng([Q, *n])
    u = rng.standard_normal((Q, 2 * int(np.prod(n)))).astype(dtype)
    khat = rng.standard_normal(P).astype(dtype)
    return u, khat


def _reference(u, khat, n, P, split):
    Q = u.shape[0]
    ref = T.toeplitz_apply64(R.as_complex(u.astype(np.float64)).reshape(Q, *n), n, P, split,
                             khat.astype(np.float64))
    return R.as_real(np.ascontiguousarray(ref.reshape(Q, -1)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("modeord", [0, 1], ids=["contig", "fftord"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_toeplitz_apply_matches_float64(case, modeord, dtype):
    n, P, Q = case
    P0, split = T.sizes(n, modeord)
    P = P0 if P is None else P
    u, khat = _inputs(n, P, Q, dtype)
    ref = _reference(u, khat, n, P, split)
    ud, kd = to_device(u), to_device(khat.ravel())
    out = _dev.toeplitz_apply(n, P, split, kd, ud)
    got = to_NUMPY(out)
    err = np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref)
    print(f"{_case_id(case)} modeord={modeord} {np.dtype(dtype).name}: rel err {err:.2e}")
    assert err <= TOL[dtype]
    assert np.array_equal(to_NUMPY(ud), u)  # the input is left alone
    again = _dev.toeplitz_apply(n, P, split, kd, ud)
    assert np.array_equal(to_NUMPY(again), got)  # no atomics: the same bits
    _dev.toeplitz_apply(n, P, split, kd, ud, out=ud)  # out aliasing in
    assert np.array_equal(to_NUMPY(ud), got)


def test_unsupported_lengths_are_refused_from_the_return_value():
    z = to_device(np.zeros((1, 10), dtype=np.float32))

    def call(code, n, p, split):
        return lib.pxa_toeplitz_apply(code, len(n), 1, i64_array(n), i64_array(p), i64_array(split), _dev.ptr(z),
                                      _dev.ptr(z), _dev.ptr(z), None, _dev.stream())

    assert call(0, (5,), (11,), (5,)) == -3  # not {2, 3, 5, 7}-smooth
    assert call(0, (5,), (26,), (5,)) == -3
    assert call(0, (5,), (8,), (5,)) == -3  # below 2 n - 1
    assert call(1, (2600,), (5250,), (2600,)) == -3  # smooth, beyond the fp64 LDS line
    assert call(0, (5200,), (10500,), (5200,)) == -3  # beyond the fp32 LDS line
    assert _dev.toeplitz_workspace_bytes(0, 1, (5,), (11,)) is None
    with pytest.raises(RuntimeError):
        _dev.toeplitz_apply((5,), (11,), (5,), to_device(np.zeros(11, dtype=np.float32)), z)
    torch.cuda.synchronize()
    assert np.array_equal(to_NUMPY(z), np.zeros((1, 10), dtype=np.float32))
