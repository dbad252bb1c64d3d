"""
GPU tests of the NUDFT entry point alone (pxa_nudft, csrc/nudft.hip), fp32 and fp64, at the edges of its tiling:
targets around one and two workgroup tiles, sources around one and two LDS tiles, stacks below / at / above the
rows of one pass, D = 1, 2, 3, both signs, forced source splits 1, 2, 3, 7 (ragged last split, more splits than
sources) and the library's own choice (tests/_nudft_refs.py::kernel_cases, shapes taken from pxa_nudft_tiles).

Every output element must lie within the derived bound of the float64 sum, |dev - ref64| <= B(u_T) + B(u_64)
(_nudft_refs.bound: valid for any summation order), and the whole result within the FFT tests' norm-wise figures,
1e-5 (fp32) / 1e-12 (fp64): tests/test_nufft_host.py checks that these inputs stay inside the cap that figure
assumes.  The same call gives the same bits twice, and splits = 0 gives the bits of the count it resolves to.
"""
import functools

import numpy as np
import pytest

import _nudft_refs as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

DTYPES = {0: np.float32, 1: np.float64}
CASES = [(code, c) for code in DTYPES for c in R.kernel_cases(*_dev.nudft_tiles(code))]
IDS = [f"{'f32' if code == 0 else 'f64'}-{R.case_id(c)}" for code, c in CASES]


@functools.lru_cache(maxsize=None)
def _reference(i):
    """(src, tgt, w) of case i and its float64 sum with the element-wise limit, computed once."""
    code, c = CASES[i]
    src, tgt, w = R.kernel_inputs(c, DTYPES[code])
    wc = R.as_complex(w)
    ref = R.nudft64(wc, src, tgt, c["isign"])
    lim = R.bound(wc, src, tgt, R.U[np.dtype(DTYPES[code])]) + R.bound(wc, src, tgt, R.U[np.dtype(np.float64)])
    for a in (src, tgt, w, ref, lim):
        a.flags.writeable = False
    return src, tgt, w, ref, lim


def _run(src, tgt, w, isign, splits):
    src, tgt, w = (to_device(np.array(a)) for a in (src, tgt, w))  # uploads of copies: the shared inputs are read-only
    return to_NUMPY(_dev.nudft(src, tgt, isign, w, splits=splits))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_nudft_edges(i):
    code, c = CASES[i]
    dt = DTYPES[code]
    src, tgt, w, ref, lim = _reference(i)
    out = _run(src, tgt, w, c["isign"], c["splits"])
    assert out.shape == (c["Q"], 2 * c["N"]) and out.dtype == dt
    dev = R.as_complex(out)
    ratio = float((np.abs(dev.astype(np.complex128) - ref) / lim).max())
    err = R.rel_err(dev, ref)
    print(f"{IDS[i]}: worst |dev - ref64| / bound {ratio:.3f}, norm-wise {err:.2e}")
    assert ratio <= 1.0
    assert err <= R.NORMWISE_TOL[np.dtype(dt)]
    # the same call, the same bits
    assert np.array_equal(out, _run(src, tgt, w, c["isign"], c["splits"]))
    if c["splits"] == 0:  # ... and the bits of the forced count it resolves to
        s = _dev.nudft_splits(code, c["D"], c["Q"], c["M"], c["N"])
        assert s >= 1
        assert np.array_equal(out, _run(src, tgt, w, c["isign"], s))


def test_auto_split_cases_do_split():
    # the cases meant to exercise the library's choice resolve to more than one split
    multi = [c for code, c in CASES if c["splits"] == 0 and _dev.nudft_splits(code, c["D"], c["Q"], c["M"], c["N"]) > 1]
    assert len(multi) >= 2


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("splits", [0, 1, 3])
def test_no_sources_gives_zero(code, splits):
    dt = DTYPES[code]
    tgt = np.linspace(-3, 3, 2 * 37).reshape(37, 2).astype(dt)
    out = torch.full((3, 2 * 37), 7.0, dtype=torch.float32 if code == 0 else torch.float64, device="cuda")
    src = torch.empty((0, 2), dtype=out.dtype, device="cuda")
    w = torch.empty((3, 0), dtype=out.dtype, device="cuda")
    got = _dev.nudft(src, to_device(tgt), 1, w, splits=splits, out=out)
    assert got is out and not to_NUMPY(out).any()


@pytest.mark.parametrize("code", [0, 1])
def test_no_targets_is_empty(code):
    dt = DTYPES[code]
    src, w = to_device(np.ones((5, 1), dtype=dt)), to_device(np.ones((2, 10), dtype=dt))
    out = _dev.nudft(src, to_device(np.empty((0, 1), dtype=dt)), -1, w)
    assert tuple(out.shape) == (2, 0)


def test_splits_agree_within_the_bound():
    # different split counts reorder the sum: equal within the bound, not bit for bit
    i = IDS.index(next(s for s in IDS if s.startswith("f32") and s.endswith("sp3")))
    src, tgt, w, ref, lim = _reference(i)
    c = CASES[i][1]
    a, b = (R.as_complex(_run(src, tgt, w, c["isign"], s)) for s in (1, 7))
    assert np.all(np.abs(a.astype(np.complex128) - b) <= 2 * lim)
