"""
GPU tests of pxa_nufft_spread_fac / pxa_nufft_interp_fac (csrc/nufft_grid.hip): the spreading and interpolation
kernels with one complex factor per point, each against the same stage of the host restatement
(tests/_nufft_grid_refs.py, float64, on the same plan) applied to factor-multiplied data: norm-wise 1e-5 (fp32) /
1e-12 (fp64).

Shapes: D = 1, 2, 3; Q in {1, 3, 5}; M in {0, 1, batch - 1, batch + 1} (pxa_nufft_grid_tiles); conj_fac 0 and 1;
w in {2, 7}, plus 16 in fp64; fine grids of three bins per axis, the last one ragged, with the points spread over
them and the first point's footprint wrapping every axis.  The factors are given in the plan's sorted order: entry
s belongs to point perm[s].  Every call runs twice and must give the same bits; spread_fac (conj 0) and interp_fac
(conj 1) are conjugate transposes of each other.
"""
import numpy as np
import pytest

import _nufft_grid_refs as G
from _nudft_refs import NORMWISE_TOL, as_complex, as_real, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
BETA = {w: G.kernel_params(10.0 ** -(w - 1))[1] for w in range(2, 17)}  # the shape that goes with each width


def _cases(code):
    out = []
    for D in (1, 2, 3):
        e, _, batch = _dev.nufft_grid_tiles(code, D)
        size = lambda w: tuple(max(2 * v + 2, 2 * w + 2) for v in e)  # noqa: E731
        add = lambda **kw: out.append(dict(D=D, e=e, nf=size(kw["w"]), **kw))  # noqa: E731
        add(M=0, Q=1, w=7, conj=0)
        add(M=1, Q=3, w=2, conj=1)
        add(M=batch - 1, Q=5, w=7, conj=1)
        add(M=batch + 1, Q=1, w=2, conj=0)
        add(M=batch + 1, Q=3, w=7, conj=0)
        if code == 1:
            add(M=batch + 1, Q=3, w=16, conj=1)
            add(M=batch - 1, Q=5, w=16, conj=0)
    return out


def _id(c):
    return "D{D}-nf{nf}-w{w}-M{M}-Q{Q}-c{conj}".format(**dict(c, nf="x".join(str(v) for v in c["nf"])))


def _setup(c, dt):
    """Plan, its device copy, the factors in point order and (device) in sorted order."""
    rng = np.random.default_rng([c["D"], c["w"], c["M"], c["Q"], c["conj"]])
    nf = np.asarray(c["nf"], dtype=np.float64)
    xi = rng.uniform(0, 1, size=(c["M"], c["D"])) * nf
    if c["M"]:
        xi[0] = 0.25  # its footprint starts below zero on every axis
    p = G.plan(xi * (2 * np.pi / nf), c["nf"], c["w"], c["e"], dt)
    if c["M"] > 1:
        assert np.count_nonzero(np.diff(p["bin_start"])) > 1  # points in more than one bin
    dev = tuple(to_device(p[k]) for k in ("l0", "off", "perm", "bin_start"))
    fac = (rng.uniform(0.5, 2.0, size=c["M"]) * np.exp(1j * rng.uniform(-np.pi, np.pi, size=c["M"])))
    fac = fac.astype(np.complex64 if dt == np.float32 else np.complex128)
    fac_sorted = to_device(np.ascontiguousarray(as_real(fac[p["perm"]]).reshape(c["M"], 2)))
    return p, dev, fac, fac_sorted, rng


CASES = [(w, c) for w, code in (("f32", 0), ("f64", 1)) for c in _cases(code)]
IDS = [f"{w}-{_id(c)}" for w, c in CASES]


def test_case_list_covers_the_edges():
    for code in (0, 1):
        cases = _cases(code)
        batch = _dev.nufft_grid_tiles(code, 1)[2]
        assert len({_id(c) for c in cases}) == len(cases)
        for D in (1, 2, 3):
            mine = [c for c in cases if c["D"] == D]
            assert {c["Q"] for c in mine} >= {1, 3, 5} and {c["conj"] for c in mine} == {0, 1}
            assert {c["M"] for c in mine} == {0, 1, batch - 1, batch + 1}
            assert {c["w"] for c in mine} == ({2, 7} if code == 0 else {2, 7, 16})
        for c in cases:
            assert all(f >= 2 * c["w"] for f in c["nf"])
            assert all(-(-f // v) == 3 for f, v in zip(c["nf"], c["e"])) or c["w"] == 16


@pytest.mark.parametrize("w, c", CASES, ids=IDS)
def test_spread_fac(w, c):
    dt = DT[w]
    p, dev, fac, fac_sorted, rng = _setup(c, dt)
    coef = rng.standard_normal((c["Q"], 2 * c["M"])).astype(dt)
    beta = BETA[c["w"]]
    got = _dev.nufft_spread(c["nf"], c["w"], beta, dev, to_device(coef), fac=fac_sorted, conj=bool(c["conj"]))
    again = _dev.nufft_spread(c["nf"], c["w"], beta, dev, to_device(coef), fac=fac_sorted, conj=bool(c["conj"]))
    assert torch.equal(got, again)
    f = np.conj(fac) if c["conj"] else fac
    weighted = as_complex(coef).reshape(c["Q"], c["M"]).astype(np.complex128) * f.astype(np.complex128)
    ref = G.spread(p, c["nf"], c["w"], beta, weighted)
    got = as_complex(to_NUMPY(got)).reshape(ref.shape)
    if c["M"] == 0:
        assert not got.any()
        return
    err = rel_err(got, ref)
    print(f"{w}-{_id(c)} spread_fac: {err:.2e}")
    assert err <= NORMWISE_TOL[np.dtype(dt)]
    assert np.array_equal(got == 0, ref == 0)  # untouched cells are written, as zeros
    # the plain entry point on pre-multiplied data is the same sum
    pre = np.ascontiguousarray(as_real(weighted.astype(fac.dtype)))
    plain = _dev.nufft_spread(c["nf"], c["w"], beta, dev, to_device(pre))
    assert rel_err(got, as_complex(to_NUMPY(plain))) <= NORMWISE_TOL[np.dtype(dt)]


@pytest.mark.parametrize("w, c", CASES, ids=IDS)
def test_interp_fac(w, c):
    dt = DT[w]
    p, dev, fac, fac_sorted, rng = _setup(c, dt)
    nft = int(np.prod(c["nf"]))
    grid = rng.standard_normal((c["Q"], 2 * nft)).astype(dt)
    beta = BETA[c["w"]]
    got = _dev.nufft_interp(c["nf"], c["w"], beta, dev, to_device(grid), fac=fac_sorted, conj=bool(c["conj"]))
    again = _dev.nufft_interp(c["nf"], c["w"], beta, dev, to_device(grid), fac=fac_sorted, conj=bool(c["conj"]))
    assert torch.equal(got, again)
    got = to_NUMPY(got)
    assert got.shape == (c["Q"], 2 * c["M"]) and got.dtype == dt
    if c["M"] == 0:
        return
    f = np.conj(fac) if c["conj"] else fac
    ref = G.interp(p, c["nf"], c["w"], beta, as_complex(grid).reshape(c["Q"], *c["nf"])) * f.astype(np.complex128)
    err = rel_err(as_complex(got), ref)
    print(f"{w}-{_id(c)} interp_fac: {err:.2e}")
    assert err <= NORMWISE_TOL[np.dtype(dt)]


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_spread_fac_and_conjugated_interp_fac_are_transposes(w, D):
    dt = DT[w]
    e, _, batch = _dev.nufft_grid_tiles(0, D)
    c = dict(D=D, e=e, nf=tuple(2 * v + 2 for v in e), w=5, M=batch + 1, Q=1, conj=0)
    p, dev, fac, fac_sorted, rng = _setup(c, dt)
    a = rng.standard_normal((1, 2 * c["M"])).astype(dt)
    g = rng.standard_normal((1, 2 * int(np.prod(c["nf"])))).astype(dt)
    SFa = as_complex(to_NUMPY(_dev.nufft_spread(c["nf"], 5, BETA[5], dev, to_device(a), fac=fac_sorted, conj=False)))
    FSg = as_complex(to_NUMPY(_dev.nufft_interp(c["nf"], 5, BETA[5], dev, to_device(g), fac=fac_sorted, conj=True)))
    lhs = np.vdot(as_complex(g).astype(np.complex128), SFa.astype(np.complex128))
    rhs = np.vdot(FSg.astype(np.complex128), as_complex(a).astype(np.complex128))
    assert abs(lhs - rhs) <= NORMWISE_TOL[np.dtype(dt)] * np.linalg.norm(SFa) * np.linalg.norm(g)


def test_wrappers_check_the_factors():
    e, _, _ = _dev.nufft_grid_tiles(0, 1)
    c = dict(D=1, e=e, nf=(2 * e[0] + 2,), w=5, M=9, Q=1, conj=0)
    p, dev, fac, fac_sorted, rng = _setup(c, np.float32)
    coef = to_device(rng.standard_normal((1, 18)).astype(np.float32))
    with pytest.raises(ValueError, match="fac"):
        _dev.nufft_spread(c["nf"], 5, BETA[5], dev, coef, fac=fac_sorted[:8].contiguous())
    with pytest.raises(ValueError, match="fac"):
        _dev.nufft_spread(c["nf"], 5, BETA[5], dev, coef, fac=fac_sorted.double())
