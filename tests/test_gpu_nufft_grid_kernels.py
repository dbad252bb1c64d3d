"""
GPU tests of the gridding kernels (csrc/nufft_grid.hip), each alone against the same stage of the host restatement
(tests/_nufft_grid_refs.py, float64) on the same plan: norm-wise 1e-5 (fp32) / 1e-12 (fp64).

Shapes come from pxa_nufft_grid_tiles: fine grids smaller than one bin, of exactly one, two and three bins per
axis, of 2 w cells, of lengths that are no power of two (28, 250); every point in one bin with more points than a
batch (the other bins empty); M = 0 and M = 1; points whose footprint wraps each axis; w = 2 and w = 16 (fp64);
Q in {1, 3, 5}.  In fp32 w <= 7 (eps >= 1e-6): the kernel value's relative rounding, about beta u, stays near 1e-6.
Every spread runs twice and must give the same bits.  pxa_nufft_deconv: odd and even N, both mode orders, both
directions.
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
        e, q_chunk, batch = _dev.nufft_grid_tiles(code, D)
        few = 67
        add = lambda **kw: out.append(dict(dict(D=D, e=e, M=few, Q=1, pts="uniform"), **kw))  # noqa: E731
        add(nf=tuple(10 for _ in e), w=5, Q=3)  # 2 w cells, smaller than a bin
        add(nf=tuple(v for v in e), w=3 if D == 3 else 7)  # exactly one bin
        add(nf=tuple(2 * v for v in e), w=5, Q=q_chunk + 1, pts="edges")  # two bins per axis: each neighbour once
        add(nf=tuple(3 * v for v in e), w=3, Q=q_chunk - 1)  # three
        add(nf=(28, 250, 14)[:D], w=5, pts="edges")  # no powers of two, ragged last bins
        add(nf=tuple(3 * v for v in e), w=4, M=2 * batch + 3, pts="one_bin")  # more than a batch in one bin
        add(nf=tuple(2 * v + 2 for v in e), w=6, M=0)
        add(nf=tuple(2 * v + 2 for v in e), w=6, M=1, pts="edges")
        if code == 1:
            add(nf=tuple(4 for _ in e), w=2, Q=3)
            add(nf=tuple(max(32, v + 4) for v in e), w=16, Q=q_chunk + 1, pts="edges")
            add(nf=tuple(max(2 * v, 26) for v in e), w=13)
    return out


def _id(c):
    return "D{D}-nf{nf}-w{w}-M{M}-Q{Q}-{pts}".format(**dict(c, nf="x".join(str(v) for v in c["nf"])))


def _points(c, rng):
    """xi (M, D) in fine-grid units, then the coordinates x = 2 pi xi / nf that fold to them."""
    nf, M, D = np.asarray(c["nf"], dtype=np.float64), c["M"], c["D"]
    if c["pts"] == "uniform":
        xi = rng.uniform(0, 1, size=(M, D)) * nf
    elif c["pts"] == "one_bin":  # the middle bin of three per axis
        e = np.asarray(c["e"], dtype=np.float64)
        xi = e + rng.uniform(0, 1, size=(M, D)) * e
    else:  # footprints that wrap either end of every axis, exact cell boundaries included
        xi = rng.uniform(0, 1, size=(M, D)) * nf
        special = np.array([0.0, 0.25, 1.0, -0.25, -1.0, -2.5])
        pick = rng.integers(0, special.size, size=(M, D))
        xi = np.where(rng.uniform(size=(M, D)) < 0.7, np.mod(special[pick], nf), xi)
    return xi * (2 * np.pi / nf)


def _setup(c, dt):
    rng = np.random.default_rng([c["D"], c["w"], c["M"], c["Q"], sum(c["nf"])])
    p = G.plan(_points(c, rng), c["nf"], c["w"], c["e"], dt)
    dev = tuple(to_device(p[k]) for k in ("l0", "off", "perm", "bin_start"))
    return p, dev, rng


CASES = [(w, c) for w, code in (("f32", 0), ("f64", 1)) for c in _cases(code)]
IDS = [f"{w}-{_id(c)}" for w, c in CASES]


def test_case_list_covers_the_edges():
    for code in (0, 1):
        cases = _cases(code)
        assert len({_id(c) for c in cases}) == len(cases)
        assert {c["Q"] for c in cases} >= {1, 3, 5}
        assert {c["M"] for c in cases} >= {0, 1}
        assert all(c["w"] <= 7 for c in cases) or code == 1
        for c in cases:
            assert all(f >= 2 * c["w"] for f in c["nf"])
    assert {c["w"] for c in _cases(1)} >= {2, 16}


@pytest.mark.parametrize("w, c", CASES, ids=IDS)
def test_spread(w, c):
    dt = DT[w]
    p, dev, rng = _setup(c, dt)
    coef = rng.standard_normal((c["Q"], 2 * c["M"])).astype(dt)
    beta = BETA[c["w"]]
    got = _dev.nufft_spread(c["nf"], c["w"], beta, dev, to_device(coef))
    again = _dev.nufft_spread(c["nf"], c["w"], beta, dev, to_device(coef))
    assert torch.equal(got, again)
    ref = G.spread(p, c["nf"], c["w"], beta, as_complex(coef).reshape(c["Q"], c["M"]))
    got = as_complex(to_NUMPY(got)).reshape(ref.shape)
    if c["M"] == 0:
        assert not got.any()
        return
    err = rel_err(got, ref)
    print(f"{w}-{_id(c)} spread: {err:.2e}")
    assert err <= NORMWISE_TOL[np.dtype(dt)]
    assert np.array_equal(got == 0, ref == 0)  # untouched cells are written, as zeros


@pytest.mark.parametrize("w, c", CASES, ids=IDS)
def test_interp(w, c):
    dt = DT[w]
    p, dev, rng = _setup(c, dt)
    nft = int(np.prod(c["nf"]))
    grid = rng.standard_normal((c["Q"], 2 * nft)).astype(dt)
    beta = BETA[c["w"]]
    got = to_NUMPY(_dev.nufft_interp(c["nf"], c["w"], beta, dev, to_device(grid)))
    assert got.shape == (c["Q"], 2 * c["M"]) and got.dtype == dt
    if c["M"] == 0:
        return
    ref = G.interp(p, c["nf"], c["w"], beta, as_complex(grid).reshape(c["Q"], *c["nf"]))
    err = rel_err(as_complex(got), ref)
    print(f"{w}-{_id(c)} interp: {err:.2e}")
    assert err <= NORMWISE_TOL[np.dtype(dt)]


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_spread_and_interp_are_transposes(w):
    dt = DT[w]
    c = dict(D=2, e=_dev.nufft_grid_tiles(0, 2)[0], nf=(28, 40), w=5, M=300, Q=1, pts="edges")
    p, dev, rng = _setup(c, dt)
    a = rng.standard_normal((1, 2 * c["M"])).astype(dt)
    g = rng.standard_normal((1, 2 * 28 * 40)).astype(dt)
    Sa = to_NUMPY(_dev.nufft_spread(c["nf"], 5, BETA[5], dev, to_device(a))).astype(np.float64)
    Stg = to_NUMPY(_dev.nufft_interp(c["nf"], 5, BETA[5], dev, to_device(g))).astype(np.float64)
    # real kernel: the interleaved views are transposes of each other as real matrices
    lhs, rhs = float(np.sum(Sa * g)), float(np.sum(a * Stg))
    assert abs(lhs - rhs) <= NORMWISE_TOL[np.dtype(dt)] * np.linalg.norm(Sa) * np.linalg.norm(g)


DECONV = [dict(N=N, nf=nf, modeord=o, Q=Q)
          for N, nf, Q in (((13,), (28,), 1), ((16,), (32,), 3), ((5, 6), (10, 12), 3), ((6, 5), (20, 20), 1),
                           ((3, 4, 2), (10, 10, 10), 5), ((1, 7, 4), (4, 14, 8), 1), ((250,), (250,), 1))
          for o in (0, 1)]


@pytest.mark.parametrize("w", ["f32", "f64"])
@pytest.mark.parametrize("c", DECONV, ids=[f"N{'x'.join(map(str, c['N']))}-o{c['modeord']}-Q{c['Q']}" for c in DECONV])
def test_deconv(w, c):
    dt = DT[w]
    N, nf, Q, o = c["N"], c["nf"], c["Q"], c["modeord"]
    rng = np.random.default_rng([len(N), sum(N), o])
    corr = rng.uniform(0.5, 2.0, size=sum(N)).astype(dt)
    u = rng.standard_normal((Q, 2 * int(np.prod(N)))).astype(dt)
    g = rng.standard_normal((Q, 2 * int(np.prod(nf)))).astype(dt)
    up = to_NUMPY(_dev.nufft_deconv(N, nf, o, True, to_device(corr), to_device(u)))
    ref = G.deconv_to_grid(N, nf, corr.astype(np.float64), o, as_complex(u).astype(np.complex128).reshape(Q, *N))
    assert rel_err(as_complex(up), ref) <= NORMWISE_TOL[np.dtype(dt)]
    assert np.array_equal(as_complex(up).reshape(ref.shape) == 0, ref == 0)  # exact zeros outside the modes
    down = to_NUMPY(_dev.nufft_deconv(N, nf, o, False, to_device(corr), to_device(g)))
    ref = G.deconv_from_grid(N, nf, corr.astype(np.float64), o, as_complex(g).astype(np.complex128).reshape(Q, *nf))
    assert down.shape == (Q, 2 * int(np.prod(N)))
    assert rel_err(as_complex(down), ref) <= NORMWISE_TOL[np.dtype(dt)]
    # extraction undoes embedding, up to the two scalings
    back = to_NUMPY(_dev.nufft_deconv(N, nf, o, False, to_device(1 / corr), to_device(up)))
    assert rel_err(back, u) <= NORMWISE_TOL[np.dtype(dt)]
    assert as_real(ref).dtype == np.float64
