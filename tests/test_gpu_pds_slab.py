"""
Slab form of the fused PD3O / Condat-Vu step (pxa_pds_slab_primal + pxa_pds_slab_dual) against pxa_pds_step on the
whole volume, bit for bit.  One process plays every rank: per iteration it cuts the ghost planes out of the
slab-assembled state of the previous iteration, runs the primal part on every slab, cuts the w ghosts, runs the dual
part and assembles.

Bit-equality is derived, not measured: kernel A's segments already give the same bits for any plane range (the ring
position does not enter the arithmetic), kernels B and C evaluate each plane / position by the same expressions, and
a ghost plane holds exactly the values the owner's plane holds.  No tolerance is involved.

Shapes are the smallest at which each piece can go wrong: (17, 9, 11) with axis-0 reach 2 split 6 / 5 / 6 (the interior
slab is 2 R0 + 1 planes, the thinnest legal one); (5, 9, 12) with axis 0 identity but differentiated split 2 / 1 / 2
(the one-plane interior slab has both ghosts and no interior); (11, 37, 70) ragged in-plane tiles with reach 8 on
axis 1 split 6 / 5 (kernel B's boundary-row corrections on slabs).  n2 odd / even selects kernel A's one- / two-position
paths and kernel C's scalar / vector paths ((17, 9, 12), (5, 9, 12) are the even ones).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import _asym_cases as ac  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import f64_array, i32_array, i64_array, lib  # noqa: E402
from pyxu_amd.util import to_device, to_NUMPY  # noqa: E402

ITERS = 3
LAM, G_L1 = 0.05, 0.01
PROX = {"none": 0, "pos": 1, "l1": 2}

# per-axis (raw taps, centre) in the style of _asym_cases: off-centre, signed, different on every axis
AX0_R2 = ([.2, .5, -.1, .2], 2)  # axis-0 reach 2
VOL = [AX0_R2, ([.1, -.2, .3, .4], 3), ([.2, .4, .1, -.2, .1], 1)]
VOL_ID0 = [ac.ID, ([.5, -.2, .1, .3], 0), ([.3, .1, .6], 2)]  # axis 0 identity, still differentiated
RAGGED = [AX0_R2, ([.3, .2, .1, .1, .05, .05, -.1, .05, .05], 0), ([.1, .2, -.3, .4], 2)]  # reach 8 on axis 1


def _taps(axes, dt):
    """[(offsets, coefficients)] per axis, normalised to sum |k| = 1 (as _asym_cases.kernels)."""
    out = []
    for k, c in axes:
        k = np.asarray(k, dtype=np.float64)
        k = (k / np.abs(k).sum()).astype(dt)
        out.append(([i - c for i in range(len(k))], [float(v) for v in k]))
    return out


class Problem:
    def __init__(self, shape, axes, sampling, algo, h_kind, g_kind, dt, stack=1, seed=0):
        self.shape, self.algo, self.dt, self.stack = tuple(shape), algo, dt, stack
        self.taps = _taps(axes, dt)
        self.R0 = max(abs(o) for o in self.taps[0][0])
        self.c0 = [-1.0 / h for h in sampling]
        self.c1 = [1.0 / h for h in sampling]
        Lk = 2 * np.sqrt(sum(1 / h ** 2 for h in sampling))
        self.tau, self.rho = 0.9, 0.95
        self.sigma = 1.0 / (self.tau * Lk ** 2)
        self.h_kind, self.prox = {"l1": 0, "iso": 1}[h_kind], PROX[g_kind]
        rng = np.random.default_rng(seed)
        n0, n1, n2 = self.shape
        self.x = rng.uniform(0, 1, (stack, n0, n1, n2)).astype(dt)
        self.u = (self.x + 0.1 * rng.standard_normal(self.x.shape)).astype(dt)
        self.z = (0.05 * rng.standard_normal((stack, 3, n0, n1, n2))).astype(dt)
        self.hty = rng.standard_normal((1, n0, n1, n2)).astype(dt)  # y_images = 1: shared by the stack

    def pre(self, nl):
        n0, n1, n2 = self.shape
        return _dev.pds_args(self.stack, 1, nl, n1, n2, 3, self.taps, self.c0, self.c1, self.tau, self.sigma, self.rho,
                             LAM, self.prox, self.tau * G_L1, self.h_kind)

    def dual(self, w, z, nl, w_hi=None, out=None):
        n0, n1, n2 = self.shape
        return _dev.pds_slab_dual(w, z, (self.stack, nl, n1, n2, 3), self.c0, self.c1, self.sigma, LAM, self.rho,
                                  self.h_kind, relax=self.algo, w_hi=w_hi, out=out)


def D(a):
    return to_device(np.ascontiguousarray(a))


def whole_volume(pb, iters=ITERS):
    """[(x, u, z)] after each iteration of pxa_pds_step on the whole volume (u is None for Condat-Vu)."""
    n0 = pb.shape[0]
    pre = pb.pre(n0)
    x, u, z, hty = D(pb.x), D(pb.u), D(pb.z), D(pb.hty)
    q, w = torch.empty_like(x), torch.empty_like(x)
    out = []
    for _ in range(iters):
        xo, zo = torch.empty_like(x), torch.empty_like(z)
        if pb.algo == 0:
            uo = torch.empty_like(u)
            _dev.pds_step(0, pre, None, u, z, hty, xo, uo, zo, q, w)
            x, u, z = xo, uo, zo
            out.append((to_NUMPY(x), to_NUMPY(u), to_NUMPY(z)))
        else:
            _dev.pds_step(1, pre, x, None, z, hty, xo, None, zo, q, w)
            x, z = xo, zo
            out.append((to_NUMPY(x), None, to_NUMPY(z)))
    return out


def _cut(a, p0, p1, axis):
    """Contiguous device copy of planes [p0, p1) along `axis` of host array a."""
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(p0, p1)
    return D(a[tuple(sl)])


def slab_iteration(pb, bounds, X, U, Z, zero_ghosts=False):
    """One iteration on the slabs [a, b) of `bounds` from the assembled host state; returns the assembled new state."""
    R2 = 2 * pb.R0
    n0 = pb.shape[0]
    src = U if pb.algo == 0 else X
    xs, us, ws = [], [], []
    for a, b in bounds:
        nl = b - a
        lo, hi = a > 0, b < n0
        gh = dict(src_lo=None, src_hi=None, z_lo=None, z_hi=None)
        if lo:
            if R2:
                gh["src_lo"] = _cut(src, a - R2, a, 1)
            gh["z_lo"] = _cut(Z, a - R2 - 1, a, 2) if pb.algo == 0 else _cut(Z[:, 0], a - 1, a, 1)
        if hi and R2:
            gh["src_hi"] = _cut(src, b, b + R2, 1)
            if pb.algo == 0:
                gh["z_hi"] = _cut(Z, b, b + R2, 2)
        if zero_ghosts:
            for t in gh.values():
                if t is not None:
                    t.zero_()
        x, u, z, hty = _cut(X, a, b, 1), _cut(U, a, b, 1), _cut(Z, a, b, 2), _cut(pb.hty, a, b, 1)
        xo, uo, q, w = (torch.empty_like(x) for _ in range(4))
        if pb.algo == 0:
            _dev.pds_slab_primal(0, pb.pre(nl), None, u, z, hty, xo, uo, q, w, **gh)
        else:
            _dev.pds_slab_primal(1, pb.pre(nl), x, None, z, hty, xo, None, q, w, **gh)
            uo = u
        xs.append(to_NUMPY(xo))
        us.append(to_NUMPY(uo))
        ws.append(to_NUMPY(w))
    Wn = np.concatenate(ws, axis=1)
    zs = []
    for a, b in bounds:
        w_hi = _cut(Wn, b, b + 1, 1) if b < n0 else None
        if w_hi is not None and zero_ghosts:
            w_hi.zero_()
        zs.append(to_NUMPY(pb.dual(_cut(Wn, a, b, 1), _cut(Z, a, b, 2), b - a, w_hi=w_hi)))
    return np.concatenate(xs, axis=1), np.concatenate(us, axis=1), np.concatenate(zs, axis=2)


def check_slabs(pb, bounds):
    ref = whole_volume(pb)
    X, U, Z = pb.x, pb.u, pb.z
    for it in range(ITERS):
        X, U, Z = slab_iteration(pb, bounds, X, U, Z)
        xr, ur, zr = ref[it]
        np.testing.assert_array_equal(X, xr, err_msg=f"x, iteration {it + 1}")
        if pb.algo == 0:
            np.testing.assert_array_equal(U, ur, err_msg=f"u, iteration {it + 1}")
        np.testing.assert_array_equal(Z, zr, err_msg=f"z, iteration {it + 1}")


B17 = [(0, 6), (6, 11), (11, 17)]
B5 = [(0, 2), (2, 3), (3, 5)]
S17, S5 = (1.9, 1.3, 0.7), (1.3, 0.7, 1.9)

# (id, shape, axes, sampling, bounds, algo, h, g, dtype, stack): a covering set, not the cross product
CASES = [
    ("r2-pd3o-iso-pos-f32-odd", (17, 9, 11), VOL, S17, B17, 0, "iso", "pos", np.float32, 1),
    ("r2-pd3o-l1-l1-f64-even", (17, 9, 12), VOL, S17, B17, 0, "l1", "l1", np.float64, 1),
    ("r2-pd3o-l1-none-f32-even", (17, 9, 12), VOL, S17, B17, 0, "l1", "none", np.float32, 1),
    ("r2-cv-iso-l1-f32-odd", (17, 9, 11), VOL, S17, B17, 1, "iso", "l1", np.float32, 1),
    ("r2-cv-l1-pos-f64-odd", (17, 9, 11), VOL, S17, B17, 1, "l1", "pos", np.float64, 1),
    ("r2-cv-iso-none-f32-even", (17, 9, 12), VOL, S17, B17, 1, "iso", "none", np.float32, 1),
    ("r2-pd3o-iso-l1-f32-even-stack2", (17, 9, 12), VOL, S17, B17, 0, "iso", "l1", np.float32, 2),
    ("r0-pd3o-l1-none-f32-even", (5, 9, 12), VOL_ID0, S5, B5, 0, "l1", "none", np.float32, 1),
    ("r0-pd3o-iso-pos-f64-odd", (5, 9, 11), VOL_ID0, S5, B5, 0, "iso", "pos", np.float64, 1),
    ("r0-cv-iso-l1-f32-even", (5, 9, 12), VOL_ID0, S5, B5, 1, "iso", "l1", np.float32, 1),
    ("r0-cv-l1-pos-f32-odd", (5, 9, 11), VOL_ID0, S5, B5, 1, "l1", "pos", np.float32, 1),
    ("r0-cv-l1-none-f64-even-stack2", (5, 9, 12), VOL_ID0, S5, B5, 1, "l1", "none", np.float64, 2),
    ("ragged-pd3o-iso-l1-f32", (11, 37, 70), RAGGED, S17, [(0, 6), (6, 11)], 0, "iso", "l1", np.float32, 1),
    ("ragged-cv-iso-l1-f32", (11, 37, 70), RAGGED, S17, [(0, 6), (6, 11)], 1, "iso", "l1", np.float32, 1),
]


def _problem(case):
    _, shape, axes, samp, bounds, algo, h, g, dt, stack = case
    return Problem(shape, axes, samp, algo, h, g, dt, stack), bounds


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_slab_step_bit_equal_to_whole_volume(case):
    pb, bounds = _problem(case)
    check_slabs(pb, bounds)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[7], CASES[9]], ids=lambda c: c[0])
def test_no_ghosts_is_pds_step(case):
    """Both sides NULL on the whole volume: the bits of pxa_pds_step."""
    pb, _ = _problem(case)
    check_slabs(pb, [(0, pb.shape[0])])


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[7], CASES[9]], ids=lambda c: c[0])
def test_zero_filled_ghosts_change_the_edge_planes(case):
    """Sensitivity of the comparison: with zero-filled ghosts the interior slab's edge planes differ."""
    pb, bounds = _problem(case)
    xr, ur, zr = whole_volume(pb, 1)[0]
    X, U, Z = slab_iteration(pb, bounds, pb.x, pb.u, pb.z, zero_ghosts=True)
    a, b = bounds[1]
    got, ref = (U, ur) if pb.algo == 0 else (X, xr)
    assert not np.array_equal(got[:, a], ref[:, a]), "lo ghosts are not read"
    assert not np.array_equal(Z[:, 0, b - 1], zr[:, 0, b - 1]), "w's hi ghost is not read"
    if pb.R0:
        assert not np.array_equal(got[:, b - 1], ref[:, b - 1]), "hi ghosts are not read"


def _raw_primal(pb, nl, algo, ghost, ptrs, D_=3, n0=None):
    """pxa_pds_slab_primal called raw: (status, outputs untouched)."""
    n0 = nl if n0 is None else n0
    _, n1, n2 = pb.shape
    offs, cfs = [], []
    for o, c in pb.taps:
        offs += list(o) + [0] * (17 - len(o))
        cfs += list(c) + [0.0] * (17 - len(c))
    dtt = torch.float32 if pb.dt == np.float32 else torch.float64
    mk = lambda *sh: torch.full(sh, 7.0, dtype=dtt, device="cuda")  # noqa: E731
    x, u, hty = mk(1, n0, n1, n2), mk(1, n0, n1, n2), mk(1, n0, n1, n2)
    z = mk(1, D_, n0, n1, n2)
    outs = [mk(1, n0, n1, n2) for _ in range(4)]  # x_out, u_out, work_q, work_w
    bufs = [None if d is None else mk(1, 3, max(d, 1), n1, n2) for d in ptrs]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = lib.pxa_pds_slab_primal(0 if pb.dt == np.float32 else 1, algo, i64_array([1, 1, n0, n1, n2, D_]),
                                 i32_array([len(t[0]) for t in pb.taps]), i32_array(offs), f64_array(cfs),
                                 f64_array(pb.c0 + pb.c1), f64_array([pb.tau, pb.sigma, pb.rho, LAM, 0.0]), pb.prox,
                                 pb.h_kind, p(x), p(u), p(z), p(hty), *(p(t) for t in outs), i64_array(ghost),
                                 *(p(t) for t in bufs), 0, _dev.stream())
    torch.cuda.synchronize()
    return st, all(bool((t == 7.0).all()) for t in outs)


def test_argument_errors_launch_nothing():
    pb = Problem((17, 9, 12), VOL, S17, 0, "iso", "pos", np.float32)  # axis-0 reach 2: depths 4 / 5
    ok = ([4, 4, 5, 4], [4, 4, 5, 4])
    bad = {
        "src_lo below 2 R0": ([3, 4, 5, 4], [3, 4, 5, 4]),
        "z_lo below 2 R0 + 1": ([4, 4, 4, 4], [4, 4, 4, 4]),
        "z_hi below 2 R0": ([4, 4, 5, 3], [4, 4, 5, 3]),
        "src_hi below 2 R0": ([4, 2, 5, 4], [4, 2, 5, 4]),
        "z_lo without src_lo": ([0, 4, 5, 4], [None, 4, 5, 4]),
    }
    for why, (ghost, ptrs) in bad.items():
        st, untouched = _raw_primal(pb, 6, 0, ghost, ptrs)
        assert st == -1 and untouched, why
    st, untouched = _raw_primal(pb, 6, 1, [4, 4, 0, 0], [4, 4, None, None])  # Condat-Vu: x ghosts without z_lo
    assert st == -1 and untouched
    # ghosts for the batch-as-axis form (directions (1, 2)): it needs none
    st, untouched = _raw_primal(pb, 6, 0, *ok, D_=2)
    assert st == -1 and untouched
    # n0 = 1 / D = 2 images, with and without ghosts
    for ghost, ptrs in (ok, ([0, 0, 0, 0], [None] * 4)):
        st, untouched = _raw_primal(pb, 1, 0, ghost, ptrs, D_=2)
        assert st == -1 and untouched
    st, untouched = _raw_primal(pb, 6, 0, *ok)  # the valid call of the same helper does launch
    assert st == 0 and not untouched
    # dual part: a zero-depth ghost, ghosts for directions (1, 2), an image
    w, z = D(np.zeros((1, 6, 9, 12), np.float32)), D(np.zeros((1, 3, 6, 9, 12), np.float32))
    wh = D(np.zeros((1, 1, 9, 12), np.float32))
    geo = lambda n0, D_: i64_array([1, n0, 9, 12, D_])  # noqa: E731
    df = f64_array(pb.c0 + pb.c1)
    call = lambda g, whp, dep: lib.pxa_pds_slab_dual(0, 0, g, df, 0.1, LAM, 1.0, 0, w.data_ptr(), whp, dep,  # noqa: E731
                                                     z.data_ptr(), z.data_ptr(), _dev.stream())
    assert call(geo(6, 3), wh.data_ptr(), 0) == -1
    assert call(geo(6, 2), wh.data_ptr(), 1) == -1
    assert call(geo(1, 2), None, 0) == -1
    assert call(geo(6, 3), wh.data_ptr(), 1) == 0
    torch.cuda.synchronize()


def test_ctypes_layer_validates_ghosts():
    pb = Problem((17, 9, 12), VOL, S17, 0, "iso", "pos", np.float32)
    nl = 6
    x = D(np.zeros((1, nl, 9, 12), np.float32))
    z = D(np.zeros((1, 3, nl, 9, 12), np.float32))
    args = lambda **gh: _dev.pds_slab_primal(0, pb.pre(nl), None, x, z, x, torch.empty_like(x), torch.empty_like(x),  # noqa: E731
                                             torch.empty_like(x), torch.empty_like(x), **gh)
    with pytest.raises(ValueError, match="whole number of planes"):
        args(src_lo=D(np.zeros(9 * 12 + 1, np.float32)))
    with pytest.raises(TypeError, match="dtype"):
        args(src_lo=D(np.zeros((1, 4, 9, 12), np.float64)))
    with pytest.raises(ValueError, match="contiguous"):
        args(src_lo=D(np.zeros((1, 4, 9, 24), np.float32))[..., ::2])
    with pytest.raises(ValueError, match="slab geometry"):
        _dev.pds_slab_primal(0, pb.pre(nl + 1), None, x, z, x, torch.empty_like(x), torch.empty_like(x),
                             torch.empty_like(x), torch.empty_like(x))
    out = torch.empty_like(x)
    with pytest.raises(ValueError, match="aliases"):
        _dev.pds_slab_primal(0, pb.pre(nl), None, x, z, x, out, torch.empty_like(x), torch.empty_like(x),
                             torch.empty_like(x), src_lo=out)
    with pytest.raises(RuntimeError, match="pxa_pds_slab_primal"):  # depth below the reach: the C-ABI's error
        args(src_lo=D(np.zeros((1, 3, 9, 12), np.float32)), z_lo=D(np.zeros((1, 3, 5, 9, 12), np.float32)))
