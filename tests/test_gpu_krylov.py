"""
The Krylov re-orthogonalisation kernels (csrc/krylov.hip: pxa_krylov_dots / pxa_krylov_update / pxa_krylov_normalize)
against extended-precision NumPy (numpy.longdouble, so that the reference's own error is negligible for both
precisions), at the edges of the column chunk, of the 16-byte vector path and of the striding grid.

Bounds, with u = 2^-53 and T the runtime type:

* dots: every product of two T values is formed in double (exact for float32 inputs, one rounding inside the fma for
  float64) and the n products are summed in double in some fixed order, so to first order
  |got - ref| <= (n + 4) u sum_m |V_im w_m| (|scale| times that with a scale: its multiplication is one more rounding,
  inside the slack of 4).
* update: w_out_m = round_T(w_m - sum_i c_i V_im) with the coefficients in double and one double fma per row, so the
  double value is off by at most (j + 1) u (|w_m| + sum_i |c_i V_im|) and the rounding to T adds u_T |ref_m|
  (u_T = 2^-24 for float32, 2^-53 for float64).
* c_next and nrm2 are dots of V with the stored w_out, so they are held to the dots bound with the w_out that the
  kernel returned as the reference's input.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import lib  # noqa: E402

DTS = [np.float32, np.float64]
IDS = ["f32", "f64"]
U = 2.0**-53
LD = np.longdouble
MAX_GRID = 2048  # workgroups of one launch: more chunks than this makes a workgroup stride


def _chunk(dt):
    return int(lib.pxa_krylov_chunk(0 if dt == np.float32 else 1))


def _sizes(dt):
    c = _chunk(dt)
    return [1, 3, 255, 257, c - 1, c, c + 1, 3 * c + 5]


def _dev_view(a, ld=None, off=0):
    """Device copy of the 2-D (or 1-D) host array `a` with row stride ld, starting `off` elements into its buffer."""
    a2 = np.atleast_2d(a)
    rows, n = a2.shape
    ld = n if ld is None else ld
    host = np.zeros(off + rows * ld + 3, dtype=a.dtype)
    host[off:off + rows * ld].reshape(rows, ld)[:, :n] = a2
    buf = torch.from_numpy(host).cuda()
    v = buf[off:off + rows * ld].view(rows, ld)[:, :n]
    return v if a.ndim == 2 else v[0]


def _case(dt, j, n, key=0):
    rng = np.random.default_rng(1000 * key + 7 * j + n % 9973)
    V = rng.standard_normal((j, n)).astype(dt)
    w = rng.standard_normal(n).astype(dt)
    c = rng.standard_normal(j) / np.sqrt(j)
    return V, w, c


def _f64(k):
    return torch.full((max(k, 1),), 123.0, dtype=torch.float64, device="cuda")


def _dots_bound(V, w, scale=1.0):
    n = V.shape[1]
    return (n + 4) * U * abs(scale) * (np.abs(V).astype(LD) @ np.abs(w).astype(LD)).astype(np.float64)


def _check_dots(dt, V, w, Vd, wd, scale=None):
    j, n = V.shape
    work = _dev.krylov_workspace(j, n, wd)
    out = _f64(j + 1)
    sd = None if scale is None else torch.tensor([scale], dtype=torch.float64, device="cuda")
    _dev.krylov_dots(Vd, j, wd, out, work, scale=sd)
    got = out.cpu().numpy()
    s = 1.0 if scale is None else scale
    ref = (V.astype(LD) @ w.astype(LD)) * LD(s)
    err = np.abs(got[:j] - ref).astype(np.float64)
    bound = _dots_bound(V, w, s)
    print(f"dots {np.dtype(dt).name} j={j} n={n}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    assert got[j] == 123.0  # nothing written past c[j - 1]
    return got[:j]


def _check_update(dt, V, w, c, Vd, wd, alias=False, want_c=True, want_n=True):
    j, n = V.shape
    work = _dev.krylov_workspace(j, n, wd)
    cd = torch.from_numpy(c).cuda()
    outd = wd if alias else torch.full((n + 8,), 77.0, dtype=wd.dtype, device="cuda")[4:n + 4]  # 16-byte aligned
    cn, nr = (_f64(j + 1) if want_c else None), (_f64(2) if want_n else None)
    _dev.krylov_update(Vd, j, wd, cd, outd, work, c_next=cn, nrm2_out=nr)
    got = outd.cpu().numpy()
    ref = w.astype(LD) - c.astype(LD) @ V.astype(LD)
    u_t = 2.0**-24 if dt == np.float32 else U
    bound = ((j + 1) * U * (np.abs(w).astype(LD) + np.abs(c).astype(LD) @ np.abs(V).astype(LD)) + u_t * np.abs(ref)).astype(np.float64)
    err = np.abs(got - ref).astype(np.float64)
    print(f"update {np.dtype(dt).name} j={j} n={n}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    if not alias:
        np.testing.assert_array_equal(wd.cpu().numpy(), w)  # the input row is left alone
        assert float(outd._base[3]) == 77.0 and float(outd._base[n + 4]) == 77.0  # nothing written around w_out
    if want_c:
        cg = cn.cpu().numpy()
        assert np.all(np.abs(cg[:j] - V.astype(LD) @ got.astype(LD)).astype(np.float64) <= _dots_bound(V, got))
        assert cg[j] == 123.0
    if want_n:
        ng = nr.cpu().numpy()
        assert abs(float(ng[0] - got.astype(LD) @ got.astype(LD))) <= (n + 4) * U * float(got.astype(LD) @ got.astype(LD))
        assert ng[1] == 123.0
    return got


SMALL = [(di, n_i, j) for di in range(2) for n_i in range(8) for j in (1, 2, 17, 64)]


@pytest.mark.parametrize("di,n_i,j", SMALL, ids=[f"{IDS[d]}-n{n}-j{j}" for d, n, j in SMALL])
def test_dots_and_update_sizes(di, n_i, j):
    dt = DTS[di]
    n = _sizes(dt)[n_i]
    V, w, c = _case(dt, j, n)
    # rows n apart take the scalar kernels unless n is a whole number of 16-byte vectors; rows a whole number of
    # vectors apart take the vector kernels, with their element-wise tail when n is not
    for ld in sorted({n, -(-n // 4) * 4}):
        Vd, wd = _dev_view(V, ld=ld), _dev_view(w)
        _check_dots(dt, V, w, Vd, wd)
        _check_update(dt, V, w, c, Vd, wd)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_striding_grid(dt):
    """More chunks than workgroups: the first workgroups walk a second chunk."""
    n = (MAX_GRID + 3) * _chunk(dt) + 7
    assert -(-n // _chunk(dt)) > MAX_GRID
    V, w, c = _case(dt, 2, n)
    Vd, wd = _dev_view(V), _dev_view(w)
    _check_dots(dt, V, w, Vd, wd)
    _check_update(dt, V, w, c, Vd, wd)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("ld_pad,off", [(8, 0), (3, 0), (8, 1), (0, 1), (5, 3)], ids=["ldvec", "ldodd", "offodd", "off1", "both"])
def test_layout_and_aliasing(dt, ld_pad, off):
    j = 5
    n = _chunk(dt) + 1 if ld_pad != 8 else _chunk(dt) + 8
    V, w, c = _case(dt, j, n, key=ld_pad + 10 * off)
    Vd, wd = _dev_view(V, ld=n + ld_pad, off=off), _dev_view(w, off=off)
    assert Vd.stride(0) == n + ld_pad
    _check_dots(dt, V, w, Vd, wd)
    _check_dots(dt, V, w, Vd, wd, scale=-0.375)
    _check_update(dt, V, w, c, Vd, wd)
    _check_update(dt, V, w, c, Vd, wd, want_c=False)
    _check_update(dt, V, w, c, Vd, wd, want_n=False)
    _check_update(dt, V, w, c, Vd, wd, want_c=False, want_n=False)
    _check_update(dt, V, w, c, Vd, wd, alias=True)  # last: it overwrites wd


def test_too_many_rows_is_unsupported():
    n = 16
    V = torch.zeros((65, n), dtype=torch.float32, device="cuda")
    w = torch.zeros((n,), dtype=torch.float32, device="cuda")
    c = _f64(65)
    work = _dev.krylov_workspace(64, n, w)
    st = _dev.stream()
    assert lib.pxa_krylov_dots(0, 65, n, V.data_ptr(), n, w.data_ptr(), None, c.data_ptr(), work.data_ptr(), st) == -3
    assert lib.pxa_krylov_update(0, 65, n, V.data_ptr(), n, w.data_ptr(), c.data_ptr(), w.data_ptr(), None, None,
                                 work.data_ptr(), st) == -3
    assert lib.pxa_krylov_dots(0, 0, n, V.data_ptr(), n, w.data_ptr(), None, c.data_ptr(), work.data_ptr(), st) == -1
    assert lib.pxa_krylov_dots(0, 2, n, V.data_ptr(), n - 1, w.data_ptr(), None, c.data_ptr(), work.data_ptr(), st) == -1
    assert int(lib.pxa_krylov_workspace_bytes(65, n)) == 0
    torch.cuda.synchronize()
    assert float(c[0]) == 123.0  # nothing was launched


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_nan_reaches_only_its_outputs(dt):
    j, n, r, m = 6, 2 * _chunk(dt) + 9, 3, _chunk(dt) + 2
    V, w, c = _case(dt, j, n)
    V[r, m] = np.nan
    Vd, wd = _dev_view(V), _dev_view(w)
    work = _dev.krylov_workspace(j, n, wd)
    out, cn, nr = _f64(j), _f64(j), _f64(1)
    _dev.krylov_dots(Vd, j, wd, out, work)
    got = out.cpu().numpy()
    assert np.isnan(got[r]) and np.isfinite(np.delete(got, r)).all()
    wo = torch.empty_like(wd)
    _dev.krylov_update(Vd, j, wd, torch.from_numpy(c).cuda(), wo, work, c_next=cn, nrm2_out=nr)
    wh = wo.cpu().numpy()
    assert np.isnan(wh[m]) and np.isfinite(np.delete(wh, m)).all()
    assert np.isnan(cn.cpu().numpy()).all() and np.isnan(nr.cpu().numpy()).all()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_zero_norm_gives_zero_row(dt):
    j, n = 3, 257
    V, _, c = _case(dt, j, n)
    Vd = _dev_view(V)
    wd = torch.zeros((n,), dtype=Vd.dtype, device="cuda")
    work = _dev.krylov_workspace(j, n, wd)
    nr = _f64(1)
    wo = torch.empty_like(wd)
    _dev.krylov_update(Vd, j, wd, torch.zeros(j, dtype=torch.float64, device="cuda"), wo, work, nrm2_out=nr)
    assert float(nr[0]) == 0.0
    x = torch.from_numpy(V[0].copy()).cuda()  # a non-zero row with a zero norm value must come out as zeros too
    for src in (wo, x):
        _dev.krylov_normalize(src, nr, src)
        np.testing.assert_array_equal(src.cpu().numpy(), np.zeros(n, dtype=dt))
    nr.fill_(4.0)
    y = torch.from_numpy(V[1].copy()).cuda()
    _dev.krylov_normalize(y, nr, y)
    np.testing.assert_array_equal(y.cpu().numpy(), (V[1].astype(np.float64) * 0.5).astype(dt))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_same_call_same_bits(dt):
    j, n = 17, 5 * _chunk(dt) + 3
    V, w, c = _case(dt, j, n)
    Vd, wd = _dev_view(V), _dev_view(w)
    cd = torch.from_numpy(c).cuda()
    runs = []
    for _ in range(2):
        work = _dev.krylov_workspace(j, n, wd)
        out, cn, nr, wo = _f64(j), _f64(j), _f64(1), torch.empty_like(wd)
        _dev.krylov_dots(Vd, j, wd, out, work)
        _dev.krylov_update(Vd, j, wd, cd, wo, work, c_next=cn, nrm2_out=nr)
        runs.append([t.cpu().numpy() for t in (out, cn, nr, wo)])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_three_launch_step_orthogonalises(dt):
    j, n = 20, 4099
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((n, j)))
    V = np.ascontiguousarray(Q.T).astype(dt)
    w = rng.standard_normal(n).astype(dt)
    Vd, wd = _dev_view(V), _dev_view(w)
    work = _dev.krylov_workspace(j, n, wd)
    c1, c2, nr = _f64(j), _f64(j), _f64(1)
    w1, w2 = torch.empty_like(wd), torch.empty_like(wd)
    _dev.krylov_dots(Vd, j, wd, c1, work)
    _dev.krylov_update(Vd, j, wd, c1, w1, work, c_next=c2)
    _dev.krylov_update(Vd, j, w1, c2, w2, work, nrm2_out=nr)
    wh = w2.cpu().numpy().astype(np.float64)
    worst = np.abs(V.astype(np.float64) @ wh).max()
    print(f"orthogonality {np.dtype(dt).name}: max|V w'| / (eps ||w'||) = {worst / (np.finfo(dt).eps * np.linalg.norm(wh)):.3f}")
    assert worst <= 8 * np.finfo(dt).eps * np.linalg.norm(wh)
    assert abs(float(nr[0]) - wh @ wh) <= (n + 4) * U * (wh @ wh)
