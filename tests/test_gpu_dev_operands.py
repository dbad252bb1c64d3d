"""
Operand checks of pyxu_amd._dev: a buffer a kernel would write (`out=`, in-place operands) that is strided, short,
of the wrong dtype or on the host raises before anything is launched -- a sentinel-filled allocation around it stays
untouched -- and every form that was legal before still gives the bits of the allocating call (`out=None`):
`out` aliasing `x`, a contiguous view off a 16-byte boundary, a flat `out` for a shaped `x`, a strided input.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

from pyxu_amd import _dev  # noqa: E402

SENTINEL = -7.25  # exact in every dtype used here
GUARD = 4  # sentinel elements on each side of the offending buffer
F32, F64 = torch.float32, torch.float64


def _dev_values(shape, dtype=F32, seed=0):
    a = np.random.default_rng(seed).standard_normal(int(np.prod(shape))).reshape(shape)
    return torch.as_tensor(a, device="cuda").to(dtype)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.int64)


# family -> (call(out), numel of a valid out, dtype of a valid out); the inputs are the smallest that pass each
# wrapper's own shape checks
def _axpby():
    x = _dev_values(5)
    return (lambda out: _dev.axpby(2.0, x, out=out)), 5, F32


def _binary():
    x, y = _dev_values(5), _dev_values(5, seed=1)
    return (lambda out: _dev.binary(_dev.BIN_ADD, x, y, out=out)), 5, F32


def _prox_l21():
    x = _dev_values(6)
    return (lambda out: _dev.prox_l21(x, 0.1, 1, 2, 3, out=out)), 6, F32


def _row_reduce():
    x = _dev_values((3, 7))
    return (lambda out: _dev.row_reduce(_dev.RED_SUMSQ, x, out=out)), 3, F64


def _row_shrink():
    x, mu = _dev_values((2, 3)), torch.full((2,), 0.5, dtype=F64, device="cuda")
    return (lambda out: _dev.row_shrink(x, mu, _dev.SHRINK_SOFT, out=out)), 6, F32


def _gather_cols():
    x, idx = _dev_values((2, 4)), torch.tensor([0, 2, 3], dtype=torch.int64, device="cuda")
    return (lambda out: _dev.gather_cols(x, idx, out=out)), 6, F32


def _complex_mul():
    a, b = _dev_values((1, 6)), _dev_values((1, 6), seed=1)
    return (lambda out: _dev.complex_mul(a, b, out=out)), 6, F32


def _fft():
    z = _dev_values(8)  # one line of 4 complex values
    return (lambda out: _dev.fft(z, (4,), (0,), 1, False, out=out)), 8, F32


def _nufft_deconv():
    z, corr = _dev_values((1, 8)), _dev_values(4, seed=1)  # 4 modes onto a fine grid of 8
    return (lambda out: _dev.nufft_deconv((4,), (8,), 0, True, corr, z, out=out)), 16, F32


def _krylov_normalize():
    x, nrm2 = _dev_values(5), torch.full((1,), 2.0, dtype=F64, device="cuda")
    return (lambda out: _dev.krylov_normalize(x, nrm2, out)), 5, F32


FAMILIES = dict(axpby=_axpby, binary=_binary, prox_l21=_prox_l21, row_reduce=_row_reduce, row_shrink=_row_shrink,
                gather_cols=_gather_cols, complex_mul=_complex_mul, fft=_fft, nufft_deconv=_nufft_deconv,
                krylov_normalize=_krylov_normalize)


def _bad_out(fault, m, dtype):
    """(the sentinel-filled allocation, the offending view of it, the exception) for a valid out of m x dtype."""
    if fault == "strided":  # every other element: buf[::2]
        base = torch.full((2 * m + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        return base, base[GUARD: GUARD + 2 * m: 2], ValueError
    if fault == "short":
        base = torch.full((m - 1 + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        return base, base[GUARD: GUARD + m - 1], ValueError
    if fault == "dtype":
        base = torch.full((m + 2 * GUARD,), SENTINEL, dtype=F64 if dtype == F32 else F32, device="cuda")
        return base, base[GUARD: GUARD + m], TypeError
    base = torch.full((m + 2 * GUARD,), SENTINEL, dtype=dtype)  # "host"
    return base, base[GUARD: GUARD + m], TypeError


@pytest.mark.parametrize("fault", ["strided", "short", "dtype", "host"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_bad_out_is_rejected_before_launch(family, fault):
    call, m, dtype = FAMILIES[family]()
    base, out, exc = _bad_out(fault, m, dtype)
    assert out.numel() == (m - 1 if fault == "short" else m) and out.is_contiguous() == (fault != "strided")
    with pytest.raises(exc):
        call(out)
    torch.cuda.synchronize()
    assert bool((base == SENTINEL).all()), f"{family}: a rejected `out` ({fault}) was written"


def test_where_condition_must_be_bool():
    x, y = _dev_values(5), _dev_values(5, seed=1)
    keep = x.clone()
    with pytest.raises(TypeError):
        _dev.where(x, x, y)  # a float condition
    with pytest.raises(TypeError):
        _dev.where((x > 0).cpu(), x, y)  # a host condition
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    np.testing.assert_array_equal(_dev.where(x > 0, x, y).cpu().numpy(), np.where((x > 0).cpu(), x.cpu(), y.cpu()))


def _guarded(shape, dtype=F32):
    n = int(np.prod(shape))
    base = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return base, base[GUARD: GUARD + n].reshape(shape)


def test_flag_buffer_with_two_flags_is_rejected():
    fb = _dev.HostFlagBuffer(1, 1, 2)  # one value, two flags: the kernels set exactly one
    rows = 2
    base_a, a = _guarded((rows,))
    base_t = torch.full((rows + 2 * GUARD,), 3, dtype=torch.int32, device="cuda")
    f = _dev_values(rows)
    with pytest.raises(ValueError, match="HostFlagBuffer"):
        _dev.ls_armijo(f, f.clone(), torch.zeros(rows, dtype=F64, device="cuda"), 0, 1e-4, 0.5, a,
                       base_t[GUARD: GUARD + rows], fb)
    n = 5
    t = _dev_values((1, n))
    base_z, z_new = _guarded((1, n))
    base_o, out = _guarded((1, n))
    work = _dev.proxadam_workspace(1, n, t)
    with pytest.raises(ValueError, match="HostFlagBuffer"):
        _dev.proxadam_sub_step(_dev.PROX_L1, 1, 0.0, 1e-4, 0.05, 0.1, t, t.clone(), t.clone(), t.clone(), z_new, out,
                               work, fb)
    torch.cuda.synchronize()
    assert fb.seq == 0 and not fb.flags.any()  # no publication was started
    assert bool((base_a == SENTINEL).all()) and bool((base_t == 3).all())
    assert bool((base_z == SENTINEL).all()) and bool((base_o == SENTINEL).all())


def test_dense_normal_pfold_takes_one_row():
    A = _dev_values((4, 8))
    p = _dev_values((2, 8), seed=1)  # two right-hand sides: the partials' offset is that of one row only
    base, p_new = _guarded((2, 8))
    with pytest.raises(ValueError, match="single row"):
        _dev.dense_normal_pfold(A, p, p, p_new, None, None, None, 0, 1.0, 0.0, None, None)
    torch.cuda.synchronize()
    assert bool((base == SENTINEL).all())


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n", [5, 8])  # the scalar tail alone; whole 16-byte vectors
def test_out_may_be_x(n, dtype):
    x, y = _dev_values(n, dtype), _dev_values(n, dtype, seed=1)
    ref = _dev.axpby(2.0, x, -0.5, y)
    xx = x.clone()
    got = _dev.axpby(2.0, xx, -0.5, y, out=xx)
    assert got is xx and torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_out_one_element_off_a_vector_boundary(dtype):
    x, y = _dev_values(8, dtype), _dev_values(8, dtype, seed=1)
    ref = _dev.axpby(2.0, x, -0.5, y)
    base = torch.full((10,), SENTINEL, dtype=dtype, device="cuda")
    out = base[1:9]
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    got = _dev.axpby(2.0, x, -0.5, y, out=out)
    assert got is out and torch.equal(_bits(got), _bits(ref))
    assert float(base[0]) == SENTINEL and float(base[9]) == SENTINEL


def test_flat_out_for_a_shaped_x():
    x = _dev_values((2, 4))
    ref = _dev.axpby(2.0, x)
    out = torch.empty(8, dtype=F32, device="cuda")
    got = _dev.axpby(2.0, x, out=out)
    assert got is out and ref.shape == (2, 4) and torch.equal(_bits(got), _bits(ref))


def test_strided_input_goes_through_the_copy():
    base = _dev_values((2, 8))
    x = base[:, ::2]
    assert not x.is_contiguous()
    keep = base.clone()
    got = _dev.axpby(2.0, x)
    assert got.shape == (2, 4) and torch.equal(_bits(got), _bits(_dev.axpby(2.0, x.contiguous())))
    assert torch.equal(base, keep)
