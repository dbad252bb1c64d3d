"""Non-uniform FFT LinOp (reference operator/linop/fft/nufft.py:84-1920).

Two paths.  The exact exponential sum the reference computes with ``eps=0`` (``_nudft``, nufft.py:2820-2892):
O(M N) work on the tiled NUDFT kernel (pxa_nudft), for types 1, 2 and 3.  And, with ``eps > 0``, the gridding
transform the reference delegates to FINUFFT (nufft.py:1367-1400, 1660-1689): spreading with the "exponential of
semicircle" kernel onto an oversampled grid, an FFT, and a per-mode correction (pxa_nufft_spread /
pxa_nufft_interp / pxa_nufft_deconv around pxa_fft_ex).  Type 3 rescales sources and targets, spreads the sources
onto an outer grid and runs a type-2 transform of that grid to the rescaled targets, with a complex factor per
source and per target (pxa_nufft_spread_fac / pxa_nufft_interp_fac).  ``method`` chooses; ``"auto"`` grids once
the transform is large enough (``GRID_CROSSOVER``; for type 3 ``GRID_CROSSOVER_T3``, ``T3_PAIRS_PER_CELL`` and
``GRID_MAX_CELLS``) and otherwise serves a positive ``eps`` by the exact sum, which meets any tolerance.
"""
import math
import warnings

import numpy as np

import pyxu_amd.abc as pxa
import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev
from pyxu_amd.operator.linop.stencil import PrecisionWarning
from pyxu_amd.util import as_canonical_shape, is_device_array, to_device, to_NUMPY

__all__ = ["NUFFT"]

_EPS_MSG = (
    "NUFFT: eps={eps:g} is served by direct evaluation of the exponential sum, which is exact but costs "
    "O(M N) = {cost:.3g} complex exponentials per transform (the gridding transform takes over from {floor:.3g} "
    "(point, mode) pairs on, or when forced: method='grid' for types 1 and 2, method='grid3' for type 3)."
)

# method="auto" grids from this many (point, mode) pairs on.  Measured (scripts/bench_nufft_grid.py):
# the smallest tested M prod(N) from which the gridded apply and adjoint both beat pxa_nudft in 1, 2 and 3 dimensions
# at eps = 1e-4 and 1e-6 (in 1 and 2 dimensions they do from 2^20 on; the 3-D spreading at eps = 1e-6 loses or
# ties up to 2^28).  Never below 2^20 pairs: a direct transform of that size is launch-bound, and the gridded chain is four
# launches.
GRID_CROSSOVER = 1 << 30
# Type 3, method="auto": grids iff eps > 0, prod(nf2) <= GRID_MAX_CELLS and
# M N >= max(GRID_CROSSOVER_T3, T3_PAIRS_PER_CELL prod(nf2)), nf2 the inner fine grid.  The grid of a type-3 transform
# follows the space-bandwidth product prod(X_d S_d) of the point clouds, not a mode count the caller chose, so the
# second term keeps a sparse transform on a huge grid with the exact sum.  Measured (scripts/bench_nufft_type3.py,
# DESIGN.md §8j), by the rule of GRID_CROSSOVER.  GRID_CROSSOVER_T3: the smallest tested M N (M = N, an outer grid of
# about M cells) from which the gridded apply and adjoint both beat pxa_nudft in 1, 2 and 3 dimensions at eps = 1e-4
# and 1e-6 (in one dimension they do from 2^20 on, in two from 2^28; the 3-D apply at eps = 1e-6 still loses at 2^30).
# T3_PAIRS_PER_CELL: the smallest M N / prod(nf2) among the cells tested at or above that crossover (4854.5, D = 3),
# rounded up; at M N = 2^30 the chain was not seen to lose on sparser grids, down to 243 pairs per cell.
# GRID_MAX_CELLS, fine-grid cells per stack row, is a declared guard against a grid nobody asked for, not a
# measurement; a stack is processed in chunks of rows that stay below it.
GRID_CROSSOVER_T3 = 1 << 32
T3_PAIRS_PER_CELL = 4855
GRID_MAX_CELLS = 1 << 30
_METHODS = ("auto", "grid", "grid3", "direct")


def _as_canonical_coordinate(x):
    """(M,) / (M, D) host or device coordinates -> (M, D) host array (nufft.py:804-811)."""
    x = to_NUMPY(x) if is_device_array(x) else np.asarray(x)
    if x.ndim == 1:
        x = x.reshape((-1, 1))
    elif x.ndim == 2:
        assert 1 <= x.shape[-1] <= 3, "Only (1,2,3)-D transforms supported."
    else:
        raise ValueError(f"Expected 1D/2D array, got {x.ndim}-D array.")
    return np.ascontiguousarray(x)


def _as_canonical_mode(N):
    N = as_canonical_shape(N)
    assert all(_ > 0 for _ in N)
    assert 1 <= len(N) <= 3, "Only (1,2,3)-D transforms supported."
    return N


def _view_as_real_mat(cmat, real_input):
    """Real (2 R, 2 C) matrix of a complex (R, C) one acting on interleaved (re, im) vectors; with `real_input`
    the columns that multiply imaginary parts are dropped: (2 R, C)."""
    R, C = cmat.shape
    rdt = np.float32 if cmat.dtype == np.complex64 else np.float64
    A = np.empty((2 * R, 2 * C), dtype=rdt)
    A[0::2, 0::2] = cmat.real
    A[0::2, 1::2] = -cmat.imag
    A[1::2, 0::2] = cmat.imag
    A[1::2, 1::2] = cmat.real
    return np.ascontiguousarray(A[:, 0::2]) if real_input else A


def _mesh(N, modeord, dtype):
    grid = np.stack(
        np.meshgrid(*[np.arange(-(n // 2), (n - 1) // 2 + 1, dtype=dtype) for n in N], indexing="ij"),
        axis=-1,
    )
    if modeord == 1:  # FFT order
        grid = np.fft.ifftshift(grid, axes=np.arange(len(N)))
    return grid


def _common(isign, eps, real, enable_warnings, kwargs, cost, gridded=False, floor=None):
    modeord = int(kwargs.get("modeord", 0))
    if modeord not in (0, 1):
        raise ValueError(f"modeord must be 0 or 1, got {modeord}.")
    eps, enable_warnings = float(eps), bool(enable_warnings)
    if eps > 0 and enable_warnings and not gridded:
        msg = _EPS_MSG.format(eps=eps, cost=float(cost), floor=float(GRID_CROSSOVER if floor is None else floor))
        warnings.warn(msg, UserWarning, stacklevel=3)
    return int(np.sign(isign)), bool(real), enable_warnings, modeord


def _method(kwargs):
    method = kwargs.get("method", "auto")
    if method not in _METHODS:
        raise ValueError(f"method must be one of {_METHODS}, got {method!r}.")
    return method


def _use_grid(method, eps, pairs):
    """Whether a type-1 / type-2 transform of `pairs` = M prod(N) runs on the gridding path."""
    if method == "grid3":
        raise ValueError("NUFFT: method='grid3' is the type-3 gridding transform; types 1 and 2 take method='grid'.")
    if method == "grid":
        if not float(eps) > 0:
            raise ValueError("NUFFT: method='grid' needs eps > 0 (eps = 0 is the exact sum, method='direct').")
        return True
    return method == "auto" and float(eps) > 0 and pairs >= GRID_CROSSOVER


# ------------------------------------------------------------------ gridding: parameters and plan (host, float64)
def _grid_sigma(upsampfac):
    """Upsampling factor: 2 unless the caller asks for 1.25 (None / 0: the default)."""
    if upsampfac is None or float(upsampfac) in (0.0, 2.0):
        return 2.0
    if float(upsampfac) == 1.25:
        return 1.25
    raise ValueError(f"upsampfac must be 2 or 1.25, got {upsampfac!r}.")


def _grid_width(eps, sigma):
    """The width the tolerance asks for, before the clamp to [2, 16]."""
    eps = float(eps)
    guard = 1e-9  # eps = 10^-k gives w = k + 1, whatever the last bit of the logarithm
    if sigma == 2.0:
        return math.ceil(-math.log10(eps) + 1 - guard)
    return math.ceil(-math.log(eps) / (math.pi * math.sqrt(1 - 1 / sigma)) - guard)


def _grid_kernel(eps, sigma):
    """(w, beta): support in fine-grid cells and shape of phi(z) = exp(beta (sqrt(1 - z^2) - 1))."""
    w = min(max(_grid_width(eps, sigma), 2), 16)
    if sigma == 2.0:
        beta = {2: 2.20, 3: 2.26, 4: 2.38}.get(w, 2.30) * w
    else:
        beta = 0.97 * math.pi * (1 - 0.5 / sigma) * w
    return w, beta


def _smooth_even(n):
    """Smallest even length >= n whose prime factors are in {2, 3, 5, 7} (the lengths the Stockham FFT handles)."""
    n = max(int(n), 2)
    n += n % 2
    while True:
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 2


def _grid_size(N, sigma, w):
    return tuple(_smooth_even(max(math.floor(sigma * n), 2 * w)) for n in N)


_GL_NODES = 128


def _grid_correction(n, nf, w, beta, nodes=_GL_NODES):
    """1 / psi_hat(k) for the n modes k = -(n // 2) .. (n - 1) // 2 of an axis of nf cells, with
    psi_hat(k) = (w / 2) int_{-1}^{1} phi(z) cos(k (2 pi / nf) (w / 2) z) dz.  With z = sin(t) the integrand is
    entire in t (no square-root end points), and Gauss-Legendre on [-pi/2, pi/2] converges geometrically."""
    t, wt = np.polynomial.legendre.leggauss(nodes)
    t, wt = 0.5 * np.pi * t, 0.5 * np.pi * wt
    k = np.arange(-(n // 2), (n - 1) // 2 + 1, dtype=np.float64)
    alpha = k * (np.pi * w / nf)
    f = np.exp(beta * (np.cos(t) - 1.0)) * np.cos(t) * wt
    psi = 0.5 * w * (np.cos(alpha[:, None] * np.sin(t)[None, :]) @ f)
    return 1.0 / psi


def _grid_plan(x, nf, w, bin_shape, dtype):
    """Plan of the M points x (M, D) on the fine grid nf: per point and axis the first touched cell
    l0 = ceil(xi - w/2) (int32) and the offset xi - l0 in [w/2 - 1, w/2] (`dtype`), xi = (x mod 2 pi) nf / 2 pi,
    both in the order of a stable sort by bin (`perm`: sorted position -> point; `bin_start`: nbins + 1 offsets).
    A bin is a tile of `bin_shape` cells, its id row-major, and a point belongs to the bin of floor(xi)."""
    x = np.asarray(x, dtype=np.float64)
    nf_a, e = np.asarray(nf, dtype=np.int64), np.asarray(bin_shape, dtype=np.int64)
    xi = np.mod(x, 2 * np.pi) * (nf_a / (2 * np.pi))
    xi[(xi >= nf_a) | (xi < 0)] = 0.0  # the fold can round up to the period itself
    l0 = np.ceil(xi - 0.5 * w)
    off = xi - l0
    cell = np.minimum(np.floor(xi).astype(np.int64), nf_a - 1)
    nb = (nf_a + e - 1) // e
    bins = np.zeros(x.shape[0], dtype=np.int64)
    for d in range(x.shape[1]):
        bins = bins * nb[d] + cell[:, d] // e[d]
    perm = np.argsort(bins, kind="stable").astype(np.int64)
    counts = np.bincount(bins, minlength=int(np.prod(nb)))
    bin_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(
        l0=np.ascontiguousarray(l0[perm].astype(np.int32)),
        off=np.ascontiguousarray(off[perm].astype(dtype)),
        perm=perm,
        bin_start=bin_start,
    )


# ------------------------------------------------------------------ type 3: rescaling and factors (host, float64)
def _t3_widths(x, z):
    """Per axis the half-widths and centres (X, C) of the sources and (S, Dc) of the targets, and the safe
    half-widths (Xs, Ss) with Xs Ss >= 1 (FINUFFT's set_nhg_type3): only one of the two is ever enlarged."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    X, C = 0.5 * (x.max(axis=0) - x.min(axis=0)), 0.5 * (x.max(axis=0) + x.min(axis=0))
    S, Dc = 0.5 * (z.max(axis=0) - z.min(axis=0)), 0.5 * (z.max(axis=0) + z.min(axis=0))
    Xs, Ss = X.copy(), S.copy()
    for d in range(x.shape[1]):
        if X[d] == 0 and S[d] == 0:
            Xs[d] = Ss[d] = 1.0
        elif X[d] == 0:
            Xs[d] = 1.0 / S[d]
        else:
            Ss[d] = max(S[d], 1.0 / X[d])
    return dict(X=X, C=C, S=S, Dc=Dc, Xs=Xs, Ss=Ss)


def _t3_cells(wd, sigma, w):
    """Per axis the least length of the outer grid, max(floor(2 sigma Xs Ss / pi + (w + 1)), 2 w) (reference
    _fft_shape, nufft.py:1932-1947), as floats: the sizes before they are rounded up to FFT lengths, which may be
    too large to round."""
    return [max(math.floor(min(2 * sigma * a * b / math.pi + (w + 1), 1e300)), 2 * w)
            for a, b in zip(wd["Xs"], wd["Ss"])]


def _t3_params(x, z, eps, sigma, max_cells=None):
    """Parameters of the gridded type 3: kernel (w, beta), outer grid nf1, inner fine grid nf2, scale gamma, the
    centres, and `cells` = prod(nf2).  With `max_cells`, a transform whose fine grid would exceed it gets nf1 = nf2 =
    None and a lower bound of `cells` (no FFT length is searched for at that size)."""
    w, beta = _grid_kernel(eps, sigma)
    wd = _t3_widths(x, z)
    least = _t3_cells(wd, sigma, w)
    cells = float(np.prod([math.floor(sigma * n) for n in least]))
    if max_cells is None or cells <= max_cells:
        nf1 = tuple(_smooth_even(n) for n in least)
        nf2 = _grid_size(nf1, sigma, w)
        cells = int(np.prod(nf2))
        if max_cells is None or cells <= max_cells:
            gamma = np.asarray(nf1, dtype=np.float64) / (2 * sigma * wd["Ss"])
            return dict(wd, w=w, beta=beta, nf1=nf1, nf2=nf2, gamma=gamma, cells=cells)
    return dict(wd, w=w, beta=beta, nf1=None, nf2=None, gamma=None, cells=cells)


def _t3_rescale(x, z, prm):
    """x' = (x - C) / gamma on the outer grid (|x'| < pi, no footprint wraps) and z' = (z - Dc) gamma 2 pi / nf1,
    the frequencies of the inner type 2 in radians per outer cell (|z'| <= pi / sigma)."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    xp = (x - prm["C"]) / prm["gamma"]
    zp = (z - prm["Dc"]) * prm["gamma"] * 2.0 * np.pi / np.asarray(prm["nf1"], dtype=np.float64)
    return xp, zp


_T3_CHUNK = 4096  # targets per pass of the correction quadrature: a (chunk, _GL_NODES) cosine table


def _t3_psi_hat(omega, w, beta, nodes=_GL_NODES):
    """psi_hat(omega) = (w / 2) int_{-1}^{1} phi(t) cos(omega (w / 2) t) dt, the quadrature of `_grid_correction`
    at real frequencies omega (radians per cell) in place of k 2 pi / nf."""
    t, wt = np.polynomial.legendre.leggauss(nodes)
    t, wt = 0.5 * np.pi * t, 0.5 * np.pi * wt
    f = np.exp(beta * (np.cos(t) - 1.0)) * np.cos(t) * wt
    sin_t = np.sin(t)
    omega = np.asarray(omega, dtype=np.float64)
    out = np.empty(omega.shape[0])
    for a in range(0, omega.shape[0], _T3_CHUNK):
        alpha = omega[a:a + _T3_CHUNK] * (0.5 * w)
        out[a:a + _T3_CHUNK] = 0.5 * w * (np.cos(alpha[:, None] * sin_t[None, :]) @ f)
    return out


def _t3_factors(x, z, zp, prm):
    """pre_j = exp(i <Dc, x_j - C>) (M,) and post_k = exp(i <z_k, C>) / prod_d psi_hat(z'_kd) (N,), complex128, for
    isign = +1 (isign = -1 conjugates them: the correction is real)."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    pre = np.exp(1j * ((x - prm["C"]) @ prm["Dc"]))
    corr = np.ones(z.shape[0])
    for d in range(z.shape[1]):
        corr /= _t3_psi_hat(zp[:, d], prm["w"], prm["beta"])
    return pre, np.exp(1j * (z @ prm["C"])) * corr


def _t3_width_ok(eps, sigma):
    """Whether the gridded type 3 can reach `eps`: at upsampling factor 1.25 a width clamped to 16 leaves the error
    of its two composed approximations far above the tolerance."""
    return not (sigma == 1.25 and _grid_width(eps, sigma) > 16)


def _interleave(c, dtype):
    """complex (K,) -> (K, 2) real pairs, rounded once to `dtype`."""
    return np.ascontiguousarray(np.stack([c.real, c.imag], axis=-1).astype(dtype))


def _NUFFT12_args(x, N):
    x, N = _as_canonical_coordinate(x), _as_canonical_mode(N)
    if x.shape[-1] == len(N):
        pass
    elif len(N) == 1:
        N = N * x.shape[-1]
    else:
        raise ValueError("x vs. N: dimensionality mis-match.")
    return x, N


class NUFFT(pxa.LinOp):
    r"""Non-uniform Fourier transforms of type 1 (non-uniform -> uniform), 2 (uniform -> non-uniform) and 3
    (non-uniform -> non-uniform) in 1, 2 or 3 dimensions (nufft.py:84-737), evaluated exactly or, with ``eps > 0``
    and a transform large enough, by gridding to relative accuracy ``eps``.

    Complex arrays are real views ``(..., 2 K)`` of interleaved (re, im) pairs; leading dimensions are a stack.

    ``type1`` / ``type2`` take ``method="auto" | "grid" | "direct"``.  ``"direct"`` is the exact sum (O(M N)).
    ``"grid"`` (needs ``eps > 0``) is the gridding transform to relative accuracy ``eps``: kernel width and shape
    from ``eps`` and ``upsampfac`` (2, the default, or 1.25; anything else is a ``ValueError``), a plan built on the
    host at construction.  ``"auto"`` grids when ``eps > 0`` and M prod(N) >= ``GRID_CROSSOVER`` and otherwise takes
    the exact sum, with a ``UserWarning`` naming its cost when ``eps > 0``.  ``apply`` and ``adjoint`` of a gridded
    operator are exact adjoints of each other (to rounding, not merely to ``eps``); its ``asarray`` /
    ``ascomplexarray`` are the exact transform's matrix, which the operator matches to ``eps``.

    ``type3`` takes ``method="auto" | "grid3" | "direct"``.  ``"grid3"`` (needs ``eps > 0``) is the gridded type 3:
    sources and targets are rescaled, the sources spread onto an outer grid, and a type-2 transform of that grid
    evaluated at the rescaled targets, with a phase factor per source and a phase and correction factor per target.
    Its grid follows the space-bandwidth product of the two point clouds: above ``GRID_MAX_CELLS`` fine-grid cells
    ``"grid3"`` is a ``ValueError``, and so is ``upsampfac=1.25`` with an ``eps`` whose kernel width would be
    clamped (``eps`` below about 1.7e-10).  ``"auto"`` grids when ``eps > 0``, the fine grid has at most
    ``GRID_MAX_CELLS`` cells and M N >= max(``GRID_CROSSOVER_T3``, ``T3_PAIRS_PER_CELL`` times the cells), and
    otherwise takes the exact sum with the warning.  ``method="grid"`` on ``type3`` still raises
    ``NotImplementedError`` and ``"grid3"`` on ``type1`` / ``type2`` is a ``ValueError``: one spelling for both is a
    follow-up (it changes what an existing test pins).  ``chunked=True`` is not available.

    ``n_trans``, ``plan_fw`` / ``plan_bw`` and the other FINUFFT options are accepted and have no effect.
    """

    def __init__(self, shape):
        super().__init__(shape=shape)

    @staticmethod
    @pxrt.enforce_precision(i="x", o=False, allow_None=False)
    def type1(x, N, isign=1, eps=1e-4, real=False, plan_fw=True, plan_bw=True, enable_warnings=True, **kwargs):
        r"""u_n = \sum_j w_j exp(i isign <n, x_j>): (..., [2] M) -> (..., 2 prod N) (nufft.py:337-434)."""
        x, N = _NUFFT12_args(x, N)
        pairs = x.shape[0] * int(np.prod(N))
        sigma, gridded = _grid_sigma(kwargs.get("upsampfac")), _use_grid(_method(kwargs), eps, pairs)
        isign, real, ew, modeord = _common(isign, eps, real, enable_warnings, kwargs, pairs, gridded)
        grid = _mesh(N, modeord, x.dtype).reshape(-1, x.shape[1])
        if gridded:
            return _NUFFTGrid(1, x, grid, isign, real, ew, N, modeord, eps, sigma)
        return _NUDFT(x, grid, isign, real, ew, mode=N, modeord=modeord, typ=1)

    @staticmethod
    @pxrt.enforce_precision(i="x", o=False, allow_None=False)
    def type2(x, N, isign=1, eps=1e-4, real=False, plan_fw=True, plan_bw=True, enable_warnings=True, **kwargs):
        r"""w_j = \sum_n u_n exp(i isign <n, x_j>): (..., [2] prod N) -> (..., 2 M) (nufft.py:438-546)."""
        x, N = _NUFFT12_args(x, N)
        pairs = x.shape[0] * int(np.prod(N))
        sigma, gridded = _grid_sigma(kwargs.get("upsampfac")), _use_grid(_method(kwargs), eps, pairs)
        isign, real, ew, modeord = _common(isign, eps, real, enable_warnings, kwargs, pairs, gridded)
        grid = _mesh(N, modeord, x.dtype).reshape(-1, x.shape[1])
        if gridded:
            return _NUFFTGrid(2, x, grid, isign, real, ew, N, modeord, eps, sigma)
        return _NUDFT(grid, x, isign, real, ew, mode=N, modeord=modeord, typ=2)

    @staticmethod
    @pxrt.enforce_precision(i=("x", "z"), o=False, allow_None=False)
    def type3(x, z, isign=1, eps=1e-4, real=False, plan_fw=True, plan_bw=True, enable_warnings=True, chunked=False,
              parallel=False, **kwargs):
        r"""v_k = \sum_j w_j exp(i isign <z_k, x_j>): (..., [2] M) -> (..., 2 N) (nufft.py:550-737)."""
        if bool(chunked):
            raise NotImplementedError("NUFFT.type3(chunked=True) is not available.")
        method = _method(kwargs)
        if method == "grid":
            raise NotImplementedError("NUFFT.type3(method='grid'): the type-3 gridding transform is method='grid3'.")
        x, z = _as_canonical_coordinate(x), _as_canonical_coordinate(z)
        assert x.shape[-1] == z.shape[-1], "x vs. z: dimensionality mis-match."
        kwargs.pop("modeord", None)
        z = z.astype(x.dtype, copy=False)
        pairs, eps = x.shape[0] * z.shape[0], float(eps)
        sigma, prm, floor = _grid_sigma(kwargs.get("upsampfac")), None, GRID_CROSSOVER_T3
        if method == "grid3":
            if not eps > 0:
                raise ValueError("NUFFT: method='grid3' needs eps > 0 (eps = 0 is the exact sum, method='direct').")
            if not _t3_width_ok(eps, sigma):
                raise ValueError(f"NUFFT.type3: upsampfac=1.25 cannot reach eps={eps:g} on the gridding path (kernel "
                                 f"width {_grid_width(eps, sigma)} > 16); use upsampfac=2.")
            prm = _t3_params(x, z, eps, sigma, GRID_MAX_CELLS)
            if prm["nf2"] is None:
                raise ValueError(f"NUFFT.type3(method='grid3'): the inner fine grid has at least {prm['cells']:.4g} "
                                 f"cells, more than GRID_MAX_CELLS = {GRID_MAX_CELLS}: it follows the space-bandwidth "
                                 "product of the sources and targets.")
        elif method == "auto" and eps > 0 and pairs >= GRID_CROSSOVER_T3 and _t3_width_ok(eps, sigma):
            prm = _t3_params(x, z, eps, sigma, GRID_MAX_CELLS)
            if prm["nf2"] is not None:
                floor = max(GRID_CROSSOVER_T3, T3_PAIRS_PER_CELL * prm["cells"])
            if prm["nf2"] is None or pairs < floor:
                prm = None
        isign, real, ew, _ = _common(isign, eps, real, enable_warnings, kwargs, pairs, prm is not None, floor)
        if prm is not None:
            return _NUFFTGrid3(x, z, isign, real, ew, eps, sigma, prm)
        return _NUDFT(x, z, isign, real, ew)


class _NUDFT(NUFFT):
    r"""out_n = \sum_m w_m exp(i isign <src_m, tgt_n>): (..., [2] M) -> (..., 2 N).  With ``real`` the input of
    ``apply`` (and the output of ``adjoint``) is real-valued."""

    def __init__(self, src, tgt, isign, real, enable_warnings, mode=None, modeord=0, typ=3):
        self._src, self._tgt = src, tgt  # host (M, D) / (N, D), one dtype
        self._typ = int(typ)
        self._isign = int(isign)
        self._real = bool(real)
        self._enable_warnings = bool(enable_warnings)
        self._mode, self._modeord = mode, int(modeord)  # type 1 / 2 only
        self._D = src.shape[1]
        self._pts = None  # device copies, uploaded at first use
        M, N = src.shape[0], tgt.shape[0]
        super().__init__(shape=(2 * N, M if self._real else 2 * M))
        self.lipschitz = float(np.sqrt(M * N))  # analytical upper bound (nufft.py:1438, 1723)

    def _device_points(self):
        if self._pts is None:
            self._pts = (to_device(self._src), to_device(self._tgt))
        return self._pts

    def _warn_cast(self, arr):
        x_width = pxrt.Width(self._src.dtype)
        if arr.dtype != x_width.torch:
            if self._enable_warnings:
                msg = f"NUFFT was configured to run with {x_width.value} inputs, but provided {arr.dtype} inputs."
                warnings.warn(msg, PrecisionWarning)
            arr = to_device(arr, dtype=x_width.torch)
        return arr

    def _stacked(self, arr, width):
        if arr.shape[-1] != width:
            raise ValueError(f"NUFFT: expected a trailing dimension of {width}, got {tuple(arr.shape)}.")
        return arr.reshape(-1, width), tuple(arr.shape[:-1])

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.dim)
        if self._real:
            w = _dev.real_to_complex(w)
        src, tgt = self._device_points()
        out = _dev.nudft(src, tgt, self._isign, w)
        return out.reshape(*sh, self.codim)

    @pxrt.enforce_precision(i="arr")
    def adjoint(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.codim)
        src, tgt = self._device_points()
        out = _dev.nudft(tgt, src, -self._isign, w)
        if self._real:
            out = _dev.complex_real_part(out)
        return out.reshape(*sh, self.dim)

    def ascomplexarray(self, xp=None, dtype=None):
        """(N, M) complex matrix exp(i isign tgt src^T), built on the host (nufft.py:1595-1610, 1871-1880)."""
        c_dtype = pxrt.getPrecision().complex.value if dtype is None else np.dtype(dtype)
        A = np.exp(1j * self._isign * (self._tgt.astype(np.float64) @ self._src.astype(np.float64).T))
        return A.astype(c_dtype)

    def asarray(self, xp=None, dtype=None):
        """Real matrix of the operator, built on the host; a device tensor unless ``xp`` is numpy."""
        c_dtype = pxrt.Width(np.dtype(pxrt.getPrecision().value if dtype is None else dtype)).complex.value
        A = _view_as_real_mat(self.ascomplexarray(dtype=c_dtype), real_input=self._real)
        return A if xp is np else to_device(A)

    def mesh(self, xp=None, dtype=None, scale="unit", upsampled=False):
        """(N1, ..., Nd, d) mode grid of a type-1 / type-2 transform (nufft.py:1612-1642)."""
        if self._mode is None:
            raise NotImplementedError("NUFFT.mesh(): the type-3 grids belong to its gridding transform (not built).")
        if scale != "unit" or upsampled:
            raise NotImplementedError("NUFFT.mesh(): only scale='unit', upsampled=False.")
        dtype = pxrt.getPrecision().value if dtype is None else dtype
        return _mesh(self._mode, self._modeord, dtype)

    def _generic_normal(self, which, weights, eps, fused):
        if not (weights is None and eps is None and fused is None):
            raise ValueError(f"NUFFT.{which}(): weights / eps / fused belong to the Toeplitz form (gram of a type-2, "
                             "cogram of a complex type-1 transform); this operator has the generic product only.")
        return getattr(pxa.LinOp, which)(self)

    def gram(self, weights=None, eps=None, fused=None):
        r"""A^H A.  For a type-2 transform the Toeplitz operator :py:class:`_NUFFTGram` (A^H diag(weights) A with
        ``weights``); otherwise the generic product ``A.T * A``."""
        if self._typ == 2:
            return _NUFFTGram(self, self._isign, self._real, weights, eps, fused)
        return self._generic_normal("gram", weights, eps, fused)

    def cogram(self, weights=None, eps=None, fused=None):
        r"""A A^H.  A type-1 transform of sign s is the adjoint of the type 2 of sign -s, so its cogram is that
        transform's Toeplitz gram (not with ``real=True``, whose adjoint drops the imaginary part between the two
        factors); otherwise the generic product ``A * A.T``."""
        if self._typ == 1 and not self._real:
            return _NUFFTGram(self, -self._isign, False, weights, eps, fused)
        return self._generic_normal("cogram", weights, eps, fused)


class _NUFFTGrid(_NUDFT):
    r"""Type-1 / type-2 transform of accuracy ``eps`` on the oversampled grid.  With S the spreading matrix of the
    plan, F the unnormalised DFT of sign ``isign`` on the fine grid, T the restriction to the N central modes and C
    the diagonal correction, type 1 is C T F S and type 2 is S^T F T^T C; each is the adjoint of the other with the
    opposite sign, so ``apply`` and ``adjoint`` share one plan and both kernels.  Shapes, ``mesh``, ``lipschitz``,
    ``asarray`` / ``ascomplexarray`` (the exact transform's matrix) come from the exact operator."""

    def __init__(self, typ, x, grid, isign, real, enable_warnings, N, modeord, eps, sigma):
        src, tgt = (x, grid) if typ == 1 else (grid, x)
        super().__init__(src, tgt, isign, real, enable_warnings, mode=N, modeord=modeord, typ=typ)
        self._eps, self._sigma = float(eps), float(sigma)
        self._w, self._beta = _grid_kernel(eps, sigma)
        self._nf = _grid_size(N, sigma, self._w)
        code = 0 if x.dtype == np.float32 else 1
        self._bin_shape = _dev.nufft_grid_tiles(code, self._D)[0]
        self._plan = _grid_plan(x, self._nf, self._w, self._bin_shape, x.dtype)
        self._plan["corr"] = np.concatenate(
            [_grid_correction(n, nf, self._w, self._beta) for n, nf in zip(N, self._nf)]
        ).astype(x.dtype)
        self._plan_dev = None  # uploaded at first use

    def _device_plan(self):
        if self._plan_dev is None:
            p = self._plan
            self._plan_dev = tuple(to_device(p[k]) for k in ("l0", "off", "perm", "bin_start", "corr"))
        return self._plan_dev

    def _type1(self, c, isign):
        """c (Q, 2 M) -> modes (Q, 2 prod N): spread, FFT, extract and correct."""
        *plan, corr = self._device_plan()
        g = _dev.nufft_spread(self._nf, self._w, self._beta, plan, c)
        _dev.fft(g, self._nf, tuple(range(self._D)), g.shape[0], isign > 0, out=g)
        return _dev.nufft_deconv(self._mode, self._nf, self._modeord, False, corr, g)

    def _type2(self, u, isign):
        """modes u (Q, 2 prod N) -> (Q, 2 M): correct and zero-embed, FFT, interpolate."""
        *plan, corr = self._device_plan()
        g = _dev.nufft_deconv(self._mode, self._nf, self._modeord, True, corr, u)
        _dev.fft(g, self._nf, tuple(range(self._D)), g.shape[0], isign > 0, out=g)
        return _dev.nufft_interp(self._nf, self._w, self._beta, plan, g)

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.dim)
        if self._real:
            w = _dev.real_to_complex(w)
        out = (self._type1 if self._typ == 1 else self._type2)(w, self._isign)
        return out.reshape(*sh, self.codim)

    @pxrt.enforce_precision(i="arr")
    def adjoint(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.codim)
        out = (self._type2 if self._typ == 1 else self._type1)(w, -self._isign)
        if self._real:
            out = _dev.complex_real_part(out)
        return out.reshape(*sh, self.dim)


class _NUFFTGrid3(_NUDFT):
    r"""Type-3 transform of accuracy ``eps``.  With P and R the diagonal factors ``pre`` and ``post``, S_x the
    spreading matrix of the rescaled sources on the outer grid nf1, C the correction that embeds that grid (its cell
    l mod nf1 is mode l of the inner type 2, FFT order) in the inner fine grid nf2, F the unnormalised DFT of sign
    ``isign`` on nf2 and S_z the spreading matrix of the rescaled targets there, the transform is
    R S_z^T F C S_x P, and its adjoint the transposed chain with the opposite sign and conjugated factors: one plan
    pair, both kernels, adjoint to rounding.  A stack runs in chunks of rows of at most ``GRID_MAX_CELLS`` fine-grid
    cells.  Shapes, ``lipschitz``, ``asarray`` / ``ascomplexarray`` (the exact transform's matrix) come from the
    exact operator."""

    def __init__(self, x, z, isign, real, enable_warnings, eps, sigma, prm=None):
        super().__init__(x, z, isign, real, enable_warnings)
        prm = _t3_params(x, z, eps, sigma) if prm is None else prm
        self._eps, self._sigma, self._prm = float(eps), float(sigma), prm
        self._w, self._beta, self._nf1, self._nf2 = prm["w"], prm["beta"], prm["nf1"], prm["nf2"]
        code = 0 if x.dtype == np.float32 else 1
        bin_shape = _dev.nufft_grid_tiles(code, self._D)[0]
        xp, zp = _t3_rescale(x, z, prm)
        pre, post = _t3_factors(x, z, zp, prm)
        self._plan_x = _grid_plan(xp, self._nf1, self._w, bin_shape, x.dtype)
        self._plan_z = _grid_plan(zp, self._nf2, self._w, bin_shape, x.dtype)
        # the factors ride with the sorted points: entry s belongs to point perm[s]
        self._plan_x["fac"] = _interleave(pre[self._plan_x["perm"]], x.dtype)
        self._plan_z["fac"] = _interleave(post[self._plan_z["perm"]], x.dtype)
        self._corr = np.concatenate(
            [_grid_correction(n, nf, self._w, self._beta) for n, nf in zip(self._nf1, self._nf2)]
        ).astype(x.dtype)
        self._plan_dev = None  # uploaded at first use

    def _device_plan(self):
        if self._plan_dev is None:
            up = lambda p: tuple(to_device(p[k]) for k in ("l0", "off", "perm", "bin_start", "fac"))  # noqa: E731
            self._plan_dev = (up(self._plan_x), up(self._plan_z), to_device(self._corr))
        return self._plan_dev

    def _rows(self, Q):
        """Stack rows per pass: rows prod(nf2) <= GRID_MAX_CELLS."""
        return max(1, min(Q, GRID_MAX_CELLS // int(np.prod(self._nf2))))

    # the normal operators of a type 3 are not Toeplitz: the generic products, whatever _NUDFT overrides
    def gram(self):
        return pxa.LinOp.gram(self)

    def cogram(self):
        return pxa.LinOp.cogram(self)

    def _chain(self, c, forward):
        """forward: c (Q, 2 M) -> (Q, 2 N); otherwise the transposed chain (Q, 2 N) -> (Q, 2 M)."""
        (*px, fx), (*pz, fz), corr = self._device_plan()
        axes, conj = tuple(range(self._D)), (self._isign < 0) == forward
        out = _dev.empty((c.shape[0], self.codim if forward else 2 * self._src.shape[0]), c)
        step = self._rows(c.shape[0])
        for r in range(0, c.shape[0], step):
            rows = c[r:r + step]
            if forward:
                g = _dev.nufft_spread(self._nf1, self._w, self._beta, px, rows, fac=fx, conj=conj)
                g = _dev.nufft_deconv(self._nf1, self._nf2, 1, True, corr, g)
                _dev.fft(g, self._nf2, axes, g.shape[0], self._isign > 0, out=g)
                _dev.nufft_interp(self._nf2, self._w, self._beta, pz, g, out=out[r:r + step], fac=fz, conj=conj)
            else:
                g = _dev.nufft_spread(self._nf2, self._w, self._beta, pz, rows, fac=fz, conj=conj)
                _dev.fft(g, self._nf2, axes, g.shape[0], self._isign < 0, out=g)
                g = _dev.nufft_deconv(self._nf1, self._nf2, 1, False, corr, g)
                _dev.nufft_interp(self._nf1, self._w, self._beta, px, g, out=out[r:r + step], fac=fx, conj=conj)
        return out

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.dim)
        if self._real:
            w = _dev.real_to_complex(w)
        return self._chain(w, True).reshape(*sh, self.codim)

    @pxrt.enforce_precision(i="arr")
    def adjoint(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        w, sh = self._stacked(arr, self.codim)
        out = self._chain(w, False)
        if self._real:
            out = _dev.complex_real_part(out)
        return out.reshape(*sh, self.dim)


# ------------------------------------------------------------------ Toeplitz gram of a type-2 transform
# Longest line the fused kernel keeps in LDS (pxa_toeplitz_apply: two buffers of complex cells in 160 KB).
_TOEPLITZ_RESIDENT = {np.dtype(np.float32): 10240, np.dtype(np.float64): 5120}
# fused=None in two and three dimensions: the fused kernel up to this many cells per axis, the length at which a
# workgroup still holds 4 lines (64 KB of LDS for two buffers).  Measured in fp32 (scripts/bench_nufft_gram.py, DESIGN.md
# §8k): against the chain of existing kernels it wins at P = 512 and 1024 and loses at 2048 (2 lines, by 3 %) and 4096
# (1 line, by 19 %), where the in-place power-of-two FFT kernel behind the chain holds more lines of a strided axis.
# The fp64 figure is the same line count, not a measurement.  One dimension is a single launch and wins at 8192.
_TOEPLITZ_BEST = {np.dtype(np.float32): 1024, np.dtype(np.float64): 512}
# The spectrum of the embedded kernel is real because t[-d] = conj(t[d]); what the transform leaves in the imaginary
# part is its own rounding: for an FFT of prod(P) cells an error of about u sqrt(log2 prod P) ||t||_2 per cell, and
# max |spectrum| >= rms(spectrum) = ||t||_2 (Parseval).  1024 u (u the unit roundoff of the working precision)
# leaves two orders of magnitude for log factors and the asymmetry of t's own rounding; a kernel that is not
# Hermitian misses it by many orders.
_KHAT_IMAG_TOL = 1024.0


def _toeplitz_sizes(N, modeord):
    """Per axis the cells P = _smooth_even(2 n - 1) of the circular convolution and the split of the cell map
    (sample i in cell i when i < split, else in cell i + P - n): n for ascending modes, (n - 1) // 2 + 1 for FFT
    order (the negative modes at the top)."""
    P = tuple(_smooth_even(2 * n - 1) for n in N)
    split = tuple(n if modeord == 0 else (n - 1) // 2 + 1 for n in N)
    return P, split


class _NUFFTGram(pxa.SelfAdjointOp):
    r"""G = A^H diag(w) A of a type-2 transform A (sign ``isign``, modes N, points x): the multilevel Toeplitz matrix
    G[n, n'] = t[n - n'], t[d] = \sum_j w_j exp(-i isign <d, x_j>), applied exactly as a circular convolution on
    P_d = _smooth_even(2 N_d - 1) cells per axis: zero-pad, FFT, multiply by the real spectrum ``khat`` of the
    embedded t, inverse FFT, crop.  t is one type-1 transform of the weights onto 2 N - 1 modes, evaluated once at
    the first ``apply`` (exactly with ``eps = 0``, else by gridding to ``eps``); after that no non-uniform point is
    touched, and the cost of an ``apply`` depends on N alone.

    ``fused=True`` runs pxa_toeplitz_apply (pruned line passes, the last axis fused in LDS); ``fused=False`` the
    chain of existing kernels (embed, FFT, product, inverse FFT, extract) on the full padded grid, which serves any
    length; ``fused=None`` takes the faster of the two as measured (``_TOEPLITZ_BEST``).  They agree to rounding.
    With ``real`` the operator acts on real vectors of length prod N."""

    def __init__(self, parent, isign, real, weights=None, eps=None, fused=None):
        x = parent._tgt if parent._typ == 2 else parent._src
        N = tuple(int(n) for n in parent._mode)
        M, cells = x.shape[0], int(np.prod(N))
        super().__init__(shape=(cells if real else 2 * cells,) * 2)
        self._x, self._N, self._isign, self._real = x, N, int(isign), bool(real)
        self._src, self._enable_warnings = x, parent._enable_warnings  # (_warn_cast)
        self._modeord = parent._modeord
        if weights is not None:
            weights = to_NUMPY(weights) if is_device_array(weights) else np.asarray(weights)
            if np.iscomplexobj(weights) or weights.dtype.kind not in "fiu":
                raise ValueError(f"NUFFT.gram(weights=...): real weights expected, got {weights.dtype}.")
            if weights.shape != (M,):
                raise ValueError(f"NUFFT.gram(weights=...): expected shape ({M},), got {weights.shape}.")
            weights = np.ascontiguousarray(weights, dtype=x.dtype)
        self._weights = weights
        self._eps = float(getattr(parent, "_eps", 0.0) if eps is None else eps)
        if not self._eps >= 0:
            raise ValueError(f"NUFFT.gram(eps=...): eps >= 0 expected, got {eps!r}.")
        self._sigma = getattr(parent, "_sigma", 2.0)
        self._P, self._split = _toeplitz_sizes(N, self._modeord)
        resident = max(self._P) <= _TOEPLITZ_RESIDENT[np.dtype(x.dtype)]
        if fused and not resident:
            raise ValueError(f"NUFFT.gram(fused=True): the padded lengths {self._P} exceed the "
                             f"{_TOEPLITZ_RESIDENT[np.dtype(x.dtype)]} cells the fused kernel keeps in LDS.")
        best = resident and (len(N) == 1 or max(self._P) <= _TOEPLITZ_BEST[np.dtype(x.dtype)])
        self._fused = best if fused is None else bool(fused)
        self._khat = self._khat_c = self._ones = None  # device plan, built at first use
        self.lipschitz = float(M if weights is None else np.abs(weights.astype(np.float64)).sum()) * cells

    _warn_cast = _NUDFT._warn_cast
    _stacked = _NUDFT._stacked

    def _plan(self):
        """khat (prod P, real, 1 / prod P folded in) on the device."""
        if self._khat is not None:
            return self._khat
        x, N, P, D = self._x, self._N, self._P, len(self._N)
        n2 = tuple(2 * n - 1 for n in N)  # modes d = -(n - 1) .. n - 1, ascending
        with pxrt.Precision(pxrt.Width(x.dtype)):
            kw = dict(method="grid", upsampfac=self._sigma) if self._eps > 0 else dict(method="direct")
            psf = NUFFT.type1(x, n2, isign=-self._isign, eps=self._eps, real=True, enable_warnings=False, **kw)
            w = np.ones(x.shape[0], dtype=x.dtype) if self._weights is None else self._weights
            with pxrt.EnforcePrecision(False):
                t = psf.apply(to_device(w.reshape(1, -1)))
        ones = to_device(np.ones(sum(n2), dtype=x.dtype))
        g = _dev.nufft_deconv(n2, P, 0, True, ones, t)  # t[d] in cell d mod P
        _dev.fft(g, P, tuple(range(D)), 1, False, out=g)
        spec = to_NUMPY(g).reshape(-1, 2)  # one-off: the check below reads every cell
        top = float(np.abs(spec[:, 0]).max())
        imag = float(np.abs(spec[:, 1]).max())
        if not imag <= _KHAT_IMAG_TOL * np.finfo(x.dtype).eps * top:
            raise RuntimeError(f"NUFFT gram: the spectrum of the Toeplitz kernel is not real (max |Im| = {imag:.3e} "
                               f"against max |Re| = {top:.3e}): the kernel t is not Hermitian.")
        self._khat = to_device(np.ascontiguousarray(spec[:, 0] / float(np.prod(P)), dtype=x.dtype))
        return self._khat

    def _rows(self, Q):
        """Stack rows per pass: the pass's workspace stays below GRID_MAX_CELLS cells."""
        N, P = self._N, self._P
        if not self._fused:
            cells = int(np.prod(P))
        elif len(N) == 1:
            cells = N[0]
        else:  # (P0, N1[, N2]) and, in three dimensions, (P0, P1, N2)
            cells = P[0] * N[-1] * (1 if len(N) == 2 else N[1] + P[1])
        return max(1, min(Q, GRID_MAX_CELLS // cells))

    def _fallback(self, u, out):
        """The same convolution from existing kernels, on the full padded grid (mode k in cell k mod P: a cyclic
        shift of the fused kernel's placement, so the same khat serves)."""
        N, P, axes = self._N, self._P, tuple(range(len(self._N)))
        if self._khat_c is None:
            self._khat_c = _dev.real_to_complex(self._khat.reshape(1, -1))
            self._ones = to_device(np.ones(sum(N), dtype=self._x.dtype))
        g = _dev.nufft_deconv(N, P, self._modeord, True, self._ones, u)
        _dev.fft(g, P, axes, g.shape[0], False, out=g)
        _dev.complex_mul(g, self._khat_c, out=g)
        _dev.fft(g, P, axes, g.shape[0], True, out=g)
        return _dev.nufft_deconv(N, P, self._modeord, False, self._ones, g, out=out)

    @pxrt.enforce_precision(i="arr")
    def apply(self, arr):
        arr = self._warn_cast(_dev.require(arr, "arr"))
        u, sh = self._stacked(arr, self.dim)
        if self._real:
            u = _dev.real_to_complex(u)
        khat = self._plan()
        out = _dev.empty(tuple(u.shape), u)
        step = self._rows(u.shape[0])
        for r in range(0, u.shape[0], step):
            if self._fused:
                _dev.toeplitz_apply(self._N, self._P, self._split, khat, u[r:r + step], out=out[r:r + step])
            else:
                self._fallback(u[r:r + step], out[r:r + step])
        if self._real:
            out = _dev.complex_real_part(out)
        return out.reshape(*sh, self.dim)
