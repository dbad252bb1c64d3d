"""
Host restatement of the gridding NUFFT (types 1 and 2), the yardstick of the kernels in csrc/nufft_grid.hip and of
the operator's ``method="grid"`` path.  Everything here is NumPy: parameters, plan, spreading and interpolation as
plain loops over the points, ``numpy.fft`` on the fine grid, the correction factors by quadrature.

    phi(z) = exp(beta (sqrt(1 - z^2) - 1)),  |z| <= 1
    type 1:  spread  g[l] = sum_j c_j prod_d phi(2 (l_d - xi_jd) / w)  (periodic),  G = DFT_isign(g),
             u_k = G[k mod nf] / prod_d psi_hat_d(k_d)
    type 2:  g[k mod nf] = u_k / prod_d psi_hat_d(k_d) (zero elsewhere),  h = DFT_isign(g),
             w_j = sum_l h[l] prod_d phi(2 (l_d - xi_jd) / w)

``dtype`` = float64 runs the chain in double precision (the algorithm's own error against the exact sum,
tests/_nudft_refs.py::nudft64); ``dtype`` = float32 rounds the plan's offsets, the kernel values, the products, the
sums and the FFT's result to single precision (the same plan, the same order of operations per point).

RATIO_CAP: the achieved relative l2 error of the float64 chain, divided by eps, stays below this over the case list of
tests/test_nufft_grid_host.py::test_achieved_error (every golden type-1 / type-2 case, D = 1, 2, 3, both upsampling
factors, eps from 1e-2 to 1e-12).  It is twice the worst ratio that test measures (printed there): 2.159, at D = 2,
upsampling factor 2; the worst per (D, factor) are 1.85 / 1.76 (D = 1, factor 2 / 1.25), 2.16 / 1.02 (D = 2) and
1.35 / 0.71 (D = 3).
"""
import math

import numpy as np

RATIO_CAP = 2 * 2.159

EPS64 = (1e-2, 1e-4, 1e-6, 1e-9, 1e-12)
SIGMAS = (2.0, 1.25)


# ------------------------------------------------------------------ parameters
def kernel_params(eps, sigma=2.0):
    """(w, beta) of the kernel for a tolerance and an upsampling factor."""
    if sigma == 2.0:
        w = int(math.ceil(round(-math.log10(eps) + 1.0, 9)))
    elif sigma == 1.25:
        w = int(math.ceil(round(-math.log(eps) / (math.pi * math.sqrt(1.0 - 1.0 / sigma)), 9)))
    else:
        raise ValueError(sigma)
    w = min(max(w, 2), 16)
    if sigma == 2.0:
        beta = (2.20 if w == 2 else 2.26 if w == 3 else 2.38 if w == 4 else 2.30) * w
    else:
        beta = 0.97 * math.pi * (1.0 - 0.5 / sigma) * w
    return w, beta


def _smooth(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def fine_size(N, sigma, w):
    out = []
    for n in N:
        m = max(int(math.floor(sigma * n)), 2 * w)
        m += m % 2
        while not _smooth(m):
            m += 2
        out.append(m)
    return tuple(out)


def phi(z, beta, dtype=np.float64):
    """The kernel in `dtype` arithmetic (z already in `dtype`)."""
    z = np.asarray(z, dtype=dtype)
    s = np.maximum(dtype(1) - z * z, dtype(0))
    return np.exp(dtype(beta) * (np.sqrt(s) - dtype(1))).astype(dtype)


def psi_hat(n, nf, w, beta, nodes=128):
    """psi_hat(k) = (w/2) int_{-1}^{1} phi(z) cos(k (2 pi / nf) (w/2) z) dz for the n modes of an axis, k ascending,
    by Gauss-Legendre quadrature after z = sin(t) (the integrand becomes entire in t)."""
    t, wt = np.polynomial.legendre.leggauss(nodes)
    t, wt = 0.5 * np.pi * t, 0.5 * np.pi * wt
    k = np.arange(-(n // 2), (n - 1) // 2 + 1, dtype=np.float64)
    out = np.empty(n)
    for a, kk in enumerate(k):
        alpha = kk * 2.0 * np.pi / nf * 0.5 * w
        out[a] = 0.5 * w * np.sum(wt * np.exp(beta * (np.cos(t) - 1.0)) * np.cos(alpha * np.sin(t)) * np.cos(t))
    return out


def correction(N, nf, w, beta, dtype=np.float64, nodes=128):
    """The concatenated per-axis vectors 1 / psi_hat_d(k), k ascending, in `dtype`."""
    return np.concatenate([1.0 / psi_hat(n, f, w, beta, nodes) for n, f in zip(N, nf)]).astype(dtype)


# ------------------------------------------------------------------ plan
def fold(x, nf):
    """x (M, D) -> xi in [0, nf) per axis, float64."""
    xi = np.mod(np.asarray(x, dtype=np.float64), 2.0 * np.pi) * (np.asarray(nf, dtype=np.float64) / (2.0 * np.pi))
    xi[xi >= np.asarray(nf, dtype=np.float64)] = 0.0
    return xi


def plan(x, nf, w, bin_shape, dtype=np.float64):
    """dict(l0, off, perm, bin_start, nb): first cells (int32) and offsets (`dtype`) in bin-sorted order, the sort
    permutation (sorted position -> point) and the bin offsets; bins of `bin_shape` cells, ids row-major."""
    xi = fold(x, nf)
    M, D = xi.shape
    l0 = np.ceil(xi - w / 2.0).astype(np.int64)
    off = xi - l0
    nb = [-(-int(f) // int(e)) for f, e in zip(nf, bin_shape)]
    bins = np.zeros(M, dtype=np.int64)
    for d in range(D):
        cell = np.minimum(np.floor(xi[:, d]).astype(np.int64), nf[d] - 1)
        bins = bins * nb[d] + cell // int(bin_shape[d])
    perm = np.argsort(bins, kind="stable").astype(np.int64)
    nbins = int(np.prod(nb))
    start = np.zeros(nbins + 1, dtype=np.int64)
    for b in bins:
        start[b + 1] += 1
    start = np.cumsum(start)
    return dict(l0=l0[perm].astype(np.int32), off=off[perm].astype(dtype), perm=perm, bin_start=start, nb=tuple(nb))


# ------------------------------------------------------------------ the three stages
def _point_footprint(p, s, nf, w, beta, dtype):
    """Per axis the wrapped cell indices and the kernel values of the sorted point `s`."""
    idx, ker = [], []
    for d in range(len(nf)):
        i = np.arange(w)
        idx.append((int(p["l0"][s, d]) + i) % nf[d])
        z = (i.astype(dtype) - dtype(p["off"][s, d])) * dtype(2.0 / w)
        ker.append(phi(z, beta, dtype))
    return idx, ker


def _outer(ker, dtype):
    k = ker[0]
    for v in ker[1:]:
        k = (k[..., None] * v).astype(dtype)
    return k


def spread(p, nf, w, beta, c, dtype=np.float64):
    """c (Q, M) complex -> (Q, *nf) complex, in `dtype` arithmetic."""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    c = np.asarray(c).astype(cdt)
    g = np.zeros((c.shape[0], *nf), dtype=cdt)
    for s in range(p["perm"].shape[0]):
        idx, ker = _point_footprint(p, s, nf, w, beta, dtype)
        k = _outer(ker, dtype)
        g[(slice(None), *np.ix_(*idx))] += c[:, p["perm"][s]].reshape(-1, *([1] * len(nf))) * k
    return g


def interp(p, nf, w, beta, g, dtype=np.float64):
    """g (Q, *nf) complex -> (Q, M) complex."""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    g = np.asarray(g).astype(cdt)
    M = p["perm"].shape[0]
    out = np.zeros((g.shape[0], M), dtype=cdt)
    for s in range(M):
        idx, ker = _point_footprint(p, s, nf, w, beta, dtype)
        k = _outer(ker, dtype)
        out[:, p["perm"][s]] = (g[(slice(None), *np.ix_(*idx))] * k).reshape(g.shape[0], -1).sum(axis=1)
    return out


def mode_cells(n, nf, modeord):
    """For the n modes of an axis in array order: (fine-grid cell k mod nf, index k + n // 2 into the correction)."""
    k = np.arange(-(n // 2), (n - 1) // 2 + 1)
    if modeord == 1:
        k = np.concatenate([k[k >= 0], k[k < 0]])
    return k % nf, k + n // 2


def _corr_nd(N, nf, corr, modeord):
    cells, fac, o = [], None, 0
    for n, f in zip(N, nf):
        cell, ci = mode_cells(n, f, modeord)
        cells.append(cell)
        v = corr[o + ci]
        fac = v if fac is None else (fac[..., None] * v).astype(corr.dtype)
        o += n
    return cells, fac


def deconv_from_grid(N, nf, corr, modeord, G):
    """G (Q, *nf) -> the N central modes (Q, *N), scaled."""
    cells, fac = _corr_nd(N, nf, corr, modeord)
    return (G[(slice(None), *np.ix_(*cells))] * fac).astype(G.dtype)


def deconv_to_grid(N, nf, corr, modeord, u):
    """u (Q, *N) -> (Q, *nf): scaled, mode k in cell k mod nf, zero elsewhere."""
    cells, fac = _corr_nd(N, nf, corr, modeord)
    g = np.zeros((u.shape[0], *nf), dtype=u.dtype)
    g[(slice(None), *np.ix_(*cells))] = (u * fac).astype(u.dtype)
    return g


def dft(g, isign, dtype):
    """Unnormalised DFT of sign `isign` over the trailing axes; the result rounded to `dtype`'s complex type."""
    axes = tuple(range(1, g.ndim))
    G = np.fft.ifftn(g.astype(np.complex128), axes=axes, norm="forward") if isign > 0 else \
        np.fft.fftn(g.astype(np.complex128), axes=axes)
    return G.astype(np.complex64 if dtype == np.float32 else np.complex128)


# ------------------------------------------------------------------ whole transforms
class Chain:
    """Plan and parameters of a point set: ``type1(c, isign)`` / ``type2(u, isign)`` on complex (Q, .) arrays."""

    def __init__(self, x, N, eps, sigma=2.0, modeord=0, dtype=np.float64, bin_shape=None):
        self.N, self.modeord, self.dtype = tuple(int(n) for n in N), int(modeord), dtype
        self.w, self.beta = kernel_params(eps, sigma)
        self.nf = fine_size(self.N, sigma, self.w)
        bin_shape = bin_shape if bin_shape is not None else self.nf  # one bin: the sorted order is the given one
        self.plan = plan(np.asarray(x).reshape(len(x), -1), self.nf, self.w, bin_shape, dtype)
        self.corr = correction(self.N, self.nf, self.w, self.beta, dtype)

    def type1(self, c, isign):
        g = spread(self.plan, self.nf, self.w, self.beta, c, self.dtype)
        G = dft(g, isign, self.dtype)
        return deconv_from_grid(self.N, self.nf, self.corr, self.modeord, G).reshape(G.shape[0], -1)

    def type2(self, u, isign):
        cdt = np.complex64 if self.dtype == np.float32 else np.complex128
        u = np.asarray(u).astype(cdt).reshape(-1, *self.N)
        g = deconv_to_grid(self.N, self.nf, self.corr, self.modeord, u)
        return interp(self.plan, self.nf, self.w, self.beta, dft(g, isign, self.dtype), self.dtype)


def op_transform(c, which, eps, sigma=2.0, dtype=np.float64, bin_shape=None):
    """apply / adjoint of a golden type-1 / type-2 case (tests/_nudft_refs.py::golden_cases) through the gridding
    chain: the complex (Q, K) result, comparable with ``_nudft_refs.op_transform(nudft64, c, which)[0]``."""
    import _nudft_refs as R

    w = R.op_weights(c, which)
    ch = Chain(c["x"], c["N"], eps, sigma, c["modeord"], dtype, bin_shape)
    forward = which == "apply"
    sgn = c["isign"] if forward else -c["isign"]
    # apply of type 1 and adjoint of type 2 are type-1 chains; the other two are type-2 chains
    return ch.type1(w, sgn) if (c["typ"] == 1) == forward else ch.type2(w, sgn)
