"""
Host restatement (float64 NumPy) of the Toeplitz form of a type-2 NUFFT's gram, the yardstick of pxa_toeplitz_apply
and of ``NUFFT.type2(..).gram()`` / ``NUFFT.type1(..).cogram()``.

    A[j, n] = exp(i isign <k_n, x_j>),   G = A^H diag(w) A,   G[n, n'] = t[k_n - k_n'],
    t[d] = sum_j w_j exp(-i isign <d, x_j>),   d_a = -(N_a - 1) .. N_a - 1

G is applied by a circular convolution on P_a >= 2 N_a - 1 cells per axis: t[d] sits in cell d mod P, khat =
fftn(embedded t) / prod P (real: t is Hermitian), and out = crop(ifftn(khat . fftn(pad(u)), norm="forward")).
Cell map of an axis: sample i sits in cell i when i < split and in cell i + P - n otherwise; split = n for modes in
ascending order (only differences of cells matter, the offset -n // 2 drops out), split = (n - 1) // 2 + 1 for FFT
order (the negative modes at the top of the line).

RATIO_CAP_GRAM: with t from the gridding type-1 chain of tolerance eps (tests/_nufft_grid_refs.py, upsampling
factor 2) in place of the exact sum, the relative l2 error of G u against the exact gram, divided by eps, stays below
this over the case list of tests/test_nufft_gram_host.py::test_achieved_error_gridded_psf (every golden type-2 point
set, eps in EPS_GRAM).  It is twice the worst ratio that test measures (printed there), by the rule of RATIO_CAP in
_nufft_grid_refs.py.  Measured worst ratios per (D, eps):

    D   1e-2    1e-4    1e-6    1e-9
    1   0.154   0.180   0.217   0.306
    2   0.374   0.399   0.489   0.459
    3   0.360   0.444   0.375   0.302
"""
import numpy as np

import _nudft_refs as R

WORST_RATIO_GRAM = 0.489  # measured (D = 2, eps = 1e-6), see the table above
RATIO_CAP_GRAM = 2 * WORST_RATIO_GRAM
EPS_GRAM = (1e-2, 1e-4, 1e-6, 1e-9)


def smooth_even(n):
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


def sizes(N, modeord):
    """(P, split) per axis."""
    P = tuple(smooth_even(2 * n - 1) for n in N)
    split = tuple(int(n) if modeord == 0 else (int(n) - 1) // 2 + 1 for n in N)
    return P, split


def cell_map(n, P, split):
    i = np.arange(n)
    return np.where(i < split, i, i + P - n)


def psf64(x, N, isign, w=None):
    """t on the (2 N_a - 1) differences, ascending per axis, complex128: the exact sum."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    d = np.stack(np.meshgrid(*[np.arange(-(n - 1), n, dtype=np.float64) for n in N], indexing="ij"), axis=-1)
    ph = d.reshape(-1, x.shape[1]) @ x.T  # (prod(2 N - 1), M)
    return (np.exp(-1j * isign * ph) @ w).reshape(*[2 * n - 1 for n in N])


def khat64(t, N, P):
    """(khat, max |Im|): the real spectrum (1 / prod P folded in) of t embedded at d mod P, and the largest imaginary
    part that was dropped, on the same scale."""
    e = np.zeros(P, dtype=np.complex128)
    cells = [np.arange(-(n - 1), n) % p for n, p in zip(N, P)]
    e[np.ix_(*cells)] = t
    spec = np.fft.fftn(e) / float(np.prod(P))
    return np.ascontiguousarray(spec.real), float(np.abs(spec.imag).max())


def toeplitz_apply64(u, N, P, split, khat):
    """u (Q, *N) complex -> (Q, *N) complex128: pad by the cell map, fftn, multiply, inverse fftn, crop."""
    u = np.asarray(u).astype(np.complex128)
    cells = [cell_map(n, p, s) for n, p, s in zip(N, P, split)]
    g = np.zeros((u.shape[0], *P), dtype=np.complex128)
    g[(slice(None), *np.ix_(*cells))] = u
    axes = tuple(range(1, g.ndim))
    g = np.fft.ifftn(np.fft.fftn(g, axes=axes) * khat, axes=axes, norm="forward")
    return g[(slice(None), *np.ix_(*cells))]


def gram_matrix64(x, N, isign, modeord=0, w=None):
    """The exact complex (prod N, prod N) matrix A^H diag(w) A of the type-2 transform, via type2_matrix64."""
    A = R.type2_matrix64(np.asarray(x, dtype=np.float64), N, isign, False, modeord)
    C = A[0::2, 0::2] + 1j * A[1::2, 0::2]  # (M, prod N)
    w = np.ones(C.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    return C.conj().T @ (w[:, None] * C)


def gram_apply64(x, N, isign, modeord, u, w=None, psf=None):
    """G u through the restatement: u (Q, prod N) complex -> (Q, prod N); `psf` replaces the exact t."""
    N = tuple(int(n) for n in N)
    P, split = sizes(N, modeord)
    t = psf64(x, N, isign, w) if psf is None else psf
    kh, _ = khat64(t, N, P)
    u = np.asarray(u)
    return toeplitz_apply64(u.reshape(-1, *N), N, P, split, kh).reshape(u.shape[0], -1)
