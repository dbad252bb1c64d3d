"""
Host restatement of the gridding NUFFT of type 3, the yardstick of pxa_nufft_spread_fac / pxa_nufft_interp_fac and of
the operator's ``method="grid3"`` path.  Built on tests/_nufft_grid_refs.py (``plan``, ``spread``, ``interp``,
``Chain(modeord=1)``); everything is NumPy, the plan arithmetic in float64.

    v_k = sum_j c_j exp(i s <z_k, x_j>),  sources x (M, D), targets z (N, D)

    per axis: X, C half-width and centre of x; S, Dc of z; safe widths (Xs, Ss), Xs Ss >= 1, only one enlarged
    nf1 = smallest even smooth length >= max(floor(2 sigma Xs Ss / pi + (w + 1)), 2 w),  gamma = nf1 / (2 sigma Ss)
    x' = (x - C) / gamma,  z' = (z - Dc) gamma 2 pi / nf1
    pre_j = exp(i <Dc, x_j - C>),  post_k = exp(i <z_k, C>) / prod_d psi_hat(z'_kd)
    forward: spread (c pre) at x' on nf1; type 2 of that grid (nf1 modes, FFT order) to z'; times post
    adjoint: the transposed chain: type 1 of (y conj(post)) at z', interpolated at x', times conj(pre)
    (s = -1 conjugates pre and the phase of post.)

``dtype`` = float32 rounds the factors once to complex64 and runs the products and the inner chain in single
precision, as tests/_nufft_grid_refs.py does.

RATIO_CAP_T3: the achieved relative l2 error of the float64 chain, divided by eps, stays below this over the case list
of tests/test_nufft_type3_host.py::test_achieved_error (every golden type-3 case, M = 67, N = 29, D = 1, 2, 3, apply
and adjoint; upsampling factor 2 with eps in EPS64, 1.25 with eps in EPS_125).  It is twice the worst ratio that test
measures (printed there): 6.977, at D = 3, upsampling factor 1.25, eps = 1e-6; the worst at factor 2 is 4.915 (D = 3,
eps = 1e-9).  Two composed approximations (the outer spreading and the inner type 2), hence above the types-1/2
figure.
"""
import math

import numpy as np

import _nufft_grid_refs as G

RATIO_CAP_T3 = 2 * 6.977

EPS_125 = (1e-2, 1e-4, 1e-6, 1e-9)


# ------------------------------------------------------------------ parameters
def widths(x, z):
    """dict of per-axis X, C, S, Dc and the safe widths Xs, Ss."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    D = x.shape[1]
    out = {k: np.zeros(D) for k in ("X", "C", "S", "Dc", "Xs", "Ss")}
    for d in range(D):
        X, C = (x[:, d].max() - x[:, d].min()) / 2, (x[:, d].max() + x[:, d].min()) / 2
        S, Dc = (z[:, d].max() - z[:, d].min()) / 2, (z[:, d].max() + z[:, d].min()) / 2
        if X == 0 and S == 0:
            Xs, Ss = 1.0, 1.0
        elif X == 0:
            Xs, Ss = 1.0 / S, S
        else:
            Xs, Ss = X, max(S, 1.0 / X)
        for k, v in zip(("X", "C", "S", "Dc", "Xs", "Ss"), (X, C, S, Dc, Xs, Ss)):
            out[k][d] = v
    return out


def outer_size(Xs, Ss, sigma, w):
    n = max(int(math.floor(2.0 * sigma * Xs * Ss / math.pi + (w + 1))), 2 * w)
    n += n % 2
    while not G._smooth(n):
        n += 2
    return n


def params(x, z, eps, sigma=2.0):
    """widths plus w, beta, nf1, nf2, gamma."""
    p = widths(x, z)
    w, beta = G.kernel_params(eps, sigma)
    nf1 = tuple(outer_size(a, b, sigma, w) for a, b in zip(p["Xs"], p["Ss"]))
    p.update(w=w, beta=beta, nf1=nf1, nf2=G.fine_size(nf1, sigma, w),
             gamma=np.asarray(nf1, dtype=np.float64) / (2.0 * sigma * p["Ss"]))
    return p


def rescale(x, z, p):
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    return (x - p["C"]) / p["gamma"], (z - p["Dc"]) * p["gamma"] * 2.0 * np.pi / np.asarray(p["nf1"], dtype=np.float64)


def psi_hat_at(omega, w, beta, nodes=128):
    """psi_hat(omega) = (w/2) int_{-1}^{1} phi(t) cos(omega (w/2) t) dt, one frequency at a time."""
    t, wt = np.polynomial.legendre.leggauss(nodes)
    t, wt = 0.5 * np.pi * t, 0.5 * np.pi * wt
    out = np.empty(len(omega))
    for a, om in enumerate(omega):
        out[a] = 0.5 * w * np.sum(wt * np.exp(beta * (np.cos(t) - 1.0)) * np.cos(om * 0.5 * w * np.sin(t)) * np.cos(t))
    return out


def factors(x, z, zp, p):
    """(pre (M,), post (N,)) complex128 for s = +1."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    pre = np.exp(1j * ((x - p["C"]) * p["Dc"]).sum(axis=1))
    post = np.exp(1j * (z * p["C"]).sum(axis=1))
    for d in range(z.shape[1]):
        post = post / psi_hat_at(zp[:, d], p["w"], p["beta"])
    return pre, post


# ------------------------------------------------------------------ the two chains
class Chain3:
    """``forward(c, isign)``: c (Q, M) complex -> (Q, N); ``adjoint(y, isign)``: the conjugate transpose of
    ``forward(., isign)``, (Q, N) -> (Q, M)."""

    def __init__(self, x, z, eps, sigma=2.0, dtype=np.float64, bin_shape=None):
        x, z = np.asarray(x).reshape(len(x), -1), np.asarray(z).reshape(len(z), -1)
        self.dtype, self.cdt = dtype, np.complex64 if dtype == np.float32 else np.complex128
        self.p = p = params(x, z, eps, sigma)
        self.w, self.beta, self.nf1, self.nf2 = p["w"], p["beta"], p["nf1"], p["nf2"]
        self.xp, self.zp = rescale(x, z, p)
        pre, post = factors(x, z, self.zp, p)
        self.pre, self.post = pre.astype(self.cdt), post.astype(self.cdt)
        self.plan_x = G.plan(self.xp, self.nf1, self.w, bin_shape if bin_shape is not None else self.nf1, dtype)
        self.inner = G.Chain(self.zp, self.nf1, eps, sigma, modeord=1, dtype=dtype, bin_shape=bin_shape)
        assert self.inner.nf == self.nf2 and self.inner.w == self.w

    def _fac(self, f, conj):
        return np.conj(f) if conj else f

    def forward(self, c, isign):
        c = (np.asarray(c).astype(self.cdt) * self._fac(self.pre, isign < 0)).astype(self.cdt)
        g = G.spread(self.plan_x, self.nf1, self.w, self.beta, c, self.dtype)
        v = self.inner.type2(g.reshape(g.shape[0], -1), isign)
        return (v * self._fac(self.post, isign < 0)).astype(self.cdt)

    def adjoint(self, y, isign):
        y = (np.asarray(y).astype(self.cdt) * self._fac(self.post, isign > 0)).astype(self.cdt)
        u = self.inner.type1(y, -isign).reshape(y.shape[0], *self.nf1)
        c = G.interp(self.plan_x, self.nf1, self.w, self.beta, u, self.dtype)
        return (c * self._fac(self.pre, isign > 0)).astype(self.cdt)


def op_transform(c, which, eps, sigma=2.0, dtype=np.float64, bin_shape=None):
    """apply / adjoint of a golden type-3 case (tests/_nudft_refs.py::golden_cases) through the gridded chain: the
    complex (Q, K) result, comparable with ``_nudft_refs.op_transform(nudft64, c, which)[0]``."""
    import _nudft_refs as R

    ch = Chain3(c["x"], c["z"], eps, sigma, dtype, bin_shape)
    w = R.op_weights(c, which)
    return ch.forward(w, c["isign"]) if which == "apply" else ch.adjoint(w, c["isign"])
