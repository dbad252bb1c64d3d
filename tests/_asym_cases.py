"""
Asymmetric deblurring problems shared by the CPU oracle pins (test_oracle_asymmetric.py), the GPU tests of the
fused steps (test_gpu_fused_asymmetric.py, and one case each of the variant tests) and tests/golden/make_goldens.py.

The fused PGD / PD3O / Condat-Vu steps apply G = H^T H as a sweep of the taps' autocorrelation and correct the R
boundary rows / columns with explicit ghost terms; a symmetric, centred kernel that is the same on every axis, with
unit sampling, hides a flipped kernel in those terms, exchanged axes, and exchanged forward-difference coefficients.
Every entry here therefore has per-axis different, off-centre taps (normalised to sum |k| = 1 per axis, so
||H|| <= 1 and f.diff_lipschitz = 1 stays valid for the data term) and per-axis different sampling.

Shapes are the smallest at which each code path exists (tiles are 32 x 64):
(7, 12) n < 2R; (30, 60) one tile; (37, 70) ragged 2 x 2 tiles, scalar rows (n1 % 4 != 0); (40, 68) vector rows;
(6, 9, 11) small volume; (11, 37, 70) ragged volume; (4, 33, 66) batch-as-axis (directions (1, 2)).

`mutants()` restates the conventions a kernel could get wrong; test_oracle_asymmetric.py proves that each of them
moves the oracle trajectory of every entry by >= 1e-3 (100x the fp32 tolerance) over the iterations the GPU tests run.
"""
import itertools
import zlib
from collections import namedtuple

import numpy as np

import oracle as orc

Entry = namedtuple("Entry", "name shape taps centers sampling dirs tv g dtype")

ID = ([1.0], 0)  # identity axis


def _e(name, shape, axes, sampling, tv, g, dtype, dirs=None):
    taps = [list(a[0]) for a in axes]
    cen = [int(a[1]) for a in axes]
    dirs = tuple(range(len(shape))) if dirs is None else dirs
    return Entry(name, shape, taps, cen, tuple(sampling), dirs, tv, g, dtype)


# (raw taps, centre); reach = max(centre, len - 1 - centre)
ENTRIES = [
    # one-sided, centre 0 (reach 4) / one-sided, centre len - 1 (reach exactly 8); both n < 2R
    _e("tiny", (7, 12), [([.4, .25, -.15, .1, .1], 0), ([.05, -.1, .05, .1, .15, .05, .1, .2, .2], 8)],
       (0.7, 1.9), "iso", "pos", np.float32),
    # two-sided asymmetric with negative taps, reach 2 on axis 0 and 7 on axis 1
    _e("onetile", (30, 60), [([.3, .4, -.1, .2], 1), ([.1, .2, .25, .1, -.1, .05, .05, .05, .05, .05], 2)],
       (1.9, 0.7), "l1", "l1", np.float64),
    # axis 0 blurred, axis 1 identity
    _e("ax0", (37, 70), [([.1, .1, -.2, .2, .3, .1], 4), ID], (1.3, 0.7), "iso", "l1", np.float32),
    # axis 0 identity, axis 1 blurred
    _e("ax1", (40, 68), [ID, ([.2, .3, -.1, .1, .1, .1, .1], 1)], (0.7, 1.3), "l1", "pos", np.float32),
    # vector rows with both axes blurred (the entry the bit-exact kernel-variant tests use: n1 % 4 == 0, 2 x 2 tiles)
    _e("vec", (40, 68), [([.15, -.1, .45, .2, .1], 1), ([.1, .3, .2, -.1, .2, .1], 4)], (1.9, 0.7), "iso", "none",
       np.float32),
    # 3-D, every axis its own taps
    _e("vol", (6, 9, 11), [([.5, .3, .2], 0), ([.1, -.2, .3, .4], 3), ([.2, .4, .1, -.2, .1], 1)],
       (0.7, 1.9, 1.3), "iso", "pos", np.float64),
    # 3-D, axis 0 identity (still differentiated)
    _e("vol_ax0id", (6, 9, 11), [ID, ([.5, -.2, .1, .3], 0), ([.3, .1, .6], 2)],
       (1.3, 0.7, 1.9), "l1", "none", np.float32),
    # ragged 3-D, axis 0 blurred, reach 8 on axis 1
    _e("vol_ragged", (11, 37, 70), [([.2, .5, -.1, .2], 2), ([.3, .2, .1, .1, .05, .05, -.1, .05, .05], 0),
                                     ([.1, .2, -.3, .4], 2)],
       (1.9, 1.3, 0.7), "iso", "l1", np.float32),
    # batch-as-axis: axis 0 identity and not differentiated
    _e("batch", (4, 33, 66), [ID, ([.3, -.1, .2, .4], 3), ([.4, .2, .1, .1, .1, .1], 1)],
       (1.3, 0.7, 1.9), "l1", "pos", np.float32, dirs=(1, 2)),
]
BY_NAME = {e.name: e for e in ENTRIES}
PGD_ENTRIES = [e for e in ENTRIES if len(e.shape) == 2 or e.dirs == (1, 2)]  # what the fused PGD step takes

PGD_ITERS, PDS_ITERS = 6, 8
PGD_LAM, PGD_MU = 0.05, 0.02
PDS_LAM = 0.05
G_L1 = 0.01


def ident(e):
    return e.name


def kernels(e, dt, taps=None):
    """Per-axis taps normalised to sum |k| = 1 in float64, then cast."""
    out = []
    for k in (e.taps if taps is None else taps):
        k = np.asarray(k, dtype=np.float64)
        out.append((k / np.abs(k).sum()).astype(dt))
    return out


def reach(taps, centers):
    return [max(c, len(k) - 1 - c) for k, c in zip(taps, centers)]


def data(e, dt):
    """(y, x0) of the entry, the same on every path."""
    rng = np.random.default_rng(zlib.crc32(e.name.encode()))  # (stable when entries are added)
    N = int(np.prod(e.shape))
    return rng.standard_normal(N).astype(dt), rng.uniform(0, 1, N).astype(dt)


def pgd_lipschitz(e, sampling=None):
    """1 + 4 (lam / mu) sum_a 1 / h_a^2 over the differentiated axes: ||H|| <= 1 and ||Grad||^2 <= 4 sum 1 / h_a^2."""
    s = e.sampling if sampling is None else sampling
    return 1 + 4 * (PGD_LAM / PGD_MU) * sum(1 / s[a] ** 2 for a in e.dirs)


def pds_steps(e, dt):
    """Oracle-side (tau, sigma, rho) for the CPU-only checks (the GPU tests take the solver's own)."""
    Lk = 2 * np.sqrt(sum(1 / e.sampling[a] ** 2 for a in e.dirs))
    tau, sigma, _, rho = orc.pd3o_step_sizes(1.0, Lk, dt)
    return tau, sigma, rho


# ----------------------------------------------------------------------------- conventions
Conv = namedtuple("Conv", "taps centers sampling boundary_only")


def true_conv(e):
    return Conv(e.taps, e.centers, e.sampling, False)


def _flip(taps, centers):
    return [list(k[::-1]) for k in taps], [len(k) - 1 - c for k, c in zip(taps, centers)]


def _swap(seq, a, b):
    seq = list(seq)
    seq[a], seq[b] = seq[b], seq[a]
    return seq


def mutants(e):
    """{name: Conv} of the wrong conventions: (a) taps flipped on every axis, (b) taps exchanged between two axes,
    (c) sampling exchanged between two axes, (d) 3-D: taps and sampling rotated, (e) the flip in the boundary band
    only (the data-term gradient true where R <= i < n - R on every blurred axis, H^T y true everywhere)."""
    D = len(e.shape)
    ft, fc = _flip(e.taps, e.centers)
    out = {"flip": Conv(ft, fc, e.sampling, False)}
    for a, b in itertools.combinations(range(D), 2):
        out[f"taps{a}{b}"] = Conv(_swap(e.taps, a, b), _swap(e.centers, a, b), e.sampling, False)
        if a in e.dirs and b in e.dirs:
            out[f"samp{a}{b}"] = Conv(e.taps, e.centers, tuple(_swap(e.sampling, a, b)), False)
    if D == 3:
        rot = lambda s: list(s[1:]) + list(s[:1])  # noqa: E731
        out["rot"] = Conv(rot(e.taps), rot(e.centers), tuple(rot(e.sampling)), False)
    out["boundary"] = Conv(ft, fc, e.sampling, True)
    return out


def blur_of(e, dt, conv=None):
    conv = true_conv(e) if conv is None else conv
    return dict(arg_shape=e.shape, kernel=kernels(e, dt, conv.taps), center=list(conv.centers), mode="constant")


def grad_kw(e, conv=None):
    conv = true_conv(e) if conv is None else conv
    return dict(arg_shape=e.shape, directions=e.dirs, sampling=tuple(conv.sampling))


def _normal(v, blur):
    t = orc.stencil_apply(v, blur["arg_shape"], blur["kernel"], blur["center"])
    return orc.stencil_adjoint(t, blur["arg_shape"], blur["kernel"], blur["center"])


def grad_f(e, dt, y, conv=None, lam=0.0, mu=1.0):
    """v -> grad of 1/2 ||H v - y||^2 (+ lam env_mu(L21) o Grad) under a convention."""
    conv = true_conv(e) if conv is None else conv
    gk = grad_kw(e, conv)
    if not conv.boundary_only:
        blur = blur_of(e, dt, conv)
        return lambda v: orc.deblur_tv_grad(v, blur, y, lam, mu, gk)
    blur, wrong = blur_of(e, dt), blur_of(e, dt, conv)
    inside = np.ones(e.shape, dtype=bool)
    for a, (n, r) in enumerate(zip(e.shape, reach(e.taps, e.centers))):
        i = np.arange(n).reshape([-1 if b == a else 1 for b in range(len(e.shape))])
        inside &= (i >= r) & (i < n - r)
    band = (~inside).reshape(-1).astype(dt)
    return lambda v: orc.deblur_tv_grad(v, blur, y, lam, mu, gk) + band * (_normal(v, wrong) - _normal(v, blur))


def g_prox(g_kind, dt):
    return {"none": None, "pos": lambda v, t: orc.positive_orthant_prox(v),
            "l1": lambda v, t: orc.l1_prox(v, t * dt(G_L1))}[g_kind]


def oracle_pgd(e, g_kind, dt, conv=None, n=PGD_ITERS, tau=None, snap=None):
    y, x0 = data(e, dt)
    tau = dt(1 / dt(pgd_lipschitz(e))) if tau is None else tau
    x, _ = orc.pgd(x0, grad_f(e, dt, y, conv, PGD_LAM, PGD_MU), g_prox(g_kind, dt), tau, n, snap=snap)
    return x


def oracle_pds(e, algo, h_kind, g_kind, dt, steps, conv=None, n=PDS_ITERS, snap=None):
    """(x, z) after n iterations of PD3O ("pd3o") / Condat-Vu ("cv"); steps = (tau, sigma, rho)."""
    conv = true_conv(e) if conv is None else conv
    y, x0 = data(e, dt)
    gk = grad_kw(e, conv)
    Dd = len(e.dirs)
    K = lambda v: orc.gradient_apply(v, **gk)  # noqa: E731
    KT = lambda v: orc.gradient_adjoint(v, **gk)  # noqa: E731
    if h_kind == "iso":
        hp = lambda v, t: orc.l21_prox(v, t * dt(PDS_LAM), (Dd, *e.shape))  # noqa: E731
    else:
        hp = lambda v, t: orc.l1_prox(v, t * dt(PDS_LAM))  # noqa: E731
    fprox = lambda v, s: orc.fenchel_prox(hp, v, s)  # noqa: E731
    gf = grad_f(e, dt, y, conv)
    tau, sigma, rho = steps
    if algo == "pd3o":
        x, z, _ = orc.pd3o(x0, gf, g_prox(g_kind, dt), K, KT, fprox, tau, sigma, rho, n, snap=snap)
    else:
        x, z = orc.condat_vu(x0, gf, g_prox(g_kind, dt), K, KT, fprox, tau, sigma, rho, n, snap=snap)
    return x, z
