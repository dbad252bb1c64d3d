"""
float64 NumPy restatements of the element-wise, reduction and array primitives (csrc/elementwise.hip, reduce.hip,
array.hip) and the error bound each one is held to.  Shared by test_prim_refs.py (CPU: the kernels' stated operation
order, emulated in NumPy with dtype T, stays inside the bounds) and test_gpu_prims_*.py (the kernels themselves).

The bounds are derived, not measured.  eps = np.finfo(T).eps, unit round-off u = eps / 2.

* Single-rounding operations (mul, div, add_scalar, fill, clip, cast, where, copies, unary / binary maps other
  than power): bit-equal to NumPy in dtype T.  No fast-math flag is set, so fp32 divide and sqrt are correctly
  rounded.  BIN_POW: OP_TOL relative.
* Multiply-add chains (axpby, axpby_bcast, axpy_rows, lincomb3, extrapolate, prox_l1, fenchel_prox_l1,
  moreau_grad_l1): |got - ref64| <= 8 eps S, S the float64 sum of the absolute values of the terms being added.
  At most 4 rounded operations, each at most u relative to a quantity <= S: 2 eps S to first order; the factor 8
  leaves 4x headroom for either fma-contraction choice of the compiler.
* L21 family, group <= 4: |got - ref64| <= 8 eps |v| per element (x scale / mu for the Moreau gradient), 8 eps n for
  the group norm.  The norm carries at most (G + 1) / 2 + 1 roundings; f = 1 - tau / max(n, tau) has absolute error
  <= (G + 3) u because tau / max <= 1; one or two more roundings form the output.  The clamped set (f == 0) must
  equal the reference's for every group whose float64 n / tau lies outside [1 - 16 eps, 1 + 16 eps].
* Reductions accumulate in float64: MAXABS, MIN, MAX, NEGCNT and the p = 0 count are exact; the sums obey the
  classical bound |got - ref| <= n 2^-53 sum |t_i| for any summation order, + OP_TOL[float64] relative for the
  device pow when p is not in {0, 1, 2}.

Inputs keep magnitudes inside [1e-6, 1e6] so that no intermediate is subnormal.
"""
import math

import numpy as np

F64 = np.float64
OP_TOL = {np.float32: 1e-5, np.float64: 1e-12}  # the project's operator tolerance (test_gpu_parity.py)
CHAIN_FACTOR = 8.0
L21_FACTOR = 8.0
BAND = 16.0  # tie band of the L21 clamp, in eps

# launch geometry of the streaming kernels (csrc/common.hpp)
K_BLOCK = 256
K_MAX_GRID = 256 * 8
N_WRAP = 2**21 + 1027  # > K_MAX_GRID * K_BLOCK 16-byte vectors in both dtypes, 3-element fp32 tail


def eps(dt):
    return float(np.finfo(dt).eps)


def vec_n(dt):
    return 16 // np.dtype(dt).itemsize


def T(dt, v):
    """The (T)v cast the C-ABI applies to its double scalars, as a Python float."""
    return float(np.asarray(v, dtype=dt))


def rng_for(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------- device placement (GPU tests only)
GUARD = 777.0


def _host_tensor(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy())  # cached inputs are read-only


def to_dev(a):
    return _host_tensor(a).cuda()


def to_host(t):
    return t.cpu().numpy()


def placed(a, off=0, pad=5):
    """(base, view): `a` copied into base[off:off + a.size] of a fresh 1-D device buffer filled with GUARD.  off = 0
    is 16-byte aligned; off = 1 is a contiguous view that starts one element into the allocation (the kernels'
    scalar path)."""
    import torch

    flat = _host_tensor(a).reshape(-1)
    base = torch.full((off + flat.numel() + pad,), GUARD, dtype=flat.dtype, device="cuda")
    view = base[off:off + flat.numel()]
    view.copy_(flat)
    assert view.is_contiguous() and view.data_ptr() % 16 == (off * flat.element_size()) % 16
    return base, view


def guards_intact(base, off, n):
    """The elements of `base` outside [off, off + n) still hold GUARD."""
    h = to_host(base)
    return bool((h[:off] == GUARD).all() and (h[off + n:] == GUARD).all())


# ----------------------------------------------------------------------------- generators
def values(n, dt, key=0):
    """Random signs, magnitudes log-uniform in [1e-2, 1e2]."""
    r = rng_for("values", n, np.dtype(dt).name, key)
    m = 10.0 ** r.uniform(-2.0, 2.0, n)
    return (m * r.choice([-1.0, 1.0], n)).astype(dt)


def sum_values(shape, dt, key=0):
    """Random signs, magnitudes in [0.5, 1.5]: one dropped or doubled element of a sum moves it by >= 0.125
    (>= 0.25 for every statistic but sum |x|^3)."""
    r = rng_for("sum", tuple(shape), np.dtype(dt).name, key)
    return (r.uniform(0.5, 1.5, shape) * r.choice([-1.0, 1.0], shape)).astype(dt)


def sum_values_pair(shape, dt):
    """(x, y) for the two-operand statistics: y has the opposite sign of x, so that |x - y| >= 1 and |x y| >= 0.25."""
    x = sum_values(shape, dt, 0)
    r = rng_for("sum_y", tuple(shape), np.dtype(dt).name)
    y = (-np.sign(x) * r.uniform(0.5, 1.5, shape)).astype(dt)
    return x, y


def l21_values(outer, group, inner, dt, key=0):
    """(outer, group, inner) array whose group norms straddle 1 (about half of them below)."""
    r = rng_for("l21", outer, group, inner, np.dtype(dt).name, key)
    x = r.standard_normal((outer, group, inner)) * (1.2 / math.sqrt(group))
    x = np.where(np.abs(x) < 1e-3, 1e-3, x)
    return x.astype(dt)


# ----------------------------------------------------------------------------- multiply-add chains
def _soft(x, tau):
    return np.sign(x) * np.maximum(np.abs(x) - tau, 0.0)


def fenchel_t(dt, sigma, lam):
    """t = (1 / sigma) * lam computed in T, as pxa_fenchel_prox_l1 / _l21 do on the host."""
    return float((dt(1) / dt(sigma)) * dt(lam))


# name -> (number of array inputs, scalar parameters); the scalars are not representable in fp32 on purpose
CHAINS = {
    "scale": (1, (0.7,)),
    "axpby": (2, (0.7, -1.3)),
    "lincomb3": (3, (0.7, -1.3, 2.1)),
    "extrapolate": (2, (0.9,)),
    "prox_l1": (1, (0.3,)),
    "fenchel_prox_l1": (1, (0.7, 0.3)),
    "moreau_grad_l1": (1, (0.3, 1.7)),
}


def chain_ref(name, dt, xs, p):
    """(ref64, S64) of a chain on arrays xs (dtype T) with double scalars p."""
    X = [a.astype(F64) for a in xs]
    if name == "scale":
        a = T(dt, p[0])
        return a * X[0], np.abs(a * X[0])
    if name == "axpby":
        a, b = T(dt, p[0]), T(dt, p[1])
        return a * X[0] + b * X[1], np.abs(a * X[0]) + np.abs(b * X[1])
    if name == "lincomb3":
        a, b, c = (T(dt, v) for v in p)
        return a * X[0] + b * X[1] + c * X[2], np.abs(a * X[0]) + np.abs(b * X[1]) + np.abs(c * X[2])
    if name == "extrapolate":
        a = T(dt, p[0])
        return (X[0] - X[1]) * a + X[0], np.abs((X[0] - X[1]) * a) + np.abs(X[0])
    if name == "prox_l1":
        return _soft(X[0], T(dt, p[0])), np.abs(X[0])
    if name == "fenchel_prox_l1":
        s, t = T(dt, p[0]), fenchel_t(dt, p[0], p[1])
        return X[0] - s * _soft(X[0] / s, t), np.abs(X[0])
    if name == "moreau_grad_l1":
        mu, sc = T(dt, p[0]), T(dt, p[1])
        return (X[0] - _soft(X[0], mu)) / mu * sc, np.abs(X[0]) * abs(sc / mu)
    raise KeyError(name)


def chain_bound(dt, S):
    return CHAIN_FACTOR * eps(dt) * S


def _fma(dt, a, b, c):
    """a * b + c with one rounding (fp32: through float64; fp64: through the platform's long double)."""
    wide = F64 if np.dtype(dt) == np.float32 else np.longdouble
    return (np.asarray(a, dtype=wide) * np.asarray(b, dtype=wide) + np.asarray(c, dtype=wide)).astype(dt)


def _soft_T(dt, x, tau):
    m = np.abs(x) - dt(tau)
    m = np.where(m > 0, m, dt(0))
    return (m * np.sign(x)).astype(dt)


def chain_emulate(name, dt, xs, p, fused):
    """The functor's stated operation order (csrc/elementwise.hip) in NumPy with dtype T; `fused`: every
    multiply-add contracted, else none."""
    x = xs[0]
    mad = (lambda a, b, c: _fma(dt, a, b, c)) if fused else (lambda a, b, c: (a * b).astype(dt) + c)
    if name == "scale":
        return dt(p[0]) * x
    if name == "axpby":
        return mad(dt(p[1]), xs[1], dt(p[0]) * x)
    if name == "lincomb3":
        return mad(dt(p[2]), xs[2], mad(dt(p[1]), xs[1], dt(p[0]) * x))
    if name == "extrapolate":
        return mad(x - xs[1], dt(p[0]), x)
    if name == "prox_l1":
        return _soft_T(dt, x, p[0])
    if name == "fenchel_prox_l1":
        s, t = dt(p[0]), dt(fenchel_t(dt, p[0], p[1]))
        return mad(_soft_T(dt, x / s, t), -s, x)
    if name == "moreau_grad_l1":
        r = x - _soft_T(dt, x, p[0])
        return (r / dt(p[0])) * dt(p[1])
    raise KeyError(name)


def axpy_rows_ref(dt, c, s, x, y):
    """out[r] = y[r] + (s c[r]) x[r]: (ref64, S64); the coefficient s c[r] is itself rounded to T."""
    a = (T(dt, s) * c.astype(F64))[:, None]
    X, Y = x.astype(F64), y.astype(F64)
    return a * X + Y, np.abs(a * X) + np.abs(Y)


def axpy_rows_emulate(dt, c, s, x, y, fused):
    a = (dt(s) * c)[:, None].astype(dt)
    return _fma(dt, a, x, y) if fused else (a * x).astype(dt) + y


def bcast_ref(dt, a, x, b, y):
    a, b = T(dt, a), T(dt, b)
    X, Y = x.astype(F64), np.tile(y.astype(F64), x.size // y.size)
    return a * X + b * Y, np.abs(a * X) + np.abs(b * Y)


# single-rounding maps: NumPy in dtype T, compared bit for bit
def exact_ref(name, dt, xs, p):
    x = xs[0]
    with np.errstate(all="ignore"):
        if name == "mul":
            return x * xs[1]
        if name == "div":
            return x / dt(p[0])
        if name == "add_scalar":
            return x + dt(p[0])
        if name == "fill":
            return np.full(x.shape, dt(p[0]), dtype=dt)
        if name == "clip":  # p = (lo, hi or None); NaN stays NaN
            r = np.maximum(x, dt(p[0]))
            return r if p[1] is None else np.minimum(r, dt(p[1]))
    raise KeyError(name)


# ----------------------------------------------------------------------------- L21 family
L21_MODES = ("prox", "fenchel", "moreau", "norm")
L21_PARAMS = {"prox": (1.0,), "fenchel": (0.8, 0.7), "moreau": (1.0, 1.7), "norm": ()}


def l21_ref(mode, dt, x, p):
    """x: (outer, group, inner) of dtype T.  Returns dict(ref, bound, clamp, band): float64 reference, element-wise
    bound, the reference's clamped groups (n <= tau: f == 0) and the groups inside the tie band, both
    (outer, 1, inner)."""
    X = x.astype(F64)
    e = eps(dt)
    if mode == "fenchel":
        s, tau = T(dt, p[0]), fenchel_t(dt, p[0], p[1])
        W = X / s
    else:
        s, tau = 1.0, (T(dt, p[0]) if mode != "norm" else 1.0)
        W = X
    n = np.sqrt((W * W).sum(axis=1, keepdims=True))
    if mode == "norm":
        return dict(ref=n[:, 0, :], bound=L21_FACTOR * e * n[:, 0, :], clamp=None, band=None)
    f = 1.0 - tau / np.maximum(n, tau)
    band = np.abs(n / tau - 1.0) <= BAND * e
    if mode == "prox":
        ref, sc = X * f, 1.0
    elif mode == "fenchel":
        ref, sc = X - s * (W * f), 1.0
    else:
        mu, scale = T(dt, p[0]), T(dt, p[1])
        ref, sc = (X - X * f) / mu * scale, abs(scale / mu)
    return dict(ref=ref, bound=L21_FACTOR * e * np.abs(X) * sc, clamp=n <= tau, band=band)


def l21_emulate(mode, dt, x, p):
    """group_kernel's operation order in NumPy with dtype T (no contraction)."""
    G = x.shape[1]
    if mode == "fenchel":
        p0, tau = dt(p[0]), dt(fenchel_t(dt, p[0], p[1]))
    elif mode == "norm":
        p0, tau = dt(0), dt(0)
    else:
        p0, tau = dt(p[0]), dt(p[0])
    s = np.zeros((x.shape[0], x.shape[2]), dtype=dt)
    for g in range(G):
        v = x[:, g, :] / p0 if mode == "fenchel" else x[:, g, :]
        s = s + (v * v).astype(dt)
    n = np.sqrt(s).astype(dt)
    if mode == "norm":
        return n
    f = (dt(1) - tau / np.where(n > tau, n, tau)).astype(dt)[:, None, :]
    if mode == "prox":
        return x * f
    if mode == "fenchel":
        return ((x / p0) * f).astype(dt) * (-p0) + x
    return ((x - x * f) / p0) * dt(p[1])


def l21_check(mode, dt, x, got, p, tag=""):
    """The assertions every L21 result is held to; `got` has x's shape ((outer, inner) for the norm)."""
    r = l21_ref(mode, dt, x, p)
    err = np.abs(got.astype(F64) - r["ref"])
    bad = err > r["bound"]
    assert not bad.any(), (tag, mode, int(bad.sum()), float((err / np.maximum(r["bound"], 1e-300)).max()))
    if mode == "norm":
        return 0.0
    share = float(r["band"].mean())
    assert share <= 0.01, (tag, mode, share)  # the test may not skip its way to passing
    ok = np.broadcast_to(~r["band"], x.shape)
    clamp = np.broadcast_to(r["clamp"], x.shape)
    if mode == "prox":  # zero set
        np.testing.assert_array_equal((got == 0)[ok], (clamp | (x == 0))[ok], err_msg=f"{tag} zero set")
    elif mode == "fenchel":  # f == 0: out = x - sigma * 0 = x exactly
        sel = ok & clamp
        np.testing.assert_array_equal(got[sel], x[sel], err_msg=f"{tag} clamped set")
    return share


# ----------------------------------------------------------------------------- reductions
RED = dict(SUMSQ=0, DIFFSQ=1, DOT=2, ABS=3, MAXABS=4, SUM=5, NEGCNT=6, MIN=7, MAX=8)
RED_NEEDS_Y = ("DIFFSQ", "DOT")
RED_SUMS = ("SUMSQ", "DIFFSQ", "DOT", "ABS", "SUM")


def red_terms(op, x, y=None):
    X = x.astype(F64)
    Y = y.astype(F64) if y is not None else None
    if op == "SUMSQ":
        return X * X
    if op == "DIFFSQ":
        return (X - Y) ** 2
    if op == "DOT":
        return X * Y
    if op == "ABS":
        return np.abs(X)
    if op == "SUM":
        return X
    raise KeyError(op)


def sum_ref(t, n_terms, extra_rel=0.0):
    """(ref, bound, delta) per row of float64 terms t (rows, n): float64 sum, n 2^-53 sum |t| (+ extra_rel sum |t|),
    and the smallest |term| (what one dropped or doubled element moves the sum by)."""
    if t.shape[-1] == 0:
        z = np.zeros(t.shape[:-1])
        return z, z, np.full(t.shape[:-1], np.inf)
    a = np.abs(t)
    sa = a.sum(axis=-1)
    if t.shape[-1] <= 4096 and t.size <= 2**20:
        # correctly rounded: the bound is (n - 1) 2^-53 sum |t| for the kernel's additions + 2^-53 |ref| for this one
        ref = np.array([math.fsum(r) for r in t.reshape(-1, t.shape[-1])]).reshape(t.shape[:-1])
    else:
        # long rows: NumPy's pairwise float64 sum, whose own error (~log2(n) 2^-53 sum |t|) is far below n 2^-53
        ref = t.sum(axis=-1)
    return ref, (n_terms * 2.0**-53 + extra_rel) * sa, a.min(axis=-1)


def red_ref(op, x, y=None):
    """(ref, bound, delta) of pxa_row_reduce `op` over the last axis; bound 0 = exact equality."""
    with np.errstate(invalid="ignore"):
        if op in RED_SUMS:
            return sum_ref(red_terms(op, x, y), x.shape[-1])
        z = np.zeros(x.shape[:-1])
        X = x.astype(F64)
        if x.shape[-1] == 0:
            return z, z, None
        if op == "MAXABS":
            return np.abs(X).max(axis=-1), z, None
        if op == "MIN":
            return X.min(axis=-1), z, None
        if op == "MAX":
            return X.max(axis=-1), z, None
        if op == "NEGCNT":
            return (X < 0).sum(axis=-1).astype(F64), z, None
    raise KeyError(op)


def pow_ref(p, x, y=None):
    """(ref, bound, delta) of pxa_row_reduce_pow: sum |x - y|^p, or the count of non-zeros (NaN included) for p = 0."""
    with np.errstate(invalid="ignore"):
        d = np.abs(x.astype(F64) - (y.astype(F64) if y is not None else 0.0))
        if p == 0:
            z = np.zeros(x.shape[:-1])
            return (d != 0).sum(axis=-1).astype(F64), z, None
        return sum_ref(d**p, x.shape[-1], 0.0 if p in (1, 2) else OP_TOL[np.float64])


def blocks_per_row(rows, n):
    """reduce.hip's partition (documented there): only used to name the paths the shapes below take."""
    per = (n + 4095) // 4096
    cap = max((4096 + rows - 1) // rows, 1) if rows > 0 else 1
    return max(min(per, cap, 1024), 1)


# (rows, n) -> which dtypes; the paths: nb = 1, 2, 4 (3 rows), 65 (strided final loop), 1024, cap-limited 2, two slabs
RED_SHAPES = [
    ((1, 1), "both"), ((1, 63), "both"), ((1, 257), "both"), ((5, 4096), "both"), ((1, 4097), "both"),
    ((3, 12293), "both"), ((1, 262145), "both"), ((1, 4 * 2**20 + 5), "f32"), ((2048, 8193), "f32_few"),
    ((65538, 3), "both"),
]
