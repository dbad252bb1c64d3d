"""
float64 NumPy restatement of the row threshold search (csrc/threshold.hip) and the bounds its results are held to.
Shared by test_threshold_refs.py (CPU: a NumPy model of the kernels' Newton loop, run with their partition, stays
inside the bounds) and test_gpu_threshold.py / test_gpu_ball_solvers.py (the kernels themselves).

Per row, mu* is the root of  h(mu) = a sum_i max(|x_i| - mu, 0) - b mu - c.  With y the magnitudes sorted in
descending order and C_k their cumulative sums, t_k = (a C_k - c) / (a k + b); mu* = t_K at the last k with
y_k > t_k, and 0 when a S <= c (the sort rule; norm.py:198-212 is the instance (2 tau, 1, 0)).

The bounds are derived, not measured.  The kernels form C_K as a float64 sum of K <= n non-negative terms in some
fixed order, |C - C_K| <= (K - 1) 2^-53 C_K to first order, and the rule's product, difference and quotient are the
same float64 operations in the same order as the restatement's (the kernels do not contract them), so that

    |mu - mu*| <= n 2^-53 (a C_K + |c|) / (a K + b)                                     (mu_bound)

(for K = 1 and K = 2 the sum is a single correctly rounded addition on both sides and the two agree bit for bit).
An output element adds one rounding to T of a value no larger than max(|x_i|, mu*):

    mu_bound + eps(T) max(|x_i|, mu*)                                                   (out_bound).

Every parity case first asserts, on the reference alone, that no magnitude lies within 10 x mu_bound of mu*
(`gap_ratio` >= 10): the active set is then determined, and a wrong count cannot hide inside the tolerance.
"""
import math

import numpy as np

import _prim_refs as R

F64 = np.float64
CLAMP, SOFT = 0, 1
RESIDENT_MAX = {np.float32: 32768, np.float64: 16384}  # include/pyxu_amd.h: pxa_row_threshold_resident_max

# n: vector tail only (1, 2, 5), one workgroup (1027), the resident limit and the first streaming row (per dtype, see
# shapes()), few blocks per row (70001), many (2^20 + 3)
N_COMMON = (1, 2, 5, 1027, 70001, 2**20 + 3)
N_CPU = (1, 2, 5, 1027, 32768, 32769, 70001, 2**20 + 3)
COEFS = ("l1_30", "l1_90", "sq_0.1", "sq_10")


def shapes(dt):
    lim = RESIDENT_MAX[dt]
    return tuple(sorted(set(N_COMMON) | {lim, lim + 1}))


def coef(name, S):
    """(a, b, c) of a named coefficient set; S = ||x||_1 of the (first) row."""
    return {"l1_30": (1.0, 0.0, 0.3 * S), "l1_90": (1.0, 0.0, 0.9 * S), "sq_0.1": (0.1, 1.0, 0.0),
            "sq_10": (10.0, 1.0, 0.0)}[name]


def l1(x):
    return float(np.abs(np.asarray(x, dtype=F64)).sum())


# ----------------------------------------------------------------------------- the sort rule
def sort_rule(x, a, b, c):
    """(mu*, K, C_K) of one row x (any float dtype), in float64; C_K correctly rounded (math.fsum)."""
    y = np.sort(np.abs(np.asarray(x, dtype=F64)))[::-1]
    if y.size == 0 or a * math.fsum(y) <= c:
        return 0.0, 0, 0.0
    C = np.cumsum(y)
    k = np.arange(1, y.size + 1, dtype=F64)
    t = (a * C - c) / (a * k + b)
    K = int(np.flatnonzero(y > t).max()) + 1
    CK = math.fsum(y[:K])
    return (a * CK - c) / (a * K + b), K, CK


def mu_bound(n, a, b, c, K, CK):
    if K == 0:
        return 0.0
    return n * 2.0**-53 * (a * CK + abs(c)) / (a * K + b)


def gap_ratio(x, mu, bound):
    """min_i | |x_i| - mu* | / bound (inf when the bound is 0)."""
    gap = float(np.abs(np.abs(np.asarray(x, dtype=F64)) - mu).min())
    return math.inf if bound == 0.0 else gap / bound


def shrink_ref(x, mu, mode):
    X = np.asarray(x, dtype=F64)
    m = np.abs(X)
    return np.sign(X) * (np.minimum(m, mu) if mode == CLAMP else np.maximum(m - mu, 0.0))


def out_bound(x, mu, bound):
    return bound + R.eps(x.dtype.type) * np.maximum(np.abs(np.asarray(x, dtype=F64)), mu)


def sort_rule_rows(x2, a, b, c):
    """sort_rule for every row of a short-row array at once; the cumulative sums run in extended precision and are
    rounded once, which for a handful of terms is math.fsum's result."""
    y = -np.sort(-np.abs(x2.astype(np.longdouble)), axis=1)
    C = np.cumsum(y, axis=1).astype(F64)
    y = y.astype(F64)
    k = np.arange(1, x2.shape[1] + 1, dtype=F64)
    t = (a * C - c) / (a * k + b)
    K = x2.shape[1] - np.argmax((y > t)[:, ::-1], axis=1)
    inside = a * C[:, -1] <= c
    rows = np.arange(x2.shape[0])
    K = np.where(inside, 0, K)
    CK = np.where(inside, 0.0, C[rows, np.maximum(K, 1) - 1])
    mu = np.where(inside, 0.0, (a * CK - c) / (a * np.maximum(K, 1) + b))
    return list(zip(mu.tolist(), K.tolist(), CK.tolist()))


class Ref:
    """The reference of one (rows, n) case with scalar coefficients: per-row mu*, K, bound; gap precondition asserted."""

    def __init__(self, x2, a, b, c, min_ratio=10.0):
        self.x2, self.abc = x2, (a, b, c)
        n = x2.shape[1]
        rr = sort_rule_rows(x2, a, b, c) if (x2.shape[0] > 1000 and n <= 16) else [sort_rule(r, a, b, c) for r in x2]
        self.mu = np.array([r[0] for r in rr])
        self.K = np.array([r[1] for r in rr])
        self.bound = np.array([mu_bound(n, a, b, c, r[1], r[2]) for r in rr])
        gap = np.abs(np.abs(x2.astype(F64)) - self.mu[:, None]).min(axis=1) if x2.size else np.zeros(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(self.bound > 0, gap / self.bound, math.inf)
        self.ratio = float(ratio.min()) if ratio.size else math.inf
        assert self.ratio >= min_ratio, ("gap precondition", x2.shape, self.abc, self.ratio)

    def check_mu(self, mu, passes=None, tag=""):
        err = np.abs(np.asarray(mu, dtype=F64) - self.mu)
        assert (err <= self.bound).all(), (tag, "mu", float((err / np.maximum(self.bound, 1e-300)).max()))
        if passes is not None:
            assert (np.asarray(passes) >= 1).all() and (np.asarray(passes) <= self.x2.shape[1] + 2).all(), (tag, "passes")

    def check_out(self, got, mode, tag=""):
        assert got.dtype == self.x2.dtype and got.shape == self.x2.shape, (tag, got.dtype, got.shape)
        X, mu = self.x2.astype(F64), self.mu[:, None]
        ref = shrink_ref(X, mu, mode)
        err = np.abs(got.astype(F64) - ref)
        bd = self.bound[:, None] + R.eps(self.x2.dtype.type) * np.maximum(np.abs(X), mu)
        assert (err <= bd).all(), (tag, "out", float((err / np.maximum(bd, 1e-300)).max()))
        if mode == SOFT:  # the support is exactly the reference's
            np.testing.assert_array_equal(got == 0, ref == 0, err_msg=f"{tag} support")
        else:  # so is the clamped set: every other element is x itself
            free = np.abs(X) <= mu
            np.testing.assert_array_equal(got[free], self.x2[free], err_msg=f"{tag} unclamped set")


# ----------------------------------------------------------------------------- NumPy model of the kernels' loop
def _tree64(v):
    """Lane 0 of the shuffle-down tree over the last axis (64 lanes)."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _dpp64(v):
    """wave_sum_f64 (csrc/common.hpp) over the last axis: quad butterflies, row rotations by 4 and 8, then the four
    row sums in ascending order."""
    q = v.reshape(*v.shape[:-1], 4, 4, 4)  # (row, quad, lane)
    Q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    r = (Q[..., 0] + Q[..., 3]) + (Q[..., 2] + Q[..., 1])
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def _seq(v, axis):
    """Sequential (left to right) float64 sum along `axis`."""
    v = np.moveaxis(v, axis, 0)
    acc = np.zeros(v.shape[1:], dtype=F64)
    for s in v:
        acc = acc + s
    return acc


def resident_geometry(n, dt):
    V = R.vec_n(dt)
    nv = -(-n // V)
    for lim, th, vpt in ((256, 256, 1), (512, 256, 2), (1024, 256, 4), (2048, 256, 8), (4096, 512, 8), (8192, 1024, 8)):
        if nv <= lim:
            return th, vpt, V
    raise ValueError(n)


def resident_sum(m, dt):
    """Sum of the float64 terms m (n,) in the resident kernel's order."""
    th, vpt, V = resident_geometry(m.size, dt)
    p = np.zeros(th * vpt * V, dtype=F64)
    p[:m.size] = m
    per_thread = _seq(p.reshape(vpt, th, V).transpose(1, 0, 2).reshape(th, vpt * V), 1)
    return float(_seq(_dpp64(per_thread.reshape(th // 64, 64)), 0))


def stream_sum(m, rows):
    """Sum of m (n,) in the streaming path's order: pxa_row_reduce's partition, then the one-wavefront fold."""
    n = m.size
    nb = R.blocks_per_row(rows, n)
    chunk = -(-n // nb)
    it = -(-chunk // R.K_BLOCK)
    p = np.zeros((nb, it * R.K_BLOCK), dtype=F64)
    flat = np.zeros(nb * chunk, dtype=F64)
    flat[:n] = m
    p[:, :chunk] = flat.reshape(nb, chunk)
    per_thread = _seq(p.reshape(nb, it, R.K_BLOCK), 1)  # (nb, 256)
    part = _seq(_tree64(per_thread.reshape(nb, R.K_BLOCK // 64, 64)), 1)  # (nb,)
    it2 = -(-nb // 64)
    q = np.zeros(it2 * 64, dtype=F64)
    q[:nb] = part
    return float(_tree64(_seq(q.reshape(it2, 64), 0)))


def newton_model(x, a, b, c, rows=1):
    """(mu, passes, k) of the kernels' loop on one row x of dtype T, every operation a float64 NumPy operation in the
    kernels' order (the rule's products and sums are not contracted on the device either)."""
    dt = x.dtype.type
    m = np.abs(x.astype(F64))
    n = m.size
    sumf = (lambda t: resident_sum(t, dt)) if n <= RESIDENT_MAX[dt] else (lambda t: stream_sum(t, rows))
    a, b, c = F64(a), F64(b), F64(c)
    S = F64(sumf(m))
    if not np.isfinite(S):
        return math.nan, 1, n
    if a * S - c <= 0:
        return 0.0, 1, n
    mu = max(F64(0), (a * S - c) / (a * F64(n) + b))
    k_prev, passes = n, 1
    for _ in range(n + 1):
        act = m > mu
        k = int(act.sum())
        C = F64(sumf(np.where(act, m, 0.0)))
        passes += 1
        if k >= k_prev or k == 0:
            break
        mu = (a * C - c) / (a * F64(k) + b)
        k_prev = k
    return float(mu), passes, k_prev if k >= k_prev else k


# ----------------------------------------------------------------------------- inputs
def rows_input(rows, n, dt):
    """(rows, n) of log-uniform magnitudes in [1e-2, 1e2] with random signs: row r is _prim_refs.values(n, dt, r)."""
    return np.stack([R.values(n, dt, key=r) for r in range(rows)]) if rows else np.zeros((0, n), dtype=dt)


def tie_row(n, dt):
    """Integers 1..3 with random signs: many equal magnitudes."""
    r = R.rng_for("ties", n, np.dtype(dt).name)
    return (r.integers(1, 4, n) * r.choice([-1.0, 1.0], n)).astype(dt)


# ----------------------------------------------------------------------------- float64 solver loops (solver tests)
def project_l1(x, r):
    mu, _, _ = sort_rule(x, 1.0, 0.0, r)
    return shrink_ref(x, mu, SOFT)


def prox_sql1(x, tau):
    mu, _, _ = sort_rule(x, 2.0 * tau, 1.0, 0.0)
    return shrink_ref(x, mu, SOFT)


def prox_linf(x, tau):
    mu, K, _ = sort_rule(x, 1.0, 0.0, tau)
    return np.zeros_like(np.asarray(x, dtype=F64)) if K == 0 else shrink_ref(x, mu, CLAMP)
