"""
NumPy restatement of the Langevin sampler kernels (csrc/sampler.hip; contracts in include/pyxu_amd.h): the Philox4x32-10
block function, the map from its words to standard normals (evaluated in float64), one ULA / MYULA step in the working
type T with NumPy's non-contracting arithmetic for the five kinds, the Welford update of the centred moments, and the
direct float64 formulas the statistics are compared with.

Shared by test_sampler_refs.py (CPU: the restatement against known answers and the reference's goldens) and
test_gpu_sampler.py.  Arrays handed out by the cached helpers are read-only.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
KINDS = {"none": 0, "l1": 1, "pos": 2, "posl1": 3, "box": 4}  # _dev.PROX_* (0: no g)
TOL = {np.float32: 1e-5, np.float64: 1e-10}  # the project's parity tolerances (test_gpu_parity.py)
CASES = ("ula", "myula_l1", "myula_pos", "myula_posl1", "myula_box", "myula_none")
# Cases whose float32 step the restatement reproduces bit for bit from the reference's own float32 gradient: the
# reference forms x - prox(x), which is exactly min(x, 0) for "pos" and the same expression for "box"; for "l1" and
# "posl1" it cancels (x - (x - t) carries the rounding of x - t) where the kernel's clip / min form is exact.
EXACT_F32 = ("ula", "myula_pos", "myula_box", "myula_none")


def philox4x32_10(ctr, key):
    """counter (4 words, each an int or an array) and key (2 ints) -> 4 uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def normals(dt, seed, step, e0, n):
    """The standard normals of global elements e0 .. e0 + n - 1 of the stream (seed, step) for working type dt, in
    float64: Philox counter (group lo, group hi, step lo, step hi), key (seed lo, seed hi); f32 groups of 4 (words
    (w0, w1) -> elements 0, 1; (w2, w3) -> elements 2, 3, 24-bit uniforms), f64 groups of 2 (53-bit uniforms);
    Box-Muller r cospi(2 u2), r sinpi(2 u2) with r = sqrt(-2 ln u1), u1 in (0, 1]."""
    G = 16 // np.dtype(dt).itemsize
    e = np.uint64(e0) + np.arange(n, dtype=np.uint64)
    grp, j = e // np.uint64(G), (e % np.uint64(G)).astype(np.int64)
    w = philox4x32_10((grp & MASK, grp >> np.uint64(32), int(step) & 0xFFFFFFFF, (int(step) >> 32) & 0xFFFFFFFF),
                      (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    if G == 4:
        pair = j // 2
        wa = np.where(pair == 0, w[0], w[2])
        wb = np.where(pair == 0, w[1], w[3])
        u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0**-24
        u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0**-24
    else:
        u1 = ((((w[0] << np.uint64(32)) | w[1]) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0**-53
        u2 = (((w[2] << np.uint64(32)) | w[3]) >> np.uint64(11)).astype(np.float64) * 2.0**-53
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(j % 2 == 0, r * np.cos(ang), r * np.sin(ang))


def step(dt, kind, x, grad, z, gamma, lam=1.0, pw=0.0):
    """One pxa_langevin_step in T = dt: every operation rounded to T, none contracted (NumPy never contracts)."""
    x, g, z = (np.asarray(v, dtype=dt) for v in (x, grad, z))
    gam = dt(gamma)
    c = dt(math.sqrt(2.0 * float(gam)))
    lamT, t, pwT = dt(lam), dt(float(lam) * float(pw)), dt(pw)
    kind = KINDS.get(kind, kind)
    with np.errstate(invalid="ignore"):
        if kind == 0:
            gt = g
        else:
            if kind == 1:
                m = np.clip(x, -t, t)
            elif kind == 2:
                m = np.minimum(x, dt(0))
            elif kind == 3:
                m = np.minimum(x, t)
            elif kind == 4:
                m = x - np.clip(x, -pwT, pwT)
            else:
                raise ValueError(kind)
            gt = g + m / lamT
        out = (x - gam * gt) + c * z
    assert out.dtype == dt
    return out


def welford(dt, samples, order):
    """pxa_online_moments over samples (K, n): (mean in dt, sums (order - 1, n) float64).  temp, -temp and k temp in dt;
    their powers, the binomial terms and the sums in float64; orders descending."""
    samples = np.asarray(samples, dtype=dt)
    mean = samples[0].copy()
    S = np.zeros((order - 1, samples.shape[1]))
    for k in range(1, samples.shape[0]):
        x = samples[k]
        temp = (x - mean) / dt(k + 1)
        a, b = (-temp).astype(np.float64), (dt(k) * temp).astype(np.float64)
        for r in range(order, 1, -1):
            for s in range(2, r):
                S[r - 2] += (math.comb(r, s) * S[s - 2]) * a ** (r - s)
            S[r - 2] += k * a**r
            S[r - 2] += b**r
        mean = mean * dt(k / (k + 1)) + x / dt(k + 1)
        assert mean.dtype == dt
    return mean, S


def direct_moment(samples, r):
    """mean((x - mu)^r) over the samples, in float64."""
    s = np.asarray(samples, dtype=np.float64)
    return ((s - s.mean(axis=0)) ** r).mean(axis=0)


def direct_standardized(samples, r):
    return direct_moment(samples, r) / direct_moment(samples, 2) ** (r / 2)


def max_norm_err(got, ref):
    """max |got - ref| / max |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def grad_quadratic(A, b, dt):
    """grad of f(x) = 1/2 ||A x - b||^2 per row, in dt."""
    A, b = np.asarray(A, dtype=dt), np.asarray(b, dtype=dt)
    return lambda x: ((x @ A.T) - b) @ A


def run_case(gold, dt, steps, grad0=None):
    """The golden's chain by the restated step with the golden's host generator: the sample after `steps` steps.
    grad0: the gradient to use at x0 instead of the restated one."""
    rng = np.random.default_rng(int(gold["seed"]))
    grad = grad_quadratic(gold["A"], gold["b"], dt)
    x = gold["x0"].astype(dt)
    for k in range(steps):
        z = rng.standard_normal(size=x.shape, dtype=dt)
        g = grad0 if (k == 0 and grad0 is not None) else grad(x)
        x = step(dt, str(gold["kind"]), x, g, z, float(gold["gamma"]), float(gold["lamb"]), float(gold["pw"]))
    return x


def ula_gaussian_variance(n, gamma, steps, seed, normal_of_step):
    """ULA on f = ||x||^2 / 2 (grad f = x) from x0 = 0 in float64: the variance across the n coordinates after `steps`
    steps.  normal_of_step(k): the step's noise."""
    x = np.zeros(n)
    for k in range(steps):
        x = step(np.float64, 0, x, x, normal_of_step(k), gamma)
    return float(x.var())


ULA_N, ULA_GAMMA, ULA_STEPS, ULA_SEED = 2**16, 0.5, 60, 1
ULA_VAR = 1.0 / (1.0 - ULA_GAMMA / 2.0)  # the chain's stationary variance (_sampler.py:225-228): 4/3
ULA_BOUND = 5.0 * ULA_VAR * math.sqrt(2.0 / ULA_N)  # 5 sigma of a sample variance over n independent Gaussians
