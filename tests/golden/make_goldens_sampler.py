"""
Generate the sampler golden results by running the upstream Pyxu reference's own ULA / MYULA and online statistics
(NumPy code path).

Run in the build container only (needs the reference snapshot, see oracle/refshim/boot.py):

    python tests/golden/make_goldens_sampler.py

Writes ``tests/golden/sampler_<case>.npz`` and ``tests/golden/sampler_stats.npz``.  Nothing from the reference is
copied: only data.

Chains (rng = default_rng(seed), draws in the stated order): A = standard_normal((24, 17)) / sqrt(24),
b = standard_normal(24), x0 = standard_normal((2, 17)); f = 1/2 ||A x - b||^2 as
0.5 * SquaredL2Norm(24).asloss(b) * LinOp.from_array(A).  "ula": ULA(f, gamma); "myula_<kind>": MYULA(f, g, gamma,
lamb) with g: "l1" pw L1Norm, "pos" PositiveOrthant, "posl1" pw PositiveL1Norm, "box" LInfinityBall(pw), "none" None.
Recorded: the inputs, the sample after 1 and after 6 steps of the reference's float64 and float32 runs with
samples(rng=default_rng(seed), x0=x0), and the reference's gradient of f at x0 in both precisions.

Statistics: K = 40 samples of n = 37, gamma(2, 1) + 3 (skewed, non-zero mean), rounded to float32 so that the float64
and float32 runs see the same numbers.  Recorded after the last update: the reference's OnlineMoment(1),
OnlineMoment(2), OnlineVariance, OnlineStd, OnlineCenteredMoment(3) and (4), OnlineSkewness and OnlineKurtosis in both
precisions, and the direct float64 formulas mean((x - mu)^r) for r = 2, 3, 4.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle", "refshim"))
import boot  # noqa: E402,F401  (makes the reference importable)

warnings.simplefilter("ignore")

import pyxu.abc as pxa  # noqa: E402
import pyxu.experimental.sampler as pxes  # noqa: E402
import pyxu.operator as pxo  # noqa: E402
import pyxu.runtime as pxrt  # noqa: E402

ROWS, N, M = 2, 17, 24
GAMMA, LAMB = 0.1, 0.25
# (case, g kind, pw, seed): the cases of tests/_sampler_refs.py
CASES = [
    ("ula", "none", 0.0, 3),
    ("myula_l1", "l1", 0.6, 5),
    ("myula_pos", "pos", 0.0, 7),
    ("myula_posl1", "posl1", 0.6, 11),
    ("myula_box", "box", 0.4, 13),
    ("myula_none", "none", 0.0, 17),
]
K, NS = 40, 37


def inputs(seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N)) / np.sqrt(M)
    b = rng.standard_normal(M)
    return dict(A=A, b=b, x0=rng.standard_normal((ROWS, N)))


def g_of(kind, pw):
    if kind == "l1":
        return pw * pxo.L1Norm(N)
    if kind == "pos":
        return pxo.PositiveOrthant(N)
    if kind == "posl1":
        return pw * pxo.PositiveL1Norm(N)
    if kind == "box":
        return pxo.LInfinityBall(N, radius=pw)
    return None


def run_chain(case, data, kind, pw, seed, width):
    dt = width.value
    with pxrt.Precision(width):
        f = 0.5 * pxo.SquaredL2Norm(M).asloss(data["b"].astype(dt)) * pxa.LinOp.from_array(data["A"].astype(dt))
        x0 = data["x0"].astype(dt)
        s = pxes.ULA(f, gamma=GAMMA) if case == "ula" else pxes.MYULA(f, g_of(kind, pw), gamma=GAMMA, lamb=LAMB)
        grad0 = np.array(f.grad(x0))
        gen = s.samples(rng=np.random.default_rng(seed), x0=x0)
        xs = [np.array(next(gen)) for _ in range(6)]
    assert all(x.dtype == dt and x.shape == (ROWS, N) for x in xs) and grad0.dtype == dt
    return xs[0], xs[5], grad0


def run_stats(samples, width):
    dt = width.value
    stats = dict(m1=pxes.OnlineMoment(1), m2=pxes.OnlineMoment(2), var=pxes.OnlineVariance(), std=pxes.OnlineStd(),
                 cm3=pxes.OnlineCenteredMoment(3), cm4=pxes.OnlineCenteredMoment(4), skew=pxes.OnlineSkewness(),
                 kurt=pxes.OnlineKurtosis())
    out = {}
    with pxrt.Precision(width):
        for name, st in stats.items():
            for x in samples.astype(dt):
                val = st.update(x.copy())
            out[name] = np.array(val)
    return out


def main():
    for case, kind, pw, seed in CASES:
        data = inputs(seed)
        x1, x6, g0 = run_chain(case, data, kind, pw, seed, pxrt.Width.DOUBLE)
        x1_32, x6_32, g0_32 = run_chain(case, data, kind, pw, seed, pxrt.Width.SINGLE)
        out = dict(data, kind=kind, pw=pw, seed=seed, gamma=GAMMA, lamb=LAMB, x1=x1, x6=x6, grad0=g0, x1_f32=x1_32,
                   x6_f32=x6_32, grad0_f32=g0_32)
        path = os.path.join(HERE, f"sampler_{case}.npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} B)")
    rng = np.random.default_rng(23)
    samples = (rng.gamma(2.0, 1.0, (K, NS)) + 3.0).astype(np.float32).astype(np.float64)
    out = dict(samples=samples)
    out.update(run_stats(samples, pxrt.Width.DOUBLE))
    out.update({f"{k}_f32": v for k, v in run_stats(samples, pxrt.Width.SINGLE).items()})
    s = samples - samples.mean(axis=0)
    out.update(direct_var=(s**2).mean(axis=0), direct_cm3=(s**3).mean(axis=0), direct_cm4=(s**4).mean(axis=0))
    path = os.path.join(HERE, "sampler_stats.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
