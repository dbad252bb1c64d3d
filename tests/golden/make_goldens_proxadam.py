"""
Generate the ProxAdam golden results by running the upstream Pyxu reference's own ProxAdam (NumPy code path).

Run in the build container only (needs the reference snapshot, see oracle/refshim/boot.py):

    python tests/golden/make_goldens_proxadam.py

Writes ``tests/golden/proxadam_<case>.npz``: the inputs and parameters, the final ``x`` of the reference's float64 run
and of its float32 run after ``MaxIter(6)``.  Nothing from the reference is copied: only data.

Objective (rng = default_rng(seed), draws in the stated order): A = standard_normal((24, 17)) / sqrt(24),
b = standard_normal(24), x0 = standard_normal((3, 17)), v0 = uniform(0.5, 2, (3, 17));
f = SquaredL2Norm(24).asloss(b) * LinOp.from_array(A).  g: "l1" lam L1Norm, "pos" PositiveOrthant, "posl1"
lam PositiveL1Norm, "box" LInfinityBall(radius), "none".  v0 is passed to fit() only where use_v0 is set.
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
import pyxu.operator as pxo  # noqa: E402
import pyxu.opt.solver as pxs  # noqa: E402
import pyxu.opt.stop as pxst  # noqa: E402
import pyxu.runtime as pxrt  # noqa: E402

ITERS, ROWS, N, M = 6, 3, 17, 24
# (case, variant, g kind, lam / radius, a, seed, use_v0, extra fit() parameters): the cases of tests/_proxadam_refs.py
CASES = [
    ("ams_l1_v0", "amsgrad", "l1", 0.1, 0.05, 0, True, {}),
    ("padam_posl1", "padam", "posl1", 0.1, 0.05, 11, False, dict(p=0.25)),
    ("ams_pos", "amsgrad", "pos", 0.0, 0.05, 0, False, {}),
    ("padam_l1", "padam", "l1", 0.1, 0.1, 27, False, dict(p=0.5)),
    ("adam_l1", "adam", "l1", 0.3, 0.2, 7, False, dict(b1=0.8, b2=0.9)),
    ("adam_pos", "adam", "pos", 0.0, 0.05, 0, False, {}),
    ("ams_box", "amsgrad", "box", 0.3, 0.05, 3, False, {}),
    ("adam_none", "adam", "none", 0.0, 0.05, 1, False, {}),
    ("ams_none", "amsgrad", "none", 0.0, 0.05, 1, False, {}),
    ("padam_none", "padam", "none", 0.0, 0.05, 0, False, dict(p=0.25)),
]


def inputs(seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N)) / np.sqrt(M)
    b = rng.standard_normal(M)
    x0 = rng.standard_normal((ROWS, N))
    return dict(A=A, b=b, x0=x0, v0=rng.uniform(0.5, 2.0, (ROWS, N)))


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


def run(data, variant, kind, pw, a, use_v0, extra, width):
    dt = width.value
    with pxrt.Precision(width):
        f = pxo.SquaredL2Norm(M).asloss(data["b"].astype(dt)) * pxa.LinOp.from_array(data["A"].astype(dt))
        s = pxs.ProxAdam(f, g_of(kind, pw), show_progress=False)
        kw = dict(extra)
        if use_v0:
            kw["v0"] = data["v0"].astype(dt)  # (the reference updates it in place: a copy of its own)
        s.fit(x0=data["x0"].astype(dt), variant=variant, a=a, stop_crit=pxst.MaxIter(ITERS), **kw)
        x = s.solution()
    assert x.dtype == dt and x.shape == (ROWS, N)
    return x


def main():
    for case, variant, kind, pw, a, seed, use_v0, extra in CASES:
        data = inputs(seed)
        x64 = run(data, variant, kind, pw, a, use_v0, extra, pxrt.Width.DOUBLE)
        x32 = run(data, variant, kind, pw, a, use_v0, extra, pxrt.Width.SINGLE)
        out = dict(data, variant=variant, g_kind=kind, g_pw=pw, a=a, seed=seed, use_v0=use_v0, iters=ITERS,
                   b1=extra.get("b1", 0.9), b2=extra.get("b2", 0.999), p=extra.get("p", 0.5), x=x64, x_f32=x32)
        path = os.path.join(HERE, f"proxadam_{case}.npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
