"""
Generate the NLCG golden trajectories by running the upstream Pyxu reference's own NLCG (NumPy code path).

Run in the build container only (needs the reference snapshot, see oracle/refshim/boot.py):

    python tests/golden/make_goldens_nlcg.py

Writes ``tests/golden/nlcg_<objective>_<variant>.npz``: the inputs and parameters, per iteration of the reference's
float64 run the step sizes ``ls_a_k`` and ``||gradient||_2`` (entry 0: the initial gradient), its final ``x``, and the
final ``x`` of the reference's float32 run.  For the T objective the dense matrix of the reference's Gradient operator
is stored as well, so that tests/_nlcg_refs.py can restate the objective without it.  Nothing from the reference is
copied: only data.

Objectives (rng = default_rng(seed), draws in the stated order):
  Q: A = standard_normal((24, 17)) / sqrt(24), b = standard_normal(24), x0 = standard_normal((3, 17));
     f = SquaredL2Norm(24).asloss(b) * LinOp.from_array(A)
  T: y = standard_normal(99), x0 = standard_normal((3, 99));
     f = 0.5 SquaredL2Norm(99).asloss(y) + 0.3 (L1Norm(198).moreau_envelope(0.05) * Gradient((9, 11), "fd", "constant"))
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

ITERS, ROWS, R, C = 12, 3, 0.5, 1e-4
T_SHAPE, T_MU, T_LAM = (9, 11), 0.05, 0.3
# (objective, variant, restart_rate, a0, seed): the cases of tests/_nlcg_refs.py CASES
CASES = [("Q", "FR", 5, 1.0, 4), ("Q", "PR", 5, 0.35, 6), ("T", "PR", 100, 0.4, 5), ("T", "FR", 5, 1.0, 5)]


def inputs(obj, seed):
    rng = np.random.default_rng(seed)
    if obj == "Q":
        A = rng.standard_normal((24, 17)) / np.sqrt(24)
        b = rng.standard_normal(24)
        return dict(A=A, b=b, x0=rng.standard_normal((ROWS, 17)))
    y = rng.standard_normal(99)
    return dict(y=y, x0=rng.standard_normal((ROWS, 99)))


def objective(obj, data, dt):
    if obj == "Q":
        return pxo.SquaredL2Norm(24).asloss(data["b"].astype(dt)) * pxa.LinOp.from_array(data["A"].astype(dt))
    G = pxo.Gradient(T_SHAPE, diff_method="fd", mode="constant")
    return 0.5 * pxo.SquaredL2Norm(99).asloss(data["y"].astype(dt)) + T_LAM * (pxo.L1Norm(198).moreau_envelope(T_MU) * G)


def run(obj, data, variant, rate, a0, width):
    dt = width.value
    with pxrt.Precision(width):
        f = objective(obj, data, dt)
        s = pxs.NLCG(f, show_progress=False)
        s.fit(x0=data["x0"].astype(dt), variant=variant, restart_rate=rate, a0=a0, r=R, c=C, mode=pxa.Mode.MANUAL,
              stop_crit=pxst.MaxIter(ITERS))
        gn = [np.linalg.norm(s._mstate["gradient"], axis=-1)]
        ak = []
        for _ in s.steps():
            gn.append(np.linalg.norm(s._mstate["gradient"], axis=-1))
            ak.append(np.asarray(s._mstate["ls_a_k"]).reshape(-1))
        x = s.solution()
    assert x.dtype == dt and len(ak) == ITERS
    return np.array(ak), np.array(gn), x


def main():
    for obj, variant, rate, a0, seed in CASES:
        data = inputs(obj, seed)
        ak, gn, x64 = run(obj, data, variant, rate, a0, pxrt.Width.DOUBLE)
        _, _, x32 = run(obj, data, variant, rate, a0, pxrt.Width.SINGLE)
        out = dict(data, variant=variant, restart_rate=rate, a0=a0, seed=seed, r=R, c=C, iters=ITERS, ls_a_k=ak, gnorm=gn,
                   x=x64, x_f32=x32)
        if obj == "T":
            with pxrt.Precision(pxrt.Width.DOUBLE):
                out["G"] = pxo.Gradient(T_SHAPE, diff_method="fd", mode="constant").asarray(dtype=np.float64)
            out.update(mu=T_MU, lam=T_LAM, shape=np.array(T_SHAPE))
        path = os.path.join(HERE, f"nlcg_{obj}_{variant}.npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
        print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
