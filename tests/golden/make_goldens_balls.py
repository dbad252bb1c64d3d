"""
Generate the norm-ball / LInfinityNorm.prox / SquaredL1Norm golden vectors by running the upstream Pyxu
reference's own NumPy code path (brentq and the sort, one row at a time).

Run in the build container only (needs the reference snapshot, see oracle/refshim/boot.py):

    python tests/golden/make_goldens_balls.py

Writes ``tests/golden/balls_<dim>_<f32|f64>.npz`` with the inputs, the parameters and the reference's outputs.
Nothing from the reference is copied: only data.  Every input row lies outside the l1 ball / has
``||x||_1 > tau``: inside it the reference's brentq raises ValueError.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle", "refshim"))
import boot  # noqa: E402,F401  (makes the reference importable)

warnings.simplefilter("ignore")

import pyxu.operator as pxo  # noqa: E402
import pyxu.runtime as pxrt  # noqa: E402

WIDTHS = {"f32": pxrt.Width.SINGLE, "f64": pxrt.Width.DOUBLE}
STACK = (2, 3)
RADIUS = 1.5
TAU = 0.7


def save(name, **data):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in data.items()})
    print(f"wrote {name}.npz ({os.path.getsize(path)} B)")


def gen_balls():
    for dim in (37, 300):
        for w, width in WIDTHS.items():
            dt = width.value
            rng = np.random.default_rng(100 + dim)
            x = rng.standard_normal((*STACK, dim)).astype(dt)
            assert (np.abs(x).sum(axis=-1) > max(RADIUS, TAU)).all()
            small = (x * (0.5 * RADIUS / np.abs(x).sum(axis=-1, keepdims=True))).astype(dt)  # inside all three balls
            out = dict(x=x, small=small, dim=dim, radius=RADIUS, tau=TAU)
            with pxrt.Precision(width):
                for name, klass in (("l1ball", pxo.L1Ball), ("l2ball", pxo.L2Ball), ("linfball", pxo.LInfinityBall)):
                    op = klass(dim=dim, radius=RADIUS)
                    out[f"{name}_prox"] = op.prox(x, tau=TAU)
                    out[f"{name}_apply"] = op.apply(x)
                    out[f"{name}_apply_small"] = op.apply(small)
                    assert out[f"{name}_prox"].dtype == dt
                op = pxo.LInfinityNorm(dim=dim)
                out["linf_prox"] = op.prox(x, tau=TAU)
                for algo in ("sort", "root"):
                    op = pxo.SquaredL1Norm(dim=dim, prox_algo=algo)
                    out[f"sql1_prox_{algo}"] = op.prox(x, tau=TAU)
                out["sql1_apply"] = op.apply(x)
            save(f"balls_{dim}_{w}", **out)


if __name__ == "__main__":
    gen_balls()
