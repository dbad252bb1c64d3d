"""
Generate the NUFFT golden vectors by running the upstream Pyxu reference's own direct evaluation
(``NUFFT.type1/2/3(..., eps=0)``, its NumPy ``_nudft`` path) through oracle/refshim.

Run in the build container only (needs the reference snapshot, see oracle/refshim/boot.py):

    python tests/golden/make_goldens_nufft.py

Writes ``tests/golden/nufft_<f32|f64>.npz``.  Nothing from the reference is copied: only data.

Layout.  Shared inputs: ``x_d<D>`` (M, D) sample points in [-pi, pi), ``z_d<D>`` (NZ, D) type-3 targets,
``n_d<D>`` the mode counts, and complex vectors as interleaved real views: ``w`` (2 M), ``u_d<D>`` (2 prod N),
``v`` (2 NZ), and stacked ones ``stk_w`` / ``stk_u_d2`` / ``stk_v`` of leading shape (2, 3).  A real-valued
input is the even entries (the real parts) of the complex one.  ``cases`` holds one row (type, D, real, isign,
modeord, stacked) per case and ``spans`` its (apply offset, apply size, adjoint offset, adjoint size) into the flat
``outputs`` array (one array instead of two per case: the zip directory would outweigh the data).  apply's input is
w (types 1, 3) or u (type 2), adjoint's input is u (type 1), w (type 2) or v (type 3); a stacked output has the
leading shape (2, 3).
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
M, NZ = 67, 29
MODES = {1: (13,), 2: (5, 6), 3: (3, 4, 2)}
STACK = (2, 3)


def save(name, **data):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in data.items()})
    print(f"wrote {name}.npz ({os.path.getsize(path)} B)")
    assert os.path.getsize(path) < 100_000


def inputs(dt):
    rng = np.random.default_rng(2024)
    d = {}
    for D in (1, 2, 3):
        d[f"x_d{D}"] = rng.uniform(-np.pi, np.pi, size=(M, D)).astype(dt)
        d[f"z_d{D}"] = rng.uniform(-8.0, 8.0, size=(NZ, D)).astype(dt)
        d[f"n_d{D}"] = np.array(MODES[D], dtype=np.int64)
        d[f"u_d{D}"] = rng.standard_normal(2 * int(np.prod(MODES[D]))).astype(dt)
    d["w"] = rng.standard_normal(2 * M).astype(dt)
    d["v"] = rng.standard_normal(2 * NZ).astype(dt)
    d["stk_w"] = rng.standard_normal((*STACK, 2 * M)).astype(dt)
    d["stk_u_d2"] = rng.standard_normal((*STACK, 2 * int(np.prod(MODES[2])))).astype(dt)
    d["stk_v"] = rng.standard_normal((*STACK, 2 * NZ)).astype(dt)
    return d


def cases():
    for typ in (1, 2, 3):
        for D in (1, 2, 3):
            for real in (0, 1):
                for sgn in (1, -1):
                    yield typ, D, real, sgn, 0, False
    for typ in (1, 2):  # FFT mode order
        for D, real, sgn in ((1, 0, 1), (2, 1, -1), (3, 0, -1)):
            yield typ, D, real, sgn, 1, False
    yield 1, 2, 0, 1, 0, True  # stacked (2, 3, .) inputs
    yield 2, 2, 1, -1, 1, True
    yield 3, 3, 0, -1, 0, True


def gen():
    for wname, width in WIDTHS.items():
        dt = width.value
        out = inputs(dt)
        table, spans, flat, pos = [], [], [], 0
        with pxrt.Precision(width):
            for typ, D, real, sgn, modeord, stk in cases():
                x = out[f"x_d{D}"]
                pre = "stk_" if stk else ""
                w, u, v = out[pre + "w"], out[pre + f"u_d{D}"] if (not stk or D == 2) else None, out[pre + "v"]
                if typ == 1:
                    op = pxo.NUFFT.type1(x, MODES[D], isign=sgn, eps=0, real=bool(real), modeord=modeord)
                    a_in, t_in = w, u
                elif typ == 2:
                    op = pxo.NUFFT.type2(x, MODES[D], isign=sgn, eps=0, real=bool(real), modeord=modeord)
                    a_in, t_in = u, w
                else:
                    op = pxo.NUFFT.type3(x, out[f"z_d{D}"], isign=sgn, eps=0, real=bool(real))
                    a_in, t_in = w, v
                if real:
                    a_in = np.ascontiguousarray(a_in[..., 0::2])
                ya, yt = op.apply(a_in), op.adjoint(t_in)
                assert ya.dtype == dt and yt.dtype == dt
                assert ya.shape == (*a_in.shape[:-1], op.codim) and yt.shape == (*t_in.shape[:-1], op.dim)
                table.append((typ, D, real, sgn, modeord, int(stk)))
                spans.append((pos, ya.size, pos + ya.size, yt.size))
                flat += [ya.ravel(), yt.ravel()]
                pos += ya.size + yt.size
        out["cases"] = np.array(table, dtype=np.int64)
        out["spans"] = np.array(spans, dtype=np.int64)
        out["outputs"] = np.concatenate(flat)
        save(f"nufft_{wname}", **out)


if __name__ == "__main__":
    gen()
