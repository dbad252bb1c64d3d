"""
Host references for the NUDFT kernel (pxa_nudft) and the NUFFT operator tests.

    out[q, n] = sum_m w[q, m] exp(i isign <src_m, tgt_n>)

* ``nudft64``: the sum in float64 / complex128 (the yardstick of every device comparison);
* ``nudft32_restated``: the reference's formula as it runs in single precision: fp32 dot product (no FMA),
  complex64 ``exp``, sequential complex64 accumulation over the sources;
* ``bound``: the element-wise error bound of a transform computed with unit roundoff ``u``, valid for any
  summation order,

      B[q, n](u) = u sum_m |w[q, m]| ((D + 3) Phi[m, n] + 8 + (M + 2)),   Phi[m, n] = sum_d |src[m, d] tgt[n, d]|

  ((D + 3) Phi: the phase dot product and its reduction; 8: a 4 u sine / cosine plus the complex multiply; M + 2:
  the accumulation).  A device result must satisfy |dev - ref64| <= B(u_T) + B(u_64): the second term is the
  float64 reference's own error.

The shapes of the kernel tests (``kernel_cases``) and the golden cases of the operator live here too, so that the
host test can check that each case checked norm-wise on the device stays inside the cap the norm-wise figure
assumes (max Phi <= 256, fp32 restatement within 1e-5).
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = {np.dtype(np.float32): 2.0**-24, np.dtype(np.float64): 2.0**-53}
PHI_CAP = 256.0
NORMWISE_TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}


# ------------------------------------------------------------------ the sum
def as_complex(a):
    """(..., 2 K) interleaved real view -> (..., K) complex."""
    a = np.ascontiguousarray(a)
    return a.view(np.complex64 if a.dtype == np.float32 else np.complex128)


def as_real(c):
    c = np.ascontiguousarray(c)
    return c.view(np.float32 if c.dtype == np.complex64 else np.float64)


def nudft64(w, src, tgt, isign):
    """w (Q, M) complex, src (M, D), tgt (N, D) -> (Q, N) complex128."""
    phase = tgt.astype(np.float64) @ src.astype(np.float64).T  # (N, M)
    return w.astype(np.complex128) @ np.exp(1j * isign * phase).T


def nudft32_restated(w, src, tgt, isign):
    """The reference's formula in single precision: fp32 dot, complex64 exp, sequential complex64 accumulation."""
    w = w.astype(np.complex64)
    src, tgt = src.astype(np.float32), tgt.astype(np.float32)
    out = np.zeros((w.shape[0], tgt.shape[0]), dtype=np.complex64)
    for m in range(src.shape[0]):
        dot = np.zeros(tgt.shape[0], dtype=np.float32)
        for d in range(src.shape[1]):
            dot += src[m, d] * tgt[:, d]
        z = np.zeros(tgt.shape[0], dtype=np.complex64)
        z.imag = np.float32(isign) * dot
        out += w[:, m, None] * np.exp(z)[None, :]
    return out


def phi(src, tgt):
    """Phi[n, m] = sum_d |src[m, d] tgt[n, d]|, (N, M) float64."""
    return np.abs(tgt.astype(np.float64)) @ np.abs(src.astype(np.float64)).T


def bound(w, src, tgt, u):
    """B[q, n](u), (Q, N) float64."""
    M, D = src.shape
    aw = np.abs(w.astype(np.complex128))  # (Q, M)
    return u * ((D + 3) * (aw @ phi(src, tgt).T) + (8 + M + 2) * aw.sum(axis=1, keepdims=True))


def within_bound(dev, w, src, tgt, isign, dtype):
    """(ok, worst ratio) of |dev - ref64| against B(u_T) + B(u_64), element-wise."""
    ref = nudft64(w, src, tgt, isign)
    lim = bound(w, src, tgt, U[np.dtype(dtype)]) + bound(w, src, tgt, U[np.dtype(np.float64)])
    err = np.abs(dev.astype(np.complex128) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst <= 1.0, worst


def rel_err(a, b):
    a, b = np.asarray(a).astype(np.complex128).ravel(), np.asarray(b).astype(np.complex128).ravel()
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


# ------------------------------------------------------------------ kernel test shapes
def kernel_cases(tile_n, tile_m, q_chunk):
    """Edge shapes of pxa_nudft as dicts (N, M, Q, D, isign, splits): a cross around one base case, not the product."""
    Ns = (1, tile_n - 1, tile_n + 1, 2 * tile_n + 3)
    Ms = (1, tile_m - 1, tile_m + 1, 2 * tile_m + 3)
    base = dict(N=tile_n + 1, M=tile_m + 1, Q=3, D=2, isign=1, splits=1)
    out = [base]
    out += [dict(base, N=n) for n in Ns if n != base["N"]]
    out += [dict(base, M=m) for m in Ms if m != base["M"]]
    out += [dict(base, Q=q) for q in (1, q_chunk + 1)]
    out += [dict(base, Q=2, D=1), dict(base, D=3, isign=-1), dict(base, isign=-1)]
    # ragged last split, splits > M, and the library's choice
    out += [dict(base, M=2 * tile_m + 3, splits=s) for s in (2, 3, 7, 0)]
    out += [dict(base, M=3, splits=7), dict(base, M=1, N=1, Q=1, D=1, splits=2)]
    out += [dict(N=1, M=1, Q=1, D=1, isign=-1, splits=1)]
    out += [dict(N=2 * tile_n + 3, M=2 * tile_m + 3, Q=q_chunk + 1, D=3, isign=-1, splits=3)]
    # few targets, many sources: splits = 0 resolves to more than one split
    out += [dict(N=tile_n - 1, M=8 * tile_m + 5, Q=1, D=2, isign=1, splits=0)]
    out += [dict(N=tile_n - 1, M=8 * tile_m + 5, Q=q_chunk + 1, D=3, isign=-1, splits=0)]
    return out


def case_id(c):
    return "N{N}-M{M}-Q{Q}-D{D}-s{isign}-sp{splits}".format(**c)


def kernel_inputs(c, dtype):
    """Seeded (src, tgt, w) of a kernel case: sources in [-pi, pi)^D, targets in [-20, 20]^D (Phi <= 3 pi 20 < 256)."""
    rng = np.random.default_rng([c["N"], c["M"], c["Q"], c["D"]])
    src = rng.uniform(-np.pi, np.pi, size=(c["M"], c["D"])).astype(dtype)
    tgt = rng.uniform(-20.0, 20.0, size=(c["N"], c["D"])).astype(dtype)
    w = rng.standard_normal((c["Q"], 2 * c["M"])).astype(dtype)
    return src, tgt, w


# ------------------------------------------------------------------ operator goldens
def mesh_unit(N, modeord):
    """(N1, ..., Nd, d) float64 mode grid: [-(n // 2), (n - 1) // 2] per axis, FFT order when modeord = 1."""
    axes = []
    for n in N:
        k = np.arange(-(int(n) // 2), (int(n) - 1) // 2 + 1, dtype=np.float64)
        axes.append(np.concatenate([k[k >= 0], k[k < 0]]) if modeord == 1 else k)
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


@functools.lru_cache(maxsize=None)
def load_golden(width):
    with np.load(os.path.join(GOLDEN, f"nufft_{width}.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def golden_cases(width):
    """One dict per golden case: parameters, (src, tgt) point sets, apply / adjoint inputs and the reference's outputs."""
    g = load_golden(width)
    out = []
    for (typ, D, real, sgn, modeord, stk), (a0, an, t0, tn) in zip(g["cases"].tolist(), g["spans"].tolist()):
        x, N = g[f"x_d{D}"], tuple(int(v) for v in g[f"n_d{D}"])
        pre = "stk_" if stk else ""
        if typ == 3:
            src, tgt = x, g[f"z_d{D}"]
            a_in, t_in = g[pre + "w"], g[pre + "v"]
        else:
            grid = mesh_unit(N, modeord).reshape(-1, D).astype(x.dtype)
            src, tgt = (x, grid) if typ == 1 else (grid, x)
            a_in, t_in = (g[pre + "w"], g[pre + f"u_d{D}"]) if typ == 1 else (g[pre + f"u_d{D}"], g[pre + "w"])
        if real:
            a_in = np.ascontiguousarray(a_in[..., 0::2])
        lead = a_in.shape[:-1]
        out.append(dict(
            id=f"t{typ}-d{D}-r{real}-s{sgn}-o{modeord}" + ("-stk" if stk else ""),
            typ=typ, D=D, real=bool(real), isign=sgn, modeord=modeord, x=x, z=g[f"z_d{D}"], N=N, src=src, tgt=tgt,
            a_in=a_in, t_in=t_in,
            apply=g["outputs"][a0:a0 + an].reshape(*lead, -1), adjoint=g["outputs"][t0:t0 + tn].reshape(*lead, -1),
        ))
    return out


def op_weights(c, which):
    """The complex (Q, K) weights the transform behind `which` ("apply" / "adjoint") of a golden case sums over."""
    if which == "apply":
        a = c["a_in"]
        w = a.astype(np.complex64 if a.dtype == np.float32 else np.complex128) if c["real"] else as_complex(a)
    else:
        w = as_complex(c["t_in"])
    return w.reshape(-1, w.shape[-1])


def op_transform(fn, c, which):
    """apply / adjoint of a golden case through the sum `fn(w, src, tgt, isign)`, as the complex (Q, N) result with
    the point sets it used: (out, w, src, tgt, isign)."""
    w = op_weights(c, which)
    src, tgt, sgn = (c["src"], c["tgt"], c["isign"]) if which == "apply" else (c["tgt"], c["src"], -c["isign"])
    return fn(w, src, tgt, sgn), w, src, tgt, sgn


def op_output(c, which, out):
    """Complex (Q, N) result -> the real array apply / adjoint return for this case."""
    lead = c["a_in"].shape[:-1]
    if which == "adjoint" and c["real"]:
        return np.ascontiguousarray(out.real).reshape(*lead, -1)
    return as_real(out).reshape(*lead, -1)


def op_worst_ratio(c, which, y, dtype):
    """max over the outputs of |y - ref64| / (B(u_T) + B(u_64)) for the real array `y` that apply / adjoint of a golden
    case returned (complex modulus; the real part alone for a real-output adjoint)."""
    ref, w, src, tgt, _ = op_transform(nudft64, c, which)
    lim = bound(w, src, tgt, U[np.dtype(dtype)]) + bound(w, src, tgt, U[np.dtype(np.float64)])
    y = np.ascontiguousarray(y).reshape(-1, y.shape[-1])
    if which == "adjoint" and c["real"]:
        err = np.abs(y.astype(np.float64) - ref.real)
    else:
        err = np.abs(as_complex(y).astype(np.complex128) - ref)
    return float((err / lim).max())


# ------------------------------------------------------------------ dense matrix of a type-2 transform
def type2_matrix64(x, N, isign, real, modeord=0):
    """float64 real matrix of NUFFT.type2(x, N, isign, real=real): (2 M, prod N) if real else (2 M, 2 prod N)."""
    grid = mesh_unit(N, modeord).reshape(-1, x.shape[1])
    C = np.exp(1j * isign * (x.astype(np.float64) @ grid.T))  # (M, prod N)
    A = np.empty((2 * C.shape[0], 2 * C.shape[1]))
    A[0::2, 0::2], A[0::2, 1::2] = C.real, -C.imag
    A[1::2, 0::2], A[1::2, 1::2] = C.imag, C.real
    return np.ascontiguousarray(A[:, 0::2]) if real else A
