"""
float64 NumPy restatement of the ProxAdam solver (opt/solver/prox_adam.py) with its four element-wise prox kinds and
the per-row accelerated-PGD sub-solve, the float64 references and derived error bounds of the two kernels of
csrc/proxadam.hip, and the conditions under which a run can be compared across precisions at all.

A trajectory can only be compared where no stop decision of a sub-solve rests on rounding.  In float32 the statistic
||z_k - z_{k-1}|| is a difference of nearly equal numbers: its relative rounding error is about 6e-8 / 1e-4 = 6e-4.  So
every run reports, and test_proxadam_refs.py asserts for every case a GPU test uses:

  stop_margin   min over all sub-iterations and rows of | ||dz|| / (eps ||z||) - 1 |     >= 1e-2
  rows_differ   some step whose rows stop at different sub-iteration counts
  max_count     largest sub-iteration count                                               >= 3

Kernel bounds (derived, in the style of tests/_prim_refs.py; e = finfo(T).eps, references in float64 on the T inputs
and the T scalars):
* m' = b1 m + (1 - b1) g, v_u = b2 v + (1 - b2) g^2: at most 4 rounded operations: 8 e S, S the sum of the absolute
  values of the terms (CHAIN_FACTOR).  The clip and the maximum are 1-Lipschitz: v' and vhat' inherit v_u's bound.
* psi: every term of v_u is non-negative, so v' carries a relative error rv <= 8 e; sqrt halves it and adds e / 2, the
  division by c2 and the sum with eps_adam add e / 2 each: |psi - ref| <= (rv + 4 e) ref, twice the first-order sum.
  vhat'^p with p != 0.5 goes through the device pow: + OP_TOL relative.
* phi = m' / c1: dphi = dm / c1 + e |phi|.  x' = x - a (phi / psi): a (dphi / psi + |q| (rpsi + 2 e)) + 8 e (|x| + |a q|).
* sub-step: y = (z - z_prev) mom + z: dy = 8 e (|z| + mom (|z| + |z_prev|)); w = (1 - r) y + r xt with r = psi / psimax
  in [0, 1]: dw = dy + 8 e (|y| + |xt|); the prox is 1-Lipschitz and its threshold gamma lam carries 3 roundings:
  dz = dw + 4 e thr.  With r == 1 the step is w = xt exactly.
* sums: double accumulation in any order: |got - ref| <= (n + 4) 2^-53 sum |t_i|.

Shared by test_proxadam_refs.py (CPU: the restatement against the reference's goldens) and test_gpu_proxadam.py.
"""
import numpy as np

STOP_MARGIN = 1e-2
F32_ADMIT = 3.3e-6  # a case counts for f32 only if the reference's own f32 x is this close to the restatement
PGD_D = 75
KINDS = ("l1", "pos", "posl1", "box")  # lam L1Norm, PositiveOrthant, lam PositiveL1Norm, LInfinityBall(r)

# name -> (golden file, f32 admitted); parameters live in the golden.  Not admitted: amsgrad from v0 = 0 and padam with
# p = 0.5 divide by sqrt(vhat) with vhat ~ (1 - b2) g^2, and 1 - b2 formed in float32 is 0.0010000467: 4.7e-5 off,
# 2.3e-5 in psi and several 1e-6 in x per step, which no bias correction cancels (adam's sqrt(1 - b2^t) does).  The
# reference's own f32 runs of these end 5.2e-6 to 9.7e-6 from float64, on every seed found that meets the conditions.
CASES = {
    "ams-l1-v0": ("proxadam_ams_l1_v0", True),
    "padam-posl1": ("proxadam_padam_posl1", True),
    "ams-pos": ("proxadam_ams_pos", False),
    "padam-l1": ("proxadam_padam_l1", False),
    "adam-l1": ("proxadam_adam_l1", True),
    "adam-pos": ("proxadam_adam_pos", True),
    "ams-box": ("proxadam_ams_box", True),
    "adam-none": ("proxadam_adam_none", True),
    "ams-none": ("proxadam_ams_none", False),
    "padam-none": ("proxadam_padam_none", True),
}


def with_g(name):
    return not name.endswith("-none")


# ------------------------------------------------------------------------------------------------ the pieces
def prox(kind, w, gamma, pw):
    """prox_{gamma g}(w): pw is lam (l1, posl1) or the radius (box)."""
    if kind == "l1":
        return np.sign(w) * np.maximum(np.abs(w) - gamma * pw, 0.0)
    if kind == "pos":
        return np.clip(w, 0.0, None)
    if kind == "posl1":
        return np.clip(w - gamma * pw, 0.0, None)
    if kind == "box":
        return np.clip(w, -pw, pw)
    raise ValueError(kind)


def sub_solve(xt, psi, a, kind, pw, eps=1e-4, max_iter=None, margins=None):
    """One row's metric prox by accelerated PGD from xt: tau = gamma = a / max(psi), momentum k / (k + 1 + 75); after
    sub-iteration k the row stops when ||z_k - z_{k-1}|| <= eps ||z_{k-1}|| (max_iter: exactly that many iterations
    instead).  Returns (z, count)."""
    gamma = a / psi.max()
    z_prev = z = xt
    k = 0
    while True:
        mom = k / (k + 1 + PGD_D)
        y = z + mom * (z - z_prev)
        w = y - gamma * (psi * (y - xt)) / a
        z_prev, z = z, prox(kind, w, gamma, pw)
        k += 1
        if max_iter is not None:
            if k >= max_iter:
                return z, k
            continue
        num, den = np.linalg.norm(z - z_prev), np.linalg.norm(z_prev)
        if margins is not None and den > 0:
            margins.append(abs(num / (eps * den) - 1.0))
        if num <= eps * den:
            return z, k


def moments(variant, t, first, g, m, v, vh, x, a, b1, b2, p, eps_adam, eps_var, omb1=None, omb2=None, c1=None, c2=None):
    """prox_adam.py:341-370 on float64 arrays: (m', v', vhat', x', psi, phi).  The derived scalars may be given (the T
    values a kernel received)."""
    omb1 = 1.0 - b1 if omb1 is None else omb1
    omb2 = 1.0 - b2 if omb2 is None else omb2
    c1 = 1.0 - b1**t if c1 is None else c1
    c2 = np.sqrt(1.0 - b2**t) if c2 is None else c2
    m1 = b1 * m + omb1 * g
    v1 = np.clip(b2 * v + omb2 * g * g, eps_var, None)
    vh1 = v1 if first else np.maximum(vh, v1)
    if variant == "adam":
        phi, psi = m1 / c1, np.sqrt(v1) / c2 + eps_adam
    elif variant == "amsgrad":
        phi, psi = m1, np.sqrt(vh1)
    elif variant == "padam":
        phi, psi = m1, vh1**p
    else:
        raise ValueError(variant)
    return m1, v1, vh1, x - a * (phi / psi), psi, phi


def proxadam(grad, x0, variant, a, iters, b1=0.9, b2=0.999, m0=None, v0=None, p=0.5, eps_adam=1e-6, eps_var=1e-6,
             g=None, eps_sub=1e-4, sub_max_iter=None):
    """`iters` ProxAdam iterations from x0 (rows, n); g = (kind, pw) or None.  Returns a dict: x, counts (iters, rows),
    stop_margin, rows_differ, max_count."""
    x = np.array(x0, dtype=np.float64)
    m = np.zeros_like(x) if m0 is None else np.broadcast_to(np.asarray(m0, dtype=np.float64), x.shape).copy()
    v = np.zeros_like(x) if v0 is None else np.broadcast_to(np.asarray(v0, dtype=np.float64), x.shape).copy()
    vh = v
    counts, margins = [], []
    for t in range(1, iters + 1):
        m, v, vh, x, psi, _ = moments(variant, t, t == 1, grad(x), m, v, vh, x, a, b1, b2, p, eps_adam, eps_var)
        if g is not None:
            rows = [sub_solve(x[r], psi[r], a, g[0], g[1], eps_sub, sub_max_iter, margins) for r in range(x.shape[0])]
            x = np.stack([z for z, _ in rows])
            counts.append([k for _, k in rows])
    counts = np.array(counts, dtype=np.int64).reshape(-1, x.shape[0])
    out = dict(x=x, counts=counts, mean=m, variance=v, variance_hat=vh)
    out["stop_margin"] = min(margins) if margins else np.inf
    out["rows_differ"] = bool(counts.size and (counts.max(axis=1) != counts.min(axis=1)).any())
    out["max_count"] = int(counts.max()) if counts.size else 0
    return out


def objective_Q(A, b):
    """grad of f(x) = ||A x - b||^2 per row."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return lambda x: 2.0 * (((x @ A.T) - b) @ A)


def g_of(gold):
    kind = str(gold["g_kind"])
    return None if kind == "none" else (kind, float(gold["g_pw"]))


_RUNS = {}


def run_case(name, gold, sub_max_iter=None):
    """The restatement's run of a CASES entry on its golden's inputs (computed once, shared, read-only)."""
    key = (name, sub_max_iter)
    if key not in _RUNS:
        v0 = gold["v0"] if bool(gold["use_v0"]) else None
        res = proxadam(objective_Q(gold["A"], gold["b"]), gold["x0"], str(gold["variant"]), float(gold["a"]),
                       int(gold["iters"]), b1=float(gold["b1"]), b2=float(gold["b2"]), v0=v0, p=float(gold["p"]),
                       g=g_of(gold), sub_max_iter=sub_max_iter)
        for val in res.values():
            if isinstance(val, np.ndarray):
                val.setflags(write=False)
        _RUNS[key] = res
    return _RUNS[key]


def row_rel(a, b):
    """Relative l2 error per row, worst row."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


# ------------------------------------------------------------------------------------------------ kernel bounds
CHAIN_FACTOR = 8.0
OP_TOL = {np.float32: 1e-5, np.float64: 1e-12}


def moments_bounds(dt, variant, g, m, v, x, ref, a, b1, omb1, b2, omb2, c1, p):
    """Absolute bounds (dm, dv, dvh, dx, dpsi) on the outputs of pxa_proxadam_moments against `ref` = moments(...) in
    float64 on the same inputs and scalars (module docstring)."""
    e = float(np.finfo(dt).eps)
    m1, v1, vh1, x1, psi, phi = ref
    dm = CHAIN_FACTOR * e * (np.abs(b1 * m) + np.abs(omb1 * g))
    dv = CHAIN_FACTOR * e * (np.abs(b2 * v) + np.abs(omb2 * g * g))
    base = v1 if variant == "adam" else vh1
    rpsi = dv / base + 4 * e + (OP_TOL[dt] if (variant == "padam" and p != 0.5) else 0.0)
    dphi = dm / abs(c1) + e * np.abs(phi) if variant == "adam" else dm
    q = phi / psi
    dx = abs(a) * (dphi / psi + np.abs(q) * (rpsi + 2 * e)) + CHAIN_FACTOR * e * (np.abs(x) + np.abs(a * q))
    return dm, dv, dv, dx, rpsi * psi


def sub_step_ref(dt, kind, pw, mom, a, xt, psi, z_prev, z):
    """(z_new, bound, thr) of one pxa_proxadam_sub_step update in float64 on T inputs: psimax, gamma = a / psimax and
    thr = gamma pw as the kernel forms them, in T."""
    e = float(np.finfo(dt).eps)
    pmax = psi.max(axis=-1, keepdims=True).astype(dt)
    gamma = (dt(a) / pmax).astype(dt)
    thr = (gamma * dt(pw)).astype(dt) if kind != "box" else np.full_like(gamma, dt(pw))
    X, P, ZP, Z = (np.asarray(t, dtype=np.float64) for t in (xt, psi, z_prev, z))
    mom = float(dt(mom))
    y = (Z - ZP) * mom + Z
    r = (psi / pmax).astype(np.float64)  # the T quotient: exactly 1 where psi == psimax
    w = (1.0 - r) * y + r * X
    t64 = thr.astype(np.float64)
    if kind == "l1":
        zn = np.sign(w) * np.maximum(np.abs(w) - t64, 0.0)
    elif kind == "pos":
        zn = np.clip(w, 0.0, None)
    elif kind == "posl1":
        zn = np.clip(w - t64, 0.0, None)
    else:
        zn = np.clip(w, -t64, t64)
    dy = CHAIN_FACTOR * e * (np.abs(Z) + mom * (np.abs(Z) + np.abs(ZP)))
    bound = dy + CHAIN_FACTOR * e * (np.abs(y) + np.abs(X)) + 4 * e * t64
    return zn, bound, thr


def blocks_per_row(rows, n):
    """csrc/common.hpp blocks_per_row."""
    per = (n + 4095) // 4096
    cap = max((4096 + rows - 1) // rows, 1)
    return max(min(per, cap, 1024), 1)


def chunk(dt, rows, n):
    """Elements per workgroup of a row: ceil(n / blocks) rounded up to a whole 16-byte vector."""
    vn = 16 // np.dtype(dt).itemsize
    c = -(-n // blocks_per_row(rows, n))
    return -(-c // vn) * vn
