"""
float64 NumPy restatement of the NLCG solver (opt/solver/nlcg.py) and its Armijo backtracking search
(math/linesearch.py), with the objective given as (apply, grad) callables on (rows, n) arrays; the two test
objectives; and the conditions under which a run's trajectory can be compared with another precision's at all.

A trajectory can only be compared where no decision rests on rounding.  Under an Armijo-only search PR regularly
produces ascent directions; the search then halves the step down to round-off and rounding decides acceptance.  So
every run reports, and test_nlcg_refs.py asserts for every case a GPU test uses:

  armijo_margin   min over all trials and rows of |lhs - rhs| / max(|lhs|, |f_x|)      >= 1e-4  (~100x the f32
                  rounding of f)
  gp_max          max over iterations and rows of <g, p>                                < 0
  pr_margin       min over PR iterations (no restart) and rows of |num| / ||g1||^2     >= 1e-3
  max_backtracks  largest number of halvings of one search                              >= 2
  rows_differ     some iteration whose rows differ in halvings
  clipped / unclipped   PR iterations (rows counted) with beta clipped to 0 / not      both > 0 for PR
  restarts        iterations with idx % restart_rate == 0                               >= 1 (Q cases)

Shared by test_nlcg_refs.py (CPU: the restatement against the reference's goldens) and test_gpu_nlcg.py.
"""
import numpy as np

ARMIJO_MARGIN = 1e-4
PR_MARGIN = 1e-3
F32_ADMIT = 3.3e-6  # a case counts for f32 only if the reference's own f32 x is this close to the restatement

# name -> (golden file, f32 admitted); parameters live in the golden
CASES = {
    "Q-FR": ("nlcg_Q_FR", True),
    "Q-PR": ("nlcg_Q_PR", True),
    "T-PR": ("nlcg_T_PR", True),
    "T-FR": ("nlcg_T_FR", False),  # FR amplifies rounding on this objective: the reference's f32 run ends 6e-4 away
}


# ------------------------------------------------------------------------------------------------ objectives
def objective_Q(A, b):
    """f(x) = ||A x - b||^2 per row."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)

    def apply(x):
        return (((x @ A.T) - b) ** 2).sum(axis=-1, keepdims=True)

    def grad(x):
        return 2.0 * (((x @ A.T) - b) @ A)

    return apply, grad


def objective_T(y, G, mu, lam):
    """f(x) = 0.5 ||x - y||^2 + lam env_mu(||.||_1)(G x): the Moreau envelope of |.| is the Huber function."""
    y, G = np.asarray(y, dtype=np.float64), np.asarray(G, dtype=np.float64)

    def apply(x):
        z = np.abs(x @ G.T)
        h = np.where(z <= mu, z * z / (2.0 * mu), z - 0.5 * mu)
        return 0.5 * ((x - y) ** 2).sum(axis=-1, keepdims=True) + lam * h.sum(axis=-1, keepdims=True)

    def grad(x):
        return (x - y) + lam * (np.clip((x @ G.T) / mu, -1.0, 1.0) @ G)

    return apply, grad


def objective_of(gold):
    if "A" in gold:
        return objective_Q(gold["A"], gold["b"])
    return objective_T(gold["y"], gold["G"], float(gold["mu"]), float(gold["lam"]))


# ------------------------------------------------------------------------------------------------ the search
def linesearch(apply, x, p, g, a0, r, c, f_x=None, margins=None):
    """Armijo backtracking on every row: returns (a (rows, 1), halvings (rows,), f at the accepted points).  All
    rows are re-evaluated on every trial with their current a."""
    if f_x is None:
        f_x = apply(x)
    d_f = c * (g * p).sum(axis=-1, keepdims=True)
    a = np.full((x.shape[0], 1), a0, dtype=np.float64)
    k = np.zeros(x.shape[0], dtype=np.int64)
    while True:
        lhs = apply(x + a * p)
        rhs = f_x + a * d_f
        if margins is not None:
            margins.append(float((np.abs(lhs - rhs) / np.maximum(np.abs(lhs), np.abs(f_x))).min()))
        mask = lhs > rhs
        if not mask.any():
            return a, k, lhs
        a[mask] *= r
        k[mask[:, 0]] += 1


def nlcg(apply, grad, x0, variant, restart_rate, a0, r, c, iters):
    """`iters` NLCG iterations from x0 (rows, n).  Returns a dict: ls_a_k (iters, rows), halvings (iters, rows),
    gnorm (iters + 1, rows), x, and the conditions of the module docstring."""
    variant = variant.lower()
    assert variant in ("fr", "pr")
    x = np.array(x0, dtype=np.float64)
    g = grad(x)
    p = -g
    f_x = None
    out = dict(ls_a_k=[], halvings=[], gnorm=[np.linalg.norm(g, axis=-1)], gp_max=-np.inf, pr_margin=np.inf,
               clipped=0, unclipped=0, restarts=0)
    margins = []
    for idx in range(1, iters + 1):
        out["gp_max"] = max(out["gp_max"], float((g * p).sum(axis=-1).max()))
        a, k, f_x = linesearch(apply, x, p, g, a0, r, c, f_x=f_x, margins=margins)
        x = x + a * p
        g1 = grad(x)
        if idx % restart_rate == 0:
            beta = np.zeros((x.shape[0], 1))
            out["restarts"] += 1
        elif variant == "fr":
            beta = (np.linalg.norm(g1, axis=-1, keepdims=True) / np.linalg.norm(g, axis=-1, keepdims=True)) ** 2
        else:
            num = (g1 * (g1 - g)).sum(axis=-1, keepdims=True)
            out["pr_margin"] = min(out["pr_margin"], float((np.abs(num) / (g1 * g1).sum(axis=-1, keepdims=True)).min()))
            beta = num / np.linalg.norm(g, axis=-1, keepdims=True) ** 2
            out["clipped"] += int((beta < 0).sum())
            out["unclipped"] += int((beta >= 0).sum())
            beta = beta.clip(min=0)
        p = beta * p - g1
        g = g1
        out["ls_a_k"].append(a[:, 0].copy())
        out["halvings"].append(k)
        out["gnorm"].append(np.linalg.norm(g, axis=-1))
    for key in ("ls_a_k", "halvings", "gnorm"):
        out[key] = np.array(out[key])
    out["x"] = x
    out["armijo_margin"] = min(margins)
    out["max_backtracks"] = int(out["halvings"].max())
    out["rows_differ"] = bool((out["halvings"].max(axis=1) != out["halvings"].min(axis=1)).any())
    return out


_RUNS = {}


def run_case(name, gold):
    """The restatement's run of a CASES entry on its golden's inputs (computed once, shared, read-only)."""
    if name not in _RUNS:
        apply, grad = objective_of(gold)
        res = nlcg(apply, grad, gold["x0"], str(gold["variant"]), int(gold["restart_rate"]), float(gold["a0"]),
                   float(gold["r"]), float(gold["c"]), int(gold["iters"]))
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[name] = res
    return _RUNS[name]


def row_rel(a, b):
    """Relative l2 error per row, worst row."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())
