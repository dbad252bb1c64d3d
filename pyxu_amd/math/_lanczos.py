"""
Thick-restart Lanczos for the extreme singular values of a LinOp (``LinOp.svdvals(k, which)``), every vector on the
device.

The method runs on the smaller Gram operator (``op.gram()`` if codim >= dim, else ``op.cogram()``, so specialised
grams such as the NUFFT Toeplitz one are used) and returns sqrt(max(theta, 0)) of its k largest ("LM") or smallest
("SM") Ritz values.  The basis V is a row-major (ncv + 1, n) device array, ncv = min(n, max(2 k + 1, 20)) <= 64.

One step j after the operator product w = G v_j is two classical Gram-Schmidt passes against rows 0 .. j:
``pxa_krylov_dots``, ``pxa_krylov_update`` (with the next coefficients), ``pxa_krylov_update`` (with ||w||^2, written
straight into row j + 1) and ``pxa_krylov_normalize`` from the device value: no host read inside a cycle.  alpha_j
(the sum of the two coefficients on row j) and beta_j^2 stay in a device buffer that one copy brings to the host at
the end of the cycle, where the (ncv, ncv) projected matrix (kept Ritz values, their couplings, the tridiagonal rest)
is diagonalised in float64 with ``numpy.linalg.eigh``.

* Convergence: |beta_last s_last,i| <= tol max|theta| for the wanted pairs (tol = 0: 32 eps); ncv == n is exact after
  one cycle.
* Restart: k + (ncv - k) // 2 Ritz vectors S^T V by one ``pxa_dense_matmat``, the residual vector as the next row.
* Breakdown: the first beta_j <= 64 eps max|T| of a cycle marks an invariant subspace; beta_j = 0, row j + 1 becomes
  a fresh host-drawn vector orthogonalised twice against rows 0 .. j, and the cycle is redone from step j + 1.
* "SM" has no shift-invert: it needs iterations on the order of the Gram's condition number, and the ``maxiter``
  RuntimeError is the expected outcome for an ill-conditioned operator.

``_FUSED = False`` runs the same algorithm with the Gram-Schmidt passes composed from ``pxa_dense_matmat`` /
``pxa_axpby`` / ``pxa_row_reduce`` (seven launches per step, coefficients in the runtime precision): the A/B
reference of scripts/bench_svdvals.py and of the parity test.
"""
import numpy as np

import pyxu_amd.runtime as pxrt
from pyxu_amd import _dev

__all__ = ["lanczos_svdvals"]

_FUSED = True
MAX_NCV = 64
_NRM = MAX_NCV  # column of the coefficient buffer that holds ||w''||^2


class _Basis:
    """The device state of one solve: basis rows, coefficient rows and the two Gram-Schmidt chains."""

    def __init__(self, n, ncv, like, fused):
        torch = _dev._torch()
        self.n, self.ncv, self.fused = n, ncv, fused
        vec = 16 // like.element_size()
        # fused: rows padded to whole 16-byte vectors (the kernels' vector path); composed: V[:j] is a dense matrix
        self.ld = -(-n // vec) * vec if fused else n
        self.V = torch.zeros((ncv + 1, self.ld), dtype=like.dtype, device=like.device)
        # coef[p, j, :j + 1]: pass p's coefficients of step j (row ncv: the breakdown replacement); [1, j, _NRM]: ||w''||^2
        self.coef = torch.zeros((2, ncv + 1, MAX_NCV + 1), dtype=torch.float64, device=like.device)
        self.tmp = torch.empty((n,), dtype=like.dtype, device=like.device)
        self.work = _dev.krylov_workspace(min(ncv + 1, MAX_NCV), n, like) if fused else None

    def row(self, j):
        return self.V[j, : self.n]

    def orthonormalise(self, rows, w, slot):
        """Row `rows` of V = w orthogonalised twice against rows 0 .. rows - 1 and normalised; the coefficients and
        ||w''||^2 go to coefficient row `slot`.  No host read."""
        c1, c2, nrm2 = self.coef[0, slot], self.coef[1, slot], self.coef[1, slot, _NRM:]
        out = self.row(rows)
        if self.fused:
            Vn = self.V[:, : self.n]
            _dev.krylov_dots(Vn, rows, w, c1, self.work)
            _dev.krylov_update(Vn, rows, w, c1, self.tmp, self.work, c_next=c2)
            _dev.krylov_update(Vn, rows, self.tmp, c2, out, self.work, nrm2_out=nrm2)
        else:
            Vj = self.V[:rows]
            for c in (c1, c2):
                ct = _dev.dense_matmat(Vj, w.reshape(1, -1), 0)  # (1, rows) = w Vj^T
                w = _dev.axpby(1.0, w, -1.0, _dev.dense_matmat(Vj, ct, 1).reshape(-1))
                c[:rows].copy_(ct.reshape(-1))
            _dev.row_reduce(_dev.RED_SUMSQ, w.reshape(1, -1), out=nrm2)
        _dev.krylov_normalize(w if not self.fused else out, nrm2, out)


def _host_vector(v0, rng, n):
    if v0 is None:
        v = rng.standard_normal(n)
    else:
        v = np.asarray(v0.cpu() if hasattr(v0, "cpu") else v0, dtype=np.float64).reshape(-1)
        if v.size != n:
            raise ValueError(f"v0: expected {n} entries, got {v.size}.")
    nv = np.linalg.norm(v)
    if not nv > 0:
        raise ValueError("v0: a non-zero start vector is needed.")
    return v / nv


def lanczos_svdvals(op, k, which="LM", ncv=None, tol=0.0, maxiter=None, v0=None, seed=0, _stats=None):
    """The k largest ("LM") / smallest ("SM") singular values of `op`, ascending, as a (k,) array of the runtime
    precision.  `_stats`: a dict that receives cycles / applications (operator products with the Gram)."""
    from pyxu_amd.util import to_device

    dtype = pxrt.getPrecision().value
    eps = float(np.finfo(dtype).eps)
    small_gram = op.codim >= op.dim
    G = op.gram() if small_gram else op.cogram()
    n = min(op.shape)
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"k: expected 1 <= k <= {n}, got {k}.")
    ncv = min(n, max(2 * k + 1, 20), MAX_NCV) if ncv is None else int(min(max(int(ncv), min(k + 1, n)), n, MAX_NCV))
    if k > ncv:
        raise ValueError(f"k = {k} exceeds the largest supported subspace ({MAX_NCV}).")
    tol = 32 * eps if not tol else float(tol)
    maxiter = 10 * n if maxiter is None else int(maxiter)
    rng = np.random.default_rng(int(seed or 0))
    start_vec = to_device(_host_vector(v0, rng, n).astype(dtype))
    B = _Basis(n, ncv, start_vec, _FUSED)
    B.row(0).copy_(start_vec)
    kept, theta_kept, coupling = 0, np.zeros(0), np.zeros(0)
    napply = nconv = 0
    amax = lambda a: float(np.abs(a).max(initial=0.0))
    with pxrt.EnforcePrecision(False):
        for cycle in range(1, maxiter + 1):
            start, broken = kept, []  # broken: the steps of this cycle whose beta was set to 0
            while True:
                for j in range(start, ncv):
                    w = _dev.require(G.apply(B.row(j))).reshape(-1)
                    napply += 1
                    B.orthonormalise(j + 1, w, j)
                coef = B.coef.cpu().numpy()  # the cycle's one device-to-host copy
                idx = np.arange(ncv)
                alpha = coef[0, idx, idx] + coef[1, idx, idx]
                beta = np.sqrt(np.maximum(coef[1, :ncv, _NRM], 0.0))
                beta[broken] = 0.0
                broke = None
                for j in range(start, ncv):
                    scale = max(amax(theta_kept), amax(coupling), amax(alpha[kept:j + 1]), amax(beta[kept:j]))
                    if not beta[j] > 64 * eps * scale:
                        broke = j
                        break
                if broke is None:
                    break
                broken.append(broke)
                beta[broke] = 0.0
                B.orthonormalise(broke + 1, to_device(rng.standard_normal(n).astype(dtype)), ncv)
                if broke == ncv - 1:
                    break
                start = broke + 1
            T = np.zeros((ncv, ncv))
            T[np.arange(kept), np.arange(kept)] = theta_kept
            if kept < ncv:
                T[kept, :kept] = coupling
                T[:kept, kept] = coupling
            for j in range(kept, ncv):
                T[j, j] = alpha[j]
                if j + 1 < ncv:
                    T[j, j + 1] = T[j + 1, j] = beta[j]
            theta, S = np.linalg.eigh(T)
            want = slice(ncv - k, ncv) if which == "LM" else slice(0, k)
            resid = np.abs(beta[ncv - 1] * S[ncv - 1, :])
            ok = resid[want] <= tol * amax(theta)
            nconv = int(ok.sum())
            if ok.all() or ncv == n:
                if _stats is not None:
                    _stats.update(cycles=cycle, applications=napply, ncv=ncv)
                return np.sqrt(np.maximum(np.sort(theta[want]), 0.0)).astype(dtype)
            keep = min(k + (ncv - k) // 2, ncv - 1)
            sel = np.arange(ncv - keep, ncv) if which == "LM" else np.arange(keep)
            Y = _dev.dense_matmat(B.V[:ncv], to_device(np.ascontiguousarray(S[:, sel].T).astype(dtype)), 1)
            B.V[keep].copy_(B.V[ncv])
            B.V[:keep].copy_(Y)
            theta_kept, coupling, kept = theta[sel], beta[ncv - 1] * S[ncv - 1, sel], keep
    if _stats is not None:
        _stats.update(cycles=maxiter, applications=napply, ncv=ncv)
    raise RuntimeError(f"svdvals: {nconv} of {k} singular values converged in {maxiter} restart cycles "
                       f"(which={which!r}, ncv={ncv}, tol={tol:.3g}).")
