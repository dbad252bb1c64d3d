"""The float64 restatement of the svdvals Lanczos (tests/_svdvals_refs.py) against numpy.linalg.svd on the cases the
device tests use, with the conditions that make those cases comparable: the wanted values are separated from the
unwanted ones by at least 10x the bound, and the cycle cap is not reached.  No GPU."""
import numpy as np
import pytest

import _svdvals_refs as R

EPS = float(np.finfo(np.float64).eps)

# name -> (matrix, k, which, most restart cycles the case may take)
CASES = {
    "A1-LM": (R.matrix_a1, 4, "LM", 12),
    "A1-SM": (R.matrix_a1, 4, "SM", 80),
    "A1T-LM": (lambda: R.matrix_a1(True), 4, "LM", 12),
    "A1T-SM": (lambda: R.matrix_a1(True), 4, "SM", 80),
    "A2-LM": (R.matrix_a2, 3, "LM", 6),
    "A3-LM": (R.matrix_a3, 5, "LM", 2),
    "A3-SM": (R.matrix_a3, 5, "SM", 2),
    "A4-LM": (R.matrix_a4, 3, "LM", 2),
    "A4-SM": (R.matrix_a4, 3, "SM", 2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_svd(name):
    make, k, which, max_cycles = CASES[name]
    A = make()
    s_all = np.sort(np.linalg.svd(A, compute_uv=False))
    n = min(A.shape)
    bound = R.sq_bound(A.shape, s_all[-1], EPS)
    got, cycles, napply = R.lanczos_svdvals(A, k, which)
    ref = R.svd_ref(A, k, which)
    print(f"{name}: cycles {cycles}, applications {napply}, max |d sigma^2| {np.abs(got**2 - ref**2).max():.3e}, bound {bound:.3e}")
    assert got.shape == (k,) and np.all(np.diff(got) >= 0)
    assert np.all(np.abs(got**2 - ref**2) <= bound)
    assert cycles <= max_cycles < 10 * n  # well inside the cap
    # comparability: the gap between the wanted and the unwanted squares is at least 10x the bound (a repeated or
    # null value on both sides of the cut, as in A3 / A4, is the same value and needs no gap)
    sq = s_all**2
    inner, outer = (sq[n - k], sq[n - k - 1]) if which == "LM" else (sq[k - 1], sq[k])
    gap = abs(inner - outer)
    assert gap >= 10 * bound or gap <= bound


def test_forced_restart_small_ncv():
    A = R.matrix_a1()
    got, cycles, _ = R.lanczos_svdvals(A, 4, "LM", ncv=12)
    assert cycles > 1
    assert np.all(np.abs(got**2 - R.svd_ref(A, 4, "LM") ** 2) <= R.sq_bound(A.shape, 9.0, EPS))


def test_cycle_cap_raises():
    with pytest.raises(RuntimeError, match="converged"):
        R.lanczos_svdvals(R.matrix_a1(), 4, "SM", maxiter=1)


def test_breakdown_returns_null_values():
    got, _, _ = R.lanczos_svdvals(R.matrix_a3(), 5, "SM")
    assert np.all(got <= np.sqrt(R.sq_bound((40, 30), 44.0, EPS)))
    got, _, _ = R.lanczos_svdvals(R.matrix_a3(), 5, "LM")
    assert np.allclose(got[2:], [30.0, 33.0, 44.0], rtol=1e-12)


def test_float32_restatement_within_float32_bound():
    eps32 = float(np.finfo(np.float32).eps)
    for make, k, which in ((R.matrix_a1, 4, "LM"), (R.matrix_a2, 3, "LM"), (R.matrix_a3, 5, "LM")):
        A = make()
        got, _, _ = R.lanczos_svdvals(A, k, which, dtype=np.float32)
        ref = R.svd_ref(A, k, which)
        assert np.all(np.abs(got**2 - ref**2) <= R.sq_bound(A.shape, ref[-1], eps32))
