"""
CPU checks of the NLCG test references: the float64 NumPy restatement of tests/_nlcg_refs.py reproduces the upstream
reference's own float64 trajectories (tests/golden/nlcg_*.npz: x and ||g|| at 1e-10 relative, every step size
exactly; measured <= 6e-13), and every case the GPU tests use satisfies the comparability conditions stated there.
"""
import numpy as np
import pytest
from conftest import load_golden

import _nlcg_refs as N


@pytest.fixture(scope="module", params=list(N.CASES))
def case(request):
    name = request.param
    gold = load_golden(N.CASES[name][0])
    return name, gold, N.run_case(name, gold)


def test_restatement_matches_reference_f64(case):
    name, gold, res = case
    assert np.array_equal(res["ls_a_k"], gold["ls_a_k"]), name
    ex = N.row_rel(res["x"], gold["x"])
    eg = float(np.abs(res["gnorm"] / gold["gnorm"] - 1.0).max())
    print(name, "x", ex, "gnorm", eg)
    assert ex <= 1e-10 and eg <= 1e-10


def test_step_sizes_are_a0_times_powers_of_r(case):
    name, gold, res = case
    a0, r = float(gold["a0"]), float(gold["r"])
    assert np.array_equal(res["ls_a_k"], a0 * r ** res["halvings"].astype(np.float64))


def test_conditions(case):
    name, gold, res = case
    pr = str(gold["variant"]).lower() == "pr"
    print(name, {k: res[k] for k in ("armijo_margin", "gp_max", "pr_margin", "max_backtracks", "rows_differ", "clipped",
                                     "unclipped", "restarts")})
    assert res["armijo_margin"] >= N.ARMIJO_MARGIN
    assert res["gp_max"] < 0
    assert res["max_backtracks"] >= 2
    assert res["rows_differ"]
    if pr:
        assert res["pr_margin"] >= N.PR_MARGIN
        assert res["clipped"] > 0 and res["unclipped"] > 0
    if "A" in gold:  # the restarts are covered by the Q cases (T-PR keeps restart_rate 100)
        assert res["restarts"] >= 1


def test_f32_admission(case):
    """A case runs in f32 on the GPU only if the reference's own f32 run stays with the float64 restatement."""
    name, gold, res = case
    err = N.row_rel(gold["x_f32"], res["x"])
    print(name, "reference f32 vs restatement", err)
    if N.CASES[name][1]:
        assert err <= N.F32_ADMIT


def test_public_names_exist():
    import pyxu_amd.math
    import pyxu_amd.opt.solver

    assert callable(pyxu_amd.math.backtracking_linesearch)
    assert pyxu_amd.math.LINESEARCH_DEFAULT_R == 0.5 and pyxu_amd.math.LINESEARCH_DEFAULT_C == 1e-4
    assert isinstance(pyxu_amd.opt.solver.NLCG, type)
