"""
CPU checks of the ProxAdam test references: the float64 NumPy restatement of tests/_proxadam_refs.py reproduces the
upstream reference's own float64 results (tests/golden/proxadam_*.npz: final x at 1e-12 relative per row), every case
with a prox that the GPU tests use satisfies the comparability conditions stated there, and a case is admitted for
float32 only where the reference's own float32 run stays with the restatement.
"""
import numpy as np
import pytest
from conftest import load_golden

import _proxadam_refs as P


@pytest.fixture(scope="module", params=list(P.CASES))
def case(request):
    name = request.param
    gold = load_golden(P.CASES[name][0])
    return name, gold, P.run_case(name, gold)


def test_restatement_matches_reference_f64(case):
    name, gold, res = case
    err = P.row_rel(res["x"], gold["x"])
    print(name, "x", err)
    assert err <= 1e-12


def test_conditions(case):
    name, gold, res = case
    if not P.with_g(name):
        assert res["counts"].size == 0
        return
    print(name, {k: res[k] for k in ("stop_margin", "rows_differ", "max_count")}, res["counts"].tolist())
    assert res["counts"].shape == (int(gold["iters"]), gold["x0"].shape[0])
    assert res["stop_margin"] >= P.STOP_MARGIN
    assert res["rows_differ"]
    assert res["max_count"] >= 3


def test_f32_admission(case):
    """A case runs in f32 on the GPU only if the reference's own f32 run stays with the float64 restatement."""
    name, gold, res = case
    err = P.row_rel(gold["x_f32"], res["x"])
    print(name, "reference f32 vs restatement", err)
    if P.CASES[name][1]:
        assert err <= P.F32_ADMIT


def test_cases_cover_the_variants_and_prox_kinds():
    golds = {name: load_golden(P.CASES[name][0]) for name in P.CASES}
    with_g = {(str(g["variant"]), str(g["g_kind"])) for n, g in golds.items() if P.with_g(n)}
    assert {v for v, _ in with_g} == {"adam", "amsgrad", "padam"}
    assert {k for _, k in with_g} == set(P.KINDS)
    assert {str(g["variant"]) for n, g in golds.items() if not P.with_g(n)} == {"adam", "amsgrad", "padam"}
    assert any(bool(g["use_v0"]) for g in golds.values())


def test_v0_does_not_reach_variance_hat():
    """The reference's first step takes variance_hat = variance whatever v0 was: with max(v0, v') instead the v0 case
    ends elsewhere."""
    gold = load_golden(P.CASES["ams-l1-v0"][0])
    res = P.run_case("ams-l1-v0", gold)
    v1 = np.clip(0.999 * gold["v0"] + 0.001 * P.objective_Q(gold["A"], gold["b"])(gold["x0"]) ** 2, 1e-6, None)
    assert (v1 < gold["v0"]).sum() >= 10  # (there max(v0, v') = v0 != v': the two rules differ from the first step on)
    assert P.row_rel(res["x"], gold["x"]) <= 1e-12


def test_sub_solve_cap_runs_exactly_that_many_iterations():
    gold = load_golden(P.CASES["padam-l1"][0])
    res = P.run_case("padam-l1", gold, sub_max_iter=4)
    assert (res["counts"] == 4).all()


def test_partition_helpers():
    assert P.blocks_per_row(1, 4096) == 1 and P.blocks_per_row(1, 4097) == 2
    assert P.blocks_per_row(4097, 5) == 1 and P.blocks_per_row(1, 2**24) == 1024
    assert P.chunk(np.float32, 1, 4097) == 2052 and P.chunk(np.float64, 1, 4097) == 2050


def test_public_names_exist():
    import pyxu_amd.opt.solver
    import pyxu_amd.opt.solver.prox_adam as mod

    assert isinstance(pyxu_amd.opt.solver.ProxAdam, type)
    assert mod._FUSED is True
