"""
PD3O / Condat-Vu on halo-exchanged slab operators (SlabLinOp(Stencil), SlabLinOp(Gradient), ShardedRelError): worlds
of 2 and 3 processes sharing cuda:0 over gloo, so that an interior rank exists.  The problem is the (17, 9, 11) volume
with off-centre taps on every axis (axis-0 reach 2) and per-axis sampling.

The fused slab step must reproduce the unsharded fused solver bit for bit (the slab step evaluates the same
expressions on the same values; S^T y is summed in the unsharded order), stop at the same iteration and use the same
step sizes on every rank.  The generic rule-by-rule path on the slab operators is held to the project's parity bound
against the unsharded CPU oracle: 1e-5 norm-wise relative after 8 iterations (conftest.rel_err).
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import _asym_cases as ac  # noqa: E402
import _slab_workers as sw  # noqa: E402


@pytest.mark.parametrize("steps", ["explicit", "default"])
@pytest.mark.parametrize("algo", ["pd3o", "cv"])
@pytest.mark.parametrize("world", [2, 3])
def test_fused_slab_solver_is_the_unsharded_solver(world, algo, steps):
    res = sw.spawn("gpu_slab_solver", world=world, algo=algo, steps=steps)
    ref = res[0]
    print(f"iterations {ref['it']} (unsharded {ref['it_ref']}), tau / sigma / rho {ref['steps']}")
    assert 2 < ref["it_ref"] < 40, "the stop must be decided by the RelError criterion, not by MaxIter"
    for r in range(world):
        assert res[r]["plan"] == "slab" and res[r]["la"] is False, r
        assert res[r]["it"] == ref["it_ref"], (r, res[r]["it"], ref["it_ref"])
        assert res[r]["steps"] == ref["steps_ref"], (r, res[r]["steps"], ref["steps_ref"])
        np.testing.assert_array_equal(res[r]["x"], ref["x_ref"])


@pytest.mark.parametrize("algo", ["pd3o", "cv"])
def test_generic_path_on_slabs_matches_the_oracle(algo):
    """fused=False on slab operators, 8 iterations, against oracle/pyxu_np.py on the whole volume."""
    res = sw.spawn("gpu_slab_solver", world=3, algo=algo, steps="explicit", fused=False, iters=ac.PDS_ITERS)
    tau, sigma, rho = res[0]["steps"]
    dt = np.float32
    xr, _ = ac.oracle_pds(sw.entry(), algo, "iso", "pos", dt, (dt(tau), dt(sigma), dt(rho)), n=ac.PDS_ITERS)
    for r in range(3):
        assert res[r]["plan"] is None and res[r]["it"] == ac.PDS_ITERS
        err = rel_err(res[r]["x"], xr)
        print(f"rank {r}: rel_err {err:.3e}")
        assert err <= 1e-5, (r, err)


@pytest.mark.parametrize("algo", ["pd3o", "cv"])
def test_world_of_one_takes_the_plain_plan(algo):
    res = sw.spawn("gpu_slab_solver", world=1, algo=algo, steps="default")[0]
    assert res["plan"] == "plain" and res["la"] is True
    assert res["it"] == res["it_ref"] and res["steps"] == res["steps_ref"]
    np.testing.assert_array_equal(res["x"], res["x_ref"])


def test_thin_slab_raises_on_every_rank():
    res = sw.spawn("gpu_slab_thin", world=3, algo="pd3o")
    assert [res[r]["nl"] for r in range(3)] == [3, 2, 2]
    for r in range(3):
        assert res[r]["raised"] is not None and "thinner" in res[r]["raised"], r
