"""
CPU checks of the sampler test references (tests/_sampler_refs.py): Philox4x32-10 known answers, the restated step
against the upstream reference's own ULA / MYULA runs (tests/golden/sampler_*.npz), the conditions under which the GPU
tests may compare the online statistics across precisions, the evidence for the declared skewness / kurtosis deviation,
and the statistical quality of the restated normals and of a restated ULA chain.
"""
import numpy as np
import pytest
from conftest import load_golden

import _sampler_refs as S

DT = {"f32": np.float32, "f64": np.float64}


def _words(ctr, key):
    return tuple(int(w[0]) for w in S.philox4x32_10(ctr, key))


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, out):
    assert _words(ctr, key) == out


def test_normals_depend_on_the_global_element_only():
    for dt in DT.values():
        full = S.normals(dt, 9, 4, 0, 64)
        assert np.array_equal(S.normals(dt, 9, 4, 3, 6), full[3:9])
        assert np.array_equal(S.normals(dt, 9, 4, 0, 5), full[:5])
        assert not np.array_equal(S.normals(dt, 10, 4, 0, 64), full)
        assert not np.array_equal(S.normals(dt, 9, 5, 0, 64), full)
        assert not np.array_equal(S.normals(dt, 9, 4 + 2**32, 0, 64), full)
        assert not np.array_equal(S.normals(dt, 9, 4, 2**32, 64), full)


@pytest.fixture(scope="module", params=S.CASES)
def case(request):
    return request.param, load_golden(f"sampler_{request.param}")


@pytest.mark.parametrize("steps", [1, 6])
def test_step_matches_reference_f64(case, steps):
    name, gold = case
    got = S.run_case(gold, np.float64, steps)
    err = S.max_norm_err(got, gold[f"x{steps}"])
    print(name, steps, err)
    assert err <= 1e-10


@pytest.mark.parametrize("steps", [1, 6])
def test_step_matches_reference_f32(case, steps):
    """At 1e-5, not bit for bit: the restated gradient's matrix products are summed in the order of whatever BLAS runs
    this test, not the one that recorded the golden, and for "l1" / "posl1" the reference forms x - prox(x), which
    cancels where the kernel's clip / min form is exact (see test_first_step_bits_f32 for what is bit-exact)."""
    name, gold = case
    got = S.run_case(gold, np.float32, steps)
    err = S.max_norm_err(got, gold[f"x{steps}_f32"])
    print(name, steps, err)
    assert got.dtype == np.float32
    assert err <= 1e-5


def test_first_step_bits_f32(case):
    """From the reference's own float32 gradient at x0 the restated step gives the reference's first float32 sample bit
    for bit, for every kind whose Moreau-Yosida term the reference forms without cancellation."""
    name, gold = case
    got = S.run_case(gold, np.float32, 1, grad0=gold["grad0_f32"])
    same = np.array_equal(got.view(np.uint32), gold["x1_f32"].view(np.uint32))
    print(name, "bit-equal" if same else S.max_norm_err(got, gold["x1_f32"]))
    if name in S.EXACT_F32:
        assert same
    else:
        assert S.max_norm_err(got, gold["x1_f32"]) <= 1e-5


def test_cases_straddle_the_thresholds():
    """Both sides of every kind's thresholds occur in the golden chains' starting points."""
    for name in S.CASES:
        gold = load_golden(f"sampler_{name}")
        x, kind = gold["x0"], str(gold["kind"])
        t = float(gold["lamb"]) * float(gold["pw"])
        if kind == "l1":
            assert (x < -t).any() and (np.abs(x) < t).any() and (x > t).any()
        elif kind == "pos":
            assert (x < 0).any() and (x > 0).any()
        elif kind == "posl1":
            assert (x < t).any() and (x > t).any()
        elif kind == "box":
            pw = float(gold["pw"])
            assert (x < -pw).any() and (np.abs(x) < pw).any() and (x > pw).any()


# ------------------------------------------------------------------------------------------------ statistics
STATS = ("m1", "m2", "var", "std", "cm3", "cm4")


@pytest.fixture(scope="module")
def stats():
    return load_golden("sampler_stats")


def test_golden_f32_statistics_stay_with_f64(stats):
    for name in STATS:
        err = S.max_norm_err(stats[f"{name}_f32"], stats[name])
        print(name, err)
        assert err <= 1e-5


def test_reference_centred_moments_match_the_direct_formula(stats):
    for name, r in (("var", 2), ("cm3", 3), ("cm4", 4)):
        err = S.max_norm_err(stats[name], stats[f"direct_{name}"])
        print(name, err)
        assert err <= 1e-10
        assert S.max_norm_err(S.direct_moment(stats["samples"], r), stats[f"direct_{name}"]) <= 1e-14


def test_reference_kurtosis_composite_is_not_the_kurtosis(stats):
    """The evidence for the declared deviation: the reference's composite calls its divisor's update three times per
    sample and ends far from mu_4 / mu_2^2 (and its skewness from mu_3 / mu_2^(3/2))."""
    kurt = S.direct_standardized(stats["samples"], 4)
    gap = float(np.abs(stats["kurt"] - kurt).max())
    print("kurtosis gap", gap, "skewness gap", float(np.abs(stats["skew"] - S.direct_standardized(stats["samples"], 3)).max()))
    assert gap > 1e-3


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("order", [2, 3, 4])
def test_restated_welford_matches_reference(stats, d, order):
    dt = DT[d]
    mean, sums = S.welford(dt, stats["samples"], order)
    K = stats["samples"].shape[0]
    names = {2: "var", 3: "cm3", 4: "cm4"}
    for r in range(2, order + 1):
        ref = stats[names[r] + ("_f32" if d == "f32" else "")]
        err = S.max_norm_err(sums[r - 2] / K, ref)
        err_direct = S.max_norm_err(sums[r - 2] / K, S.direct_moment(stats["samples"], r))
        print(d, order, r, err, err_direct)
        assert err <= S.TOL[dt] and err_direct <= S.TOL[dt]
    assert S.max_norm_err(mean, stats["m1"]) <= S.TOL[dt]


# ------------------------------------------------------------------------------------------------ the normals
@pytest.mark.parametrize("d", list(DT))
def test_restated_normals_are_standard_normal(d):
    N = 2**20
    z = S.normals(DT[d], 1, 0, 0, N)
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var**2
    corr = np.corrcoef(z[0::2], z[1::2])[0, 1]
    print(d, mean, var, kurt, corr)
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert abs(kurt - 3) <= 5 * np.sqrt(24 / N)
    assert abs(corr) <= 5 / np.sqrt(N / 2)


def test_restated_ula_reaches_the_stationary_variance():
    var = S.ula_gaussian_variance(S.ULA_N, S.ULA_GAMMA, S.ULA_STEPS, S.ULA_SEED,
                                  lambda k: S.normals(np.float64, S.ULA_SEED, k, 0, S.ULA_N))
    print(var, S.ULA_VAR, S.ULA_BOUND)
    assert abs(var - S.ULA_VAR) <= S.ULA_BOUND


def test_ula_check_catches_reused_noise_and_a_wrong_scale():
    """The variance check fails when every step reuses the first step's noise, and when sqrt(2 gamma) is sqrt(gamma)."""
    z0 = S.normals(np.float64, S.ULA_SEED, 0, 0, S.ULA_N)
    reused = S.ula_gaussian_variance(S.ULA_N, S.ULA_GAMMA, S.ULA_STEPS, S.ULA_SEED, lambda k: z0)
    scaled = S.ula_gaussian_variance(S.ULA_N, S.ULA_GAMMA, S.ULA_STEPS, S.ULA_SEED,
                                     lambda k: S.normals(np.float64, S.ULA_SEED, k, 0, S.ULA_N) / np.sqrt(2.0))
    print(reused, scaled)
    assert abs(reused - S.ULA_VAR) > S.ULA_BOUND
    assert abs(scaled - S.ULA_VAR) > S.ULA_BOUND
