"""
The Langevin samplers on the device (csrc/sampler.hip, pyxu_amd/experimental/sampler) against the NumPy restatement of
tests/_sampler_refs.py and the upstream reference's goldens (tests/golden/sampler_*.npz), whose comparability
conditions tests/test_sampler_refs.py asserts.  Sizes cross every path edge of the kernels: below, at and above one
16-byte group, one wavefront and one workgroup, a range that is no whole number of groups, several workgroups; every
operand is also taken as a view one element into its allocation, which forces the element-by-element path.
"""
import numpy as np
import pytest
from conftest import load_golden

import _prim_refs as R
import _sampler_refs as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.experimental.sampler as pxes  # noqa: E402
import pyxu_amd.experimental.sampler._sampler as smod  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.util import to_NUMPY  # noqa: E402

DT = {"f32": np.float32, "f64": np.float64}
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027, 65539)
N, M = 17, 24
LAM, PW = 0.25, 0.6  # t = lam pw = 0.15


def W(dt):
    return pxrt.Width.SINGLE if dt == np.float32 else pxrt.Width.DOUBLE


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def fill_normals(dt, n, seed, step, e0=0, off=0):
    """pxa_philox_normal into a guarded buffer, as a host array; the guards are checked."""
    base, view = R.placed(np.zeros(n, dtype=dt), off)
    _dev.philox_normal(view, seed, step, e0)
    assert R.guards_intact(base, off, n)
    return R.to_host(view)


# ------------------------------------------------------------------------------------------------ pxa_philox_normal
@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("n", SIZES)
def test_normals_match_restatement(d, n):
    dt = DT[d]
    ref = S.normals(dt, 5, 2, 0, n)
    got = fill_normals(dt, n, 5, 2)
    err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(d, n, err)
    assert got.dtype == dt
    assert err <= S.TOL[dt]
    assert same_bits(fill_normals(dt, n, 5, 2, off=1), got)  # the element-by-element path
    assert same_bits(fill_normals(dt, n, 5, 2), got)  # the same call again


@pytest.mark.parametrize("d", list(DT))
def test_normals_are_a_function_of_the_global_element(d):
    dt = DT[d]
    full = fill_normals(dt, 1027, 5, 2)
    assert same_bits(fill_normals(dt, 5, 5, 2), full[:5])
    for off in (0, 1):  # a range that starts and ends inside a group
        assert same_bits(fill_normals(dt, 6, 5, 2, e0=3, off=off), full[3:9])
        assert same_bits(fill_normals(dt, 1, 5, 2, e0=2, off=off), full[2:3])
        assert same_bits(fill_normals(dt, 1020, 5, 2, e0=7, off=off), full[7:])
    assert not same_bits(fill_normals(dt, 1027, 6, 2), full)
    assert not same_bits(fill_normals(dt, 1027, 5, 3), full)
    assert not same_bits(fill_normals(dt, 1027, 5 + 2**32, 2), full)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("step,e0", [(2**32 - 1, 0), (2**32, 0), (0, 2**32 - 2), (0, 2**34 + 1), (2**40 + 3, 2**34 + 1)])
def test_normals_with_wide_counters(d, step, e0):
    dt = DT[d]
    n = 11
    ref = S.normals(dt, 2**63 + 12345, step, e0, n)
    for off in (0, 1):
        got = fill_normals(dt, n, 2**63 + 12345, step, e0=e0, off=off)
        err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(d, step, e0, off, err)
        assert err <= S.TOL[dt]


# ------------------------------------------------------------------------------------------------ pxa_langevin_step
def step_inputs(dt, n, kind):
    """x on both sides of t, of 0 and of pw (and on t and pw themselves), grad and noise."""
    r = R.rng_for("sampler-step", n, np.dtype(dt).name, kind)
    x = r.standard_normal(n)
    t = LAM * PW
    edge = np.array([-2 * t, -t, -0.5 * t, 0.5 * t, t, 2 * t, -2 * PW, -PW, -0.5 * PW, 0.5 * PW, PW, 2 * PW, 1e-30, -1e-30])
    k = min(n, edge.size)
    x[:k] = r.permutation(edge)[:k]
    return x.astype(dt), r.standard_normal(n).astype(dt), r.standard_normal(n).astype(dt)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_step_with_supplied_noise_is_bit_equal(d, kind):
    dt = DT[d]
    for n in SIZES:
        x, g, z = step_inputs(dt, n, kind)
        ref = S.step(dt, kind, x, g, z, 0.1, LAM, PW)
        for off in (0, 1):
            (_, xv), (_, gv), (_, zv) = (R.placed(a, off) for a in (x, g, z))
            base, out = R.placed(np.zeros(n, dtype=dt), off)
            _dev.langevin_step(S.KINDS[kind], 0.1, LAM, PW, xv, gv, out, noise=zv)
            assert R.guards_intact(base, off, n)
            assert same_bits(R.to_host(out), ref), (kind, d, n, off, "out of place")
            assert same_bits(R.to_host(xv), x)
            base, xv2 = R.placed(x, off)
            _dev.langevin_step(S.KINDS[kind], 0.1, LAM, PW, xv2, gv, xv2, noise=zv)
            assert R.guards_intact(base, off, n)
            assert same_bits(R.to_host(xv2), ref), (kind, d, n, off, "in place")


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("kind", ["none", "l1", "box"])
def test_step_with_device_noise_equals_supplied_philox(d, kind):
    dt = DT[d]
    seed, step = 77, 2**32 + 5
    for n in SIZES:
        x, g, _ = step_inputs(dt, n, kind)
        for off, e0 in ((0, 0), (1, 0), (0, 3), (1, 2**34 + 1)):
            (_, xv), (_, gv) = (R.placed(a, off) for a in (x, g))
            _, zv = R.placed(np.zeros(n, dtype=dt), 0)
            _dev.philox_normal(zv, seed, step, e0)
            _, want = R.placed(np.zeros(n, dtype=dt), 0)
            _dev.langevin_step(S.KINDS[kind], 0.1, LAM, PW, xv, gv, want, noise=zv)
            base, out = R.placed(np.zeros(n, dtype=dt), off)
            _dev.langevin_step(S.KINDS[kind], 0.1, LAM, PW, xv, gv, out, seed=seed, step=step, e0=e0)
            assert R.guards_intact(base, off, n)
            assert same_bits(R.to_host(out), R.to_host(want)), (kind, d, n, off, e0)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_step_keeps_a_nan_in_its_element(d, kind):
    dt = DT[d]
    n = 259
    x, g, z = step_inputs(dt, n, kind)
    clean = S.step(dt, kind, x, g, z, 0.1, LAM, PW)
    x[[2, 130]] = np.nan
    g[[7, 258]] = np.nan
    for off in (0, 1):
        (_, xv), (_, gv), (_, zv) = (R.placed(a, off) for a in (x, g, z))
        _, out = R.placed(np.zeros(n, dtype=dt), off)
        got = R.to_host(_dev.langevin_step(S.KINDS[kind], 0.1, LAM, PW, xv, gv, out, noise=zv))
        bad = np.zeros(n, dtype=bool)
        bad[[2, 130, 7, 258]] = True
        assert np.isnan(got[bad]).all()
        assert same_bits(got[~bad], clean[~bad])


def test_step_rejects_bad_operands():
    x = R.to_dev(np.zeros(8, dtype=np.float32))
    with pytest.raises(ValueError):
        _dev.langevin_step(9, 0.1, 1.0, 0.0, x, x.clone(), x.clone())
    with pytest.raises(ValueError):
        g = x.clone()
        _dev.langevin_step(0, 0.1, 1.0, 0.0, x, g, g)
    with pytest.raises(ValueError):
        _dev.langevin_step(0, 0.0, 1.0, 0.0, x, x.clone(), x.clone())
    with pytest.raises(TypeError):
        _dev.philox_normal(np.zeros(4, dtype=np.float32), 1, 0)


# ------------------------------------------------------------------------------------------------ pxa_online_moments
STAT_NAME = {2: "var", 3: "cm3", 4: "cm4"}


@pytest.fixture(scope="module")
def stats():
    return load_golden("sampler_stats")


def run_moments(dt, samples, order, off=0):
    """K updates of pxa_online_moments; mean, x and sums taken `off` elements into their allocations."""
    K, n = samples.shape
    bm, mean = R.placed(np.zeros(n, dtype=dt), off)
    bs, sums = R.placed(np.zeros((order - 1) * n, dtype=np.float64), off)
    for k in range(K):
        _, xv = R.placed(samples[k].astype(dt), off)
        _dev.online_moments(order, k, xv, mean, sums)
    assert R.guards_intact(bm, off, n) and R.guards_intact(bs, off, (order - 1) * n)
    return R.to_host(mean), R.to_host(sums).reshape(order - 1, n)


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("order", [2, 3, 4])
def test_moments_match_reference_and_direct_formula(stats, d, order):
    dt = DT[d]
    samples = stats["samples"]
    K = samples.shape[0]
    mean, sums = run_moments(dt, samples, order)
    assert S.max_norm_err(mean, stats["m1"]) <= S.TOL[dt]
    for r in range(2, order + 1):
        got = sums[r - 2] / K
        err = S.max_norm_err(got, stats[STAT_NAME[r] + ("_f32" if d == "f32" else "")])
        err_direct = S.max_norm_err(got, S.direct_moment(samples, r))
        print(d, order, r, err, err_direct)
        assert err <= S.TOL[dt] and err_direct <= S.TOL[dt]


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("order", [2, 3, 4])
@pytest.mark.parametrize("n", [1027, 1028])
def test_moments_paths_agree(d, order, n):
    """Views one element into their allocations (element by element) against the aligned run (16-byte accesses at
    n = 1028; at n = 1027 the planes of orders 3 and 4 are not all aligned and that run goes element by element too),
    and both against the restatement."""
    dt = DT[d]
    samples = (R.rng_for("moments", n).gamma(2.0, 1.0, (4, n)) + 3.0).astype(dt)
    mean, sums = run_moments(dt, samples, order)
    mean_v, sums_v = run_moments(dt, samples, order, off=1)
    assert same_bits(mean, mean_v) and same_bits(sums, sums_v)
    ref_mean, ref_sums = S.welford(dt, samples, order)
    assert same_bits(mean, ref_mean)
    for r in range(2, order + 1):
        assert S.max_norm_err(sums[r - 2], ref_sums[r - 2]) <= 1e-14  # (NumPy's pow against repeated products)


# ------------------------------------------------------------------------------------------------ classes
def objective(gold, dt):
    return 0.5 * pxo.SquaredL2Norm(dim=M).asloss(R.to_dev(gold["b"].astype(dt))) * pxa.LinOp.from_array(
        R.to_dev(gold["A"].astype(dt)))


def g_of(kind, pw):
    if kind == "l1":
        return pw * pxo.L1Norm(dim=N)
    if kind == "pos":
        return pxo.PositiveOrthant(dim=N)
    if kind == "posl1":
        return pw * pxo.PositiveL1Norm(dim=N)
    if kind == "box":
        return pxo.LInfinityBall(dim=N, radius=pw)
    return None


def sampler_of(name, gold, dt):
    f = objective(gold, dt)
    if name == "ula":
        return pxes.ULA(f, gamma=float(gold["gamma"]))
    return pxes.MYULA(f, g_of(str(gold["kind"]), float(gold["pw"])), gamma=float(gold["gamma"]), lamb=float(gold["lamb"]))


def chain(name, gold, dt, rng, steps=6, fused=True):
    """The samples after 1 and after `steps` steps, as host arrays, and the sampler."""
    prev = smod._FUSED
    smod._FUSED = fused
    try:
        with pxrt.Precision(W(dt)):
            s = sampler_of(name, gold, dt)
            gen = s.samples(rng=rng, x0=R.to_dev(gold["x0"].astype(dt)))
            xs = [next(gen) for _ in range(steps)]
            return to_NUMPY(xs[0]), to_NUMPY(xs[-1]), s
    finally:
        smod._FUSED = prev


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("name", S.CASES)
def test_chain_matches_reference(name, d):
    dt = DT[d]
    gold = load_golden(f"sampler_{name}")
    sfx = "_f32" if d == "f32" else ""
    runs = {fused: chain(name, gold, dt, np.random.default_rng(int(gold["seed"])), fused=fused) for fused in (True, False)}
    for fused, (x1, x6, _) in runs.items():
        e1, e6 = S.max_norm_err(x1, gold["x1" + sfx]), S.max_norm_err(x6, gold["x6" + sfx])
        print(name, d, "fused" if fused else "generic", e1, e6)
        assert x6.dtype == dt and x6.shape == gold["x0"].shape
        assert e1 <= S.TOL[dt] and e6 <= S.TOL[dt]
    assert S.max_norm_err(runs[True][1], runs[False][1]) <= S.TOL[dt]


@pytest.mark.parametrize("d", list(DT))
@pytest.mark.parametrize("name", ["ula", "myula_l1", "myula_box"])
def test_device_noise_is_reproducible_and_is_the_philox_stream(name, d):
    dt = DT[d]
    gold = load_golden(f"sampler_{name}")
    _, a, s = chain(name, gold, dt, 7, steps=4)
    _, b, _ = chain(name, gold, dt, 7, steps=4)
    assert same_bits(a, b)
    assert (s.seed, s.step) == (7, 4)
    assert not same_bits(chain(name, gold, dt, 8, steps=4)[1], a)
    with pxrt.Precision(W(dt)):  # the same chain from explicit pxa_philox_normal noise
        kind, lam, pw, f = s._step_terms()
        x = R.to_dev(gold["x0"].astype(dt))
        for k in range(4):
            z = _dev.philox_normal(_dev.empty_like(x), 7, k)
            x = _dev.langevin_step(kind, s._gamma, lam, pw, x, f.grad(x), _dev.empty_like(x), noise=z)
    assert same_bits(to_NUMPY(x), a)
    # resuming: a fresh generator set to (x, seed, step) of the second sample continues the same chain
    with pxrt.Precision(W(dt)):
        s2 = sampler_of(name, gold, dt)
        gen = s2.samples(rng=7, x0=R.to_dev(gold["x0"].astype(dt)))
        next(gen), next(gen)
        s3 = sampler_of(name, gold, dt)
        gen3 = s3.samples(rng=0, x0=s2.x)
        s3.seed, s3.step = s2.seed, s2.step
        next(gen3)
        assert same_bits(to_NUMPY(next(gen3)), a)


def test_defaults_and_errors():
    with pxrt.Precision(pxrt.Width.DOUBLE):
        f = 0.5 * pxo.SquaredL2Norm(dim=N)  # diff_lipschitz 1
        assert float(pxes.ULA(f)._gamma) == pytest.approx(0.98, rel=1e-15)
        assert float(pxes.ULA(f, gamma=0.3)._gamma) == 0.3
        s = pxes.MYULA(f, pxo.L1Norm(dim=N))
        assert float(s._lambda) == 1.0  # min(2, 1 / 1)
        assert float(s._gamma) == pytest.approx(0.98 / 2.0, rel=1e-15)  # 1 + 1 / lamb
        s = pxes.MYULA(4.0 * f, pxo.L1Norm(dim=N))
        assert float(s._lambda) == 0.25 and float(s._gamma) == pytest.approx(0.98 / 8.0, rel=1e-15)
        assert float(pxes.MYULA(f)._lambda) == 1.0  # no g
        assert float(pxes.MYULA(g=pxo.L1Norm(dim=N))._lambda) == 2.0  # f = NullFunc: diff_lipschitz 0
        assert float(pxes.MYULA(f, pxo.L1Norm(dim=N), lamb=0.5)._lambda) == 0.5
        rough = pxo.L1Norm(dim=N).moreau_envelope(0.1)
        rough.diff_lipschitz = np.inf
        with pytest.raises(ValueError):
            pxes.ULA(rough)
        with pytest.raises(ValueError):
            pxes.MYULA(rough, pxo.L1Norm(dim=N))
        assert float(pxes.ULA(rough, gamma=0.1)._gamma) == 0.1
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError):
                pxes.ULA(f, gamma=bad)
        with pytest.raises(ValueError):
            pxes.MYULA()
    with pxrt.Precision(pxrt.Width.SINGLE):
        assert pxes.ULA(0.5 * pxo.SquaredL2Norm(dim=N))._gamma.dtype == np.float32


@pytest.mark.parametrize("name", ["ula", "myula_l1"])
def test_objective_func_of_stacked_chains(name):
    gold = load_golden(f"sampler_{name}")
    _, x6, s = chain(name, gold, np.float64, 3)
    val = to_NUMPY(s.objective_func())
    assert val.shape == (2, 1)
    r = x6 @ gold["A"].T - gold["b"]
    want = 0.5 * (r * r).sum(axis=-1, keepdims=True)
    if name == "myula_l1":  # + the Huber envelope of pw |.|_1 at lamb
        t, lamb = float(gold["pw"]) * float(gold["lamb"]), float(gold["lamb"])
        a = np.abs(x6)
        want = want + np.where(a <= t, a * a / (2 * lamb), float(gold["pw"]) * a - t * float(gold["pw"]) / 2).sum(
            axis=-1, keepdims=True)
    assert np.abs(val - want).max() <= 1e-10 * np.abs(want).max()


def test_reference_docstring_example():
    """_sampler.py:250-278 on device arrays."""
    from pyxu_amd.experimental.sampler import MYULA, ULA, OnlineMoment, OnlineVariance  # noqa: F401

    with pxrt.Precision(pxrt.Width.DOUBLE):
        f = 0.5 * pxo.SquaredL2Norm(dim=1)
        ula = ULA(f=f)
        gen = ula.samples(x0=R.to_dev(np.zeros(1)))
        mean, var = OnlineMoment(order=1), OnlineVariance()
        for _ in range(5):
            x = next(gen)
            m, v = float(mean.update(x)), float(var.update(x))
        assert np.isfinite(m) and v > 0 and float(var.stat()) == v
        assert isinstance(ula.seed, int) and ula.step == 5


# ------------------------------------------------------------------------------------------------ statistics classes
def feed(stat, samples, dt):
    with pxrt.Precision(W(dt)):
        for x in samples:
            out = stat.update(R.to_dev(x.astype(dt)))
    return to_NUMPY(out)


@pytest.mark.parametrize("d", list(DT))
def test_statistics_match_reference(stats, d):
    dt = DT[d]
    sfx = "_f32" if d == "f32" else ""
    samples = stats["samples"]
    made = dict(m1=pxes.OnlineMoment(1), m2=pxes.OnlineMoment(2), var=pxes.OnlineVariance(), std=pxes.OnlineStd(),
                cm3=pxes.OnlineCenteredMoment(3), cm4=pxes.OnlineCenteredMoment(4))
    for name, st in made.items():
        got = feed(st, samples, dt)
        err = S.max_norm_err(got, stats[name + sfx])
        print(d, name, err)
        assert got.dtype == dt and got.shape == (samples.shape[1],)
        assert err <= S.TOL[dt]
        assert np.array_equal(to_NUMPY(st.stat()), got)


@pytest.mark.parametrize("d", list(DT))
def test_skewness_and_kurtosis_are_the_documented_quantities(stats, d):
    dt = DT[d]
    samples = stats["samples"]
    for r, st in ((3, pxes.OnlineSkewness()), (4, pxes.OnlineKurtosis())):
        err = S.max_norm_err(feed(st, samples, dt), S.direct_standardized(samples, r))
        print(d, r, err)
        assert err <= S.TOL[dt]
    const = np.full((3, 9), 1.5)
    for st in (pxes.OnlineSkewness(), pxes.OnlineKurtosis()):
        assert np.isnan(feed(st, const, dt)).all()
    mixed = np.array(samples[:5, :8])
    mixed[:, 3] = 2.0  # one constant pixel among varying ones
    got = feed(pxes.OnlineKurtosis(), mixed, dt)
    assert np.isnan(got[3]) and np.isfinite(np.delete(got, 3)).all()


@pytest.mark.parametrize("d", list(DT))
def test_compositions(stats, d):
    dt = DT[d]
    samples = stats["samples"][:7, :12]
    var = feed(pxes.OnlineVariance(), samples, dt)
    mean = feed(pxes.OnlineMoment(1), samples, dt)
    assert same_bits(feed(pxes.OnlineVariance() ** 0.5, samples, dt), feed(pxes.OnlineStd(), samples, dt))
    assert same_bits(feed(pxes.OnlineStd(), samples, dt), np.sqrt(var))
    tol = 4 * np.finfo(dt).eps
    checks = {
        "+": (pxes.OnlineMoment(1) + pxes.OnlineVariance(), mean + var),
        "-": (pxes.OnlineMoment(1) - pxes.OnlineVariance(), mean - var),
        "*": (pxes.OnlineMoment(1) * pxes.OnlineVariance(), mean * var),
        "/": (pxes.OnlineMoment(1) / pxes.OnlineVariance(), mean / var),
        "* s": (pxes.OnlineVariance() * 3, var * dt(3)),
        "s *": (2.5 * pxes.OnlineVariance(), var * dt(2.5)),
        "/ s": (pxes.OnlineVariance() / 4, var / dt(4)),
        "**": (pxes.OnlineVariance() ** 3, var.astype(np.float64) ** 3),
    }
    for name, (st, want) in checks.items():
        got = feed(st, samples, dt)
        err = float((np.abs(got - want) / np.abs(want)).max())
        print(d, name, err)
        assert got.dtype == dt and err <= (1e-5 if (name == "**" and dt == np.float32) else tol if name != "**" else 1e-12)
    zero_var = np.full((3, 5), 2.0)
    assert np.isnan(feed(pxes.OnlineMoment(1) / pxes.OnlineVariance(), zero_var, dt)).all()  # NaN, not inf
    with pytest.raises(TypeError):
        pxes.OnlineVariance() + 1.0


@pytest.mark.parametrize("d", list(DT))
def test_centred_order_five_by_the_chain(stats, d):
    dt = DT[d]
    samples = stats["samples"]
    err = S.max_norm_err(feed(pxes.OnlineCenteredMoment(5), samples, dt), S.direct_moment(samples, 5))
    print(d, err)
    assert err <= S.TOL[dt]


# ------------------------------------------------------------------------------------------------ end to end
def device_ula_variance(step_of):
    with pxrt.Precision(pxrt.Width.DOUBLE):
        ula = pxes.ULA(0.5 * pxo.SquaredL2Norm(dim=S.ULA_N), gamma=S.ULA_GAMMA)
        gen = ula.samples(rng=S.ULA_SEED, x0=R.to_dev(np.zeros(S.ULA_N)))
        for k in range(S.ULA_STEPS):
            ula.step = step_of(k)
            x = next(gen)
    return float(to_NUMPY(x).var())


def test_ula_reaches_the_stationary_variance():
    var = device_ula_variance(lambda k: k)
    print(var, S.ULA_VAR, S.ULA_BOUND)
    assert abs(var - S.ULA_VAR) <= S.ULA_BOUND


def test_ula_variance_check_catches_reused_noise():
    var = device_ula_variance(lambda k: 0)
    print(var)
    assert abs(var - S.ULA_VAR) > S.ULA_BOUND
