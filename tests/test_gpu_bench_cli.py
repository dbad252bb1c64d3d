"""
bench.py's command line on the GPU, at a small image (in-process, `bench.main(argv)`):

  * a plain run does the headline work only: no kernel-time window (`roofline`), no CPU baseline, no
    sub-record; `--steps` is the number of timed steps and `ms_per_step` / `value` are consistent with it;
  * `--dump-outputs DIR` writes the iterate the last timed step returned, which is the oracle's PGD iterate
    after warmup + steps iterations on the same seeded problem (1e-5 norm-wise, fp32), and two runs with the
    same arguments write the same bits;
  * `--full` brings the kernel-time window back.

The kernels themselves are checked at the benchmarked shapes in test_gpu_bench_shapes.py; 96 x 96 keeps this
file about the command line.
"""
import json

import numpy as np
import pytest

import oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs an MI355X", allow_module_level=True)

import bench  # noqa: E402

N, STEPS, WARMUP = 96, 6, 2
SUBS = ("stop_rate_1", "c2_4096", "c5", "c4", "c3", "k4", "dense_mfma")


def _run(capsys, *extra):
    capsys.readouterr()
    bench.main(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--n", str(N), "--prime-seconds", "0", *extra])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _oracle_iterate(n_iter, lam=0.01, mu=0.01, sigma=2.0):
    """bench.build_problem's rank-0 problem restated on the host (as bench.cpu_baseline does), n_iter PGD steps."""
    sh = (N, N)
    rng = np.random.default_rng(1234)
    taps, c = orc.gaussian_taps(sigma, 3.0, np.float32)
    blur = dict(arg_shape=sh, kernel=[taps, taps], center=[c, c])
    y = orc.stencil_apply(bench.phantom(sh, rng).reshape(-1), sh, [taps, taps], [c, c])
    y = (y + (0.01 * rng.standard_normal(N * N)).astype(np.float32)).astype(np.float32)
    tau = np.float32(1 / np.float32(1.0 + (lam / mu) * 8.0))
    grad = lambda v: orc.deblur_tv_grad(v, blur, y, lam, mu, dict(arg_shape=sh))
    x, _ = orc.pgd(np.zeros(N * N, np.float32), grad, lambda z, t: orc.positive_orthant_prox(z), tau, n_iter)
    return x


def test_plain_run_is_the_headline_only_and_dumps_its_iterate(capsys, tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    line = _run(capsys, "--dump-outputs", str(d1))
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "image-iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) <= 1e-2  # one image: value = 1 / seconds per step
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert not [k for k in SUBS if k in line]
    assert line["config"]["fused_m_step"] is True
    assert sorted(p.name for p in d1.iterdir()) == ["x.npy"]
    x = np.load(d1 / "x.npy")
    assert x.dtype == np.float32 and x.shape == (N * N,)
    assert rel_err(x, _oracle_iterate(WARMUP + STEPS)) <= 1e-5
    _run(capsys, "--dump-outputs", str(d2))
    assert np.array_equal(x.view(np.uint32), np.load(d2 / "x.npy").view(np.uint32))


def test_full_run_times_the_kernel(capsys):
    line = _run(capsys, "--full", "--no-sub", "--cpu-seconds", "0")
    assert line["roofline"]["kernel_ms"] > 0 and line["roofline"]["kernel_timer"] == "post_region"
    assert 1 <= line["roofline"]["launches_timed"] <= STEPS
    assert line["cpu_baseline"] is None and not [k for k in SUBS if k in line]
