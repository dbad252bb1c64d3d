"""Kernel D of the look-ahead PD3O / Condat-Vu step on the paths bench.py's c3 record does not time: a 2-D image
(R0 = 0, one plane per thread), a stack of images as one volume without axis-0 blur (R0 = 0, many planes) and a
volume with isotropic TV (R0 = 6), all fp32 with g = PositiveOrthant.  Per-kernel HIP-event times (pxa_pds_kernel_ms)
over 50 steps; one JSON line.  To compare two builds, run it once per library (PXA_LIB_PATH), alternating.
usage: python scripts/pds_la_probe.py"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd.operator.linop.filter import gaussian_kernel1d  # noqa: E402

K = 50
out = {"only": "la2d"}
gen = torch.Generator(device="cuda").manual_seed(3)


def run(tag, sh, batch_axis=False):
    N = int(np.prod(sh))
    with pxrt.Precision(pxrt.Width.SINGLE):
        if batch_axis:  # axis 0 neither blurred nor differentiated
            taps = np.asarray(gaussian_kernel1d(2.0, 0, 6), dtype=np.float32)
            S = pxo.Stencil(arg_shape=sh, kernel=[np.array([1.0], dtype=np.float32), taps, taps], center=[0, 6, 6], mode="constant")
            dirs = (1, 2)
        else:
            S = pxo.Gaussian(arg_shape=sh, sigma=2.0, truncate=3.0)
            dirs = tuple(range(len(sh)))
        y = torch.rand(N, device="cuda", dtype=torch.float32, generator=gen)
        f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(y) * S
        f.diff_lipschitz = 1.0
        Kop = pxo.Gradient(arg_shape=sh, directions=dirs)
        h = 0.01 * pxo.L21Norm(arg_shape=(len(dirs), *sh))
        g = pxo.PositiveOrthant(dim=N)
        for algo, klass in (("pd3o", pxs.PD3O), ("cv", pxs.CondatVu)):
            s = klass(f=f, g=g, h=h, K=Kop, show_progress=False, stop_rate=K)
            s.fit(x0=torch.zeros(N, device="cuda", dtype=torch.float32), stop_crit=pxst.MaxIter(10 ** 9), mode=pxa.Mode.MANUAL)
            it = s.steps()
            for _ in range(10):
                next(it)
            torch.cuda.synchronize()
            assert s._plan is not None and s._plan["la"]
            prev = _dev.tuning(_dev.TUNE_PDS_EVENTS, 1)
            _dev.pds_kernel_ms(reset=True)
            try:
                for _ in range(K):
                    next(it)
                torch.cuda.synchronize()
                nrec, ms = _dev.pds_kernel_ms(reset=True)
            finally:
                _dev.tuning(_dev.TUNE_PDS_EVENTS, prev)
            out[f"{tag} {algo}"] = {"steps": nrec, "kernel_B_ms": round(ms[1] / nrec, 5), "kernel_D_ms": round(ms[2] / nrec, 5)}
            del s, it
            torch.cuda.empty_cache()


run("4096^2", (4096, 4096))
run("64x1024^2 batch", (64, 1024, 1024), batch_axis=True)
run("512^3", (512, 512, 512))
print(json.dumps(out), flush=True)
