"""Development probe: host cost per fused PD3O / Condat-Vu step (look-ahead on, fp32) on a (32, 64, 64) volume, where
the device time per step is far below the host's: wall time of 400 steps() items after 20 warm-up items."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyxu_amd.abc as pxa  # noqa: E402
import pyxu_amd.operator as pxo  # noqa: E402
import pyxu_amd.opt.solver as pxs  # noqa: E402
import pyxu_amd.opt.stop as pxst  # noqa: E402
import pyxu_amd.runtime as pxrt  # noqa: E402
from pyxu_amd.util import to_device  # noqa: E402

sh, steps, warm = (32, 64, 64), 400, 20
N = int(np.prod(sh))
rng = np.random.default_rng(0)
with pxrt.Precision(pxrt.Width.SINGLE):
    S = pxo.Gaussian(arg_shape=sh, sigma=1.0, truncate=3.0)
    f = 0.5 * pxo.SquaredL2Norm(dim=N).asloss(to_device(rng.standard_normal(N).astype(np.float32))) * S
    f.diff_lipschitz = 1.0
    K, h = pxo.Gradient(arg_shape=sh), 0.05 * pxo.L1Norm(dim=3 * N)
    for name, klass in (("pd3o", pxs.PD3O), ("cv", pxs.CondatVu)):
        s = klass(f=f, g=None, h=h, K=K, show_progress=False)
        s.fit(x0=to_device(rng.uniform(0, 1, N).astype(np.float32)), stop_crit=pxst.MaxIter(10**9), mode=pxa.Mode.MANUAL)
        assert s._plan is not None and s._plan["la"], "fused look-ahead step not selected"
        gen = s.steps()
        for _ in range(warm):
            next(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            next(gen)
        torch.cuda.synchronize()
        print(f"pds host {name} {1e6 * (time.perf_counter() - t0) / steps:.1f} us/step", flush=True)
        gen.close()
