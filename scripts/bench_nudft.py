#!/usr/bin/env python
"""
Measure the NUDFT kernel (pxa_nudft, behind NUFFT.type1/2/3) against what a user had before it: the matrix
exp(i isign T X^T) built by torch in complex64 blocks and multiplied.

    python scripts/bench_nudft.py [--rounds 5] [--reps 3] [--small] [--out FILE]

Workloads (fp32): type-2 apply and adjoint for N = 256^2 modes and M = 65536 samples with Q = 1 and 8 stacked
inputs, and the few-targets case, type-1 apply onto N = 64^2 modes from M = 2^20 samples, which runs on source splits.
The baseline runs in the fastest of eight forms (512 MiB / 2 GiB blocks x four ways to multiply: one complex matmul,
its transpose, multiply-and-sum, four real matmuls on cos / sin), chosen per workload by timing one block of each.  Both sides run on the same GPU in the same process in alternating
rounds; times are HIP-event times of `reps` back-to-back calls, and the median over the rounds is reported.  One JSON
line per workload:

    pairs            M N (the (source, target) pairs of one transform; each feeds Q stack rows)
    kernel_ms / baseline_ms, kernel_pairs_per_s / baseline_pairs_per_s, speedup
    valu_per_pair    VALU instructions per (m, n) pair in the kernel's inner loop, counted from the gfx950
                     assembly (scripts/nudft_valu_count.py), times the passes a stack of Q rows takes
    ceiling_pairs_per_s = CUs x SIMDs x lanes per cycle x clock / valu_per_pair: the rate at which the chip can issue
                     that many vector instructions and do nothing else; fraction_of_ceiling = kernel / ceiling
    rel_diff         norm-wise difference of the two results (a sanity check, not the accuracy test)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# inner-loop VALU instructions per (m, n) pair of nudft_kernel<float, 2, QC> (scripts/nudft_valu_count.py)
VALU_PER_PAIR_D2 = {1: 25.5, 2: 27.5, 4: 31.5}
# MI355X: 256 CUs x 4 SIMDs, a wave64 VALU instruction issues over 2 cycles (32 lanes per cycle), 2.4 GHz peak clock
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def passes(Q, q_chunk):
    """Stack rows per pass, as pxa_nudft runs them: chunks of q_chunk, a remainder of 3 padded to 4."""
    out, q = [], Q
    while q > 0:
        qc = q_chunk if q >= 3 else q
        out.append(qc)
        q -= min(qc, q)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="1/16 of the pairs (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_nudft.py needs an MI355X: no timing is taken without one")
    from pyxu_amd import _dev

    dev = torch.device("cuda", 0)
    tile_n, tile_m, q_chunk = _dev.nudft_tiles(0)
    g = torch.Generator(device="cpu").manual_seed(0)

    def mesh(n):
        k = torch.arange(-(n // 2), (n - 1) // 2 + 1, dtype=torch.float32)
        return torch.stack(torch.meshgrid(k, k, indexing="ij"), dim=-1).reshape(-1, 2)

    def samples(m):
        return (torch.rand((m, 2), generator=g) * 2 - 1) * np.pi

    s = 4 if a.small else 1
    grid256, grid64 = mesh(256 // s), mesh(64)
    x16, x20 = samples(65536 // s), samples((1 << 20) // (s * s))
    work = [  # (name, src, tgt, isign, Q)
        ("type2_apply_N256x256_M65536", grid256, x16, 1, 1),
        ("type2_adjoint_N256x256_M65536", x16, grid256, -1, 1),
        ("type2_apply_N256x256_M65536", grid256, x16, 1, 8),
        ("type2_adjoint_N256x256_M65536", x16, grid256, -1, 8),
        ("type1_apply_N64x64_M1048576", x20, grid64, 1, 1),
    ]

    def baseline(src, tgt, isign, w, out, block_bytes, mult, blocks=None):
        """out (Q, N) complex64 = w (Q, M) @ exp(i isign tgt src^T)^T, the matrix built in blocks of `block_bytes` and
        multiplied as `mult` says (`blocks`: stop after that many blocks, for the trial that picks the form):
          "mm"   E @ w^T, one complex matmul;            "mmT"  w @ E^T, the same product transposed;
          "sum"  (E * w[q]).sum(-1) per stack row;       "real" four real matmuls on cos / sin of the phase."""
        M, N = src.shape[0], tgt.shape[0]
        rows = max(1, min(N, block_bytes // (8 * M)))
        st, wt = (isign * src).T.contiguous(), w.T.contiguous()  # (D, M), (M, Q)
        wr, wi = wt.real.contiguous(), wt.imag.contiguous()
        for b, n0 in enumerate(range(0, N, rows)):
            if blocks is not None and b >= blocks:
                break
            ph = tgt[n0:n0 + rows] @ st  # (rows, M) float32
            if mult == "real":
                C, S = torch.cos(ph), torch.sin(ph)
                o = torch.complex(C @ wr - S @ wi, S @ wr + C @ wi).T
            else:
                E = torch.polar(torch.ones_like(ph), ph)  # (rows, M) complex64
                if mult == "mm":
                    o = (E @ wt).T
                elif mult == "mmT":
                    o = w @ E.T
                else:
                    o = torch.stack([(E * w[q]).sum(-1) for q in range(w.shape[0])])
            out[:, n0:n0 + rows] = o
        return min(rows, N)

    # The baseline runs in the fastest of these forms, chosen per workload by timing one block of each (per row of
    # the block) after a warm-up call: rocBLAS's complex matmul takes ~10 ms on a (1024 x 65536) @ (65536 x 1)
    # product whatever the row count, so the plain "mm" form alone would flatter the kernel.
    FORMS = [(bb << 20, mult) for bb in (512, 2048) for mult in ("mm", "mmT", "sum", "real")]

    def timed(fn, reps=None):
        reps = a.reps if reps is None else reps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = []
    for name, src, tgt, isign, Q in work:
        src, tgt = src.to(dev).contiguous(), tgt.to(dev).contiguous()
        M, N = src.shape[0], tgt.shape[0]
        w = torch.randn((Q, 2 * M), generator=g).to(dev)
        wc = torch.view_as_complex(w.reshape(Q, M, 2))
        out_k = torch.empty((Q, 2 * N), dtype=torch.float32, device=dev)
        out_b = torch.empty((Q, N), dtype=torch.complex64, device=dev)
        run_k = lambda: _dev.nudft(src, tgt, isign, w, out=out_k)  # noqa: E731
        run_k()  # warm-up: code objects, allocator, library heuristics
        pick = {}
        for form in FORMS:
            run_f = lambda: baseline(src, tgt, isign, wc, out_b, *form, blocks=1)  # noqa: E731
            rows = run_f()
            torch.cuda.synchronize()
            pick[form] = timed(run_f, 1) * N / rows  # extrapolated to all blocks
        form = min(pick, key=pick.get)
        run_b = lambda: baseline(src, tgt, isign, wc, out_b, *form)  # noqa: E731
        tk, tb = [], []
        for _ in range(a.rounds):
            tk.append(timed(run_k))
            tb.append(timed(run_b))
        k_ms, b_ms = statistics.median(tk), statistics.median(tb)
        diff = (torch.view_as_complex(out_k.reshape(Q, N, 2)) - out_b).norm() / out_b.norm()
        pairs = M * N
        valu = sum(VALU_PER_PAIR_D2[qc] for qc in passes(Q, q_chunk))
        ceiling = LANE_OPS_PER_S / valu
        rec = dict(
            workload=name, Q=Q, M=M, N=N, pairs=pairs, splits=_dev.nudft_splits(0, 2, Q, M, N),
            kernel_ms=round(k_ms, 4), baseline_ms=round(b_ms, 4), baseline_form=f"{form[0] >> 20} MiB blocks, {form[1]}",
            baseline_forms_est_ms={f"{bb >> 20}MiB-{mu}": round(t, 3) for (bb, mu), t in pick.items()},
            kernel_ms_rounds=[round(t, 4) for t in tk], baseline_ms_rounds=[round(t, 4) for t in tb],
            kernel_pairs_per_s=pairs / (k_ms * 1e-3), baseline_pairs_per_s=pairs / (b_ms * 1e-3),
            speedup=b_ms / k_ms, valu_per_pair=valu, ceiling_pairs_per_s=ceiling,
            fraction_of_ceiling=pairs / (k_ms * 1e-3) / ceiling, rel_diff=float(diff), small=bool(a.small),
        )
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
