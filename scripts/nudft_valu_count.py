#!/usr/bin/env python
"""
Count the instructions of the NUDFT kernel's inner loop from the compiler's gfx950 assembly (no GPU needed).

    python scripts/nudft_valu_count.py [--arch gfx950]

Compiles pyxu_amd/csrc/nudft.hip with the library's flags and --save-temps into a temporary directory, finds in each
nudft_kernel<T, D, QC> the hot loop (the innermost backward-branching block that reads LDS and holds the most VALU
instructions), and prints per instantiation: VALU / LDS / scalar instructions per loop iteration, the (source,
target) pairs one iteration covers (source unroll x targets per thread, read off the count of v_rndne, one per pair in
fp32), and VALU per pair.  scripts/bench_nudft.py uses the fp32 figures for its issue-bound ceiling.
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-munsafe-fp-atomics"]


def hot_loops(asm):
    """{(T, D, QC): dict(valu, lds, salu, rndne)} of the hot loop of every nudft_kernel instantiation."""
    out = {}
    funcs = re.split(r"^(_ZN3pxa\S*nudft_kernelI(\w)Li(\d)ELi(\d)E\S*):.*$", asm, flags=re.M)
    for k in range(1, len(funcs), 5):
        T, D, QC, body = funcs[k + 1], int(funcs[k + 2]), int(funcs[k + 3]), funcs[k + 4]
        body = body.split(".Lfunc_end")[0]  # blocks may be laid out after s_endpgm
        lines = [ln.strip() for ln in body.splitlines()]
        labels = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", ln)}
        loops = []  # (first line, branch line) of every backward branch
        for i, ln in enumerate(lines):
            m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln)
            if m and labels.get(m.group(1), i + 1) <= i:
                loops.append((labels[m.group(1)], i))
        best = None
        for lo, hi in loops:
            if any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in loops):
                continue  # not innermost
            blk = [x.split(";")[0].strip() for x in lines[lo + 1:hi + 1]]
            ops = [x.split()[0] for x in blk if x and not x.endswith(":")]
            c = dict(
                valu=sum(o.startswith("v_") for o in ops), lds=sum(o.startswith("ds_") for o in ops),
                salu=sum(o.startswith("s_") for o in ops), rndne=sum(o.startswith("v_rndne") for o in ops),
                trans=sum(o.startswith(("v_sin", "v_cos", "v_rcp", "v_exp", "v_log", "v_sqrt", "v_rsq")) for o in ops),
            )
            if c["lds"] and (best is None or c["valu"] > best["valu"]):
                best = c
        out[("f32" if T == "f" else "f64", D, QC)] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(ROOT, "pyxu_amd", "csrc", "nudft.hip")
        subprocess.run([a.hipcc, f"--offload-arch={a.arch}", *FLAGS, "--save-temps", "-c", src, "-o", "nudft.o"], cwd=tmp, check=True)
        name = next(f for f in os.listdir(tmp) if f.endswith(f"{a.arch}.s"))
        asm = open(os.path.join(tmp, name)).read()
    print(f"{'kernel':<14}{'VALU':>6}{'LDS':>5}{'SALU':>6}{'trans':>6}{'pairs':>6}{'VALU/pair':>11}")
    for (T, D, QC), c in sorted(hot_loops(asm).items()):
        if c is None:
            print(f"{T} D={D} QC={QC}: no loop found")
            continue
        pairs = c["rndne"] if T == "f32" and c["rndne"] else None
        per = f"{c['valu'] / pairs:.1f}" if pairs else "-"
        print(f"{T} D={D} QC={QC:<4}{c['valu']:>6}{c['lds']:>5}{c['salu']:>6}{c['trans']:>6}{pairs or '-':>6}{per:>11}")


if __name__ == "__main__":
    main()
