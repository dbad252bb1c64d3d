"""Development probe (probe build: make -C pyxu_amd/csrc probe, PXA_LIB_PATH=build/libpyxu_amd_probe.so): the tile
kernel (pgd_tv2d_kernel) from its s_memtime trace (PXA_TUNE_PGD_DIAG bit 5).

  python scripts/tile_trace.py [n] [sigma] [--timeline] [--generic] [--corners-generic] [--save=raw.npy]

Phase durations of workgroups 0 (corner tile), 9 and grid/2 + 8 (interior tiles at 2048^2), grid-1 (first-column tile)
and 8 (top-row tile).  --timeline: also the launch timeline from every workgroup's start / end stamps, per XCD (the
counter's base differs between XCDs and between CUs, so stamps are taken relative to the first start on the same CU).  --generic: col, row
and corner tiles on the generic path (bit 11), the dispatch before the tile classes existed; --corners-generic: corner
tiles alone (bit 12), the dispatch before the corner class."""
import ctypes as ct
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from pyxu_amd import _dev  # noqa: E402
from pyxu_amd._lib import lib  # noqa: E402
from scripts.pgd_probe import taps  # noqa: E402

flags = [a for a in sys.argv[1:] if a.startswith("--")]
pos = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(pos[0]) if len(pos) > 0 else 2048
sigma = float(pos[1]) if len(pos) > 1 else 2.0
diag = 32 | (2048 if "--generic" in flags else 0) | (4096 if "--corners-generic" in flags else 0)
g = torch.Generator(device="cuda").manual_seed(0)
x, xp, b = (torch.rand((n, n), device="cuda", generator=g) for _ in range(3))
out = torch.empty_like(x)
t = taps(sigma)
prev = [(_dev.TUNE_PGD_DIAG, _dev.tuning(_dev.TUNE_PGD_DIAG, diag))]
for _ in range(10):
    _dev.pgd_tv2d_step(x, xp, b, out, 1, 1, n, n, t, t, 1.0, 1.0, 0.02, 0.01, 0.3, 0.5, 1, 0.0)
torch.cuda.synchronize()
buf = np.zeros(160, dtype=np.uint64)
assert lib.pxa_pgd_tile_trace(buf.ctypes.data_as(ct.c_void_p), 160) == 0
nwg = (-(-n // 32)) * (-(-n // 64))
tl = np.zeros(3 * nwg, dtype=np.uint64)
if "--timeline" in flags:
    assert nwg <= 16384 and lib.pxa_pgd_tile_timeline(tl.ctypes.data_as(ct.c_void_p), nwg) == 0
    save = [a.split("=", 1)[1] for a in flags if a.startswith("--save=")]
    if save:
        np.save(save[0], tl)
for k, v in prev:
    _dev.tuning(k, v)
print(f"n = {n}, sigma = {sigma}, dispatch: "
      f"{'generic edge tiles' if diag & 2048 else 'tile classes, corners generic' if diag & 4096 else 'tile classes'}")
# fp32 (row-major pass-B blocks, no staging): H^T y loads + first PT rows issued + TV chain, the G1 sweep, finish in
# registers + x_new stores; fp64 would be pass B, H^T y loads + O staging, row-major epilogue (this probe runs fp32)
names = ["load", "B1", "passA", "B2(+ghost)", "loads+TV", "sweep", "epilogue"]
tr = buf.astype(np.int64).reshape(5, 4, 8)
for slot, lab in enumerate(["wg0", "wg9", "wg n/2+8", "wg n-1", "wg8"]):
    t0 = tr[slot, :, 0].min()
    for w in range(4):
        d = np.diff(tr[slot, w])
        print(f"{lab:8s} w{w} start {tr[slot, w, 0] - t0:7d}  " + "  ".join(f"{names[i]} {d[i]:6d}" for i in range(7)),
              f"| total {tr[slot, w, 7] - tr[slot, w, 0]:6d}")

if "--timeline" in flags:
    CLS = ["interior", "col", "row", "generic", "corner"]  # (the kernel's TileClass values)
    tl = tl.astype(np.int64).reshape(nwg, 3)
    tile, cls = tl[:, 2] & 0xFFFFFFFF, (tl[:, 2] >> 32) & 15
    xcc, hw = (tl[:, 2] >> 36) & 15, (tl[:, 2] >> 40) & 0xFFFF
    cu = (hw >> 8) & 0xFF  # CU, SH and SE of the workgroup's first wave: one compute unit of its XCD
    order = np.arange(nwg) // 8  # dispatch order within the XCD band (blockIdx // 8)
    tiles1 = -(-n // 64)
    slots = 4 * 32  # resident workgroups per XCD: 32 CUs x 4
    print("\nlaunch timeline (ticks from the first start on the same CU; XCD = XCC_ID of the workgroup); round = dispatch order // %d" % slots)
    print("blockIdx %% 8 == XCC_ID + const for %d of %d workgroups" % (int((((np.arange(nwg) - xcc) % 8) == ((0 - xcc[0]) % 8)).sum()), nwg))
    life = tl[:, 1] - tl[:, 0]
    print("life per class (median / max over the launch): " + "  ".join(
        f"{CLS[c]} {int(np.median(life[cls == c]))} / {int(life[cls == c].max())} (n={int((cls == c).sum())})"
        for c in range(len(CLS)) if (cls == c).any()))
    tails = []
    for x_ in sorted(set(xcc.tolist())):
        idx = np.nonzero(xcc == x_)[0]
        # the counter's base differs between XCDs and, as measured, between compute units of one XCD too: stamps are
        # taken relative to the first start on the same CU (all CUs receive their first workgroups at the launch's start)
        base = np.array([tl[idx, 0][cu[idx] == u].min() for u in cu[idx]])
        st, en = tl[idx, 0] - base, tl[idx, 1] - base
        rnd = order[idx] // slots
        c, tix = cls[idx], tile[idx]
        line = f"XCD {x_}: {len(idx)} wgs, last end {en.max():6d};"
        for r in range(rnd.max() + 1):
            m = (rnd == r) & (c == 0)
            if m.any():
                line += f" last interior end of round {r}: {en[m].max():6d};"
        print(line)
        last = np.argsort(en)[::-1][:4]
        print("        ends last: " + ", ".join(
            f"tile ({tix[i] // tiles1},{tix[i] % tiles1}) {CLS[c[i]]} round {rnd[i]} start {st[i]} end {en[i]}" for i in last))
        late = np.argsort(st)[::-1][:4]  # the XCD's last dispatches: the slots that freed last
        print("        starts last: " + ", ".join(
            f"tile ({tix[i] // tiles1},{tix[i] % tiles1}) {CLS[c[i]]} start {st[i]}" for i in late))
        slow = np.nonzero(c >= 3)[0]  # generic and corner tiles of this XCD
        if len(slow):
            print("        generic / corner: " + ", ".join(
                f"tile ({tix[i] // tiles1},{tix[i] % tiles1}) {CLS[c[i]]} round {rnd[i]} start {st[i]} end {en[i]}" for i in slow[:8]))
        # a compute unit is done when the last of its workgroups ends: the idle time of its slots until the XCD's last end
        ce = np.array([en[cu[idx] == u].max() for u in sorted(set(cu[idx].tolist()))])
        tails.append((en.max() - np.median(ce), float(np.mean(en.max() - ce))))
        print(f"        {len(ce)} CUs end: first {ce.min()}, median {int(np.median(ce))}, last {en.max()}: the median CU idles"
              f" {int(tails[-1][0])} ticks, the mean CU {tails[-1][1]:.0f}, before the XCD's last workgroup ends")
    print("all XCDs: median-CU idle %d .. %d ticks, mean-CU idle %.0f .. %.0f" % (
        min(a for a, _ in tails), max(a for a, _ in tails), min(b_ for _, b_ in tails), max(b_ for _, b_ in tails)))
