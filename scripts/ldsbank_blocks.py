"""LDS bank-conflict audit of the fp32 PGD tile kernel's row-major pass-B blocks (csrc/tile2d.hpp BlockB, csrc/pgd_tv2d.hip
pass_b_blocks / tv_block) under the MI355X_MICROARCH.md §LDS model (scripts/ldsbank.py, scripts/ldsbank_tiles.py):
per access site the worst LDS-array cycles per wave-instruction over the four waves against the conflict-free count,
and a check that the lane map covers every 2 x 4 block of the 32 x 64 tile once.
usage: python scripts/ldsbank_blocks.py [R ...]   (default 6 7 8: the exchange form; smaller R take the window form)"""
import sys

sys.path.insert(0, "scripts")
from ldsbank import cost_read_b128, cost_read_b32  # noqa: E402
from ldsbank_tiles import cost_read_b64, cost_write, pad_to  # noqa: E402

TY, TX, V = 32, 64, 4
PTP = TY + 4
WR, WC = 16, 32
EP0 = 40  # pitch of the exchange area's q0 rows (kTvxP0)


def item(wv, ln):
    """BlockB::item: (row pair, column item) within the wave's region and the region's first row / column"""
    l, k = ln & 31, (ln & 31) >> 2
    return k ^ (((k + 2) >> 2) & 1), 4 * (ln >> 5) + (l & 3), WR * (wv >> 1), WC * (wv & 1)


def audit(R):
    CA = -(-2 * R // V) * V
    AC, AR = TX + 2 * CA, TY + 4 * R
    AP = pad_to(AC, 32, 28)
    exchange = (2 * R - 1) * AP >= 2 * (9 * EP0 + 9 * WR)
    res = {}

    def rec(name, cost, ideal):
        c, _ = res.get(name, (0, ideal))
        res[name] = (max(c, cost), ideal)

    seen = set()
    for wv in range(4):
        its = [item(wv, ln) for ln in range(64)]
        for rpl, cil, wr0, wc0 in its:
            seen.add((wr0 // 2 + rpl, wc0 // 4 + cil))
        r0 = [wr0 + 2 * rpl for rpl, cil, wr0, wc0 in its]
        c0 = [wc0 + 4 * cil for rpl, cil, wr0, wc0 in its]
        for j in range(4 + 4 * R):  # G1 sweep: b64 rows of PT
            rec("passB PT reads (read_b64)", cost_read_b64([(CA - 2 * R + c0[l] + j) * PTP + r0[l] for l in range(64)]), 2)
        own = [(r0[l] + 2 * R) * AP + CA + c0[l] for l in range(64)]
        if exchange:
            for r in range(3):
                rec("TV own rows + row below (read_b128)", cost_read_b128([own[l] + r * AP for l in range(64)]), 4)
            for r in range(2):
                rec("TV column to the right (read_b64)", cost_read_b64([own[l] + r * AP + 4 for l in range(64)]), 2)
            e0 = [(its[l][0] + 1) * EP0 + 4 * its[l][1] for l in range(64)]
            e1 = [9 * EP0 + (its[l][1] + 1) * WR + 2 * its[l][0] for l in range(64)]
            rec("exchange q0 store (write_b128)", cost_write(e0, 4), 8)
            rec("exchange q1 store (write_b64)", cost_write(e1, 2), 4)
            rec("exchange q0 read (read_b128)", cost_read_b128([a - EP0 for a in e0]), 4)
            rec("exchange q1 read (read_b64)", cost_read_b64([a - WR for a in e1]), 2)
        else:
            for r in range(-1, 3):
                rec("TV window rows (read_b128)", cost_read_b128([own[l] + r * AP for l in range(64)]), 4)
                for off in (-1, 4):
                    rec("TV window side columns (read_b32)", cost_read_b32([own[l] + r * AP + off for l in range(64)]), 2)
    assert seen == {(rp, ci) for rp in range(TY // 2) for ci in range(TX // 4)}, "block map"
    # pass A's transposed stores at the new pitch (items tid -> row group tid % 8, column group tid // 8)
    for w in range(3):
        for v in range(V):
            addrs = [None if 64 * w + l >= 8 * (AC // V) else (V * ((64 * w + l) // 8) + v) * PTP + V * ((64 * w + l) % 8)
                     for l in range(64)]
            rec("passA PT stores (write_b128)", cost_write(addrs, 4), 8)
    print(f"== R={R}: AP={AP} PTP={PTP} TV {'exchange' if exchange else 'window'} form; every block covered once")
    for k, (c, i) in res.items():
        print(f"   {k:40s} worst {c:3d} cycles (conflict-free {i}){'' if c <= i else '  <-- conflicts'}")


if __name__ == "__main__":
    for R in ([int(v) for v in sys.argv[1:]] or [6, 7, 8]):
        audit(R)
