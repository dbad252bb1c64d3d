"""Static phase summary of the PGD tile kernel's interior tile from a device-only assembly listing of csrc/pgd_tv2d.hip
(hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S pgd_tv2d.hip -o pgd.s):

    python3 scripts/pgd_blocks_isa.py pgd.s ["pgd_tv2d_kernelIfLi6E"]
    python3 scripts/pgd_blocks_isa.py --check pgd.s      (exit status 1 unless the R = 6 fp32 interior tile has the shape
                                                          the row-major pass-B blocks are built for, see check())

The interior tile is the code from the lowered s_setprio of the window phase whose loads are all 16-B to the barrier
before the last-workgroup fold's atomic add.  It is cut at its s_barriers into segments (window tail, pass A, pass B +
epilogue, ...), and each segment is printed as counts of LDS / global / packed-FMA / VALU instructions and as a run-length string
of its LDS reads (r32 / r64 / r128), LDS writes (w..), global loads (G) / stores (S), v_pk_fma_f32 (F), other VALU (v)
and waits (|lgkmcnt(n)|, |vmcnt(n)|).  Needs no GPU.
"""
import re
import sys


def kernel_body(text, piece):
    start = next(i for i, ln in enumerate(text) if re.match(r"^_Z\w*%s\w*:" % re.escape(piece), ln))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[start:end + 1]


def interior(body):
    """lines of the interior tile: after the s_setprio 0 that closes the all-16-B window phase"""
    i = 0
    while i < len(body):
        m = re.match(r"\s*s_setprio\s+(\d+)", body[i])
        if m and int(m.group(1)) > 0:
            j = next(q for q in range(i + 1, len(body)) if re.match(r"\s*s_setprio\s+0\b", body[q]))
            ops = [ln.split()[0] for ln in body[i + 1:j] if ln.strip() and not ln.strip().startswith((";", "."))]
            narrow = sum(x.startswith("global_load") and not x.startswith("global_load_dwordx4") for x in ops)
            if narrow == 0:
                k = next((q for q in range(j + 1, len(body))
                          if re.match(r"\s*(s_endpgm|s_setprio\s+[1-9])", body[q])), len(body))
                return body[j + 1:k]
            i = j
        i += 1
    raise SystemExit("no interior window phase found")


def token(ln):
    t = ln.strip()
    if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
        return None
    op = t.split()[0]
    if op == "s_barrier":
        return "BARRIER"
    if op == "s_waitcnt":
        return "|" + " ".join(t.split()[1:]) + "|"
    m = re.match(r"ds_(read|write)(2?)_b(\d+)", op)
    if m:
        return ("r" if m.group(1) == "read" else "w") + m.group(2) + m.group(3)
    if op.startswith("ds_"):
        return "ds"
    if op.startswith("global_load"):
        return "G"
    if op.startswith("global_atomic_add"):
        return "ATOM"
    if op.startswith("global_store") or op.startswith("global_atomic"):
        return "S"
    if op.startswith("v_pk_fma_f32"):
        return "F"
    if op.startswith("v_"):
        return "v"
    return None


def rle(tokens):
    out, prev, n = [], None, 0
    for t in tokens + [None]:
        if t == prev:
            n += 1
            continue
        if prev is not None:
            out.append(prev if n == 1 or prev.startswith("|") else "%s%d" % (prev, n) if len(prev) == 1 else "%sx%d" % (prev, n))
        prev, n = t, 1
    return " ".join(out)


def check(segs):
    """the shape the fp32 R = 6 interior tile must keep: no barrier behind pass A's, pass B's 28 rows as single
    ds_read_b64 (no ds_read2_b64 pairing, no ds_read_b128 sweep), no O staging (ds_write2_b64), 100 + 16 packed FMAs"""
    bad = []
    if len(segs) != 3:
        bad.append("%d barriers after the window phase's own, expected 1" % (len(segs) - 2))
    b = segs[-1]
    n = lambda t: sum(x == t for x in b)
    if n("r64") < 28:
        bad.append("pass B: %d ds_read_b64, expected >= 28" % n("r64"))
    if n("r264"):
        bad.append("pass B: %d ds_read2_b64 (paired row reads)" % n("r264"))
    if n("r128") > 3:
        bad.append("pass B: %d ds_read_b128, expected <= 3 (TV chain only)" % n("r128"))
    if n("w264"):
        bad.append("pass B: O-staging stores")
    if n("F") != 116:
        bad.append("pass B: %d v_pk_fma_f32, expected 116" % n("F"))
    for m in bad:
        print("CHECK FAILED:", m)
    print("check:", "failed" if bad else "ok")
    return 1 if bad else 0


def main():
    checking = sys.argv[1] == "--check"
    if checking:
        del sys.argv[1]
    path = sys.argv[1]
    piece = sys.argv[2] if len(sys.argv) > 2 else "pgd_tv2d_kernelIfLi6E"
    text = open(path).read().split("\n")
    body = kernel_body(text, piece)
    toks = [t for t in (token(ln) for ln in interior(body)) if t]
    segs, cur = [], []
    for t in toks:
        if t == "BARRIER":
            segs.append(cur)
            cur = []
        else:
            cur.append(t)
    segs.append(cur)
    # the tile ends where the last-workgroup fold begins: the barrier before the counter's atomic add
    tail = next((i for i, s in enumerate(segs) if "ATOM" in s), len(segs))
    segs = segs[:tail]
    print("kernel piece %s: interior tile, %d barriers after the window phase's own" % (piece, len(segs) - 2))
    for i, s in enumerate(segs):
        c = {}
        for t in s:
            if not t.startswith("|"):
                c[t] = c.get(t, 0) + 1
        full = sum(t.startswith("|") and "lgkmcnt(0)" in t for t in s)
        print("segment %d: %s; lgkmcnt(0) waits %d" % (i, " ".join("%s=%d" % kv for kv in sorted(c.items())), full))
        print("   " + rle(s))
    if checking:
        sys.exit(check(segs))


if __name__ == "__main__":
    main()
