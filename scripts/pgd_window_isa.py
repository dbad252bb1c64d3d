"""Static instruction counts of the PGD tile kernel from a device-only assembly listing of csrc/pgd_tv2d.hip
(hipcc <the Makefile's CXXFLAGS and PGD_FLAGS> --cuda-device-only -S pgd_tv2d.hip -o pgd.s):

    python3 scripts/pgd_window_isa.py pgd.s ["pgd_tv2d_kernelIfLi6E"]

Prints, for the kernel whose mangled name contains the given piece, the VALU / SALU / conditional-branch / saveexec
counts of the whole kernel and of each window phase (the code between a raised and a lowered s_setprio; the interior
tile's is the one whose loads are all 16-B), the division-like and 64-bit address instructions of each window phase,
and the kernel's register / scratch / occupancy figures.  The '64-bit address VALU' class includes v_mad_u64_u32, which the
compiler also emits for 32-bit multiply-adds, so it can over-count.

    python3 scripts/pgd_window_isa.py --all pgd.s [parent.s]

prints NumVgprs / ScratchSize / Occupancy of every instantiation of the three PGD kernels (tile, strip, pipe), beside
those of a second listing (the parent's) when given, and marks the instantiations that are worse than it.  Needs no GPU.
"""
import re
import sys

NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier", "s_setprio", "s_endpgm", "s_load_", "s_buffer_load_", "s_cbranch",
            "s_branch", "s_sleep", "s_code_end", "s_memtime", "s_memrealtime")
DIVLIKE = ("v_mul_hi_u32", "v_mul_hi_i32", "v_mul_u32_u24", "v_mul_i32_i24", "v_mul_hi_u32_u24", "v_mad_u32_u24",
           "v_mad_i32_i24", "v_mul_lo_u32")
ADDR64 = ("v_lshlrev_b64", "v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_addc_co_u32")


def ops(lines):
    out = []
    for ln in lines:
        t = ln.strip()
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        out.append(t.split()[0])
    return out


def counts(o):
    c = {
        "VALU": sum(x.startswith("v_") for x in o),
        "SALU": sum(x.startswith("s_") and not x.startswith(NOT_SALU) for x in o),
        "cbranch": sum(x.startswith("s_cbranch") for x in o),
        "saveexec": sum("saveexec" in x for x in o),
    }
    return c


def resources(path):
    """{demangled-ish kernel id: (NumVgprs, ScratchSize, Occupancy)} of every pgd_*_kernel in the listing"""
    text = open(path).read().split("\n")
    out = {}
    for i, ln in enumerate(text):
        m = re.match(r"^_Z\w*?\d+(pgd_(?:tv2d|strip|pipe)_kernel)I([fd])Li(\d)E\w*:", ln)
        if not m:
            continue
        end = next(q for q in range(i, len(text)) if text[q].startswith(".Lfunc_end"))
        meta = "\n".join(text[end:end + 80])
        vals = tuple(int(re.search(r";\s*%s:\s*(\d+)" % k, meta).group(1)) for k in ("NumVgprs", "ScratchSize", "Occupancy"))
        out["%s<%s, %s>" % (m.group(1), "float" if m.group(2) == "f" else "double", m.group(3))] = vals
    return out


def all_kernels(path, parent=None):
    new = resources(path)
    old = resources(parent) if parent else {}
    print("%-34s %s%s" % ("kernel", "VGPRs / scratch B / occupancy", "   (parent)" if parent else ""))
    worse = 0
    for k in sorted(new, key=lambda n: (n.split("<")[0], "double" in n, n)):
        v = new[k]
        line = "%-34s %4d / %4d / %d" % (k, *v)
        if k in old:
            o = old[k]
            bad = v[1] > o[1] or v[2] < o[2]
            worse += bad
            line += "      (%4d / %4d / %d)%s" % (*o, "   WORSE" if bad else "")
        print(line)
    if parent:
        print("instantiations with more scratch or lower occupancy than the parent: %d" % worse)


def main():
    if sys.argv[1] == "--all":
        all_kernels(*sys.argv[2:4])
        return
    path = sys.argv[1]
    piece = sys.argv[2] if len(sys.argv) > 2 else "pgd_tv2d_kernelIfLi6E"
    text = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(text) if re.match(r"^_Z\w*%s\w*:" % re.escape(piece), ln))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    body = text[start:end + 1]
    o = ops(body)
    print("kernel", text[start].rstrip(":"))
    print("  whole kernel:", counts(o))
    # window phases: s_setprio N (N > 0) ... s_setprio 0
    i, nwin = 0, 0
    while i < len(body):
        m = re.match(r"\s*s_setprio\s+(\d+)", body[i])
        if m and int(m.group(1)) > 0:
            j = next(q for q in range(i + 1, len(body)) if re.match(r"\s*s_setprio\s+0\b", body[q]))
            w = ops(body[i + 1:j])
            narrow = sum(x.startswith("global_load") and not x.startswith("global_load_dwordx4") for x in w)
            kind = "interior" if narrow == 0 else "edge"
            c = counts(w)
            c["f64 VALU"] = sum(x.startswith("v_") and "f64" in x for x in w)
            c["pk_f32"] = sum(x.startswith("v_pk_") for x in w)
            c["div-like int mul"] = sum(x in DIVLIKE for x in w)
            c["v_cndmask"] = sum(x.startswith("v_cndmask") for x in w)
            c["64-bit address VALU"] = sum(x in ADDR64 for x in w)
            c["global_load_dwordx4"] = sum(x.startswith("global_load_dwordx4") for x in w)
            c["ds_write_b128"] = sum(x.startswith("ds_write_b128") for x in w)
            print("  window phase %d (%s tile):" % (nwin, kind), c)
            nwin += 1
            i = j
        i += 1
    meta = "\n".join(text[end:end + 80])
    for key in ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
        m = re.search(r";\s*%s:\s*(\d+)" % key, meta)
        if m:
            print("  %s: %s" % (key, m.group(1)))


if __name__ == "__main__":
    main()
