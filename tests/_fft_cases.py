"""
The case table of tests/test_gpu_fft_paths.py, kept apart from it (pure Python) so that
tests/test_fft_paths_host.py can check on a CPU, with the dispatch mirror tests/_fft_paths.py, that the cases
reach every path of pyxu_amd/csrc/fft.hip they are meant to reach (REQUIRED below).

A case is (family, dtype, shape, axes, stack); its id is "<family>-<dtype>-<shape>-<axes>-s<stack>".
"""
import _fft_paths as P

F32, F64 = "float32", "float64"
DTYPES = (F32, F64)


def case_id(c):
    fam, dt, sh, axes, stack = c
    return f"{fam}-{P.dname(dt)}-{'x'.join(map(str, sh))}-ax{''.join(map(str, axes))}-s{stack}"


def sweep_lines(n, dt):
    """L of the contiguous power-of-two sweep: the lines of one full group of the in-LDS kernel"""
    th = P.lds_fft_threads(n, 1, dt)
    return max(1, P.lds_elems(dt, th) // n)


def _pow2_contig():
    # (2 L + 1, n): two full groups on the fast path, a one-line tail group on the generic one, three groups
    out = []
    for dt, top in ((F32, 16384), (F64, 8192)):
        n = 2
        while n <= top:
            out.append(("pow2c", dt, (2 * sweep_lines(n, dt) + 1, n), (1,), 1))
            n *= 2
    return out


def _pow2_strided():
    out = []
    for dt in DTYPES:
        for n in (8, 128, 1024, 4096):
            for inner in (3, 48, 64):
                out.append(("pow2s", dt, (n, inner), (0,), 2))
        out.append(("pow2s", dt, (2, 256, 48), (1,), 2))
    # more lines per group than threads divide (L = 1024 of 512 threads): full M2 groups that straddle the outer block
    out += [("pow2s", F32, (8, 1500), (0,), 2), ("pow2s", F64, (4, 1500), (0,), 2)]
    return out


POW2_CONTIG = _pow2_contig()
POW2_STRIDED = _pow2_strided()
FOUR_STEP = [("four", F32, (32768,), (0,), 2), ("four", F32, (32768, 3), (0,), 2),
             ("four", F64, (16384, 3), (0,), 2), ("four", F64, (16384, 40), (0,), 2)]
PINGPONG = ([("pp", F32, (n,), (0,), 3) for n in (49, 81, 343, 625, 2401, 3125, 6561, 9261, 10000, 10240, 10290)]
            + [("pp", F32, (10000, 3), (0,), 2)]
            + [("pp", F64, (n,), (0,), 3) for n in (2401, 3125, 4375, 5000, 5120, 5145)]
            + [("pp", F64, (5000, 3), (0,), 2)])
DIRECT = [("direct", dt, sh, (0,), 2) for dt in DTYPES
          for sh in ((257,), (509,), (521,), (2039,), (2046,), (2047,), (2039, 2), (521, 5))]
BLUESTEIN = [("blue", dt, sh, (0,), 2) for dt in DTYPES for sh in ((2053, 3), (2049,), (8209,))]

CASES = POW2_CONTIG + POW2_STRIDED + FOUR_STEP + PINGPONG + DIRECT + BLUESTEIN

# fast path against generic path, bit for bit: every power-of-two case with a fast group, and the shape family
# of the fp64 store corruption fft_lds_kernel once shipped (2048^2 axis 0) at a fraction of its size
HAZARD = ("pow2s", F64, (2048, 64), (0,), 2)
FAST_CASES = [c for c in POW2_CONTIG + POW2_STRIDED + [HAZARD] if P.has_fast_path(c[2], c[3], c[4], c[1])]

# one length per path family, for the unit-impulse test
IMPULSE = {"lds": 1024, "four": 32768, "pp": 9261, "direct": 2039, "blue": 2053}


def tags_of(cases, tuning=0):
    got = set()
    for _, dt, sh, axes, stack in cases:
        got |= P.tags(sh, axes, stack, dt, tuning)
    return got


# Every path the table must reach.  A dispatch change that takes a case off its path fails
# tests/test_fft_paths_host.py::test_case_table_reaches_required_paths: move the case, do not trim this set.
REQUIRED = {
    # in-LDS kernel: both workgroup sizes, every stage list of both precisions, both LDS addressing variants
    "lds:th512", "lds:th1024",
    *{f"lds:radix:f32:{r}" for r in ("2", "4", "8", "16", "16,2", "16,4", "16,8", "16,16", "16,16,2", "16,16,4",
                                     "16,16,8", "16,16,16", "16,16,16,2", "16,16,16,4")},
    *{f"lds:radix:f64:{r}" for r in ("2", "4", "8", "8,2", "8,4", "8,8", "8,8,2", "8,8,4", "8,8,8", "8,8,8,2",
                                     "8,8,8,4", "8,8,8,8", "8,8,8,8,2")},
    "lds:stage:read-lin", "lds:stage:read-swz", "lds:stage:write-lin", "lds:stage:write-swz",
    # contiguous axis: full fast groups and a partial generic tail group in one launch, nb % 8 != 0
    "lds:load:M0F:full", "lds:store:M0F:full", "lds:load:M0G:partial", "lds:store:M0G:partial",
    "lds:tail", "lds:fast+generic-tail", "lds:nb%8", "lds:nb>8:nb%8",
    # strided axis
    "lds:load:M2G:partial", "lds:store:M2G:partial", "lds:load:M1G:partial", "lds:store:M1G:partial",
    "lds:load:M1F:full", "lds:store:M1F:full", "lds:load:M1Flin:full", "lds:store:M1Flin:full",
    "lds:load:M1G:full:straddle", "lds:store:M1G:full:straddle",
    "lds:load:M2G:full:straddle", "lds:store:M2G:full:straddle",
    # four-step through the in-LDS kernel, both precisions: the transposed store from a contiguous axis, in M1
    # generic, in M2, and with straddling groups
    "four:f32:lds", "four:f64:lds", "four:128x256", "four:128x128", "four:contig", "four:strided",
    "lds:store:M1GT:full", "lds:store:M2GT:partial", "lds:store:M1GT:full:straddle",
    # ping-pong kernel: every radix, pure odd powers, above 64 KB of LDS with each odd radix, both LDS edges,
    # strided, tail groups, four-step on it
    *{f"pp:radix{r}" for r in (8, 4, 2, 3, 5, 7)}, "pp:pure3", "pp:pure5", "pp:pure7",
    "pp:smem>64K:radix3", "pp:smem>64K:radix5", "pp:smem>64K:radix7", "pp:edge:f32", "pp:edge:f64", "pp:contig", "pp:strided",
    "pp:tail", "pp:T", "four:f32:pp", "four:f64:pp", "four:98x105", "four:49x105",
    # direct kernel: 2 .. 8 results per thread (the length decides), primes and composites, the top of its envelope
    "direct:per2", "direct:per3", "direct:per8", "direct:edge", "direct:prime", "direct:composite",
    "direct:contig", "direct:strided",
    # Bluestein: strided, at its lower edge on a composite, with a four-step inner transform in both precisions
    "blue:strided", "blue:contig", "blue:edge", "blue:composite", "blue:prime", "blue:inner:lds",
    "blue:f32:inner:four", "blue:f64:inner:four", "blue:m8192", "blue:m32768",
}
