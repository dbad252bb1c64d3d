"""
Host-only mirror of the FFT dispatch of pyxu_amd/csrc/fft.hip (pure Python, no torch, no NumPy).

Given (shape, axes, stack, dtype, tuning) `launches` lists what fft_entry enqueues, one record per kernel
launch or copy, each with a readable `label` and a set of `tags` naming the code paths the launch takes.  The
tests use it to choose shapes (tests/test_gpu_fft_paths.py) and to prove on a CPU that those shapes reach every
path they are meant to reach (tests/test_fft_paths_host.py, which also holds the mirror to the library:
`workspace_bytes` against pxa_fft_workspace_bytes over a sweep of lengths).

Mirrored functions, by their names in fft.hip: smooth, factor, factor_lds, stockham_fits, direct_fits,
lds_fft_fits, four_step_n1, next_pow2, axis_work, fft_work_elems, lds_fft_threads, launch_lds_fft_th (and the
per-group load / store mode selection of fft_lds_kernel), launch_stockham, launch_direct, fft_axis, fft_entry.
A change to any of them belongs here too.

Tags
  lds:th512 | lds:th1024                    workgroup size of fft_lds_kernel
  lds:load:<mode> | lds:store:<mode>        <mode> = M0|M1|M2 (position-fastest, line-fastest with a fixed line
                                            per thread, line-fastest with the multiply-high divide) + F|G (raw-
                                            buffer fast path, generic 64-bit path) + T (four-step transposed
                                            store) + lin (fast line-fastest path with a linear swizzle)
  ...:<mode>:full | ...:<mode>:partial      the group fills the workgroup's E elements or not
  ...:<mode>:full:straddle (or partial)     the group's lines lie in two outer blocks of a strided axis
  lds:tail                                  full-size groups followed by a smaller last group in one launch
  lds:fast+generic-tail                     ... the former on the fast path, the latter on the generic one
  lds:nb%8 | lds:nb>8:nb%8                  group count no multiple of 8 (XCD band reorder with a remainder)
  lds:radix:<f32|f64>:<r0,r1,..>            stage list
  lds:stage:read-lin|read-swz|write-lin|write-swz   per-stage LDS addressing variants (nr & 127, ns & 127)
  pp:contig | pp:strided, pp:lpb<k>, pp:tail, pp:straddle, pp:T, pp:smem>64K, pp:radix<r>, pp:smem>64K:radix<r>,
  pp:pure<r> (length a power of the odd radix r), pp:edge:<f32|f64> (the last resident length of the precision)
  direct:per<k> (results per thread), direct:contig | direct:strided, direct:edge (the longest
  non-smooth length of its envelope), direct:prime |
  direct:composite
  four:<n1>x<n2>, four:<f32|f64>:lds | four:<f32|f64>:pp (kernel of its two passes), four:contig | four:strided
  blue:m<m>, blue:contig | blue:strided, blue:edge (n just above the direct envelope), blue:composite |
  blue:prime, blue:inner:lds | blue:inner:pp | blue:inner:four, blue:<f32|f64>:inner:four
  twiddle, copy, copy:noaxes
"""
import math

K_FFT_THREADS = 256
K_FFT_LDS = 64 * 1024
K_FFT_LDS_MAX = 160 * 1024
K_DIRECT_MAX_N = 8 * K_FFT_THREADS
K_MAX_STAGES = 24

TUNE_PINGPONG_MASK = 15  # PXA_TUNE_FFT_KERNEL & 15 != 0: the ping-pong kernel for every resident length
TUNE_TH512, TUNE_TH1024, TUNE_NO_FAST = 256, 512, 1024


def csize(dtype):
    """bytes of one complex element; dtype: 'f32' / 'f64', 'float32' / 'float64' or anything named so"""
    name = dtype if isinstance(dtype, str) else getattr(dtype, "__name__", str(dtype))
    if name in ("f32", "float32", "single"):
        return 8
    if name in ("f64", "float64", "double"):
        return 16
    raise ValueError(f"dtype {dtype!r}")


def dname(dtype):
    return "f32" if csize(dtype) == 8 else "f64"


def smooth(n):
    for r in (2, 3, 5, 7):
        while n % r == 0:
            n //= r
    return n == 1


def is_prime(n):
    return n >= 2 and all(n % d for d in range(2, math.isqrt(n) + 1))


def _factor(n, radices):
    out = []
    for r in radices:
        while n % r == 0:
            if len(out) == K_MAX_STAGES:
                return None
            out.append(r)
            n //= r
    return tuple(out) if n == 1 else None


def factor(n):
    """stage list of the ping-pong kernel (None: not smooth / too many stages)"""
    return _factor(n, (8, 4, 2, 3, 5, 7))


def factor_lds(n, dtype):
    """stage list of the in-LDS kernel"""
    return _factor(n, (16 if csize(dtype) == 8 else 8, 8, 4, 2))


def stockham_fits(n, dtype):
    return smooth(n) and 2 * n * csize(dtype) <= K_FFT_LDS_MAX


def direct_fits(n, dtype):
    return n <= K_DIRECT_MAX_N and n * csize(dtype) <= K_FFT_LDS_MAX


def lds_elems(dtype, th):
    """LdsFft<T, TH>::E"""
    return th * 128 // csize(dtype)


def fft_pitch(n, L):
    return n + 16 // min(L, 16)


def lds_fft_fits(n, dtype):
    return (2 <= n <= lds_elems(dtype, 1024) and n & (n - 1) == 0
            and fft_pitch(n, 1) * csize(dtype) <= K_FFT_LDS_MAX)


def four_step_n1(n, dtype):
    if not smooth(n):
        return 0
    for n1 in range(math.isqrt(n) + 1, 1, -1):
        if n % n1 == 0 and n1 * n1 <= n and stockham_fits(n1, dtype) and stockham_fits(n // n1, dtype):
            return n1
    return 0


def next_pow2(v):
    m = 1
    while m < v:
        m <<= 1
    return m


def axis_work(n, lines, dtype):
    """workspace (complex elements) of one axis transform; -1: unsupported"""
    if n == 1 or stockham_fits(n, dtype) or (not smooth(n) and direct_fits(n, dtype)):
        return 0
    if smooth(n):
        return n * lines if four_step_n1(n, dtype) else -1
    m = next_pow2(2 * n - 1)
    inner = axis_work(m, lines, dtype)
    return -1 if inner < 0 else lines * m + m + inner


def _check(shape, axes, stack):
    """fft_check: total element count, or None for PXA_ERR_ARG"""
    ndim = len(shape)
    if not (1 <= ndim <= 8 and 0 <= len(axes) <= ndim and stack >= 0):
        return None
    total = stack
    for s in shape:
        if s < 1:
            return None
        total *= s
    for i, a in enumerate(axes):
        if not 0 <= a < ndim or a in axes[:i]:
            return None
    return total


def workspace_bytes(shape, axes, stack, dtype):
    """pxa_fft_workspace_bytes; (size_t)-1 as 2**64 - 1"""
    total = _check(shape, axes, stack)
    if total is None:
        return (1 << 64) - 1
    need = 0
    if total > 0:
        for a in axes:
            w = axis_work(shape[a], total // shape[a], dtype)
            if w < 0:
                return (1 << 64) - 1
            need = max(need, w)
    return need * csize(dtype)


def lds_fft_threads(n, inner, dtype, tuning=0):
    e512 = lds_elems(dtype, 512)
    if n > e512 or tuning & TUNE_TH1024:
        return 1024
    if tuning & TUNE_TH512:
        return 512
    return 1024 if inner > 1 and 2 * n >= e512 else 512


def lds_lines_per_group(n, inner, lines, dtype, tuning=0):
    """(threads, L) of launch_lds_fft_th"""
    th = lds_fft_threads(n, inner, dtype, tuning)
    L = lds_elems(dtype, th) // n
    L = min(L, lines)
    if inner > 1:
        L = min(L, inner)
    L = max(L, 1)
    while L > 1 and L * fft_pitch(n, L) * csize(dtype) > K_FFT_LDS_MAX:
        L //= 2
    return th, L


def _straddles(first_line, nl, inner):
    return inner > 1 and first_line // inner != (first_line + nl - 1) // inner


def _group_kinds(lines, L, inner):
    """[(count, lines in the group, straddles an outer block)] of the full-size groups and of the last, smaller one"""
    nfull, tail = divmod(lines, L)
    kinds = []
    if nfull:
        strad = inner > 1 and inner % L != 0 and any(_straddles(g * L, L, inner) for g in range(nfull))
        kinds.append((nfull, L, strad))
    if tail:
        kinds.append((1, tail, _straddles(nfull * L, tail, inner)))
    return kinds


def _lds_modes(n, inner, tn1, L, th, dtype, no_fast):
    """(load mode, store mode) of one group of L lines in fft_lds_kernel"""
    full = L * n == lds_elems(dtype, th)
    fixed_line = th % L == 0
    span_ok = n * inner * csize(dtype) < 1 << 31

    def mode(lf, out):
        transposed = out and tn1 > 0
        fast = (not no_fast) and full and (not lf or (not transposed and fixed_line and inner % L == 0 and span_ok))
        m = "M0" if not lf else ("M1" if fixed_line else "M2")
        m += "F" if fast else "G"
        if transposed:
            m += "T"
        if fast and lf and ((th // L) & 127) == 0:
            m += "lin"
        return m

    return mode(inner != 1, False), mode(tn1 > 0 or inner != 1, True), full


def _launch_lds(n, inner, lines, tn1, dtype, tuning):
    th, L = lds_lines_per_group(n, inner, lines, dtype, tuning)
    radix = factor_lds(n, dtype)
    no_fast = bool(tuning & TUNE_NO_FAST)
    nb = -(-lines // L)
    d = dname(dtype)
    tags = {f"lds:th{th}", f"lds:radix:{d}:{','.join(map(str, radix))}"}
    parts = []
    kinds = _group_kinds(lines, L, inner)
    fast_main = fast_any = False
    for i, (count, nl, strad) in enumerate(kinds):
        ld, st, full = _lds_modes(n, inner, tn1, nl, th, dtype, no_fast)
        fill = "full" if full else "partial"
        for what, m in (("load", ld), ("store", st)):
            tags |= {f"lds:{what}:{m}", f"lds:{what}:{m}:{fill}"}
            if strad and m[:2] != "M0":
                tags.add(f"lds:{what}:{m}:{fill}:straddle")
        fast_any |= ld[2] == "F" or st[2] == "F"
        if i == 0 and nl == L:
            fast_main = ld[2] == "F" or st[2] == "F"
        parts.append(f"{count}x{nl}:{ld}>{st}:{fill}" + (":straddle" if strad else ""))
    if len(kinds) == 2:
        tags.add("lds:tail")
        ld, st, _ = _lds_modes(n, inner, tn1, kinds[1][1], th, dtype, no_fast)
        if fast_main and ld[2] == "G" and st[2] == "G":
            tags.add("lds:fast+generic-tail")
    if nb % 8:
        tags.add("lds:nb%8")
        if nb > 8:
            tags.add("lds:nb>8:nb%8")
    ns = 1
    for r in radix:
        tags.add("lds:stage:read-lin" if (n // r) & 127 == 0 else "lds:stage:read-swz")
        tags.add("lds:stage:write-lin" if ns & 127 == 0 else "lds:stage:write-swz")
        ns *= r
    smem = L * fft_pitch(n, L) * csize(dtype)
    assert smem <= K_FFT_LDS_MAX
    return dict(kind="lds", n=n, inner=inner, lines=lines, tn1=tn1, threads=th, lpb=L, blocks=nb, radix=radix,
                smem=smem, fast=fast_any, tags=tags, label=f"lds{th} n={n} inner={inner} " + " + ".join(parts) + f" nb={nb} r={radix}")


def _launch_stockham(n, inner, lines, tn1, dtype):
    radix = factor(n)
    if radix is None:
        return None
    line_bytes = n * csize(dtype)
    lpb = max(1, min(16, K_FFT_LDS // (2 * line_bytes)))
    if inner > 1 and lpb > inner:
        lpb = inner
    smem = 2 * lpb * line_bytes
    if smem > K_FFT_LDS_MAX:
        return None
    d = dname(dtype)
    tags = {"pp:contig" if inner == 1 else "pp:strided", f"pp:lpb{lpb}"}
    tags |= {f"pp:radix{r}" for r in set(radix)}
    big = smem > K_FFT_LDS
    if big:
        tags.add("pp:smem>64K")
        tags |= {f"pp:smem>64K:radix{r}" for r in set(radix)}
    for r in (3, 5, 7):
        if set(radix) == {r}:
            tags.add(f"pp:pure{r}")
    if n == K_FFT_LDS_MAX // (2 * csize(dtype)):
        tags.add(f"pp:edge:{d}")
    tail = lines % lpb != 0
    strad = any(s for _, _, s in _group_kinds(lines, lpb, inner))
    if tail:
        tags.add("pp:tail")
    if strad:
        tags.add("pp:straddle")
    if tn1 > 0:
        tags.add("pp:T")
    return dict(kind="pingpong", n=n, inner=inner, lines=lines, tn1=tn1, lpb=lpb, blocks=-(-lines // lpb), radix=radix,
                smem=smem, fast=False, tags=tags,
                label=f"pp {d} n={n} inner={inner} lines={lines} lpb={lpb}" + (" tail" if tail else "")
                + (" straddle" if strad else "") + (" T" if tn1 > 0 else "") + (" smem>64K" if big else "")
                + f" r={sorted(set(radix))}")


def _launch_lines(n, inner, lines, tn1, dtype, tuning):
    if tuning & TUNE_PINGPONG_MASK == 0 and lds_fft_fits(n, dtype):
        return _launch_lds(n, inner, lines, tn1, dtype, tuning)
    return _launch_stockham(n, inner, lines, tn1, dtype)


def fft_axis(n, inner, lines, dtype, tuning=0):
    """launches of one axis transform (None: unsupported)"""
    d = dname(dtype)
    where = "contig" if inner == 1 else "strided"
    if stockham_fits(n, dtype) or (tuning & TUNE_PINGPONG_MASK == 0 and lds_fft_fits(n, dtype)):
        r = _launch_lines(n, inner, lines, 0, dtype, tuning)
        return None if r is None else [r]
    if not smooth(n) and direct_fits(n, dtype):
        per = -(-n // K_FFT_THREADS)
        tags = {f"direct:per{per}", f"direct:{where}", "direct:prime" if is_prime(n) else "direct:composite"}
        if n == K_DIRECT_MAX_N or not any(not smooth(k) for k in range(n + 1, K_DIRECT_MAX_N + 1)):
            tags.add("direct:edge")
        return [dict(kind="direct", n=n, inner=inner, lines=lines, per=per, fast=False, tags=tags,
                     label=f"direct {d} n={n} inner={inner} lines={lines} per={per}")]
    if axis_work(n, lines, dtype) < 0:
        return None
    if smooth(n):
        n1 = four_step_n1(n, dtype)
        n2 = n // n1
        a = _launch_lines(n1, n2 * inner, n * lines // n1, 0, dtype, tuning)
        b = _launch_lines(n2, inner, n * lines // n2, n1, dtype, tuning)
        if a is None or b is None:
            return None
        kern = {"lds": "lds", "pingpong": "pp"}
        tags = {f"four:{n1}x{n2}", f"four:{where}", f"four:{d}:{kern[a['kind']]}", f"four:{d}:{kern[b['kind']]}"}
        head = dict(kind="four", n=n, n1=n1, n2=n2, inner=inner, lines=lines, fast=False, tags=tags,
                    label=f"four-step {d} n={n} = {n1} x {n2} inner={inner} lines={lines}")
        tw = dict(kind="twiddle", fast=False, tags={"twiddle"}, label=f"four-step twiddle {n1} x {n2}")
        cp = dict(kind="copy", fast=False, tags={"copy"}, label="copy back from the workspace")
        return [head, a, tw, b, cp]
    m = next_pow2(2 * n - 1)
    sub = [fft_axis(m, 1, lines, dtype, tuning), fft_axis(m, 1, 1, dtype, tuning), fft_axis(m, 1, lines, dtype, tuning)]
    if any(s is None for s in sub):
        return None
    inner_kind = {"lds": "lds", "pingpong": "pp", "four": "four"}[sub[0][0]["kind"]]
    tags = {f"blue:m{m}", f"blue:{where}", "blue:prime" if is_prime(n) else "blue:composite",
            f"blue:inner:{inner_kind}", f"blue:{d}:inner:{inner_kind}"}
    if not any(not smooth(k) for k in range(K_DIRECT_MAX_N + 1, n)):
        tags.add("blue:edge")
    head = dict(kind="bluestein", n=n, m=m, inner=inner, lines=lines, fast=False, tags=tags,
                label=f"bluestein {d} n={n} m={m} inner={inner} lines={lines} inner transform {inner_kind}")
    aux = lambda s: dict(kind="bluestein_aux", fast=False, tags=set(), label=f"bluestein {s}")  # noqa: E731
    return [head, aux("chirp in"), aux("filter"), *sub[0], *sub[1], aux("product"), *sub[2], aux("chirp out")]


def launches(shape, axes, stack, dtype, tuning=0, in_place=False):
    """what fft_entry enqueues for these arguments (None: PXA_ERR_ARG / PXA_ERR_UNSUPPORTED)"""
    shape, axes = tuple(int(s) for s in shape), tuple(int(a) for a in axes)
    total = _check(shape, axes, stack)
    if total is None:
        return None
    out = []
    if total == 0:
        return out
    for a in axes:
        n = shape[a]
        if n == 1:
            continue
        inner = 1
        for s in shape[a + 1:]:
            inner *= s
        r = fft_axis(n, inner, total // n, dtype, tuning)
        if r is None:
            return None
        out += r
    if not out and not in_place:
        out.append(dict(kind="copy", fast=False, tags={"copy", "copy:noaxes"}, label="plain copy (no axis transformed)"))
    return out


def tags(shape, axes, stack, dtype, tuning=0):
    got = set()
    for ln in launches(shape, axes, stack, dtype, tuning):
        got |= ln["tags"]
    return got


def has_fast_path(shape, axes, stack, dtype, tuning=0):
    """some group of some in-LDS launch loads or stores by the raw-buffer fast path"""
    return any(ln["fast"] for ln in launches(shape, axes, stack, dtype, tuning))


def describe(shape, axes, stack, dtype, tuning=0):
    return [ln["label"] for ln in launches(shape, axes, stack, dtype, tuning)]
