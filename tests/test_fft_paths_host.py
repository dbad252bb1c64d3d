"""
CPU checks that tie the FFT path tests to the dispatch of pyxu_amd/csrc/fft.hip.

* tests/_fft_paths.py mirrors that dispatch in Python.  Its workspace size equals pxa_fft_workspace_bytes (host
  arithmetic of the built library: runs without a GPU) for n = 1 .. 2999 and the lengths around every threshold
  above, with 1 and 3 lines, in both precisions -- so a change to stockham_fits / direct_fits / four_step_n1 /
  axis_work that the mirror does not follow fails here.
* The case table of tests/test_gpu_fft_paths.py (tests/_fft_cases.py) reaches every label of an explicit
  required set -- so a dispatch change that takes a case off the path it was chosen for fails here, on a CPU,
  instead of silently thinning the GPU tests.
"""
import math

import _fft_cases as C
import _fft_paths as P
import pytest

import pyxu_amd
from pyxu_amd._lib import i64_array, int_array

LONG = (4096, 4099, 5000, 5120, 5121, 5184, 6002, 8192, 8209, 10000, 10240, 10241, 10368, 12000, 16384, 32768, 65536,
        100003)


@pytest.mark.parametrize("dt,code", [(C.F32, 0), (C.F64, 1)])
def test_mirror_workspace_equals_library(dt, code):
    lib = pyxu_amd.lib
    ax = int_array([0])
    bad = []
    for n in (*range(1, 3000), *LONG):
        for lines in (1, 3):
            got = int(lib.pxa_fft_workspace_bytes(code, 1, i64_array([n]), 1, ax, lines))
            want = P.workspace_bytes((n,), (0,), lines, dt)
            if got != want:
                bad.append((n, lines, got, want))
    assert not bad, bad[:10]


def test_mirror_workspace_entry_checks():
    lib = pyxu_amd.lib
    big = (1 << 64) - 1
    for sh, axes, stack in (((5, 3, 4), (2, 0), 2), ((5, 3, 4), (0, 0), 2), ((5, 3, 4), (3,), 2), ((6002, 2), (), 1),
                            ((6002, 2), (1, 0), 0), ((2, 12000), (0, 1), 3), ((0, 4), (0,), 1)):
        got = int(lib.pxa_fft_workspace_bytes(1, len(sh), i64_array(sh), len(axes), int_array(axes), stack))
        assert got == P.workspace_bytes(sh, axes, stack, C.F64), (sh, axes, stack)
    assert P.workspace_bytes((5, 3, 4), (0, 0), 2, C.F64) == big and P.launches((5, 3, 4), (3,), 2, C.F32) is None
    assert [ln["kind"] for ln in P.launches((5, 3, 4), (), 2, C.F32)] == ["copy"]
    assert P.launches((5, 3, 4), (0,), 0, C.F32) == []


def test_mirror_known_dispatch():
    """Figures fft.hip's comments and the existing tests state, read off the mirror."""
    assert P.lds_elems(C.F32, 512) == 8192 and P.lds_elems(C.F64, 1024) == 8192
    assert P.four_step_n1(16384, C.F64) == 128 and P.four_step_n1(32768, C.F32) == 128
    assert P.four_step_n1(10290, C.F32) == 98 and P.four_step_n1(5145, C.F64) == 49
    assert P.stockham_fits(10240, C.F32) and not P.stockham_fits(10290, C.F32)
    assert P.stockham_fits(5120, C.F64) and not P.stockham_fits(5145, C.F64)
    assert P.factor_lds(1024, C.F32) == (16, 16, 4) and P.factor_lds(1024, C.F64) == (8, 8, 8, 2)
    assert P.next_pow2(2 * 4099 - 1) == 16384  # (not 8192)
    # 2048 x 2048, axis 0 then 1: line-fastest fast path, then whole lines
    a0, a1 = P.launches((2048, 2048), (0, 1), 1, C.F64)
    assert (a0["threads"], a0["lpb"], a1["threads"], a1["lpb"]) == (1024, 4, 512, 2)
    assert "lds:load:M1Flin:full" in a0["tags"] and "lds:store:M0F:full" in a1["tags"]
    # the tuning knob: bit 1024 takes every group off the fast path, 1 selects the ping-pong kernel
    assert not P.has_fast_path((2048, 2048), (0, 1), 1, C.F64, P.TUNE_NO_FAST)
    assert [ln["kind"] for ln in P.launches((2048, 2048), (0, 1), 1, C.F64, 1)] == ["pingpong", "pingpong"]


def test_case_table_reaches_required_paths():
    got = C.tags_of(C.CASES)
    missing = sorted(C.REQUIRED - got)
    assert not missing, f"no case of tests/_fft_cases.py reaches {missing}"


def test_case_table_shapes():
    ids = [C.case_id(c) for c in C.CASES]
    assert len(set(ids)) == len(ids)
    for fam, dt, sh, axes, stack in C.CASES:
        assert P.launches(sh, axes, stack, dt) is not None
    # the contiguous sweep: every power of two the in-LDS kernel takes, as two full groups and a one-line tail
    for dt, top in ((C.F32, 16384), (C.F64, 8192)):
        ns = [c[2][1] for c in C.POW2_CONTIG if c[1] == dt]
        assert ns == [2 ** k for k in range(1, int(math.log2(top)) + 1)]
        assert P.lds_fft_fits(top, dt) and not P.lds_fft_fits(2 * top, dt)
    for _, dt, (lines, n), _, stack in C.POW2_CONTIG:
        (ln,) = P.launches((lines, n), (1,), stack, dt)
        assert ln["kind"] == "lds" and ln["blocks"] == 3 and ln["lpb"] == (lines - 1) // 2
    # one impulse length per path family
    kinds = {fam: P.launches((n,), (0,), 1, C.F32)[0]["kind"] for fam, n in C.IMPULSE.items()}
    assert kinds == {"lds": "lds", "four": "four", "pp": "pingpong", "direct": "direct", "blue": "bluestein"}
    # (fp64 holds half as long a line: there 9261 is a 21 x 441 four-step, both passes on the ping-pong kernel)
    assert [ln["kind"] for ln in P.launches((C.IMPULSE["pp"],), (0,), 1, C.F64)][1::2] == ["pingpong", "pingpong"]


def test_fast_cases_cover_every_fast_mode():
    """The bit-equality test runs each of these with and without PXA_TUNE_FFT_KERNEL bit 1024: they hold every
    fast load / store mode in both precisions, and the bit removes every one of them."""
    assert C.HAZARD in C.FAST_CASES
    for dt in C.DTYPES:
        got = C.tags_of([c for c in C.FAST_CASES if c[1] == dt])
        for m in ("M0F", "M1F", "M1Flin"):
            assert {f"lds:load:{m}:full", f"lds:store:{m}:full"} <= got, (dt, m)
    for _, dt, sh, axes, stack in C.FAST_CASES:
        assert not P.has_fast_path(sh, axes, stack, dt, P.TUNE_NO_FAST)
        slow = [ln for ln in P.launches(sh, axes, stack, dt, P.TUNE_NO_FAST)]
        fast = [ln for ln in P.launches(sh, axes, stack, dt)]
        assert [(a["threads"], a["lpb"], a["radix"]) for a in slow] == [(a["threads"], a["lpb"], a["radix"]) for a in fast]
