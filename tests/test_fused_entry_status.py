"""
Status codes of the fused PDS and PGD entry points for calls the host rejects (no GPU needed).

Every call here is one the C-ABI turns down during argument validation: it returns before any HIP call, so the
array arguments are small fake addresses that are never dereferenced (all 16-byte aligned and distinct, so no
case depends on an alignment choice or on accidental aliasing).  Geometry, tap and scalar arrays are real: the
validation reads them.  There is deliberately no accepted call in this file.

The expected codes are literals: PXA_ERR_ARG = -1, PXA_ERR_DTYPE = -2, PXA_ERR_UNSUPPORTED = -3.
"""
import ctypes as ct

import pytest

import pyxu_amd
from pyxu_amd._lib import f64_array, i32_array, i64_array

lib = pyxu_amd.lib

ARG, DTYPE, UNSUPPORTED = -1, -2, -3
W = 17  # tap slots per axis (2 * 8 + 1)


def _ptrs(*names):
    """name -> fake device address: 16-byte aligned, distinct, never dereferenced."""
    return {n: 0x10000 + 0x100 * i for i, n in enumerate(names)}


def _taps(per_axis):
    """(ntaps, offs, coefs) arrays of the PDS entry points from [(offsets, coefficients)] per axis."""
    offs, cfs = [], []
    for o, c in per_axis:
        offs += list(o) + [0] * (W - len(o))
        cfs += list(c) + [0.0] * (W - len(c))
    return [len(o) for o, _ in per_axis], offs, cfs


BLUR = ([-1, 0, 1], [0.25, 0.5, 0.25])
REACH2 = ([-2, -1, 0, 1], [0.2, 0.5, -0.1, 0.2])  # axis-0 reach 2: slab ghost depths 4 (src, z_hi) and 5 (z_lo)
DIFF = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
SCAL = [0.9, 0.1, 0.95, 0.05, 0.01]


def _pds_base(**kw):
    """Arguments of an otherwise valid PD3O step on a blurred (2, 6, 9, 12) stack; `kw` overrides."""
    a = dict(dtype=0, algo=0, geom=[2, 1, 6, 9, 12, 3], taps=[REACH2, BLUR, BLUR], ntaps=None, diff=DIFF, scal=SCAL,
             prox=1, h_kind=1, primed=0, nseg=0, ghost=None, src_lo=None, src_hi=None, z_lo=None, z_hi=None)
    a.update(_ptrs("x", "u", "z", "hty", "x_out", "u_out", "z_out", "work_q", "work_kt", "work_w"))
    a.update(kw)
    return a


def _pds_head(a):
    nt, offs, cfs = _taps(a["taps"])
    if a["ntaps"] is not None:
        nt = a["ntaps"]
    return [a["dtype"], a["algo"], i64_array(a["geom"]), i32_array(nt), i32_array(offs), f64_array(cfs),
            f64_array(a["diff"]), f64_array(a["scal"]), a["prox"], a["h_kind"]]


def pds_step(**kw):
    a = _pds_base(**kw)
    return lib.pxa_pds_step(*_pds_head(a), a["x"], a["u"], a["z"], a["hty"], a["x_out"], a["u_out"], a["z_out"],
                            a["work_q"], a["work_w"], a["nseg"], None)


def pds_step_la(**kw):
    a = _pds_base(**kw)
    return lib.pxa_pds_step_la(*_pds_head(a), a["primed"], a["x"], a["u"], a["z"], a["hty"], a["x_out"], a["u_out"],
                               a["z_out"], a["work_q"], a["work_kt"], a["work_w"], a["nseg"], None)


def pds_slab_primal(**kw):
    a = _pds_base(**kw)
    ghost = None if a["ghost"] is None else i64_array(a["ghost"])
    return lib.pxa_pds_slab_primal(*_pds_head(a), a["x"], a["u"], a["z"], a["hty"], a["x_out"], a["u_out"],
                                   a["work_q"], a["work_w"], ghost, a["src_lo"], a["src_hi"], a["z_lo"], a["z_hi"],
                                   a["nseg"], None)


PDS_ENTRIES = [pds_step, pds_step_la, pds_slab_primal]

# rejected by every step entry point: (why, overrides, status)
PDS_COMMON = [
    ("dtype 7", dict(dtype=7), DTYPE),
    ("algo 2", dict(algo=2), ARG),
    ("D = 4", dict(geom=[2, 1, 6, 9, 12, 4]), ARG),
    ("stack 65536", dict(geom=[65536, 1, 6, 9, 12, 3]), ARG),
    ("stack % y_images", dict(geom=[3, 2, 6, 9, 12, 3]), ARG),
    ("tap at offset 9", dict(taps=[REACH2, ([9, 0, -1], [0.25, 0.5, 0.25]), BLUR]), UNSUPPORTED),
    ("ntaps 0", dict(ntaps=[4, 0, 3]), ARG),
    ("null hty", dict(hty=None), ARG),
    ("PD3O, null u", dict(u=None), ARG),
    ("Condat-Vu, x_out == x", dict(algo=1, x_out=_ptrs("x")["x"]), ARG),
    ("blurred axis 0, null work_q", dict(work_q=None), ARG),
]


@pytest.mark.parametrize("entry", PDS_ENTRIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("why,kw,status", PDS_COMMON, ids=[c[0] for c in PDS_COMMON])
def test_step_entries_reject(entry, why, kw, status):
    assert entry(**kw) == status, why


def test_look_ahead_step_rejects():
    p = _ptrs("x", "u", "z")
    assert pds_step_la(z_out=p["z"]) == ARG  # neighbours read z while z_out is written
    assert pds_step_la(algo=1, z_out=p["z"]) == ARG
    assert pds_step_la(algo=1, work_kt=None) == ARG  # Condat-Vu keeps K^T z there
    assert pds_step_la(x=None) == ARG


# ghost cases of tests/test_gpu_pds_slab.py::test_argument_errors_launch_nothing: the valid depths are (4, 4, 5, 4)
G = _ptrs("src_lo", "src_hi", "z_lo", "z_hi")
G = {k: v + 0x100000 for k, v in G.items()}
SLAB_GHOSTS = [
    ("src_lo below 2 R0", dict(ghost=[3, 4, 5, 4], **G)),
    ("z_lo below 2 R0 + 1", dict(ghost=[4, 4, 4, 4], **G)),
    ("z_hi below 2 R0", dict(ghost=[4, 4, 5, 3], **G)),
    ("src_hi below 2 R0", dict(ghost=[4, 2, 5, 4], **G)),
    ("z_lo without src_lo", dict(ghost=[0, 4, 5, 4], **dict(G, src_lo=None))),
    ("Condat-Vu: x ghosts without z_lo", dict(algo=1, ghost=[4, 4, 0, 0], **dict(G, z_lo=None, z_hi=None))),
    ("ghosts with D = 2", dict(geom=[2, 1, 6, 9, 12, 2], ghost=[4, 4, 5, 4], **G)),
    ("n0 = 1 image with ghosts", dict(geom=[2, 1, 1, 9, 12, 2], ghost=[4, 4, 5, 4], **G)),
    ("n0 = 1 image without ghosts", dict(geom=[2, 1, 1, 9, 12, 2], ghost=[0, 0, 0, 0])),
    ("n0 = 1 image, no ghost array", dict(geom=[2, 1, 1, 9, 12, 2])),
    ("ghost pointers without depths", dict(ghost=None, **G)),
    ("negative depth", dict(ghost=[4, 4, -1, 4], **G)),
    ("src_lo aliases x_out", dict(ghost=[4, 4, 5, 4], **dict(G, src_lo=_pds_base()["x_out"]))),
    ("z_hi aliases work_w", dict(ghost=[4, 4, 5, 4], **dict(G, z_hi=_pds_base()["work_w"]))),
    ("src_hi aliases u_out", dict(ghost=[4, 4, 5, 4], **dict(G, src_hi=_pds_base()["u_out"]))),
    ("z_lo aliases work_q", dict(ghost=[4, 4, 5, 4], **dict(G, z_lo=_pds_base()["work_q"]))),
]


@pytest.mark.parametrize("why,kw", SLAB_GHOSTS, ids=[c[0] for c in SLAB_GHOSTS])
def test_slab_primal_rejects_ghosts(why, kw):
    assert pds_slab_primal(**kw) == ARG, why


def _dual_base(**kw):
    a = dict(dtype=0, relax=0, geom=[2, 6, 9, 12, 3], diff=DIFF, sigma=0.1, lam=0.05, rho=0.95, h_kind=1, w_hi=None,
             depth=0)
    a.update(_ptrs("w", "z", "z_out"))
    a.update(kw)
    return a


def tv_dual_update(**kw):
    a = _dual_base(**kw)
    return lib.pxa_tv_dual_update(a["dtype"], a["relax"], i64_array(a["geom"]), f64_array(a["diff"]), a["sigma"],
                                  a["lam"], a["rho"], a["h_kind"], a["w"], a["z"], a["z_out"], None)


def pds_slab_dual(**kw):
    a = _dual_base(**kw)
    return lib.pxa_pds_slab_dual(a["dtype"], a["relax"], i64_array(a["geom"]), f64_array(a["diff"]), a["sigma"],
                                 a["lam"], a["rho"], a["h_kind"], a["w"], a["w_hi"], a["depth"], a["z"], a["z_out"],
                                 None)


DUAL_COMMON = [
    ("dtype 7", dict(dtype=7), DTYPE),
    ("relax 2", dict(relax=2), ARG),
    ("h_kind 2", dict(h_kind=2), ARG),
    ("z_out == w", dict(z_out=_ptrs("w")["w"]), ARG),
    ("D = 4", dict(geom=[2, 6, 9, 12, 4]), ARG),
    ("stack 65536", dict(geom=[65536, 6, 9, 12, 3]), ARG),
    ("null z", dict(z=None), ARG),
]


@pytest.mark.parametrize("entry", [tv_dual_update, pds_slab_dual], ids=lambda f: f.__name__)
@pytest.mark.parametrize("why,kw,status", DUAL_COMMON, ids=[c[0] for c in DUAL_COMMON])
def test_dual_entries_reject(entry, why, kw, status):
    assert entry(**kw) == status, why


def test_dual_entries_reject_their_own_conditions():
    wh = 0x200000
    assert tv_dual_update(geom=[2, 6, 9, 12, 2]) == ARG  # D = 2 is for n0 = 1 images
    assert pds_slab_dual(geom=[2, 1, 9, 12, 2]) == ARG  # an image has no axis-0 neighbour
    assert pds_slab_dual(w_hi=wh, depth=0) == ARG  # kernel C reads one plane ahead
    assert pds_slab_dual(geom=[2, 6, 9, 12, 2], w_hi=wh, depth=1) == ARG  # axis 0 not differentiated: no ghost
    assert pds_slab_dual(depth=-1) == ARG
    assert pds_slab_dual(w_hi=_ptrs("w", "z", "z_out")["z_out"], depth=1) == ARG


def _pgd_base(**kw):
    a = dict(dtype=0, stack=2, y_images=1, n0=40, n1=72, nt0=3, off0=[-1, 0, 1], coef0=[0.25, 0.5, 0.25], nt1=3,
             off1=[-1, 0, 1], coef1=[0.25, 0.5, 0.25], prox=1)
    a.update(kw)
    return a


def _pgd_head(a):
    return [a["dtype"], a["stack"], a["y_images"], a["n0"], a["n1"], a["nt0"], i32_array(a["off0"]),
            f64_array(a["coef0"]), a["nt1"], i32_array(a["off1"]), f64_array(a["coef1"]), 1.0, 1.0, 0.01, 0.01]


def pgd_step(**kw):
    a = _pgd_base(**kw)
    p = _ptrs("x", "x_prev", "hty", "x_new")
    return lib.pxa_pgd_tv2d_step(*_pgd_head(a), 0.5, 0.1, a["prox"], 0.0, p["x"], p["x_prev"], p["hty"], p["x_new"],
                                 None, None, None)


def pgd_plan(**kw):
    a = _pgd_base(**kw)
    plan = ct.c_void_p(0x1234)
    st = lib.pxa_pgd_tv2d_plan(*_pgd_head(a), a["prox"], ct.byref(plan))
    assert plan.value is None  # a rejected plan leaves no handle
    return st


PGD_COMMON = [
    ("dtype 7", dict(dtype=7), DTYPE),
    ("reach 9", dict(off0=[9, 0, -1]), UNSUPPORTED),
    ("reach 9 on axis 1", dict(off1=[-9, 0, 1]), UNSUPPORTED),
    ("prox 3", dict(prox=3), ARG),
    ("stack % y_images", dict(stack=3, y_images=2), ARG),
    ("nt0 = 0", dict(nt0=0), ARG),
]


@pytest.mark.parametrize("entry", [pgd_step, pgd_plan], ids=lambda f: f.__name__)
@pytest.mark.parametrize("why,kw,status", PGD_COMMON, ids=[c[0] for c in PGD_COMMON])
def test_pgd_entries_reject(entry, why, kw, status):
    assert entry(**kw) == status, why


def test_pgd_plan_entries_reject_null_plan():
    a = _pgd_base()
    assert lib.pxa_pgd_tv2d_plan(*_pgd_head(a), a["prox"], None) == ARG
    p = _ptrs("x", "x_prev", "hty", "x_new", "partials", "x_ref", "rel_values", "rel_flags", "prev")
    step = (0.5, 0.1, 0.0, p["x"], p["x_prev"], p["hty"], p["x_new"], p["partials"])
    rel = (p["rel_values"], p["rel_flags"], 1, None)
    assert lib.pxa_pgd_tv2d_plan_step(None, *step, p["x_ref"], *rel) == ARG
    assert lib.pxa_pgd_tv2d_plan_step_fold(None, *step, p["x_ref"], *rel) == ARG
    assert lib.pxa_pgd_tv2d_plan_step_wfold(None, *step, *rel) == ARG
    assert lib.pxa_pgd_tv2d_plan_step_wpub(None, *step, p["prev"], *rel) == ARG
