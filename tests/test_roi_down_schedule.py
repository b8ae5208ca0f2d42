"""CPU: what a down pass launches under each form of the down path (csrc/roi_plan.h:RoiDownForm through tmat_roi_down_schedule).

The launches read ONE schedule: per layer a segment table, the strips a stored tensor takes from the constant patches and the items it
takes from its neighbours.  The planner tests pin every table of every form on its own (test_roi_plan_*.py); how the tables are put
together used to show only in the GPU parity tests.  Here the schedule is composed a second time, in Python, from the older exports by
the documented rule, and compared item by item:
  rectangles   region: roi_plan_down's rects; const and share: roi_plan_const's rect_live; share_rect: roi_plan_share_rect's rects;
               share_fused_rect: roi_plan_share_fused_rect's -- classes in order at first patch k class_base, k class_count patches,
               classes without patches and empty rectangles left out, then from const upwards one whole-patch segment for the k
               constant patches behind them
  stem layer   18 (its own) under share_fused_rect where the plan has that form, else 4 (block 0's residual)
  copies       const upwards: roi_plan_const's fill strips; share upwards: roi_plan_share's fills of the layer, the fused-rect fills in
               their place where fill_on[layer]; under both rect forms the items of roi_plan_share_rect's fills too (the bottleneck)
A form the plan does not have runs as the highest one below it that it has."""
import functools

import numpy as np
import pytest

from test_gpu_roi_share_fused_rect import table_total
from tmat_amd import _lib

GEOMS = [(320, 320), (480, 320), (100, 90), (250, 300)]
FORMS = ["region", "const", "share", "share_rect", "share_fused_rect"]
REGION, CONST, SHARE, SHARE_RECT, SHARE_FUSED_RECT = range(1, 6)
NL, LS, WS = 22, 18, 320
MAX_SEGS = 64                   # csrc/tmat_internal.h:ROI_MAX_SEGS
RES = [(WS // 2) >> (l // 6) >> (1 if l % 6 >= 4 else 0) for l in range(18)] + [WS // 4, WS // 2, WS, WS]
# the rectangle launches of a pass with levels 0 and 1 fused, after the stem at the even pixels: residual and fix-up, the unfused level whole
LAUNCHED = [4, 5, 10, 11] + list(range(12, 18))


@functools.lru_cache(maxsize=None)
def plans(hh, ww):
    return (_lib.roi_plan(hh, ww), _lib.roi_plan_down(hh, ww), _lib.roi_plan_const(hh, ww), _lib.roi_plan_share(hh, ww),
            _lib.roi_plan_share_rect(hh, ww), _lib.roi_plan_share_fused_rect(hh, ww))


def form_that_runs(hh, ww, want):
    """the highest form not above `want` that the plan has, every form below it included"""
    up, down, cst, shr, rct, fr = plans(hh, ww)
    has = CONST
    if len(shr["fills"]):
        has = SHARE
    if has == SHARE and rct["any"] and rct["max_segs"] + 1 <= MAX_SEGS:
        has = SHARE_RECT
    if has == SHARE_RECT and fr["any"] and fr["max_segs"] + 1 <= MAX_SEGS:
        has = SHARE_FUSED_RECT
    return min(has, want)


def rects_of(hh, ww, form, l, c):
    up, down, cst, shr, rct, fr = plans(hh, ww)
    if form >= SHARE_RECT:
        p = fr if form == SHARE_FUSED_RECT else rct
        return [tuple(q) for q in p["rects"][l, c, :p["n_rects"][l, c]]]
    q = (down["rects"] if form == REGION else cst["rect_live"])[l, c]
    return [tuple(q)] if q[2] > 0 and q[3] > 0 else []


def composed(hh, ww, form, k):
    """(segs per layer, stem layer, const fills, copies) by the rule of the module docstring"""
    up, down, cst, shr, rct, fr = plans(hh, ww)
    cnt = up["class_count"]
    base = np.concatenate([[0], np.cumsum(cnt)])
    live = [c for c in range(up["n_classes"]) if cnt[c] > 0]
    segs = []
    for l in range(NL):
        t = [(k * base[c], k * cnt[c]) + q for c in live for q in rects_of(hh, ww, form, l, c)]
        if form >= CONST:
            t.append((k * up["tiles_per_img"], k, 0, 0, RES[l], RES[l]))
        segs.append(np.array(t, np.int32).reshape(-1, 6))
    stem = LS if form == SHARE_FUSED_RECT else 4
    fills, copies = [], []
    for l in range(NL):
        if form >= CONST:
            fills += [(l, k * base[c], k * cnt[c]) + tuple(q) for c in live for q in cst["fill"][l, c] if q[2] > 0 and q[3] > 0]
        if form >= SHARE:
            strips = form == SHARE_FUSED_RECT and fr["fill_on"][l]
            items = [f for f in (fr if strips else shr)["fills"] if f[0] == l]
            if form >= SHARE_RECT:
                items += [f for f in rct["fills"] if f[0] == l]
            copies += [(l, k * base[f[1]], k * cnt[f[1]]) + tuple(f[2:]) for f in items]
    return segs, stem, np.array(fills, np.int32).reshape(-1, 7), np.array(copies, np.int32).reshape(-1, 8)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hh, ww", GEOMS, ids=lambda v: str(v))
def test_schedule_is_the_older_exports_composed_by_the_rule(hh, ww, form, k):
    up, down, cst, shr, rct, fr = plans(hh, ww)
    want = FORMS.index(form) + 1
    runs = form_that_runs(hh, ww, want)
    got = _lib.roi_down_schedule(hh, ww, form, k)
    assert got["form"] == runs
    segs, stem, fills, copies = composed(hh, ww, runs, k)
    assert got["stem_layer"] == stem
    assert got["stem_layer"] == (LS if want == SHARE_FUSED_RECT and fr["any"] else 4)
    assert len(got["segs"]) == NL
    for l in range(NL):
        assert np.array_equal(got["segs"][l], segs[l]), f"segments of layer {l}"
    assert np.array_equal(got["const_fills"], fills)
    assert np.array_equal(got["copies"], copies)
    if runs >= SHARE:
        assert len(copies) > 0
    # the longest table and all tables of the pass's rectangle launches added up, as the GPU tests read them off a handle
    if want >= SHARE_RECT:
        plan = fr if want == SHARE_FUSED_RECT else rct
        assert got["max_segs"] == plan["max_segs"] + 1
        assert got["seg_total"] == table_total(plan, hh, ww, LS if want == SHARE_FUSED_RECT else 4)
    else:       # one rectangle per class: the same sums over a table of 0 / 1 counts
        rects = down["rects"] if want == REGION else cst["rect_live"]
        one = dict(n_classes=up["n_classes"], n_rects=((rects[..., 2] > 0) & (rects[..., 3] > 0)).astype(np.int32))
        extra = 1 if want >= CONST else 0       # table_total counts the constant patches' segment in each of its 11 tables
        assert got["seg_total"] == table_total(one, hh, ww, 4) - (1 - extra) * (len(LAUNCHED) + 1)
        assert got["max_segs"] == max(sum(int(one["n_rects"][l, c]) for c in range(up["n_classes"]) if up["class_count"][c] > 0)
                                      for l in LAUNCHED) + extra


@pytest.mark.parametrize("k", [1, 3])
def test_without_a_neighbour_the_sharing_forms_are_the_constant_ring_form(k):
    """100 x 90: one patch per orientation"""
    ref = _lib.roi_down_schedule(100, 90, "const", k)
    assert ref["form"] == CONST and len(ref["copies"]) == 0 and len(ref["const_fills"]) > 0
    for form in FORMS[2:]:
        got = _lib.roi_down_schedule(100, 90, form, k)
        assert {key: got[key] for key in ("form", "stem_layer", "max_segs", "seg_total")} == \
               {key: ref[key] for key in ("form", "stem_layer", "max_segs", "seg_total")}
        assert all(np.array_equal(a, b) for a, b in zip(got["segs"], ref["segs"]))
        assert np.array_equal(got["const_fills"], ref["const_fills"]) and np.array_equal(got["copies"], ref["copies"])


def test_the_forms_differ_where_there_are_neighbours():
    """320 x 320, a 3 x 3 grid: every form runs as itself, and each changes what is launched or copied"""
    s = [_lib.roi_down_schedule(320, 320, form, 3) for form in FORMS]
    assert [x["form"] for x in s] == [REGION, CONST, SHARE, SHARE_RECT, SHARE_FUSED_RECT]
    assert len(s[0]["const_fills"]) == 0 and len(s[1]["const_fills"]) > 0 and len(s[1]["copies"]) == 0
    assert 0 < len(s[2]["copies"]) < len(s[3]["copies"])
    assert s[2]["seg_total"] < s[3]["seg_total"] < s[4]["seg_total"]
    assert s[4]["stem_layer"] == LS and all(x["stem_layer"] == 4 for x in s[:4])


def test_refusals():
    with pytest.raises(RuntimeError):
        _lib.roi_down_schedule(320, 320, "full", 1)
    with pytest.raises(RuntimeError):
        _lib.roi_down_schedule(320, 320, 6, 1)
    with pytest.raises(RuntimeError):
        _lib.roi_down_schedule(320, 320, "share", 0)
