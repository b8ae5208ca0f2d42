"""GPU: the shared-interior form of the fused levels' rectangle launches (TMAT_ROI_SHARE_FUSED_RECT) computes what whole patches compute
(TMAT_ROI=0).

With the form the stem at the even pixels, the two stride-2 residual convolutions and the two pooling fix-ups take up to four disjoint
rectangles per class (tests/test_roi_plan_share_fused_rect.py), the first and the last on compact grids, and the pooled outputs of the
160 x 160 and 80 x 80 levels take from the neighbour patches only the halo strips that the next level taps.  A needed pixel that took
an operand nobody wrote or copied shows under the poison patterns (0xFF: NaN, 0x7F: large finite floats) as a NaN or a bit difference
against the full-frame run; so does a copy from the wrong patch, the frame being random.  The cases and the method are those of
tests/test_gpu_roi_share_rect.py: 320 x 320 has a 3 x 3 grid per orientation (right, lower and diagonal copies all run, and so do
four-rectangle classes), 480 x 320 a 4 x 3 grid that the transposed orientations swap, 100 x 90 one patch per orientation and no
neighbour."""
import numpy as np
import pytest

from test_gpu_roi_share import CASES, CFG, counts, make_handle, tiles_per_img
from test_gpu_roi_share_rect import RECT

pytestmark = pytest.mark.gpu

FUSED_RECT = "TMAT_ROI_SHARE_FUSED_RECT"
LS = 18                         # the stem at the even pixels in the down plan's layer numbering


def table_total(plan, hh, ww, stem_layer):
    """The segment tables of the rectangle launches of one down pass added up, the constant patches' segment included: stem at the even
    pixels, residual and fix-up of both fused levels, the six launches of the unfused level.  The form makes no table longer than the
    longest of the unfused level's (25 + 1 on a 3 x 3 grid either way), so the longest table cannot tell the forms apart; the sum can."""
    from tmat_amd import _lib
    cnt = _lib.roi_plan(hh, ww)["class_count"]
    layers = [stem_layer, 4, 5, 10, 11] + list(range(12, 18))
    return sum(sum(int(plan["n_rects"][l, c]) for c in range(plan["n_classes"]) if cnt[c] > 0) + 1 for l in layers)


@pytest.fixture(scope="module")
def full_frame(weights):
    """per case: the input and the whole-patch prediction (TMAT_ROI=0), computed once"""
    out = {}
    for hh, ww, per_pass, n in CASES:
        rs = np.random.RandomState(1400 + hh)
        x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
        h0 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, False, **{RECT: None, FUSED_RECT: None})
        try:
            full = h0.predict_smooth(x)
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_share_fused_rect_equals_full_frame(weights, full_frame, hh, ww, per_pass, n):
    from tmat_amd import _lib
    x, full = full_frame[(hh, ww)]
    plan = _lib.roi_plan_share_fused_rect(hh, ww)
    old = _lib.roi_plan_share_rect(hh, ww)
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1", **{RECT: "1", FUSED_RECT: "1"})
    try:
        held = None
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, {FUSED_RECT}=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
            k_last = n % per_pass or per_pass
            assert h1.debug_sep_tiles() == counts(_lib.roi_sep_tiles_share, hh, ww, k_last), "the fused launches still visit the share table's tiles"
            segs = h1.debug_down_segs()
            print(f"  longest segment table of the last pass: {segs} (plan: {plan['max_segs']} + 1, without the form {old['max_segs']} + 1)")
            total = h1.debug_down_seg_total()
            print(f"  all segment tables of the last pass: {total} (plan: {table_total(plan, hh, ww, LS)}, without the form {table_total(old, hh, ww, 4)})")
            assert segs == plan["max_segs"] + 1 and total == table_total(plan, hh, ww, LS)
            if tiles_per_img(hh, ww) > 8:
                assert plan["any"] and total > table_total(old, hh, ww, 4), "the fused levels' launches take several rectangles per class"
            else:
                assert not plan["any"] and segs <= plan["n_classes"] + 1 and total == table_total(old, hh, ww, 4), "no neighbour: one rectangle per class"
            if held is None:
                held = h1.debug_held_bytes()
            else:
                assert h1.debug_held_bytes() == held, "held bytes change between calls"
    finally:
        h1.close()


@pytest.mark.parametrize("form", ["TMAT_FUSED_SEP", "TMAT_FUSED_POOL", "TMAT_STEM_FUSED", "TMAT_ROI_DOWN=1", "TMAT_ROI_DOWN=2", "TMAT_ROI_CONST",
                                  "TMAT_ROI_SHARE", RECT])
def test_other_forms_at_320_by_320(weights, full_frame, form):
    """the new switch at 1 beside every other form of the down path switched off: the separate depthwise / pointwise kernels, the unfused
    pooling, the stem written to memory, either bit of TMAT_ROI_DOWN alone, the constant-ring or the shared-interior form, and the
    rectangle form of the unfused level (the new form then stays off too: strips are not enough for a level that reads whole tensors)"""
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    name, value = form.split("=") if "=" in form else (form, "0")
    share, roi_const = ("0" if name == "TMAT_ROI_SHARE" else "1"), ("0" if name == "TMAT_ROI_CONST" else "1")
    env = {RECT: "1", FUSED_RECT: "1"}
    if name not in ("TMAT_ROI_SHARE", "TMAT_ROI_CONST"):
        env[name] = value
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, share, roi_const, **env)
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            assert not np.isnan(got).any(), f"{form}, pattern {pattern:#x}: NaN"
            assert nbad == 0, f"{form}, pattern {pattern:#x}: {nbad} of {got.size} differ"
        print(f"{form}: longest segment table {h1.debug_down_segs()}")
    finally:
        h1.close()


def test_predict_smooth_keeps_its_launches_with_the_switch_unset(weights, full_frame):
    """unset or 0, beside the rectangle form of the unfused level at 1: the parent's segment counts"""
    from tmat_amd import _lib
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    old = _lib.roi_plan_share_rect(hh, ww)
    for setting in (None, "0"):
        h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1", **{RECT: "1", FUSED_RECT: setting})
        try:
            h1.debug_poison(0xFF)
            got = h1.predict_smooth(x)
            assert np.array_equal(got.view(np.uint64), full.view(np.uint64)), setting
            assert h1.debug_down_segs() == old["max_segs"] + 1 and h1.debug_down_seg_total() == table_total(old, hh, ww, 4), \
                f"{FUSED_RECT}={setting}: the tables of the older form"
        finally:
            h1.close()


def test_analyze_batch_share_fused_rect_equals_full_frame(weights):
    """the 250 x 300 source of test_gpu_roi_sep.py through the whole pipeline: rows equal with the switch unset, 0 and 1; the pipeline
    runs the form unless the switch is 0"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    imgs = np.stack([odd, odd[::-1]])
    h0 = make_handle(weights, 64, False, **{RECT: None, FUSED_RECT: None})
    try:
        rows0 = branches.analyze_batch(h0, imgs, CFG, 300.0)
    finally:
        h0.close()
    segs = {}
    for setting in (None, "0", "1"):
        h1 = make_handle(weights, 64, True, None, **{RECT: None, FUSED_RECT: setting})
        try:
            held = None
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, imgs, CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"{FUSED_RECT}={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            segs[setting] = (h1.debug_down_segs(), h1.debug_down_seg_total())
        finally:
            h1.close()
    print("(longest segment table, all tables together) per setting:", segs)
    # (the longest table is the unfused level's with and without the form: 14 + 1 on this 2 x 2 grid)
    assert segs[None] == segs["1"] and segs["1"][0] >= segs["0"][0] and segs["1"][1] > segs["0"][1], \
        "unset runs the form (several rectangles per class in the fused levels), 0 does not"
