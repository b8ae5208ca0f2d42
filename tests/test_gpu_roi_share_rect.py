"""GPU: the shared-interior form of the down path's rectangle launches (TMAT_ROI_SHARE_RECT) computes what whole patches compute
(TMAT_ROI=0).

With the form the launches of the unfused 40 x 40 level take up to four disjoint rectangles per class (tests/test_roi_plan_share_rect.py)
and the bottleneck tensor and its activated copy take their shared zone from the right, lower and diagonal neighbour patches.  A needed
pixel that took an operand nobody wrote or copied shows under the poison patterns (0xFF: NaN, 0x7F: large finite floats) as a NaN or a
bit difference against the full-frame run; so does a copy from the wrong patch, the frame being random.  The cases and the method are
those of tests/test_gpu_roi_share.py: 320 x 320 has a 3 x 3 grid per orientation (first / middle / last classes on both axes: right,
lower and diagonal copies all run, and so do four-rectangle classes), 480 x 320 a 4 x 3 grid that the transposed orientations swap,
100 x 90 one patch per orientation and no neighbour."""
import numpy as np
import pytest

from test_gpu_roi_share import CASES, CFG, counts, make_handle, tiles_per_img

pytestmark = pytest.mark.gpu

RECT = "TMAT_ROI_SHARE_RECT"


@pytest.fixture(scope="module")
def full_frame(weights):
    """per case: the input and the whole-patch prediction (TMAT_ROI=0), computed once"""
    out = {}
    for hh, ww, per_pass, n in CASES:
        rs = np.random.RandomState(900 + hh)
        x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
        h0 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, False, **{RECT: None})
        try:
            full = h0.predict_smooth(x)
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_share_rect_equals_full_frame(weights, full_frame, hh, ww, per_pass, n):
    from tmat_amd import _lib
    x, full = full_frame[(hh, ww)]
    plan = _lib.roi_plan_share_rect(hh, ww)
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1", **{RECT: "1"})
    try:
        held = None
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, {RECT}=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
            k_last = n % per_pass or per_pass
            assert h1.debug_sep_tiles() == counts(_lib.roi_sep_tiles_share, hh, ww, k_last), "the fused launches still visit the share table's tiles"
            segs = h1.debug_down_segs()
            print(f"  longest segment table of the last pass: {segs} (plan: {plan['max_segs']} + 1)")
            if tiles_per_img(hh, ww) > 8:
                assert plan["any"] and segs == plan["max_segs"] + 1 > plan["n_classes"] + 1, "the launches take several rectangles per class"
            else:
                assert not plan["any"] and segs <= plan["n_classes"] + 1, "no neighbour: one rectangle per class"
            if held is None:
                held = h1.debug_held_bytes()
            else:
                assert h1.debug_held_bytes() == held, "held bytes change between calls"
    finally:
        h1.close()


@pytest.mark.parametrize("form", ["TMAT_FUSED_SEP", "TMAT_FUSED_POOL", "TMAT_STEM_FUSED", "TMAT_ROI_DOWN=1", "TMAT_ROI_DOWN=2", "TMAT_ROI_CONST",
                                  "TMAT_ROI_SHARE"])
def test_other_forms_at_320_by_320(weights, full_frame, form):
    """the new switch at 1 beside every other form of the down path: the separate depthwise / pointwise kernels, the unfused pooling,
    the stem written to memory, either bit of TMAT_ROI_DOWN alone, and the constant-ring or the shared-interior form switched off (the
    rectangle form then stays off too)"""
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    name, value = form.split("=") if "=" in form else (form, "0")
    share, roi_const = ("0" if name == "TMAT_ROI_SHARE" else "1"), ("0" if name == "TMAT_ROI_CONST" else "1")
    env = {RECT: "1"}
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
    from tmat_amd import _lib
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    plan = _lib.roi_plan_share_rect(hh, ww)
    for setting in (None, "0"):
        h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1", **{RECT: setting})
        try:
            h1.debug_poison(0xFF)
            got = h1.predict_smooth(x)
            assert np.array_equal(got.view(np.uint64), full.view(np.uint64)), setting
            assert h1.debug_down_segs() <= plan["n_classes"] + 1, f"{RECT}={setting}: one rectangle per class"
        finally:
            h1.close()


def test_analyze_batch_share_rect_equals_full_frame(weights):
    """the 250 x 300 source of test_gpu_roi_sep.py through the whole pipeline: rows equal with the switch unset, 0 and 1; the pipeline
    runs the form unless the switch is 0"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    imgs = np.stack([odd, odd[::-1]])
    h0 = make_handle(weights, 64, False, **{RECT: None})
    try:
        rows0 = branches.analyze_batch(h0, imgs, CFG, 300.0)
    finally:
        h0.close()
    segs = {}
    for setting in (None, "0", "1"):
        h1 = make_handle(weights, 64, True, None, **{RECT: setting})
        try:
            held = None
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, imgs, CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"{RECT}={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            segs[setting] = h1.debug_down_segs()
        finally:
            h1.close()
    print("longest segment table per setting:", segs)
    assert segs[None] == segs["1"] > segs["0"], "unset runs the form (several rectangles per class), 0 does not"


def test_segment_tables_the_launcher_refuses(handle):
    """host-side checks of the longer tables: a refused table launches nothing (the two accepted ones run, on zeros)"""
    from tmat_amd import _lib
    N, S, C = 3, 20, 64
    x = np.zeros((N, S, S, C), np.float32)
    w = np.zeros((1, 1, C, 64), np.float32)
    shift = np.zeros(64, np.float32)
    out = np.zeros((N, S, S, 64), np.float32)
    ok = [(0, 2, 0, 0, 5, 8), (0, 2, 0, 12, 5, 4), (0, 2, 8, 0, 4, 8), (0, 2, 8, 12, 4, 4), (2, 1, 0, 0, S, S)]
    handle.conv2d_roi(x, w, None, shift, ok, out)
    too_long = [(0, 3, y, 4 * (i % 5), 1, 4) for y in range(13) for i in range(5)]
    assert len(too_long) == 65
    handle.conv2d_roi(x, w, None, shift, too_long[:64], out)
    for name, segs in (("a table longer than the cap", too_long),
                       ("overlapping rectangles on one patch range", [(0, 2, 0, 0, 5, 8), (0, 2, 4, 4, 5, 8)]),
                       ("a rectangle that overlaps an earlier one of its range", [(0, 2, 0, 0, 5, 8), (0, 2, 0, 12, 5, 4), (0, 2, 2, 6, 5, 4)]),
                       ("patch ranges that overlap without being equal", [(0, 2, 0, 0, 5, 8), (1, 2, 8, 0, 5, 8)]),
                       ("descending patch order", [(1, 1, 0, 0, 4, 8), (1, 1, 8, 0, 4, 8), (0, 1, 0, 0, 4, 8)])):
        with pytest.raises(_lib.TmatError):
            handle.conv2d_roi(x, w, None, shift, segs, out)
        print(f"refused: {name}")
