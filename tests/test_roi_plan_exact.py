"""CPU: the exact rectangles of the UNet up path's region plan (csrc/roi_plan.cpp through tmat_roi_plan_exact).

The tight plan (tests/test_roi_plan_tight.py) gives every layer its own need with the columns rounded outwards once, because the
row-uniform prologue and epilogue of the convolution kernel wanted 8 (or 4) consecutive pixels in one image row.  The kernel's per-lane
prologue and row-split epilogue take any first column and any width, so the exact plan -- the default -- launches the need itself: in every layer but the final
convolution the rectangle is the bounding box of the pixels the blend depends on, rows and columns.  Checked here: brute-force
need ⊆ exact ⊆ tight in every layer and class and equality with the need's bounding box (the need from tests/helpers/roi_brute.py:
blend_kernel's gathers and mask dilation, nothing of the planner), the final layer, classes and patch order equal to the nested plan's,
the multiply-accumulate counts, caps on the share that the tight plan fails, and that the segments of a pass have the odd first columns,
odd widths and pixel counts that reach the kernel's row-split and per-lane paths (tests/test_gpu_roi_exact.py runs them).
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:68-79, 136-217 (pad, tile, blend, crop)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import roi_brute as rb  # noqa: E402

from tmat_amd import _lib  # noqa: E402

WS = 320
CHANNELS = (512, 512, 256, 128, 64)
N_UP = len(CHANNELS) - 1
L = 3 * N_UP + 1
# the geometries of tests/test_roi_plan_tight.py
GEOMS = [(640, 640), (320, 320), (157, 188), (100, 90), (512, 512)]


def res_of(layer):
    return rb.layer_res(layer, WS, N_UP)


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    hh, ww = request.param
    gm = rb.geom(hh, ww, WS)
    nested, tight, exact = (f(hh, ww, WS, CHANNELS) for f in (_lib.roi_plan, _lib.roi_plan_tight, _lib.roi_plan_exact))
    assert exact["tiles_per_img"] == gm["tiles"]
    assert 1 <= exact["n_classes"] <= 16, "these geometries have few classes: no fall-back"
    read = rb.blend_reads(gm)
    needs = []
    for c in range(exact["n_classes"]):
        tiles = np.flatnonzero(exact["tile_class"] == c)
        assert tiles.size == exact["class_count"][c]
        needs.append(rb.layer_needs(read[tiles].any(axis=0), N_UP))
    return gm, nested, tight, exact, needs


def test_classes_and_patch_order_are_the_nested_plans(planned):
    _, nested, _, exact, _ = planned
    assert exact["n_classes"] == nested["n_classes"]
    for key in ("tile_class", "tile_rank", "class_count", "mac_full"):
        assert np.array_equal(exact[key], nested[key]), key
    assert not exact["rects"][:, exact["n_classes"]:].any(), "rectangles of classes that do not exist"


def test_need_inside_exact_inside_tight(planned):
    _, _, tight, exact, needs = planned
    for c in range(exact["n_classes"]):
        for l in range(L):
            E, T = rb.rect_mask(exact["rects"][l, c], res_of(l)), rb.rect_mask(tight["rects"][l, c], res_of(l))
            assert not (needs[c][l] & ~E).any(), f"class {c}, layer {l}: a needed pixel outside the exact rectangle"
            assert not (E & ~T).any(), f"class {c}, layer {l}: the exact rectangle leaves the tight one"


def test_exact_is_the_bounding_box_of_the_need(planned):
    """rows AND columns, in every layer in front of the final convolution"""
    _, _, _, exact, needs = planned
    for c in range(exact["n_classes"]):
        for l in range(3 * N_UP):
            y0, x0, rh, rw = (int(v) for v in exact["rects"][l, c])
            ys, xs = np.flatnonzero(needs[c][l].any(axis=1)), np.flatnonzero(needs[c][l].any(axis=0))
            if ys.size == 0:
                assert rh == 0 or rw == 0, (l, c)
                continue
            assert (y0, y0 + rh) == (ys[0], ys[-1] + 1), (l, c, "rows", (y0, rh), (ys[0], ys[-1]))
            assert (x0, x0 + rw) == (xs[0], xs[-1] + 1), (l, c, "columns", (x0, rw), (xs[0], xs[-1]))


def test_final_layer_is_the_nested_plans(planned):
    """whole 8 x 16 blocks of final_kernel, as before"""
    _, nested, _, exact, _ = planned
    assert np.array_equal(exact["rects"][3 * N_UP], nested["rects"][3 * N_UP])
    assert exact["mac_planned"][3 * N_UP] == nested["mac_planned"][3 * N_UP]


def test_macs_match_the_rectangles(planned):
    gm, _, tight, exact, _ = planned
    per_px = []
    for j in range(N_UP):
        per_px += [(16 if j else 9) * CHANNELS[j] * CHANNELS[j + 1], CHANNELS[j] * CHANNELS[j + 1], 9 * CHANNELS[j + 1] ** 2]
    per_px.append(16 * CHANNELS[N_UP])
    for l, m in enumerate(per_px):
        want = sum(int(exact["class_count"][c]) * int(exact["rects"][l, c, 2]) * int(exact["rects"][l, c, 3]) for c in range(exact["n_classes"])) * m
        assert exact["mac_planned"][l] == want
        assert exact["mac_full"][l] == gm["tiles"] * res_of(l) ** 2 * m
    assert (exact["mac_planned"] <= tight["mac_planned"]).all()


@pytest.mark.parametrize("hh, ww, cap", [(640, 640, 0.70), (320, 320, 0.53)])
def test_share_is_capped(hh, ww, cap):
    """the planner gives 0.6804 at 640 x 640 and 0.5020 at 320 x 320 (the walk without the sub-pixel layers' parity, which the caps were
    set for: 0.6918 and 0.5188); the tight plan's 0.7146 and 0.5519 fail the caps"""
    plan, tight = _lib.roi_plan_exact(hh, ww, WS, CHANNELS), _lib.roi_plan_tight(hh, ww, WS, CHANNELS)
    frac = plan["mac_planned"].sum() / plan["mac_full"].sum()
    print(f"exact / full-frame multiply-accumulates of the up path at {hh} x {ww}: {frac:.4f}")
    for l in range(L):
        print(f"  layer {l:2d}: exact {plan['mac_planned'][l] / plan['mac_full'][l]:.4f}  tight {tight['mac_planned'][l] / plan['mac_full'][l]:.4f}")
    assert frac <= cap
    assert tight["mac_planned"].sum() / tight["mac_full"].sum() > cap


def pass_segments(hh, ww, k):
    """the segments of a k-image pass: one per class and layer in front of the final convolution (the patches k base[c] .. of the
    class-major order, the class's rectangle), as (patches, y0, x0, rows, columns)"""
    plan = _lib.roi_plan_exact(hh, ww, WS, CHANNELS)
    segs = []
    for l in range(3 * N_UP):
        for c in range(plan["n_classes"]):
            y0, x0, rh, rw = (int(v) for v in plan["rects"][l, c])
            if rh > 0 and rw > 0 and plan["class_count"][c] > 0:
                assert rw >= 2, "launch_conv takes rectangles of two columns at least"
                segs.append((k * int(plan["class_count"][c]), y0, x0, rh, rw))
    return segs


@pytest.mark.parametrize("hh, ww", [(640, 640), (320, 320)])
def test_a_pass_reaches_the_row_split_paths(hh, ww):
    """the segments of a 2-image pass include an odd first column, a width that is no multiple of 4 and a width of 8 or more off the multiples of 8.
    (A pixel count np rh rw that is no multiple of 8 cannot occur at these two sizes: every class holds 8 k tiles -- the eight
    orientations -- so np is a multiple of 16 whatever the rectangle; test_a_pass_has_a_pixel_count_off_the_multiples_of_8 finds one in
    the 157 x 188 case that tests/test_gpu_roi_exact.py runs one image per pass.)"""
    segs = pass_segments(hh, ww, 2)
    assert any(x0 % 2 == 1 for _, _, x0, _, _ in segs), "no odd first column"
    assert any(rw % 4 != 0 for *_, rw in segs), "no width off the multiples of 4"
    assert any(rw >= 8 and rw % 8 != 0 for *_, rw in segs), "no width of 8 or more off the multiples of 8"
    assert all(np_ % 16 == 0 for np_, *_ in segs)


def test_a_pass_has_a_pixel_count_off_the_multiples_of_8():
    """157 x 188, one image per pass (a case of tests/test_gpu_roi_exact.py): classes of 4 patches, odd rectangles -- the group of 8 pixels
    that contains M is cut per lane"""
    segs = pass_segments(157, 188, 1)
    assert any((np_ * rh * rw) % 8 != 0 and rw >= 8 for np_, _, _, rh, rw in segs), "every segment's pixel count is a multiple of 8"


def test_too_many_classes_falls_back_to_everything():
    plan = _lib.roi_plan_exact(640, 640, WS, CHANNELS, max_classes=4)
    assert plan["n_classes"] == 0
    assert (plan["mac_planned"] == plan["mac_full"]).all()
    assert not plan["rects"].any()
