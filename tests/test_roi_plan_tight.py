"""CPU: the tight rectangles of the UNet up path's region plan (csrc/roi_plan.cpp through tmat_roi_plan_tight).

tmat_roi_plan's rectangles are NESTED: a producer covers its consumer's rounded rectangle plus the taps and rounds its columns again,
so the columns drift outwards layer after layer (tests/test_roi_plan.py pins that plan; it is what TMAT_ROI_TIGHT=0 launches).  The
tight plan, the default, gives every layer its own need -- the exact dependency closure of what the blend reads -- with the columns
rounded once.  A pixel of a rectangle outside the need may then see operands nobody wrote; nothing needed depends on it.  Checked
here: the form the kernels' row-uniform paths rely on, brute-force need ⊆ tight ⊆ nested in every layer and class (the need from
tests/helpers/roi_brute.py: blend_kernel's gathers and mask dilation, nothing of the planner), the final layer, classes and patch
order equal to the nested plan's, the multiply-accumulate counts, and caps on the share that a planner returning the nested plan fails.
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
# the geometries of tests/test_roi_plan.py: the bench geometry, one patch wide, the non-square 157 x 188, smaller than a patch, 512 x 512
GEOMS = [(640, 640), (320, 320), (157, 188), (100, 90), (512, 512)]


def res_of(layer):
    return rb.layer_res(layer, WS, N_UP)


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    hh, ww = request.param
    gm = rb.geom(hh, ww, WS)
    nested, tight = _lib.roi_plan(hh, ww, WS, CHANNELS), _lib.roi_plan_tight(hh, ww, WS, CHANNELS)
    assert tight["tiles_per_img"] == gm["tiles"]
    assert 1 <= tight["n_classes"] <= 16, "these geometries have few classes: no fall-back"
    return gm, nested, tight, rb.blend_reads(gm)


def test_classes_and_patch_order_are_the_nested_plans(planned):
    _, nested, tight, _ = planned
    assert tight["n_classes"] == nested["n_classes"]
    for key in ("tile_class", "tile_rank", "class_count", "mac_full"):
        assert np.array_equal(tight[key], nested[key]), key


def test_rectangles_have_the_form_the_kernels_take(planned):
    """inside the frame, first column a multiple of 4, width a multiple of 8 (of 4 below 64 pixels a side) or the whole row"""
    _, _, tight, _ = planned
    for c in range(tight["n_classes"]):
        for l in range(3 * N_UP):
            y0, x0, rh, rw = (int(v) for v in tight["rects"][l, c])
            R = res_of(l)
            assert 0 <= y0 and y0 + rh <= R and 0 <= x0 and x0 + rw <= R and rh >= 1 and rw >= 2, (l, c)
            assert x0 % 4 == 0 and (rw % 8 == 0 or rw == R or (R < 64 and rw % 4 == 0)), (l, c, x0, rw)
    assert not tight["rects"][:, tight["n_classes"]:].any(), "rectangles of classes that do not exist"


def test_need_inside_tight_inside_nested(planned):
    gm, nested, tight, read = planned
    for c in range(tight["n_classes"]):
        tiles = np.flatnonzero(tight["tile_class"] == c)
        assert tiles.size == tight["class_count"][c]
        need = rb.layer_needs(read[tiles].any(axis=0), N_UP)
        for l in range(L):
            T, P = rb.rect_mask(tight["rects"][l, c], res_of(l)), rb.rect_mask(nested["rects"][l, c], res_of(l))
            assert not (need[l] & ~T).any(), f"class {c}, layer {l}: a needed pixel outside the tight rectangle"
            assert not (T & ~P).any(), f"class {c}, layer {l}: the tight rectangle leaves the nested one"


def test_final_layer_is_the_nested_plans(planned):
    """whole 8 x 16 blocks of final_kernel, as before"""
    _, nested, tight, _ = planned
    assert np.array_equal(tight["rects"][3 * N_UP], nested["rects"][3 * N_UP])
    assert tight["mac_planned"][3 * N_UP] == nested["mac_planned"][3 * N_UP]


def test_macs_match_the_rectangles(planned):
    gm, _, tight, _ = planned
    per_px = []
    for j in range(N_UP):
        per_px += [(16 if j else 9) * CHANNELS[j] * CHANNELS[j + 1], CHANNELS[j] * CHANNELS[j + 1], 9 * CHANNELS[j + 1] ** 2]
    per_px.append(16 * CHANNELS[N_UP])
    for l, m in enumerate(per_px):
        want = sum(int(tight["class_count"][c]) * int(tight["rects"][l, c, 2]) * int(tight["rects"][l, c, 3]) for c in range(tight["n_classes"])) * m
        assert tight["mac_planned"][l] == want
        assert tight["mac_full"][l] == gm["tiles"] * res_of(l) ** 2 * m


def test_total_is_strictly_below_the_nested_plans(planned):
    gm, nested, tight, _ = planned
    t, n, f = tight["mac_planned"].sum(), nested["mac_planned"].sum(), tight["mac_full"].sum()
    print(f"{gm['hh']} x {gm['ww']}: tight {t / f:.4f}, nested {n / f:.4f} of the full-frame multiply-accumulates of the up path")
    assert (tight["mac_planned"] <= nested["mac_planned"]).all()
    assert t < n


@pytest.mark.parametrize("hh, ww, cap", [(640, 640, 0.72), (320, 320, 0.56)])
def test_share_is_capped(hh, ww, cap):
    """an independent replica of the exact walk with one rounding gives 0.7146 at 640 x 640 and 0.5519 at 320 x 320; the nested plan's
    0.7731 and 0.6371 fail the caps"""
    plan = _lib.roi_plan_tight(hh, ww, WS, CHANNELS)
    frac = plan["mac_planned"].sum() / plan["mac_full"].sum()
    print(f"tight / full-frame multiply-accumulates of the up path at {hh} x {ww}: {frac:.4f}")
    for l in range(L):
        print(f"  layer {l:2d}: {plan['mac_planned'][l] / plan['mac_full'][l]:.4f}")
    assert frac <= cap


def test_too_many_classes_falls_back_to_everything():
    plan = _lib.roi_plan_tight(640, 640, WS, CHANNELS, max_classes=4)
    assert plan["n_classes"] == 0
    assert (plan["mac_planned"] == plan["mac_full"]).all()
    assert sorted(plan["tile_rank"]) == list(range(plan["tiles_per_img"]))
    assert not plan["rects"].any()
