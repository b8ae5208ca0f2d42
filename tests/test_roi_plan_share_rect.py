"""CPU: the shared-interior form of the down path's rectangle launches (csrc/roi_plan.cpp:share_rect_keys / share_rect_classes through
tmat_roi_plan_share_rect).

The unfused 40 x 40 level computed `rect_live`, one rectangle per class, overlap with the neighbour patches included.  With the form a
patch copies the shared zone of the bottleneck tensor from its right, lower and diagonal neighbours (`fills`) and computes `comp`:
live minus that zone for the bottleneck tensor, and backwards from there through the taps for the level's other five layers, whose
halo pixels join comp (no other tensor is copied).  Per axis comp is live minus one interval, so a class launches at most four
disjoint rectangles (`rects`: rows exact, the columns of the depthwise, pointwise and residual layers rounded to multiples of 4 inside
rect_live).  Checked here by brute force on pixel masks, without the planner's interval arithmetic, and against the oracle: overlapping
patches cut from one frame are equal, as uint32, on every rectangle the plan copies.  The helpers are those of test_roi_plan_share.py."""
import numpy as np
import pytest

import test_roi_plan_share as base
from test_roi_plan_share import (DOWN_CH, FUSED, LS, NL, SHIFT, UP_CH, WS, brute_ring, consumers, inside, live_classes, mask_of, res_of)
from tmat_amd import _lib

LEVEL = 2                       # the unfused level: layers 12 .. 17
LAYERS = tuple(range(6 * LEVEL, 6 * LEVEL + 6))
BOTTLENECK = 6 * LEVEL + 5


def plans(hh, ww):
    up, down, cst, shr = base.plans(hh, ww)
    rct = _lib.roi_plan_share_rect(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    assert rct["n_classes"] == up["n_classes"]
    return up, down, cst, shr, rct


# (250 x 300, a 2 x 2 grid: there the residual under the add is constant where the pooled pixel is not, so its comp is cut by its own live)
@pytest.fixture(scope="module", params=base.GEOMS + [(250, 300)], ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    return request.param + plans(*request.param)


def class_masks(up, cst, shr, rct, c):
    """per layer: the exact comp, the launched rectangles' union, constant fill, share fill (the fused levels' and the new one) per direction"""
    comp, fill, sfill = base.class_masks(up, cst, shr, c)
    launched = []
    for l in range(NL):
        R = res_of(l)
        if l in LAYERS:
            comp[l] = np.outer(rct["comp"][l, c, 0, :R], rct["comp"][l, c, 1, :R]).astype(bool)
        cover = np.zeros((R, R), int)
        for i in range(int(rct["n_rects"][l, c])):
            y0, x0, rh, rw = (int(v) for v in rct["rects"][l, c, i])
            assert rh > 0 and rw > 0, f"class {c} layer {l}: an empty rectangle in the table"
            cover[y0:y0 + rh, x0:x0 + rw] += 1
        assert cover.max(initial=0) <= 1, f"class {c} layer {l}: the rectangles of a class overlap"
        launched.append(cover > 0)
    rfill = [{d: np.zeros((res_of(l), res_of(l)), bool) for d in range(3)} for l in range(NL)]
    for l, cl, d, y0, x0, rh, rw in rct["fills"]:
        if cl != c:
            continue
        m = mask_of((y0, x0, rh, rw), res_of(l))
        assert not any((m & s).any() for s in rfill[l].values()), f"class {c} layer {l}: copied rectangles overlap"
        rfill[l][int(d)] |= m
    return comp, launched, fill, sfill, rfill


def test_masks_by_brute_force(planned):
    hh, ww, up, down, cst, shr, rct = planned
    assert rct["any"] and rct["level"] == LEVEL
    assert 1 <= rct["max_segs"] <= 4 * up["n_classes"]
    ring = brute_ring()
    classes = live_classes(up)
    masks = {c: class_masks(up, cst, shr, rct, c) for c in classes}
    four = False
    for c in classes:
        comp, launched, fill, sfill, rfill = masks[c]
        live = [mask_of(cst["live"][l, c], res_of(l)) for l in range(NL)]
        rect_live = [mask_of(cst["rect_live"][l, c], res_of(l)) for l in range(NL)]
        need = [mask_of(down["needs"][l, c], res_of(l)) for l in range(NL)]
        for l in range(NL):
            held = rfill[l][0] | rfill[l][1] | rfill[l][2]
            assert inside(launched[l], rect_live[l]), f"class {c} layer {l}: a rectangle leaves rect_live"
            assert inside(comp[l], launched[l]), f"class {c} layer {l}: a comp pixel no rectangle holds"
            assert inside(comp[l], live[l]), f"class {c} layer {l}: comp inside live"
            if l not in LAYERS:
                assert np.array_equal(launched[l], rect_live[l]) and rct["n_rects"][l, c] == (1 if rect_live[l].any() else 0), \
                    f"class {c} layer {l}: a layer outside the level keeps rect_live"
                assert not held.any()
                continue
            four |= int(rct["n_rects"][l, c]) == 4
            if l != BOTTLENECK:
                assert not held.any(), f"class {c} layer {l}: only the bottleneck tensor is copied"
            assert not (held & comp[l]).any() and not (held & fill[l]).any(), f"class {c} layer {l}: copied, computed and constant are disjoint"
            assert inside(held, live[l]), f"class {c} layer {l}: a copied pixel lies outside live"
            if l % 6 < 5:           # columns in multiples of 4 (the depthwise strips, the epilogue's pixel groups); rows exact
                for i in range(int(rct["n_rects"][l, c])):
                    y0, x0, rh, rw = (int(v) for v in rct["rects"][l, c, i])
                    assert x0 % 4 == 0 and rw % 4 == 0, f"class {c} layer {l}: columns {x0} + {rw}"
                    assert comp[l][y0].any() and comp[l][y0 + rh - 1].any(), f"class {c} layer {l}: rows are not rounded"
            else:
                assert np.array_equal(launched[l], comp[l]), f"class {c}: the pooling computes single pixels"
            S = res_of(l) // 2
            ring1 = ring[l][S]
            for d, (sy, sx) in SHIFT.items():
                ys, xs = np.nonzero(rfill[l][d])
                assert (ys - sy * S >= 0).all() and (xs - sx * S >= 0).all()
                if sy:
                    assert not ring1[ys].any() and not ring1[ys - S].any(), f"class {c} layer {l} direction {d}: a row in the ring"
                if sx:
                    assert not ring1[xs].any() and not ring1[xs - S].any(), f"class {c} layer {l} direction {d}: a column in the ring"
        # the invariant: every tap of every computed pixel lies in the producer's computed set, its constant fill or a share fill
        for prod, cons, taps in consumers():
            t = taps(comp[cons])
            have = comp[prod] | fill[prod]
            for d in range(3):
                have = have | sfill[prod][d] | rfill[prod][d]
            assert inside(t, have), f"class {c}: a tap of layer {cons}'s comp outside comp, fill and share fill of layer {prod}"
        # what up block 0 reads of the bottleneck tensor: computed, constant or copied -- all of live
        got = comp[BOTTLENECK] | rfill[BOTTLENECK][0] | rfill[BOTTLENECK][1] | rfill[BOTTLENECK][2]
        assert np.array_equal(got, live[BOTTLENECK]), f"class {c}: comp and the copies make up live"
        assert inside(need[BOTTLENECK], got | fill[BOTTLENECK])
    assert four, "some class launches four rectangles"
    # every neighbour pair that occurs: a source pixel is one its patch computed itself, and no destination of that patch
    nbr = shr["neighbours"]
    pairs = set()
    copies = 0
    for t in range(up["tiles_per_img"]):
        c = int(up["tile_class"][t])
        if c not in masks:
            continue
        for d, (sy, sx) in SHIFT.items():
            if (c, d, int(nbr[t, d])) in pairs:
                continue
            pairs.add((c, d, int(nbr[t, d])))
            m = masks[c][4][BOTTLENECK][d]
            if not m.any():
                continue
            copies += 1
            assert nbr[t, d] >= 0, f"tile {t} (class {c}) copies from a neighbour it does not have (direction {d})"
            cs = int(up["tile_class"][nbr[t, d]])
            assert cs in masks, f"tile {t}: the neighbour's class computes nothing"
            S = res_of(BOTTLENECK) // 2
            src = np.zeros_like(m)
            ys, xs = np.nonzero(m)
            src[ys - sy * S, xs - sx * S] = True
            assert inside(src, masks[cs][0][BOTTLENECK]), f"tile {t} class {c} direction {d}: a source pixel its patch (class {cs}) does not compute"
            dst_of_src = masks[cs][4][BOTTLENECK]
            assert not (src & (dst_of_src[0] | dst_of_src[1] | dst_of_src[2])).any(), f"tile {t} class {c} direction {d}: the launch reads what it writes"
    assert copies > 0


def test_the_share_export_has_nothing_of_the_new_form(planned):
    """the new tables live in fields of their own: tmat_roi_plan_share still has no share outside the fused levels' stored tensors and
    keeps live at the unfused level.  (That the older exports keep every value is what the older test files pin, unchanged.)"""
    hh, ww, up, down, cst, shr, rct = planned
    assert set(int(f[0]) for f in shr["fills"]) <= set(base.SHARED)
    for c in live_classes(up):
        for l in range(NL):
            if l not in base.SHARED:
                assert not shr["share"][l, c].any()
        for l in LAYERS:
            R = res_of(l)
            assert np.array_equal(np.outer(shr["comp"][l, c, 0, :R], shr["comp"][l, c, 1, :R]).astype(bool), mask_of(cst["live"][l, c], R))


def test_the_form_is_not_vacuous():
    """640 x 640: the 40 x 40 pointwise layers plan strictly fewer multiply-accumulates than rect_live.  The printed ratios are the
    prediction the per-launch traces are held against."""
    cst = _lib.roi_plan_const(640, 640)
    rct = _lib.roi_plan_share_rect(640, 640)
    for l in range(NL):
        for what, new, old in (("multiply-accumulates", rct["mac_rect"][l], cst["mac_live"][l]), ("bytes", rct["bytes_rect"][l], cst["bytes_live"][l])):
            if old > 0:
                print(f"  640 x 640 layer {l}: planned / live {what} = {new / old:.4f}")
                assert new <= old
            else:
                assert new == 0
    for l in (13, 15):
        assert rct["mac_rect"][l] < cst["mac_live"][l]
    n = int(rct["n_classes"])
    print(f"  longest segment table: {rct['max_segs']} (+ 1 for the constant patches), {len(rct['fills'])} copied rectangles, {n} classes")


def test_no_neighbour_no_share():
    """100 x 90: one patch per orientation -- the tables are the constant-ring form's"""
    cst = _lib.roi_plan_const(100, 90)
    rct = _lib.roi_plan_share_rect(100, 90)
    assert not rct["any"] and rct["level"] == -1 and len(rct["fills"]) == 0 and not rct["share"].any()
    for l in range(NL):
        for c in range(rct["n_classes"]):
            q = cst["rect_live"][l, c]
            if q[2] > 0 and q[3] > 0:
                assert rct["n_rects"][l, c] == 1 and np.array_equal(rct["rects"][l, c, 0], q)
            else:
                assert rct["n_rects"][l, c] == 0
        assert rct["mac_rect"][l] == cst["mac_live"][l] and rct["bytes_rect"][l] == cst["bytes_live"][l]


def test_overlapping_patches_are_equal_where_the_plan_copies(weights):
    """the patches of test_roi_plan_share.py: four cut at stride 160 from a random 480 x 480 frame, three in a row from a 320 x 640
    frame.  The bottleneck tensor is the only tensor the form copies."""
    from oracle import unet as ou
    rs = np.random.RandomState(23)
    frame = rs.uniform(0, 1, (480, 480)).astype(np.float32)
    row = rs.uniform(0, 1, (320, 640)).astype(np.float32)
    x = np.stack([frame[y:y + WS, x0:x0 + WS] for y in (0, 160) for x0 in (0, 160)] + [row[:, x0:x0 + WS] for x0 in (0, 160, 320)])
    taps = {}
    ou.forward_exact(weights, x, taps=taps)
    pairs = [(0, 0, 1), (0, 1, 2), (0, 2, 3), (1, 1, 3), (2, 0, 3), (4, 0, 5), (5, 0, 6)]      # (destination, direction, source)
    rct = _lib.roi_plan_share_rect(320, 320, WS, UP_CH, DOWN_CH, FUSED)
    assert len(rct["fills"]) > 0 and set(int(f[0]) for f in rct["fills"]) == {BOTTLENECK}
    R = res_of(BOTTLENECK)
    S = R // 2
    t = taps["down2"].view(np.uint32)
    assert t.shape[1:3] == (R, R)
    checked = 0
    for dst, d, src in pairs:
        sy, sx = SHIFT[d]
        eq = np.zeros((R, R), bool)
        eq[sy * S:, sx * S:] = (t[dst][sy * S:, sx * S:] == t[src][:R - sy * S, :R - sx * S]).all(axis=-1)
        for l, cl, dd, y0, x0, rh, rw in rct["fills"]:
            if dd == d:
                # rows (columns) of an unshifted axis see the same borders in both patches: every rectangle of the direction must hold
                assert eq[mask_of((y0, x0, rh, rw), R)].all(), f"patch {dst} direction {d}: the copied rectangle {(y0, x0, rh, rw)} differs"
                checked += 1
    assert checked > 0
