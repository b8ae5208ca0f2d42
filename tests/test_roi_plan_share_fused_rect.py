"""CPU: the shared-interior form of the FUSED levels' rectangle launches (csrc/roi_plan.cpp:share_fused_rect_classes through
tmat_roi_plan_share_fused_rect).

The stem at the even pixels, the two stride-2 residual convolutions and the two pooling fix-ups computed `rect_live`, overlap with the
neighbour patches included, and because they read their inputs whole, the whole shared zone of both pooled outputs was copied.  With the
form they compute the exact `comp` of the pooled output (live minus the shared zone; the residual and the stem cut by their own live)
as at most four disjoint rectangles per class, and a pooled output takes from the neighbours only the HALO STRIPS: the shared pixels
that the next level's exact sets tap.  Checked here by brute force on pixel masks, without the planner's interval arithmetic.  The
helpers are those of test_roi_plan_share.py; that file also shows oracle patches equal, as uint32, on the whole shared zone, inside
which every strip lies."""
import hashlib

import numpy as np
import pytest

import test_roi_plan_share as base
from test_roi_plan_share import (DOWN_CH, FUSED, LS, NL, SHIFT, UP_CH, WS, consumers, inside, live_classes, mask_of, res_of)
from tmat_amd import _lib

POOLED = (5, 11)                # the pooled outputs of the fused levels
RESID = (4, 10)
CUT = POOLED + RESID + (LS,)    # the rectangle launches of the form: fix-ups, residuals, stem at the even pixels
COPIED = POOLED                 # tensors whose copies become strips
GEOMS = base.GEOMS + [(250, 300)]
# sha256 over the arrays of the two older exports, recorded on the parent commit (digest() below)
OLDER = {
    (320, 320): "f23077354d462fcc350d871f525ae6a8f0b08c5a05f3404648b2e5ca29544db5",
    (480, 320): "536d1650f689700e6d7af85de2e7f461520fe132f89a3c1dc7f2b80431e52291",
    (640, 640): "84a25de8ec90344f0f7cba12f45f8fdf3a22e33b3e77d27694880c84af95f6d0",
    (250, 300): "ecf5757dab8bb186eccc7fd2dee6ec1a061e89f8401017e8241e49f6961e4844",
    (100, 90): "b791146ec1a8bd9fedaeaadc80422a6f2f6bb3a66b45fe2d51eaaa7aebbbf024",
}


def digest(hh, ww):
    shr = _lib.roi_plan_share(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    rct = _lib.roi_plan_share_rect(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    h = hashlib.sha256()
    for d in (shr, rct):
        for key in sorted(d):
            v = d[key]
            h.update(key.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def plans(hh, ww):
    up, down, cst, shr = base.plans(hh, ww)
    rct = _lib.roi_plan_share_rect(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    fr = _lib.roi_plan_share_fused_rect(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    assert fr["n_classes"] == rct["n_classes"] == up["n_classes"]
    return up, down, cst, shr, rct, fr


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    return request.param + plans(*request.param)


def fills_of(table, c):
    out = [{d: np.zeros((res_of(l), res_of(l)), bool) for d in range(3)} for l in range(NL)]
    for l, cl, d, y0, x0, rh, rw in table:
        if cl != c:
            continue
        m = mask_of((y0, x0, rh, rw), res_of(l))
        assert not any((m & s).any() for s in out[l].values()), f"class {c} layer {l}: copied rectangles overlap"
        out[l][int(d)] |= m
    return out


def class_masks(cst, shr, rct, fr, c):
    """per layer: the exact comp in force, the launched rectangles' union, the constant fill, the copies in force per direction, the
    whole-zone copies the strips stand in for"""
    comp, launched, fill = [], [], []
    old, rect, strips = fills_of(shr["fills"], c), fills_of(rct["fills"], c), fills_of(fr["fills"], c)
    copies = []
    for l in range(NL):
        R = res_of(l)
        comp.append(np.outer(fr["comp"][l, c, 0, :R], fr["comp"][l, c, 1, :R]).astype(bool))
        cover = np.zeros((R, R), int)
        for i in range(int(fr["n_rects"][l, c])):
            y0, x0, rh, rw = (int(v) for v in fr["rects"][l, c, i])
            assert rh > 0 and rw > 0, f"class {c} layer {l}: an empty rectangle in the table"
            cover[y0:y0 + rh, x0:x0 + rw] += 1
        assert cover.max(initial=0) <= 1, f"class {c} layer {l}: the rectangles of a class overlap"
        launched.append(cover > 0)
        f = np.zeros((R, R), bool)
        for i in range(4):
            f |= mask_of(cst["fill"][l, c, i], R)
        fill.append(f)
        src = strips[l] if fr["fill_on"][l] else old[l]
        copies.append({d: src[d] | rect[l][d] for d in range(3)})
        if not fr["fill_on"][l]:
            assert not any(s.any() for s in strips[l].values()), f"class {c} layer {l}: strips of a layer that keeps its whole zone"
    return comp, launched, fill, copies, old


def test_masks_by_brute_force(planned):
    hh, ww, up, down, cst, shr, rct, fr = planned
    assert fr["any"] and fr["levels"] == 3 and [l for l in range(NL) if fr["fill_on"][l]] == list(COPIED)
    assert 1 <= fr["max_segs"] <= 4 * up["n_classes"]
    classes = live_classes(up)
    masks = {c: class_masks(cst, shr, rct, fr, c) for c in classes}
    four = cut = False
    for c in classes:
        comp, launched, fill, copies, old = masks[c]
        live = [mask_of(cst["live"][l, c], res_of(l)) for l in range(NL)]
        rect_live = [mask_of(cst["rect_live"][l, c], res_of(l)) for l in range(NL)]
        old_comp = [np.outer(shr["comp"][l, c, 0, :res_of(l)], shr["comp"][l, c, 1, :res_of(l)]).astype(bool) for l in range(NL)]
        for l in range(NL):
            held = copies[l][0] | copies[l][1] | copies[l][2]
            assert inside(launched[l], rect_live[l]), f"class {c} layer {l}: a rectangle leaves rect_live"
            assert inside(comp[l], live[l]), f"class {c} layer {l}: comp inside live"
            assert not (held & comp[l]).any() and not (held & fill[l]).any(), f"class {c} layer {l}: copied, computed and constant are disjoint"
            if l % 6 in (4, 5) or l >= LS:          # the rectangle launches (the fused layers run tiles)
                assert inside(comp[l], launched[l]), f"class {c} layer {l}: a comp pixel no rectangle holds"
            if l not in CUT:
                # every other layer: what the older export gives
                assert fr["n_rects"][l, c] == rct["n_rects"][l, c] and np.array_equal(fr["rects"][l, c], rct["rects"][l, c]), \
                    f"class {c} layer {l}: a layer outside the form keeps its rectangles"
                continue
            four |= int(fr["n_rects"][l, c]) == 4
            cut |= not np.array_equal(launched[l], rect_live[l])
            if l in POOLED:
                assert np.array_equal(comp[l], old_comp[l]), f"class {c} layer {l}: the pooled output keeps its comp"
                assert np.array_equal(launched[l], comp[l]) or np.array_equal(launched[l], rect_live[l]), \
                    f"class {c} layer {l}: the fix-up computes single pixels (or the class stays out of the form)"
            elif not np.array_equal(launched[l], rect_live[l]):
                for i in range(int(fr["n_rects"][l, c])):
                    y0, x0, rh, rw = (int(v) for v in fr["rects"][l, c, i])
                    assert x0 % 4 == 0 and rw % 4 == 0, f"class {c} layer {l}: columns {x0} + {rw}"
                    assert comp[l][y0].any() and comp[l][y0 + rh - 1].any(), f"class {c} layer {l}: rows are not rounded"
            # the strips lie inside the zone the older form copies whole, direction by direction
            if l in COPIED:
                for d in range(3):
                    assert inside(copies[l][d], old[l][d]), f"class {c} layer {l} direction {d}: a strip outside the old shared zone"
        # the invariant: every tap of every computed pixel lies in the producer's computed set, its constant fill or the copies in force
        for prod, cons, taps in consumers():
            t = taps(comp[cons])
            have = comp[prod] | fill[prod] | copies[prod][0] | copies[prod][1] | copies[prod][2]
            assert inside(t, have), f"class {c}: a tap of layer {cons}'s comp outside comp, fill and copies of layer {prod}"
    assert four, "some class launches four rectangles"
    assert cut, "some rectangle launch is smaller than rect_live"
    # every neighbour pair that occurs: a source pixel is one its patch computed itself, and no destination of that patch
    nbr = shr["neighbours"]
    pairs = set()
    n_copies = 0
    for t in range(up["tiles_per_img"]):
        c = int(up["tile_class"][t])
        if c not in masks:
            continue
        for l in COPIED:
            S = res_of(l) // 2
            for d, (sy, sx) in SHIFT.items():
                if (l, c, d, int(nbr[t, d])) in pairs:
                    continue
                pairs.add((l, c, d, int(nbr[t, d])))
                m = masks[c][3][l][d]
                if not m.any():
                    continue
                n_copies += 1
                assert nbr[t, d] >= 0, f"tile {t} (class {c}) copies from a neighbour it does not have (direction {d})"
                cs = int(up["tile_class"][nbr[t, d]])
                assert cs in masks, f"tile {t}: the neighbour's class computes nothing"
                src = np.zeros_like(m)
                ys, xs = np.nonzero(m)
                assert (ys - sy * S >= 0).all() and (xs - sx * S >= 0).all()
                src[ys - sy * S, xs - sx * S] = True
                assert inside(src, masks[cs][0][l]), f"tile {t} class {c} layer {l} direction {d}: a source pixel its patch (class {cs}) does not compute"
                dst = masks[cs][3][l]
                assert not (src & (dst[0] | dst[1] | dst[2])).any(), f"tile {t} class {c} layer {l} direction {d}: the launch reads what it writes"
    assert n_copies > 0


def test_the_launcher_takes_the_strips(planned):
    """the strips of every pooled output through the share-fill launcher's own host-side checks, on the patches of one image"""
    hh, ww, up, down, cst, shr, rct, fr = planned
    nbr = np.full((up["tiles_per_img"], 3), -1, np.int32)
    cnt, cls, rank = up["class_count"], up["tile_class"], up["tile_rank"]
    base_ = np.concatenate([[0], np.cumsum(cnt)])
    pos = lambda t: int(base_[cls[t]] + rank[t])
    for t in range(up["tiles_per_img"]):
        for d in range(3):
            if shr["neighbours"][t, d] >= 0:
                nbr[pos(t), d] = pos(int(shr["neighbours"][t, d]))
    for l in COPIED:
        items = [(int(base_[cl]), int(cnt[cl]), d, y0, x0, rh, rw) for ll, cl, d, y0, x0, rh, rw in fr["fills"] if ll == l]
        assert items
        assert _lib.debug_share_fill_check(up["tiles_per_img"], res_of(l), DOWN_CH[l // 6 + 1], nbr, items) is None


def test_the_older_exports_keep_their_values():
    for (hh, ww), want in OLDER.items():
        assert digest(hh, ww) == want, f"{hh} x {ww}: tmat_roi_plan_share or tmat_roi_plan_share_rect changed"


def test_the_form_is_not_vacuous():
    """640 x 640: the residuals, the stem and the fix-ups plan strictly fewer pixels than rect_live, and the strips are fewer pixels than
    the whole zones.  The printed ratios are the prediction the per-launch traces are held against."""
    cst = _lib.roi_plan_const(640, 640)
    fr = _lib.roi_plan_share_fused_rect(640, 640)
    for l in range(NL):
        assert fr["px"][l] <= fr["px_live"][l] and fr["mac"][l] <= cst["mac_live"][l] and fr["bytes"][l] <= cst["bytes_live"][l]
        if fr["px_live"][l] > 0:
            print(f"  640 x 640 layer {l}: planned / live pixels = {fr['px'][l] / fr['px_live'][l]:.4f}")
    for l in CUT:
        assert fr["px"][l] < fr["px_live"][l]
    for l in RESID:
        assert fr["mac"][l] < cst["mac_live"][l]
    for l in COPIED:
        print(f"  640 x 640 layer {l}: copied pixels per image {fr['copy_old'][l]:.0f} -> {fr['copy_new'][l]:.0f}"
              f" ({fr['copy_new'][l] / fr['copy_old'][l]:.4f})")
        assert 0 < fr["copy_new"][l] < fr["copy_old"][l]
    print(f"  longest segment table: {fr['max_segs']} (+ 1 for the constant patches), {len(fr['fills'])} strips, {fr['n_classes']} classes")
    assert fr["max_segs"] + 1 <= 64


def test_no_neighbour_no_share():
    """100 x 90: one patch per orientation -- the tables are the constant-ring form's"""
    cst = _lib.roi_plan_const(100, 90)
    fr = _lib.roi_plan_share_fused_rect(100, 90)
    assert not fr["any"] and fr["levels"] == 0 and len(fr["fills"]) == 0 and not fr["fill_on"].any()
    for l in range(NL):
        for c in range(fr["n_classes"]):
            q = cst["rect_live"][l, c]
            if q[2] > 0 and q[3] > 0:
                assert fr["n_rects"][l, c] == 1 and np.array_equal(fr["rects"][l, c, 0], q)
            else:
                assert fr["n_rects"][l, c] == 0
        assert fr["mac"][l] == cst["mac_live"][l] and fr["bytes"][l] == cst["bytes_live"][l]
