"""CPU: the constant-ring form of the down plan (csrc/roi_plan.cpp:walk_const_axis through tmat_roi_plan_const).

predict_img_with_smooth_windowing pads every image with one value, so a patch is image data inside the rectangle the blend reads of it
(`read`, layer 6 n_down + 3 of the down plan) and that value outside.  The planner walks `read` FORWARDS through the taps of the down
path: `nonconst` is what the image data reaches; outside it every tensor equals the tensor of an all-constant patch at the same position.
A launch then computes live = need ∩ nonconst only, and the strips `fill` are copied from the constant patch.  Checked here without the
planner's interval arithmetic, by brute force on pixel masks, and against the oracle: bits outside nonconst equal the all-constant
patch's."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
UP_CH = (512, 512, 256, 128, 64)
DOWN_CH = (64, 128, 256, 512)
N_DOWN = len(DOWN_CH) - 1
FUSED = 3
LS = 6 * N_DOWN                  # stem at the even pixels; LS + 1 the stem, LS + 2 the input window, LS + 3 what the blend reads
NL = LS + 4
GEOMS = [(320, 320), (640, 640), (100, 90), (157, 188)]
FUSED_LAYERS = (1, 3, 7, 9)


def res_of(l):
    if l >= LS:
        return (WS // 4, WS // 2, WS, WS)[l - LS]
    b, k = divmod(l, 6)
    H = (WS // 2) >> b
    return H if k < 4 else H // 2


def mask_of(r, R):
    m = np.zeros((R, R), bool)
    y0, x0, rh, rw = (int(v) for v in r)
    m[y0:y0 + rh, x0:x0 + rw] = True
    return m


def dil3(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def window_s2(m):
    """the inputs of a 3-wide stride-2 "same" window on an even side: output i reads 2 i .. 2 i + 2, clipped"""
    R = 2 * m.shape[0]
    out = np.zeros((R + 2, R + 2), bool)
    for dy in range(3):
        for dx in range(3):
            out[dy:dy + R:2, dx:dx + R:2] |= m
    return out[:R, :R]


def reached_s2(m):
    """the outputs of that window that see a pixel of m"""
    R = m.shape[0] // 2
    p = np.pad(m, ((0, 2), (0, 2)))
    out = np.zeros((R, R), bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + 2 * R:2, dx:dx + 2 * R:2]
    return out


def evens(m):
    out = np.zeros((2 * m.shape[0], 2 * m.shape[1]), bool)
    out[0::2, 0::2] = m
    return out


def inside(a, b):
    return not (a & ~b).any()


def plans(hh, ww):
    up = _lib.roi_plan(hh, ww, WS, UP_CH)
    down = _lib.roi_plan_down(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    cst = _lib.roi_plan_const(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    assert cst["n_classes"] == down["n_classes"] == up["n_classes"] >= 1
    return up, down, cst


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    return request.param + plans(*request.param)


def live_classes(up):
    return [c for c in range(up["n_classes"]) if up["rects"][0, c, 2] > 0 and up["class_count"][c] > 0]


def fill_mask(cst, l, c):
    m = np.zeros((res_of(l), res_of(l)), bool)
    for i in range(4):
        s = mask_of(cst["fill"][l, c, i], res_of(l))
        assert not (m & s).any(), "strips do not overlap"
        m |= s
    return m


def brute_nonconst(read):
    """what the image data reaches, layer by layer, on masks"""
    nc = [None] * NL
    nc[LS + 3] = nc[LS + 2] = read
    nc[LS + 1] = reached_s2(read)
    nc[LS] = nc[LS + 1][0::2, 0::2]
    x = nc[LS + 1]
    for b in range(N_DOWN):
        L = 6 * b
        nc[L] = nc[L + 1] = dil3(x)
        nc[L + 2] = nc[L + 3] = dil3(nc[L + 1])
        nc[L + 4] = x[0::2, 0::2]
        nc[L + 5] = reached_s2(nc[L + 3]) | nc[L + 4]
        x = nc[L + 5]
    return nc


def consumers():
    """(producer layer, consumer layer, the consumer's taps as a function of its mask)"""
    out = [(LS + 1, 0, dil3), (LS, 4, lambda m: m), (LS + 1, LS, evens), (LS + 2, LS + 1, window_s2)]
    for b in range(N_DOWN):
        L = 6 * b
        out += [(L, L + 1, lambda m: m), (L + 1, L + 2, dil3), (L + 2, L + 3, lambda m: m), (L + 3, L + 5, window_s2), (L + 4, L + 5, lambda m: m)]
        if b:
            out += [(L - 1, L, dil3), (L - 1, L + 4, evens)]
    return out


def test_masks_by_brute_force(planned):
    hh, ww, up, down, cst = planned
    for c in live_classes(up):
        read = mask_of(down["needs"][LS + 3, c], WS)
        nc_ref = brute_nonconst(read)
        need = [mask_of(down["needs"][l, c], res_of(l)) for l in range(NL)]
        rect = [mask_of(down["rects"][l, c], res_of(l)) for l in range(NL)]
        nc = [mask_of(cst["nonconst"][l, c], res_of(l)) for l in range(NL)]
        live = [mask_of(cst["live"][l, c], res_of(l)) for l in range(NL)]
        rlive = [mask_of(cst["rect_live"][l, c], res_of(l)) for l in range(NL)]
        fill = [fill_mask(cst, l, c) for l in range(NL)]
        for l in range(NL):
            assert inside(nc_ref[l], nc[l]), f"class {c} layer {l}: a pixel the image data reaches lies outside nonconst"
            assert np.array_equal(nc_ref[l], nc[l]), f"class {c} layer {l}: nonconst is exactly what the data reaches"
            assert inside(live[l], rlive[l]) and inside(rlive[l], rect[l]), f"class {c} layer {l}: live in rect_live in rect"
            assert live[l].any(), (c, l)
            assert not (fill[l] & nc[l]).any(), f"class {c} layer {l}: a fill pixel depends on image data"
            if cst["stored"][l]:
                assert np.array_equal(live[l], need[l] & nc[l]), f"class {c} layer {l}: live of a stored tensor"
            else:
                assert not fill[l].any(), f"class {c} layer {l}: a tensor that is never stored cannot be copied"
        for prod, cons, taps in consumers():
            t = taps(live[cons])
            assert inside(t, live[prod] | fill[prod]), f"class {c}: a tap of layer {cons}'s live outside live and fill of layer {prod}"
            if not cst["stored"][prod] and prod < LS:
                assert inside(t, live[prod]), f"class {c}: never-stored layer {prod} covers its consumer's window"
        # what up block 0 reads of the bottleneck tensor (the dependency plan's need of the last pooling)
        assert inside(need[LS - 1], live[LS - 1] | fill[LS - 1])
        assert np.array_equal(fill[LS - 1], need[LS - 1] & ~nc[LS - 1])


def test_rect_live_has_the_form_its_kernels_want(planned):
    hh, ww, up, down, cst = planned
    for c in live_classes(up):
        for b in range(N_DOWN):
            H = (WS // 2) >> b
            for k in range(4):
                y0, x0, rh, rw = (int(v) for v in cst["rect_live"][6 * b + k, c])
                if (FUSED >> b) & 1:
                    assert y0 % 16 == 0 and x0 % 16 == 0 and rh % 16 == 0 and rw % 16 == 0, (c, b, k)
                else:
                    assert x0 % 4 == 0 and rw >= 2 and (rw % 8 == 0 or rw == H or (H < 64 and rw % 4 == 0)), (c, b, k)
            for k in (0, 2):
                assert (cst["rect_live"][6 * b + k, c] == cst["rect_live"][6 * b + k + 1, c]).all()
            y0, x0, rh, rw = (int(v) for v in cst["rect_live"][6 * b + 4, c])
            assert x0 % 4 == 0 and rw >= 2 and (rw % 8 == 0 or rw == H // 2 or (H // 2 < 64 and rw % 4 == 0)), (c, b)
        assert (cst["rect_live"][LS, c] == cst["rect_live"][4, c]).all()


def test_totals_match_rect_live(planned):
    hh, ww, up, down, cst = planned
    for l in range(NL):
        area = sum(int(up["class_count"][c]) * int(cst["rect_live"][l, c, 2]) * int(cst["rect_live"][l, c, 3]) for c in range(up["n_classes"]))
        area0 = sum(int(up["class_count"][c]) * int(down["rects"][l, c, 2]) * int(down["rects"][l, c, 3]) for c in range(up["n_classes"]))
        assert cst["mac_live"][l] * area0 == down["mac_planned"][l] * area
        assert cst["bytes_live"][l] * area0 == down["bytes_planned"][l] * area
        assert cst["mac_live"][l] <= down["mac_planned"][l] and cst["bytes_live"][l] <= down["bytes_planned"][l]


@pytest.mark.parametrize("k", [1, 3])
def test_tile_table_is_the_tiles_of_rect_live_in_the_old_order(planned, k):
    hh, ww, up, down, cst = planned
    base = np.concatenate([[0], np.cumsum(up["class_count"][:up["n_classes"]])])
    for layer in FUSED_LAYERS:
        old, full = _lib.roi_sep_tiles(hh, ww, layer, k, WS, UP_CH, DOWN_CH, FUSED)
        new, full2 = _lib.roi_sep_tiles_live(hh, ww, layer, k, WS, UP_CH, DOWN_CH, FUSED)
        assert full == full2
        TW = res_of(layer) // 16
        keep = []
        for tid in old:
            pt, t = divmod(int(tid), TW * TW)
            ty, tx = divmod(t, TW)
            c = int(np.searchsorted(k * base, pt, side="right")) - 1
            y0, x0, rh, rw = (int(v) for v in cst["rect_live"][layer, c])
            if y0 <= 16 * ty < y0 + rh and x0 <= 16 * tx < x0 + rw:
                keep.append(int(tid))
        assert list(new) == keep, f"layer {layer}"


@pytest.mark.parametrize("hh, ww", [(320, 320), (640, 640)])
def test_the_form_is_not_vacuous(hh, ww):
    """every fused layer and the unfused level keep strictly less than the dependency plan"""
    up, down, cst = plans(hh, ww)
    for l in range(NL):
        if down["mac_planned"][l]:
            print(f"  {hh} x {ww} layer {l:2d}: matrix work live / planned {cst['mac_live'][l] / down['mac_planned'][l]:.4f}, "
                  f"planned / full {down['mac_planned'][l] / down['mac_full'][l]:.4f}")
        if down["bytes_planned"][l]:
            print(f"  {hh} x {ww} layer {l:2d}: bytes live / planned {cst['bytes_live'][l] / down['bytes_planned'][l]:.4f}")
    for l in FUSED_LAYERS + (13, 15, 16):
        assert cst["mac_live"][l] < down["mac_planned"][l], l
    for l in (12, 14, 17):
        assert cst["bytes_live"][l] < down["bytes_planned"][l], l
    for layer in FUSED_LAYERS:
        assert len(_lib.roi_sep_tiles_live(hh, ww, layer, 1)[0]) < len(_lib.roi_sep_tiles(hh, ww, layer, 1)[0]), layer


TAPS = (("stem", LS + 1), ("down0", 5), ("down1", 11), ("down2", 17))


def test_tensors_outside_nonconst_equal_the_constant_patch(weights):
    """all nine classes at 320 x 320, pad values 0.0 and 0.37: a patch that is the pad value outside `read` and random inside, against
    the all-constant patch -- stem and block outputs equal, as uint32, at every pixel outside nonconst"""
    from oracle import unet as ou
    up, down, cst = plans(320, 320)
    classes = live_classes(up)
    assert len(classes) == 9
    rs = np.random.RandomState(11)
    shrunk_differs = False
    seen = {}
    for pad in (0.0, 0.37):
        x = np.full((len(classes) + 1, WS, WS), pad, np.float32)
        for i, c in enumerate(classes):
            rd = mask_of(down["needs"][LS + 3, c], WS)
            x[i][rd] = rs.uniform(0.4, 1, int(rd.sum())).astype(np.float32)
        taps = {}
        ou.forward_exact(weights, x, taps=taps)
        for i, c in enumerate(classes):
            for name, l in TAPS:
                nc = mask_of(cst["nonconst"][l, c], res_of(l))
                a, k = taps[name][i].view(np.uint32), taps[name][-1].view(np.uint32)
                assert a.shape[:2] == nc.shape
                eq = (a == k).all(axis=-1)
                assert eq[~nc].all(), f"pad {pad}, class {c}, {name}: {int((~eq & ~nc).sum())} pixels outside nonconst differ from the constant patch"
                # the check can fail: with nonconst one pixel further in, the ring between the two holds pixels that differ
                y0, x0, rh, rw = (int(v) for v in cst["nonconst"][l, c])
                inner = np.zeros_like(nc)
                inner[y0 + 1:y0 + rh - 1, x0 + 1:x0 + rw - 1] = True
                shrunk_differs |= bool((~eq & nc & ~inner).any())
                seen[(tuple(int(v) for v in down["needs"][LS + 3, c]), name)] = (eq, (y0, x0, rh, rw))
    assert shrunk_differs, "nonconst moved one pixel inwards must break the equality"
    # the rows measured with the oracle when the form was proposed: upper half constant -> rows 0-78 / 0-37 / 0-17 / 0-7 of stem, down0,
    # down1, down2 equal; lower half constant -> equal from row 80 / 41 / 21 / 11.  The planner's equal zone lies inside the observed one.
    upper = {"stem": 79, "down0": 38, "down1": 18, "down2": 8}
    lower = {"stem": 80, "down0": 41, "down1": 21, "down2": 11}
    for name, _ in TAPS:
        eq, (y0, x0, rh, rw) = seen[((160, 0, 160, 320), name)]
        assert y0 <= upper[name] and eq[:upper[name]].all(), name
        eq, (y0, x0, rh, rw) = seen[((0, 0, 160, 320), name)]
        assert y0 + rh >= lower[name] and eq[lower[name]:].all(), name
