"""CPU: the region planner continued through the UNet down path (csrc/roi_plan.cpp:roi_plan_down through tmat_roi_plan_down).

The region-form up path reads only a rectangle of the bottleneck tensor; the planner walks that rectangle backwards through the down
blocks (max-pool 3 / stride 2 "same", pointwise, depthwise +-1, the stride-2 residual 1x1), the stem and the input window.  Checked here
without the planner's interval arithmetic: by brute force on pixel masks (every needed pixel inside `needs`, `needs` inside `rects`, the
rounding each kernel wants), and by running the oracle forward twice -- once on a random patch, once with every input pixel outside the
planned input window replaced -- and comparing bits inside the rectangles the plan says depend on the window only.
Reference: fl_tissue_model_tools/models.py:119-144 (stem, down blocks)."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
UP_CH = (512, 512, 256, 128, 64)
DOWN_CH = (64, 128, 256, 512)
N_DOWN = len(DOWN_CH) - 1
FUSED = 3                      # blocks 0 and 1 (160 and 80 pixels a side) on the fused separable kernel, block 2 (40) unfused
NL = 6 * N_DOWN + 4
N_UP = len(UP_CH) - 1
GEOMS = [(640, 640), (512, 512), (320, 320), (157, 188), (100, 90)]


def res_of(l):
    if l >= 6 * N_DOWN:
        return (WS // 4, WS // 2, WS, WS)[l - 6 * N_DOWN]
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
    """inputs of a 3-wide, stride-2 "same" window on an even side: output i reads 2 i .. 2 i + 2, clipped (padding lies behind only)"""
    R = 2 * m.shape[0]
    out = np.zeros((R + 2, R + 2), bool)
    for dy in range(3):
        for dx in range(3):
            out[dy:dy + R:2, dx:dx + R:2] |= m
    return out[:R, :R]


def evens(m):
    out = np.zeros((2 * m.shape[0], 2 * m.shape[1]), bool)
    out[0::2, 0::2] = m
    return out


def inside(a, b):
    return not (a & ~b).any()


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    hh, ww = request.param
    up = _lib.roi_plan(hh, ww, WS, UP_CH)
    down = _lib.roi_plan_down(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    assert down["n_classes"] == up["n_classes"] >= 1
    return up, down


def live_classes(up):
    return [c for c in range(up["n_classes"]) if up["rects"][0, c, 2] > 0 and up["class_count"][c] > 0]


def half_any(m):
    return m[0::2, 0::2] | m[0::2, 1::2] | m[1::2, 0::2] | m[1::2, 1::2]


def subpixel_sources(t1):
    """stored pixels a sub-pixel layer reads for the needed outputs t1: output (2i + py, 2j + px) sees stored
    (i + py - 1 + {0, 1}, j + px - 1 + {0, 1})"""
    R = t1.shape[0] // 2
    need = np.zeros((R, R), bool)
    for py in range(2):
        for px in range(2):
            i, j = np.nonzero(t1[py::2, px::2])
            for da in range(2):
                for db in range(2):
                    ii, jj = i + py - 1 + da, j + px - 1 + db
                    ok = (ii >= 0) & (ii < R) & (jj >= 0) & (jj < R)
                    need[ii[ok], jj[ok]] = True
    return need


def bottleneck_reads(down, c):
    """the pixels of the bottleneck tensor that the blend's rectangle of the output depends on, by brute force through the up path
    (models.py:146-166: per block a transposed 3x3 on the upsampled input, a residual 1x1, a second 3x3; then the final 3x3 on the
    upsampled last block): what the up path needs, not the rounded rectangles its kernels compute"""
    s_need = dil3(half_any(mask_of(down["needs"][6 * N_DOWN + 3, c], WS)))
    for j in range(N_UP - 1, 0, -1):
        t1_need = dil3(s_need)
        s_need = half_any(s_need) | subpixel_sources(t1_need)
    return s_need | dil3(dil3(s_need))          # block 0: the residual 1x1 under the second 3x3, the first 3x3 one pixel around it


def test_needs_cover_every_dependency_and_rects_cover_needs(planned):
    up, down = planned
    for c in live_classes(up):
        need = [mask_of(down["needs"][l, c], res_of(l)) for l in range(NL)]
        rect = [mask_of(down["rects"][l, c], res_of(l)) for l in range(NL)]
        for l in range(NL):
            assert need[l].any() and inside(need[l], rect[l]), (c, l)
        out = bottleneck_reads(down, c)
        for b in range(N_DOWN - 1, -1, -1):
            L = 6 * b
            assert inside(out, need[L + 5]), f"class {c} block {b}: pooled pixels"
            assert inside(out, need[L + 4]), f"class {c} block {b}: residual pixels the add takes"
            p2 = window_s2(out)
            assert inside(p2, need[L + 3]) and inside(p2, need[L + 2]), f"class {c} block {b}: second separable layer"
            p1 = dil3(p2)
            assert inside(p1, need[L + 1]) and inside(p1, need[L]), f"class {c} block {b}: first separable layer"
            sampled = out                       # the stride-2 residual 1x1 samples the block's input under these pixels
            out = dil3(p1) | evens(out)
        L = 6 * N_DOWN
        assert inside(sampled, need[L]), f"class {c}: stem at the even pixels (read by block 0's residual 1x1 only)"
        assert inside(out, need[L + 1]), f"class {c}: stem"
        assert inside(window_s2(out), need[L + 2]), f"class {c}: input window"
        # a consumer's NEED, grown by its taps, lies inside what its producer computes -- also for the rounded rectangles of the pooled
        # pixels, which the fix-up pass of a fused level finishes from the strips of the tiles below and to the right
        for b in range(N_DOWN):
            L = 6 * b
            assert inside(window_s2(need[L + 5]), rect[L + 3])
            assert inside(need[L + 3], rect[L + 2]) and inside(dil3(need[L + 2]), rect[L + 1]) and inside(need[L + 1], rect[L])
            assert inside(need[L + 5], rect[L + 4])
            if b:
                assert inside(dil3(need[L]), rect[6 * (b - 1) + 5]) and inside(evens(need[L + 4]), rect[6 * (b - 1) + 5])


def test_rects_have_the_form_their_kernels_want(planned):
    up, down = planned
    for c in live_classes(up):
        for l in range(NL):
            y0, x0, rh, rw = (int(v) for v in down["rects"][l, c])
            R = res_of(l)
            assert 0 <= y0 and y0 + rh <= R and 0 <= x0 and x0 + rw <= R and rh >= 1 and rw >= 1, (c, l)
        for b in range(N_DOWN):
            H = (WS // 2) >> b
            for k in range(4):
                y0, x0, rh, rw = (int(v) for v in down["rects"][6 * b + k, c])
                if (FUSED >> b) & 1:            # whole 16 x 16 tiles
                    assert y0 % 16 == 0 and x0 % 16 == 0 and rh % 16 == 0 and rw % 16 == 0, (c, b, k)
                else:                           # conv_mfma_kernel<..., ROI>'s column rule; the depthwise strips (4 columns) in front of it
                    assert x0 % 4 == 0 and rw >= 2 and (rw % 8 == 0 or rw == H or (H < 64 and rw % 4 == 0)), (c, b, k)
            for k in (0, 2):                    # a depthwise layer computes what its pointwise layer takes
                assert (down["rects"][6 * b + k, c] == down["rects"][6 * b + k + 1, c]).all()
            y0, x0, rh, rw = (int(v) for v in down["rects"][6 * b + 4, c])
            assert x0 % 4 == 0 and rw >= 2 and (rw % 8 == 0 or rw == H // 2 or (H // 2 < 64 and rw % 4 == 0)), (c, b)
        # the stem at the even pixels is written for exactly the pixels block 0's residual 1x1 enumerates, in whole groups of 4 columns
        assert (down["rects"][6 * N_DOWN, c] == down["rects"][4, c]).all()
        assert down["rects"][6 * N_DOWN, c, 1] % 4 == 0 and down["rects"][6 * N_DOWN, c, 3] % 4 == 0


def test_totals_match_the_rectangles(planned):
    up, down = planned
    per_px = np.zeros(NL)
    for b in range(N_DOWN):
        per_px[6 * b + 1] = DOWN_CH[b] * DOWN_CH[b + 1]
        per_px[6 * b + 3] = DOWN_CH[b + 1] ** 2
        per_px[6 * b + 4] = DOWN_CH[b] * DOWN_CH[b + 1]
    tiles = up["tiles_per_img"]
    for l in range(NL):
        area = sum(int(up["class_count"][c]) * int(down["rects"][l, c, 2]) * int(down["rects"][l, c, 3]) for c in range(up["n_classes"]))
        assert down["mac_planned"][l] == area * per_px[l]
        assert down["mac_full"][l] == tiles * res_of(l) ** 2 * per_px[l]
        assert down["mac_planned"][l] <= down["mac_full"][l] and down["bytes_planned"][l] <= down["bytes_full"][l]
        if down["bytes_full"][l]:
            assert down["bytes_planned"][l] * tiles * res_of(l) ** 2 == down["bytes_full"][l] * area


def test_bench_geometry_is_tight():
    """640 x 640: a half-needed axis keeps 32 of 40 rows at the unfused level (the bottleneck rectangle starts at row 4 of 20, the pool
    window and two depthwise layers reach 8 - 2 = 6 at most), so its matrix work stays below 0.9 of full-frame; a planner that falls back
    to everything fails."""
    down = _lib.roi_plan_down(640, 640, WS, UP_CH, DOWN_CH, FUSED)
    for l in range(NL):
        if down["mac_full"][l]:
            print(f"  layer {l:2d}: matrix work planned / full {down['mac_planned'][l] / down['mac_full'][l]:.4f}")
        if down["bytes_full"][l]:
            print(f"  layer {l:2d}: bytes planned / full {down['bytes_planned'][l] / down['bytes_full'][l]:.4f}")
    lv = slice(12, 18)
    assert down["mac_planned"][lv].sum() <= 0.9 * down["mac_full"][lv].sum()
    assert down["bytes_planned"][lv].sum() <= 0.9 * down["bytes_full"][lv].sum()
    print(f"  whole free tiles per level: {list(down['free_tile'])}")
    assert down["free_tile"][N_DOWN - 1] == 0, "the unfused level has no tiles"


def test_outputs_depend_on_the_planned_window_only(weights):
    """one patch of each of the 3 x 3 classes at 320 x 320 through the oracle, then again with every input pixel outside the class's
    planned input window replaced: the bottleneck tensor inside the rectangle up block 0 reads, the outputs of down blocks 0 and 1 inside
    their needed rectangles and the final output inside the rectangle the blend reads keep their bits; and the window is not everything"""
    from oracle import unet as ou
    up = _lib.roi_plan(320, 320, WS, UP_CH)
    down = _lib.roi_plan_down(320, 320, WS, UP_CH, DOWN_CH, FUSED)
    classes = live_classes(up)
    assert len(classes) == 9
    rs = np.random.RandomState(5)
    x = rs.uniform(0, 1, (len(classes), WS, WS)).astype(np.float32)
    y = x.copy()
    cut = 0
    for i, c in enumerate(classes):
        win = mask_of(down["needs"][6 * N_DOWN + 2, c], WS)
        other = rs.uniform(0, 1, (WS, WS)).astype(np.float32)
        y[i][~win] = other[~win]
        cut += int((~win).sum())
    assert cut > 0, "no class has a window smaller than the patch"
    tx, ty = {}, {}
    ox, oy = ou.forward_exact(weights, x, taps=tx), ou.forward_exact(weights, y, taps=ty)
    for i, c in enumerate(classes):
        for b in range(N_DOWN):
            m = mask_of(down["needs"][6 * b + 5, c], res_of(6 * b + 5))
            if b == N_DOWN - 1:
                assert inside(bottleneck_reads(down, c), m)
            a, bb = tx[f"down{b}"][i][m], ty[f"down{b}"][i][m]
            assert np.array_equal(a.view(np.uint32), bb.view(np.uint32)), f"class {c}: output of down block {b}"
        fy0, fx0, fh, fw = (int(v) for v in down["needs"][6 * N_DOWN + 3, c])        # what the blend reads of the patch
        a, bb = ox[i, fy0:fy0 + fh, fx0:fx0 + fw], oy[i, fy0:fy0 + fh, fx0:fx0 + fw]
        assert np.array_equal(a.view(np.uint32), bb.view(np.uint32)), f"class {c}: final output"
    # the check can fail: one replaced pixel just inside a window changes the bottleneck rectangle
    c = classes[0]
    ny0, nx0, nh, nw = (int(v) for v in down["needs"][6 * N_DOWN + 2, c])
    z = x[:1].copy()
    z[0, ny0 + nh // 2, nx0 + nw // 2] += 0.5
    tz = {}
    ou.forward_exact(weights, z, taps=tz)
    m = mask_of(down["needs"][6 * N_DOWN - 1, c], res_of(6 * N_DOWN - 1))
    assert not np.array_equal(tz[f"down{N_DOWN - 1}"][0][m], tx[f"down{N_DOWN - 1}"][0][m])
