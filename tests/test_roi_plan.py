"""CPU: the region planner of the UNet up path (csrc/roi_plan.cpp through tmat_roi_plan).

The smooth blend throws the padding ring away, so of a patch only the rectangle  patch ∩ interior  is read; the tiled entry points
compute that rectangle, grown backwards through the up path, instead of whole patches.  Checked here against brute force:
coverage (everything blend_kernel reads lies inside the final rectangle), nesting (needed ⊆ planned in every layer, and a consumer's
planned region, dilated by its taps' reach, inside what its producer plans to write), tightness for the bench geometry (a planner
that falls back to "everything" fails) and the class-major patch order (a bijection).
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:68-79, 136-217 (pad, tile, blend, crop)."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
CHANNELS = (512, 512, 256, 128, 64)
N_UP = len(CHANNELS) - 1
# the bench geometry, one patch wide, the non-square 157 x 188 (a 250 x 300 source at 0.625), smaller than a patch, and 512 x 512
GEOMS = [(640, 640), (320, 320), (157, 188), (100, 90), (512, 512)]


def geom(hh, ww, ws=WS):
    step, aug = ws // 2, (ws + 1) // 2
    Hp, Wp = hh + 2 * aug, ww + 2 * aug
    cntH, cntW = (Hp - ws) // step + 1, (Wp - ws) // step + 1
    na, nb = (cntH, cntW), (cntW, cntH)
    off, o = [], 0
    for g in range(8):
        off.append(o)
        o += na[g & 1] * nb[g & 1]
    return dict(hh=hh, ww=ww, ws=ws, step=step, aug=aug, Hp=Hp, Wp=Wp, na=na, nb=nb, off=off, tiles=o)


def pad_to_frame(g, y, x, Hp, Wp):
    """blend_kernels.hip:pad_to_frame"""
    k = g & 3
    xp = Wp - 1 - x if g & 4 else x
    if k == 0:
        return y, xp
    if k == 1:
        return Wp - 1 - xp, y
    if k == 2:
        return Hp - 1 - y, Wp - 1 - xp
    return xp, Hp - 1 - y


def blend_reads(gm):
    """[tiles][ws][ws] bool: the (patch, p, q) that blend_kernel gathers (its loop bounds restated)"""
    ws, step = gm["ws"], gm["step"]
    read = np.zeros((gm["tiles"], ws, ws), bool)
    yo, xo = np.mgrid[0:gm["hh"], 0:gm["ww"]]
    y, x = yo + gm["aug"], xo + gm["aug"]
    for g in range(8):
        u, v = pad_to_frame(g, y, x, gm["Hp"], gm["Wp"])
        na, nb = gm["na"][g & 1], gm["nb"][g & 1]
        a_hi = np.minimum(u // step, na - 1)
        a_lo = np.where(u - ws + step > 0, (u - ws + step) // step, 0)
        b_hi = np.minimum(v // step, nb - 1)
        b_lo = np.where(v - ws + step > 0, (v - ws + step) // step, 0)
        for a in range(na):
            p = u - a * step
            oka = (a >= a_lo) & (a <= a_hi) & (p < ws)
            for b in range(nb):
                q = v - b * step
                ok = oka & (b >= b_lo) & (b <= b_hi) & (q < ws)
                assert (p[ok] >= 0).all() and (q[ok] >= 0).all()
                read[gm["off"][g] + a * nb + b, p[ok], q[ok]] = True
    return read


def dil3(m):
    """3 x 3 binary dilation, clipped to the frame"""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def half_any(m):
    """a half-resolution pixel is needed when any of the 2 x 2 pixels on it is ((y >> 1, x >> 1))"""
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


def rect_mask(r, R, scale=1):
    m = np.zeros((R * scale, R * scale), bool)
    y0, x0, rh, rw = (int(v) for v in r)
    m[y0 * scale:(y0 + rh) * scale, x0 * scale:(x0 + rw) * scale] = True
    return m


def res_of(layer):
    if layer == 3 * N_UP:
        return WS // 2
    j, kind = divmod(layer, 3)
    Hs = WS >> N_UP if j == 0 else (WS >> N_UP) << (j - 1)
    return Hs if kind < 2 or j == 0 else 2 * Hs


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    hh, ww = request.param
    gm = geom(hh, ww)
    plan = _lib.roi_plan(hh, ww, WS, CHANNELS)
    assert plan["tiles_per_img"] == gm["tiles"]
    assert 1 <= plan["n_classes"] <= 16, "these geometries have few classes: no fall-back"
    return gm, plan, blend_reads(gm)


def test_blend_reads_lie_inside_the_final_rectangle(planned):
    gm, plan, read = planned
    final = plan["rects"][3 * N_UP]
    for t in range(gm["tiles"]):
        planned_out = rect_mask(final[plan["tile_class"][t]], WS // 2, 2)      # a stored pixel makes 2 x 2 outputs
        assert not (read[t] & ~planned_out).any(), f"tile {t}: the blend reads outside the planned rectangle"
    # and every pixel of the image is produced by at least one read per orientation
    assert read.any()


def test_needed_and_planned_regions_nest(planned):
    gm, plan, read = planned
    rects = plan["rects"]
    for c in range(plan["n_classes"]):
        tiles = np.flatnonzero(plan["tile_class"] == c)
        assert tiles.size == plan["class_count"][c]
        P = [rect_mask(rects[l, c], res_of(l)) for l in range(3 * N_UP + 1)]
        # the form conv_mfma_kernel's row-uniform paths rely on: inside the frame, first column a multiple of 4, width a multiple of 8 (of 4 below 64 pixels a side) or the whole row
        for l in range(3 * N_UP):
            y0, x0, rh, rw = (int(v) for v in rects[l, c])
            R = res_of(l)
            assert 0 <= y0 and y0 + rh <= R and 0 <= x0 and x0 + rw <= R and rh >= 1 and rw >= 2
            assert x0 % 4 == 0 and (rw % 8 == 0 or rw == R or (R < 64 and rw % 4 == 0)), (l, c, x0, rw)
        # ---- needed, by brute force from what the blend reads of the class's tiles
        out_need = read[tiles].any(axis=0)
        need = half_any(out_need)                       # final convolution: stored pixels whose 2 x 2 outputs are read
        assert not (need & ~P[3 * N_UP]).any(), f"class {c}: final"
        s_need = dil3(need)                             # of the last block's output
        for j in range(N_UP - 1, -1, -1):
            assert not (s_need & ~P[3 * j + 2]).any(), f"class {c}: block {j} second convolution"
            t1_need = dil3(s_need)
            r_need = half_any(s_need) if j else s_need
            assert not (r_need & ~P[3 * j + 1]).any(), f"class {c}: block {j} residual"
            c1_need = half_any(t1_need) if j else t1_need       # sub-pixel form: stored pixel i makes outputs 2i, 2i + 1
            assert not (c1_need & ~P[3 * j]).any(), f"class {c}: block {j} first convolution"
            if j:
                s_need = r_need | subpixel_sources(t1_need)     # plain copy for the residual, activated copy for the first convolution
        # ---- planned: a consumer's region, dilated by its taps' reach and clipped, inside what its producer writes
        assert not (dil3(P[3 * N_UP]) & ~P[3 * N_UP - 1]).any(), f"class {c}: final reads outside block {N_UP - 1}"
        for j in range(N_UP - 1, -1, -1):
            c1, rs, c2 = P[3 * j], P[3 * j + 1], P[3 * j + 2]
            t1_written = np.kron(c1, np.ones((2, 2), bool)).astype(bool) if j else c1
            assert not (dil3(c2) & ~t1_written).any(), f"class {c}: block {j} second convolution reads t1 outside the first one's region"
            assert not ((half_any(c2) if j else c2) & ~rs).any(), f"class {c}: block {j} residual rows outside the 1x1's region"
            if j:
                prev = P[3 * (j - 1) + 2]
                assert not (dil3(c1) & ~prev).any(), f"class {c}: block {j} first convolution reads outside block {j - 1}"
                assert not (rs & ~prev).any(), f"class {c}: block {j} residual 1x1 reads outside block {j - 1}"


def test_macs_match_the_rectangles(planned):
    gm, plan, _ = planned
    per_px = []
    for j in range(N_UP):
        per_px += [(16 if j else 9) * CHANNELS[j] * CHANNELS[j + 1], CHANNELS[j] * CHANNELS[j + 1], 9 * CHANNELS[j + 1] ** 2]
    per_px.append(16 * CHANNELS[N_UP])
    for l, m in enumerate(per_px):
        want = sum(int(plan["class_count"][c]) * int(plan["rects"][l, c, 2]) * int(plan["rects"][l, c, 3]) for c in range(plan["n_classes"])) * m
        assert plan["mac_planned"][l] == want
        assert plan["mac_full"][l] == gm["tiles"] * res_of(l) ** 2 * m
        assert plan["mac_planned"][l] <= plan["mac_full"][l]


def test_bench_geometry_is_tight():
    """640 x 640: 9 classes; the hand estimate with 8-pixel alignment is 0.71 of the full-frame multiply-accumulates, the cap 0.78 leaves
    room for a coarser choice at 20 x 20 and fails a planner that silently computes everything"""
    plan = _lib.roi_plan(640, 640, WS, CHANNELS)
    assert plan["n_classes"] == 9
    frac = plan["mac_planned"].sum() / plan["mac_full"].sum()
    print(f"planned / full-frame multiply-accumulates of the up path at 640 x 640: {frac:.4f}")
    for l in range(3 * N_UP + 1):
        print(f"  layer {l:2d}: {plan['mac_planned'][l] / plan['mac_full'][l]:.4f}")
    assert frac <= 0.78


def test_too_many_classes_falls_back_to_everything():
    plan = _lib.roi_plan(640, 640, WS, CHANNELS, max_classes=4)
    assert plan["n_classes"] == 0
    assert (plan["mac_planned"] == plan["mac_full"]).all()
    assert sorted(plan["tile_rank"]) == list(range(plan["tiles_per_img"]))


@pytest.mark.parametrize("k", [1, 3, 8])
def test_class_major_order_is_a_bijection(planned, k):
    gm, plan, _ = planned
    base = np.concatenate([[0], np.cumsum(plan["class_count"])])
    cls = plan["tile_class"]
    pos = np.array([[k * base[cls[t]] + img * plan["class_count"][cls[t]] + plan["tile_rank"][t] for t in range(gm["tiles"])] for img in range(k)])
    assert sorted(pos.ravel()) == list(range(k * gm["tiles"]))
    for c in range(plan["n_classes"]):           # a class is a contiguous range of patches
        got = np.sort(pos[:, cls == c].ravel())
        assert got[0] == k * base[c] and got[-1] == k * base[c + 1] - 1
