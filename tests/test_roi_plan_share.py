"""CPU: the shared-interior form of the down plan (csrc/roi_plan.cpp:roi_plan_share through tmat_roi_plan_share).

predict_img_with_smooth_windowing tiles every orientation's padded frame with stride ws / 2, so position v of a tensor of side H is
position v - H / 2 of the next patch on that axis.  Both patches hold the same bits there unless the position's receptive field crosses
either patch's border (the `ring`), where SAME pads zeros.  The planner lets a patch copy that part of the stored tensors of the fused
levels from its right, lower and diagonal neighbours (`fills`) and compute the rest (`comp`); the fused separable layers visit only
the tiles that hold a comp pixel.  Checked here without the planner's interval arithmetic, by brute force on pixel masks, and against
the oracle: overlapping patches cut from one frame are equal, as uint32, on every rectangle the planner copies."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
UP_CH = (512, 512, 256, 128, 64)
DOWN_CH = (64, 128, 256, 512)
N_DOWN = len(DOWN_CH) - 1
FUSED = 3
LS = 6 * N_DOWN
NL = LS + 4
GEOMS = [(320, 320), (480, 320), (640, 640)]
FUSED_LAYERS = (1, 3, 7, 9)
SHARED = (1, 5, 7, 11)           # the stored tensors of the fused levels: first-layer outputs and pooled outputs
SHIFT = {0: (0, 1), 1: (1, 0), 2: (1, 1)}       # direction -> (rows, columns) shifted by half a side


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


def dil3(m, border=False):
    p = np.pad(m, 1, constant_values=border)
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


def reached_s2(m, border=False):
    """the outputs of that window that see a pixel of m (border: or a position behind the far edge)"""
    R = m.shape[0] // 2
    p = np.pad(m, ((0, 2), (0, 2)), constant_values=border)
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


def brute_ring():
    """the outputs whose receptive field, clipped to the patch, touches the patch border: a dilation from outside the patch, layer by layer"""
    ring = [None] * NL
    ring[LS + 3] = ring[LS + 2] = np.zeros((WS, WS), bool)
    ring[LS + 1] = reached_s2(ring[LS + 2], True)
    ring[LS] = ring[LS + 1][0::2, 0::2]
    x = ring[LS + 1]
    for b in range(N_DOWN):
        L = 6 * b
        ring[L] = ring[L + 1] = dil3(x, True)
        ring[L + 2] = ring[L + 3] = dil3(ring[L + 1], True)
        ring[L + 4] = x[0::2, 0::2]
        ring[L + 5] = reached_s2(ring[L + 3], True) | ring[L + 4]
        x = ring[L + 5]
    return ring


def consumers():
    """(producer layer, consumer layer, the consumer's taps as a function of its mask)"""
    out = [(LS + 1, 0, dil3), (LS, 4, lambda m: m), (LS + 1, LS, evens), (LS + 2, LS + 1, window_s2)]
    for b in range(N_DOWN):
        L = 6 * b
        out += [(L, L + 1, lambda m: m), (L + 1, L + 2, dil3), (L + 2, L + 3, lambda m: m), (L + 3, L + 5, window_s2), (L + 4, L + 5, lambda m: m)]
        if b:
            out += [(L - 1, L, dil3), (L - 1, L + 4, evens)]
    return out


def plans(hh, ww):
    up = _lib.roi_plan(hh, ww, WS, UP_CH)
    down = _lib.roi_plan_down(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    cst = _lib.roi_plan_const(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    shr = _lib.roi_plan_share(hh, ww, WS, UP_CH, DOWN_CH, FUSED)
    assert shr["n_classes"] == cst["n_classes"] == up["n_classes"] >= 1
    return up, down, cst, shr


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def planned(request):
    return request.param + plans(*request.param)


def live_classes(up):
    return [c for c in range(up["n_classes"]) if up["rects"][0, c, 2] > 0 and up["class_count"][c] > 0]


def class_masks(up, cst, shr, c):
    """per layer: comp (the product of the two axis sets), the constant fill, the share fill per direction"""
    comp, fill, sfill = [], [], []
    for l in range(NL):
        R = res_of(l)
        comp.append(np.outer(shr["comp"][l, c, 0, :R], shr["comp"][l, c, 1, :R]).astype(bool))
        f = np.zeros((R, R), bool)
        for i in range(4):
            f |= mask_of(cst["fill"][l, c, i], R)
        fill.append(f)
        sfill.append({d: np.zeros((R, R), bool) for d in range(3)})
    for l, cl, d, y0, x0, rh, rw in shr["fills"]:
        if cl != c:
            continue
        m = mask_of((y0, x0, rh, rw), res_of(l))
        assert not any((m & s).any() for s in sfill[l].values()), f"class {c} layer {l}: share-fill rectangles overlap"
        sfill[l][int(d)] |= m
    return comp, fill, sfill


def test_ring_by_brute_force(planned):
    hh, ww, up, down, cst, shr = planned
    ring = brute_ring()
    for c in live_classes(up):
        for l in range(NL):
            assert np.array_equal(~ring[l], mask_of(shr["inner"][l, c], res_of(l))), f"class {c} layer {l}: inner is the complement of the ring"


def test_masks_by_brute_force(planned):
    hh, ww, up, down, cst, shr = planned
    ring = brute_ring()
    classes = live_classes(up)
    masks = {c: class_masks(up, cst, shr, c) for c in classes}
    some_share = False
    for c in classes:
        comp, fill, sfill = masks[c]
        live = [mask_of(cst["live"][l, c], res_of(l)) for l in range(NL)]
        need = [mask_of(down["needs"][l, c], res_of(l)) for l in range(NL)]
        for l in range(NL):
            held = sfill[l][0] | sfill[l][1] | sfill[l][2]
            assert inside(comp[l], live[l]), f"class {c} layer {l}: comp inside live"
            assert not (held & comp[l]).any() and not (held & fill[l]).any(), f"class {c} layer {l}: copied, computed and constant are disjoint"
            assert inside(held, live[l]), f"class {c} layer {l}: a copied pixel lies outside live"
            if l not in SHARED:
                assert not held.any(), f"class {c} layer {l}: only the stored tensors of the fused levels are copied"
            if l % 6 == 4 or l >= 12:
                assert np.array_equal(comp[l], live[l]), f"class {c} layer {l}: a rectangle launch keeps live"
            # on every shifted axis (the other axis has the same borders in both patches) the position and the position half a side
            # back lie outside the ring
            S = res_of(l) // 2
            ring1 = ring[l][S]
            for d, (sy, sx) in SHIFT.items():
                ys, xs = np.nonzero(sfill[l][d])
                assert (ys - sy * S >= 0).all() and (xs - sx * S >= 0).all()
                if sy:
                    assert not ring1[ys].any() and not ring1[ys - S].any(), f"class {c} layer {l} direction {d}: a row in the ring"
                if sx:
                    assert not ring1[xs].any() and not ring1[xs - S].any(), f"class {c} layer {l} direction {d}: a column in the ring"
            some_share |= bool(held.any())
        # the invariant: every tap of every computed pixel lies in the producer's computed set, its constant fill or its share fill
        for prod, cons, taps in consumers():
            t = taps(comp[cons])
            have = comp[prod] | fill[prod] | sfill[prod][0] | sfill[prod][1] | sfill[prod][2]
            assert inside(t, have), f"class {c}: a tap of layer {cons}'s comp outside comp, fill and share fill of layer {prod}"
            if not cst["stored"][prod] and prod < LS:
                assert inside(t, comp[prod]), f"class {c}: never-stored layer {prod} covers its consumer's window"
        assert inside(need[LS - 1], comp[LS - 1] | fill[LS - 1])
        # a pooled output is read whole by the next level's rectangle launches
        for l in (5, 11):
            assert np.array_equal(comp[l] | sfill[l][0] | sfill[l][1] | sfill[l][2], live[l]), (c, l)
    assert some_share
    # every neighbour pair that occurs: the source pixels are pixels the source patch computed itself
    nbr = shr["neighbours"]
    pairs = set()
    for t in range(up["tiles_per_img"]):
        c = int(up["tile_class"][t])
        if c not in masks:
            continue
        for d, (sy, sx) in SHIFT.items():
            if (c, d, int(nbr[t, d])) in pairs:
                continue
            pairs.add((c, d, int(nbr[t, d])))
            for l in SHARED:
                m = masks[c][2][l][d]
                if not m.any():
                    continue
                assert nbr[t, d] >= 0, f"tile {t} (class {c}) copies from a neighbour it does not have (direction {d})"
                cs = int(up["tile_class"][nbr[t, d]])
                assert cs in masks, f"tile {t}: the neighbour's class computes nothing"
                S = res_of(l) // 2
                src = np.zeros_like(m)
                ys, xs = np.nonzero(m)
                src[ys - sy * S, xs - sx * S] = True
                assert inside(src, masks[cs][0][l]), f"tile {t} class {c} layer {l} direction {d}: a source pixel its patch (class {cs}) does not compute"
    # the neighbour map is the grid's
    step = WS // 2
    off = 0
    for g in range(8):
        na, nb = ((hh // step + 1, ww // step + 1), (ww // step + 1, hh // step + 1))[g & 1]
        for a in range(na):
            for b in range(nb):
                t = off + a * nb + b
                want = (t + 1 if b + 1 < nb else -1, t + nb if a + 1 < na else -1, t + nb + 1 if a + 1 < na and b + 1 < nb else -1)
                assert tuple(int(v) for v in nbr[t]) == want, (g, a, b)
        off += na * nb
    assert off == up["tiles_per_img"]


@pytest.mark.parametrize("k", [1, 3])
def test_tile_table_is_a_subsequence_that_covers_comp(planned, k):
    hh, ww, up, down, cst, shr = planned
    base = np.concatenate([[0], np.cumsum(up["class_count"][:up["n_classes"]])])
    for layer in FUSED_LAYERS:
        live, full = _lib.roi_sep_tiles_live(hh, ww, layer, k, WS, UP_CH, DOWN_CH, FUSED)
        new, full2 = _lib.roi_sep_tiles_share(hh, ww, layer, k, WS, UP_CH, DOWN_CH, FUSED)
        assert full == full2
        it = iter(live.tolist())
        assert all(any(t == u for u in it) for t in new.tolist()), f"layer {layer}: a subsequence of the live table, in its order"
        TW = res_of(layer) // 16
        visited = {}
        for tid in new.tolist():
            pt, t = divmod(tid, TW * TW)
            visited.setdefault(pt, np.zeros((TW, TW), bool))[divmod(t, TW)] = True
        for c in live_classes(up):
            R = res_of(layer)
            comp = np.outer(shr["comp"][layer, c, 0, :R], shr["comp"][layer, c, 1, :R]).astype(bool)
            tiles = comp.reshape(TW, 16, TW, 16).any(axis=(1, 3))
            for pt in range(k * int(base[c]), k * int(base[c + 1])):
                assert np.array_equal(visited.get(pt, np.zeros((TW, TW), bool)), tiles), f"layer {layer} class {c}: the tiles that hold a comp pixel"


def test_the_form_is_not_vacuous():
    """640 x 640: strictly fewer tiles than the constant-ring form in all four fused layers -- per orientation frame 900 of 1764 at
    160 x 160 and 289 of 441 at 80 x 80 (tiles 6, 7, 8 of 10 resp. tile 3 of 5 skipped on an axis with a successor)"""
    for layer, want in zip(FUSED_LAYERS, (900, 900, 289, 289)):
        new, live = len(_lib.roi_sep_tiles_share(640, 640, layer, 1)[0]), len(_lib.roi_sep_tiles_live(640, 640, layer, 1)[0])
        print(f"  640 x 640 layer {layer}: {new} of {live} tiles per image ({new // 8} of {live // 8} per orientation frame)")
        assert new < live
        assert new == 8 * want


def test_no_neighbour_no_share():
    """100 x 90: one patch per orientation -- nothing is shared, the tables are the constant-ring form's"""
    shr = _lib.roi_plan_share(100, 90)
    assert len(shr["fills"]) == 0 and not shr["share"].any() and (shr["neighbours"] == -1).all()
    for layer in FUSED_LAYERS:
        assert np.array_equal(_lib.roi_sep_tiles_share(100, 90, layer, 2)[0], _lib.roi_sep_tiles_live(100, 90, layer, 2)[0])


TAPS = (("stem", LS + 1), ("down0", 5), ("down1", 11), ("down2", 17))
# the columns of a patch measured equal, with the oracle, to its right neighbour's columns v - H / 2 when the form was proposed
OBSERVED = {"stem": (80, 158), "down0": (41, 77), "down1": (21, 37), "down2": (11, 17)}


def test_overlapping_patches_are_equal_where_the_planner_copies(weights):
    """four 320 x 320 patches cut at stride 160 from a random 480 x 480 frame (right, lower and diagonal neighbour of the first) and
    three in a row from a 320 x 640 frame (the middle patch is source and destination)"""
    from oracle import unet as ou
    rs = np.random.RandomState(23)
    frame = rs.uniform(0, 1, (480, 480)).astype(np.float32)
    row = rs.uniform(0, 1, (320, 640)).astype(np.float32)
    x = np.stack([frame[y:y + WS, x0:x0 + WS] for y in (0, 160) for x0 in (0, 160)] + [row[:, x0:x0 + WS] for x0 in (0, 160, 320)])
    taps = {}
    ou.forward_exact(weights, x, taps=taps)
    # (destination patch, direction) -> source patch
    pairs = [(0, 0, 1), (0, 1, 2), (0, 2, 3), (1, 1, 3), (2, 0, 3), (4, 0, 5), (5, 0, 6)]
    up, down, cst, shr = plans(320, 320)
    ring = brute_ring()
    ring_differs = False
    for name, l in TAPS:
        R = res_of(l)
        S = R // 2
        t = taps[name].view(np.uint32)
        assert t.shape[1:3] == (R, R)
        rects = [(int(d), mask_of((y0, x0, rh, rw), R)) for ll, cl, d, y0, x0, rh, rw in shr["fills"] if ll == l]
        assert bool(rects) == (l in SHARED)
        # every position the ring argument calls equal, the planner's rectangles among them
        inner1 = ~ring[l][S]           # one axis: the other axis has the same borders in both patches
        lo, hi = OBSERVED[name]
        for dst, d, src in pairs:
            sy, sx = SHIFT[d]
            eq = np.zeros((R, R), bool)
            eq[sy * S:, sx * S:] = (t[dst][sy * S:, sx * S:] == t[src][:R - sy * S, :R - sx * S]).all(axis=-1)
            zr = np.ones(R, bool) if not sy else np.concatenate([np.zeros(S, bool), inner1[S:] & inner1[:S]])
            zc = np.ones(R, bool) if not sx else np.concatenate([np.zeros(S, bool), inner1[S:] & inner1[:S]])
            zone = np.outer(zr, zc)
            assert eq[zone].all(), f"{name}, patch {dst} direction {d}: {int((zone & ~eq).sum())} pixels outside both rings differ"
            for dd, m in rects:
                if dd == d:
                    assert inside(m, zone) and eq[m].all(), f"{name}, patch {dst} direction {d}: a copied rectangle differs"
            if d == 0:
                cols = np.nonzero(zone.any(axis=0))[0]
                assert lo <= cols.min() and cols.max() <= hi, f"{name}: the planner's zone {cols.min()} .. {cols.max()} inside the observed {lo} .. {hi}"
                assert eq[:, lo:hi + 1].all(), f"{name}, patch {dst}: the observed columns {lo} .. {hi} are equal over all rows"
            ring_differs |= bool((~eq & ~zone)[sy * S:, sx * S:].any())
    assert ring_differs, "some pixel inside the ring must differ, or the form is vacuous"
