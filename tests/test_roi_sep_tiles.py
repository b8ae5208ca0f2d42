"""CPU: the tile tables of the fused separable layers' region form (csrc/roi_plan.cpp:roi_sep_tile_table through tmat_roi_sep_tiles).

With TMAT_ROI_DOWN bit 1 a fused separable launch visits only the 16 x 16 tiles its table names.  The table is checked here against a
brute-force enumeration that shares nothing with it but the planner's outputs: the rectangles of tmat_roi_plan_down, the classes and ranks
of tmat_roi_plan and the position formula of include/tmat.h,
    position(img, tile) = k * base[c] + img * class_count[c] + tile_rank[tile],  c = tile_class[tile].
Every planned (patch, ty, tx) must appear exactly once, patches in ascending position and row-major inside a patch's rectangle, as the
full-frame id  position * TPP + ty * TW + tx  (the strips of the pooled form are addressed by that id).  The table depends on the images
per pass k: 1, 3 and 8 are checked, on geometries from one smaller than a patch to the bench's 640 x 640, 200 x 330 among them (11
classes with unequal counts).  The planned counts are pinned to the figures the layers were costed with."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
FUSED_LAYERS = (1, 3, 7, 9)             # 6 b + 1 and 6 b + 3 of the fused levels b = 0 (160 pixels a side) and b = 1 (80)
GEOMS = [(640, 640), (320, 320), (200, 330), (157, 188), (100, 90)]
KS = (1, 3, 8)
# tiles per image, planned: layer -> count; full: 100 (160 a side) resp. 25 (80 a side) per patch
PLANNED = {
    (100, 90): {1: 648, 9: 128},
    (157, 188): {1: 1368, 9: 288},
    (320, 320): {1: 6272, 9: 1568},
}
SHARE = {
    (640, 640): {1: 0.9216, 3: 0.9216, 7: 1.0, 9: 0.9216},
    (100, 90): {1: 0.81, 3: 0.81, 9: 0.64},
    (157, 188): {1: 0.855, 3: 0.855, 9: 0.72},
}


def side(layer):
    return (WS // 2) >> (layer // 6)


def brute_force(hh, ww, layer, k):
    up, down = _lib.roi_plan(hh, ww), _lib.roi_plan_down(hh, ww)
    tpi, cnt = up["tiles_per_img"], up["class_count"]
    base = np.concatenate([[0], np.cumsum(cnt)])
    TW = side(layer) // 16
    TPP = TW * TW
    entries = []
    for img in range(k):
        for tile in range(tpi):
            c = int(up["tile_class"][tile])
            pos = k * int(base[c]) + img * int(cnt[c]) + int(up["tile_rank"][tile])
            y0, x0, rh, rw = (int(v) for v in down["rects"][layer][c])
            assert y0 % 16 == 0 and x0 % 16 == 0 and rh % 16 == 0 and rw % 16 == 0, "a fused level's rectangles are whole tiles"
            for ty in range(y0 // 16, (y0 + rh) // 16):
                for tx in range(x0 // 16, (x0 + rw) // 16):
                    entries.append((pos, ty, tx))
    entries.sort()
    return np.array([p * TPP + ty * TW + tx for p, ty, tx in entries], np.int64), k * tpi * TPP


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("hh, ww", GEOMS, ids=lambda v: str(v))
def test_table_equals_brute_force(hh, ww, k):
    for layer in FUSED_LAYERS:
        ids, full = _lib.roi_sep_tiles(hh, ww, layer, k)
        want, want_full = brute_force(hh, ww, layer, k)
        assert full == want_full
        assert len(ids) == len(want), f"layer {layer}: {len(ids)} tiles, brute force {len(want)}"
        assert np.array_equal(ids.astype(np.int64), want), f"layer {layer}: table differs from the brute-force enumeration"
        assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < full


def test_200_by_330_has_eleven_unequal_classes():
    up = _lib.roi_plan(200, 330)
    counts = [int(c) for c in up["class_count"] if c > 0]
    assert up["n_classes"] == 11 and len(set(counts)) > 1, counts


@pytest.mark.parametrize("hh, ww", sorted(PLANNED), ids=lambda v: str(v))
def test_planned_counts(hh, ww):
    tpi = _lib.roi_plan(hh, ww)["tiles_per_img"]
    for layer, planned in PLANNED[(hh, ww)].items():
        for k in KS:
            ids, full = _lib.roi_sep_tiles(hh, ww, layer, k)
            assert (len(ids), full) == (k * planned, k * tpi * (side(layer) // 16) ** 2), f"layer {layer}, k {k}"


@pytest.mark.parametrize("hh, ww", sorted(SHARE), ids=lambda v: str(v))
def test_planned_share(hh, ww):
    for layer, share in SHARE[(hh, ww)].items():
        ids, full = _lib.roi_sep_tiles(hh, ww, layer, 1)
        assert abs(len(ids) / full - share) < 5e-4, f"layer {layer}: {len(ids)} of {full}"
    free = _lib.roi_plan_down(hh, ww)["free_tile"]
    assert free[0] == 1 and free[1] == 1


def test_not_a_fused_layer_is_refused():
    for layer in (0, 2, 4, 5, 13, 15, -1, 99):
        with pytest.raises(_lib.TmatError):
            _lib.roi_sep_tiles(320, 320, layer, 1)
    with pytest.raises(_lib.TmatError):
        _lib.roi_sep_tiles(320, 320, 1, 1, fused_mask=2)       # level 0 unfused: no tile rectangles there
