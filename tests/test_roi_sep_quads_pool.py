"""CPU: the quadrant tables of the POOLED fused separable layers (csrc/roi_plan.cpp:roi_sep_quad_pool_table through
tmat_roi_sep_quads_pool).

Under the shared-interior form a pooled fused launch (layer 6 b + 3) may visit 8 x 8 quadrants, four to a packed tile, like the plain
layer in front of it (tests/test_roi_sep_quads.py).  The table is checked against a brute-force enumeration that shares nothing with it
but the planner's outputs: the comp masks of tmat_roi_plan_share, the classes and ranks of tmat_roi_plan and the position formula of
include/tmat.h,
    position(img, tile) = k * base[c] + img * class_count[c] + tile_rank[tile],  c = tile_class[tile].
Every quadrant of a patch that holds a comp pixel of the layer must be listed exactly once, no other quadrant of the pass's own patches,
in the order of the tile table of the same form, then every quadrant of the k all-constant patches tile by tile, then the padding.

The pooled launch leaves the last pooled row and column of a QUADRANT as partial maxima, which the fix-up pass completes from the strips
of the quadrants below and to the right.  So the table must satisfy the window invariant: for every pooled pixel the patch computes for
a later launch or copy (comp of layer 6 b + 5), every quadrant that holds a pixel of its window, rows 2 y .. 2 y + 2 x columns
2 x .. 2 x + 2 cut to the patch (MaxPooling2D(3, 2, "same") pads behind the last row and column), is listed."""
import numpy as np
import pytest

from tmat_amd import _lib

WS = 320
GEOMS = [(320, 320), (480, 320), (640, 640), (100, 90), (250, 300)]
LAYERS = (3, 9)
KS = (1, 3)
TILES_640 = {3: 7200, 9: 2312}          # the tile tables at the bench's geometry, per image
GROUPS_640 = {3: 5000, 9: 1800}         # packed tiles per image there: the counts of the plain layers 1 and 7


def side(layer):
    return (WS // 2) >> (layer // 6)


def patches_of(hh, ww, k):
    """(position, class) of every patch of a pass of k images"""
    up = _lib.roi_plan(hh, ww)
    tpi, cnt = up["tiles_per_img"], up["class_count"]
    base = np.concatenate([[0], np.cumsum(cnt)])
    out = []
    for img in range(k):
        for tile in range(tpi):
            c = int(up["tile_class"][tile])
            out.append((k * int(base[c]) + img * int(cnt[c]) + int(up["tile_rank"][tile]), c))
    return out, k * tpi


def brute_force(hh, ww, layer, k):
    """the own patches' needed quadrants as a sorted array of ids"""
    share = _lib.roi_plan_share(hh, ww)
    QW = side(layer) // 8
    pts, n = patches_of(hh, ww, k)
    ids = []
    for pos, c in pts:
        rows = share["comp"][layer][c][0][: 8 * QW].reshape(QW, 8).any(axis=1)
        cols = share["comp"][layer][c][1][: 8 * QW].reshape(QW, 8).any(axis=1)
        for qy in np.flatnonzero(rows):
            for qx in np.flatnonzero(cols):
                ids.append(pos * QW * QW + int(qy) * QW + int(qx))
    return np.array(sorted(ids), np.int64), n


def tile_of(q, layer):
    QW = side(layer) // 8
    TW = QW // 2
    pt, r = q // (QW * QW), q % (QW * QW)
    return pt * TW * TW + (r // QW // 2) * TW + (r % QW) // 2


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("hh, ww", GEOMS, ids=lambda v: str(v))
def test_table_equals_brute_force(hh, ww, layer, k):
    ids, own, n_ids, full = _lib.roi_sep_quads_pool(hh, ww, layer, k)
    ids = ids.astype(np.int64)
    want, patches = brute_force(hh, ww, layer, k)
    QW = side(layer) // 8
    QPP, TPP = QW * QW, (QW // 2) ** 2
    assert full == patches * TPP
    # the own patches: every needed quadrant exactly once, no other
    assert own == len(want), f"{own} quadrants of the pass's own patches, brute force {len(want)}"
    assert np.array_equal(np.sort(ids[:own]), want), "the listed quadrants differ from the brute-force set"
    assert ids[:own].max() < patches * QPP
    # a refinement of the tile table of the form, in its order: the quadrants of one tile together, row-major inside it
    tiles, tfull = _lib.roi_sep_tiles_share(hh, ww, layer, k)
    assert tfull == full
    t = tile_of(ids[:own], layer)
    first = np.concatenate([[True], t[1:] != t[:-1]])
    assert np.array_equal(t[first], tiles.astype(np.int64)), "the quadrants' tiles are not the tile table in its order"
    same = ~first[1:]
    assert np.all(ids[1:own][same] > ids[:own - 1][same]), "slot order inside a tile is (qy, qx) row-major"
    # the k constant patches behind them: every tile as itself
    const = ids[own:n_ids]
    assert n_ids - own == k * QPP
    tc = np.arange(patches * TPP, (patches + k) * TPP)
    pt, r = tc // TPP, tc % TPP
    TW = QW // 2
    q0 = pt * QPP + (r // TW) * 2 * QW + (r % TW) * 2
    assert np.array_equal(const, (q0[:, None] + np.array([0, 1, QW, QW + 1])[None, :]).ravel())
    # ceil(n / 4) groups, the last one padded with its last id
    assert len(ids) == 4 * ((n_ids + 3) // 4)
    assert np.all(ids[n_ids:] == ids[n_ids - 1])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("hh, ww", GEOMS, ids=lambda v: str(v))
def test_window_invariant(hh, ww, layer, k):
    """every quadrant under the window of a pooled pixel the patch computes is listed (brute force over the pixels)"""
    ids, own, _, _ = _lib.roi_sep_quads_pool(hh, ww, layer, k)
    listed = set(int(q) for q in ids[:own])
    share = _lib.roi_plan_share(hh, ww)
    H = side(layer)
    QW = H // 8
    pts, _ = patches_of(hh, ww, k)
    checked = 0
    by_class = {}
    for pos, c in pts:
        if c not in by_class:
            rows = np.flatnonzero(share["comp"][layer + 2][c][0][: H // 2])
            cols = np.flatnonzero(share["comp"][layer + 2][c][1][: H // 2])
            need = set()
            for py in rows:
                for px in cols:
                    for y in range(2 * py, min(2 * py + 3, H)):
                        for x in range(2 * px, min(2 * px + 3, H)):
                            need.add((y // 8) * QW + x // 8)
            by_class[c] = (need, len(rows) * len(cols))
        need, npix = by_class[c]
        checked += npix
        missing = [q for q in need if pos * QW * QW + q not in listed]
        assert not missing, f"patch {pos} (class {c}): quadrants {sorted(missing)[:8]} hold window pixels and are not listed"
    assert checked > 0


@pytest.mark.parametrize("k", KS)
def test_counts_at_the_bench_geometry(k):
    for layer, groups in GROUPS_640.items():
        ids, own, n_ids, full = _lib.roi_sep_quads_pool(640, 640, layer, k)
        tiles, _ = _lib.roi_sep_tiles_share(640, 640, layer, k)
        print(f"layer {layer}, k {k}: {own} quadrants = {own / 4 / k} packed tiles per image, {len(tiles) // k} tiles per image")
        assert len(tiles) == TILES_640[layer] * k
        assert own == 4 * groups * k, f"layer {layer}: {own} quadrants"
        assert own < 4 * len(tiles)


def test_the_forms_above_share_keep_the_table():
    for layer in LAYERS:
        want = _lib.roi_sep_quads_pool(640, 640, layer, 2, "share")
        for form in ("share_rect", "share_fused_rect"):
            got = _lib.roi_sep_quads_pool(640, 640, layer, 2, form)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (layer, form)


def test_refusals():
    for layer in (1, 7, 0, 2, 4, 5, 15, -1, 99):            # the plain layers have tmat_roi_sep_quads; the others are no fused layers
        with pytest.raises(_lib.TmatError):
            _lib.roi_sep_quads_pool(320, 320, layer, 1)
    for form in ("full", "region", "const", 6, -1):
        for layer in LAYERS:
            with pytest.raises(_lib.TmatError):
                _lib.roi_sep_quads_pool(320, 320, layer, 1, form)
    with pytest.raises(_lib.TmatError):
        _lib.roi_sep_quads_pool(320, 320, 3, 1, fused_mask=2)       # level 0 unfused
    with pytest.raises(_lib.TmatError):
        _lib.roi_sep_quads_pool(320, 320, 3, 0)
    for layer in LAYERS:                                            # and the plain entry goes on refusing the pooled layers
        with pytest.raises(_lib.TmatError):
            _lib.roi_sep_quads(320, 320, layer, 1)
