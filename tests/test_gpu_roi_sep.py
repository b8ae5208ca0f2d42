"""GPU: the fused separable layers in region form (TMAT_ROI_DOWN bit 1, default on) compute what whole patches compute (TMAT_ROI=0).

With bit 1 a launch of sepconv_ws_kernel<..., ROI> visits only the 16 x 16 tiles of the layer's rectangles (a device table of full-frame
tile ids, tests/test_roi_sep_tiles.py); a visited tile runs the code of the full-frame form, so it produces the same bits.  Why skipping
the others is safe:
  * a needed pooled pixel on a tile's last row or column reads the strips of the tile below / to the right; the planner's `need` dilates
    by the pool's 2 i .. 2 i + 2, so that tile lies in the layer's rectangle and is visited;
  * a skipped tile leaves its outputs and strips unwritten, and those are read only into pixels outside `need` -- the contract bit 0
    already has for its rectangles;
  * pool_fix_add_kernel restricts itself to its box of pooled pixels.
A needed pixel that took an operand nobody wrote shows under the poison patterns (0xFF: NaN, 0x7F: large finite floats) as a NaN or a
bit difference against the full-frame run.  So that the comparison cannot pass vacuously, the planner's free_tile and tile counts are
asserted for every geometry, and the launches' own counters (taken on the host at launch time) must equal k x those counts.
Geometries: the small ones of test_gpu_roi_down.py -- 100 x 90 (8 patches per image, corner classes), 157 x 188 (16, non-square),
320 x 320 in passes of 3 + 3 + 1 images (all nine classes, two values of k on one handle)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
# None: the default (3); "3": both bits named; "2": the tile tables alone, the small kernels full-frame
SETTINGS = [None, "3", "2"]
# (hh, ww, images per pass, images)
CASES = [(320, 320, 3, 7), (157, 188, 1, 2), (100, 90, 3, 4)]
# tiles per image, planned of full: first fused layer (160 pixels a side), second layer of the 80-pixel level
TILES = {(100, 90): ((648, 800), (128, 200)), (157, 188): ((1368, 1600), (288, 400)), (320, 320): ((6272, 7200), (1568, 1800))}
FUSED_LAYERS = (1, 3, 7, 9)


def make_handle(weights, max_patches, roi, roi_down=None, **env):
    """TMAT_ROI, TMAT_ROI_DOWN and the form switches are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_DOWN": roi_down, "TMAT_FUSED_SEP": None, "TMAT_FUSED_POOL": None, "TMAT_STEM_FUSED": None}
    want.update(env)
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return _lib.Handle(synth.pack_weights(weights), 0, max_patches)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tiles_per_img(hh, ww, ws=320):
    return 8 * (hh // (ws // 2) + 1) * (ww // (ws // 2) + 1)


def planner_counts(hh, ww, k):
    """[(planned, full)] of the four fused launches of a pass of k images, in launch order; a whole layer launches full-frame"""
    from tmat_amd import _lib
    out = []
    for layer in FUSED_LAYERS:
        ids, full = _lib.roi_sep_tiles(hh, ww, layer, k)
        out.append((len(ids), full))
    return out


@pytest.fixture(scope="module")
def full_frame(weights):
    """per case: the input and the whole-patch prediction (TMAT_ROI=0), computed once"""
    out = {}
    for hh, ww, per_pass, n in CASES:
        rs = np.random.RandomState(300 + hh)
        x = rs.uniform(0, 1, (n, hh, ww)).astype(np.float32)
        x[0, : hh // 2] = 0.0
        h0 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, False)
        try:
            full = h0.predict_smooth(x)
            assert all(p == f for p, f in h0.debug_sep_tiles()), "TMAT_ROI=0 launches whole patches"
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_the_plan_has_free_tiles(hh, ww, per_pass, n):
    """not vacuous: every geometry skips tiles in both 160-pixel layers and in the second 80-pixel layer, by the stated counts"""
    from tmat_amd import _lib
    free = _lib.roi_plan_down(hh, ww)["free_tile"]
    assert free[0] == 1 and free[1] == 1
    got = planner_counts(hh, ww, 1)
    (p1, f1), (p9, f9) = TILES[(hh, ww)]
    assert tiles_per_img(hh, ww) * 100 == f1 and tiles_per_img(hh, ww) * 25 == f9
    assert got[0] == (p1, f1) and got[3] == (p9, f9)
    assert got[1][0] < got[1][1]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda v: f"down={v}")
@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_sep_roi_equals_full_frame(weights, full_frame, hh, ww, per_pass, n, setting):
    x, full = full_frame[(hh, ww)]
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, setting)
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, TMAT_ROI_DOWN={setting}, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the region-form prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
            k_last = n % per_pass or per_pass
            assert h1.debug_sep_tiles() == planner_counts(hh, ww, k_last), "the last pass's launches visit the planned tiles"
    finally:
        h1.close()


def test_counters_follow_the_images_per_pass(weights, full_frame):
    """320 x 320 on one handle: a pass of 3 images, then 3 + 3 + 1 (the last pass holds 1), then 2: k x the planner's counts each time;
    with bit 1 off the same launches report whole patches"""
    x, full = full_frame[(320, 320)]
    h1 = make_handle(weights, 72 * 3, True)
    try:
        for imgs, k_last in ((3, 3), (7, 1), (2, 2)):
            h1.predict_smooth(x[:imgs])
            want = planner_counts(320, 320, k_last)
            got = h1.debug_sep_tiles()
            print(f"{imgs} images, last pass {k_last}: {got}")
            assert got == want
            assert got[0] == (k_last * 6272, k_last * 7200) and got[3] == (k_last * 1568, k_last * 1800)
            assert got[1][0] < got[1][1]
    finally:
        h1.close()
    h2 = make_handle(weights, 72 * 3, True, "1")
    try:
        h2.predict_smooth(x[:3])
        assert h2.debug_sep_tiles() == [(f, f) for _, f in planner_counts(320, 320, 3)]
    finally:
        h2.close()


def test_analyze_batch_sep_roi_equals_full_frame(weights):
    """a small non-square source (250 x 300 -> 188 x 156 network input) through the whole pipeline: rows equal between the settings"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    h0 = make_handle(weights, 64, False)
    try:
        rows0 = branches.analyze_batch(h0, np.stack([odd, odd[::-1]]), CFG, 300.0)
    finally:
        h0.close()
    for setting in SETTINGS:
        h1 = make_handle(weights, 64, True, setting)
        try:
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, np.stack([odd, odd[::-1]]), CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_DOWN={setting}, pattern {pattern:#x}"
            got = h1.debug_sep_tiles()
            assert got and any(p < f for p, f in got), "the pipeline's passes take the region form too"
        finally:
            h1.close()


@pytest.mark.parametrize("form", ["TMAT_FUSED_SEP", "TMAT_FUSED_POOL", "TMAT_STEM_FUSED"])
def test_other_forms_at_100_by_90(weights, full_frame, form):
    """the separate depthwise / pointwise kernels, the unfused pooling and the stem written to memory: each may take the region form or
    stay full-frame, and gives the full-frame bits either way"""
    x, full = full_frame[(100, 90)]
    h1 = make_handle(weights, tiles_per_img(100, 90) * 3, True, None, **{form: "0"})
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            assert not np.isnan(got).any(), f"{form}=0, pattern {pattern:#x}: NaN"
            assert nbad == 0, f"{form}=0, pattern {pattern:#x}: {nbad} of {got.size} differ"
        print(f"{form}=0: fused launches (planned, full) {h1.debug_sep_tiles()}")
    finally:
        h1.close()
