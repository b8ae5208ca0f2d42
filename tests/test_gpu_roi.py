"""GPU: the region form of the tiled up path (TMAT_ROI=1, the default) computes what whole patches compute (TMAT_ROI=0).

The smooth blend reads of a patch only the rectangle  patch ∩ interior; the tiled entry points compute that rectangle, grown backwards
through the up path by the planner (tests/test_roi_plan.py), in class-major patch order.  A computed pixel sees the same operands in
the same order, so every result is bit-identical; a read outside what a producer wrote shows under the poison patterns (0xFF: NaN,
0x7F: large finite floats) as a NaN or a bit difference.  Passes of 8, 3 and 1 images with a ragged last pass, by the handle's
patch capacity.  One handle per setting; nothing is retried.
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:220-267 (predict_img_with_smooth_windowing), models.py:146-166 (up path)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)


def make_handle(weights, max_patches, roi):
    """TMAT_ROI is read at tmat_create"""
    from tmat_amd import synth, _lib
    old = os.environ.get("TMAT_ROI")
    os.environ["TMAT_ROI"] = "1" if roi else "0"
    try:
        return _lib.Handle(synth.pack_weights(weights), 0, max_patches)
    finally:
        if old is None:
            del os.environ["TMAT_ROI"]
        else:
            os.environ["TMAT_ROI"] = old


def tiles_per_img(hh, ww, ws=320):
    return 8 * (hh // (ws // 2) + 1) * (ww // (ws // 2) + 1)       # aug = ws / 2: the padded frame holds hh / step + 1 windows


# (hh, ww, images per pass, images): the bench geometry in passes of 8 + 1, one patch wide in passes of 3 + 3 + 1, the non-square
# 157 x 188 one image per pass, an image smaller than a patch in passes of 3 + 1, 512 x 512 (all but one patch of 9 on the border)
SMOOTH_CASES = [(640, 640, 8, 9), (320, 320, 3, 7), (157, 188, 1, 2), (100, 90, 3, 4), (512, 512, 3, 4)]
ORACLE_CASES = {(157, 188), (100, 90)}          # the sizes the CPU oracle runs in seconds (the existing tests compare at 200 x 180)


@pytest.mark.parametrize("hh, ww, per_pass, n", SMOOTH_CASES, ids=lambda v: str(v))
def test_predict_smooth_roi_equals_full_frame(weights, hh, ww, per_pass, n):
    rs = np.random.RandomState(100 + hh)
    x = rs.uniform(0, 1, (n, hh, ww)).astype(np.float32)
    x[0, : hh // 2] = 0.0
    maxp = tiles_per_img(hh, ww) * per_pass
    h0, h1 = make_handle(weights, maxp, False), make_handle(weights, maxp, True)
    try:
        full = h0.predict_smooth(x)
        assert not np.isnan(full).any()
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, pattern {pattern:#x}: {nbad} of {got.size} values differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the region-form prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
    finally:
        h0.close()
        h1.close()
    if (hh, ww) in ORACLE_CASES:
        from oracle import unet as ou, blend
        ref = blend.predict_img_with_smooth_windowing(x[0], 320, 2, ou.predict_exact(weights))
        nbad = int((full[0].view(np.uint64) != ref.view(np.uint64)).sum())
        assert nbad == 0, f"{nbad} of {ref.size} differ from the oracle"


def test_analyze_batch_roi_equals_full_frame(weights):
    """the bench geometry (1024 x 1024 sources, 640 x 640 network input) in passes of 8 + 1, and a non-square source whose tiling
    leaves a remainder; rows equal between the settings, and equal to the oracle for the small one"""
    from oracle import pipeline
    from tmat_amd import branches, synth
    big = np.stack([synth.synth_image(50 + i, 1024) for i in range(9)])
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]            # 250 x 300 -> 188 x 156
    want_odd = pipeline.analyze_image(odd, weights, CFG, 300.0)
    h0, h1 = make_handle(weights, 1600, False), make_handle(weights, 1600, True)
    try:
        rows0 = branches.analyze_batch(h0, big, CFG, 1000.0)
        odd0 = branches.analyze_batch(h0, odd[None], CFG, 300.0)[0]
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            rows1 = branches.analyze_batch(h1, big, CFG, 1000.0)
            assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"pattern {pattern:#x}"
            h1.debug_poison(pattern)
            odd1 = branches.analyze_batch(h1, odd[None], CFG, 300.0)[0]
            assert odd1[1:] == odd0[1:], f"pattern {pattern:#x}"
        assert (odd0[1], odd0[2], odd0[3]) == tuple(want_odd)
    finally:
        h0.close()
        h1.close()


def test_unet_forward_stays_whole_patches(weights):
    """the raw entry point computes full frames whatever TMAT_ROI says: equal to oracle/unet_exact.c on ALL pixels"""
    from oracle import unet as ou
    rs = np.random.RandomState(77)
    x = rs.uniform(0, 1, (5, 320, 320)).astype(np.float32)
    ref = ou.forward_exact(weights, x)
    h1 = make_handle(weights, 8, True)
    try:
        h1.debug_poison(0xFF)
        got = h1.unet_predict(x)
        assert int((got.view(np.uint32) != ref.view(np.uint32)).sum()) == 0
    finally:
        h1.close()
