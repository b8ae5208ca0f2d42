"""GPU: the exact rectangles of the up path's region plan (TMAT_ROI_EXACT=1, the default) give what the tight ones (TMAT_ROI_EXACT=0)
and whole patches (TMAT_ROI=0) give.

In the exact plan every up-path layer computes its own need and nothing else, columns unrounded (tests/test_roi_plan_exact.py): odd
first columns, odd widths and -- at 157 x 188, one image per pass -- pixel counts off the multiples of 8, which the convolution
kernel's per-lane prologue and row-split epilogue take (tests/test_gpu_conv_roi.py has them one launch at a time).  Every pixel just outside a
rectangle is now one nobody wrote: a computed pixel that read one -- a tap, a low-resolution residual row, a stored pixel under a
sub-pixel layer, final_kernel's 10 x 18 stage -- and fed the blend would show under the poison patterns (0xFF: NaN, 0x7F: large finite
floats) as a NaN or a bit difference.  A computed pixel sees the same operands in the same order in all three settings, so the
predictions are bit-identical; there is no tolerance.  One handle per setting and case (the patch capacity sets the images per pass);
nothing is retried.
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:220-267 (predict_img_with_smooth_windowing), models.py:146-166 (up path)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_handle(weights, max_patches, **env):
    """TMAT_ROI, TMAT_ROI_TIGHT and TMAT_ROI_EXACT are read at tmat_create"""
    from tmat_amd import synth, _lib
    names = ("TMAT_ROI", "TMAT_ROI_TIGHT", "TMAT_ROI_EXACT")
    old = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(env)
    try:
        return _lib.Handle(synth.pack_weights(weights), 0, max_patches)
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def tiles_per_img(hh, ww, ws=320):
    return 8 * (hh // (ws // 2) + 1) * (ww // (ws // 2) + 1)       # aug = ws / 2: the padded frame holds hh / step + 1 windows


# (hh, ww, images per pass, images): one patch wide (every class is half-needed on some axis) in passes of 3 + 3 + 1, the non-square
# 157 x 188 one image per pass, an image smaller than a patch in passes of 3 + 1, the bench geometry in passes of 2 + 1
CASES = [(320, 320, 3, 7), (157, 188, 1, 2), (100, 90, 3, 4), (640, 640, 2, 3)]


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_exact_equals_tight_equals_full_frame(weights, hh, ww, per_pass, n):
    rs = np.random.RandomState(300 + hh)
    x = rs.uniform(0, 1, (n, hh, ww)).astype(np.float32)
    x[0, : hh // 2] = 0.0
    maxp = tiles_per_img(hh, ww) * per_pass
    hs = dict(full=make_handle(weights, maxp, TMAT_ROI="0"), tight=make_handle(weights, maxp, TMAT_ROI_EXACT="0"),
              exact=make_handle(weights, maxp))
    try:
        got, flops = {}, {}
        for pattern in (0xFF, 0x7F):
            for name, h in hs.items():
                h.debug_poison(pattern)
                h.prof_enable(True)
                got[name, pattern] = h.predict_smooth(x)
                flops[name] = h.prof_read()[2]
                assert not np.isnan(got[name, pattern]).any(), f"{name}, pattern {pattern:#x}: NaN in the prediction"
        ref = got["full", 0xFF]
        for key, y in got.items():
            nbad = int((y.view(np.uint64) != ref.view(np.uint64)).sum())
            print(f"{hh} x {ww}, {key[0]}, pattern {key[1]:#x}: {nbad} of {y.size} values differ from the full-frame run")
            assert nbad == 0, f"{key}: {nbad} of {y.size} differ, max |d| = {np.abs(y - ref).max()}"
        print(f"{hh} x {ww}: FLOPs of the dominant 3x3 launches: full {flops['full']:.4g}, tight {flops['tight']:.4g}, exact {flops['exact']:.4g}")
        if (hh, ww) == (640, 640):
            assert flops["exact"] < flops["tight"] < flops["full"]
    finally:
        for h in hs.values():
            h.close()
    if (hh, ww) == (157, 188):
        from oracle import unet as ou, blend
        want = blend.predict_img_with_smooth_windowing(x[0], 320, 2, ou.predict_exact(weights))
        nbad = int((ref[0].view(np.uint64) != want.view(np.uint64)).sum())
        assert nbad == 0, f"{nbad} of {want.size} differ from the oracle"
