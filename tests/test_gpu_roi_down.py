"""GPU: the region form of the down path (TMAT_ROI_DOWN, default on) computes what whole patches compute (TMAT_ROI=0).

The region-form up path reads only a rectangle of the bottleneck tensor; with TMAT_ROI_DOWN bit 0 the unfused 40-pixel level (depthwise,
pointwise, max-pool + add), the three residual 1x1 layers, the stem at the even pixels and the pooling fix-ups of the fused levels
compute only what that rectangle depends on (tests/test_roi_plan_down.py checks the planner).  A computed pixel sees the same operands
in the same order, so every blended value is bit-identical; a needed pixel that took an operand nobody wrote shows under the poison
patterns (0xFF: NaN, 0x7F: large finite floats) as a NaN or a bit difference.  Small geometries only: 320 x 320 has all nine classes
(the centre included) in passes of 3 + 3 + 1 images, 157 x 188 corner classes on a non-square frame, 100 x 90 an image smaller than a
patch.  TMAT_ROI_DOWN=0 (the up path alone in region form) is compared as well: the switch must select the parent's down path.
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:220-267, models.py:119-144."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
# bit 0: the unfused level and the small kernels; "0": the up path alone in region form.  (Bit 1, the tile-granular form of the fused
# separable layers, is not built; tmat_create refuses it.)
DOWN_SETTINGS = ["1", "0"]


def make_handle(weights, max_patches, roi, roi_down=None):
    """TMAT_ROI and TMAT_ROI_DOWN are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_DOWN": roi_down}
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


# (hh, ww, images per pass, images)
CASES = [(320, 320, 3, 7), (157, 188, 1, 2), (100, 90, 3, 4)]
ORACLE_CASES = {(157, 188), (100, 90)}


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
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("setting", DOWN_SETTINGS)
@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_down_roi_equals_full_frame(weights, full_frame, hh, ww, per_pass, n, setting):
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
    finally:
        h1.close()


@pytest.mark.parametrize("hh, ww", sorted(ORACLE_CASES), ids=lambda v: str(v))
def test_full_frame_reference_equals_the_oracle(weights, full_frame, hh, ww):
    """what the region forms are compared with is itself the oracle's prediction, bit for bit"""
    from oracle import unet as ou, blend
    x, full = full_frame[(hh, ww)]
    ref = blend.predict_img_with_smooth_windowing(x[0], 320, 2, ou.predict_exact(weights))
    nbad = int((full[0].view(np.uint64) != ref.view(np.uint64)).sum())
    assert nbad == 0, f"{nbad} of {ref.size} differ from the oracle"


def test_analyze_batch_down_roi_equals_full_frame(weights):
    """a small non-square source (250 x 300 -> 188 x 156 network input) through the whole pipeline: rows equal between the settings"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    h0 = make_handle(weights, 64, False)
    try:
        rows0 = branches.analyze_batch(h0, np.stack([odd, odd[::-1]]), CFG, 300.0)
    finally:
        h0.close()
    for setting in ("1", "0"):
        h1 = make_handle(weights, 64, True, setting)
        try:
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, np.stack([odd, odd[::-1]]), CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_DOWN={setting}, pattern {pattern:#x}"
        finally:
            h1.close()
