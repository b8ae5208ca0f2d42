"""GPU: the constant-ring form of the down path (TMAT_ROI_CONST) computes what whole patches compute (TMAT_ROI=0).

With the form a pass of k images carries k all-constant patches, one per image and filled with its pad value, through the same launches;
the pass's own patches compute rect_live only (tests/test_roi_plan_const.py), and after every launch that writes a stored tensor the
strips of the plan's `fill` are copied from the constant patch of the image.  A needed pixel that took an operand nobody wrote or copied
shows under the poison patterns (0xFF: NaN, 0x7F: large finite floats) as a NaN or a bit difference against the full-frame run.  The
images of a pass have different minima, so a copy from the wrong image's constant patch shows too; one image has its upper half equal to
its minimum (image data that continues the ring).  Geometries and pass sizes: those of test_gpu_roi_sep.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
# (hh, ww, images per pass, images): the last pass is shorter
CASES = [(320, 320, 3, 7), (157, 188, 3, 4), (100, 90, 3, 4)]
FUSED_LAYERS = (1, 3, 7, 9)


def make_handle(weights, max_patches, roi, roi_const=None, **env):
    """the switches are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_CONST": roi_const, "TMAT_ROI_DOWN": None, "TMAT_FUSED_SEP": None,
            "TMAT_FUSED_POOL": None, "TMAT_STEM_FUSED": None}
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


def counts(fn, hh, ww, k):
    out = []
    for layer in FUSED_LAYERS:
        ids, full = fn(hh, ww, layer, k)
        out.append((len(ids), full))
    return out


@pytest.fixture(scope="module")
def full_frame(weights):
    """per case: the input and the whole-patch prediction (TMAT_ROI=0), computed once"""
    out = {}
    for hh, ww, per_pass, n in CASES:
        rs = np.random.RandomState(500 + hh)
        x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
        x[1, : hh // 2] = x[1].min()
        assert len({float(v.min()) for v in x}) == n
        h0 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, False)
        try:
            full = h0.predict_smooth(x)
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_const_equals_full_frame(weights, full_frame, hh, ww, per_pass, n):
    from tmat_amd import _lib
    x, full = full_frame[(hh, ww)]
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1")
    try:
        held = None
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, TMAT_ROI_CONST=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
            k_last = n % per_pass or per_pass
            visited = h1.debug_sep_tiles()
            live, old = counts(_lib.roi_sep_tiles_live, hh, ww, k_last), counts(_lib.roi_sep_tiles, hh, ww, k_last)
            print(f"  last pass ({k_last} images): visited {visited}, dependency plan {old}")
            assert visited == live, "the last pass's launches visit the tiles of rect_live"
            assert all(v[0] < o[0] for v, o in zip(visited, old)), "strictly fewer tiles than the dependency plan in every fused launch"
            if held is None:
                held = h1.debug_held_bytes()
            else:
                assert h1.debug_held_bytes() == held, "held bytes change between calls"
    finally:
        h1.close()


@pytest.mark.parametrize("form", ["TMAT_FUSED_SEP", "TMAT_FUSED_POOL", "TMAT_STEM_FUSED", "TMAT_ROI_DOWN=1", "TMAT_ROI_DOWN=2"])
def test_other_forms_at_100_by_90(weights, full_frame, form):
    """the separate depthwise / pointwise kernels, the unfused pooling, the stem written to memory, and either bit of TMAT_ROI_DOWN alone"""
    x, full = full_frame[(100, 90)]
    env = {form.split("=")[0]: form.split("=")[1] if "=" in form else "0"}
    h1 = make_handle(weights, tiles_per_img(100, 90) * 3, True, "1", **env)
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            assert not np.isnan(got).any(), f"{form}, pattern {pattern:#x}: NaN"
            assert nbad == 0, f"{form}, pattern {pattern:#x}: {nbad} of {got.size} differ"
    finally:
        h1.close()


def test_analyze_batch_const_equals_full_frame(weights):
    """the 250 x 300 source of test_gpu_roi_sep.py through the whole pipeline: rows equal with the switch unset, 0 and 1; the pipeline
    runs the form unless the switch is 0"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    imgs = np.stack([odd, odd[::-1]])
    h0 = make_handle(weights, 64, False)
    try:
        rows0 = branches.analyze_batch(h0, imgs, CFG, 300.0)
    finally:
        h0.close()
    visited = {}
    for setting in (None, "0", "1"):
        h1 = make_handle(weights, 64, True, setting)
        try:
            held = None
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, imgs, CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_CONST={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            visited[setting] = h1.debug_sep_tiles()
        finally:
            h1.close()
    print("visited (planned, full) per fused launch:", visited)
    assert visited[None] == visited["1"]
    assert all(a[0] < b[0] and a[1] == b[1] for a, b in zip(visited[None], visited["0"])), "unset visits fewer tiles than TMAT_ROI_CONST=0"
