"""GPU: the shared-interior form of the down path (TMAT_ROI_SHARE) computes what whole patches compute (TMAT_ROI=0).

The patches of an orientation overlap by half a side.  With the form a patch copies, of the stored tensors of the fused levels, what its
right, lower and diagonal neighbours computed of the overlap (tests/test_roi_plan_share.py), and the fused separable layers skip the
tiles that leaves without a needed pixel.  A needed pixel that took an operand nobody wrote or copied shows under the poison patterns
(0xFF: NaN, 0x7F: large finite floats) as a NaN or a bit difference against the full-frame run; so does a copy from the wrong patch,
the frame being random.  320 x 320 has a 3 x 3 grid per orientation (first / middle / last on both axes: right, lower and diagonal
copies all run), 480 x 320 a 4 x 3 grid that the transposed orientations swap, 100 x 90 one patch per orientation and no neighbour."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
# (hh, ww, images per pass, images): the last pass is shorter
CASES = [(320, 320, 3, 7), (480, 320, 3, 4), (100, 90, 3, 4)]
FUSED_LAYERS = (1, 3, 7, 9)


def make_handle(weights, max_patches, roi, share=None, roi_const=None, **env):
    """the switches are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_SHARE": share, "TMAT_ROI_CONST": roi_const, "TMAT_ROI_DOWN": None,
            "TMAT_FUSED_SEP": None, "TMAT_FUSED_POOL": None, "TMAT_STEM_FUSED": None}
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
        rs = np.random.RandomState(700 + hh)
        x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
        h0 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, False)
        try:
            full = h0.predict_smooth(x)
        finally:
            h0.close()
        assert not np.isnan(full).any()
        out[(hh, ww)] = (x, full)
    return out


@pytest.mark.parametrize("hh, ww, per_pass, n", CASES, ids=lambda v: str(v))
def test_predict_smooth_share_equals_full_frame(weights, full_frame, hh, ww, per_pass, n):
    from tmat_amd import _lib
    x, full = full_frame[(hh, ww)]
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1")
    try:
        held = None
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            print(f"{hh} x {ww}, TMAT_ROI_SHARE=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
            k_last = n % per_pass or per_pass
            assert k_last != per_pass, "the last pass has a different size than the first"
            visited = h1.debug_sep_tiles()
            share, live = counts(_lib.roi_sep_tiles_share, hh, ww, k_last), counts(_lib.roi_sep_tiles_live, hh, ww, k_last)
            print(f"  last pass ({k_last} images): visited {visited}, constant-ring form {live}")
            assert visited == share, "the last pass's launches visit the share table's tiles"
            if tiles_per_img(hh, ww) > 8:
                assert all(v[0] < o[0] for v, o in zip(visited, live)), "strictly fewer tiles than the constant-ring form in every fused launch"
            else:
                assert visited == live, "no neighbour: the form falls back to rect_live's tiles"
            if held is None:
                held = h1.debug_held_bytes()
            else:
                assert h1.debug_held_bytes() == held, "held bytes change between calls"
    finally:
        h1.close()


@pytest.mark.parametrize("form", ["TMAT_FUSED_SEP", "TMAT_FUSED_POOL", "TMAT_STEM_FUSED", "TMAT_ROI_DOWN=1", "TMAT_ROI_DOWN=2"])
def test_other_forms_at_320_by_320(weights, full_frame, form):
    """the separate depthwise / pointwise kernels (no fused level: nothing shared), the unfused pooling behind the share table, the stem
    written to memory, and either bit of TMAT_ROI_DOWN alone (without bit 1 there are no tile tables and the form stays off)"""
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    env = {form.split("=")[0]: form.split("=")[1] if "=" in form else "0"}
    h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, "1", "1", **env)
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint64) != full.view(np.uint64)).sum())
            assert not np.isnan(got).any(), f"{form}, pattern {pattern:#x}: NaN"
            assert nbad == 0, f"{form}, pattern {pattern:#x}: {nbad} of {got.size} differ"
    finally:
        h1.close()


def test_predict_smooth_keeps_the_dependency_plan_with_the_switch_unset(weights, full_frame):
    from tmat_amd import _lib
    hh, ww, per_pass, n = CASES[0]
    x, full = full_frame[(hh, ww)]
    k_last = n % per_pass or per_pass
    for share, roi_const, fn in ((None, "1", _lib.roi_sep_tiles_live), (None, None, _lib.roi_sep_tiles), ("1", "0", _lib.roi_sep_tiles)):
        h1 = make_handle(weights, tiles_per_img(hh, ww) * per_pass, True, share, roi_const)
        try:
            h1.debug_poison(0xFF)
            got = h1.predict_smooth(x)
            assert np.array_equal(got.view(np.uint64), full.view(np.uint64)), (share, roi_const)
            assert h1.debug_sep_tiles() == counts(fn, hh, ww, k_last), (share, roi_const)
        finally:
            h1.close()


def test_analyze_batch_share_equals_full_frame(weights):
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
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_SHARE={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            visited[setting] = h1.debug_sep_tiles()
        finally:
            h1.close()
    print("visited (planned, full) per fused launch:", visited)
    assert visited[None] == visited["1"]
    assert all(a[0] < b[0] and a[1] == b[1] for a, b in zip(visited[None], visited["0"])), "unset visits fewer tiles than TMAT_ROI_SHARE=0"


def test_launcher_refusals():
    """host-side argument checks of the share-fill launcher; nothing is launched"""
    from tmat_amd import _lib
    H, C = 80, 64
    nbr = np.full((4, 3), -1, np.int32)
    nbr[0] = (1, 2, 3)
    nbr[1, 1] = 3
    nbr[2, 0] = 3
    ok = [(0, 1, 0, 0, 41, 41, 37), (0, 1, 1, 41, 0, 37, 41), (0, 1, 2, 41, 41, 37, 37), (1, 1, 1, 41, 0, 37, 41), (2, 1, 0, 0, 41, 41, 37)]
    assert _lib.debug_share_fill_check(4, H, C, nbr, ok) is None
    assert _lib.debug_share_fill_check(4, H, C, nbr, []) is None
    for bad, why in (((0, 1, 0, 0, 41, 41, 40), "leaves its tensor"),           # past the right edge
                     ((0, 1, 0, 0, 39, 41, 37), "leaves its tensor"),           # the source starts left of the neighbour
                     ((0, 1, 1, 39, 0, 37, 41), "leaves its tensor"),
                     ((0, 5, 0, 0, 41, 41, 37), "leaves its tensor"),           # more patches than the tensor has
                     ((0, 1, 3, 0, 41, 41, 37), "leaves its tensor"),           # no such direction
                     ((3, 1, 0, 0, 41, 41, 37), "source patch out of range"),   # the last patch has no neighbour
                     ((1, 1, 0, 0, 41, 41, 37), "source patch out of range")):
        msg = _lib.debug_share_fill_check(4, H, C, nbr, [bad])
        assert msg is not None and why in msg, (bad, msg)
    # a copy of a copy: patch 0 takes rows 41 .. 50 from its right neighbour, patch 1, which takes those rows from patch 3 in the same launch
    msg = _lib.debug_share_fill_check(4, H, C, nbr, [(0, 1, 0, 41, 41, 10, 37), (1, 1, 1, 41, 0, 37, 41)])
    assert msg is not None and "overlaps a destination" in msg, msg
    # the same rows from the diagonal neighbour, which copies nothing
    assert _lib.debug_share_fill_check(4, H, C, nbr, [(0, 1, 2, 41, 41, 10, 37), (1, 1, 1, 41, 0, 37, 41)]) is None
    assert _lib.debug_share_fill_check(4, H, 66, nbr, ok) is not None, "channels not a multiple of 4"
