"""GPU: what a handle retains between calls (tmat_debug_held_bytes: the workspaces tmat_debug_poison fills).

Call-scoped device memory (csrc/dev_mem.h:DevScope) must be gone when its entry point returns, and a new image geometry must
release EVERY per-pass buffer of the previous one (PassBuf's WsList): a buffer left off a hand-kept free list leaks silently and
shows nowhere else."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)


def _maps():
    """2 probability maps of 48 x 40 with a few thick strokes, 3 DMT fields of 12 x 9"""
    rs = np.random.RandomState(5)
    pred = rs.uniform(0.0, 0.3, (2, 48, 40))
    pred[0, 6:12, 4:36] = 0.9
    pred[0, 10:42, 16:22] = 0.8
    pred[1, 20:27, 3:38] = 0.95
    pred[1, 5:44, 8:13] = 0.7
    pred[1, 30:40, 25:35] = 0.85
    fields = rs.uniform(0, 255, (3, 12, 9)).astype(np.float32)
    return pred, fields


def _round(h, pred, fields):
    """every call-scoped entry point once; all outputs as bytes"""
    from tmat_amd import _lib
    filt, dist = h.filter_edt(pred)
    mask = h.filter_mask(pred > 0.5)
    skel, mdist = h.medial_axis(filt)
    f, f255 = h.finish(pred, dist, skel, (24, 20))
    post = np.empty((2, 24, 20), np.float32)
    _lib.check(_lib.lib().tmat_postprocess_batch(h.raw, _lib.ptr(pred), 2, 48, 40, 24, 20, _lib.ptr(post)), "tmat_postprocess_batch")
    graphs = _lib.dmt_graph_batch(fields, 5.0, 10.0, handle=h)
    out = [filt, dist, mask, skel, mdist, f, f255, post] + [a for g in graphs for a in g]
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_call_scoped_entry_points_retain_nothing():
    """filter_edt, filter_mask, medial_axis, finish, postprocess and dmt_graph_batch twice on a plain handle: held bytes after the
    second round equal those after the first, and the two rounds' outputs are byte-identical"""
    from tmat_amd import _lib
    pred, fields = _maps()
    h = _lib.Handle(None)
    try:
        first = _round(h, pred, fields)
        held1 = h.debug_held_bytes()
        second = _round(h, pred, fields)
        held2 = h.debug_held_bytes()
        print("held after round 1 / 2 (device, pinned):", held1, held2)
        assert held2 == held1
        assert second == first
    finally:
        h.close()


def test_new_geometry_releases_the_old_pass_buffers(weights):
    """patch 64, max_patches 8: two identical analyze_batch calls on 2 images of 128 x 128 hold the same bytes and give the same rows;
    after one call on 128 x 192 the handle holds what a fresh handle that only ever saw 128 x 192 holds -- pinned bytes, and the device
    bytes grown since creation (the pass buffers, and patch_in / patch_out re-made for the larger geometry's patch count on both)"""
    from tmat_amd import _lib, branches, synth
    blob = synth.pack_weights(weights, patch_size=64)
    sq = np.stack([synth.synth_image(50 + i, 128, n_vessels=4, scale=1.0) for i in range(2)])
    wide = np.stack([synth.synth_image(60 + i, 192, n_vessels=4, scale=1.0)[:128] for i in range(2)])
    assert sq.shape == (2, 128, 128) and wide.shape == (2, 128, 192)
    a, b = _lib.Handle(blob, 0, 8), _lib.Handle(blob, 0, 8)
    try:
        fresh_a, fresh_b = a.debug_held_bytes(), b.debug_held_bytes()
        assert fresh_a == fresh_b and fresh_a[1] == 0
        rows1 = branches.analyze_batch(a, sq, CFG, 250.0)
        held1 = a.debug_held_bytes()
        rows2 = branches.analyze_batch(a, sq, CFG, 250.0)
        held2 = a.debug_held_bytes()
        assert held2 == held1 and held1[0] > fresh_a[0] and held1[1] > 0
        assert rows2 == rows1
        rows_a = branches.analyze_batch(a, wide, CFG, 250.0)
        rows_b = branches.analyze_batch(b, wide, CFG, 250.0)
        held_a, held_b = a.debug_held_bytes(), b.debug_held_bytes()
        print("fresh", fresh_a, "square", held1, "square then wide", held_a, "wide only", held_b)
        assert held_a[1] == held_b[1]
        assert held_a[0] - fresh_a[0] == held_b[0] - fresh_b[0]
        assert rows_a == rows_b
    finally:
        a.close()
        b.close()
