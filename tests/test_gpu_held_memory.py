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


def _tool_inputs():
    """the smallest inputs the tool entry points accept that still take every branch of their staging"""
    rs = np.random.RandomState(11)
    well = rs.uniform(0.0, 0.2, (24, 20)).astype(np.float32)
    well[5:19, 4:16] += 0.6                                              # a bright well on a dark plate
    mask = np.zeros((24, 20), np.uint8)
    mask[6:18, 5:15] = 1
    cells = rs.randint(200, 900, (2, 32, 32)).astype(np.uint16)
    cells[:, 8:20, 10:26] += rs.randint(3000, 9000, (2, 12, 16)).astype(np.uint16)
    cmask = np.zeros((2, 32, 32), np.uint8)
    cmask[:, 4:28, 3:29] = 1
    return dict(g2=rs.uniform(0, 1, (24, 20)).astype(np.float32), g3=rs.uniform(0, 1, (3, 24, 20)).astype(np.float32), well=well, mask=mask,
                masks=np.stack([mask, 1 - mask]), stacks=rs.randint(0, 65536, (2, 3, 16, 16)).astype(np.uint16),
                x=rs.uniform(-1, 1, (1, 8, 8, 64)).astype(np.float32), w=(rs.uniform(-1, 1, (3, 3, 64, 64)) / 24).astype(np.float32),
                scale=rs.uniform(0.5, 1.5, 64).astype(np.float32), shift=rs.uniform(-0.1, 0.1, 64).astype(np.float32),
                resid=rs.uniform(-1, 1, (1, 8, 8, 64)).astype(np.float32), cells=cells, cmask=cmask)


SE_PARAMS = [(0.11, 0.81, 1.04, 0.93, 0.17, -0.12), (-0.14, 0.7, 0.95, 1.08, -0.21, 0.09), (0.0, 1.3, 1.1, 1.1, 0.0, 0.0)]


def _tool_round(h, t):
    """the converted entry points _round does not reach, once each; all outputs as bytes"""
    from tmat_amd import _lib, preprocessing, sato
    from tmat_amd import well_mask_generation as wm
    out = [sato.gaussian(h, t["g2"]), sato.gaussian(h, t["g3"])]                                   # two and three passes
    out += [wm.auto_threshold_well(t["well"], h), wm.auto_threshold_well(t["well"].astype(np.float64), h), wm._border(h, t["mask"])]
    out += [wm.resize_nearest_dev(h, t["masks"], (12, 10))]
    out += [h.zproj(t["stacks"], "fs"), h.zproj(t["stacks"], "avg")]                               # u16 and f64 output
    out += [h.conv2d(t["x"], t["w"], t["scale"], t["shift"], resid=t["resid"], relu_out=True, prec=p) for p in (0, 3, 4)]
    masks, band = wm.gen_superellipse_masks_dev(h, SE_PARAMS, [2] * 3, (7, 5), return_band=True)
    out += [masks, band]
    # a superellipse through grid points of the 5-point linspace: four undecided pixels, so the band comes back as well
    out += list(wm.gen_superellipse_masks_dev(h, [(0.0, 0.5, 1.0, 1.0, 0.0, 0.0)], [8], (5, 5), return_band=True))
    out += list(preprocessing.cell_area_batch(h, t["cells"], 16, 0.0, return_params=True))         # resized, thresholded and params
    area, thr, par = np.empty(2, np.float64), np.empty((2, 32, 32), np.uint8), np.empty((2, 9), np.float64)
    _lib.check(_lib.lib().tmat_cell_area_masked(h.raw, _lib.ptr(t["cells"]), _lib.ptr(t["cmask"]), 2, 32, 32, 0.0, _lib.ptr(area), _lib.ptr(thr),
                                                _lib.ptr(par)), "tmat_cell_area_masked")          # the host-built init table
    out += [area, thr, par]
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_tool_entry_points_retain_nothing():
    """gaussian, well threshold (f32 / f64), canny, nearest resize, Z projection, conv2d (prec 0 / 3 / 4), superellipse masks and cell
    area (plain and masked) twice on a plain handle: held bytes after the second round equal those after the first, and the two rounds'
    outputs are byte-identical"""
    from tmat_amd import _lib
    t = _tool_inputs()
    h = _lib.Handle(None)
    try:
        first = _tool_round(h, t)
        held1 = h.debug_held_bytes()
        second = _tool_round(h, t)
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
