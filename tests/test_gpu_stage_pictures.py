"""GPU: the stage pictures (csrc/vis_kernels.hip) -- the kernels against their host twin, and the pictures out of the batched pipeline
(tmat_analyze_batch_ex with stage_out) against the staged evaluation of the same image (branches.stage_pictures_staged), for the plain
form over three passes, on poisoned workspaces, for non-square images, together with the tree and the masks, and through the script."""
import numpy as np
import pytest

from tmat_amd import _lib
from test_stage_pictures_host import CASES

pytestmark = pytest.mark.gpu
CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)
PLANES = _lib.STAGE_PLANES


@pytest.mark.parametrize("name, a", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_host_twin(handle, name, a):
    got = handle.stage_pictures(a)
    want = _lib.host_stage_pictures(a)
    assert got.dtype == np.uint8 and got.shape == a.shape
    assert np.array_equal(got, want), int((got != want).sum())


def test_kernel_equals_host_twin_all_types_at_picture_size(handle):
    """640 x 400 pixels (several workgroups, whole 16-pixel groups only) and 401 x 37 (an odd pixel count: every image of the batch starts
    at another offset inside a 16-pixel group), each as u16, f32, f64 and u8"""
    rs = np.random.RandomState(11)
    for shape in ((3, 400, 640), (5, 401, 37)):
        base = rs.uniform(0, 1, shape)
        for a in ((base * 65535).astype(np.uint16), base.astype(np.float32) * 3 - 1, base * 1e-3, (base > 0.5).astype(np.uint8)):
            got = handle.stage_pictures(a)
            assert np.array_equal(got, _lib.host_stage_pictures(a)), (shape, a.dtype)


@pytest.fixture(scope="module")
def seven():
    from tmat_amd import synth
    imgs = np.stack([synth.synth_image(i, 512, n_vessels=12, scale=1.0) for i in range(7)])       # 72 patches each, 256 per pass: 3 + 3 + 1
    imgs[5] = 1000                       # no branches: the clip branch for `original`, an empty mask and skeleton for `weighted`
    return imgs


@pytest.fixture(scope="module")
def seven_ref(handle, seven):
    """rows of the plain entry and the staged pictures of every image: computed once, shared, left unchanged"""
    from tmat_amd import branches
    rows = branches.analyze_batch(handle, seven, CFG, 500.0)
    staged = np.stack([np.stack(branches.stage_pictures_staged(handle, im)) for im in seven])
    staged.setflags(write=False)
    return rows, staged


def _assert_planes(pics, staged):
    assert pics.shape == staged.shape and pics.dtype == np.uint8
    for i in range(len(staged)):
        for k, plane in enumerate(PLANES):
            assert np.array_equal(pics[i, k], staged[i, k]), (i, plane, int((pics[i, k] != staged[i, k]).sum()))


def test_plain_form_over_three_passes(handle, seven, seven_ref):
    from tmat_amd import branches
    rows0, staged = seven_ref
    rows, ex = branches.analyze_batch_ex(handle, seven, CFG, 500.0, stage_pictures=True)
    assert rows == rows0                                    # bit for bit: tuples of ints and floats
    assert sum(r[1] for r in rows) > 0 and rows[5][1] == 0
    assert set(ex) == {"pictures"} and ex["pictures"].shape == (7, 4, 320, 320)
    _assert_planes(ex["pictures"], staged)
    assert (ex["pictures"][5, 0] == 255).all()              # constant 1000: clip(a, 0, 255)
    assert not ex["pictures"][5, 2].any() and not ex["pictures"][5, 3].any()
    assert ex["pictures"][0, 2].any() and set(np.unique(ex["pictures"][0, 2])) <= {0, 255}
    rows2, ex2 = branches.analyze_batch_ex(handle, seven, CFG, 500.0, stage_pictures=True)
    assert rows2 == rows and np.array_equal(ex2["pictures"], ex["pictures"])
    assert branches.analyze_batch(handle, seven, CFG, 500.0) == rows0           # the plain entry is untouched by the call before it
    rows3, ex3 = branches.analyze_batch_ex(handle, seven, CFG, 500.0)            # no request: the plain rows, nothing else
    assert rows3 == rows0 and ex3 == {}


def test_pictures_on_poisoned_workspaces(handle, seven, seven_ref):
    from tmat_amd import branches
    rows0, staged = seven_ref
    for pattern in (0xFF, 0x00):
        handle.debug_poison(pattern)
        rows, ex = branches.analyze_batch_ex(handle, seven, CFG, 500.0, stage_pictures=True)
        assert rows == rows0
        _assert_planes(ex["pictures"], staged)


def test_non_square_images(handle):
    from tmat_amd import branches, synth
    imgs = np.stack([synth.synth_image(20 + i, 512, n_vessels=12, scale=1.0)[:384] for i in range(4)])     # H x W = 384 x 512
    assert imgs.shape == (4, 384, 512)
    rows, ex = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, stage_pictures=True)
    assert ex["pictures"].shape == (4, 4, 320, 240)         # (round(W r), round(H r)): cv2 reads dsize as (width, height)
    assert rows == branches.analyze_batch(handle, imgs, CFG, 500.0)
    _assert_planes(ex["pictures"], np.stack([np.stack(branches.stage_pictures_staged(handle, im)) for im in imgs]))


def test_unknown_opts_size_is_refused(handle):
    import ctypes as C
    imgs = np.zeros((1, 64, 64), np.uint16)
    rows = (_lib.Row * 1)()
    o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts) - 8, ds_ratio=0.625, ds_width=384)
    assert _lib.lib().tmat_analyze_batch_ex(handle.raw, _lib.ptr(imgs), 1, 64, 64, C.byref(o), rows) == _lib.E_ARG


def test_all_requests_at_once(handle):
    """tree + given well and pruning masks + pictures in one call: rows of the masked entry, pictures of a staged evaluation with the masks
    applied, overlays = the pruned graph's tree over the unmasked u16 down-sampled image"""
    from scipy.ndimage import distance_transform_edt
    from tmat_amd import branches, synth
    from test_gpu_analyze_masked import _given_masks
    imgs = np.stack([synth.synth_image(40 + i, 512, n_vessels=12, scale=1.0) for i in range(4)])
    hw, fshape = (320, 320), branches.dsamp_shape((512, 512))
    well, pruning = _given_masks(4, hw, fshape)
    rows0 = branches.analyze_batch_masked(handle, imgs, CFG, 500.0, well_masks=well, pruning_masks=pruning)
    rows, ex = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, well_masks=well, pruning_masks=pruning, tree=True, vis_width=500,
                                         stage_pictures=True)
    assert rows == rows0 and sum(r[1] for r in rows) > 0
    assert set(ex) == {"pictures", "overlays", "bars"} and ex["overlays"].shape == (4, 500, 500, 3)
    L = _lib.lib()
    x = np.empty((4,) + hw, np.float32)
    _lib.check(L.tmat_preprocess_batch(handle.raw, _lib.ptr(imgs), 4, 512, 512, 0.625, _lib.ptr(x)), "tmat_preprocess_batch")
    pred = handle.predict_smooth(x * well)                                  # compute_branches.py:328
    filt = handle.filter_mask((pred > 0.5) & well)                          # :334-337
    skel, dist = handle.medial_axis(filt)
    _, f255 = handle.finish(pred, dist, skel, fshape)
    for i in range(4):
        cdt = distance_transform_edt(np.logical_not(skel[i]))
        with np.errstate(invalid="ignore", divide="ignore"):
            weighted = pred[i] * (dist[i] / (dist[i] + cdt))
        bg = _lib.host_lanczos4_u16(imgs[i], hw)
        want = [branches.save_vis_u8(a) for a in (bg, pred[i], filt[i].astype(np.float64), weighted)]
        for k, plane in enumerate(PLANES):
            assert np.array_equal(ex["pictures"][i, k], want[k]), (i, plane, int((ex["pictures"][i, k] != want[k]).sum()))
        tree, bars, (cnt, tot, avg) = branches.field_tree(handle, f255[i], CFG, 500.0, (5.0, 10.0), pruning[i], hw[1] / fshape[1])
        assert (cnt, tot, avg) == rows[i][1:] and len(ex["bars"][i]) == cnt
        assert np.array_equal(ex["bars"][i], bars)
        assert np.array_equal(ex["overlays"][i], _lib.host_render_tree(bg, [tree], 500)[0]), i


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


FILES = ("original_image.png", "prediction.png", "segmentation_mask.png", "distance_transform.png")


def test_script_visualizations_from_the_batched_call(tmp_path, handle):
    """--visualizations: the four PNGs of each image decode to the staged arrays; a 2 x 2 threshold grid still writes each picture once"""
    from tmat_amd import branches, synth
    from test_gpu_script import run
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    imgs = {f"p_{i}": synth.synth_image(60 + i, 512, n_vessels=12, scale=1.0) for i in range(2)}
    for k, v in imgs.items():
        np.save(ind / f"{k}.npy", v)
    r = run([str(ind), str(outd), "--image-width-microns", "500", "--visualizations", "--graph-thresh-1", "2", "5", "--graph-thresh-2", "4", "10"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(list(outd.glob("branching_analysis_CONFIG*.csv"))) == 4
    for k, img in imgs.items():
        vdir = outd / "visualizations" / k
        assert sorted(p.name for p in vdir.iterdir()) == sorted(FILES)
        for name, want in zip(FILES, branches.stage_pictures_staged(handle, img)):
            assert np.array_equal(_png(vdir / name), want), (k, name)


def test_script_detect_well_visualizations(tmp_path, handle):
    """-w --visualizations adds well_mask.png = save_vis(well * 255); the CSV is the one of a run without --visualizations.  Image 3's
    mask is dropped (all ones: the clip branch, a picture of 255s), image 5 has a real well (tests/test_gpu_wellmask.py pins both)."""
    from tmat_amd import branches
    from test_gpu_script import run
    from test_gpu_wellmask import _well_image
    ind = tmp_path / "in"
    ind.mkdir()
    imgs = {"w_3": _well_image(3), "w_5": _well_image(5)}
    for k, im in imgs.items():
        np.save(ind / f"{k}.npy", im)
    base = ["--image-width-microns", "500", "-w", "--well-seed", "7"]
    r0 = run([str(ind), str(tmp_path / "plain")] + base)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = run([str(ind), str(tmp_path / "vis")] + base + ["--visualizations"])
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert (tmp_path / "vis" / "branching_analysis.csv").read_bytes() == (tmp_path / "plain" / "branching_analysis.csv").read_bytes()
    assert not (tmp_path / "plain" / "visualizations").exists()
    fields = branches.well_fields(handle, np.stack([imgs["w_3"], imgs["w_5"]]), 0.625, 16, 7, warn=lambda m: None)
    for i, k in enumerate(("w_3", "w_5")):
        vdir = tmp_path / "vis" / "visualizations" / k
        assert sorted(p.name for p in vdir.iterdir()) == sorted(FILES + ("well_mask.png",))
        wm, well = _png(vdir / "well_mask.png"), fields[i][2]
        assert np.array_equal(wm, branches.save_vis_u8(well * 255)), k
        seg, pred = _png(vdir / "segmentation_mask.png"), _png(vdir / "prediction.png")
        assert wm.shape == seg.shape == pred.shape
        assert not seg[wm == 0].any()                                   # the mask picture is the filtered seg * well (:334-337)
    assert (wm == 0).any() and (wm == 255).any()                        # image 5: a real well


def test_script_z_stack_visualizations(tmp_path):
    """the two pictures of a Z-stack run are save_stack_visualizations' pixel arrays"""
    from PIL import Image
    from tmat_amd import branches, synth
    from test_gpu_script import run
    ind, outd, refd = tmp_path / "in", tmp_path / "out", tmp_path / "ref"
    ind.mkdir()
    st = synth.synth_stack(1, 4, 200, 256, n_vessels=8)
    for z, sl in enumerate(st):
        Image.fromarray(sl).save(ind / f"wellA_z{z}.tif")
    r = run([str(ind), str(outd), "--image-width-microns", "800", "--visualizations", "--graph-thresh-1", "2", "5"])
    assert r.returncode == 0, r.stdout + r.stderr
    vdir = outd / "visualizations" / "wellA"
    assert sorted(p.name for p in vdir.iterdir()) == ["original_image.png", "vesselness_image.png"]
    plain = _lib.Handle(None, 0)
    try:
        branches.save_stack_visualizations(plain, st, refd)
    finally:
        plain.close()
    for name in ("original_image.png", "vesselness_image.png"):
        assert np.array_equal(_png(vdir / name), _png(refd / name)), name
