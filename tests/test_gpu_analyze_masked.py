"""GPU: the --detect-well form of the 2-D branch through the batch pipeline (tmat_analyze_batch_masked, branches.analyze_batch_well)
against the staged entry points the form used before (the body of branches.well_fields + well_rows), rows compared with ==."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SCRIPT = REPO / "tissue-model-analysis-tools_amd" / "scripts" / "compute_branches.py"
CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)


def _staged_rows(handle, imgs, well, pruning, ds_ratio=0.625, thresh=(5.0, 10.0)):
    """well_fields + well_rows with GIVEN masks: predict_smooth(x * well), filter_mask((pred > 0.5) & well), medial_axis, finish,
    dmt_graph, morse_stats with the pruning mask"""
    from tmat_amd import _lib, branches
    imgs = np.ascontiguousarray(imgs, np.uint16)
    n, H, W = imgs.shape
    hh, ww = int(round(W * ds_ratio)), int(round(H * ds_ratio))
    L = _lib.lib()
    x = np.empty((n, hh, ww), np.float32)
    _lib.check(L.tmat_set_input_depth(handle.raw, 16), "tmat_set_input_depth")
    _lib.check(L.tmat_preprocess_batch(handle.raw, _lib.ptr(imgs), n, H, W, float(ds_ratio), _lib.ptr(x)), "tmat_preprocess_batch")
    pred = handle.predict_smooth(x * well)
    filt = handle.filter_mask((pred > 0.5) & well)
    skel, dist = handle.medial_axis(filt)
    fshape = branches.dsamp_shape((H, W))
    _, f255 = handle.finish(pred, dist, skel, fshape)
    return branches.well_rows(handle, [(f255[i], pruning[i], well[i]) for i in range(n)], CFG, 500.0, thresh)


def _given_masks(n_img, hw, fshape):
    """superellipse wells covering roughly 60 % of the (h, w) image, a little different per image; images 2 and 9 all ones, image 5
    all zeros; pruning masks = the complement of the 10 % smaller superellipse at the field shape"""
    from tmat_amd import well_mask_generation as wm
    well, pruning = np.ones((n_img,) + hw, bool), np.zeros((n_img,) + fshape, bool)
    for i in range(n_img):
        if i in (2, 9):
            continue
        if i == 5:
            well[i] = False
            pruning[i] = True
            continue
        n = 2 if i % 2 else 8
        p = (0.02 * (i % 5) - 0.04, (0.9 if n == 2 else 0.8) + 0.01 * (i % 3), 1.0, 0.95, 0.03 * (i % 4) - 0.05, 0.02 * (i % 3), n)
        well[i] = wm.gen_superellipse_mask(*p, hw)
        shrunk = wm.gen_superellipse_mask(p[0], p[1] * 0.9, *p[2:], hw)
        pruning[i] = wm._resize_nearest(np.logical_not(shrunk), fshape)
    return well, pruning


@pytest.fixture(scope="module")
def images():
    from tmat_amd import synth
    # Two to four vessels per image: sparse enough for filter_branch_seg_mask to keep them (ten merge into one blob, which it drops).
    # 256^2 images are smaller than a patch and most keep nothing; the generator settings below are those of a sweep that leave a
    # branch in images 0, 1, 2, 6, 9 and 15 without masks.
    other = {1: (2, 1.0), 2: (3, 0.5), 6: (4, 1.0), 9: (2, 1.0), 15: (3, 0.5)}
    return np.stack([synth.synth_image(200 + i, 256, n_vessels=other.get(i, (3, 1.0))[0], scale=other.get(i, (3, 1.0))[1]) for i in range(17)])


@pytest.fixture(scope="module")
def unmasked_rows(handle, images):
    from tmat_amd import branches
    return branches.analyze_batch(handle, images, CFG, 500.0)


def test_masked_batch_rows_equal_the_staged_entry_points(handle, images, unmasked_rows):
    """17 images of 256^2 = 32 patches each on the 256-patch handle: passes of 8, 8 and 1 images"""
    from tmat_amd import branches
    well, pruning = _given_masks(17, (160, 160), (384, 384))
    cover = [w.mean() for i, w in enumerate(well) if i not in (2, 5, 9)]
    assert 0.5 < min(cover) and max(cover) < 0.75
    want = _staged_rows(handle, images, well, pruning)
    got = branches.analyze_batch_masked(handle, images, CFG, 500.0, well_masks=well, pruning_masks=pruning, first_index=0)
    print("masked", got, "\nstaged", want, "\nunmasked", unmasked_rows)
    assert got == want
    assert sum(r[1] for r in got) > 0
    assert got[5][1] == 0, "an all-zero well leaves nothing to trace"
    assert any(g != u for g, u in zip(got, unmasked_rows)), "the masks must change at least one row"
    # each mask alone, against the same staged functions
    ones, none = np.ones_like(well), np.zeros_like(pruning)
    assert branches.analyze_batch_masked(handle, images, CFG, 500.0, well_masks=well) == _staged_rows(handle, images, well, none)
    assert branches.analyze_batch_masked(handle, images, CFG, 500.0, pruning_masks=pruning) == _staged_rows(handle, images, ones, pruning)


def test_without_masks_the_rows_are_those_of_analyze_batch(handle, images, unmasked_rows):
    from tmat_amd import branches
    assert branches.analyze_batch_masked(handle, images, CFG, 500.0) == unmasked_rows
    assert branches.analyze_batch_masked(handle, images, CFG, 500.0, first_index=40) == [(r[0] + 40,) + r[1:] for r in unmasked_rows]
    well, pruning = np.ones((17, 160, 160), bool), np.zeros((17, 384, 384), bool)
    assert branches.analyze_batch_masked(handle, images, CFG, 500.0, well_masks=well, pruning_masks=pruning) == unmasked_rows


def test_non_square_images_take_masks_of_the_transposed_shape(handle):
    """a 256 x 320 image is down-sampled to (round(W r), round(H r)) = (200, 160) (cv2 reads dsize as (width, height)); the field is
    (307, 384).  Masks of those shapes are used; the untransposed ones are refused by the wrapper"""
    from tmat_amd import branches, synth
    imgs = np.stack([synth.synth_image(i, 320, n_vessels=3, scale=1.0)[:256] for i in (205, 211)])
    assert branches.dsamp_shape(imgs.shape[1:]) == (307, 384)
    well, pruning = _given_masks(2, (200, 160), (307, 384))
    got = branches.analyze_batch_masked(handle, imgs, CFG, 500.0, well_masks=well, pruning_masks=pruning)
    print("non-square", got)
    assert got == _staged_rows(handle, imgs, well, pruning)
    with pytest.raises(ValueError):
        branches.analyze_batch_masked(handle, imgs, CFG, 500.0, well_masks=np.ones((2, 160, 200), bool))
    with pytest.raises(ValueError):
        branches.analyze_batch_masked(handle, imgs, CFG, 500.0, pruning_masks=np.zeros((2, 384, 307), bool))
    with pytest.raises(ValueError):
        branches.analyze_batch_masked(handle, imgs, CFG, 500.0, well_masks=well[:1])


def _well_image(seed, size=512):
    """a synthetic projection whose vessels sit inside a bright round well (the generator of tests/test_gpu_wellmask.py)"""
    from tmat_amd import synth
    img = synth.synth_image(seed, size, n_vessels=12, scale=1.0).astype(np.float64)
    yy, xx = np.mgrid[0:size, 0:size]
    inside = (xx - size * 0.52) ** 2 + (yy - size * 0.49) ** 2 < (size * 0.42) ** 2
    img = np.where(inside, img + 12000.0, 0.0)
    return np.clip(img, 0, 65535).astype(np.uint16)


@pytest.fixture(scope="module")
def well_pair(handle):
    """the two images of test_branch_rows_with_detect_well_equal_the_oracle with the staged path's fields and rows (seed 7)"""
    from tmat_amd import branches
    imgs = np.stack([_well_image(3), _well_image(5)])
    fields = branches.well_fields(handle, imgs, 0.625, 16, well_seed=7, warn=lambda m: None)
    return imgs, fields, branches.well_rows(handle, fields, CFG, 500.0, (5.0, 10.0))


def test_analyze_batch_well_equals_the_staged_path_end_to_end(handle, well_pair):
    from tmat_amd import branches
    imgs, fields, want = well_pair
    warned = []
    rows, well, pruning = branches.analyze_batch_well(handle, imgs, CFG, 500.0, 0.625, (5.0, 10.0), 0, 16, 7, warned.append)
    assert rows == want and sum(r[1] for r in rows) > 0
    for i in range(2):
        assert np.array_equal(well[i], fields[i][2]) and np.array_equal(pruning[i], fields[i][1]), i
    # image 3: coverage below 40 % -> the mask is dropped with the warning; image 5: a real well
    assert well[0].all() and not pruning[0].any() and len(warned) == 1 and "coverage is too low" in warned[0]
    assert 0.4 < well[1].mean() < 0.95 and pruning[1].any()
    # the masks of one call serve the next threshold configuration
    again, _, _ = branches.analyze_batch_well(handle, imgs, CFG, 500.0, 0.625, (2.0, 5.0), masks=(well, pruning))
    assert again == branches.well_rows(handle, fields, CFG, 500.0, (2.0, 5.0))


def test_script_detect_well_writes_the_staged_csv(tmp_path, well_pair):
    """compute_branches.py IN OUT -w --well-seed 7: the CSV bytes the staged functions' rows give"""
    import csv
    import io
    from tmat_amd import branches
    imgs, _, want = well_pair
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    ids = ["w_3", "w_5"]
    for k, im in zip(ids, imgs):
        np.save(ind / f"{k}.npy", im)
    r = subprocess.run([sys.executable, str(SCRIPT), str(ind), str(outd), "--image-width-microns", "500", "-w", "--well-seed", "7"],
                       capture_output=True, text=True, env=dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1"), timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator="\n")
    wr.writerow(["Image", "Total # of branches", "Total branch length (µm)", "Average branch length (µm)"])
    for k, row in zip(ids, want):
        wr.writerow([k, row[1], branches.pixels_to_microns(row[2], 384, 500.0), branches.pixels_to_microns(row[3], 384, 500.0)])
    assert (outd / "branching_analysis.csv").read_bytes() == buf.getvalue().encode("utf-16")
