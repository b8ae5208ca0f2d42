"""GPU: the stages of csrc/morph_kernels.hip one by one (tmat_debug_filter_stages: median, labels, per-label area / perimeter codes,
Zhang skeleton, launches used, filtered mask) and the EDT, against scipy.ndimage and oracle/morph.py.  Every comparison is exact
and covers every pixel.  Inputs and references: tests/helpers/morph_cases.py, whose own properties tests/test_morph_cases.py pins
(which inputs wake sleeping tiles of zhang_tile_kernel, which shapes leave a partial wave to the ballots of ccl_init_kernel and
region_stats_kernel, ...)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import morph_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("median", "labels", "stats", "skeleton", "filtered", "thin_launches")


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


_REFS = {}


def refs_of(key, named_masks):
    """references of a list of (name, mask) of one shape, computed once per module: labels, stats, skeleton, removing launches"""
    if key not in _REFS:
        from oracle import morph
        names = [k for k, _ in named_masks]
        masks = np.stack([m for _, m in named_masks])
        _REFS[key] = dict(names=names, masks=masks, labels=np.stack([mc.ref_labels(m) for m in masks]),
                          stats=np.stack([mc.ref_stats(m) for m in masks]),
                          skeleton=np.stack([morph.skeletonize_zhang(m) for m in masks]),
                          launches=np.array([len(mc.launch_trace(m)) - 1 for m in masks], np.int32))
    return _REFS[key]


_GOT = {}


def stages_of(plain, key, named_masks):
    """(references, the device's stages) of the masks as ONE batch with use_median 0, run once per module"""
    ref = refs_of(key, named_masks)
    if key not in _GOT:
        _GOT[key] = plain.debug_filter_stages(ref["masks"], use_median=False, remove_isolated=True)
    return ref, _GOT[key]


def assert_images_equal(got, want, names, what):
    """exact, every pixel; names the images that differ and the first differing pixel"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = [(names[i], int((got[i] != want[i]).sum()), tuple(int(v) for v in np.argwhere(got[i] != want[i])[0]))
           for i in range(len(names)) if not np.array_equal(got[i], want[i])]
    assert not bad, (what, bad)


def mixed_batch():
    return [("stair240", mc.stair(240)), ("empty", np.zeros((240, 240), bool)), ("full240", mc.full(240, 240)),
            ("noise45", mc.noise(240, 240, 0.45, 7))]


def triple_batch():
    return [("noise35", mc.noise(37, 127, 0.35, 11)), ("checker", mc.checker(37, 127)), ("runs64", mc.runs64(37, 127))]


SHAPE_IDS = [f"{h}x{w}" for h, w in mc.SHAPES]


# ---- labels and per-label statistics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES, ids=SHAPE_IDS)
def test_labels_are_component_roots(plain, shape):
    ref, got = stages_of(plain, shape, mc.cases(*shape))
    assert_images_equal(got["median"], ref["masks"], ref["names"], "median (use_median 0: the mask itself)")
    assert_images_equal(got["labels"], ref["labels"], ref["names"], "labels")


@pytest.mark.parametrize("shape", mc.SHAPES, ids=SHAPE_IDS)
def test_area_and_perimeter_codes_per_root(plain, shape):
    ref, got = stages_of(plain, shape, mc.cases(*shape))
    assert_images_equal(got["stats"], ref["stats"], ref["names"], "stats (area, n1, n2, n3)")


def test_labels_and_stats_of_a_batch_whose_image_base_is_no_multiple_of_64(plain):
    assert (37 * 127) % 64
    ref, got = stages_of(plain, "triple", triple_batch())
    assert_images_equal(got["labels"], ref["labels"], ref["names"], "labels")
    assert_images_equal(got["stats"], ref["stats"], ref["names"], "stats")
    assert_images_equal(got["skeleton"], ref["skeleton"], ref["names"], "skeleton")
    assert got["thin_launches"].tolist() == ref["launches"].tolist(), ref["names"]


# ---- Zhang skeleton, sleeping tiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES, ids=SHAPE_IDS)
def test_skeleton_and_launch_count(plain, shape):
    ref, got = stages_of(plain, shape, mc.cases(*shape))
    assert_images_equal(got["skeleton"], ref["skeleton"], ref["names"], "skeleton")
    assert got["thin_launches"].tolist() == ref["launches"].tolist(), ref["names"]


@pytest.mark.parametrize("name", [k for k, _ in mc.solid_cases()])
def test_solid_inputs_skeleton_launches_and_repeat(plain, name):
    """the wake-up inputs (tiles sleep while the fronts are far, and must run again when they arrive) and the other solid shapes,
    one image per call; the same call again on the same handle gives the same bytes (per-tile flags of a pooled workspace)"""
    m = dict(mc.solid_cases())[name]
    ref, got = stages_of(plain, name, [(name, m)])
    assert_images_equal(got["skeleton"], ref["skeleton"], ref["names"], "skeleton")
    assert got["thin_launches"].tolist() == ref["launches"].tolist()
    assert_images_equal(got["labels"], ref["labels"], ref["names"], "labels")
    assert_images_equal(got["stats"], ref["stats"], ref["names"], "stats")
    again = plain.debug_filter_stages(ref["masks"], use_median=False, remove_isolated=True)
    for k in KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_mixed_batch_of_wake_up_empty_full_and_noise(plain):
    """per-image flags stay separate: one image converges at once, two need 30 launches with waking tiles, one a few"""
    ref, got = stages_of(plain, "mixed", mixed_batch())
    assert_images_equal(got["skeleton"], ref["skeleton"], ref["names"], "skeleton")
    assert got["thin_launches"].tolist() == ref["launches"].tolist()
    assert_images_equal(got["labels"], ref["labels"], ref["names"], "labels")
    assert_images_equal(got["stats"], ref["stats"], ref["names"], "stats")
    again = plain.debug_filter_stages(ref["masks"], use_median=False, remove_isolated=True)
    for k in KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_largest_frame_twice_on_one_handle(plain):
    ref, got = stages_of(plain, (513, 513), mc.cases(513, 513))
    again = plain.debug_filter_stages(ref["masks"], use_median=False, remove_isolated=True)
    for k in KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k


# ---- the whole filter --------------------------------------------------------------------------------------------------------
def filter_inputs():
    """(513, 513) noise, blobs and the disc pairs.  noise35 is the one with some ten thousand separate roots for the decision and
    drop kernels, on both trips of their grid-stride loops; noise45 and noise60 are one giant component each."""
    c = dict(mc.cases(513, 513))
    return [(k, c[k]) for k in ("noise35", "noise45", "noise60", "blobs", "discs_gap", "discs_diag")]


@pytest.mark.parametrize("use_median,remove_isolated", [(True, True), (False, True), (True, False), (False, False)])
def test_filtered_mask_matches_oracle_for_every_option_pair(plain, use_median, remove_isolated):
    from oracle import morph
    names = [k for k, _ in filter_inputs()]
    masks = np.stack([m for _, m in filter_inputs()])
    got = plain.debug_filter_stages(masks, use_median, remove_isolated)
    med = np.stack([morph.median13(m) if use_median else m for m in masks])
    assert_images_equal(got["median"], med, names, "median")
    want = np.stack([morph.filter_branch_seg_mask(m, use_median, remove_isolated) for m in masks])
    assert_images_equal(got["filtered"], want, names, "filtered")
    assert plain.filter_mask(masks, use_median, remove_isolated).astype(np.uint8).tobytes() == got["filtered"].tobytes()


@pytest.mark.parametrize("shape", mc.SHAPES[:7], ids=SHAPE_IDS[:7])
def test_median_and_what_follows_it_at_tiny_shapes(plain, shape):
    """frames smaller than the 5 x 5 footprint: every tap is clamped ('nearest')"""
    from oracle import morph
    names = [k for k, _ in mc.cases(*shape)]
    masks = np.stack([m for _, m in mc.cases(*shape)])
    got = plain.debug_filter_stages(masks, use_median=True, remove_isolated=True)
    med = np.stack([morph.median13(m) for m in masks])
    assert_images_equal(got["median"], med, names, "median")
    assert_images_equal(got["labels"], np.stack([mc.ref_labels(m) for m in med]), names, "labels")
    assert_images_equal(got["stats"], np.stack([mc.ref_stats(m) for m in med]), names, "stats")
    assert_images_equal(got["skeleton"], np.stack([morph.skeletonize_zhang(m) for m in med]), names, "skeleton")
    assert_images_equal(got["filtered"], np.stack([morph.filter_branch_seg_mask(m, True, True) for m in masks]), names, "filtered")
    assert plain.filter_mask(masks, True, True).astype(np.uint8).tobytes() == got["filtered"].tobytes()


@pytest.mark.parametrize("shape", mc.SHAPES[:10], ids=SHAPE_IDS[:10])
def test_filtered_mask_without_median_at_every_small_shape(plain, shape):
    from oracle import morph
    ref, got = stages_of(plain, shape, mc.cases(*shape))
    want = np.stack([morph.filter_branch_seg_mask(m, False, True) for m in ref["masks"]])
    assert_images_equal(got["filtered"], want, ref["names"], "filtered")
    assert plain.filter_mask(ref["masks"], False, True).astype(np.uint8).tobytes() == got["filtered"].tobytes()


# ---- EDT ---------------------------------------------------------------------------------------------------------------------
def one_zero(shape, at):
    m = np.ones(shape, bool)
    m[at] = False
    return m


def check_medial_axis(plain, masks):
    from oracle import morph
    from tmat_amd import _lib
    m8 = np.ascontiguousarray(masks, np.uint8)
    skel = np.full(m8.shape, 0xA5, np.uint8)
    dist = np.full(m8.shape, -7.0, np.float64)
    rc = _lib.lib().tmat_medial_axis_batch(plain.raw, _lib.ptr(m8), *m8.shape, _lib.ptr(skel), _lib.ptr(dist))
    assert rc == 0, _lib.lib().tmat_last_error()          # the library takes every shape used here, one-pixel-wide frames included
    for i, m in enumerate(masks):
        want = ndi.distance_transform_edt(m)
        assert np.array_equal(dist[i].view(np.uint64), want.view(np.uint64)), i
        osk, odist = morph.medial_axis(m)
        assert np.array_equal(dist[i], odist), i
        assert np.array_equal(skel[i].astype(bool), osk), i


def test_edt_with_a_single_zero_pixel_in_a_wide_frame(plain):
    """distances up to the frame's diagonal: the row pass scans the whole row, the column pass carries a long ramp"""
    shape = (130, 300)
    check_medial_axis(plain, np.stack([one_zero(shape, (0, 0)), one_zero(shape, (129, 299)), one_zero(shape, (65, 150))]))


@pytest.mark.parametrize("shape,at", [((1, 70), (0, 13)), ((70, 1), (41, 0))])
def test_edt_of_one_pixel_wide_frames(plain, shape, at):
    check_medial_axis(plain, one_zero(shape, at)[None])


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_behave_as_filter_mask_batch(plain):
    from tmat_amd import _lib
    L = _lib.lib()
    m = np.ones((2, 5, 7), np.uint8)
    out = {k: np.full(s, 0x5A, d) for k, s, d in (("median", m.shape, np.uint8), ("labels", m.shape, np.int32), ("stats", (2, 4, 5, 7), np.int32),
                                                   ("skeleton", m.shape, np.uint8), ("filtered", m.shape, np.uint8), ("thin_launches", (2,), np.int32))}
    ptrs = [_lib.ptr(out[k]) for k in KEYS]
    filt = np.full(m.shape, 0x5A, np.uint8)

    def both(h, mask, n, hh, ww):
        return (L.tmat_debug_filter_stages(h, mask, n, hh, ww, 0, 1, *ptrs), L.tmat_filter_mask_batch(h, mask, n, hh, ww, 0, 1, _lib.ptr(filt)))

    assert both(None, _lib.ptr(m), 2, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, None, 2, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), 2, 0, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), -1, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), 0, 5, 7) == (0, 0)                        # nothing to do, nothing written
    assert all((v == 0x5A).all() for v in out.values()) and (filt == 0x5A).all()
    # no output at all: refused like tmat_filter_mask_batch without its `filtered`
    none = [C.c_void_p()] * 6
    assert L.tmat_debug_filter_stages(plain.raw, _lib.ptr(m), 2, 5, 7, 0, 1, *none) == _lib.E_ARG
    assert L.tmat_filter_mask_batch(plain.raw, _lib.ptr(m), 2, 5, 7, 0, 1, None) == _lib.E_ARG
    assert b"bad argument" in L.tmat_last_error()
    # every single output alone is enough, and gives what the full call gives
    full = plain.debug_filter_stages(m, False, True)
    for j, k in enumerate(KEYS):
        one = np.full(out[k].shape, 0x5A, out[k].dtype)
        args = [C.c_void_p()] * 6
        args[j] = _lib.ptr(one)
        assert L.tmat_debug_filter_stages(plain.raw, _lib.ptr(m), 2, 5, 7, 0, 1, *args) == 0, k
        assert one.tobytes() == full[k].tobytes(), k
