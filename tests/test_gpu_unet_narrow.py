"""GPU parity of the NARROW models -- filter_counts (32, 64, 128, 256), build_UNetXception's own default, and (16, 32, 64, 128), both in the
search of the reference's training notebook -- against the oracle, bit for bit: the patch network in its forms, the smooth tiled
prediction with and without the region forms, poisoned workspaces, the rows of the batch pipeline, and the refusal of the split-precision
modes.  Their 16- and 32-channel convolutions run on conv_narrow_kernel (csrc/conv_narrow_kernels.hip).  The process never imports torch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FCS = [(32, 64, 128, 256), (16, 32, 64, 128)]
IDS = ["32", "16"]
CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)

_cache = {}


def weights_of(fc, kind):
    """structured synthetic weights, or O(1) random ones in every tensor (the recipe of tests/test_gpu_unet.py); made once, read-only"""
    from tmat_amd import synth
    key = ("w", fc, kind)
    if key not in _cache:
        if kind == "synthetic":
            w = synth.synth_weights(0, filter_counts=fc)
        else:
            rs = np.random.RandomState(5)
            w = synth.synth_weights(1, filter_counts=fc)
            for k in w:
                if k.rsplit(".", 1)[-1].startswith("bn"):
                    C = w[k].shape[1]
                    w[k][0] = rs.uniform(0.5, 1.5, C); w[k][1] = rs.normal(0, 0.3, C)
                    w[k][2] = rs.normal(0, 0.3, C); w[k][3] = rs.uniform(0.5, 1.5, C)
                else:
                    fan = int(np.prod(w[k].shape[:-1])) if w[k].ndim > 1 else 1
                    w[k] = rs.normal(0, 1.0 / np.sqrt(max(fan, 1)), w[k].shape).astype(np.float32)
        for a in w.values():
            a.setflags(write=False)
        _cache[key] = w
    return _cache[key]


def patches():
    rs = np.random.RandomState(3)
    x = rs.uniform(0, 1, (3, 320, 320)).astype(np.float32)
    x[1] = 0.0                      # all-zero patch
    x[2, :160] = 1.0                # saturated half
    return x


def patch_ref(fc, kind):
    from oracle import unet as ou
    key = ("patch", fc, kind)
    if key not in _cache:
        _cache[key] = ou.forward_exact(weights_of(fc, kind), patches())
    return _cache[key]


def smooth_image():
    return np.random.RandomState(4).uniform(0, 1, (200, 180)).astype(np.float32)


def smooth_ref(fc):
    from oracle import unet as ou, blend
    key = ("smooth", fc)
    if key not in _cache:
        _cache[key] = blend.predict_img_with_smooth_windowing(smooth_image(), 320, 2, ou.predict_exact(weights_of(fc, "synthetic")))
    return _cache[key]


def make_handle(fc, kind, max_patches):
    from tmat_amd import synth, _lib
    return _lib.Handle(synth.pack_weights(weights_of(fc, kind)), 0, max_patches)


def same_bits(got, ref, what):
    view = np.uint64 if ref.dtype == np.float64 else np.uint32
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nbad = int((got.view(view) != ref.view(view)).sum())
    print(f"{what}: {nbad} of {got.size} outputs differ from the oracle", flush=True)
    assert nbad == 0, f"{what}: {nbad} of {got.size} outputs differ, max |d| = {np.abs(got - ref).max()}"


@pytest.mark.parametrize("kind", ["synthetic", "random"])
@pytest.mark.parametrize("fc", FCS, ids=IDS)
def test_patch_network_bitexact(fc, kind):
    h = make_handle(fc, kind, 8)
    try:
        same_bits(h.unet_predict(patches()), patch_ref(fc, kind), f"{fc} {kind}")
    finally:
        h.close()


@pytest.mark.parametrize("env", [{"TMAT_FUSED_SEP": "0"}, {"TMAT_STEM_FUSED": "0", "TMAT_RELU_COPY": "0", "TMAT_FUSED_POOL": "0"}], ids=["unfused", "plain"])
@pytest.mark.parametrize("kind", ["synthetic", "random"])
@pytest.mark.parametrize("fc", FCS, ids=IDS)
def test_forms_of_the_network_give_the_same_bits(fc, kind, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = make_handle(fc, kind, 8)
    try:
        same_bits(h.unet_predict(patches()), patch_ref(fc, kind), f"{fc} {kind} {env}")
    finally:
        h.close()


@pytest.mark.parametrize("env", [{}, {"TMAT_ROI": "0"}], ids=["region", "full-frame"])
@pytest.mark.parametrize("fc", FCS, ids=IDS)
def test_predict_smooth_bitexact(fc, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = make_handle(fc, "synthetic", 32)
    try:
        same_bits(h.predict_smooth(smooth_image()), smooth_ref(fc), f"{fc} predict_smooth {env}")
    finally:
        h.close()


@pytest.mark.parametrize("fc", FCS, ids=IDS)
def test_poisoned_workspaces(fc):
    """every workspace filled with NaNs before a call: a launch that reads a word no launch of the same call wrote shows"""
    h = make_handle(fc, "synthetic", 32)
    try:
        h.debug_poison(0xFF)
        got = h.unet_predict(patches())
        assert not np.isnan(got).any()
        same_bits(got, patch_ref(fc, "synthetic"), f"{fc} poisoned patches")
        h.debug_poison(0xFF)
        got = h.predict_smooth(smooth_image())
        assert not np.isnan(got).any()
        same_bits(got, smooth_ref(fc), f"{fc} poisoned predict_smooth")
    finally:
        h.close()


@pytest.mark.parametrize("fc,seeds", [(FCS[1], (0, 1)), (FCS[0], (0,))], ids=["16", "32"])
def test_analyze_batch_rows_match_oracle(fc, seeds):
    """the batch pipeline with its default forms (a pass holds whole images: 72 patches each): rows equal to the oracle's, exactly"""
    from oracle import pipeline
    from tmat_amd import branches, synth
    images = np.stack([synth.synth_image(i, 512, n_vessels=12, scale=1.0) for i in seeds])
    w = weights_of(fc, "synthetic")
    want = [pipeline.analyze_image(img, w, CFG, 500.0) for img in images]
    h = make_handle(fc, "synthetic", 144)
    try:
        h.debug_poison(0xFF)            # the forms that copy instead of computing read nothing that this call did not write
        rows = branches.analyze_batch(h, images, CFG, 500.0, first_index=7)
    finally:
        h.close()
    for i, (idx, cnt, tot, avg) in enumerate(rows):
        print(f"{fc} image {seeds[i]}: GPU {cnt} {tot!r} {avg!r}  oracle {want[i]}", flush=True)
        assert idx == 7 + i and cnt > 0
        assert (cnt, tot, avg) == tuple(want[i]), (fc, seeds[i])
    # a small handle (an image needs more patches than it holds: whole patches, one image per pass) gives the same rows
    h = make_handle(fc, "synthetic", 32)
    try:
        assert branches.analyze_batch(h, images[:1], CFG, 500.0, first_index=7) == rows[:1]
    finally:
        h.close()


@pytest.mark.parametrize("fc", FCS, ids=IDS)
def test_split_precision_is_refused(fc):
    from tmat_amd import _lib
    h = make_handle(fc, "synthetic", 8)
    try:
        before = h.unet_predict(patches())
        for mode in ("bf16x3", "bf16x6"):
            with pytest.raises(_lib.TmatError) as e:
                h.set_precision(mode)
            assert f"({_lib.E_ARG})" in str(e.value) and "f32 only" in str(e.value)
        after = h.unet_predict(patches())
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        same_bits(after, patch_ref(fc, "synthetic"), f"{fc} after the refusal")
        h.set_precision("f32")
    finally:
        h.close()


def test_precision_from_the_environment_fails_creation(monkeypatch):
    from tmat_amd import _lib
    monkeypatch.setenv("TMAT_PRECISION", "bf16x3")
    with pytest.raises(_lib.TmatError, match="f32 only"):
        make_handle(FCS[0], "synthetic", 8).close()


def test_blob_no_kernel_takes_is_refused_at_creation():
    from tmat_amd import _lib, synth
    with pytest.raises(_lib.TmatError) as e:
        _lib.Handle(synth.pack_weights(synth.synth_weights(0, filter_counts=(8, 16, 32, 64))), 0, 8).close()
    assert "(-3)" in str(e.value) and "multiple of 16" in str(e.value)


def test_mirror_api_runs_a_narrow_checkpoint():
    """UNetXceptionPatchSegmentor with the filter counts of the checkpoint"""
    from tmat_amd import models, synth
    fc = FCS[0]
    seg = models.UNetXceptionPatchSegmentor(320, synth.pack_weights(weights_of(fc, "synthetic")), list(fc), ds_ratio=0.625, max_patches=32)
    try:
        p = seg.predict(smooth_image(), auto_resample=False)
        assert np.array_equal(p.view(np.uint64), smooth_ref(fc).view(np.uint64))
    finally:
        seg.handle.close()
