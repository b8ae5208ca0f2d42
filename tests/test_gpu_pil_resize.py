"""GPU: the device resize of float32 images in Pillow's arithmetic (csrc/pil_resize_kernels.hip) against its host twin, and
UNetXceptionPatchSegmentor.predict(x) with the default auto_resample -- one device chain, tmat_predict_auto_resample -- against the
host chain it replaces: Pillow LANCZOS -> norm -> smooth prediction -> Pillow NEAREST.  The process never imports torch."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import pil_resize_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = pr.cases()


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


@pytest.mark.parametrize("key, shape, tgt, flt", CASES, ids=[c[0] for c in CASES])
def test_device_resize_equals_the_host_twin(plain, key, shape, tgt, flt):
    from tmat_amd import _lib
    x = pr.case_input(shape)
    got = plain.resize_pil_f32(x, tgt, flt)
    ref = _lib.host_resize_pil_f32(x, tgt, flt)
    assert got.shape == ref.shape == tgt and got.dtype == np.float32
    nbad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert nbad == 0, f"{key}: {nbad} of {got.size} pixels differ"


def test_device_resize_batch_and_poisoned_workspaces(plain):
    from tmat_amd import _lib
    x = np.stack([pr.case_input((75, 130)), pr.case_input((75, 130))[::-1], pr.case_input((75, 130))[:, ::-1]])
    for flt in pr.FILTERS:
        _lib.check(_lib.lib().tmat_debug_poison(plain.raw, 0xFF), "poison")
        got = plain.resize_pil_f32(x, (65, 47), flt)
        assert np.array_equal(got.view(np.uint32), _lib.host_resize_pil_f32(x, (65, 47), flt).view(np.uint32))


def host_chain(seg, x, norm):
    """models.py:624-653 as the mirror ran it before: Pillow (the restatement where Pillow is absent) around the smooth prediction"""
    original_shape = x.shape
    target_shape = tuple(np.round(np.multiply(original_shape[:2], seg.ds_ratio)).astype(int))
    try:
        from PIL import Image
        small = np.array(Image.fromarray(x).resize(target_shape, resample=Image.Resampling.LANCZOS))
    except ImportError:
        Image = None
        small = pr.resize(x, target_shape[::-1], "lanczos")
    if norm is not None:
        small = ((small - norm[0]) / norm[1]).astype(np.float32)
    pred = seg.handle.predict_smooth(small)
    if Image is not None:
        return np.array(Image.fromarray(pred).resize(original_shape, resample=Image.Resampling.NEAREST))
    return pr.resize(pred.astype(np.float32), original_shape[::-1], "nearest")


@pytest.mark.parametrize("norm", [None, (0.45, 0.25)], ids=["plain", "normed"])
def test_predict_auto_resample_equals_the_host_chain(weights, norm):
    from tmat_amd import models, synth
    seg = models.UNetXceptionPatchSegmentor(320, synth.pack_weights(weights), [64, 128, 256, 512], ds_ratio=0.625, max_patches=16,
                                            norm_mean=norm and norm[0], norm_std=norm and norm[1])
    try:
        x = np.random.RandomState(12).uniform(0, 1, (64, 48)).astype(np.float32)
        small = np.random.RandomState(13).uniform(0, 1, (40, 30)).astype(np.float32)
        before = seg.handle.predict_smooth(small)
        want = host_chain(seg, x, norm)
        got = seg.predict(x)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (48, 64)     # Pillow's (width, height): the axes swap
        nbad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert nbad == 0, f"{nbad} of {got.size} pixels differ, max |d| = {np.abs(got - want).max()}"
        assert float(got.std()) > 0
        # the chain leaves the handle's input norm off, as it found it
        assert np.array_equal(seg.handle.predict_smooth(small), before)
    finally:
        seg.handle.close()
