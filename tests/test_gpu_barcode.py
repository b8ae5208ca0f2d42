"""GPU: the barcode picture on the device (tmat_render_barcode, barcode_kernel in overlay_kernels.hip) equals its host twin byte for byte,
and its PNG form equals the host PNG of the host picture."""
import sys
from pathlib import Path

import numpy as np
import pytest

from tmat_amd import _lib

from test_grid_host import BARCODE_CASES

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
from png_check import check_png  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    h = _lib.Handle(None, 0)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(BARCODE_CASES))
def test_device_barcode_equals_host_twin(plain, name):
    bars, vw = BARCODE_CASES[name]
    got = plain.render_barcode([bars], vw)
    want = _lib.host_render_barcode(bars, vw)
    assert got.shape == (1,) + want.shape
    assert np.array_equal(got[0], want), int((got[0] != want).sum())


def test_batch_of_five_with_different_bar_counts(plain):
    """five pictures in one launch, one of them empty: the canvases run through in one flat buffer (333 -> S = 300, 270000 bytes per
    picture is a multiple of 16; 57 -> S = 51, 7803 bytes is not, so 16-byte groups straddle pictures and the last group is short)"""
    for vw in (333, 57):
        blist = [BARCODE_CASES[k][0] for k in ("n37_w333", "n0_w333", "n300_w20", "n1_w1000", "all_equal_births")]
        got = plain.render_barcode(blist, vw)
        assert got.shape[0] == 5
        for i, b in enumerate(blist):
            want = _lib.host_render_barcode(b, vw)
            assert np.array_equal(got[i], want), (vw, i, int((got[i] != want).sum()))
        assert (got[1] == 255).all() and not (got[0] == 255).all()
        assert np.array_equal(got, plain.render_barcode(blist, vw))


def test_png_form_equals_host_png_of_host_barcode(plain):
    blist = [BARCODE_CASES[k][0] for k in ("n37_w333", "n0_w333", "zero_span", "n300_w20")]
    for vw in (333, 20):
        files = plain.render_barcode_png(blist, vw)
        pics = np.stack([_lib.host_render_barcode(b, vw) for b in blist])
        assert files == _lib.host_png_encode(pics)
        for f, p in zip(files, pics):
            check_png(f, p)


def test_bad_arguments(plain):
    L = _lib.lib()
    bars = np.zeros((2, 2))
    out = np.full((1, 18, 18, 3), 7, np.uint8)
    off = np.array([0, 2], np.int32)
    assert L.tmat_render_barcode(plain.raw, _lib.ptr(bars), _lib.ptr(np.array([1, 2], np.int32)), 1, 20, _lib.ptr(out)) == _lib.E_ARG     # offsets start at 0
    assert L.tmat_render_barcode(plain.raw, None, _lib.ptr(off), 1, 20, _lib.ptr(out)) == _lib.E_ARG
    assert L.tmat_render_barcode(plain.raw, _lib.ptr(bars), _lib.ptr(off), 1, 0, _lib.ptr(out)) == _lib.E_ARG
    sizes = np.zeros(1, np.uintp)
    files = np.full(_lib.png_bound(18, 18, 3), 7, np.uint8)
    assert L.tmat_render_barcode_png(plain.raw, _lib.ptr(bars), _lib.ptr(off), 1, 20, _lib.ptr(files), files.size - 1, _lib.ptr(sizes)) == _lib.E_CAP
    assert (out == 7).all() and (files == 7).all() and sizes[0] == 0
