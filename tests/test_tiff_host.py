"""CPU: the TIFF container parser and the decoder's host twin (csrc/tiff_host.cpp over csrc/tiff.h, through tmat_tiff_probe and
tmat_host_tiff_decode_batch) against Pillow / libtiff, an independent decoder, exactly: the cross product of shapes,
depths, rows per strip, compressions and contents of tests/helpers/tiff_files.py; multi-page selection; big-endian files; a stream that
runs with a full table; the unsupported kinds (FALLBACK, reason, output untouched); corrupt files (CORRUPT, guard words intact)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib  # noqa: E402

import tiff_files as tf  # noqa: E402
from tiff_files import SENTINEL, assert_guards, grid_cases, guarded  # noqa: E402


@pytest.mark.parametrize("dtype", tf.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", tf.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_product_equals_pillow(shape, dtype):
    H, W = shape
    cases = grid_cases(shape, dtype)
    files = [c[1] for c in cases]
    for name, f, arr in cases:
        pages = _lib.tiff_probe(f)
        assert len(pages) == 1, name
        p = pages[0]
        assert (p["status"], p["reason"]) == (_lib.TIFF_OK, "none"), (name, p)       # no hiding behind the fallback
        assert (p["height"], p["width"], p["bits"]) == (H, W, np.dtype(dtype).itemsize * 8), (name, p)
        assert p["n_strips"] == -(-H // p["rows_per_strip"]), (name, p)
        ref = tf.pil_decode(f)
        assert np.array_equal(ref, arr), name                                       # Pillow reads back what it wrote
    buf, out = guarded(len(files), H, W)
    _, bits, status = _lib.host_tiff_decode(files, [(i, 0) for i in range(len(files))], H, W, out)
    assert bits == np.dtype(dtype).itemsize * 8
    assert (status == _lib.TIFF_OK).all(), [cases[i][0] for i in np.nonzero(status)[0]]
    for i, (name, f, arr) in enumerate(cases):
        assert np.array_equal(out[i], arr.astype(np.uint16)), name
    assert_guards(buf)


def test_rows_per_strip_reach_the_file():
    """the fixtures really have the strip layouts they are named for"""
    arr = tf.content("smooth", (300, 257), np.uint16, 1)
    for comp in tf.COMPRESSIONS:
        for rps in (1, 7, 300):
            p = _lib.tiff_probe(tf.pil_tiff(arr, comp, rps))[0]
            assert (p["rows_per_strip"], p["n_strips"]) == (rps, -(-300 // rps)), (comp, rps, p)
        p = _lib.tiff_probe(tf.pil_tiff(arr, comp))[0]
        assert p["n_strips"] == (1 if comp == "none" else 3), (comp, p)     # libtiff's 64 KiB strips; Pillow's own raw writer: one strip
    assert _lib.tiff_probe(tf.pil_tiff(arr, "lzw_pred"))[0]["predictor"] == 2
    assert _lib.tiff_probe(tf.pil_tiff(arr, "lzw"))[0]["compression"] == 5
    assert _lib.tiff_probe(tf.pil_tiff(arr, "packbits"))[0]["compression"] == 32773


def test_noise_strip_is_larger_than_raw():
    """uniform noise: the LZW strip is larger than its raw bytes, and still decodes"""
    arr = tf.content("noise", (64, 80), np.uint16, 9)
    f = tf.pil_tiff(arr, "lzw", 64)
    assert len(f) > arr.nbytes * 1.2
    out, _, status = _lib.host_tiff_decode([f], [(0, 0)], 64, 80)
    assert status[0] == _lib.TIFF_OK and np.array_equal(out[0], arr)


def test_multipage_any_order_and_twice():
    arrs = [tf.content(k, (64, 80), np.uint16, i) for i, k in enumerate(("smooth", "noise", "checker"))]
    f = tf.pil_tiff(arrs, "lzw_pred", 7)
    other = tf.pil_tiff(arrs[1], "packbits")
    pages = _lib.tiff_probe(f)
    assert len(pages) == 3 and all(p["status"] == _lib.TIFF_OK for p in pages)
    planes = [(0, 2), (1, 0), (0, 0), (0, 2), (0, 1)]
    buf, out = guarded(len(planes), 64, 80)
    _, bits, status = _lib.host_tiff_decode([f, other], planes, 64, 80, out)
    assert bits == 16 and (status == _lib.TIFF_OK).all()
    for i, (fi, pg) in enumerate(planes):
        assert np.array_equal(out[i], tf.pil_decode([f, other][fi], pg)), (fi, pg)
        assert np.array_equal(out[i], arrs[pg] if fi == 0 else arrs[1])
    assert_guards(buf)
    _, _, status = _lib.host_tiff_decode([f], [(0, 3)], 64, 80)          # a page the file does not have
    assert status[0] == _lib.TIFF_CORRUPT


@pytest.mark.parametrize("dtype", tf.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("comp, rps", [("none", 3), ("lzw_pred", 3), ("lzw", None), ("packbits", 2)])
def test_big_endian_files(comp, rps, dtype):
    arr = tf.content("ramp" if comp == "lzw_pred" else "smooth", (7, 5), dtype, 4)
    f = tf.check_with_pillow(tf.hand_tiff(arr, comp, rps, order=">"), arr)
    p = _lib.tiff_probe(f)[0]
    assert p["big_endian"] == 1 and p["status"] == _lib.TIFF_OK, p
    buf, out = guarded(1, 7, 5)
    _, bits, status = _lib.host_tiff_decode([f], [(0, 0)], 7, 5, out)
    assert status[0] == _lib.TIFF_OK and bits == arr.dtype.itemsize * 8
    assert np.array_equal(out[0], arr)
    assert_guards(buf)


def test_little_endian_hand_written_files_match_too():
    """the helper's own encoders against both decoders, in the byte order Pillow also writes"""
    for comp in tf.COMPRESSIONS:
        arr = tf.content("checker", (64, 80), np.uint16, 6)
        f = tf.check_with_pillow(tf.hand_tiff(arr, comp, 7), arr)
        out, _, status = _lib.host_tiff_decode([f], [(0, 0)], 64, 80)
        assert status[0] == _lib.TIFF_OK and np.array_equal(out[0], arr), comp


def test_stream_with_a_full_table():
    f, arr = tf.full_table_file()
    tf.check_with_pillow(f, arr)
    H, W = arr.shape
    buf, out = guarded(1, H, W)
    _, _, status = _lib.host_tiff_decode([f], [(0, 0)], H, W, out)
    assert status[0] == _lib.TIFF_OK and np.array_equal(out[0], arr)
    assert_guards(buf)


def test_unsupported_kinds_fall_back_untouched():
    files = tf.unsupported_files()
    names = sorted(files)
    for name in names:
        f, reason = files[name]
        p = _lib.tiff_probe(f)[0]
        assert (p["status"], p["reason"]) == (_lib.TIFF_FALLBACK, reason), (name, p)
    good = tf.pil_tiff(tf.content("smooth", (7, 5), np.uint8, 1), "lzw")
    blobs = [files[n][0] for n in names] + [good]
    buf, out = guarded(len(blobs), 7, 5)
    _, bits, status = _lib.host_tiff_decode(blobs, [(i, 0) for i in range(len(blobs))], 7, 5, out)
    assert list(status[:-1]) == [_lib.TIFF_FALLBACK] * len(names) and status[-1] == _lib.TIFF_OK and bits == 8
    assert (out[:-1] == SENTINEL).all(), "a fallback plane was written"
    assert np.array_equal(out[-1], tf.pil_decode(good))
    assert_guards(buf)


def test_corrupt_files_are_refused_inside_their_planes():
    files = tf.corrupt_files()
    names = sorted(files)
    for name in names:
        f, page, at_probe = files[name]
        pages = _lib.tiff_probe(f)
        assert any(p["status"] == _lib.TIFF_CORRUPT for p in pages) == at_probe, (name, pages)
    assert _lib.tiff_probe(files["ifd_loop"][0])[-1]["reason"] == "loop"
    assert _lib.tiff_probe(files["entry_count_overruns"][0])[-1]["reason"] == "ifd"
    assert _lib.tiff_probe(files["offset_past_end"][0])[0]["reason"] == "strips"
    good = tf.pil_tiff(tf.content("smooth", (7, 5), np.uint8, 1), "packbits")
    blobs = [files[n][0] for n in names] + [good]
    planes = [(i, files[n][1]) for i, n in enumerate(names)] + [(len(names), 0)]
    buf, out = guarded(len(blobs), 7, 5)
    _, _, status = _lib.host_tiff_decode(blobs, planes, 7, 5, out)
    assert list(status[:-1]) == [_lib.TIFF_CORRUPT] * len(names), dict(zip(names, status))
    assert status[-1] == _lib.TIFF_OK and np.array_equal(out[-1], tf.pil_decode(good))      # the other planes are unaffected
    assert (out[:-1] == SENTINEL).all(), "a corrupt plane was written"
    assert_guards(buf)


def test_every_truncation_of_a_small_file_is_handled():
    """no prefix of a valid file reads out of bounds or writes outside its plane (the sanitizer program runs the same sweep)"""
    arr = tf.content("smooth", (7, 5), np.uint16, 8)
    for comp in ("lzw_pred", "packbits"):
        f = tf.pil_tiff(arr, comp, 3)
        for cut in range(0, len(f)):
            buf, out = guarded(1, 7, 5)
            _, _, status = _lib.host_tiff_decode([f[:cut]], [(0, 0)], 7, 5, out)
            assert status[0] in (_lib.TIFF_OK, _lib.TIFF_CORRUPT, _lib.TIFF_FALLBACK)
            if status[0] != _lib.TIFF_OK:
                assert (out == SENTINEL).all()
            assert_guards(buf)


def test_mixed_shape_or_depth_is_an_argument_error():
    a = tf.pil_tiff(tf.content("smooth", (7, 5), np.uint8, 1), "lzw")
    b = tf.pil_tiff(tf.content("smooth", (7, 5), np.uint16, 1), "lzw")
    c = tf.pil_tiff(tf.content("smooth", (5, 7), np.uint8, 1), "lzw")
    with pytest.raises(_lib.TmatError, match="bit depth"):
        _lib.host_tiff_decode([a, b], [(0, 0), (1, 0)], 7, 5)
    with pytest.raises(_lib.TmatError, match="shape"):
        _lib.host_tiff_decode([a, c], [(0, 0), (1, 0)], 7, 5)
    out, bits, status = _lib.host_tiff_decode([], [], 7, 5)
    assert out.shape == (0, 7, 5) and bits == 0 and len(status) == 0
