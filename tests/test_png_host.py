"""CPU: the PNG encoder's host twin (csrc/png_host.cpp through tmat_host_png_encode_batch) -- every file decodes to its
picture through two independent decoders (tests/helpers/png_check.py), the batch form, determinism, the guard bytes behind every
file, the error codes, the bound and the two size conditions."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib  # noqa: E402

import png_check as pc  # noqa: E402

S = _lib.png_stripe()
SHAPES = pc.shapes(S)
_files = {}


def picture(shape_name, kind):
    return pc.content(kind, SHAPES[shape_name], seed=len(shape_name))


def encoded(shape_name, kind):
    """the host twin's file of one case, made once and shared"""
    key = (shape_name, kind)
    if key not in _files:
        _files[key] = _lib.host_png_encode(picture(*key))[0]
    return _files[key]


def raw_bytes(shape):
    return shape[0] * (shape[1] * (3 if len(shape) == 3 else 1) + 1)


def test_stripe_is_sensible():
    assert 1024 <= S <= 65535        # one stored block holds a stripe; the stripe overhead stays a fraction of a percent


@pytest.mark.parametrize("kind", pc.CONTENTS)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_file_decodes_to_the_picture(shape_name, kind):
    pic = picture(shape_name, kind)
    data = encoded(shape_name, kind)
    pc.check_png(data, pic)
    raw = raw_bytes(pic.shape)
    assert len(data) <= _lib.png_bound(*pic.shape[:2], 3 if pic.ndim == 3 else 1)
    assert len(data) <= 1.01 * raw + 1024, (len(data), raw)
    if kind == "constant" and raw >= 65536:
        assert len(data) <= raw / 64, (len(data), raw)


def test_constant_pictures_compress():
    """raw >= 64 KiB: at most raw / 64 (a 258-byte match costs about 13 to 21 bits in fixed Huffman)"""
    for shape in ((256, 256), (640, 640), (150, 150, 3)):
        pic = pc.content("constant", shape)
        raw = raw_bytes(shape)
        assert raw >= 65536
        data = _lib.host_png_encode(pic)[0]
        pc.check_png(data, pic)
        assert len(data) <= raw / 64, (shape, len(data), raw)


def test_filter_choice_follows_the_content():
    """minimum sum of |signed residual|, ties to the lowest type.  Rows that repeat (a ramp along x) are all zero under Up, and only the
    first row needs Sub (3 per byte against the value itself); rows that are constant and step by 5 (a ramp along y) cost 5 under Paeth
    (the first byte; the others predict from the left) against |value| under Sub, 5 W under Up and |value| W under None"""
    f = pc.check_png(encoded("401x37", "hramp"), picture("401x37", "hramp"))
    assert f[0] == 1 and set(f[1:].tolist()) == {2}
    pic = picture("401x37", "vramp")
    f = pc.check_png(encoded("401x37", "vramp"), pic)
    for y in range(401):
        v = int(pic[y, 0])
        mag = v if v < 128 else 256 - v
        assert f[y] == (0 if v == 0 else 1 if (mag <= 5 or y == 0) else 4), (y, v, f[y])
    zero = np.zeros((5, 9), np.uint8)
    assert set(pc.check_png(_lib.host_png_encode(zero)[0], zero).tolist()) == {0}


def test_overlay_picture():
    bg, tree = pc.synthetic_tree()
    ov = _lib.host_render_tree(bg[None], [tree], 500)[0]
    assert ov.shape[1] == 500 and ov.shape[2] == 3
    data = _lib.host_png_encode(ov)[0]
    pc.check_png(data, ov)
    assert len(data) < ov.size / 2       # an overlay is a nearest-neighbour enlargement: rows repeat


def test_batch_equals_single_calls_and_calls_repeat():
    pics = np.stack([pc.content(k, (33, 31, 3), seed=3) for k in pc.CONTENTS])
    batch = _lib.host_png_encode(pics)
    assert len(batch) == len(pics)
    for i, p in enumerate(pics):
        assert batch[i] == _lib.host_png_encode(p)[0]
        pc.check_png(batch[i], p)
    assert batch == _lib.host_png_encode(pics)
    grey = np.stack([pc.content(k, SHAPES["S+1"], seed=4) for k in ("noise", "blob", "pattern")])
    gb = _lib.host_png_encode(grey)
    assert [gb[i] for i in range(3)] == [_lib.host_png_encode(g)[0] for g in grey]


def raw_call(fn, pics, n, H, W, ch, cap, fill=0xA5):
    """the C entry point on a pre-filled output -> (rc, out (n, cap) u8, sizes)"""
    out = np.full((max(n, 1), cap), fill, np.uint8)
    sizes = np.zeros(max(n, 1), np.uintp)
    rc = fn(None if pics is None else _lib.ptr(pics), n, H, W, ch, _lib.ptr(out), cap, _lib.ptr(sizes))
    return rc, out, sizes


def test_bytes_past_each_file_are_untouched():
    L = _lib.lib()
    pics = np.stack([pc.content(k, SHAPES["2S+1"], seed=2) for k in ("noise", "constant", "smooth")])
    n, H, W = pics.shape
    cap = _lib.png_bound(H, W, 1) + 100
    rc, out, sizes = raw_call(L.tmat_host_png_encode_batch, pics, n, H, W, 1, cap)
    assert rc == 0
    for i in range(n):
        k = int(sizes[i])
        assert 0 < k <= _lib.png_bound(H, W, 1)
        assert (out[i, k:] == 0xA5).all()
        pc.check_png(out[i, :k].tobytes(), pics[i])


def test_error_codes():
    L = _lib.lib()
    pic = pc.content("noise", (9, 11))
    bound = _lib.png_bound(9, 11, 1)
    rc, out, sizes = raw_call(L.tmat_host_png_encode_batch, pic, 1, 9, 11, 1, bound - 1)
    assert rc == _lib.E_CAP and (out == 0xA5).all() and sizes[0] == 0
    for H, W, ch in ((0, 11, 1), (9, 0, 1), (-1, 11, 1), (9, 11, 2), (9, 11, 4), (9, 11, 0)):
        rc, out, _ = raw_call(L.tmat_host_png_encode_batch, pic, 1, H, W, ch, bound)
        assert rc == _lib.E_ARG and (out == 0xA5).all(), (H, W, ch)
        b = C.c_size_t(77)
        assert L.tmat_png_bound(H, W, ch, C.byref(b)) == _lib.E_ARG and b.value == 77
    rc, out, _ = raw_call(L.tmat_host_png_encode_batch, None, 0, 9, 11, 1, bound)
    assert rc == 0 and (out == 0xA5).all()
    assert _lib.host_png_encode(np.zeros((0, 9, 11), np.uint8)) == []


def test_python_entry_shapes():
    g = pc.content("smooth", (12, 10))
    rgb = pc.content("smooth", (12, 10, 3))
    assert _lib.host_png_encode(g) == _lib.host_png_encode(g[None])
    assert _lib.host_png_encode(rgb) == _lib.host_png_encode(rgb[None])
    pc.check_png(_lib.host_png_encode(rgb)[0], rgb)
    with pytest.raises(ValueError):
        _lib.host_png_encode(g.astype(np.uint16))
    with pytest.raises(ValueError):
        _lib.host_png_encode(np.zeros((2, 3, 4, 5), np.uint8))


def test_unique_names_and_batched_writer(tmp_path):
    """branches' writers with an encoder: the "-N" rule of the PIL path, one encoder call per shape"""
    from tmat_amd import branches
    calls = []

    def enc(p):
        calls.append(np.asarray(p).shape)
        return _lib.host_png_encode(p)
    pics = np.stack([pc.content(k, (20, 24), seed=1) for k in ("noise", "blob", "smooth", "hramp")])
    a = branches.save_stage_pictures(pics, tmp_path / "pil")
    b = branches.save_stage_pictures(pics, tmp_path / "dev", well_mask=pics[1] > 0, encoder=enc)
    assert calls == [(5, 20, 24)]
    assert [Path(p).name for p in b] == [Path(p).name for p in a] + ["well_mask.png"]
    b2 = branches.save_stage_pictures(pics, tmp_path / "dev", encoder=enc)
    assert [Path(p).name for p in b2] == [n.replace(".png", "-2.png") for n in branches.STAGE_PICTURE_FILES]
    from PIL import Image
    for pa, pb in zip(a, b):
        assert np.array_equal(np.asarray(Image.open(pa)), np.asarray(Image.open(pb)))
    assert np.array_equal(np.asarray(Image.open(b[4])), (pics[1] > 0).astype(np.uint8) * 255)
