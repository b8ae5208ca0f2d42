"""CPU: the PNG encoder's compact mode (one-step lazy parse, stored / fixed / dynamic Huffman block per stripe) through the
host twin, tmat_host_png_encode_batch_mode -- every file decodes through the two independent decoders of tests/helpers/png_check.py
as one whole zlib stream, is never larger than the fast file, fast stays what tmat_host_png_encode_batch gives; the size bounds; the
code lengths of png_code_lengths directly; and a picture that compresses by its dynamic block alone."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib  # noqa: E402

import png_blocks as pb  # noqa: E402
import png_check as pc  # noqa: E402

S = _lib.png_stripe()
SHAPES = pc.shapes(S)
_files = {}


def picture(shape_name, kind):
    return pc.content(kind, SHAPES[shape_name], seed=len(shape_name))


def encoded(shape_name, kind, mode):
    """the host twin's file of one case and mode, made once and shared"""
    key = (shape_name, kind, mode)
    if key not in _files:
        _files[key] = _lib.host_png_encode(picture(shape_name, kind), mode=mode)[0]
    return _files[key]


@pytest.mark.parametrize("kind", pc.CONTENTS)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_compact_file_decodes_and_is_never_larger(shape_name, kind):
    """check_png reads the IDAT chunks as ONE zlib stream (eof reached, nothing unused), then un-filters, then asks Pillow"""
    pic = picture(shape_name, kind)
    compact, fast = encoded(shape_name, kind, "compact"), encoded(shape_name, kind, "fast")
    pc.check_png(compact, pic)
    assert len(compact) <= _lib.png_bound(*pic.shape[:2], 3 if pic.ndim == 3 else 1)
    assert len(compact) <= len(fast), (len(compact), len(fast))
    if kind == "noise":
        # nothing to gain: the same file in both modes, every stripe stored.  A stripe of a few bytes is the exception the arithmetic
        # demands: a stored block costs 5 bytes over the data, a fixed block 8 or 9 bits a byte and 10 bits around them, so noise of
        # under about a hundred bytes is smaller fixed.  From 512 bytes on (over 20 bytes of expected excess) every stripe is stored
        assert compact == fast
        raw = pic.shape[0] * (pic.shape[1] * (3 if pic.ndim == 3 else 1) + 1)
        sizes = [min(S, raw - k * S) for k in range((raw + S - 1) // S)]
        for mode_file in (compact, fast):
            bt = pb.btypes(mode_file)
            assert len(bt) == len(sizes)
            assert all(b == 0 for b, n in zip(bt, sizes) if n >= 512), (bt, sizes)
            assert 2 not in bt


@pytest.mark.parametrize("shape_name", ["1x1", "33x31rgb", "401x37", "2S+1", "640"])
def test_fast_is_todays_file(shape_name):
    pics = np.stack([picture(shape_name, k) for k in pc.CONTENTS])
    old = _lib._png_call(_lib.lib().tmat_host_png_encode_batch, pics, "tmat_host_png_encode_batch")
    assert old == _lib.host_png_encode(pics, mode="fast") == _lib.host_png_encode(pics)
    for f in old:
        assert 2 not in pb.btypes(f)


def test_size_bounds():
    """compact <= 0.70 fast on the smooth pictures (the issue's prototype: 0.62 and 0.63); strictly smaller on blob and hramp"""
    for shape in ((640, 640), (300, 300, 3)):
        pic = pc.content("smooth", shape)
        fast, compact = _lib.host_png_encode(pic)[0], _lib.host_png_encode(pic, mode="compact")[0]
        pc.check_png(compact, pic)
        print(f"smooth {shape}: fast {len(fast)} compact {len(compact)} ratio {len(compact) / len(fast):.4f}")
        assert len(compact) <= 0.70 * len(fast), (shape, len(compact), len(fast))
        assert 2 in pb.btypes(compact)
    for kind in ("blob", "hramp"):
        fast, compact = encoded("640", kind, "fast"), encoded("640", kind, "compact")
        print(f"{kind} 640: fast {len(fast)} compact {len(compact)}")
        assert len(compact) < len(fast), (kind, len(compact), len(fast))


def test_code_lengths_direct():
    for name, f, limit in pb.direct_histograms():
        pb.check_lengths(f, limit, _lib.host_png_code_lengths(f, limit), name)
    # the two Fibonacci histograms are deeper than their limits unrestricted: the limit is met, not merely unneeded
    assert pb.huffman(pb.fibonacci(18))[1] == 17 and pb.huffman(pb.fibonacci(10))[1] == 9
    assert _lib.host_png_code_lengths(pb.fibonacci(18), 15).max() == 15
    assert _lib.host_png_code_lengths(pb.fibonacci(10), 7).max() == 7
    two = _lib.host_png_code_lengths(pb.direct_histograms()[3][1], 15)
    assert sorted(two[two > 0].tolist()) == [1, 1]
    assert set(_lib.host_png_code_lengths(np.full(256, 3, np.uint32), 15).tolist()) == {8}


@pytest.mark.parametrize("limit", [15, 7])
def test_code_lengths_random(limit):
    deep = 0
    for j, f in enumerate(pb.random_histograms(limit)):
        lens = _lib.host_png_code_lengths(f, limit)
        pb.check_lengths(f, limit, lens, (limit, j))
        deep += pb.huffman(f)[1] > limit
        assert np.array_equal(lens, _lib.host_png_code_lengths(f, limit))
    assert deep >= 10, deep              # the limiter is exercised, not only the Huffman tree


def test_code_lengths_error_codes():
    L = _lib.lib()
    f = np.ones(20, np.uint32)
    out = np.full(20, 0xA5, np.uint8)
    for n, limit in ((0, 15), (287, 15), (20, 0), (20, 16), (20, 4)):
        assert L.tmat_host_png_code_lengths(_lib.ptr(f), n, limit, _lib.ptr(out)) == _lib.E_ARG
    big = np.full(20, 1 << 20, np.uint32)
    assert L.tmat_host_png_code_lengths(_lib.ptr(big), 20, 15, _lib.ptr(out)) == _lib.E_ARG
    assert (out == 0xA5).all()


def de_bruijn(k, n):
    """the standard Lyndon-word construction: every n-gram over k symbols once, cyclically"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def test_a_dynamic_block_without_any_match():
    """one grey row whose Sub residuals are a de Bruijn sequence of order 3 over {0, 2, 3, 4, 5, 6} (216 + 2 values, so that every
    trigram stands once and none repeats; 1 is left to the filter byte): no candidate finds a match, the fixed block spends 8 bits a
    byte, the dynamic block under 3"""
    alphabet = np.array([0, 2, 3, 4, 5, 6])
    cyc = de_bruijn(6, 3)
    assert len(cyc) == 216
    res = alphabet[np.array(cyc + cyc[:2])]
    assert len(res) == 218
    tri = {tuple(res[i: i + 3]) for i in range(216)}
    assert len(tri) == 216
    pic = (np.cumsum(res) & 255).astype(np.uint8)[None]
    fast, compact = _lib.host_png_encode(pic)[0], _lib.host_png_encode(pic, mode="compact")[0]
    filters = pc.check_png(compact, pic)
    assert filters.tolist() == [1]          # Sub: Paeth ties to it on a first row, None, Up and Average sum far higher
    pc.check_png(fast, pic)
    assert pb.btypes(compact) == [2] and pb.btypes(fast) == [1]
    assert len(compact) < len(fast), (len(compact), len(fast))
    assert len(compact) < 33 + 28 + 12 + 2 + 219 * 3 // 8 + 40      # under 3 bits a byte and a header of 40 bytes at the most


def test_batch_guard_bytes_and_error_codes():
    L = _lib.lib()
    pics = np.stack([pc.content(k, SHAPES["2S+1"], seed=2) for k in ("noise", "constant", "smooth")])
    n, H, W = pics.shape
    bound = _lib.png_bound(H, W, 1)
    out = np.full((n, bound + 100), 0xA5, np.uint8)
    sizes = np.zeros(n, np.uintp)
    assert L.tmat_host_png_encode_batch_mode(_lib.ptr(pics), n, H, W, 1, _lib.ptr(out), bound + 100, _lib.ptr(sizes), 1) == 0
    single = [_lib.host_png_encode(p, mode="compact")[0] for p in pics]
    for i in range(n):
        k = int(sizes[i])
        assert out[i, :k].tobytes() == single[i] and (out[i, k:] == 0xA5).all()
    out[:] = 0xA5
    for mode in (-1, 2, 7):
        assert L.tmat_host_png_encode_batch_mode(_lib.ptr(pics), n, H, W, 1, _lib.ptr(out), bound + 100, _lib.ptr(sizes), mode) == _lib.E_ARG
    assert L.tmat_host_png_encode_batch_mode(_lib.ptr(pics), n, H, W, 1, _lib.ptr(out), bound - 1, _lib.ptr(sizes), 1) == _lib.E_CAP
    assert (out == 0xA5).all()
    with pytest.raises(ValueError):
        _lib.host_png_encode(pics, mode="small")
    assert L.tmat_png_set_mode(None, 1) == _lib.E_ARG
