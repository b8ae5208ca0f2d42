"""GPU: the TIFF decoder on the device (csrc/tiff_kernels.hip through tmat_tiff_decode_batch and tmat_tiff_decode_batch_dev)
against its host twin and against Pillow, bit for bit, on the fixtures of tests/test_tiff_host.py; one batch of 256 strips; the status
vectors of unsupported and corrupt files with guard planes on both sides; what the handle holds; and the resident hand-off to
tmat_zproj_dev and tmat_analyze_batch_grid_dev."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib, branches, synth  # noqa: E402

import tiff_files as tf  # noqa: E402
from tiff_files import SENTINEL, assert_guards, grid_cases, guarded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    h = _lib.Handle(None, 0)
    yield h
    h.close()


class DevPlanes:
    """(n + 2, H, W) uint16 on the device, every word SENTINEL; `mid` is the (n, H, W) middle a decode may write"""

    def __init__(self, handle, n, H, W):
        self.handle, self.shape = handle, (n + 2, H, W)
        self.ptr = C.c_void_p()
        fill = np.full(self.shape, SENTINEL, np.uint16)
        _lib.check(_lib.lib().tmat_dev_alloc(handle.raw, fill.nbytes, C.byref(self.ptr)), "tmat_dev_alloc")
        _lib.check(_lib.lib().tmat_dev_upload(handle.raw, self.ptr, _lib.ptr(fill), fill.nbytes), "tmat_dev_upload")
        self.mid = C.c_void_p(self.ptr.value + H * W * 2)

    def download(self):
        out = np.empty(self.shape, np.uint16)
        _lib.check(_lib.lib().tmat_dev_download(self.handle.raw, _lib.ptr(out), self.ptr, out.nbytes), "tmat_dev_download")
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.lib().tmat_dev_free(self.handle.raw, self.ptr), "tmat_dev_free")


def both_device_forms(handle, files, planes, H, W):
    """the two device entry points on guarded buffers -> [(whole buffer, bits, status)] for the host-output and the resident form"""
    buf, mid = guarded(len(planes), H, W)
    _, bits, status = handle.tiff_decode(files, planes, H, W, mid)
    with DevPlanes(handle, len(planes), H, W) as d:
        bits_d, status_d = handle.tiff_decode_dev(files, planes, H, W, d.mid)
        return [(buf, bits, status), (d.download(), bits_d, status_d)]


def assert_same_as_host(handle, files, planes, H, W, names=None):
    hbuf, hmid = guarded(len(planes), H, W)
    _, hbits, hstatus = _lib.host_tiff_decode(files, planes, H, W, hmid)
    for form, (buf, bits, status) in zip(("host output", "resident output"), both_device_forms(handle, files, planes, H, W)):
        assert bits == hbits, form
        assert np.array_equal(status, hstatus), (form, dict(zip(names or range(len(planes)), zip(status, hstatus))))
        bad = [i for i in range(len(planes)) if not np.array_equal(buf[1 + i], hbuf[1 + i])]
        assert not bad, (form, [names[i] if names else i for i in bad][:8])
        assert_guards(buf)
    return hmid, hstatus


@pytest.mark.parametrize("dtype", tf.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", tf.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_product_equals_host_twin_and_pillow(plain, shape, dtype):
    cases = grid_cases(shape, dtype)
    files = [c[1] for c in cases]
    got, status = assert_same_as_host(plain, files, [(i, 0) for i in range(len(files))], shape[0], shape[1], [c[0] for c in cases])
    assert (status == _lib.TIFF_OK).all()
    for i, (name, f, arr) in enumerate(cases):
        assert np.array_equal(got[i], tf.pil_decode(f)), name


def test_multipage_big_endian_and_full_table(plain):
    arrs = [tf.content(k, (64, 80), np.uint16, i) for i, k in enumerate(("smooth", "noise", "checker"))]
    f, other = tf.pil_tiff(arrs, "lzw_pred", 7), tf.pil_tiff(arrs[1], "packbits")
    planes = [(0, 2), (1, 0), (0, 0), (0, 2), (0, 1), (0, 3)]
    got, status = assert_same_as_host(plain, [f, other], planes, 64, 80)
    assert list(status) == [_lib.TIFF_OK] * 5 + [_lib.TIFF_CORRUPT]
    for i, (fi, pg) in enumerate(planes[:5]):
        assert np.array_equal(got[i], tf.pil_decode([f, other][fi], pg))
    for dtype in tf.DTYPES:
        mm, want = [], []
        for comp, rps in (("none", 3), ("lzw_pred", 3), ("lzw", None), ("packbits", 2)):
            arr = tf.content("ramp" if comp == "lzw_pred" else "smooth", (7, 5), dtype, 4)
            mm.append(tf.check_with_pillow(tf.hand_tiff(arr, comp, rps, order=">"), arr))
            want.append(arr)
        got, status = assert_same_as_host(plain, mm, [(i, 0) for i in range(len(mm))], 7, 5)
        assert (status == _lib.TIFF_OK).all() and np.array_equal(got, np.stack(want).astype(np.uint16))
    full, arr = tf.full_table_file()
    got, status = assert_same_as_host(plain, [full], [(0, 0)], arr.shape[0], arr.shape[1])
    assert status[0] == _lib.TIFF_OK and np.array_equal(got[0], arr)


def test_one_batch_of_256_strips(plain):
    """8 planes of 1024 x 1024 uint16, LZW + predictor, Pillow's default strips: 256 decoders in one launch set"""
    arrs = [synth.synth_image(i, 1024, n_vessels=12, scale=1.0).astype(np.uint16) for i in range(2)]
    arrs += [tf.content(k, (1024, 1024), np.uint16, 3) for k in ("smooth", "const", "checker", "ramp", "zero", "noise")]
    files = [tf.pil_tiff(a, "lzw_pred") for a in arrs]
    assert sum(_lib.tiff_probe(f)[0]["n_strips"] for f in files) == 256
    want = np.stack([tf.pil_decode(f) for f in files])
    assert np.array_equal(want, np.stack(arrs))
    out, bits, status = plain.tiff_decode(files, [(i, 0) for i in range(8)], 1024, 1024)
    assert bits == 16 and (status == _lib.TIFF_OK).all()
    assert np.array_equal(out, want)
    with DevPlanes(plain, 8, 1024, 1024) as d:
        bits, status = plain.tiff_decode_dev(files, [(i, 0) for i in range(8)], 1024, 1024, d.mid)
        buf = d.download()
    assert bits == 16 and (status == _lib.TIFF_OK).all() and np.array_equal(buf[1:-1], want)
    assert_guards(buf)


def test_unsupported_and_corrupt_status_equal_the_host_twin(plain):
    un, co = tf.unsupported_files(), tf.corrupt_files()
    good = tf.pil_tiff(tf.content("smooth", (7, 5), np.uint8, 1), "lzw")
    names = [f"unsupported {k}" for k in sorted(un)] + [f"corrupt {k}" for k in sorted(co)] + ["good"]
    files = [un[k][0] for k in sorted(un)] + [co[k][0] for k in sorted(co)] + [good]
    planes = [(i, 0) for i in range(len(un))] + [(len(un) + i, co[k][1]) for i, k in enumerate(sorted(co))] + [(len(files) - 1, 0)]
    got, status = assert_same_as_host(plain, files, planes, 7, 5, names)
    assert list(status) == [_lib.TIFF_FALLBACK] * len(un) + [_lib.TIFF_CORRUPT] * len(co) + [_lib.TIFF_OK]
    assert (got[:-1] == SENTINEL).all() and np.array_equal(got[-1], tf.pil_decode(good))


def test_a_handle_that_never_decodes_holds_nothing_for_it():
    a, b = _lib.Handle(None, 0), _lib.Handle(None, 0)
    try:
        before = a.debug_held_bytes()
        assert before == b.debug_held_bytes()
        arr = tf.content("smooth", (64, 80), np.uint16, 0)
        out, _, status = b.tiff_decode([tf.pil_tiff(arr, "lzw")], [(0, 0)], 64, 80)
        assert status[0] == _lib.TIFF_OK and np.array_equal(out[0], arr)
        assert a.debug_held_bytes() == before                   # the handle that never decoded holds what it held
        assert b.debug_held_bytes()[0] > before[0]              # the decoder's blocks sit in the pool of the handle that did
    finally:
        a.close()
        b.close()


def test_analyze_rows_are_stable_across_a_decode(handle):
    cfg = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)
    img = synth.synth_image(0, 512, n_vessels=12, scale=1.0)
    before = branches.analyze_batch(handle, img[None], cfg, 500.0)
    f = tf.pil_tiff(img.astype(np.uint16), "lzw_pred")
    out, _, status = handle.tiff_decode([f], [(0, 0)], 512, 512)
    assert status[0] == _lib.TIFF_OK and np.array_equal(out[0], img)
    assert branches.analyze_batch(handle, out, cfg, 500.0) == before
    assert branches.analyze_batch(handle, img[None], cfg, 500.0) == before


def test_decoded_stack_feeds_zproj_dev(plain):
    stack = np.stack([tf.content(k, (64, 80), np.uint16, z) for z, k in enumerate(("smooth", "noise", "checker", "smooth"))])
    f = tf.pil_tiff(list(stack), "lzw_pred", 7)
    L = _lib.lib()
    for method in ("fs", "max"):
        want = plain.zproj(tf.pil_decode_all(f)[None], method)
        with DevPlanes(plain, 4, 64, 80) as d, DevPlanes(plain, 1, 64, 80) as o:
            bits, status = plain.tiff_decode_dev([f], [(0, z) for z in range(4)], 64, 80, d.mid)
            assert bits == 16 and (status == _lib.TIFF_OK).all()
            _lib.check(L.tmat_zproj_dev(plain.raw, d.mid, 1, 4, 64, 80, _lib.Handle.ZPROJ_METHODS[method], o.mid), "tmat_zproj_dev")
            got = o.download()[1:-1]
        assert np.array_equal(got, want), method


def test_decoded_images_feed_the_grid_entry(handle):
    cfg = dict(graph_smoothing_window=12, min_branch_length=12)
    pairs = [(1.0, 4.0), (5.0, 40.0)]
    imgs = np.stack([synth.synth_image(i, 512, n_vessels=12, scale=1.0) for i in range(2)]).astype(np.uint16)
    files = [tf.pil_tiff(a, "lzw_pred") for a in imgs]
    want, _ = branches.analyze_batch_grid(handle, np.stack([tf.pil_decode(f) for f in files]), cfg, 500.0, pairs=pairs)
    with DevPlanes(handle, 2, 512, 512) as d:
        bits, status = handle.tiff_decode_dev(files, [(0, 0), (1, 0)], 512, 512, d.mid)
        assert bits == 16 and (status == _lib.TIFF_OK).all()
        got, _ = branches.analyze_batch_grid(handle, (d.mid, (2, 512, 512)), cfg, 500.0, pairs=pairs, input_bits=bits)
    assert got == want
    assert any(r[1] > 0 for r in want[pairs[0]])
