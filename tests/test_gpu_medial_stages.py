"""GPU: the stages of csrc/thin_kernels.hip (tmat_debug_medial_stages: skeleton, distance, order keys, predecessor bytes, launches of
ma_round_kernel) against scipy's EDT, oracle.morph.medial_axis and the wavefront model of tests/helpers/medial_cases.py.  Every
comparison is exact and covers every pixel.  tests/test_medial_cases.py pins the model and the properties of the inputs: which ones
put tiles to sleep and wake them, which frame sends the chunk scan through its slab loop twice."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import medial_cases as md  # noqa: E402
import morph_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("skel", "dist", "keys", "dep", "launches")


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def reference(key, named_masks):
    """the model of every mask of a batch (each computed once per module) stacked, and the launch count of the batch"""
    models = [md.model((key, name), m) for name, m in named_masks]
    ref = {k: np.stack([r[k] for r in models]) for k in ("mask", "skel", "dist", "keys", "dep")}
    ref["names"] = [name for name, _ in named_masks]
    ref["depths"] = [r["depth"] for r in models]
    ref["launches"] = md.expected_launches(max(ref["depths"]))
    return ref


def assert_images_equal(got, want, names, what):
    """exact, every pixel; names the images that differ and the first differing pixel"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = [(names[i], int((got[i] != want[i]).sum()), tuple(int(v) for v in np.argwhere(got[i] != want[i])[0]))
           for i in range(len(names)) if not np.array_equal(got[i], want[i])]
    assert not bad, (what, bad)


def check_stages(plain, ref, got=None):
    """one call of the debug entry point on the batch against its reference, and tmat_medial_axis_batch against the debug entry"""
    if got is None:
        got = plain.debug_medial_stages(ref["mask"])
    names = ref["names"]
    print(f"{names}: depths {ref['depths']}, launches {int(got['launches'][0])} (model {ref['launches']})")
    assert_images_equal(got["dist"].view(np.uint64), ref["dist"].view(np.uint64), names, "dist (bits)")
    assert_images_equal(got["keys"], ref["keys"], names, "keys")
    assert_images_equal(got["dep"], ref["dep"], names, "dep")
    assert_images_equal(got["skel"], ref["skel"].astype(np.uint8), names, "skel")
    assert got["launches"].tolist() == [ref["launches"]], names
    skel, dist = plain.medial_axis(ref["mask"])
    assert skel.astype(np.uint8).tobytes() == got["skel"].tobytes() and dist.tobytes() == got["dist"].tobytes(), names
    return got


def assert_same_bytes(a, b, what):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- sleeping tiles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, _ in md.wake_cases()])
def test_wake_inputs_one_image_per_call(plain, name):
    """chains of up to 1423 levels: tiles sleep while the front is far away and must wake when it arrives.  A tile that wakes late
    costs launches, one that never wakes ends in the library's error"""
    check_stages(plain, reference("wake", [(name, dict(md.wake_cases())[name])]))


# ---- small and odd frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", md.SMALL_SHAPES, ids=[f"{h}x{w}" for h, w in md.SMALL_SHAPES])
def test_small_and_odd_frames_every_generator_as_one_batch(plain, shape):
    check_stages(plain, reference(shape, mc.cases(*shape)))


# ---- ranks beyond 1024 chunks ------------------------------------------------------------------------------------------------
def test_frame_beyond_1024_chunks_then_another_geometry(plain):
    """the scan's second slab, an image base that is no multiple of 1024; then a small frame on the same handle"""
    check_stages(plain, reference("chunks", md.chunks_batch()))
    check_stages(plain, reference((37, 127), mc.cases(37, 127)))


# ---- mixed depths ------------------------------------------------------------------------------------------------------------
def test_mixed_depths_in_one_call_equal_the_single_image_results(plain):
    """images that finish after 1 to 3 launches are copied through for 70 more, across many ping-pong swaps"""
    batch = md.mixed_batch()
    ref = reference("mixed", batch)
    got = check_stages(plain, ref)
    for i, (name, m) in enumerate(batch):
        one = plain.debug_medial_stages(m[None])
        for k in KEYS[:4]:
            assert one[k][0].tobytes() == got[k][i].tobytes(), (name, k)
        assert one["launches"].tolist() == [md.expected_launches(ref["depths"][i])], name


# ---- per-tile flags of a recycled workspace ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["wake", "small"])
def test_repeat_and_poison_leave_every_output_unchanged(plain, which):
    """tile_final, tile_left and the progress ring are read before they are written: only thin_dev's memset stands between them and
    whatever a recycled block holds.  The workspace is a block of the handle's pool, which tmat_debug_poison fills and which hands the
    same block to the next call of the same size: without the memset every tile reads `final` and the call ends after 4 launches
    with the mask as its skeleton."""
    ref = reference("wake", md.wake_cases()[1:2]) if which == "wake" else reference((40, 129), mc.cases(40, 129))
    first = check_stages(plain, ref)
    assert_same_bytes(first, plain.debug_medial_stages(ref["mask"]), "second call")
    for pattern in (0xFF, 0x7F):
        plain.debug_poison(pattern)
        assert_same_bytes(first, plain.debug_medial_stages(ref["mask"]), f"after poison {pattern:#x}")


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_behave_as_medial_axis_batch(plain):
    from tmat_amd import _lib
    L = _lib.lib()
    m = np.ascontiguousarray(np.stack([mc.disc(5, 7, 2), mc.full(5, 7)]), np.uint8)
    shapes = {"skel": (m.shape, np.uint8), "dist": (m.shape, np.float64), "keys": (m.shape, np.uint64), "dep": (m.shape, np.uint8),
              "launches": ((1,), np.int32)}
    out = {k: np.full(s, 0x5A, d) for k, (s, d) in shapes.items()}
    ptrs = [_lib.ptr(out[k]) for k in KEYS]

    def both(h, mask, n, hh, ww):
        return (L.tmat_debug_medial_stages(h, mask, n, hh, ww, *ptrs), L.tmat_medial_axis_batch(h, mask, n, hh, ww, ptrs[0], ptrs[1]))

    assert both(None, _lib.ptr(m), 2, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, None, 2, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), 2, 0, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), -1, 5, 7) == (_lib.E_ARG, _lib.E_ARG)
    assert both(plain.raw, _lib.ptr(m), 0, 5, 7) == (0, 0)                        # nothing to do, nothing written
    assert all((v == 0x5A).all() for v in out.values())
    # too large for the 64-bit key (h^2 + w^2 >= 2^27): refused before anything is read
    assert both(plain.raw, _lib.ptr(m), 1, 1, 11586) == (_lib.E_ARG, _lib.E_ARG)
    assert b"too large" in L.tmat_last_error()
    assert all((v == 0x5A).all() for v in out.values())
    # no output at all
    none = [C.c_void_p()] * 5
    assert L.tmat_debug_medial_stages(plain.raw, _lib.ptr(m), 2, 5, 7, *none) == _lib.E_ARG
    assert b"bad argument" in L.tmat_last_error()
    # every single output alone is enough, and gives what the full call gives
    full = plain.debug_medial_stages(m)
    check_stages(plain, reference("args", [("disc", m[0].astype(bool)), ("full", m[1].astype(bool))]), full)
    for j, k in enumerate(KEYS):
        one = np.full(out[k].shape, 0x5A, out[k].dtype)
        args = [C.c_void_p()] * 5
        args[j] = _lib.ptr(one)
        assert L.tmat_debug_medial_stages(plain.raw, _lib.ptr(m), 2, 5, 7, *args) == 0, k
        assert one.tobytes() == full[k].tobytes(), k
