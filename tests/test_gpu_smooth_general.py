"""GPU: smooth tiling as a device stage around any predictor (csrc/smooth_kernels.hip: tmat_smooth_begin / _tiles / _put / _end,
tmat_predict_smooth_ex) -- bit for bit against tests/golden/smooth_general.npz, which the imported reference driver made (cases:
tests/helpers/smooth_cases.py), with the log of predictor calls equal to the reference's; and tied to the subdivisions = 2 kernels of
csrc/blend_kernels.hip through the library's own network.  The process never imports torch."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import smooth_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(Path(__file__).parent / "golden" / "smooth_general.npz")


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def same_bits(got, ref, what):
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape)
    nbad = int((got.view(np.uint64) != ref.view(np.uint64)).sum())
    print(f"{what}: {nbad} of {got.size} outputs differ", flush=True)
    assert nbad == 0, f"{what}: {nbad} of {got.size} outputs differ, max |d| = {np.abs(got - ref).max()}"


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_mirror_with_handle_matches_the_reference(plain, name, poison):
    from tmat_amd import _lib, smooth_tiled_predictions as stp
    _, _, ws, sub, _ = sc.CASES[sc.NAMES.index(name)]
    if poison:
        _lib.check(_lib.lib().tmat_debug_poison(plain.raw, 0xFF), "poison")
    pred = sc.predictor_of(name)
    got = stp.predict_img_with_smooth_windowing(G[name + "_in"], ws, sub, pred, handle=plain)
    same_bits(got, G[name + "_out"], name)
    shapes, sha = pred.log()
    assert np.array_equal(shapes, G[name + "_calls"]), "the predictor was not called as the reference calls it"
    assert np.array_equal(sha, G[name + "_calls_sha256"]), "the batches differ from the reference's"


def test_identity_case_has_the_reference_error(plain):
    from tmat_amd import smooth_tiled_predictions as stp
    img = G["identity_in"]
    got = stp.predict_img_with_smooth_windowing(img, 16, 4, sc.predictor_of("identity"), handle=plain)
    assert float(np.abs(got - img).max()) == float(G["identity_maxerr"])


def test_module_level_handle_serves_the_four_argument_call(plain):
    from tmat_amd import smooth_tiled_predictions as stp
    stp.use_handle(plain)
    try:
        got = stp.predict_img_with_smooth_windowing(G["s3_in"], 12, 3, sc.predictor_of("s3"))
    finally:
        stp.use_handle(None)
    same_bits(got, G["s3_out"], "use_handle")
    with pytest.raises(TypeError, match="handle="):
        stp.predict_img_with_smooth_windowing(G["s3_in"], 12, 3, sc.predictor_of("s3"))


def test_wrong_result_shape_is_a_type_error(plain):
    from tmat_amd import smooth_tiled_predictions as stp
    with pytest.raises(TypeError):
        stp.predict_img_with_smooth_windowing(G["s3_in"], 12, 3, lambda b, verbose=0: b, handle=plain)
    with pytest.raises(TypeError):
        stp.predict_img_with_smooth_windowing(G["s3_in"], 12, 3, lambda b, verbose=0: np.repeat(b[..., None], 2, -1), handle=plain)


def test_tiles_in_uneven_ranges_equal_one_range(plain):
    n = plain.smooth_begin(G["step_rest_in"], 16, 3)
    assert n == int(G["step_rest_geom"][8])
    whole = plain.smooth_tiles(0, n)
    a, b = plain.smooth_tiles(0, 7), plain.smooth_tiles(7, n - 7)       # the first range ends inside orientation 0
    assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32))
    c = plain.smooth_tiles(n - 3, 3)
    assert np.array_equal(c.view(np.uint32), whole[-3:].view(np.uint32))
    # the first tile of orientation 0 is the top left corner of the padded image: the pad value, then the image
    aug = int(G["step_rest_geom"][2])
    img = G["step_rest_in"]
    assert np.all(whole[0][:aug, :] == img.min()) and np.array_equal(whole[0][aug:, aug:], img[:16 - aug, :16 - aug])


def test_dtype_change_widens_and_changes_no_bit(plain):
    """a predictor that answers float32 first and float64 or float32 in turn later: the stored results are widened"""
    from tmat_amd import smooth_tiled_predictions as stp
    base = sc.predictor_of("s4")
    calls = []

    def mixed(batch, verbose=0):
        r = base(batch, verbose=verbose)
        calls.append(len(calls))
        return r if len(calls) <= 5 else r.astype(np.float64) if len(calls) % 2 else r.astype(np.float32)
    got = stp.predict_img_with_smooth_windowing(G["s4_in"], 16, 4, mixed, handle=plain)
    same_bits(got, G["s4_out"], "mixed dtypes")


def test_session_argument_checks_and_recovery(plain):
    from tmat_amd import _lib
    L = _lib.lib()
    img = G["s3_in"]
    out = np.empty(img.shape, np.float64)
    assert L.tmat_smooth_end(plain.raw, _lib.ptr(out)) == _lib.E_ARG, "end without a session"
    n = plain.smooth_begin(img, 12, 3)
    tiles = plain.smooth_tiles(0, n)
    pred = sc.predictor_of("s3")
    res = np.concatenate([pred(tiles[i:i + 16]) for i in range(0, n, 16)])
    buf = np.zeros((4, 12, 12), np.float32)
    for first, count in ((-1, 2), (n - 1, 2), (n, 1), (0, n + 1), (0, -1)):
        assert L.tmat_smooth_tiles(plain.raw, first, count, _lib.ptr(buf)) == _lib.E_ARG, (first, count)
        assert L.tmat_smooth_put(plain.raw, first, count, _lib.ptr(buf), 0) == _lib.E_ARG, (first, count)
    assert L.tmat_smooth_put(plain.raw, 0, 1, _lib.ptr(buf), 7) == _lib.E_ARG, "unknown dtype"
    plain.smooth_put(0, res[:n - 5])
    assert L.tmat_smooth_end(plain.raw, _lib.ptr(out)) == _lib.E_ARG, "five tiles were never put"
    assert b"never put" in L.tmat_last_error()
    # a float32 put into a float64 session is refused
    plain.smooth_begin(img, 12, 3)                  # a second begin discards the open session
    plain.smooth_put(0, res[:3].astype(np.float64))
    assert L.tmat_smooth_put(plain.raw, 3, 1, _lib.ptr(np.ascontiguousarray(res[3:4, ..., 0])), 0) == _lib.E_ARG
    # ... and the handle still serves the next session; the puts may come in any order
    from tmat_amd import smooth_tiled_predictions as stp
    want = stp.predict_img_with_smooth_windowing(img, 12, 3, sc.predictor_of("s3"), handle=plain)
    same_bits(want, G["s3_out"], "session after the refusals")
    plain.smooth_begin(img, 12, 3)
    plain.smooth_put(n - 5, res[n - 5:])
    plain.smooth_put(0, res[:n - 5])
    same_bits(plain.smooth_end(img.shape), G["s3_out"], "puts in reverse order")
    assert L.tmat_smooth_tiles(plain.raw, 0, 1, _lib.ptr(buf)) == _lib.E_ARG, "end released the session"


def test_session_around_the_device_model_equals_predict_smooth(handle):
    """ties the general kernels to blend_kernels.hip: 100 x 90, the default synthetic model, 8 patches"""
    from tmat_amd import models, smooth_tiled_predictions as stp
    x = np.random.RandomState(8).uniform(0, 1, (100, 90)).astype(np.float32)
    model = models._DeviceModel(handle, 320)
    want = handle.predict_smooth(x)
    got = stp.predict_img_with_smooth_windowing(x, 320, 2, lambda b, verbose=0: model.predict(b), handle=handle)
    same_bits(got, want, "session vs predict_smooth")
    same_bits(handle.predict_smooth_ex(x, 2), want, "predict_smooth_ex at 2 vs predict_smooth")
    same_bits(stp.predict_img_with_smooth_windowing(x, 320, 2, model.predict), want, "device model through the mirror")


def test_predict_smooth_ex_at_4_equals_the_session_route():
    """40 x 30, the (16, 32, 64, 128) synthetic model: 72 patches, through a workspace of 32 (three chunks)"""
    from tmat_amd import _lib, models, synth, smooth_tiled_predictions as stp
    h = _lib.Handle(synth.pack_weights(synth.synth_weights(0, filter_counts=(16, 32, 64, 128))), 0, 32)
    try:
        x = np.random.RandomState(9).uniform(0, 1, (40, 30)).astype(np.float32)
        model = models._DeviceModel(h, 320)
        assert _lib.smooth_plan(40, 30, 320, 4)[3] == 72
        got = h.predict_smooth_ex(x, 4)
        want = stp.predict_img_with_smooth_windowing(x, 320, 4, lambda b, verbose=0: model.predict(b), handle=h)
        same_bits(got, want, "predict_smooth_ex vs session")
        same_bits(stp.predict_img_with_smooth_windowing(x, 320, 4, model.predict), want, "device model through the mirror")
        assert float(np.abs(want).max()) > 0 and np.isfinite(want).all()
        # the input norm applies as in predict_smooth
        h.set_input_norm(0.4, 0.3)
        try:
            normed = h.predict_smooth_ex(x, 4)
        finally:
            h.set_input_norm(None, None)
        xn = ((x - np.float32(0.4)) / np.float32(0.3)).astype(np.float32)
        same_bits(normed, h.predict_smooth_ex(xn, 4), "input norm")
        with pytest.raises(_lib.TmatError, match=r"\(-1\)"):
            h.predict_smooth_ex(x, 1)
    finally:
        h.close()


def test_predict_smooth_ex_refuses_a_plain_handle(plain):
    from tmat_amd import _lib
    with pytest.raises(_lib.TmatError, match="no model"):
        plain.predict_smooth_ex(np.zeros((10, 10), np.float32), 4)
