"""CPU: the host entry points of the general smooth-tiling stage (tmat_smooth_plan, tmat_spline_window) and oracle/blend.py against
tests/golden/smooth_general.npz, which tools/make_goldens.py:gen_smooth_general made from the imported reference driver at subdivisions
2, 3 and 4, odd windows and steps that do not divide the frame (cases: tests/helpers/smooth_cases.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import smooth_cases as sc  # noqa: E402

from oracle import blend  # noqa: E402
from tmat_amd import _lib  # noqa: E402

G = np.load(Path(__file__).parent / "golden" / "smooth_general.npz")


def test_fixture_lists_the_cases():
    assert [str(n) for n in G["names"]] == sc.NAMES
    for name in sc.NAMES:
        assert np.array_equal(G[name + "_in"], sc.case_image(name))


@pytest.mark.parametrize("name", sc.NAMES)
def test_plan_matches_the_reference_geometry(name):
    ws, sub, aug, step, na0, nb0, na1, nb1, n_tiles, n_calls = (int(v) for v in G[name + "_geom"])
    hh, ww = G[name + "_in"].shape
    got = _lib.smooth_plan(hh, ww, ws, sub)
    assert got == (aug, step, (na0, nb0, na1, nb1), n_tiles)
    # the calls of :174-182: per orientation chunks of 16 when it has more than 16 tiles, otherwise one call
    calls = sum(-(-(got[2][2 * (g & 1)] * got[2][2 * (g & 1) + 1]) // 16) for g in range(8))
    assert calls == n_calls == len(G[name + "_calls"])


def test_plan_rounds_halves_to_even():
    assert _lib.smooth_plan(9, 14, 6, 4)[0] == 4           # 4.5
    assert _lib.smooth_plan(17, 11, 10, 4)[0] == 8         # 7.5
    assert _lib.smooth_plan(10, 10, 320, 2)[:2] == (160, 160)
    assert _lib.smooth_plan(640, 640, 320, 4)[3] == 968


@pytest.mark.parametrize("ws", sc.WINDOWS)
def test_spline_window_bitexact(ws):
    win = _lib.spline_window(ws)
    ref = G[f"window{ws}"]
    assert win.dtype == ref.dtype and np.array_equal(win.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(blend.spline_window(ws).view(np.uint64), ref.view(np.uint64))


def test_spline_window_320_is_the_handle_window():
    assert np.array_equal(_lib.spline_window(320), np.load(Path(__file__).parent / "golden" / "blend.npz")["window320"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_blend_bitexact(name):
    _, _, ws, sub, _ = sc.CASES[sc.NAMES.index(name)]
    pred = sc.predictor_of(name)
    r = blend.predict_img_with_smooth_windowing(G[name + "_in"], ws, sub, pred)
    assert np.array_equal(r.view(np.uint64), G[name + "_out"].view(np.uint64))
    shapes, sha = pred.log()
    assert np.array_equal(shapes, G[name + "_calls"]) and np.array_equal(sha, G[name + "_calls_sha256"])


def test_identity_case_error_is_stored():
    assert float(G["identity_maxerr"]) == float(np.abs(G["identity_out"] - G["identity_in"]).max())
    assert float(G["identity_maxerr"]) <= 2 ** -50         # a few f64 ulps of values below 1


@pytest.mark.parametrize("args", [(10, 10, 3, 2), (10, 10, 16, 1), (10, 10, 16, 0), (10, 10, 8, 9), (0, 10, 16, 2), (10, 0, 16, 2),
                                  (10, -1, 16, 4), (10, 10, -16, 2)])
def test_plan_refuses(args):
    with pytest.raises(_lib.TmatError, match=r"\(-1\)"):
        _lib.smooth_plan(*args)


def test_spline_window_refuses():
    for ws in (3, 0, -5):
        with pytest.raises(_lib.TmatError, match=r"\(-1\)"):
            _lib.spline_window(ws)
    import ctypes as C
    assert _lib.lib().tmat_spline_window(16, C.c_void_p()) == _lib.E_ARG


def test_session_calls_refuse_a_null_handle():
    import ctypes as C
    L = _lib.lib()
    buf = np.zeros(16, np.float64)
    n = C.c_int(0)
    assert L.tmat_smooth_begin(C.c_void_p(), _lib.ptr(buf), 2, 2, 16, 2, C.byref(n)) == _lib.E_ARG
    assert L.tmat_smooth_tiles(C.c_void_p(), 0, 1, _lib.ptr(buf)) == _lib.E_ARG
    assert L.tmat_smooth_put(C.c_void_p(), 0, 1, _lib.ptr(buf), 0) == _lib.E_ARG
    assert L.tmat_smooth_end(C.c_void_p(), _lib.ptr(buf)) == _lib.E_ARG
    assert L.tmat_predict_smooth_ex(C.c_void_p(), _lib.ptr(buf), 1, 2, 2, 4, _lib.ptr(buf)) == _lib.E_ARG


def test_mirror_names_the_handle_argument_without_one():
    from tmat_amd import smooth_tiled_predictions as stp
    stp.use_handle(None)
    with pytest.raises(TypeError, match="handle="):
        stp.predict_img_with_smooth_windowing(np.zeros((10, 10), np.float32), 16, 4, lambda b, verbose=0: b[..., None])
