"""CPU: tmat_host_resize_pil_f32, the host twin of the device resize behind predict(x, auto_resample=True), bit for bit against
tests/golden/pil_resize.npz (Pillow's own results, tools/make_goldens.py:gen_pil_resize), against Pillow itself where it imports, and
against the Python restatement of tests/helpers/pil_resize_ref.py."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import pil_resize_ref as pr  # noqa: E402

from tmat_amd import _lib  # noqa: E402

G = np.load(Path(__file__).parent / "golden" / "pil_resize.npz")
CASES = pr.cases()
IDS = [c[0] for c in CASES]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def test_fixture_lists_the_cases():
    assert [str(k) for k in G["keys"]] == IDS
    for shape in pr.SHAPES:
        assert np.array_equal(sha(pr.case_input(shape)), G[f"in_{shape[0]}x{shape[1]}_sha256"])
    # the shapes and ratios asked for, both filters
    assert {c[1] for c in CASES} == {(37, 23), (75, 130), (64, 64)} and {c[3] for c in CASES} == {"lanczos", "nearest"}


@pytest.mark.parametrize("key, shape, tgt, flt", CASES, ids=IDS)
def test_host_twin_equals_the_stored_pillow_result(key, shape, tgt, flt):
    got = _lib.host_resize_pil_f32(pr.case_input(shape), tgt, flt)
    assert got.shape == tgt and got.dtype == np.float32
    if key + "_out" in G.files:
        ref = G[key + "_out"]
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert np.array_equal(sha(got), G[key + "_sha256"])


@pytest.mark.parametrize("key, shape, tgt, flt", CASES, ids=IDS)
def test_host_twin_equals_pillow_itself(key, shape, tgt, flt):
    Image = pytest.importorskip("PIL.Image")
    x = pr.case_input(shape)
    ref = np.array(Image.fromarray(x).resize(tgt[::-1], resample={"lanczos": Image.Resampling.LANCZOS, "nearest": Image.Resampling.NEAREST}[flt]))
    got = _lib.host_resize_pil_f32(x, tgt, flt)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("key, shape, tgt, flt", [c for c in CASES if c[1] == (37, 23)], ids=[c[0] for c in CASES if c[1] == (37, 23)])
def test_python_restatement_equals_the_stored_pillow_result(key, shape, tgt, flt):
    got = pr.resize(pr.case_input(shape), tgt, flt)
    assert np.array_equal(got.view(np.uint32), G[key + "_out"].view(np.uint32))


def test_batch_form_and_identity():
    x = np.stack([pr.case_input((37, 23)), pr.case_input((37, 23))[::-1]])
    got = _lib.host_resize_pil_f32(x, (23, 14), "lanczos")
    for i in range(2):
        assert np.array_equal(got[i], _lib.host_resize_pil_f32(x[i], (23, 14), "lanczos"))
    for flt in pr.FILTERS:
        assert np.array_equal(_lib.host_resize_pil_f32(x, (37, 23), flt), x)


def test_refusals():
    x = np.zeros((4, 4), np.float32)
    L = _lib.lib()
    out = np.zeros(64, np.float32)
    for args in ((1, 0, 4, 2, 2, 1), (1, 4, 4, 0, 2, 1), (1, 4, 4, 2, 2, 5), (-1, 4, 4, 2, 2, 0), (1, 4, 4, 2, 40000, 0)):
        assert L.tmat_host_resize_pil_f32(_lib.ptr(x), *args, _lib.ptr(out)) == _lib.E_ARG, args
    assert L.tmat_host_resize_pil_f32(None, 1, 4, 4, 2, 2, 1, _lib.ptr(out)) == _lib.E_ARG
