"""GPU: the PNG encoder on the device (csrc/png_kernels.hip) against its host twin, byte for byte, and against the two
independent decoders of tests/helpers/png_check.py; tmat_render_tree_png; the guard bytes; a model handle that encodes between two
analyses; and scripts/compute_branches.py with --png-encoder device against the same run with pil."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib  # noqa: E402

import png_check as pc  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SCRIPT = REPO / "tissue-model-analysis-tools_amd" / "scripts" / "compute_branches.py"
S = _lib.png_stripe()
SHAPES = pc.shapes(S)


@pytest.fixture(scope="module")
def plain():
    h = _lib.Handle(None, 0)
    yield h
    h.close()


@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_device_files_equal_the_host_twin(plain, shape_name):
    """all contents of one shape in one batched call: device bytes == host bytes, and both decoders return the pictures"""
    pics = np.stack([pc.content(k, SHAPES[shape_name], seed=len(shape_name)) for k in pc.CONTENTS])
    dev = plain.png_encode(pics)
    host = _lib.host_png_encode(pics)
    assert len(dev) == len(pics)
    for k, d, h, p in zip(pc.CONTENTS, dev, host, pics):
        assert len(d) == len(h) and d == h, (shape_name, k, len(d), len(h))
        pc.check_png(d, p)
    assert plain.png_encode(pics) == dev                 # the same call twice
    assert plain.png_encode(pics[3])[0] == dev[3]        # a file does not depend on its batch


def test_device_pointer_form(plain):
    L = _lib.lib()
    pics = np.stack([pc.content(k, (33, 31, 3), seed=9) for k in ("noise", "blob", "smooth")])
    d = C.c_void_p()
    _lib.check(L.tmat_dev_alloc(plain.raw, pics.nbytes, C.byref(d)), "tmat_dev_alloc")
    try:
        _lib.check(L.tmat_dev_upload(plain.raw, d, _lib.ptr(pics), pics.nbytes), "tmat_dev_upload")
        got = plain.png_encode_dev(d, 3, 33, 31, 3)
    finally:
        L.tmat_dev_free(plain.raw, d)
    assert got == _lib.host_png_encode(pics)
    for f, p in zip(got, pics):
        pc.check_png(f, p)


def test_render_tree_png_decodes_to_render_tree(plain):
    from PIL import Image
    import io
    bg, tree = pc.synthetic_tree()
    bgs = np.stack([bg, bg[::-1].copy()])
    trees = [tree, (tree[0][:2], tree[1][:2])]
    ov = plain.render_tree(bgs, trees, 500)
    files = plain.render_tree_png(bgs, trees, 500)
    assert ov.shape[2] == 500 and len(files) == 2
    for f, o in zip(files, ov):
        pc.check_png(f, o)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), o)
    assert files == _lib.host_png_encode(ov)
    assert files == plain.render_tree_png(bgs, trees, 500)


def test_bytes_past_each_file_are_untouched_and_error_codes(plain):
    L = _lib.lib()
    pics = np.stack([pc.content(k, SHAPES["2S+1"], seed=2) for k in ("noise", "constant", "smooth")])
    n, H, W = pics.shape
    bound = _lib.png_bound(H, W, 1)
    cap = bound + 100
    out = np.full((n, cap), 0xA5, np.uint8)
    sizes = np.zeros(n, np.uintp)
    assert L.tmat_png_encode_batch(plain.raw, _lib.ptr(pics), n, H, W, 1, _lib.ptr(out), cap, _lib.ptr(sizes)) == 0
    host = _lib.host_png_encode(pics)
    for i in range(n):
        k = int(sizes[i])
        assert out[i, :k].tobytes() == host[i]
        assert (out[i, k:] == 0xA5).all()
    out[:] = 0xA5
    assert L.tmat_png_encode_batch(plain.raw, _lib.ptr(pics), n, H, W, 1, _lib.ptr(out), bound - 1, _lib.ptr(sizes)) == _lib.E_CAP
    assert (out == 0xA5).all()
    for hh, ww, ch in ((0, W, 1), (H, 0, 1), (H, W, 2)):
        assert L.tmat_png_encode_batch(plain.raw, _lib.ptr(pics), n, hh, ww, ch, _lib.ptr(out), cap, _lib.ptr(sizes)) == _lib.E_ARG
    assert (out == 0xA5).all()
    assert L.tmat_png_encode_batch(plain.raw, None, 0, H, W, 1, _lib.ptr(out), cap, _lib.ptr(sizes)) == 0
    assert plain.png_encode(np.zeros((0, 4, 4), np.uint8)) == []


def test_a_handle_that_never_encodes_holds_nothing_for_it():
    h = _lib.Handle(None, 0)
    try:
        before = h.debug_held_bytes()
        files = h.png_encode(pc.content("smooth", (40, 50)))
        pc.check_png(files[0], pc.content("smooth", (40, 50)))
        after = h.debug_held_bytes()
    finally:
        h.close()
    assert after[0] > before[0], (before, after)         # the encoder's blocks appear in the pool with the first call, not before


def test_encoding_between_two_analyses_leaves_the_rows(handle):
    from tmat_amd import branches, synth
    imgs = np.stack([synth.synth_image(40 + i, 512, n_vessels=12, scale=1.0) for i in range(2)])
    cfg = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)
    first = branches.analyze_batch(handle, imgs, cfg, 500.0)
    pics = np.stack([pc.content(k, (320, 320), seed=1) for k in ("noise", "blob")])
    files = handle.png_encode(pics)
    assert files == _lib.host_png_encode(pics)
    again = branches.analyze_batch(handle, imgs, cfg, 500.0)
    assert again == first and first[0][1] > 0


def test_script_with_the_device_encoder(tmp_path):
    """--visualizations --tree-visualizations with --png-encoder device: the file names of the pil run, every file the same pixels,
    the CSV byte for byte"""
    from PIL import Image
    from tmat_amd import synth
    ind = tmp_path / "in"
    ind.mkdir()
    for i in range(3):
        np.save(ind / f"img_{i}.npy", synth.synth_image(20 + i, 512, n_vessels=12, scale=1.0))
    env = dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1")
    outs = {}
    for enc in ("pil", "device"):
        outs[enc] = tmp_path / enc
        r = subprocess.run([sys.executable, str(SCRIPT), str(ind), str(outs[enc]), "--image-width-microns", "500", "--visualizations",
                            "--tree-visualizations", "--vis-width", "600", "--png-encoder", enc], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    names = {enc: sorted(str(p.relative_to(outs[enc])) for p in outs[enc].rglob("*.png")) for enc in outs}
    assert names["pil"] == names["device"] and len(names["pil"]) == 3 * 6, names
    for rel in names["pil"]:
        a, b = np.asarray(Image.open(outs["pil"] / rel)), np.asarray(Image.open(outs["device"] / rel))
        assert a.shape == b.shape and np.array_equal(a, b), rel
        pc.check_png((outs["device"] / rel).read_bytes(), b)
    assert (outs["pil"] / "branching_analysis.csv").read_bytes() == (outs["device"] / "branching_analysis.csv").read_bytes()
