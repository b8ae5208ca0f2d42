"""GPU: the PNG encoder's compact mode on the device (png_stripe_kernel<true>) against the host twin in compact mode, byte
for byte, on every shape and content of tests/helpers/png_check.py; the way back to fast; the other entry points that encode; the
code lengths computed on the device against the host's; a model handle's rows around a compact encode; and the script with
--png-compression compact against pil and against fast."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib  # noqa: E402

import png_blocks as pb  # noqa: E402
import png_check as pc  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SCRIPT = REPO / "tissue-model-analysis-tools_amd" / "scripts" / "compute_branches.py"
S = _lib.png_stripe()
SHAPES = pc.shapes(S)


@pytest.fixture()
def compact():
    """a plain handle in compact mode"""
    h = _lib.Handle(None, 0)
    h.png_set_mode("compact")
    yield h
    h.close()


@pytest.fixture(scope="module")
def compact_shared():
    h = _lib.Handle(None, 0)
    h.png_set_mode("compact")
    yield h
    h.close()


@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_device_files_equal_the_host_twin_compact(compact_shared, shape_name):
    """all contents of one shape in one batched call, through the C entry with guard bytes behind every file"""
    L = _lib.lib()
    pics = np.stack([pc.content(k, SHAPES[shape_name], seed=len(shape_name)) for k in pc.CONTENTS])
    n, H, W = pics.shape[:3]
    ch = 3 if pics.ndim == 4 else 1
    cap = _lib.png_bound(H, W, ch) + 64
    out = np.full((n, cap), 0xA5, np.uint8)
    sizes = np.zeros(n, np.uintp)
    assert L.tmat_png_encode_batch(compact_shared.raw, _lib.ptr(pics), n, H, W, ch, _lib.ptr(out), cap, _lib.ptr(sizes)) == 0
    host = _lib.host_png_encode(pics, mode="compact")
    kinds = set()
    for i, k in enumerate(pc.CONTENTS):
        sz = int(sizes[i])
        d = out[i, :sz].tobytes()
        assert sz == len(host[i]) and d == host[i], (shape_name, k, sz, len(host[i]))
        assert (out[i, sz:] == 0xA5).all(), (shape_name, k)
        pc.check_png(d, pics[i])
        kinds |= set(pb.btypes(d))
    if shape_name == "640":
        assert kinds == {0, 1, 2} or kinds == {0, 2}, kinds          # stored (noise) and dynamic blocks both occur
    assert compact_shared.png_encode(pics[5])[0] == host[5]          # a file does not depend on its batch


def test_back_to_fast(compact):
    pics = np.stack([pc.content(k, SHAPES["2S+1"], seed=4) for k in pc.CONTENTS])
    assert compact.png_encode(pics) == _lib.host_png_encode(pics, mode="compact")
    compact.png_set_mode("fast")
    fast = compact.png_encode(pics)
    assert fast == _lib.host_png_encode(pics)
    assert all(2 not in pb.btypes(f) for f in fast)
    L = _lib.lib()
    for mode in (-1, 2):
        assert L.tmat_png_set_mode(compact.raw, mode) == _lib.E_ARG
    assert compact.png_encode(pics) == fast                          # a refused mode leaves the handle's
    with pytest.raises(ValueError):
        compact.png_set_mode("best")


def test_device_pointer_form_and_tree_overlay(compact):
    L = _lib.lib()
    pics = np.stack([pc.content(k, (33, 31, 3), seed=9) for k in ("noise", "blob", "smooth")])
    d = C.c_void_p()
    _lib.check(L.tmat_dev_alloc(compact.raw, pics.nbytes, C.byref(d)), "tmat_dev_alloc")
    try:
        _lib.check(L.tmat_dev_upload(compact.raw, d, _lib.ptr(pics), pics.nbytes), "tmat_dev_upload")
        got = compact.png_encode_dev(d, 3, 33, 31, 3)
    finally:
        L.tmat_dev_free(compact.raw, d)
    assert got == _lib.host_png_encode(pics, mode="compact")
    bg, tree = pc.synthetic_tree()
    bgs = np.stack([bg, bg[::-1].copy()])
    trees = [tree, (tree[0][:2], tree[1][:2])]
    ov = compact.render_tree(bgs, trees, 500)
    files = compact.render_tree_png(bgs, trees, 500)
    assert files == _lib.host_png_encode(ov, mode="compact")
    for f, o in zip(files, ov):
        pc.check_png(f, o)
    assert sum(map(len, files)) < sum(map(len, _lib.host_png_encode(ov)))
    bars = [np.array([[0.0, 0.5], [0.1, 0.9], [0.2, 0.25]])]
    bar_files = compact.render_barcode_png(bars, 300)
    assert bar_files == _lib.host_png_encode(_lib.host_render_barcode(bars[0], 300), mode="compact")


def test_code_lengths_on_the_device(compact):
    for limit in (15, 7):
        nmax = 286 if limit == 15 else 19
        hists = [f for _, f, lim in pb.direct_histograms() if lim == limit] + pb.random_histograms(limit)
        for n in sorted({len(f) for f in hists}):
            group = np.stack([f for f in hists if len(f) == n])
            if n > nmax or (1 << limit) < n:
                continue
            dev = compact.debug_png_code_lengths(group, limit)
            for f, lens in zip(group, dev):
                assert np.array_equal(lens, _lib.host_png_code_lengths(f, limit)), (limit, n)
                pb.check_lengths(f, limit, lens)
    L = _lib.lib()
    f = np.ones((2, 20), np.uint32)
    out = np.zeros((2, 20), np.uint8)
    assert L.tmat_debug_png_code_lengths(compact.raw, _lib.ptr(f), 2, 20, 4, _lib.ptr(out)) == _lib.E_ARG
    assert L.tmat_debug_png_code_lengths(compact.raw, _lib.ptr(f), 0, 20, 7, _lib.ptr(out)) == 0


def test_compact_encode_between_two_analyses_leaves_the_rows(handle):
    from tmat_amd import branches, synth
    imgs = np.stack([synth.synth_image(40 + i, 512, n_vessels=12, scale=1.0) for i in range(2)])
    cfg = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)
    first = branches.analyze_batch(handle, imgs, cfg, 500.0)
    pics = np.stack([pc.content(k, (320, 320), seed=1) for k in ("noise", "blob", "smooth")])
    handle.png_set_mode("compact")
    try:
        files = handle.png_encode(pics)
    finally:
        handle.png_set_mode("fast")
    assert files == _lib.host_png_encode(pics, mode="compact")
    again = branches.analyze_batch(handle, imgs, cfg, 500.0)
    assert again == first and first[0][1] > 0
    assert handle.png_encode(pics) == _lib.host_png_encode(pics)


def test_script_with_compact_compression(tmp_path):
    """--png-encoder device --png-compression compact: the file names of the pil run, every file the same pixels, the CSV byte for
    byte, and fewer PNG bytes in all than the same run with fast"""
    from PIL import Image
    from tmat_amd import synth
    ind = tmp_path / "in"
    ind.mkdir()
    for i in range(2):
        np.save(ind / f"img_{i}.npy", synth.synth_image(20 + i, 512, n_vessels=12, scale=1.0))
    env = dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1")
    outs = {}
    for name, extra in (("pil", ["--png-encoder", "pil"]), ("fast", ["--png-encoder", "device"]),
                        ("compact", ["--png-encoder", "device", "--png-compression", "compact"])):
        outs[name] = tmp_path / name
        r = subprocess.run([sys.executable, str(SCRIPT), str(ind), str(outs[name]), "--image-width-microns", "500", "--visualizations",
                            "--tree-visualizations", "--vis-width", "600"] + extra, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    names = {k: sorted(str(p.relative_to(outs[k])) for p in outs[k].rglob("*.png")) for k in outs}
    assert names["pil"] == names["compact"] == names["fast"] and len(names["pil"]) == 2 * 6, names
    total = {k: 0 for k in outs}
    for rel in names["pil"]:
        a, b = np.asarray(Image.open(outs["pil"] / rel)), np.asarray(Image.open(outs["compact"] / rel))
        assert a.shape == b.shape and np.array_equal(a, b), rel
        data = (outs["compact"] / rel).read_bytes()
        pc.check_png(data, b)
        assert data == _lib.host_png_encode(b, mode="compact")[0], rel
        for k in outs:
            total[k] += (outs[k] / rel).stat().st_size
    assert total["compact"] < total["fast"], total
    csv = {k: (outs[k] / "branching_analysis.csv").read_bytes() for k in outs}
    assert csv["pil"] == csv["compact"] == csv["fast"]
    r = subprocess.run([sys.executable, str(SCRIPT), str(ind), str(tmp_path / "bad"), "--image-width-microns", "500", "--png-compression", "compact"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 1 and "--png-encoder device" in r.stdout, r.stdout + r.stderr
