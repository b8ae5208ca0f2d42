"""CPU: the host side of the threshold-grid form (tmat_analyze_batch_grid) and of the device barcode (tmat_render_barcode) -- header and
exports, the struct's size, the call-size rule, the pair order, the argument checks that need no device, and the rectangle helper both
barcode rasterisers fill."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tmat_amd import _lib, branches

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "tmat.h"
NEW = ("tmat_analyze_batch_grid", "tmat_analyze_batch_grid_dev", "tmat_render_barcode", "tmat_render_barcode_png", "tmat_host_barcode_rects")


def test_header_declares_and_library_exports_the_new_symbols():
    text = HEADER.read_text()
    L = _lib.lib()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", text), name
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    assert "typedef struct tmat_grid_opts" in text


def test_grid_opts_size_matches_the_header(tmp_path):
    """sizeof(tmat_grid_opts) and the offsets of its fields as a C compiler sees the header = ctypes' layout"""
    src = tmp_path / "sz.c"
    fields = [f for f, _ in _lib.GridOpts._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmat.h"\nint main(void) { printf("%zu", sizeof(tmat_grid_opts));\n' +
                   "".join(f'printf(" %zu", offsetof(tmat_grid_opts, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.GridOpts)
    assert got[1:] == [getattr(_lib.GridOpts, f).offset for f in fields]


def test_grid_images_per_call_edges():
    f = branches.grid_images_per_call
    assert f(1, 1 << 30) == 1 and f(1, (1 << 30) + 1) == 1          # one picture of the budget's size, one larger than the budget
    assert f(9, 1 << 40) == 1
    assert f(1, 1 << 29) == 2 and f(2, 1 << 29) == 1 and f(3, 1 << 29) == 1
    assert f(4, 12_000_000) == (1 << 30) // 48_000_000 == 22
    assert f(4, 1000, budget=8000) == 2 and f(4, 1000, budget=7999) == 1 and f(4, 1000, budget=0) == 1
    assert f(25, 1) == (1 << 30) // 25


def test_pair_order_is_threshold_grid_order():
    cfg = dict(graph_thresh_1=[2, 5, 0.5], graph_thresh_2=[10, 4])
    want = [(c["thresh1"], c["thresh2"]) for c, _ in branches.threshold_grid(cfg)]
    assert want == [(2, 10), (2, 4), (5, 10), (5, 4), (0.5, 10), (0.5, 4)]
    assert branches.grid_pairs(cfg) == want
    # no image: no device call, the result still carries every pair, in order
    rows, extras = branches.analyze_batch_grid(None, np.zeros((0, 64, 64), np.uint16), cfg, 500.0, tree=True, vis_width=100, stage_pictures=True)
    assert list(rows) == want and all(v == [] for v in rows.values())
    assert list(extras["bars"]) == want and list(extras["overlays"]) == want
    assert extras["overlays"][want[0]].shape == (0, 100, 100, 3) and extras["pictures"].shape == (0, 4, 40, 40)
    explicit = [(7.0, 1.0), (3.0, 2.0)]
    assert list(branches.analyze_batch_grid(None, np.zeros((0, 64, 64), np.uint16), cfg, 500.0, pairs=explicit)[0]) == explicit
    assert branches.grid_pairs({}) == [(5, 10)]


def test_null_handle_and_bad_opts_are_refused_without_a_device():
    L = _lib.lib()
    imgs = np.zeros((1, 64, 64), np.uint16)
    rows = (_lib.Row * 4)()
    for r in rows:
        r.index = -7
    thresh = np.array([[5, 10], [2, 10]], np.float32)
    o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts), ds_ratio=0.625, ds_width=384)
    g = _lib.GridOpts(size=C.sizeof(_lib.GridOpts), n_thresh=2, thresh=thresh.ctypes.data)
    for fn in (L.tmat_analyze_batch_grid, L.tmat_analyze_batch_grid_dev):
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(o), C.byref(g), rows) == _lib.E_ARG                  # NULL handle
        bad_o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts) - 8, ds_ratio=0.625, ds_width=384)
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(bad_o), C.byref(g), rows) == _lib.E_ARG
        bad_g = _lib.GridOpts(size=C.sizeof(_lib.GridOpts) + 8, n_thresh=2, thresh=thresh.ctypes.data)
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(o), C.byref(bad_g), rows) == _lib.E_ARG
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, None, C.byref(g), rows) == _lib.E_ARG
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(o), None, rows) == _lib.E_ARG
    for fn in (L.tmat_analyze_batch_ex, L.tmat_analyze_batch_ex_dev):
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(o), rows) == _lib.E_ARG                              # NULL handle
        bad_o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts) - 8, ds_ratio=0.625, ds_width=384)
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, C.byref(bad_o), rows) == _lib.E_ARG
        assert fn(None, _lib.ptr(imgs), 1, 64, 64, None, rows) == _lib.E_ARG
    # the five positional entries with a NULL handle
    positional = (1, 64, 64, 0.625, 384, 5.0, 10.0, 12, 12, 0, 0, 0)
    rgb, bars, nb = np.zeros((1, 100, 100, 3), np.uint8), np.zeros((1, 8, 2)), np.zeros(1, np.int32)
    tree = (100, _lib.ptr(rgb), _lib.ptr(bars), 8, _lib.ptr(nb))
    assert L.tmat_analyze_batch(None, _lib.ptr(imgs), *positional, rows) == _lib.E_ARG
    assert L.tmat_analyze_batch_dev(None, _lib.ptr(imgs), *positional, rows) == _lib.E_ARG
    assert L.tmat_analyze_batch_masked(None, _lib.ptr(imgs), *positional, None, None, rows) == _lib.E_ARG
    assert L.tmat_analyze_batch_tree(None, _lib.ptr(imgs), *positional, rows, *tree) == _lib.E_ARG
    assert L.tmat_analyze_batch_tree_dev(None, _lib.ptr(imgs), *positional, rows, *tree) == _lib.E_ARG
    assert all(r.index == -7 for r in rows)
    assert L.tmat_render_barcode(None, None, _lib.ptr(np.zeros(1, np.int32)), 0, 100, _lib.ptr(np.zeros(4, np.uint8))) == _lib.E_ARG


def barcode_cases():
    """{name: (bars (n, 2), vis_width)}: n in {0, 1, 2, 37, 300} at widths {20, 333, 1000} (300 bars at width 20: more bars than the 18
    rows), equal births (the stable order decides the rows), a zero span, births above deaths mixed in"""
    rs = np.random.RandomState(11)
    out = {}
    for n in (0, 1, 2, 37, 300):
        for vw in (20, 333, 1000):
            b = np.stack([rs.uniform(0, 40, n), rs.uniform(40, 90, n)], axis=1)
            if n >= 37:
                b[::5, 0] = b[0, 0]                     # equal births
                b[3, 1] = b[3, 0] - 5.0                 # death in front of birth: an empty rectangle
            out[f"n{n}_w{vw}"] = (b, vw)
    out["zero_span"] = (np.full((4, 2), 3.25), 333)
    out["all_equal_births"] = (np.stack([np.full(9, 2.0), np.arange(9) + 3.0], axis=1), 333)
    out["odd_width"] = (np.stack([rs.uniform(-5, 5, 11), rs.uniform(5, 6, 11)], axis=1), 57)
    return out


BARCODE_CASES = barcode_cases()


def fill_rects(rects, S):
    """numpy restatement of the fill both rasterisers do"""
    pic = np.full((S, S, 3), 255, np.uint8)
    for xa, xb, ya, yb, rgb in rects:
        if ya < yb and xa < xb:
            pic[S - yb: S - ya, xa:xb] = [rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255]
    return pic


@pytest.mark.parametrize("name", list(BARCODE_CASES))
def test_rectangle_helper_reproduces_the_host_barcode(name):
    bars, vw = BARCODE_CASES[name]
    pic = _lib.host_render_barcode(bars, vw)
    rects = _lib.host_barcode_rects(bars, vw)
    S = pic.shape[0]
    assert S == int(round(0.9 * vw))
    assert len(rects) in (0, len(bars))
    if name == "zero_span" or len(bars) == 0:
        assert len(rects) == 0 and (pic == 255).all()
    assert np.array_equal(fill_rects(rects, S), pic)
    if len(rects):
        # what the kernel's index arithmetic relies on: bar k's rows lie inside [k pitch, (k + 1) pitch) and inside the canvas, in order
        pitch = S / len(rects)
        k = np.arange(len(rects))
        assert (rects[:, 2] >= np.floor(k * pitch)).all() and (rects[:, 3] <= np.ceil((k + 1) * pitch)).all()
        assert (rects[:, 2] >= 0).all() and (rects[:, 3] <= S).all() and (rects[1:, 2] >= rects[:-1, 3]).all()
        assert (rects[:, 0] >= 0).all() and (rects[:, 1] <= S).all()
        # the colour of entry k is the colour of the bar the stable sort by birth, descending, puts on row k
        order = np.argsort(-bars[:, 0], kind="stable")
        col = np.zeros(3, np.uint8)
        for row in (0, len(rects) - 1):
            _lib.check(_lib.lib().tmat_branch_color(int(order[row]), _lib.ptr(col)))
            assert int(rects[row, 4]) == int(col[0]) | int(col[1]) << 8 | int(col[2]) << 16
