"""CPU: branch geometry (tmat_morse_tree) against the reference-generated fixture tests/golden/morse_tree.npz, the branch colour, and the
host twins of the tree overlay and barcode rasterisers against their numpy restatements (tests/helpers/tree_raster_ref.py), byte for byte."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from make_goldens import MORSE_CASES, prune_mask
from make_tree_goldens import TREE_FIELDS, TREE_SCALES, tree_fields
from tmat_amd import _lib

import tree_raster_ref as ref

GT = np.load(Path(__file__).parent / "golden" / "morse_tree.npz")
FIELDS = tree_fields()
_GRAPHS = {}


def graph(name, ci):
    d1, d2 = MORSE_CASES[ci][:2]
    key = (name, d1, d2)
    if key not in _GRAPHS:
        _GRAPHS[key] = _lib.dmt_graph(FIELDS[name], d1, d2)
    return _GRAPHS[key]


def tree(name, ci, sf):
    _, _, sw, mn, mx, iso, um = MORSE_CASES[ci]
    V, E = graph(name, ci)
    f = FIELDS[name]
    return _lib.morse_tree(V, E, f.shape, sw, mn, mx, iso, prune_mask(f.shape) if um else None, sf)


def test_fixture_covers_what_it_must():
    assert str(GT["numpy_version"])
    keys = [k for k in GT.files if k.endswith("_segs")]
    assert len(keys) == len(TREE_FIELDS) * len(MORSE_CASES) * len(TREE_SCALES) >= 24
    assert any(MORSE_CASES[c][6] for c in range(len(MORSE_CASES))) and any(MORSE_CASES[c][5] for c in range(len(MORSE_CASES)))
    assert sum(len(GT[k]) for k in keys) > 1000


@pytest.mark.parametrize("name", TREE_FIELDS)
@pytest.mark.parametrize("ci", range(len(MORSE_CASES)))
def test_morse_tree_equals_the_reference_fixture(name, ci):
    _, _, sw, mn, mx, iso, um = MORSE_CASES[ci]
    V, E = graph(name, ci)
    f = FIELDS[name]
    pm = prune_mask(f.shape) if um else None
    bars0, n0, tot0, avg0 = _lib.morse_stats(V, E, f.shape, sw, mn, mx, iso, pm)
    for sname, sf in TREE_SCALES:
        segs, sb, bars, n, tot, avg = tree(name, ci, sf)
        key = f"{name}_c{ci}_{sname}"
        assert np.array_equal(segs, GT[key + "_segs"].astype(np.float64))
        assert np.array_equal(sb, GT[key + "_branch"])
        assert np.array_equal(bars, GT[key + "_bars"].astype(np.float64))
        assert (n, tot, avg) == (n0, tot0, avg0) and n == len(bars)
        assert np.array_equal(bars, bars0 * sf)
        if name == "zero":
            assert len(segs) == 0 and len(bars) == 0


def test_morse_tree_reports_capacity_errors():
    V, E = graph("s96", 0)
    _, _, sw, mn, mx, iso, _ = MORSE_CASES[0]
    segs, sb, bars, n, _, _ = tree("s96", 0, 1.0)
    assert len(segs) > 4 and len(bars) > 1
    L = _lib.lib()
    cnt, tot, avg, ns, nb = C.c_int64(), C.c_double(), C.c_double(), C.c_int(), C.c_int()

    def call(cap_s, cap_b):
        s_, b_, k_ = np.empty((max(cap_s, 1), 4)), np.empty(max(cap_s, 1), np.int32), np.empty((max(cap_b, 1), 2))
        return L.tmat_morse_tree(_lib.ptr(V), len(V), _lib.ptr(E), len(E), 96, 96, sw, mn, 0, int(iso), None, 1.0, C.byref(cnt), C.byref(tot),
                                 C.byref(avg), _lib.ptr(s_), _lib.ptr(b_), cap_s, _lib.ptr(k_), cap_b, C.byref(ns), C.byref(nb))

    assert call(len(segs) - 1, len(bars)) == -4 and (ns.value, nb.value) == (len(segs), len(bars))      # TMAT_E_CAP
    assert call(len(segs), len(bars) - 1) == -4
    assert call(len(segs), len(bars)) == 0
    bad = E.copy(); bad[0, 0] = len(V)
    assert L.tmat_morse_tree(_lib.ptr(V), len(V), _lib.ptr(bad), len(bad), 96, 96, sw, mn, 0, 0, None, 1.0, C.byref(cnt), C.byref(tot), C.byref(avg),
                             None, None, 0, None, 0, C.byref(ns), C.byref(nb)) == -1


def test_branch_color_equals_the_restatement():
    got = np.array([_lib.branch_color(i) for i in range(1000)])
    want = np.array([ref.branch_color(i) for i in range(1000)])
    assert np.array_equal(got, want)
    assert len({tuple(c) for c in got}) > 100 and got.max() == 255          # V = 1: one channel is always full


def background(seed, bh, bw, dtype=np.uint16):
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 1, (bh, bw)) * np.linspace(0.2, 1.0, bw)[None, :]
    return (a * 40000 + 300).astype(np.uint16) if dtype == np.uint16 else (a * 3.0 - 1.0).astype(np.float32)


def constructed_cases():
    """(name, background, segs, seg_branch, vis_width); canvas tiles are 64 x 16 pixels"""
    S = lambda *rows: np.array(rows, np.float64).reshape(-1, 4)
    I = lambda *v: np.array(v, np.int32)
    c = []
    # vis 500 on 50 x 50: one background pixel = 10 canvas pixels; (6.35, 1.55) -> canvas (64, 16), a tile corner
    c.append(("tile_corner", background(1, 50, 50), S([2.0, 0.3, 11.0, 2.9], [6.35, 1.55, 6.35, 1.55]), I(0, 1), 500))
    c.append(("overlap_later_wins", background(2, 40, 40), S([5, 5, 30, 30], [5, 30, 30, 5], [5, 5, 30, 30]), I(0, 1, 2), 500))
    c.append(("zero_length", background(3, 30, 30, np.float32), S([10, 10, 10, 10], [20.5, 3.25, 20.5, 3.25]), I(3, 4), 500))
    c.append(("off_canvas", background(4, 40, 40), S([-20, 10, 15, 12], [30, 35, 70, 90], [-5, -5, -1, -1], [200, 200, 300, 300], [39.4, 0, 39.4, 39.6]),
              I(0, 1, 2, 3, 5), 500))
    c.append(("non_square_wide", background(5, 24, 50, np.float32), S([1, 1, 48, 22], [48, 1, 1, 22]), I(7, 300), 500))
    c.append(("non_square_tall_odd_width", background(6, 47, 31), S([1, 1, 29, 45], [15, 0, 15, 46]), I(0, 1), 501))       # vw % 4 != 0: byte stores
    c.append(("constant_background", np.full((16, 16), 9, np.uint16), S([2, 2, 13, 13]), I(0), 500))
    c.append(("non_finite_dropped", background(7, 20, 20), S([np.nan, 2, 10, 10], [2, 2, 17, 9], [1, np.inf, 3, 3]), I(0, 1, 2), 500))
    c.append(("empty", background(8, 20, 26), np.zeros((0, 4)), np.zeros(0, np.int32), 500))
    c.append(("vis2000", background(9, 48, 48), S([4, 4, 40, 44], [40, 4, 4.5, 44.25], [24, 24, 24, 24]), I(0, 1, 2), 2000))
    return c


def fixture_cases():
    """four trees of the fixture over their own fields as backgrounds"""
    out = []
    for name, ci, sname, vis in (("s96", 0, "s1", 500), ("s96", 6, "s1", 500), ("s_rect", 7, "s1", 500), ("s96", 1, "s1", 2000)):
        key = f"{name}_c{ci}_{sname}"
        out.append((key, FIELDS[name], GT[key + "_segs"].astype(np.float64), GT[key + "_branch"], vis))
    return out


ALL_CASES = constructed_cases() + fixture_cases()
_REF = {}


def reference_picture(case):
    """the restatement's picture of a case, computed once per session (the GPU tests share it)"""
    name, bg, segs, sb, vis = case
    if name not in _REF:
        _REF[name] = ref.render_tree(bg, segs, sb, vis)
        _REF[name].setflags(write=False)
    return _REF[name]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_host_render_tree_equals_the_restatement(case):
    name, bg, segs, sb, vis = case
    got = _lib.host_render_tree(bg, [(segs, sb)], vis)[0]
    want = reference_picture(case)
    assert got.shape == want.shape == ref.canvas_shape(*bg.shape, vis) + (3,)
    assert np.array_equal(got, want), int((got != want).sum())
    if name == "overlap_later_wins":        # canvas centre: branch 2 was drawn last
        assert np.array_equal(got[got.shape[0] // 2 - 32, got.shape[1] // 2 - 32], ref.branch_color(2))
    if name in ("empty", "constant_background"):
        assert (got[0, 0] == got[0, 0, 0]).all()
    if len(segs) and name != "non_finite_dropped":
        assert (got.max(axis=2) != got.min(axis=2)).any()           # something coloured was drawn


def test_host_render_tree_batches_like_single_images():
    cases = [c for c in ALL_CASES if c[1].shape == (96, 96) and c[4] == 500]
    assert len(cases) == 2
    got = _lib.host_render_tree(np.stack([c[1] for c in cases]), [(c[2], c[3]) for c in cases], 500)
    for g, c in zip(got, cases):
        assert np.array_equal(g, reference_picture(c))


@pytest.mark.parametrize("vis", [500, 2000])
def test_host_barcode_equals_the_restatement(vis):
    for key in ("s96_c0_s640_bars", "s_rect_c7_s1_bars", "zero_c0_s1_bars"):
        bars = GT[key].astype(np.float64)
        got = _lib.host_render_barcode(bars, vis)
        assert got.shape == (round(vis * 0.9),) * 2 + (3,)
        assert np.array_equal(got, ref.render_barcode(bars, vis))
        if len(bars) == 0:
            assert (got == 255).all()
        else:
            assert (got != 255).any()
    ties = np.array([[-5.0, 1.0], [-5.0, 3.0], [-9.0, -2.0], [-1.0, 0.0]])       # equal births: the sort is stable
    assert np.array_equal(_lib.host_render_barcode(ties, vis), ref.render_barcode(ties, vis))
    one = np.array([[2.0, 2.0]])                                                # empty range: nothing to draw
    assert (_lib.host_render_barcode(one, vis) == 255).all()


def test_morse_graph_mirror_draws_the_reference_artists():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.collections import LineCollection
    from tmat_amd.topology import MorseGraph
    d1, d2, sw, mn, mx, iso, _ = MORSE_CASES[0]
    g = MorseGraph(FIELDS["s96"], thresholds=(d1, d2), min_branch_length=mn, max_branch_length=mx, remove_isolated_branches=iso, smoothing_window=sw)
    fig, (a0, a1) = plt.subplots(1, 2)
    try:
        g.plot_colored_tree(640 / 384, ax=a0)
        lc = [c for c in a0.collections if isinstance(c, LineCollection)]
        assert len(lc) == 1 and len(lc[0].get_segments()) == len(GT["s96_c0_s640_segs"])
        assert np.array_equal(np.array(lc[0].get_segments()).reshape(-1, 4), GT["s96_c0_s640_segs"].astype(np.float64))
        g.plot_colored_barcode(640 / 384, ax=a1)
        assert len(a1.patches) == len(GT["s96_c0_s640_bars"]) == len(g.barcode)
    finally:
        plt.close(fig)


def test_save_tree_visualizations_names_and_contents(tmp_path):
    from PIL import Image
    from tmat_amd import branches
    name, bg, segs, sb, vis = ALL_CASES[-4]                     # a fixture tree at width 500
    bars = GT[name + "_bars"].astype(np.float64)
    assert len(bars)
    first = branches.save_tree_visualizations(None, bg, (segs, sb), bars, tmp_path, "", vis)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["barcode.png", "morse_tree.png"]
    assert np.array_equal(np.asarray(Image.open(first[0])), reference_picture(ALL_CASES[-4]))
    assert np.array_equal(np.asarray(Image.open(first[1])), ref.render_barcode(bars, vis))
    second = branches.save_tree_visualizations(None, bg, (segs, sb), bars, tmp_path, "", vis)
    assert [Path(p).name for p in second] == ["morse_tree-2.png", "barcode-2.png"]
    sfx = branches.threshold_grid({"graph_thresh_1": [1, 12], "graph_thresh_2": [3, 4]})[0][1]
    third = branches.save_tree_visualizations(None, bg, (segs, sb), bars, tmp_path, sfx, vis)
    assert [Path(p).name for p in third] == [f"morse_tree{sfx}.png", f"barcode{sfx}.png"]
    assert branches.save_tree_visualizations(None, bg, (np.zeros((0, 4)), np.zeros(0, np.int32)), np.zeros((0, 2)), tmp_path / "none", "", vis) == []
    assert not (tmp_path / "none").exists()
