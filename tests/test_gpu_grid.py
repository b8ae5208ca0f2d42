"""GPU: the threshold-grid form of the 2-D branch (tmat_analyze_batch_grid): the whole grid of (graph_thresh_1, graph_thresh_2) pairs from
one pass of the network -- rows, trees, stage pictures and the device-made PNG files against the per-pair entries, the launch counts of
one pass, poisoned workspaces, the argument checks, and the script's files."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from tmat_amd import _lib, branches, synth

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
from png_check import check_png  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = dict(graph_smoothing_window=12, min_branch_length=12)
# a 2 x 2 grid; graph_thresh_1 = 1 and 5 give image 0 five and four branches (the CPU oracle's rows), so the pairs really differ
PAIRS = [(1.0, 4.0), (1.0, 40.0), (5.0, 4.0), (5.0, 40.0)]
VIS = 500
GUARD = 0xA5
FSHAPE = (384, 384)
HW = (320, 320)


@pytest.fixture(scope="module")
def imgs():
    """four 512 x 512 images of 72 patches: two passes (3 + 1) on the session handle; image 2 is constant and has no branches"""
    a = np.stack([synth.synth_image(i, 512, n_vessels=12, scale=1.0) for i in range(4)])
    a[2] = 1000
    return a


@pytest.fixture(scope="module")
def per_pair(handle, imgs):
    """the parent's way, once for the module: one analyze_batch_tree call per pair -> {pair: (rows, overlays, bars)}"""
    return {p: branches.analyze_batch_tree(handle, imgs, CFG, 500.0, thresh=p, vis_width=VIS) for p in PAIRS}


def grid_call(handle, imgs, pairs, tree=False, rgb=True, tree_png=False, barcode_png=False, stage=False, well=None, pruning=None, cap_b=4096,
              tree_cap=None, bar_cap=None, dev=False, opts_size=None, grid_size=None, n_thresh=None, thresh_null=False):
    """tmat_analyze_batch_grid through ctypes with every output buffer pre-filled with GUARD; returns (rc, dict of the buffers)"""
    L = _lib.lib()
    n, H, W = imgs.shape
    T = len(pairs)
    sw_px, min_px, max_px = branches.graph_px_params(CFG, 384, 500.0)
    thresh = np.ascontiguousarray(np.asarray(pairs, np.float32).reshape(-1, 2))
    out = {"rows": (_lib.Row * (T * n))()}
    for r in out["rows"]:
        r.index, r.count, r.total_px, r.avg_px = -7, -7, -7.0, -7.0
    o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts) if opts_size is None else opts_size, ds_ratio=0.625, ds_width=384, smoothing_window_px=int(sw_px),
                         min_branch_length_px=int(min_px), max_branch_length_px=int(max_px or 0), remove_isolated=0, first_index=0,
                         well_masks=None if well is None else well.ctypes.data, pruning_masks=None if pruning is None else pruning.ctypes.data)
    g = _lib.GridOpts(size=C.sizeof(_lib.GridOpts) if grid_size is None else grid_size, n_thresh=T if n_thresh is None else n_thresh,
                      thresh=None if thresh_null else thresh.ctypes.data)
    vh, vw = _lib.tree_canvas_shape(HW[0], HW[1], VIS)
    S = int(round(0.9 * VIS))
    if stage:
        out["pictures"] = np.full((n, 4) + HW, GUARD, np.uint8)
        o.stage_out = out["pictures"].ctypes.data
    if tree or tree_png or barcode_png:
        out["bars"] = np.full((T, n, cap_b, 2), -7.0)
        out["n_bars"] = np.full((T, n), -7, np.int32)
        o.vis_width, o.bars_out, o.cap_b, o.n_bars = VIS, out["bars"].ctypes.data, cap_b, out["n_bars"].ctypes.data
        if rgb:
            out["rgb"] = np.full((T, n, vh, vw, 3), GUARD, np.uint8)
            o.rgb_out = out["rgb"].ctypes.data
    if tree_png:
        cap = _lib.png_bound(vh, vw, 3) if tree_cap is None else tree_cap
        out["tree_png"], out["tree_sizes"] = np.full((T, n, cap), GUARD, np.uint8), np.zeros((T, n), np.uintp)
        g.tree_png, g.tree_png_cap, g.tree_png_sizes = out["tree_png"].ctypes.data, cap, out["tree_sizes"].ctypes.data
    if barcode_png:
        cap = _lib.png_bound(S, S, 3) if bar_cap is None else bar_cap
        out["barcode_png"], out["barcode_sizes"] = np.full((T, n, cap), GUARD, np.uint8), np.zeros((T, n), np.uintp)
        g.barcode_png, g.barcode_png_cap, g.barcode_png_sizes = out["barcode_png"].ctypes.data, cap, out["barcode_sizes"].ctypes.data
    _lib.check(L.tmat_set_input_depth(handle.raw, 16), "tmat_set_input_depth")
    if dev:
        dptr = C.c_void_p()
        _lib.check(L.tmat_dev_alloc(handle.raw, imgs.nbytes, C.byref(dptr)), "tmat_dev_alloc")
        try:
            _lib.check(L.tmat_dev_upload(handle.raw, dptr, _lib.ptr(imgs), imgs.nbytes), "tmat_dev_upload")
            rc = L.tmat_analyze_batch_grid_dev(handle.raw, dptr, n, H, W, C.byref(o), C.byref(g), out["rows"])
        finally:
            L.tmat_dev_free(handle.raw, dptr)
    else:
        rc = L.tmat_analyze_batch_grid(handle.raw, _lib.ptr(imgs), n, H, W, C.byref(o), C.byref(g), out["rows"])
    out["row_tuples"] = [(r.index, r.count, r.total_px, r.avg_px) for r in out["rows"]]
    return rc, out


def untouched(out):
    """no output of a refused call was written"""
    ok = all(r == (-7, -7, -7.0, -7.0) for r in out["row_tuples"])
    for k in ("pictures", "rgb", "tree_png", "barcode_png"):
        ok = ok and (k not in out or bool((out[k] == GUARD).all()))
    for k in ("tree_sizes", "barcode_sizes"):
        ok = ok and (k not in out or not out[k].any())
    return ok and ("n_bars" not in out or bool((out["n_bars"] == -7).all())) and ("bars" not in out or bool((out["bars"] == -7.0).all()))


def test_rows_of_a_2x2_grid_equal_four_per_pair_calls(handle, imgs, per_pair):
    want = {p: branches.analyze_batch(handle, imgs, CFG, 500.0, thresh=p) for p in PAIRS}
    # precondition, on the per-pair entry alone: the pairs really differ, so a grid that ignores `thresh` cannot pass
    stats = {p: [r[1:] for r in rows] for p, rows in want.items()}
    print("per-pair rows", stats)
    assert any(stats[a][i] != stats[b][i] for a in PAIRS for b in PAIRS for i in range(4)), stats
    assert len({tuple(v) for v in stats.values()}) >= 2
    assert all(sum(r[0] for r in v) > 0 for v in stats.values()), "every pair should find branches"
    assert all(v[2] == (0, 0.0, 0.0) for v in stats.values()), "the constant image has none"
    got, extras = branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=PAIRS)
    assert extras == {} and list(got) == PAIRS
    for p in PAIRS:
        assert got[p] == want[p], p
        assert got[p] == per_pair[p][0], p
    rc, out = grid_call(handle, imgs, PAIRS, dev=True)              # images already in HBM: the same rows
    assert rc == 0 and out["row_tuples"] == [r for p in PAIRS for r in want[p]]


def _masks(n):
    from test_gpu_analyze_masked import _given_masks
    well, pruning = _given_masks(n, HW, FSHAPE)
    return np.ascontiguousarray(well, np.uint8), np.ascontiguousarray(pruning, np.uint8)


@pytest.mark.parametrize("combo", range(16), ids=lambda c: "".join(k for k, b in zip("WPTS", (c & 1, c & 2, c & 4, c & 8)) if b) or "plain")
def test_one_pair_equals_analyze_batch_ex(handle, imgs, combo):
    """n_thresh = 1 against tmat_analyze_batch_ex for every combination of well masks, pruning masks, tree and stage pictures"""
    use_well, use_prune, tree, stage = bool(combo & 1), bool(combo & 2), bool(combo & 4), bool(combo & 8)
    well, pruning = _masks(4)
    pair = (5.0, 10.0)
    rows, ex = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, thresh=pair, well_masks=well if use_well else None,
                                         pruning_masks=pruning if use_prune else None, tree=tree, vis_width=VIS, stage_pictures=stage)
    got, gx = branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=[pair], well_masks=well if use_well else None,
                                          pruning_masks=pruning if use_prune else None, tree=tree, vis_width=VIS, stage_pictures=stage)
    assert got[pair] == rows
    assert set(gx) == set(ex)
    if tree:
        assert np.array_equal(gx["overlays"][pair], ex["overlays"])
        assert len(gx["bars"][pair]) == 4 and all(np.array_equal(a, b) for a, b in zip(gx["bars"][pair], ex["bars"]))
    if stage:
        assert np.array_equal(gx["pictures"], ex["pictures"])


def test_trees_per_pair_equal_analyze_batch_tree(handle, imgs, per_pair):
    rc, out = grid_call(handle, imgs, PAIRS, tree=True, stage=True)
    assert rc == 0, _lib.lib().tmat_last_error()
    for t, p in enumerate(PAIRS):
        rows, overlays, bars = per_pair[p]
        assert out["row_tuples"][4 * t: 4 * t + 4] == rows
        assert np.array_equal(out["rgb"][t], overlays), (p, int((out["rgb"][t] != overlays).sum()))
        for i in range(4):
            nb = int(out["n_bars"][t, i])
            assert nb == len(bars[i]) == rows[i][1]
            assert np.array_equal(out["bars"][t, i, :nb], bars[i])
            assert (out["bars"][t, i, nb:] == -7.0).all()
    assert any(not np.array_equal(out["rgb"][0], out["rgb"][t]) for t in range(1, 4)), "the overlays of different pairs differ"
    _, ex = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, thresh=PAIRS[0], stage_pictures=True)
    assert np.array_equal(out["pictures"], ex["pictures"])


@pytest.mark.parametrize("rgb", [True, False], ids=["with_raw", "rgb_null"])
def test_png_files_from_the_raster_in_hbm(handle, imgs, per_pair, rgb):
    pairs = PAIRS[1:3]
    rc, out = grid_call(handle, imgs, pairs, rgb=rgb, tree_png=True, barcode_png=True)
    assert rc == 0, _lib.lib().tmat_last_error()
    assert ("rgb" in out) == rgb
    S = int(round(0.9 * VIS))
    for t, p in enumerate(pairs):
        rows, overlays, bars = per_pair[p]
        assert out["row_tuples"][4 * t: 4 * t + 4] == rows
        if rgb:
            assert np.array_equal(out["rgb"][t], overlays)
        want_tree = handle.png_encode(overlays)
        want_bar = _lib.host_png_encode(np.stack([_lib.host_render_barcode(b, VIS) for b in bars]))
        for i in range(4):
            for files, sizes, want, pic in ((out["tree_png"], out["tree_sizes"], want_tree[i], overlays[i]),
                                            (out["barcode_png"], out["barcode_sizes"], want_bar[i], _lib.host_render_barcode(bars[i], VIS))):
                sz = int(sizes[t, i])
                assert files[t, i, :sz].tobytes() == want, (p, i)
                assert (files[t, i, sz:] == GUARD).all(), "bytes behind a file are not written"
                check_png(want, pic)
            assert np.array_equal(out["bars"][t, i, : out["n_bars"][t, i]], bars[i])
    assert _lib.host_render_barcode(per_pair[pairs[0]][2][2], VIS).shape == (S, S, 3) and len(per_pair[pairs[0]][2][2]) == 0     # the empty barcode was in


def test_the_network_runs_once(handle, imgs):
    """launch counts of the profiled kernel family: a 2 x 2 grid call = ONE analyze_batch call on the same images"""
    handle.prof_enable(True)
    try:
        handle.prof_read(reset=True)
        branches.analyze_batch(handle, imgs, CFG, 500.0, thresh=PAIRS[0])
        one = handle.prof_read(reset=True)[1]
        branches.analyze_batch_grid(handle, imgs, CFG, 500.0, pairs=PAIRS)
        grid = handle.prof_read(reset=True)[1]
    finally:
        handle.prof_enable(False)
    assert one > 0 and grid == one, (one, grid)


def test_poisoned_workspaces_and_a_repeat(handle, imgs, per_pair):
    kw = dict(tree=True, tree_png=True, barcode_png=True, stage=True)
    rc, first = grid_call(handle, imgs, PAIRS[:2], **kw)
    assert rc == 0
    held = handle.debug_held_bytes()
    handle.debug_poison(0xFF)
    rc, poisoned = grid_call(handle, imgs, PAIRS[:2], **kw)
    assert rc == 0
    rc, again = grid_call(handle, imgs, PAIRS[:2], **kw)
    assert rc == 0
    for other in (poisoned, again):
        assert other["row_tuples"] == first["row_tuples"]
        for k in ("rgb", "pictures", "tree_png", "tree_sizes", "barcode_png", "barcode_sizes", "n_bars", "bars"):
            assert np.array_equal(other[k], first[k]), k
    assert handle.debug_held_bytes() == held, "a repeat allocates nothing more"
    # what the grid form adds is held (and so poisoned): twice the bar capacity grows the rectangle tables of a pass of 3 images, 20 bytes
    # a rectangle, and the held bytes with them
    rc, _ = grid_call(handle, imgs, PAIRS[:2], cap_b=8192, **kw)
    assert rc == 0
    assert handle.debug_held_bytes()[0] >= held[0] + 3 * 4096 * 20
    assert first["row_tuples"][:4] == per_pair[PAIRS[0]][0]
    assert branches.analyze_batch(handle, imgs, CFG, 500.0, thresh=PAIRS[1]) == per_pair[PAIRS[1]][0]


def test_refused_calls_write_nothing(handle, imgs):
    E_ARG, E_CAP = _lib.E_ARG, _lib.E_CAP
    two = imgs[:2]
    full = dict(tree=True, tree_png=True, barcode_png=True, stage=True)
    cases = {
        "n_thresh_0": (E_ARG, dict(n_thresh=0)),
        "n_thresh_negative": (E_ARG, dict(n_thresh=-1)),
        "thresh_null": (E_ARG, dict(thresh_null=True)),
        "opts_size": (E_ARG, dict(opts_size=C.sizeof(_lib.AnalyzeOpts) + 8)),
        "grid_size": (E_ARG, dict(grid_size=C.sizeof(_lib.GridOpts) - 8)),
        "tree_png_cap": (E_CAP, dict(tree_cap=_lib.png_bound(VIS, VIS, 3) - 1)),
        "barcode_png_cap": (E_CAP, dict(bar_cap=_lib.png_bound(450, 450, 3) - 1)),
    }
    for name, (want, kw) in cases.items():
        rc, out = grid_call(handle, two, PAIRS[:2], **full, **kw)
        assert rc == want, (name, rc)
        assert untouched(out), name
    plain = _lib.Handle(None, 0)
    try:
        rc, out = grid_call(plain, two, PAIRS[:2], **full)
        assert rc == E_ARG and untouched(out), "a handle without a model"
    finally:
        plain.close()
    # more bars than cap_b at some (t, i): TMAT_E_CAP
    rc, out = grid_call(handle, two, PAIRS[:2], tree=True, cap_b=1)
    assert rc == E_CAP
    # the handle still works
    rc, out = grid_call(handle, two, PAIRS[:2])
    assert rc == 0 and all(r[0] in (0, 1) for r in out["row_tuples"])


def test_script_grid_with_tree_visualizations(tmp_path, handle):
    """two .npy images, a 2 x 1 grid, --tree-visualizations: per suffix the CSV of a single-pair run, picture names under the _CONFIG rule,
    and --png-encoder device decodes to the pixels of pil"""
    from PIL import Image
    from test_gpu_script import read_csv, run
    ind = tmp_path / "in"
    ind.mkdir()
    for i in range(2):
        np.save(ind / f"g_{i}.npy", synth.synth_image(70 + i, 512, n_vessels=12, scale=1.0))
    base = [str(ind)], ["--image-width-microns", "500", "--graph-thresh-2", "10", "--tree-visualizations", "--vis-width", str(VIS)]
    outs = {}
    for enc in ("pil", "device"):
        outs[enc] = tmp_path / enc
        r = run(base[0] + [str(outs[enc])] + base[1] + ["--graph-thresh-1", "2", "5", "--png-encoder", enc])
        assert r.returncode == 0, r.stdout + r.stderr
    grid = branches.threshold_grid(dict(graph_thresh_1=[2.0, 5.0], graph_thresh_2=[10.0]))
    suffixes = {int(cfg["thresh1"]): sfx for cfg, sfx in grid}
    assert suffixes == {2: "_CONFIG_thresh1_2.0", 5: "_CONFIG_thresh1_5.0"}
    for t1, sfx in suffixes.items():
        single = tmp_path / f"single_{t1}"
        r = run(base[0] + [str(single)] + ["--image-width-microns", "500", "--graph-thresh-2", "10", "--graph-thresh-1", str(t1)])
        assert r.returncode == 0, r.stdout + r.stderr
        want = read_csv(single / "branching_analysis.csv")
        assert len(want) == 3 and sum(int(w[1]) for w in want[1:]) > 0
        for enc in ("pil", "device"):
            assert read_csv(outs[enc] / f"branching_analysis{sfx}.csv") == want, (enc, sfx)
    names = sorted(f"{stem}{sfx}.png" for stem in ("morse_tree", "barcode") for sfx in suffixes.values())
    for i in range(2):
        for enc in ("pil", "device"):
            assert sorted(p.name for p in (outs[enc] / "visualizations" / f"g_{i}").iterdir()) == names, (enc, i)
        for name in names:
            a = np.asarray(Image.open(outs["pil"] / "visualizations" / f"g_{i}" / name))
            b = np.asarray(Image.open(outs["device"] / "visualizations" / f"g_{i}" / name))
            assert a.shape == b.shape and np.array_equal(a, b), (i, name)
    assert sorted(p.name for p in outs["pil"].glob("*.csv")) == sorted(f"branching_analysis{s}.csv" for s in suffixes.values())
