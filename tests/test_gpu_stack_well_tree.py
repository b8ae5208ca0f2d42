"""GPU tests of what the Z-stack batch path gained for --detect-well and --tree-visualizations: the batched front end of the well
threshold (tmat_stack_well_front_dev, tmat_canny_mask_batch), the masks made from it (sato.stack_well_masks_batch), the entry for
stacks resident in HBM (tmat_analyze_stack_batch_dev) and the tree request of tmat_stack_opts.  Every stack of a batch must come out
exactly as it does alone and as the oracle computes it on the CPU.  Inputs and the oracle's results: tests/helpers/well_stacks.py."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import well_stacks as ws  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def out_hw_of(stacks):
    from tmat_amd import sato
    return sato.dsamp_shape(stacks.shape, 384)


# ---- front end ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["four", "odd"])
def test_front_end_equals_the_oracle_and_the_resize_entry(plain, which):
    from tmat_amd import sato
    stacks = ws.four_stacks() if which == "four" else ws.odd_stacks()
    out_hw = out_hw_of(stacks)
    assert out_hw == ((307, 384) if which == "four" else (411, 384))
    thresh, border, proj = sato.stack_well_front(plain, stacks, out_hw, return_proj=True)
    for i, (aa, ts, bs, _) in enumerate(ws.oracle_front(which)):
        assert thresh.shape[1:] == ts.shape
        assert np.array_equal(thresh[i].astype(bool), ts), (which, i)
        assert np.array_equal(border[i].astype(bool), bs), (which, i)
        assert same_bits(proj[i], sato.resize_aa(plain, stacks[i].max(0), out_hw)), (which, i)
        assert np.array_equal(proj[i], aa), (which, i)
    assert all(t.any() and b.any() for t, b in zip(thresh[:3], border[:3]))


def test_a_stack_alone_equals_itself_inside_a_batch(plain):
    from tmat_amd import sato
    stacks = ws.four_stacks()
    out_hw = out_hw_of(stacks)
    four = sato.stack_well_front(plain, stacks, out_hw, return_proj=True)
    for i in range(4):
        one = sato.stack_well_front(plain, stacks[i:i + 1], out_hw, return_proj=True)
        for a, b in zip(one, four):
            assert same_bits(a[0], b[i]), i


def test_a_blank_stack_changes_neither_neighbour(plain):
    """[40, blank, 42]: extrema or histograms shared across the batch would move a threshold of one of the two"""
    from tmat_amd import sato
    stacks = ws.four_stacks()
    out_hw = out_hw_of(stacks)
    want = sato.stack_well_front(plain, stacks, out_hw, return_proj=True)
    got = sato.stack_well_front(plain, stacks[[0, 3, 2]], out_hw, return_proj=True)
    for a, b in zip(got, want):
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[3]) and same_bits(a[2], b[2])


def test_canny_batch_equals_canny_alone(plain):
    from tmat_amd import _lib
    from tmat_amd import well_mask_generation as wmg
    masks = np.stack([f[1] for f in ws.oracle_front("four")] + [np.zeros((160, 200), bool), np.ones((160, 200), bool)])
    got = wmg._border_batch(plain, masks)
    for i, m in enumerate(masks):
        assert np.array_equal(got[i], wmg._border(plain, m)), i
    m = np.ascontiguousarray(masks[:2], np.uint8)
    L = _lib.lib()
    assert L.tmat_canny_mask_batch(plain.raw, _lib.ptr(m), 0, 160, 200, 1.0, _lib.ptr(m)) == _lib.E_ARG
    assert L.tmat_canny_mask_batch(plain.raw, _lib.ptr(m), 2, 2, 200, 1.0, _lib.ptr(m)) == _lib.E_ARG


# ---- masks -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["four", "odd"])
def test_masks_equal_the_per_stack_route_and_the_oracle(plain, which, capsys):
    from tmat_amd import sato
    from tmat_amd import well_mask_generation as wmg
    stacks = ws.four_stacks() if which == "four" else ws.odd_stacks()
    out_hw = out_hw_of(stacks)
    warned = []
    well, pruning = sato.stack_well_masks_batch(plain, stacks, out_hw, ws.SEED, warn=warned.append)
    assert well.shape == pruning.shape == (len(stacks),) + out_hw and well.dtype == pruning.dtype == bool
    single_warned = []
    for i, st in enumerate(stacks):
        w1, s1 = wmg.make_well_mask(sato.resize_aa(plain, st.max(0), out_hw), handle=plain, seed=ws.SEED, warn=single_warned.append)
        assert np.array_equal(well[i], w1) and np.array_equal(pruning[i], np.logical_not(s1)), (which, i)
        w2, p2 = sato.stack_well_masks(plain, st, out_hw, ws.SEED)
        assert np.array_equal(well[i], w2) and np.array_equal(pruning[i], p2), (which, i)
        ow, oshr = ws.oracle_front(which)[i][3]
        assert np.array_equal(well[i], ow) and np.array_equal(pruning[i], np.logical_not(oshr)), (which, i)
    assert warned == single_warned and len(warned) == 1
    if which == "four":
        assert int(pruning[0].sum()) == 70568 and well[1].all() and not pruning[1].any() and int(pruning[3].sum()) == 8802


def test_masks_from_resident_stacks_equal_masks_from_arrays(plain):
    from tmat_amd import sato
    stacks = ws.four_stacks()
    out_hw = out_hw_of(stacks)
    quiet = lambda m: None  # noqa: E731
    want = sato.stack_well_masks_batch(plain, stacks, out_hw, ws.SEED, warn=quiet)
    with sato.upload_stacks(plain, stacks) as dev:
        got = sato.stack_well_masks_batch(plain, dev, out_hw, ws.SEED, warn=quiet)
        also = sato.stack_well_masks_batch(plain, (dev.ptr, dev.shape), out_hw, ws.SEED, warn=quiet)
        assert np.array_equal(dev.download(), stacks)
    for a, b, c in zip(got, want, also):
        assert np.array_equal(a, b) and np.array_equal(c, b)


# ---- stacks resident in HBM --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pass_stacks", [1, 2])
def test_dev_entry_equals_the_host_pointer_form_and_leaves_the_buffer_alone(plain, pass_stacks):
    from tmat_amd import sato
    stacks = ws.four_stacks()[:3]
    sw, mn, mx = ws.px_params()
    kw = dict(return_fields=True, return_pictures=True, pass_stacks=pass_stacks)
    rows, fields, (proj, fpic) = sato.analyze_stack_batch(plain, stacks, ws.PAIRS, sw, mn, mx, False, **kw)
    assert all(r[0] > 0 for r in rows[0])
    with sato.upload_stacks(plain, stacks) as dev:
        drows, dfields, (dproj, dfpic) = sato.analyze_stack_batch(plain, dev, ws.PAIRS, sw, mn, mx, False, **kw)
        assert np.array_equal(dev.download(), stacks), "the caller's device buffer must come out unchanged"
    assert drows == rows
    assert same_bits(dfields, fields) and np.array_equal(dproj, proj) and np.array_equal(dfpic, fpic)


def test_pruned_rows_of_the_batch_masks(plain):
    """stack 40's rows change under its own mask at both pairs (11 -> 10 and 15 -> 14 branches), stack 42's do not"""
    from tmat_amd import sato
    stacks = ws.four_stacks()
    sw, mn, mx = ws.px_params()
    out_hw = out_hw_of(stacks)
    _, pruning = sato.stack_well_masks_batch(plain, stacks, out_hw, ws.SEED, warn=lambda m: None)
    with sato.upload_stacks(plain, stacks) as dev:
        rows, fields = sato.analyze_stack_batch(plain, dev, ws.PAIRS, sw, mn, mx, False, pruning_masks=pruning, return_fields=True, pass_stacks=3)
        bare = sato.analyze_stack_batch(plain, dev, ws.PAIRS, sw, mn, mx, False, pass_stacks=3)
    for t, (t1, t2) in enumerate(ws.PAIRS):
        for i in range(4):
            assert rows[t][i] == sato.field_stats(plain, fields[i], t1, t2, sw, mn, mx, False, pruning_mask=pruning[i]), (t, i)
    assert [bare[t][0][0] for t in range(2)] == [11, 15] and [rows[t][0][0] for t in range(2)] == [10, 14]
    assert all(rows[t][2] == bare[t][2] for t in range(2))
    assert all(rows[t][3][0] == 0 for t in range(2))


def test_recycled_blocks_hold_nothing_the_new_entries_read_before_writing(plain):
    from tmat_amd import sato
    stacks = ws.four_stacks()
    sw, mn, mx = ws.px_params()
    out_hw = out_hw_of(stacks)
    quiet = lambda m: None  # noqa: E731

    def run():
        with sato.upload_stacks(plain, stacks) as dev:
            front = sato.stack_well_front(plain, dev, out_hw, return_proj=True)
            masks = sato.stack_well_masks_batch(plain, dev, out_hw, ws.SEED, warn=quiet)
            rows = sato.analyze_stack_batch(plain, dev, ws.PAIRS, sw, mn, mx, False, pruning_masks=masks[1], pass_stacks=2)
        return front, masks, rows
    want = run()
    for pattern in (0xFF, 0x7F):
        plain.debug_poison(pattern)
        got = run()
        assert all(same_bits(a, b) for a, b in zip(got[0], want[0])), pattern
        assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1])), pattern
        assert got[2] == want[2], pattern


def test_front_end_refuses_bad_arguments(plain):
    from tmat_amd import _lib, sato
    stacks = ws.four_stacks()[:1]
    L = _lib.lib()
    th, bd = np.zeros((1, 160, 200), np.uint8), np.zeros((1, 160, 200), np.uint8)
    with sato.upload_stacks(plain, stacks) as dev:
        def call(ptr=dev.ptr, n=1, oh=307, ow=384, t=th):
            return L.tmat_stack_well_front_dev(plain.raw, ptr, n, 3, 128, 160, oh, ow, None, _lib.ptr(t) if t is not None else None, _lib.ptr(bd))
        sato.install_gaussian_tables(plain, (128, 160), (307, 384), sigmas=())
        assert call() == 0
        for bad in (dict(ptr=None), dict(n=0), dict(oh=19), dict(ow=19), dict(t=None)):
            assert call(**bad) == _lib.E_ARG, bad
            assert L.tmat_last_error()


# ---- tree request ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree_case(plain):
    """2 pairs x [40, 41, blank] with their pruning masks, two passes (the last one ragged); the references are made once"""
    from tmat_amd import _lib, branches, sato
    stacks = ws.four_stacks()[[0, 1, 3]]
    sw, mn, mx = ws.px_params()
    out_hw = out_hw_of(stacks)
    _, pruning = sato.stack_well_masks_batch(plain, stacks, out_hw, ws.SEED, warn=lambda m: None)
    rows, fields = sato.analyze_stack_batch(plain, stacks, ws.PAIRS, sw, mn, mx, False, pruning_masks=pruning, return_fields=True, pass_stacks=2)
    trees = [[branches.field_tree(plain, _lib.host_rescale255_f32(fields[i]), ws.CFG, ws.WIDTH_UM, pair, pruning[i], stacks.shape[3] / out_hw[1])
              for i in range(3)] for pair in ws.PAIRS]
    return dict(stacks=stacks, pruning=pruning, rows=rows, fields=fields, trees=trees, px=(sw, mn, mx))


@pytest.mark.parametrize("vis_width, pass_stacks", [(200, 2), (301, 2), (200, 1)])
def test_tree_request_gives_the_per_stack_geometry_and_overlays(plain, tree_case, vis_width, pass_stacks):
    """passes of 2: two passes, the last one ragged, both drawn after the loop; passes of 1: three passes, the first drawn inside the loop
    while the third is queued"""
    from tmat_amd import _lib, sato
    tc = tree_case
    sw, mn, mx = tc["px"]
    with sato.upload_stacks(plain, tc["stacks"]) as dev:
        rows, fields, extra = sato.analyze_stack_batch(plain, dev, ws.PAIRS, sw, mn, mx, False, pruning_masks=tc["pruning"], return_fields=True,
                                                       pass_stacks=pass_stacks, tree=True, vis_width=vis_width)
    assert rows == tc["rows"] and same_bits(fields, tc["fields"])
    vh, vw = _lib.tree_canvas_shape(128, 160, vis_width)
    assert extra["overlays"].shape == (2, 3, vh, vw, 3) and vw == vis_width
    proj = tc["stacks"].max(1)
    for t, (t1, t2) in enumerate(ws.PAIRS):
        for i in range(3):
            tree, bars, stats = tc["trees"][t][i]
            assert rows[t][i] == tuple(stats) == sato.field_stats(plain, fields[i], t1, t2, sw, mn, mx, False, pruning_mask=tc["pruning"][i]), (t, i)
            assert same_bits(extra["bars"][t][i], bars), (t, i)
            assert np.array_equal(extra["overlays"][t, i], _lib.host_render_tree(proj[i][None], [tree], vis_width)[0]), (t, i)
        assert len(extra["bars"][t][0]) > 0 and len(extra["bars"][t][1]) > 0
        # the blank stack: no bars, and the overlay of a constant background
        assert len(extra["bars"][t][2]) == 0 and not extra["overlays"][t, 2].any()
    # a line is drawn: the overlay differs from the bare background somewhere
    bare = _lib.host_render_tree(proj[0][None], [(np.zeros((0, 4)), np.zeros(0, np.int32))], vis_width)[0]
    assert not np.array_equal(extra["overlays"][0, 0], bare)


def test_overlays_do_not_depend_on_the_pass_size(plain):
    """four stacks in passes of 1 (the fourth pass takes the first one's projection slot again), 3 and 4, with the pictures of
    --visualizations out of the same call"""
    from tmat_amd import sato
    stacks = ws.four_stacks()
    sw, mn, mx = ws.px_params()
    want = None
    for k in (4, 1, 3):
        rows, pics, extra = sato.analyze_stack_batch(plain, stacks, ws.PAIRS, sw, mn, mx, False, return_pictures=True, pass_stacks=k, tree=True, vis_width=200)
        got = (rows, pics[0], pics[1], extra["overlays"], [b for t in extra["bars"] for b in t])
        if want is None:
            want = got
            assert extra["overlays"][:, :3].any(axis=(2, 3, 4)).all()
            continue
        assert got[0] == want[0], k
        assert all(np.array_equal(a, b) for a, b in zip(got[1:4], want[1:4])), k
        assert all(same_bits(a, b) for a, b in zip(got[4], want[4])), k


def test_tree_geometry_alone_and_host_pointer_form(plain, tree_case):
    from tmat_amd import sato
    tc = tree_case
    sw, mn, mx = tc["px"]
    rows, extra = sato.analyze_stack_batch(plain, tc["stacks"], ws.PAIRS, sw, mn, mx, False, pruning_masks=tc["pruning"], pass_stacks=1, tree=True,
                                           overlays=False, cap_bars=1)         # cap_bars 1: the wrapper's retry with fh * fw
    assert rows == tc["rows"] and extra["overlays"] is None
    for t in range(2):
        for i in range(3):
            assert same_bits(extra["bars"][t][i], tc["trees"][t][i][1]), (t, i)


def _raw_opts(tc, th, **kw):
    from tmat_amd import _lib
    sw, mn, mx = tc["px"]
    o = _lib.StackOpts()
    o.size, o.ds_width, o.hessian, o.n_thresh, o.thresh = C.sizeof(_lib.StackOpts), 384, 0, len(th), th.ctypes.data
    o.smoothing_window_px, o.min_branch_length_px, o.max_branch_length_px, o.pass_stacks = int(sw), int(mn), int(mx or 0), 2
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bar_capacity_and_bad_tree_requests(plain, tree_case):
    from tmat_amd import _lib, sato
    tc = tree_case
    stacks = np.ascontiguousarray(tc["stacks"])
    sato.install_gaussian_tables(plain, (128, 160), (307, 384))
    th = np.ascontiguousarray(ws.PAIRS, np.float32)
    L = _lib.lib()
    rows = (_lib.Row * 6)()
    bars, nb = np.zeros((2, 3, 64, 2)), np.zeros((2, 3), np.int32)
    rgb = np.zeros((2, 3, 160, 200, 3), np.uint8)

    def call(**kw):
        o = _raw_opts(tc, th, **kw)
        return L.tmat_analyze_stack_batch(plain.raw, _lib.ptr(stacks), 3, 3, 128, 160, C.byref(o), rows)
    assert call(bars_out=bars.ctypes.data, n_bars=nb.ctypes.data, cap_b=64) == 0
    assert nb[0, 0] > 0 and nb[0, 2] == 0
    assert call(bars_out=bars.ctypes.data, n_bars=nb.ctypes.data, cap_b=0) == _lib.E_CAP
    assert call(bars_out=bars.ctypes.data, n_bars=nb.ctypes.data, cap_b=int(nb.max()) - 1) == _lib.E_CAP
    for bad in (dict(bars_out=bars.ctypes.data, cap_b=64), dict(n_bars=nb.ctypes.data, cap_b=64), dict(bars_out=bars.ctypes.data, n_bars=nb.ctypes.data, cap_b=-1),
                dict(rgb_out=rgb.ctypes.data, vis_width=200), dict(bars_out=bars.ctypes.data, n_bars=nb.ctypes.data, cap_b=64, rgb_out=rgb.ctypes.data, vis_width=0)):
        assert call(**bad) == _lib.E_ARG, bad
        assert L.tmat_last_error()
    assert call() == 0          # the handle is still usable; no pruning masks here: stack 40 keeps its 11 branches
    assert rows[0].count == 11 and tc["rows"][0][0][0] == 10


def test_the_first_version_of_the_options_struct_is_still_served(plain, tree_case):
    """size = TMAT_STACK_OPTS_SIZE_V1: the fields up to pass_stacks are read and nothing behind them -- a tree request there (which would
    be refused as incomplete) is not seen"""
    from tmat_amd import _lib, sato
    tc = tree_case
    stacks = np.ascontiguousarray(tc["stacks"])
    th = np.ascontiguousarray(ws.PAIRS, np.float32)
    pm = np.ascontiguousarray(tc["pruning"], np.uint8)
    nb = np.zeros((2, 3), np.int32)
    L = _lib.lib()
    for entry, src in ((L.tmat_analyze_stack_batch, None), (L.tmat_analyze_stack_batch_dev, "dev")):
        rows = (_lib.Row * 6)()
        o = _raw_opts(tc, th, size=_lib.STACK_OPTS_SIZE_V1, pruning_masks=pm.ctypes.data, vis_width=77, n_bars=nb.ctypes.data, cap_b=-3)
        if src is None:
            assert entry(plain.raw, _lib.ptr(stacks), 3, 3, 128, 160, C.byref(o), rows) == 0
        else:
            with sato.upload_stacks(plain, stacks) as dev:
                assert entry(plain.raw, dev.ptr, 3, 3, 128, 160, C.byref(o), rows) == 0
        got = [[(rows[t * 3 + i].count, rows[t * 3 + i].total_px, rows[t * 3 + i].avg_px) for i in range(3)] for t in range(2)]
        assert got == tc["rows"]
        assert not nb.any()
    o = _raw_opts(tc, th, size=_lib.STACK_OPTS_SIZE_V1 + 8)
    assert L.tmat_analyze_stack_batch(plain.raw, _lib.ptr(stacks), 3, 3, 128, 160, C.byref(o), rows) == _lib.E_ARG


def test_recycled_blocks_hold_nothing_the_tree_request_reads_before_writing(plain, tree_case):
    from tmat_amd import sato
    tc = tree_case
    sw, mn, mx = tc["px"]

    def run():
        return sato.analyze_stack_batch(plain, tc["stacks"], ws.PAIRS, sw, mn, mx, False, pruning_masks=tc["pruning"], pass_stacks=1, tree=True, vis_width=200)
    rows, extra = run()
    for pattern in (0xFF, 0x7F):
        plain.debug_poison(pattern)
        rows2, extra2 = run()
        assert rows2 == rows and np.array_equal(extra2["overlays"], extra["overlays"]), pattern
        assert all(same_bits(a, b) for t in range(2) for a, b in zip(extra2["bars"][t], extra["bars"][t])), pattern
