"""GPU parity of the batch form of the Z-stack (Sato) branch (tmat_vessel_field_batch, tmat_analyze_stack_batch; reference
scripts/compute_branches.py:224-306, 366-395, 391-426): several stacks through one launch set per pass, the host graph stage of a pass
beside the device stages of the next.  Every stack of a batch must come out exactly as it does alone: float stages bit for bit, masks,
rows and pictures equal, whatever the pass size.  The oracle (oracle/sato.py) runs on the CPU inside the tests, on small shapes."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]

FLOAT_STAGES = ("vess", "sharp", "vessels")
MASK_STAGES = ("edges", "skel", "mask_sel", "grown", "closed", "filt")
CFG = {"graph_thresh_1": 5, "graph_thresh_2": 10, "graph_smoothing_window": 12, "min_branch_length": 12, "remove_isolated_branches": False}


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def px_params():
    from tmat_amd import branches
    return branches.graph_px_params(CFG, 384, 1000.0)


def _synth_vol(Z, h, w, seed):
    from oracle import sato as osato
    from tmat_amd import synth
    return osato.stack_prepare(synth.synth_stack(seed, Z, h * 2, w * 2, n_vessels=10), (h, w))


@pytest.fixture(scope="module")
def three_vols():
    return np.stack([_synth_vol(6, 120, 160, seed) for seed in (3, 4, 5)])


def assert_stages_equal(st, i, ost, what=""):
    for k in FLOAT_STAGES:
        assert same_bits(st[k][i], ost[k]), (what, i, k)
    for k in MASK_STAGES:
        assert np.array_equal(st[k][i], ost[k]), (what, i, k)


@pytest.mark.parametrize("hessian", ["gradient", "gaussian_derivatives"])
def test_every_stage_of_every_stack_equals_the_oracle(plain, three_vols, hessian):
    from oracle import sato as osato
    from tmat_amd import sato
    fields, st = sato.vessel_field_batch(plain, three_vols, hessian, return_stages=True)
    for i, vol in enumerate(three_vols):
        ofield, ost = osato.vessel_field(vol, return_stages=True, hessian=hessian)
        assert ost["edges"].sum() > 100 and ost["filt"].sum() > 100           # the case exercises every stage
        assert_stages_equal(st, i, ost, hessian)
        assert same_bits(fields[i], ofield), i


def _border_vol(seed, where, Z=4, h=96, w=128):
    """a prepared volume with three bright vertical vessels that run into its last (or first) rows"""
    vol = _synth_vol(Z, h, w, seed).copy()
    xx = np.mgrid[0:h, 0:w][1]
    rows = slice(h - 36, h) if where == "last" else slice(0, 36)
    for x0 in (30, 64, 100):
        line = (0.9 * np.exp(-0.5 * ((xx - x0) / 1.5) ** 2)).astype(np.float32)
        vol[:, rows] = np.maximum(vol[:, rows], line[rows])
    return vol


def test_nothing_leaks_between_neighbours_of_a_batch(plain):
    """[structure in its last rows, blank, structure in its first rows]: per-batch extrema, labels that merge across images and
    neighbourhoods that read the next image would each change a stage of one of the three.

    The border rows: skimage's canny never marks row 0 or row h - 1 (its non-maximum suppression works on the image eroded by one pixel,
    feature/_canny.py; oracle/sato.py:canny_from_smoothed restates it), so `edges` cannot have pixels there for any input.  The inputs
    are built so that the oracle's `edges` reach the outermost rows canny can mark, h - 2 and 1, and so that the masks of the stages that
    read a neighbourhood (`grown`, `closed`, `filt`) are set in rows h - 1 and 0 themselves -- the rows that touch the neighbour image."""
    from oracle import sato as osato
    from tmat_amd import sato
    a, c = _border_vol(31, "last"), _border_vol(32, "first")
    vols = np.stack([a, np.zeros_like(a), c])
    oa, oc = osato.vessel_field(a, return_stages=True), osato.vessel_field(c, return_stages=True)
    assert oa[1]["edges"][-2].any() and oc[1]["edges"][1].any()
    for k in ("grown", "closed", "filt"):
        assert oa[1][k][-1].any() and oc[1][k][0].any(), k
    fields, st = sato.vessel_field_batch(plain, vols, return_stages=True)
    for i, (ofield, ost) in ((0, oa), (2, oc)):
        assert_stages_equal(st, i, ost)
        assert same_bits(fields[i], ofield)
        single, sst = sato.vessel_field(plain, vols[i], return_stages=True)
        assert same_bits(fields[i], single)
        for k in FLOAT_STAGES + MASK_STAGES:
            assert np.array_equal(st[k][i], sst[k]), k
    assert not fields[1].any() and not any(st[k][1].any() for k in MASK_STAGES)


def test_two_slices_and_odd_geometry(plain):
    """n = 2, Z = 2 (one slice pair per stack), a 75 x 101 field: no side is a multiple of a tile"""
    from oracle import sato as osato
    from tmat_amd import sato, synth
    vols = np.stack([osato.stack_prepare(synth.synth_stack(seed, 2, 150, 202, n_vessels=6), (75, 101)) for seed in (21, 22)])
    fields, st = sato.vessel_field_batch(plain, vols, return_stages=True)
    for i, vol in enumerate(vols):
        ofield, ost = osato.vessel_field(vol, return_stages=True)
        assert same_bits(st["sharp"][i], ost["sharp"]) and np.array_equal(st["edges"][i], ost["edges"]) and np.array_equal(st["filt"][i], ost["filt"])
        assert same_bits(fields[i], ofield)
    one, st1 = sato.vessel_field_batch(plain, vols[:1], return_stages=True)
    single, sst = sato.vessel_field(plain, vols[0], return_stages=True)
    assert same_bits(one[0], single)
    for k in FLOAT_STAGES + MASK_STAGES:
        assert np.array_equal(st1[k][0], sst[k]), k


def test_rows_and_fields_equal_the_per_stack_entry_and_the_oracle(plain):
    from oracle import sato as osato
    from tmat_amd import sato, synth
    stacks = np.stack([synth.synth_stack(seed, 5, 300, 400, n_vessels=12) for seed in (7, 8, 9)])
    sw, mn, mx = px_params()
    pairs = [(5, 10), (2, 4)]
    rows, fields = sato.analyze_stack_batch(plain, stacks, pairs, sw, mn, mx, False, ds_width=384, return_fields=True)
    assert fields.shape == (3, 288, 384)
    for t, (t1, t2) in enumerate(pairs):
        for i in range(3):
            n, tot, avg, field = sato.analyze_stack(plain, stacks[i], t1, t2, sw, mn, mx, False, return_field=True)
            assert rows[t][i] == (n, tot, avg), (t, i)
            assert same_bits(fields[i], field)
            assert n > 0
    assert rows[0][0] == tuple(osato.analyze_stack(stacks[0], CFG, 1000.0))


def _five_stacks():
    from tmat_amd import synth
    return np.stack([synth.synth_stack(40 + i, 3, 128, 160, n_vessels=6) for i in range(5)])


CHILD = """
import json, sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
from tmat_amd import _lib, sato
from test_gpu_stack_batch import _five_stacks, px_params
h = _lib.Handle(None, 0)
sw, mn, mx = px_params()
rows = sato.analyze_stack_batch(h, _five_stacks(), [(5, 10), (2, 4)], sw, mn, mx, False, pass_stacks=2)
h.close()
print("ROWS " + json.dumps(rows))
"""


def test_pass_size_and_host_threads_do_not_change_a_bit(plain):
    """5 stacks in passes of 1, 2 (a short last pass, both result slots reused) and 5; then passes of 2 with one host worker thread, in a
    fresh child process (the thread count is read from the environment)"""
    from tmat_amd import sato
    stacks = _five_stacks()
    sw, mn, mx = px_params()
    pairs = [(5, 10), (2, 4)]
    want_rows = [[None] * 5 for _ in pairs]
    want_fields = []
    for i in range(5):
        for t, (t1, t2) in enumerate(pairs):
            n, tot, avg, field = sato.analyze_stack(plain, stacks[i], t1, t2, sw, mn, mx, False, return_field=True)
            want_rows[t][i] = (n, tot, avg)
        want_fields.append(field)
    for k in (1, 2, 5):
        rows, fields = sato.analyze_stack_batch(plain, stacks, pairs, sw, mn, mx, False, return_fields=True, pass_stacks=k)
        assert rows == want_rows, k
        assert all(same_bits(fields[i], want_fields[i]) for i in range(5)), k
    code = CHILD.format(repo=str(REPO), pkg=str(REPO / "tissue-model-analysis-tools_amd"), tests=str(REPO / "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, TMAT_HOST_THREADS="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1]
    assert [[tuple(x) for x in row] for row in json.loads(line[5:])] == want_rows


def _well_stack(seed, Z=4, h=300, w=400):
    """a synthetic stack whose vessels sit inside a round well that is brighter than its surroundings"""
    from tmat_amd import synth
    st = synth.synth_stack(seed, Z, h, w, n_vessels=14).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (xx - w * 0.5) ** 2 / (w * 0.42) ** 2 + (yy - h * 0.52) ** 2 / (h * 0.42) ** 2 < 1
    out = np.where(inside, st * 0.6 + 14000.0, st * 0.05 + 900.0)
    return np.clip(out, 0, 65535).astype(np.uint16)


def test_pruning_masks_prune_each_stack_with_its_own_mask(plain):
    from tmat_amd import sato
    stacks = np.stack([_well_stack(11), _well_stack(12)])
    sw, mn, mx = px_params()
    out_hw = sato.dsamp_shape(stacks.shape, 384)
    pruning = np.stack([sato.stack_well_masks(plain, st, out_hw, seed=3)[1] for st in stacks])
    rows, fields = sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False, pruning_masks=pruning, return_fields=True)
    unpruned = sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False)
    for i in range(2):
        field = sato.stack_field(plain, stacks[i])
        assert same_bits(fields[i], field)
        assert rows[0][i] == sato.field_stats(plain, field, 5, 10, sw, mn, mx, False, pruning_mask=pruning[i]), i
        assert unpruned[0][i] == sato.field_stats(plain, field, 5, 10, sw, mn, mx, False), i
    assert rows[0][0] != unpruned[0][0], "the pruning mask should remove something from the seed-11 stack"


def test_pictures_are_the_bytes_of_stage_pictures(plain):
    from tmat_amd import sato, synth
    stacks = np.stack([synth.synth_stack(50 + i, 3, 128, 160, n_vessels=6) for i in range(2)])
    sw, mn, mx = px_params()
    rows, fields, (proj, fpic) = sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False, return_fields=True, return_pictures=True)
    assert proj.shape == (2, 128, 160) and fpic.shape == fields.shape and fpic.dtype == np.uint8
    for i in range(2):
        assert np.array_equal(proj[i], plain.stage_pictures(stacks[i].max(0)))
        assert np.array_equal(fpic[i], plain.stage_pictures(fields[i]))
        assert proj[i].max() == 255 and fpic[i].max() == 255
    assert rows == sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False)


def test_recycled_blocks_hold_nothing_a_batch_reads_before_writing(plain):
    """the pooled device blocks and the pinned result slots filled with 0xFF / 0x7F between batch calls of two geometries: the rows are
    those of a fresh handle"""
    from tmat_amd import _lib, sato, synth
    sw, mn, mx = px_params()
    a = np.stack([synth.synth_stack(60 + i, 3, 128, 160, n_vessels=6) for i in range(3)])
    b = np.stack([synth.synth_stack(70 + i, 4, 150, 140, n_vessels=6) for i in range(2)])
    pairs = [(5, 10), (2, 4)]
    fresh = _lib.Handle(None, 0)
    try:
        want = [sato.analyze_stack_batch(fresh, s, pairs, sw, mn, mx, False, pass_stacks=2) for s in (a, b)]
    finally:
        fresh.close()
    assert all(r[0] > 0 for r in want[0][0])
    for pattern in (0xFF, 0x7F):
        for s, w in ((a, want[0]), (b, want[1]), (a, want[0])):
            plain.debug_poison(pattern)
            assert sato.analyze_stack_batch(plain, s, pairs, sw, mn, mx, False, pass_stacks=2) == w


def test_bad_arguments_are_refused_and_leave_the_handle_usable(plain):
    import ctypes as C
    from tmat_amd import _lib, sato
    stacks = _five_stacks()[:2]
    sw, mn, mx = px_params()
    want = sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False)
    L = _lib.lib()
    th = np.array([5, 10], np.float32)
    rows = (_lib.Row * 2)()

    def call(n=2, Z=3, n_thresh=1, thresh=th.ctypes.data, size=C.sizeof(_lib.StackOpts), hessian=0):
        o = _lib.StackOpts()
        o.size, o.ds_width, o.hessian, o.n_thresh, o.thresh = size, 384, hessian, n_thresh, thresh
        o.smoothing_window_px, o.min_branch_length_px = sw, mn
        return L.tmat_analyze_stack_batch(plain.raw, _lib.ptr(stacks), n, Z, 128, 160, C.byref(o), rows)

    assert call() == 0
    for bad in (dict(n=0), dict(Z=1), dict(n_thresh=0), dict(thresh=None), dict(size=C.sizeof(_lib.StackOpts) - 4), dict(hessian=7)):
        assert call(**bad) == _lib.E_ARG, bad
        assert L.tmat_last_error(), bad
    vols = np.zeros((2, 3, 16, 16), np.float32)
    out = np.zeros((2, 16, 16), np.float32)
    assert L.tmat_vessel_field_batch(plain.raw, _lib.ptr(vols), 0, 3, 16, 16, 0, _lib.ptr(out), None) == _lib.E_ARG
    assert L.tmat_vessel_field_batch(plain.raw, _lib.ptr(vols), 2, 1, 16, 16, 0, _lib.ptr(out), None) == _lib.E_ARG
    assert L.tmat_vessel_field_batch(plain.raw, _lib.ptr(vols), 2, 3, 16, 16, 7, _lib.ptr(out), None) == _lib.E_ARG
    assert sato.analyze_stack_batch(plain, stacks, [(5, 10)], sw, mn, mx, False) == want
