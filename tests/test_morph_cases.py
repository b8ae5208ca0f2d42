"""CPU: the inputs and references of tests/helpers/morph_cases.py have the properties tests/test_gpu_morph_stages.py relies on, so
that none of its comparisons is vacuous: the per-root statistics are skimage's, the component counts are what the names promise,
and the wake-up inputs really put tiles of the Zhang kernel to sleep and wake them within the kernel's launch budget."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import morph_cases as mc  # noqa: E402
from oracle import morph  # noqa: E402

G = np.load(Path(__file__).parent / "golden" / "filter.npz")
SQ2 = math.sqrt(2.0)


def unpack(name, key):
    shape = tuple(G[name + "_shape"])
    return np.unpackbits(G[name + "_" + key])[: shape[0] * shape[1]].reshape(shape).astype(bool)


@pytest.mark.parametrize("name", ["blobs", "noise", "small"])
def test_ref_stats_are_the_oracles_area_and_perimeter(name):
    """every region of the golden masks: area and perimeter4 region by region (as filter_branch_seg_mask does) == ref_stats at the
    region's root, and nothing anywhere else"""
    m = unpack(name, "mask")
    labels, stats = mc.ref_labels(m), mc.ref_stats(m)
    lab, n = ndi.label(m, mc.EIGHT)
    assert n > 3
    seen = np.zeros(m.shape, bool)
    for i, sl in enumerate(ndi.find_objects(lab), start=1):
        reg = lab[sl] == i
        ys, xs = np.nonzero(lab == i)
        root = (ys[0], xs[0])                                     # first pixel in raster order = smallest flat index
        assert (labels[lab == i] == root[0] * m.shape[1] + root[1]).all()
        area, n1, n2, n3 = (int(v) for v in stats[(slice(None),) + root])
        assert area == int(reg.sum())
        assert float(n1) + n2 * SQ2 + n3 * ((1 + SQ2) / 2) == morph.perimeter4(reg), (i, n1, n2, n3)
        seen[root] = True
    assert not stats[:, ~seen].any()
    assert (labels[~m] == -1).all()


def n_components(m):
    return ndi.label(m, mc.EIGHT)[1]


@pytest.mark.parametrize("shape", [s for s in mc.SHAPES if min(s) >= 2 and max(s) >= 4])
def test_inputs_have_the_components_their_names_promise(shape):
    H, W = shape
    c = dict(mc.cases(H, W))
    assert n_components(c["spiral"]) == 1 and ndi.label(c["spiral"])[1] == 1          # one 4-connected path
    assert n_components(c["serpentine"]) == 1 and n_components(c["comb"]) == 1
    assert n_components(c["checker"]) == 1 and ndi.label(c["checker"])[1] == c["checker"].sum()       # diagonal unions alone
    assert n_components(c["lattice"]) == ((H + 1) // 2) * ((W + 1) // 2) == c["lattice"].sum()
    assert n_components(c["discs_gap"]) == 2
    assert n_components(c["discs_diag"]) == 1 and ndi.label(c["discs_diag"])[1] == 2  # touching through one diagonal only
    assert c["full"].all() and not c["empty"].any()


def test_lattice_of_an_even_frame_has_a_quarter_of_the_pixels():
    assert n_components(mc.lattice(40, 64)) == 40 * 64 // 4


def test_spiral_arms_are_one_pixel_wide_with_background_between():
    m = mc.spiral(37, 127)
    assert not (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).any()             # no 2 x 2 block
    deg = ndi.correlate(m.astype(int), np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]]), mode="constant")[m]
    assert deg.max() == 2 and (deg == 1).sum() == 2                                   # a path: two ends, no branch
    assert m.sum() > 37 * 127 // 3


@pytest.mark.parametrize("shape", [(5, 63), (5, 64), (5, 65), (37, 127), (513, 513)])
def test_runs_cross_every_chunk_boundary(shape):
    f = mc.runs64(*shape).ravel()
    ks = np.arange(64, f.size, 64)
    assert len(ks) and f[ks].all() and f[ks - 1].all()
    assert not f.all()


@pytest.mark.parametrize("name", [n for n, _ in mc.wake_cases()])
def test_wake_inputs_sleep_and_wake_within_the_launch_budget(name):
    """recomputed from launch_trace: the removing launches fit filter_mask_dev's budget, at least one tile removes something after
    it has slept, and a sleeping tile never has anything to remove in the launch it sleeps through (the kernel's premise)"""
    m = dict(mc.wake_cases())[name]
    trace, sk = mc.launch_trace(m, True)
    woken = mc.woken_tiles(trace)
    print(f"{name}: {len(trace)} launches (budget {mc.launch_budget(*m.shape)} removing), {int(woken.sum())} slept-then-woken tiles")
    assert len(trace) - 1 <= mc.launch_budget(*m.shape)
    assert woken.sum() >= 1
    for j in range(1, len(trace)):
        assert not (trace[j] & ~ndi.binary_dilation(trace[j - 1], mc.EIGHT)).any(), j
    assert not trace[-1].any() and all(t.any() for t in trace[:-1])
    assert np.array_equal(sk, morph.skeletonize_zhang(m))


def test_launch_trace_ends_in_the_oracles_skeleton():
    """launch_trace restates skeletonize_zhang's loop; on every kind of input its fixed point is skeletonize_zhang's"""
    for name, m in mc.solid_cases()[5:] + mc.cases(37, 127) + mc.cases(5, 64) + mc.cases(1, 70) + mc.cases(70, 1) + mc.cases(2, 2):
        trace, sk = mc.launch_trace(m, True)
        assert np.array_equal(sk, morph.skeletonize_zhang(m)), name
        assert len(trace) - 1 <= mc.launch_budget(*m.shape), name


def test_solid_inputs_that_never_wake_a_tile():
    for name in ("disc110", "triangle240", "full16x200", "full200x16", "stair240_slash"):
        assert not mc.woken_tiles(mc.launch_trace(dict(mc.solid_cases())[name])).any(), name
