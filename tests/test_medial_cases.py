"""CPU: the reference model and the inputs of tests/helpers/medial_cases.py have the properties tests/test_gpu_medial_stages.py
relies on, so that none of its comparisons is vacuous: the model's keys sort like oracle.morph.medial_axis's lexsort, its level-by-level
evaluation ends in the oracle's skeleton, the wake inputs really put tiles of ma_round_kernel to sleep and wake them, and the large
frame really sends the chunk scan round its slab loop twice."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import medial_cases as md  # noqa: E402
import morph_cases as mc  # noqa: E402
from oracle import morph  # noqa: E402

# (levels, launches, woken tiles, tiles) of the wake inputs: recomputed below, written down here so that a change shows
WAKE = {"full320": (1276, 80, 21, 25), "full250x245": (986, 64, 12, 16), "framed386": (670, 44, 4, 49), "disc220": (721, 48, 5, 64),
        "triangle450": (1423, 92, 10, 64)}


def oracle_order(mask):
    """the visiting order of oracle.morph.medial_axis (its lines, not its result): indices into the raster-ordered foreground pixels"""
    m = np.asarray(mask, bool)
    dist = ndi.distance_transform_edt(m)
    code = ndi.correlate(m.astype(np.int32), np.array([[1, 2, 4], [8, 16, 32], [64, 128, 256]]), mode="constant", cval=0)
    corner = np.array([9 - bin(i).count("1") for i in range(512)])[code]
    tiebreak = np.random.RandomState(0).permutation(np.arange(int(m.sum())))
    return np.lexsort((tiebreak, corner[m], dist[m]))


def check_model(name, mask):
    r = md.model(name, mask)
    m, keys, dep, level = r["mask"], r["keys"], r["dep"], r["level"]
    assert (keys[~m] == md.BACKGROUND_KEY).all() and not dep[~m].any() and not level[~m].any(), name
    k = keys[m]
    assert len(np.unique(k)) == k.size, name                                       # distinct: sorting them is a total order
    assert np.array_equal(np.argsort(k), oracle_order(m)), name
    # the level is 1 + the largest level of the predecessors, recomputed here from the bytes; neighbours never share a level
    P = np.pad(level, 1)
    H, W = m.shape
    best = np.zeros((H, W), np.int32)
    for b, (dy, dx) in enumerate(md.NEIGHBOURS):
        nb = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        best = np.maximum(best, np.where((dep >> b) & 1 == 1, nb, 0))
        assert not (m & (nb == level)).any(), name
    assert np.array_equal(level[m], best[m] + 1), name
    assert np.array_equal(md.skeleton_by_levels(m, level), r["skel"]), name
    assert np.array_equal(r["skel"], morph.medial_axis(m)[0]), name
    return r


def test_constants_are_the_kernels():
    src = (Path(__file__).resolve().parents[1] / "tissue-model-analysis-tools_amd" / "csrc" / "thin_kernels.hip").read_text()
    for name, value in (("MA_T", md.MA_T), ("MA_R", md.MA_R), ("GROUP", md.MA_GROUP)):
        found = re.findall(rf"\b{name}\s*=\s*(\d+)\s*[,;]", src)
        assert found == [str(value)], f"thin_kernels.hip defines {name} as {found}, tests/helpers/medial_cases.py has {value}"


@pytest.mark.parametrize("shape", md.SMALL_SHAPES, ids=[f"{h}x{w}" for h, w in md.SMALL_SHAPES])
def test_model_is_the_oracle_at_small_and_odd_frames(shape):
    assert len(md.SMALL_SHAPES) == 10 and (513, 513) not in md.SMALL_SHAPES
    cases = mc.cases(*shape)
    assert len(cases) == 17
    depths = [check_model((shape, name), m)["depth"] for name, m in cases]
    print(f"{shape}: depths {depths}")
    assert max(depths) <= 662


@pytest.mark.parametrize("name", list(WAKE))
def test_wake_inputs_put_tiles_to_sleep_and_wake_them(name):
    """a condition on the inputs, not a measurement of the kernel: depth, launch count and the tiles that sleep and have to wake, all
    from the model; woken_tiles also asserts that a tile asleep in a launch finishes no pixel of its own in it (the kernel's premise)"""
    m = dict(md.wake_cases())[name]
    r = check_model(name, m)
    woken = md.woken_tiles(r["level"])
    got = (r["depth"], md.expected_launches(r["depth"]), int(woken.sum()), woken.size)
    print(f"{name}: {got[0]} levels, {got[1]} launches, {got[2]} of {got[3]} tiles sleep and wake")
    assert woken.sum() >= 4
    assert got == WAKE[name]
    H, W = m.shape
    assert got[1] <= 64 * ((H + W) // md.MA_R + 8)                                 # far inside thin_dev's launch budget
    if m.all():
        assert (r["dist"] > 0).all()                                               # no background: the EDT's branch of its own


def test_sleep_model_on_a_hand_made_trace():
    """tile_trace, asleep_tiles and woken_tiles on level maps written by hand.  First two tiles side by side: the right tile has
    nothing of its own until launch 2, but its left neighbour has progress in every launch, so it never sleeps."""
    level = np.zeros((64, 128), np.int32)
    level[0, :40] = np.arange(1, 41)                  # launches 0, 1, 2 in the left tile; x = 16 ... 31 is level 17 ... 32: launch 1
    level[0, 100] = 41                                # launch 2, right tile (its staged area starts at x = 49)
    progress, own = md.tile_trace(level)
    assert progress.shape == (3, 1, 2)
    assert progress[:, 0, 0].tolist() == [True, True, True] and progress[:, 0, 1].tolist() == [False, False, True]
    assert own[:, 0, 1].tolist() == [False, False, True]
    asleep = md.asleep_tiles(progress)
    assert asleep[:, 0, 1].tolist() == [False, False, False]        # the left neighbour always had progress: never asleep
    level[0, :40] = 0
    level[0, 0:16] = np.arange(1, 17)
    level[0, 100] = 33
    with pytest.raises(AssertionError):               # a tile that finishes a pixel while the model has it asleep: the claim is checked
        md.woken_tiles(level)
    # a chain along row 0 to the right end of four tiles and back along row 2: the right tiles sleep until it arrives, the left
    # tiles while it is far away (launch 15 follows progress at x = 224 ... 239, inside the staged area of the last tile alone)
    level = np.zeros((64, 256), np.int32)
    level[0] = np.arange(1, 257)
    level[1, 255] = 257
    level[2] = np.arange(513, 257, -1)
    progress, own = md.tile_trace(level)
    assert progress[14].tolist() == [[False, False, False, True]]
    assert md.asleep_tiles(progress)[[1, 15]].tolist() == [[[False, False, True, True]], [[True, True, False, False]]]
    assert md.woken_tiles(level).all()
    level[2] = 0                                      # without the way back the left tiles have nothing to wake for
    assert md.woken_tiles(level).tolist() == [[False, False, True, True]]
    # the staged area minus its rim reaches MA_R - 1 pixels into the neighbour
    for x, seen in ((63 + md.MA_R - 1, True), (63 + md.MA_R, False)):
        lv = np.zeros((64, 128), np.int32)
        lv[5, x] = 1
        assert md.tile_trace(lv)[0][0, 0].tolist() == [seen, True]


def test_expected_launches():
    assert [md.expected_launches(d) for d in (0, 1, 64, 65, 128, 129, 1276, 1423)] == [4, 4, 4, 8, 8, 12, 80, 92]


def test_frame_beyond_1024_chunks():
    H, W = md.CHUNKS_SHAPE
    assert -(-H * W // 1024) == 1027 and (H * W) % 1024
    (_, m), (_, f) = md.chunks_batch()
    assert np.array_equal(f, m[::-1]) and m.sum() == 113473
    r = check_model("chunks", m)
    assert r["depth"] == 39
    assert check_model("chunks_flipped", f)["depth"] <= 64
    # ranks from the scan's second slab decide ties: neighbours with equal (distance, corner score) among the pixels beyond chunk 1024
    flat = np.arange(H * W).reshape(H, W)
    hi = r["keys"] >> np.uint64(32)
    ties = 0
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(dy, H), slice(max(0, dx), W + min(0, dx)))
        ties += int((m[a] & m[b] & (hi[a] == hi[b]) & (flat[a] >= 1024 * 1024)).sum())
    print(f"chunks: {ties} neighbour pairs beyond chunk 1024 ordered by the tie-break alone")
    assert ties >= 100


def test_mixed_batch_has_depths_on_both_sides_of_a_launch_group():
    depths = {name: check_model(("mixed", name), m)["depth"] for name, m in md.mixed_batch()}
    print(depths)
    assert depths["empty"] == 0 and depths["full"] == 1276
    assert depths["noise45"] <= md.MA_R < depths["blobs"] <= 3 * md.MA_R          # done after 1 and after 2 to 3 launches
    assert md.expected_launches(depths["framed"]) < md.expected_launches(depths["full"]) - 40
